"""Records tests/golden/golden_seginput.npz by running the REFERENCE's own downstream/semseg/lib/voxelizer.py and
lib/transforms.py on small seeded inputs:  python tests/golden/make_golden_seginput.py <reference root>

MinkowskiEngine is not installed where this runs, so `ME.utils.sparse_quantize(coords, feats, labels, ignore_label)` -- the
only thing voxelizer.py needs from it -- is stubbed below.  Its label rule is RECALLED from MinkowskiEngine 0.4.3 (the
source is not available here): one row per distinct coordinate; the voxel keeps the common label of its rows and gets
ignore_label as soon as two of them differ.  Everything else that is recorded comes out of the reference's code.

The random draws are recorded next to the outputs (they are inputs of our kernels): the voxelizer's matrix is recovered from
the transformation it returns (M_r M_v has no translation, so the returned translation column is -min), the translation ratio
by wrapping Voxelizer.clip, the colour draws by re-seeding, the elastic noise volume by wrapping np.random.randn.  The jitter's normals are rounded to float32 before the reference
uses them, because pcmi_seg_color_augment takes float32 normals."""
import collections
import collections.abc
import importlib.util
import os
import random
import sys
import types

import numpy as np

collections.Iterable = collections.abc.Iterable  # voxelizer.py:58 predates Python 3.10


def sparse_quantize(coords, feats=None, labels=None, ignore_label=255):
  seen, rows, out = {}, [], []
  for i, c in enumerate(np.floor(coords).astype(np.int64)):
    k = tuple(c)
    if k not in seen:
      seen[k] = len(rows)
      rows.append(i)
      out.append(int(labels[i]))
    elif out[seen[k]] != int(labels[i]):
      out[seen[k]] = ignore_label
  rows = np.asarray(rows)
  return np.floor(coords[rows]).astype(np.int32), feats[rows], np.asarray(out, dtype=np.int32)


def load(root, name):
  me = types.ModuleType("MinkowskiEngine")
  me.utils = types.SimpleNamespace(sparse_quantize=sparse_quantize)
  sys.modules["MinkowskiEngine"] = me
  spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(root, "downstream", "semseg", "lib", name + ".py"))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def main(root):
  vz, tf = load(root, "voxelizer"), load(root, "transforms")
  out = {}
  # ---- Voxelizer.voxelize: (clip bound, augmentation) per case -------------------------------------------------------------
  cases = [(None, False), (None, True), (1.5, True), (((-1.0, 1.2), (-0.8, 0.9), (-5.0, 5.0)), True), (50.0, True)]
  rot = ((-np.pi / 64, np.pi / 64), (-np.pi / 64, np.pi / 64), (-np.pi, np.pi))
  for k, (clip, augment) in enumerate(cases):
    rng = np.random.RandomState(100 + k)
    n = 400 + 37 * k
    xyz = rng.uniform(-2, 2, size=(n, 3))
    xyz[n // 2:] = xyz[:n - n // 2] + rng.uniform(-0.01, 0.01, size=(n - n // 2, 3))  # neighbours that share voxels
    feats = rng.randint(0, 256, size=(n, 3)).astype(np.float64)
    labels = rng.randint(0, 3, size=n).astype(np.int32)
    v = vz.Voxelizer(voxel_size=0.05, clip_bound=clip, use_augmentation=augment, scale_augmentation_bound=(0.9, 1.1),
                     rotation_augmentation_bound=rot, translation_augmentation_ratio_bound=((-0.2, 0.2), (-0.2, 0.2), (0, 0)),
                     ignore_label=255)
    seen_ratio = []
    inner = v.clip
    v.clip = lambda c, center=None, r=None: (seen_ratio.append(np.array(r)), inner(c, center, r))[1]
    np.random.seed(200 + k)
    c, f, l, T = v.voxelize(xyz.copy(), feats.copy(), labels.copy())
    T = T.reshape(4, 4)
    M = T.copy()
    M[:3, 3] = 0.0
    h = np.hstack([xyz, np.ones((n, 1))]) @ M.T[:, :3]
    assert np.abs(h - np.rint(h)).min() > 1e-9, "case %d: a transformed coordinate lies within 1e-9 of an integer" % k
    out.update({"vox%d_xyz" % k: xyz, "vox%d_feats" % k: feats, "vox%d_labels" % k: labels, "vox%d_M" % k: M, "vox%d_T" % k: T,
                "vox%d_ratio" % k: seen_ratio[0] if seen_ratio else np.zeros(3), "vox%d_coords" % k: c.astype(np.int32),
                "vox%d_out_labels" % k: l.astype(np.int32), "vox%d_out_feats" % k: f,
                "vox%d_clip" % k: np.zeros(0) if clip is None else np.asarray(clip, dtype=np.float64).reshape(-1)})
  out["vox_cases"] = np.int64(len(cases))
  # ---- flip and the three chromatic transforms, each forced on ----------------------------------------------------------------
  real_randn = np.random.randn
  np.random.randn = lambda *s: real_randn(*s).astype(np.float32).astype(np.float64)
  for k in range(3):
    rng = np.random.RandomState(300 + k)
    m = 150 + 50 * k
    coords = rng.randint(0, 30, size=(m, 3)).astype(np.float64)
    feats = rng.randint(5, 250, size=(m, 3)).astype(np.float64)
    labels = rng.randint(0, 3, size=m)
    chain = [tf.RandomHorizontalFlip("z", False), tf.ChromaticAutoContrast(), tf.ChromaticTranslation(0.1), tf.ChromaticJitter(0.05)]
    real_random = random.random
    # python's random.random() decides which transforms apply; 0.1 says yes to all four (and flips both horizontal axes);
    # the blend factor -- the only draw of it that is a VALUE -- is the fifth call
    seq = iter([0.1, 0.1, 0.1, 0.1, 0.23 + 0.3 * k, 0.1, 0.1])
    random.random = lambda: next(seq)
    np.random.seed(400 + k)
    c, f, l = coords.copy(), feats.copy(), labels.copy()
    for t in chain:
      c, f, l = t(c, f, l)
    random.random = real_random
    np.random.seed(400 + k)
    tr = (np.random.rand(1, 3) - 0.5) * 255 * 2 * 0.1
    normals = np.random.randn(m, 3)
    out.update({"col%d_coords" % k: coords.astype(np.int32), "col%d_feats" % k: feats, "col%d_blend" % k: np.float64(0.23 + 0.3 * k),
                "col%d_tr" % k: tr.reshape(3), "col%d_normals" % k: normals.astype(np.float32), "col%d_out_coords" % k: c.astype(np.int32),
                "col%d_out_feats" % k: f})
  np.random.randn = real_randn
  out["col_cases"] = np.int64(3)
  # ---- ElasticDistortion.elastic_distortion, one stage per case (the two stages of ELASTIC_DISTORT_PARAMS and a finer one) -------
  real_randn = np.random.randn
  for k, (g, mag, n) in enumerate([(0.2, 0.4, 300), (0.8, 1.6, 300), (0.1, 0.2, 150)]):
    rng = np.random.RandomState(500 + k)
    xyz = rng.uniform(-1.0, 1.3, size=(n, 3)) * [1.0, 0.7, 0.4]
    drawn = []
    np.random.randn = lambda *s: (drawn.append(real_randn(*s)), drawn[-1])[1]
    np.random.seed(600 + k)
    c, _, _ = tf.ElasticDistortion(((g, mag),)).elastic_distortion(xyz.copy(), None, None, g, mag)
    np.random.randn = real_randn
    out.update({"el%d_xyz" % k: xyz, "el%d_gm" % k: np.array([g, mag]), "el%d_noise" % k: drawn[0].astype(np.float32), "el%d_out" % k: c})
  out["el_cases"] = np.int64(3)
  np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden_seginput.npz"), **out)


if __name__ == "__main__":
  main(sys.argv[1])
