"""tests/semseg_input_ref.py (the restatement that the GPU tests compare the kernels with) held to what the reference's own
Voxelizer.voxelize and transforms produced on seeded inputs: tests/golden/golden_seginput.npz, recorded by
tests/golden/make_golden_seginput.py (which stubs ME.utils.sparse_quantize; its label rule is recalled from MinkowskiEngine
0.4.3, whose source was not at hand)."""
import os

import numpy as np
import pytest

import semseg_input_ref as sr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_seginput.npz")


@pytest.fixture(scope="module")
def G():
  return np.load(GOLDEN)


def _clip(a):
  return None if a.size == 0 else (float(a[0]) if a.size == 1 else a.reshape(3, 2).tolist())


def test_voxelizer_cases_integer_outputs_equal(G):
  assert int(G["vox_cases"]) == 5
  clipped = 0
  for k in range(int(G["vox_cases"])):
    xyz, labels, M, clip = G["vox%d_xyz" % k], G["vox%d_labels" % k], G["vox%d_M" % k], _clip(G["vox%d_clip" % k])
    n = len(xyz)
    # no transformed coordinate lies within 1e-9 of an integer: np.dot and the fixed order cannot disagree on a floor
    h = np.hstack([xyz, np.ones((n, 1))]) @ M.T[:, :3]
    assert np.abs(h - np.rint(h)).min() > 1e-9
    vox, keep, mn, aligned, f1 = sr.seg_transform(xyz, [0, n], [M], clip, [G["vox%d_ratio" % k]])
    coords, index, lab, counts, f2 = sr.seg_quantize(vox, [0, n], labels, keep, mn, 255)
    assert not f1.any() and not f2.any()
    clipped += int(keep.sum() < n)
    want_c, want_l = G["vox%d_coords" % k], G["vox%d_out_labels" % k]
    assert counts.tolist() == [len(want_c)] * 2, "case %d: %s voxels, the reference has %d" % (k, counts, len(want_c))
    ours = {tuple(c[1:]): int(l) for c, l in zip(coords, lab)}
    theirs = {tuple(c): int(l) for c, l in zip(want_c, want_l)}
    assert ours == theirs, "case %d: voxel set or labels differ" % k
    assert 255 in theirs.values() and len(theirs) < int(keep.sum()), "case %d exercises neither merging nor the label rule" % k
    # the aligned matrix: the reference's M_t @ M (equal values; +-0 aside)
    assert np.array_equal(aligned.reshape(4, 4), G["vox%d_T" % k]), "case %d: transformation differs" % k
    # the representative row carries the colour the reference kept for the voxel iff it is the voxel's first row too
    first = {tuple(c): f for c, f in zip(want_c, G["vox%d_out_feats" % k])}
    assert all(np.array_equal(first[tuple(c[1:])], G["vox%d_feats" % k][i]) for c, i in zip(coords, index))
  assert clipped == 2, "two of the cases clip points; the bound above the extent and the unclipped ones do not"


def test_order_of_first_occurrence_and_truncation():
  vox = [[5, 5, 5], [1, 1, 1], [5, 5, 5], [0, 0, 0], [1, 1, 1], [9, 9, 9]]
  coords, index, lab, counts, _ = sr.seg_quantize(vox, [0, 4, 4, 6], [1, 2, 3, 4, 2, 7])
  assert index.tolist() == [0, 1, 3, 4, 5] and coords[:, 0].tolist() == [0, 0, 0, 2, 2] and lab.tolist() == [255, 2, 4, 2, 7]
  assert counts.tolist() == [3, 0, 2, 5]
  assert sr.truncate([3, 0, 2], 0) == (3, 5) and sr.truncate([3, 0, 2], 4) == (2, 3) and sr.truncate([3, 0, 2], 2) == (0, 0)


def test_colour_chain_at_float64_round_off(G):
  for k in range(int(G["col_cases"])):
    coords = np.concatenate([np.zeros((len(G["col%d_coords" % k]), 1), np.int32), G["col%d_coords" % k]], 1)
    P = np.zeros((1, 12))
    P[0, :3] = [1, 1, 0]  # RandomHorizontalFlip("z"): both horizontal axes were drawn
    P[0, 3:5] = [1, G["col%d_blend" % k]]
    P[0, 5], P[0, 6:9] = 1, G["col%d_tr" % k]
    P[0, 9:11] = [1, 0.05 * 255]
    c, f, _ = sr.seg_color_augment(G["col%d_feats" % k].astype(np.float32), coords, 1, None, None, P, G["col%d_normals" % k])
    assert np.array_equal(c[:, 1:], G["col%d_out_coords" % k]), "case %d: flipped coordinates differ" % k
    want = G["col%d_out_feats" % k]
    err = np.abs(f - want).max() / 255.0
    assert np.all(np.abs(f - want) <= 1e-12 * np.maximum(np.abs(want), 1.0)), "case %d: colours differ by %g of the range" % (k, err)
    assert want.min() == 0.0 or want.max() == 255.0, "case %d reaches no clip" % k


def test_hi_equals_lo_is_left_alone_and_label_map():
  feats = np.array([[7, 10, 3], [7, 20, 9]], np.float32)
  P = np.zeros((1, 12))
  P[0, 3:5] = [1, 1.0]
  _, f, lab = sr.seg_color_augment(feats, [[0, 0, 0, 0], [0, 1, 0, 0]], 1, params=P, labels=[1, 5], label_lut=[9, 255, 3])
  assert f[:, 0].tolist() == [7.0, 7.0] and f[:, 1].tolist() == [0.0, 255.0] and lab.tolist() == [255, 255]


# the largest |ours - scipy| over the elastic fixtures below, measured with scipy 1.15.3 / numpy on x86-64: exactly 0 (the
# restatement's operation order is scipy's).  The assertion is four times that, as for every bound taken from a measurement.
ELASTIC_MEASURED_MAX_ABS_DIFF = 0.0


def _stage(xyz, g, mag, noise, pad=(0, 0, 0)):
  block = np.zeros((1,) + tuple(np.array(noise.shape[:3]) + pad) + (3,), np.float32)
  block[0, :noise.shape[0], :noise.shape[1], :noise.shape[2]] = noise
  out, blurred, dims, flags = sr.elastic_stage(xyz, [0, len(xyz)], g, mag, block)
  assert dims.tolist() == [list(noise.shape[:3]) + [1]] and not flags.any()
  return out, blurred[0, :noise.shape[0], :noise.shape[1], :noise.shape[2]]


def test_elastic_against_the_reference_and_scipy(G):
  scipy_ndimage, scipy_interpolate = pytest.importorskip("scipy.ndimage"), pytest.importorskip("scipy.interpolate")
  worst = 0.0
  assert int(G["el_cases"]) == 3
  for k in range(3):
    xyz, (g, mag), noise = G["el%d_xyz" % k], G["el%d_gm" % k], G["el%d_noise" % k]
    ours, blurred = _stage(xyz, g, mag, noise, pad=(k, 0, 2))
    # the reference's own output, recorded
    worst = max(worst, float(np.abs(ours - G["el%d_out" % k]).max()))
    # scipy here: convolve + RegularGridInterpolator as transforms.py:194-216 calls them
    v = noise
    for _ in range(2):
      for shape in ((3, 1, 1, 1), (1, 3, 1, 1), (1, 1, 3, 1)):
        v = scipy_ndimage.convolve(v, np.ones(shape).astype("float32") / 3, mode="constant", cval=0)
    mn, d = xyz.min(0), np.array(noise.shape[:3])
    assert np.array_equal(d, ((xyz - mn).max(0) // g).astype(int) + 3)
    ax = [np.linspace(a, b, n) for a, b, n in zip(mn - g, mn + g * (d - 2), d)]
    want = xyz + scipy_interpolate.RegularGridInterpolator(ax, v, bounds_error=0, fill_value=0)(xyz) * mag
    worst = max(worst, float(np.abs(blurred - v).max()), float(np.abs(ours - want).max()))
    assert np.abs(want - xyz).max() > 0.01 * mag, "case %d does not move the points" % k
  print("elastic: largest |ours - scipy| = %g" % worst)
  assert worst <= 4 * ELASTIC_MEASURED_MAX_ABS_DIFF


def test_elastic_grid_rules_and_dropout_rows():
  vol = np.arange(4 * 4 * 4 * 3, dtype=np.float32).reshape(4, 4, 4, 3)
  # nodes -0.25, 0, 0.25, 0.5: on the last node, on an inner node, on the first node, outside above and below
  p = np.array([[0.5, 0.5, 0.5], [0.25, 0.0, -0.25], [-0.25, -0.25, -0.25], [0.5000001, 0.0, 0.0], [0.0, -0.26, 0.0]])
  out = sr.elastic_apply_scene(p, vol, [0.0, 0.0, 0.0], [4, 4, 4], 0.25, 2.0)
  assert np.array_equal(out[0], p[0] + vol[3, 3, 3] * 2.0) and np.array_equal(out[1], p[1] + vol[2, 1, 0] * 2.0)
  assert np.array_equal(out[2], p[2] + vol[0, 0, 0] * 2.0) and np.array_equal(out[3:], p[3:])
  # a capacity one too small: flagged and unchanged; an inactive scene: unchanged, no flag
  xyz = np.random.RandomState(0).uniform(0, 1, size=(40, 3))
  out, _, dims, flags = sr.elastic_stage(xyz, [0, 20, 40], 0.5, 1.0, np.ones((2, 4, 4, 4, 3), np.float32), active=[1, 0])
  assert np.array_equal(out[20:], xyz[20:]) and flags.tolist() == [0, 0] and dims[:, 3].tolist() == [1, 0] and not np.array_equal(out[:20], xyz[:20])
  out, _, dims, flags = sr.elastic_stage(xyz, [0, 20, 40], 0.5, 1.0, np.ones((2, 3, 4, 4, 3), np.float32))
  assert np.array_equal(out, xyz) and flags.tolist() == [sr.FLAG_ELASTIC] * 2 and not dims.any()
  assert sr.dropout_rows([0.5, 0.1, 0.9, 0.1, 0.3]).tolist() == [0, 1, 3, 4] and sr.dropout_rows([0.2]).tolist() == []
