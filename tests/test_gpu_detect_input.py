"""The detection input kernels (csrc/detect_input.hip) and DetectionInputPipeline on the device, against the numpy restatement
tests/detect_input_ref.py BIT FOR BIT (fp32 and fp64 compared as integers), and the pipeline against the reference's own
outputs in tests/golden/golden_detinput.npz within the bounds that tests/test_detect_input_ref.py derives."""
import ctypes as C

import numpy as np
import pytest
import torch

import detect_input_ref as dr
import votenet_fixtures as VF
from c_contract import DEV, Guarded, PCMI_ERR_INVALID, PCMI_ERR_WORKSPACE, PCMI_OK
from test_detect_input_ref import GOLDEN, INT_KEYS, vote_bound, within_ulp

pytestmark = pytest.mark.gpu

LABEL_KEYS = ("center_label", "heading_class_label", "heading_residual_label", "size_class_label", "size_residual_label",
              "sem_cls_label", "box_label_mask")
NYU = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39], np.int32)


def PF():
  import pointcontrast_amd.functional as f
  return f


def _dev(a, dtype=None):
  t = torch.as_tensor(np.ascontiguousarray(a))
  return (t if dtype is None else t.to(dtype)).to(DEV)


def bits(a):
  a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
  return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same_bits(got, want, what=""):
  g, w = bits(got), bits(want)
  assert g.dtype == w.dtype and g.shape == w.shape, "%s: %s %s against %s %s" % (what, g.dtype, g.shape, w.dtype, w.shape)
  assert np.array_equal(g, w), "%s: %d of %d elements differ in their bits" % (what, int((g != w).sum()), g.size)


def draws(rng, B, angle=0.5, scale=True):
  ang = rng.uniform(-angle, angle, B)
  return dict(flip=rng.randint(0, 2, (B, 2)).astype(np.int32), rot=np.stack([dr.rotz(t).reshape(9) for t in ang]),
              scale=rng.uniform(0.85, 1.15, B) if scale else np.ones(B)), ang


def cloud(rng, sizes):
  n = int(sum(sizes))
  return (rng.uniform(-3, 3, (n, 3)).astype(np.float32), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))


# ---- sample and transform -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 63, 255, 256, 257, 1025])
def test_sample_transform_and_votes_transform(P):
  rng = np.random.RandomState(P)
  sizes = [400, 37]
  xyz, offs = cloud(rng, sizes)
  ch = np.stack([rng.randint(0, n, P) for n in sizes]).astype(np.int32)
  ins, sem = rng.randint(0, 50, len(xyz)).astype(np.int32), rng.randint(0, 41, len(xyz)).astype(np.int32)
  votes = rng.uniform(-1, 1, (len(xyz), 10))
  votes[:, 0] = rng.randint(0, 2, len(xyz))
  d, _ = draws(rng, 2)
  for augment in (True, False):
    got = PF().det_sample_transform(_dev(xyz), offs, ch, augment=augment, instance=ins, semantic=sem, **d)
    want = dr.sample_transform(xyz, offs, ch, augment=augment, instance=ins, semantic=sem, **d)
    for k in ("point_clouds", "out_instance", "out_semantic", "flags"):
      same_bits(got[k], want[k], "%s (augment %s)" % (k, augment))
    got = PF().det_votes_transform(_dev(xyz), _dev(votes), offs, ch, augment=augment, **d)
    want = dr.sample_transform(xyz, offs, ch, augment=augment, votes=votes, **d)
    for k in ("point_clouds", "vote_label", "vote_label_mask", "flags"):
      same_bits(got[k], want[k], "votes_transform %s (augment %s)" % (k, augment))
    assert not want["flags"].any() and want["vote_label_mask"].dtype == np.int64


def test_identity_rotation_and_scale_one():
  rng = np.random.RandomState(3)
  xyz, offs = cloud(rng, [5, 300])
  ch = np.stack([rng.randint(0, 5, 257), rng.randint(0, 300, 257)]).astype(np.int32)  # a scan of 5 rows sampled 257 times
  eye = dict(flip=np.zeros((2, 2), np.int32), rot=np.tile(np.eye(3).reshape(9), (2, 1)), scale=np.ones(2))
  got = PF().det_sample_transform(_dev(xyz), offs, ch, **eye)
  want = np.stack([xyz[ch[0]], xyz[5 + ch[1]]])
  same_bits(got["point_clouds"], want, "identity draws return the chosen rows")
  assert int(got["flags"].abs().sum()) == 0
  # scale 1 returns the rotated inputs: the same as a call whose scale is left out of the arithmetic (the restatement's r32)
  d, ang = draws(rng, 2, scale=False)
  votes = rng.uniform(-1, 1, (305, 10))
  got = PF().det_votes_transform(_dev(xyz), _dev(votes), offs, ch, **d)
  want = dr.sample_transform(xyz, offs, ch, votes=votes, **d)
  same_bits(got["point_clouds"], want["point_clouds"]), same_bits(got["vote_label"], want["vote_label"])
  for b in range(2):
    R = d["rot"][b].reshape(3, 3)
    p = want["point_clouds"][b].astype(np.float64)
    src = xyz[offs[b] + ch[b]].astype(np.float64)
    src[:, 0] *= -1 if d["flip"][b, 0] else 1
    src[:, 1] *= -1 if d["flip"][b, 1] else 1
    assert np.abs(p - src @ R.T).max() < 1e-6


def test_empty_scene_bad_choices_and_nan_rows_are_dropped():
  rng = np.random.RandomState(4)
  sizes = [100, 0, 120]
  xyz, offs = cloud(rng, sizes)
  xyz[100 + 7] = [np.nan, 0.0, 1.0]
  P = 64
  ch = np.stack([rng.randint(0, 100, P), rng.randint(0, 5, P), rng.randint(0, 120, P)]).astype(np.int32)
  ch[0, 3], ch[0, 9], ch[2, 5] = -1, 100, 7
  ins = rng.randint(1, 4, len(xyz)).astype(np.int32)
  sem = np.full(len(xyz), 5, np.int32)
  d, _ = draws(rng, 3)
  got = PF().det_sample_transform(_dev(xyz), offs, ch, instance=ins, semantic=sem, **d)
  want = dr.sample_transform(xyz, offs, ch, instance=ins, semantic=sem, **d)
  for k in ("point_clouds", "out_instance", "out_semantic", "flags"):
    same_bits(got[k], want[k], k)
  assert want["flags"].tolist() == [dr.FLAG_CHOICE, dr.FLAG_CHOICE, dr.FLAG_RANGE]
  pc = got["point_clouds"].cpu().numpy()
  assert not pc[0, 3].any() and not pc[0, 9].any() and not pc[1].any() and not pc[2, 5].any() and pc[0, 4].any()
  v = PF().det_votes_from_instances(got["point_clouds"], got["out_instance"], got["out_semantic"], NYU)
  wv = dr.votes_from_instances(want["point_clouds"], want["out_instance"], want["out_semantic"], NYU)
  same_bits(v["vote_label"], wv[0]), same_bits(v["vote_label_mask"], wv[1]), same_bits(v["flags"], wv[2])
  m = v["vote_label_mask"].cpu().numpy()
  assert m[0, 3] == 0 and m[0, 9] == 0 and m[2, 5] == 0 and not m[1].any() and m[0, 4] == 1 and not wv[2].any()
  # the SUN RGB-D mode drops the same rows
  votes = np.ones((len(xyz), 10))
  g2 = PF().det_votes_transform(_dev(xyz), _dev(votes), offs, ch, **d)
  w2 = dr.sample_transform(xyz, offs, ch, votes=votes, **d)
  for k in ("point_clouds", "vote_label", "vote_label_mask", "flags"):
    same_bits(g2[k], w2[k], k)
  assert w2["vote_label_mask"][0, 3] == 0 and not w2["vote_label"][2, 5].any() and w2["vote_label_mask"][0, 4] == 1


# ---- votes from instances -------------------------------------------------------------------------------------------------------
def test_instance_votes_edges():
  rng = np.random.RandomState(5)
  B, P = 2, 70000
  pc = rng.uniform(-4, 4, (B, P, 3)).astype(np.float32)
  ins = rng.randint(10, 40, (B, P)).astype(np.int32)
  sem = np.full((B, P), 5, np.int32)
  lim = dr.MAX_INSTANCES
  ins[0, 17] = 1            # an instance of one point: vote 0, mask 1
  ins[0, [20, 30, 40]] = 2  # two semantic labels, valid only at the first row
  sem[0, [30, 40]] = 1
  ins[0, [21, 31, 41]] = 3  # and the converse: no vote
  sem[0, 21] = 1
  ins[0, [5, 6, P - 2, P - 1]] = 7  # rows in the first and in the last workgroup of the scene
  ins[0, [50, 51]] = lim - 1
  ins[1, 60] = lim          # flagged, no vote
  ins[1, 61] = -5
  ins[1, 62] = -1           # a dropped row: silent
  sem[1, ins[1] == 12] = 2  # the same id is valid in scene 0 and not in scene 1: nothing leaks
  ins[1, [70, 71, 72, 73]] = 8  # -0.0, +0.0 and both signs: the ordered-integer image
  pc[1, [70, 71, 72, 73]] = np.array([[-0.0, -1.5, 0.0], [0.0, 2.5, -0.0], [-0.0, -0.0, -0.0], [0.0, 1e-30, -1e-30]], np.float32)
  ins[1, [80, 81]] = 9      # every coordinate -0.0: the centre is -0.0, the vote +0.0
  pc[1, [80, 81]] = np.float32(-0.0)
  sem[1, [70, 71, 72, 73, 80, 81]] = 5
  got = PF().det_votes_from_instances(_dev(pc), _dev(ins), _dev(sem), NYU)
  vl, vm, fl = dr.votes_from_instances(pc, ins, sem, NYU)
  same_bits(got["vote_label"], vl, "vote_label"), same_bits(got["vote_label_mask"], vm, "mask"), same_bits(got["flags"], fl, "flags")
  assert fl.tolist() == [0, dr.FLAG_INSTANCE]
  assert vm[0, 17] == 1 and not vl[0, 17].any()
  assert vm[0, [20, 30, 40]].all() and not vm[0, [21, 31, 41]].any()
  assert vm[0, [50, 51]].all() and vm[1, 60] == 0 and vm[1, 61] == 0 and vm[1, 62] == 0
  assert vm[0][ins[0] == 12].all() and not vm[1][ins[1] == 12].any()
  c7 = 0.5 * (pc[0, [5, 6, P - 2, P - 1]].min(0) + pc[0, [5, 6, P - 2, P - 1]].max(0))
  assert np.array_equal(vl[0, P - 1, :3], c7 - pc[0, P - 1]), "the instance's box spans the first and the last workgroup"
  got2 = PF().det_votes_from_instances(_dev(pc), _dev(ins), _dev(sem), NYU)
  same_bits(got2["vote_label"], got["vote_label"], "two runs")


# ---- vote transform and boxes ---------------------------------------------------------------------------------------------------
def _box_case(rng, mode):
  B, K = 4, dr.MAX_NUM_OBJ
  boxes = np.zeros((B, K, 8))
  n_boxes = np.array([0, K, 6, 3], np.int32)
  for b in range(B):
    k = n_boxes[b]
    boxes[b, :k, 0:3] = rng.uniform(-3, 3, (k, 3))
    boxes[b, :k, 3:6] = rng.uniform(0.1, 1.5, (k, 3))
    if mode == dr.SUNRGBD:
      boxes[b, :k, 6] = rng.uniform(-np.pi, np.pi, k)
      boxes[b, :k, 7] = rng.randint(0, 10, k)
    else:
      boxes[b, :k, 7] = rng.choice(NYU, k)
  per = 2 * np.pi / 12
  # exactly on a bin border (shifted = per), negative, above 2 pi, 0 and 2 pi itself
  boxes[2, :6, 6] = [per / 2, -2.5, 7.0, 0.0, 2 * np.pi, -1e-20] if mode == dr.SUNRGBD else 0.0
  return boxes, n_boxes


@pytest.mark.parametrize("mode", [dr.SCANNET, dr.SUNRGBD])
def test_box_labels(mode):
  rng = np.random.RandomState(6 + mode)
  boxes, n_boxes = _box_case(rng, mode)
  B = len(boxes)
  mean = rng.uniform(0.3, 2.0, (18 if mode == dr.SCANNET else 10, 3))
  lut = dr.nyu40id_table(NYU)
  name = "scannet" if mode == dr.SCANNET else "sunrgbd"
  ang = np.array([0.3, -0.4, 0.0, 0.2])  # scene 2: rotate_aligned_boxes at angle 0, heading borders unmoved
  flip = np.array([[1, 1], [1, 0], [0, 0], [0, 1]], np.int32)
  scale = np.array([1.1, 0.9, 1.0, 1.0])  # scene 3: scale 1 returns the rotated inputs
  rot = np.stack([dr.rotz(t).reshape(9) for t in ang])
  for augment in (True, False):
    cs = dr.heading_cs(boxes, n_boxes, augment, flip, ang)
    want = dr.box_labels(boxes, n_boxes, mode, augment=augment, flip=flip, rot=rot, rot_angle=ang, scale=scale, label_to_class=lut,
                         mean_size=mean, num_heading_bin=12, cs=cs)
    got = PF().det_box_labels(_dev(boxes), n_boxes, name, mean, augment=augment, flip=flip, rot=rot, rot_angle=ang, scale=scale,
                              heading_cs=cs if mode == dr.SUNRGBD else None, label_to_class=lut if mode == dr.SCANNET else None,
                              num_heading_bin=12)
    live = np.arange(dr.MAX_NUM_OBJ)[None] < n_boxes[:, None]
    for k in LABEL_KEYS + ("flags",):
      g, w = got[k].cpu().numpy(), want[k]
      assert g.dtype == w.dtype and g.shape == w.shape, k
      if k == "flags":
        assert np.array_equal(g, w) and not w.any()
        continue
      same_bits(g[live], w[live], "%s, live slots (augment %s)" % (k, augment))
      assert np.array_equal(g[~live], w[~live]), "%s, padded slots by value" % k  # a flipped zero is -0
    assert want["box_label_mask"].sum(1).tolist() == n_boxes.tolist()
    if mode == dr.SUNRGBD:
      hc, hr = want["heading_class_label"][2, :6], want["heading_residual_label"][2, :6]
      if not augment:
        assert hc.tolist() == [1, 7, 1, 0, 0, 0], hc  # border -> the upper bin; -2.5 and 7.0 wrap by the % rule
        assert hr[0] == np.float32(-(2 * np.pi / 12) / 2) and hr[3] == 0 and hr[4] == 0
      else:
        # flip with pi - h (scene 0 flips x): the final heading's class is that of pi - h - angle
        h0 = np.pi - boxes[0, 0, 6] - ang[0] if n_boxes[0] else 0.0
        assert n_boxes[0] == 0 or want["heading_class_label"][0, 0] == int(((h0 % (2 * np.pi)) + np.pi / 12) % (2 * np.pi) / (2 * np.pi / 12))
        h1 = (np.pi - boxes[1, :, 6]) - ang[1]
        wc = [int((((h % (2 * np.pi)) + (2 * np.pi / 12) / 2) % (2 * np.pi)) / (2 * np.pi / 12)) for h in h1]
        assert want["heading_class_label"][1].tolist() == wc
        # scale 1 (scene 3): the centre of an upright hull is the rotated centre
        c = boxes[3, :3, 0:3] @ rot[3].reshape(3, 3).T
        assert np.abs(want["center_label"][3, :3] - c).max() < 1e-5
    elif augment:
      # angle 0 (scene 2, no flip): rotate_aligned_boxes returns the boxes
      assert np.array_equal(want["center_label"][2, :6], boxes[2, :6, 0:3].astype(np.float32))
      res = boxes[2, :6, 3:6] - mean[lut[boxes[2, :6, 7].astype(int)]]
      assert np.array_equal(want["size_residual_label"][2, :6], res.astype(np.float32))


def test_box_labels_flags():
  rng = np.random.RandomState(8)
  boxes, n_boxes = _box_case(rng, dr.SCANNET)
  boxes[1, 4, 7] = 13       # not one of the detection classes
  boxes[2, 1, 0] = np.inf
  n_boxes[3] = 65
  mean, lut = rng.uniform(0.3, 2.0, (18, 3)), dr.nyu40id_table(NYU)
  want = dr.box_labels(boxes, n_boxes, dr.SCANNET, augment=False, label_to_class=lut, mean_size=mean)
  got = PF().det_box_labels(_dev(boxes), n_boxes, "scannet", mean, augment=False, label_to_class=lut)
  assert want["flags"].tolist() == [0, dr.FLAG_LABEL, dr.FLAG_RANGE, dr.FLAG_BOXES]
  for k in LABEL_KEYS + ("flags",):
    same_bits(got[k], want[k], k)
  assert want["box_label_mask"][2, 1] == 1 and not want["center_label"][2, 1].any() and not want["box_label_mask"][3].any()
  boxes, n_boxes = _box_case(rng, dr.SUNRGBD)
  boxes[1, 4, 7], boxes[2, 1, 6], n_boxes[3] = 10, np.nan, -1
  cs = dr.heading_cs(boxes, n_boxes, False, None, None)
  want = dr.box_labels(boxes, n_boxes, dr.SUNRGBD, augment=False, mean_size=mean[:10], cs=cs)
  got = PF().det_box_labels(_dev(boxes), n_boxes, "sunrgbd", mean[:10], augment=False, heading_cs=cs, num_heading_bin=12)
  assert want["flags"].tolist() == [0, dr.FLAG_LABEL, dr.FLAG_RANGE, dr.FLAG_BOXES]
  for k in LABEL_KEYS + ("flags",):
    same_bits(got[k], want[k], k)


# ---- voxelize -------------------------------------------------------------------------------------------------------------------
def _check_voxelize(pc, vs):
  got = PF().det_voxelize(_dev(pc), vs)
  vc, vi, vf, counts, flags = dr.voxelize(pc, vs)
  M = int(counts[-1])
  same_bits(got["counts"], counts, "counts"), same_bits(got["flags"], flags, "flags")
  same_bits(got["voxel_coords"][:M], vc, "voxel_coords"), same_bits(got["voxel_inds"][:M], vi, "voxel_inds")
  same_bits(got["voxel_feats"][:M], vf, "voxel_feats")
  return vc, vi, counts, flags


def test_voxelize_edges():
  rng = np.random.RandomState(9)
  vs = 0.025
  P = 1025
  pc = rng.uniform(-1.5, 1.5, (4, P, 3)).astype(np.float32)  # scene 0: negative coordinates and both signs
  k = rng.randint(-40, 40, (P, 3))
  pc[1] = (k * vs).astype(np.float32)                        # scene 1: points exactly on voxel faces, k voxel_size rounded to fp32
  pc[2] = np.float32(0.2505) + rng.uniform(0, 0.02, (P, 3)).astype(np.float32)  # scene 2: one voxel, [10.02, 10.82) voxel sizes
  pc[3] = pc[0][rng.randint(0, 40, P)]                       # scene 3: the duplicates of a replacement choice
  vc, vi, counts, flags = _check_voxelize(pc, vs)
  assert not flags.any() and counts[2] == 1 and vi[counts[0] + counts[1]] == 0 and counts[3] <= 40
  q1 = np.floor(pc[1] / np.float32(vs)).astype(np.int32)
  assert (q1 != k).any() and (q1 == k).any(), "the face case has points on both sides of the fp32 rounding"
  first3 = vi[counts[:3].sum():]
  assert np.array_equal(np.sort(first3), first3) and len(np.unique(pc[3][first3], axis=0)) == len(first3)
  # a NaN and a far point are dropped with the flag
  pc[0, 5], pc[2, 3] = np.nan, 1e9
  _, _, _, flags = _check_voxelize(pc, vs)
  assert flags.tolist() == [dr.FLAG_RANGE, 0, dr.FLAG_RANGE, 0]


def test_voxelize_70000_rows():
  rng = np.random.RandomState(10)
  pc = (rng.uniform(-3, 3, (1, 70000, 3)) * [1, 1, 0.3]).astype(np.float32)
  pc[0, 35000:] = pc[0, :35000] + np.float32(0.003)
  vc, vi, counts, flags = _check_voxelize(pc, 0.025)
  assert not flags.any() and counts[0] < 70000


# ---- the pipeline ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def G():
  return np.load(GOLDEN)


def _golden_batch(G, ds):
  from pointcontrast_amd.downstream.votenet import DetectionDraws, DetectionInputPipeline
  if ds == "scannet":
    scenes = [(G["scannet%d_vert" % s], G["scannet%d_ins" % s], G["scannet%d_sem" % s], G["scannet%d_bbox" % s]) for s in range(3)]
    pipe = DetectionInputPipeline("scannet", int(G["num_points"]), float(G["voxel_size"]), DEV, valid_sem=G["scannet_nyu40ids"],
                                  mean_size_arr=G["scannet_mean_size_arr"])
    kw = dict(valid_sem=G["scannet_nyu40ids"], label_to_class=dr.nyu40id_table(G["scannet_nyu40ids"]), mean_size=G["scannet_mean_size_arr"])
    scale = np.ones(3)
  else:
    scenes = [(G["sunrgbd%d_pc" % s], G["sunrgbd%d_bbox" % s], G["sunrgbd%d_votes" % s]) for s in range(3)]
    pipe = DetectionInputPipeline("sunrgbd", int(G["num_points"]), float(G["voxel_size"]), DEV, mean_size_arr=G["sunrgbd_mean_size_arr"],
                                  num_heading_bin=int(G["sunrgbd_num_heading_bin"]))
    kw = dict(mean_size=G["sunrgbd_mean_size_arr"], num_heading_bin=int(G["sunrgbd_num_heading_bin"]))
    scale = np.array([float(G["sunrgbd_run%d_scale" % r]) for r in range(3)])
  pre = [ds + "_run%d_" % r for r in range(3)]
  flip = np.stack([G[p + "flip"] for p in pre])
  d = DetectionDraws(np.stack([G[p + "choices"] for p in pre]), flip[:, 0], flip[:, 1], [float(G[p + "rot_angle"]) for p in pre], scale)
  return scenes, pipe, d, kw


@pytest.mark.parametrize("ds", ["scannet", "sunrgbd"])
def test_pipeline_on_the_golden_scans(G, ds):
  scenes, pipe, d, kw = _golden_batch(G, ds)
  out = pipe(scenes, d)
  want = dr.batch(ds, scenes, d.choices, True, d.flip(), d.rot_angle, d.scale, float(G["voxel_size"]), **kw)
  assert not want["flags"].any()
  for k in LABEL_KEYS + ("point_clouds", "vote_label", "vote_label_mask", "voxel_coords", "voxel_inds", "voxel_feats"):
    if k == "center_label":  # the padded slots by value: a flipped zero is -0
      assert np.array_equal(out[k].cpu().numpy(), want[k]), k
      live = want["box_label_mask"] > 0
      same_bits(out[k].cpu().numpy()[live], want[k][live], k)
    else:
      same_bits(out[k], want[k], k)
  assert out["voxel_coords"].dtype == torch.int32 and out["voxel_inds"].dtype == torch.int32 and out["vote_label_mask"].dtype == torch.int64
  # and the golden file, within the bounds of tests/test_detect_input_ref.py
  for r in range(3):
    pre = "%s_run%d_" % (ds, r)
    for k in ("point_clouds", "center_label", "size_residual_label", "heading_residual_label"):
      assert within_ulp(out[k][r].cpu().numpy(), G[pre + k]), "%s of scene %d beyond 1 fp32 ulp of the reference" % (k, r)
    for k in INT_KEYS + ("vote_label_mask",):
      assert np.array_equal(out[k][r].cpu().numpy(), G[pre + k]), k
    got, ref = out["vote_label"][r].cpu().numpy(), G[pre + "vote_label"]
    bound = vote_bound(ds, G[pre + "point_clouds"], float(d.scale[r]), got, ref)
    assert (np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= bound).all(), "vote_label of scene %d" % r
  # the voxels: the reference's sets per scene (its order is unspecified)
  vc = out["voxel_coords"].cpu().numpy()
  same = all(np.array_equal(out["point_clouds"][r].cpu().numpy(), G["%s_run%d_point_clouds" % (ds, r)]) for r in range(3))
  if same:
    assert sorted(map(tuple, vc)) == sorted(map(tuple, G[ds + "_batch_voxel_coords"].astype(np.int32)))


def test_draws_are_reproducible_and_identity_without_augment():
  from pointcontrast_amd.downstream.votenet import DetectionDraws
  sizes = [500, 100, 300]
  for ds in ("scannet", "sunrgbd"):
    a, b = DetectionDraws.sample(sizes, 256, ds, 7), DetectionDraws.sample(sizes, 256, ds, 7)
    c = DetectionDraws.sample(sizes, 256, ds, 8)
    for f in ("choices", "flip_x", "flip_y", "rot_angle", "scale"):
      same_bits(getattr(a, f).astype(np.float64) if f.startswith("flip") else getattr(a, f),
                getattr(b, f).astype(np.float64) if f.startswith("flip") else getattr(b, f), f)
    assert not np.array_equal(a.choices, c.choices)
    assert len(np.unique(a.choices[0])) == 256 and len(np.unique(a.choices[1])) < 256, "without and with replacement"
    w = np.pi / 36 if ds == "scannet" else np.pi / 6
    assert (np.abs(a.rot_angle) <= w).all() and a.rot_angle.any()
    assert (a.scale == 1).all() if ds == "scannet" else ((a.scale >= 0.85) & (a.scale < 1.15) & (a.scale != 1)).all()
    assert ds == "scannet" or not a.flip_y.any()
    e = DetectionDraws.sample(sizes, 256, ds, 7, augment=False)
    assert not e.augment and not e.flip_x.any() and not e.flip_y.any() and not e.rot_angle.any() and (e.scale == 1).all()


def test_no_augment_is_the_identity_apart_from_the_choice(G):
  from pointcontrast_amd.downstream.votenet import DetectionDraws
  for ds in ("scannet", "sunrgbd"):
    scenes, pipe, d, kw = _golden_batch(G, ds)
    e = DetectionDraws.sample([len(s[0]) for s in scenes], pipe.num_points, ds, 3, augment=False)
    out = pipe(scenes, e)
    for b, s in enumerate(scenes):
      same_bits(out["point_clouds"][b], s[0][e.choices[b]], "point_clouds")
      if ds == "sunrgbd":
        same_bits(out["vote_label"][b], s[2][e.choices[b], 1:].astype(np.float32), "vote_label")
    # the reference's own run without augmentation (run 3, scan 0)
    pre = ds + "_run3_"
    e1 = DetectionDraws(G[pre + "choices"][None], augment=False)
    o1 = pipe(scenes[:1], e1)
    for k in LABEL_KEYS + ("point_clouds", "vote_label", "vote_label_mask"):
      assert np.array_equal(o1[k][0].cpu().numpy(), G[pre + k]), k


def test_pipeline_raises_on_a_flagged_scene(G):
  scenes, pipe, d, _ = _golden_batch(G, "scannet")
  d.choices[1, 4] = 100000
  with pytest.raises(ValueError, match=r"scene 1: a choice is outside"):
    pipe(scenes, d)


def test_dict_feeds_sample_seeds_and_get_loss():
  import pointcontrast_amd.minkowski as ME
  from pointcontrast_amd.downstream import votenet
  from pointcontrast_amd.lib.config import get_config
  from pointcontrast_amd.model import load_model
  rng = np.random.RandomState(11)
  B, P, num_seed, K = 2, 256, 64, 32
  scenes = []
  for b in range(B):
    n = 400 + 50 * b
    ins = rng.randint(0, 6, n)
    cen = rng.uniform(0.5, 2.5, (6, 3))
    xyz = (cen[ins] + rng.uniform(-0.4, 0.4, (n, 3))).astype(np.float32)
    sem = np.array([0, 3, 4, 5, 1, 7])[ins]
    boxes = np.concatenate([rng.uniform(0.5, 2.5, (4, 3)), rng.uniform(0.3, 1.0, (4, 3)), rng.choice(NYU, (4, 1))], 1)
    scenes.append((xyz, ins, sem, boxes))
  mean = rng.uniform(0.4, 1.5, (18, 3))
  pipe = votenet.DetectionInputPipeline("scannet", P, 0.05, DEV, mean_size_arr=mean)
  batch = pipe(scenes, votenet.DetectionDraws.sample([len(s[0]) for s in scenes], P, "scannet", 5))
  assert batch["vote_label_mask"].any() and batch["box_label_mask"].sum() == 8
  torch.manual_seed(0)
  cfg = get_config(["net.normalize_feature=False"])
  model = load_model("Res16UNet14")(3, 32, cfg, D=3).to(DEV)
  sparse = model(ME.SparseTensor(batch["voxel_feats"].cpu(), coords=batch["voxel_coords"].cpu()).to(DEV))
  xyz, feats, inds = votenet.sample_seeds(sparse, batch["point_clouds"], batch["voxel_inds"], num_seed)
  assert xyz.shape == (B, num_seed, 3) and feats.shape == (B, 32, num_seed) and inds.dtype == torch.int64
  assert torch.equal(xyz, torch.gather(batch["point_clouds"], 1, inds[..., None].expand(-1, -1, 3)))
  ep, lcfg = VF.loss_inputs(B=B, num_points=P, num_seed=num_seed, K=K, K2=dr.MAX_NUM_OBJ, H=1, S=18, Cls=18, seed=1)
  lcfg.mean_size_arr = mean.astype(np.float32)
  ep = {k: v.to(DEV) for k, v in ep.items()}
  ep.update({k: v for k, v in batch.items() if k in ep})
  ep["seed_xyz"], ep["seed_inds"] = xyz, inds
  ep["vote_xyz"] = (xyz + 0.1).requires_grad_()
  loss, _ = votenet.get_loss(ep, lcfg)
  assert bool(torch.isfinite(loss))


# ---- C contract -----------------------------------------------------------------------------------------------------------------
def test_c_contract_exact_workspaces_and_refusals():
  from pointcontrast_amd._lib import lib
  rng = np.random.RandomState(12)
  B, P, n = 3, 300, 777
  SENT = 0x7FC0BEEF
  xyz, offs = cloud(rng, [300, 0, 477])
  xyz_d, offs_d = _dev(xyz), _dev(offs)
  ch = _dev(np.stack([rng.randint(0, 300, P), np.zeros(P, np.int64), rng.randint(0, 477, P)]).astype(np.int32))
  d, ang = draws(rng, B)
  flip, rot, scale, ang_d = _dev(d["flip"]), _dev(d["rot"]), _dev(d["scale"]), _dev(ang)
  ins, sem = _dev(rng.randint(0, 9, n).astype(np.int32)), _dev(rng.choice(NYU, n).astype(np.int32))
  votes = _dev(rng.uniform(-1, 1, (n, 10)))
  valid = _dev(NYU)
  boxes, n_boxes = _box_case(rng, dr.SUNRGBD)
  boxes_d, nb_d = _dev(boxes[:B]), _dev(n_boxes[:B])
  cs = _dev(dr.heading_cs(boxes[:B], n_boxes[:B], True, d["flip"], ang))
  mean = _dev(rng.uniform(0.3, 2.0, (10, 3)))
  i32 = lambda *s: torch.full(s, SENT, dtype=torch.int32, device=DEV)  # noqa: E731
  f32 = lambda *s: i32(*s).view(torch.float32)  # noqa: E731
  i64 = lambda *s: torch.full(s, SENT, dtype=torch.int64, device=DEV)  # noqa: E731
  pc, oi, os_ = f32(B, P, 3), i32(B, P), i32(B, P)
  vl, vm = f32(B, P, 9), i64(B, P)
  lab = dict(c=f32(B, 64, 3), hc=i64(B, 64), hr=f32(B, 64), sc=i64(B, 64), sr=f32(B, 64, 3), se=i64(B, 64), bm=f32(B, 64))
  vc, vi, vf, counts = i32(B * P, 4), i32(B * P), f32(B * P, 3), i64(B + 1)
  flags = torch.zeros(B, dtype=torch.int32, device=DEV)
  p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
  off1 = lambda t: C.c_void_p(t.data_ptr() + 1)  # noqa: E731
  st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
  outputs = [pc, oi, os_, vl, vm, vc, vi, vf, counts] + list(lab.values())

  def untouched():
    torch.cuda.synchronize()
    return all(bool((t.view(torch.int32) == SENT).all()) if t.dtype != torch.int64 else bool((t == SENT).all()) for t in outputs) \
        and int(flags.abs().sum()) == 0

  def sample(B_=B, P_=P, xyz_=p(xyz_d), rot_=p(rot), pc_=p(pc), oi_=p(oi), ch_=p(ch)):
    return lib.pcmi_det_sample_transform(xyz_, p(offs_d), n, B_, P_, ch_, 1, p(flip), rot_, p(scale), p(ins), p(sem), pc_, oi_, p(os_),
                                         p(flags), st)

  def vtrans(B_=B, votes_=p(votes), vm_=p(vm), rot_=p(rot)):
    return lib.pcmi_det_votes_transform(p(xyz_d), votes_, p(offs_d), n, B_, P, p(ch), 1, p(flip), rot_, p(scale), p(pc), p(vl), vm_,
                                        p(flags), st)

  def vinst(ws, size, B_=B, P_=P, pc_=p(pc), nv=len(NYU)):
    return lib.pcmi_det_votes_from_instances(pc_, p(oi), p(os_), B_, P_, p(valid), nv, p(vl), p(vm), p(flags), ws, size, st)

  def box(B_=B, mode=1, boxes_=p(boxes_d), cs_=p(cs), hc_=p(lab["hc"]), nhb=12):
    return lib.pcmi_det_box_labels(boxes_, p(nb_d), B_, mode, 1, p(flip), p(rot), p(ang_d), p(scale), cs_, None, 0, p(mean), 10, nhb,
                                   p(lab["c"]), hc_, p(lab["hr"]), p(lab["sc"]), p(lab["sr"]), p(lab["se"]), p(lab["bm"]), p(flags), st)

  def vox(ws, size, B_=B, P_=P, pc_=p(pc), vs=0.05):
    return lib.pcmi_det_voxelize(pc_, B_, P_, vs, p(vc), p(vi), p(vf), p(counts), p(flags), ws, size, st)

  # every refusal first: nothing is enqueued, every output keeps its sentinel
  for bad in (0, 1024, -1):
    assert sample(B_=bad) == PCMI_ERR_INVALID and vtrans(B_=bad) == PCMI_ERR_INVALID and box(B_=bad) == PCMI_ERR_INVALID
  assert sample(P_=0) == PCMI_ERR_INVALID and sample(xyz_=None) == PCMI_ERR_INVALID and sample(rot_=None) == PCMI_ERR_INVALID
  assert sample(pc_=None) == PCMI_ERR_INVALID and sample(oi_=None) == PCMI_ERR_INVALID and sample(ch_=None) == PCMI_ERR_INVALID
  assert sample(rot_=off1(rot)) == PCMI_ERR_INVALID and sample(pc_=off1(pc)) == PCMI_ERR_INVALID
  assert vtrans(votes_=None) == PCMI_ERR_INVALID and vtrans(vm_=None) == PCMI_ERR_INVALID and vtrans(votes_=off1(votes)) == PCMI_ERR_INVALID
  assert vtrans(vm_=off1(vm)) == PCMI_ERR_INVALID and vtrans(rot_=None) == PCMI_ERR_INVALID
  assert box(mode=2) == PCMI_ERR_INVALID and box(boxes_=None) == PCMI_ERR_INVALID and box(cs_=None) == PCMI_ERR_INVALID
  assert box(hc_=None) == PCMI_ERR_INVALID and box(boxes_=off1(boxes_d)) == PCMI_ERR_INVALID and box(hc_=off1(lab["hc"])) == PCMI_ERR_INVALID
  assert box(nhb=0) == PCMI_ERR_INVALID
  qi, qv = lib.pcmi_det_votes_from_instances_workspace_bytes(B), lib.pcmi_det_voxelize_workspace_bytes(B, P)
  assert qi > 0 and qv > 0
  gi, gv = Guarded(qi), Guarded(qv)
  for call, g, q in ((vinst, gi, qi), (vox, gv, qv)):
    assert call(g.vp, C.c_size_t(q - 1)) == PCMI_ERR_WORKSPACE and call(None, g.size) == PCMI_ERR_WORKSPACE, call.__name__
    assert call(C.c_void_p(g.ptr + 8), g.size) == PCMI_ERR_INVALID, "a workspace that is not 16-byte aligned"
    for bad in (0, 1024, -1):
      assert call(g.vp, g.size, B_=bad) == PCMI_ERR_INVALID, call.__name__
    assert call(g.vp, g.size, P_=0) == PCMI_ERR_INVALID and call(g.vp, g.size, pc_=None) == PCMI_ERR_INVALID
    assert call(g.vp, g.size, pc_=off1(pc)) == PCMI_ERR_INVALID
  assert vinst(gi.vp, gi.size, nv=1025) == PCMI_ERR_INVALID and vox(gv.vp, gv.size, vs=0.0) == PCMI_ERR_INVALID
  assert vox(gv.vp, gv.size, vs=float("nan")) == PCMI_ERR_INVALID
  assert lib.pcmi_det_votes_from_instances_workspace_bytes(0) == 0 and lib.pcmi_det_voxelize_workspace_bytes(1024, 5) == 0
  assert lib.pcmi_det_voxelize_workspace_bytes(2, 1 << 29) == 0
  assert untouched(), "a refused call wrote to an output or to the flags"
  gi.check("refused"), gv.check("refused")
  # the exact workspaces succeed and stay inside them; the chain equals the restatement
  assert sample() == PCMI_OK and vinst(gi.vp, gi.size) == PCMI_OK and box() == PCMI_OK and vox(gv.vp, gv.size) == PCMI_OK
  torch.cuda.synchronize()
  gi.check("votes_from_instances"), gv.check("voxelize")
  ws = dr.sample_transform(xyz, offs, ch.cpu().numpy(), instance=ins.cpu().numpy(), semantic=sem.cpu().numpy(), **d)
  wv = dr.votes_from_instances(ws["point_clouds"], ws["out_instance"], ws["out_semantic"], NYU)
  wx = dr.voxelize(ws["point_clouds"], 0.05)
  wb = dr.box_labels(boxes[:B], n_boxes[:B], dr.SUNRGBD, rot_angle=ang, mean_size=mean.cpu().numpy(), num_heading_bin=12, **d)
  same_bits(pc, ws["point_clouds"]), same_bits(vl, wv[0]), same_bits(vm, wv[1])
  M = int(wx[3][-1])
  same_bits(counts, wx[3]), same_bits(vc[:M], wx[0]), same_bits(vi[:M], wx[1])
  assert bool((vc[M:] == SENT).all()) and bool((vi[M:] == SENT).all()), "rows beyond counts[B] are not written"
  same_bits(lab["hc"], wb["heading_class_label"]), same_bits(lab["sr"], wb["size_residual_label"])
  assert flags.cpu().tolist() == (ws["flags"] | wv[2] | wx[4] | wb["flags"]).tolist() == [0, dr.FLAG_CHOICE, 0]
  assert vtrans() == PCMI_OK
  wt = dr.sample_transform(xyz, offs, ch.cpu().numpy(), votes=votes.cpu().numpy(), **d)
  same_bits(vl, wt["vote_label"]), same_bits(vm, wt["vote_label_mask"])
