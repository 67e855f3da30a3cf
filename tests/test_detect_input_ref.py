"""tests/detect_input_ref.py (the restatement that the GPU tests compare the detection input kernels with) held to what the
reference's own ScannetDetectionDataset, SunrgbdDetectionVotesDataset, VoxelizationDataset and collate_fn returned on small
synthetic scans: tests/golden/golden_detinput.npz, recorded by tests/golden/make_golden_detinput.py with the draws np.random
handed out.

Bounds.  The two sides differ only in the order of the three fp64 terms inside np.dot (the BLAS's) against the fixed order of
pcmi.h: an error of some 1e-16 relative, which can move a final fp32 rounding by one step at most.  So point_clouds, box
centres and size residuals are held to 1 fp32 ulp, integers and masks to equality.  The SUN RGB-D votes are end - fp32(rotated
point): a rotated point that moved by its one ulp moves the vote by that much, times the scale, on top of the vote's own
rounding -- the bound is ulp(point) * scale + ulp(vote) (vote_bound below).  Fed the reference's own point_clouds, the instance votes (float32
min, max, subtract) and the voxels (a float32 division and a floor) are exact."""
import os

import numpy as np
import pytest

import detect_input_ref as dr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_detinput.npz")
INT_KEYS = ("heading_class_label", "size_class_label", "sem_cls_label", "box_label_mask")


@pytest.fixture(scope="module")
def G():
  return np.load(GOLDEN)


def within_ulp(a, b, n=1):
  a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
  return bool((np.abs(a.astype(np.float64) - b.astype(np.float64)) <= n * np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)).all())


def vote_bound(ds, point_clouds, scale, got, want):
  """How far a vote computed from points that sit within one fp32 ulp of the reference's may lie from the reference's vote.
  u = the ulp of the ROTATED point (point_clouds / scale, taken two floats up: the division and the reference's own rounding
  each move it by 2^-24 at most).  SUN RGB-D: vote = fp32((end - rotated) scale), so u scale, plus one ulp of the vote for
  its own rounding.  ScanNet: min and max move by u each (u at the scene's largest coordinate), fp32(mn + mx) rounds by
  another u on either side, halved: 2 u for the centre; the point itself u; the subtraction's rounding one ulp of the vote:
  3 u + ulp(vote)."""
  pc = np.abs(np.asarray(point_clouds, dtype=np.float64)) / scale
  if ds == "scannet":
    pc = np.broadcast_to(pc.max(0, keepdims=True), pc.shape)
  x = pc.astype(np.float32)
  x = np.nextafter(np.nextafter(x, np.float32(np.inf)), np.float32(np.inf))
  u = np.tile(np.spacing(x).astype(np.float64), (1, 3))
  own = np.spacing(np.maximum(np.abs(got), np.abs(want)).astype(np.float32)).astype(np.float64)
  return u * (scale if ds == "sunrgbd" else 3.0) + own


def run(G, ds, r, point_clouds=None):
  """The restatement on run r of dataset ds, from the scans and the recorded draws."""
  s = int(G["%s_run%d_scan" % (ds, r)])
  if ds == "scannet":
    scene = (G["scannet%d_vert" % s], G["scannet%d_ins" % s], G["scannet%d_sem" % s], G["scannet%d_bbox" % s])
    kw = dict(valid_sem=G["scannet_nyu40ids"], label_to_class=dr.nyu40id_table(G["scannet_nyu40ids"]), mean_size=G["scannet_mean_size_arr"],
              scale=[1.0])
  else:
    scene = (G["sunrgbd%d_pc" % s], G["sunrgbd%d_bbox" % s], G["sunrgbd%d_votes" % s])
    kw = dict(mean_size=G["sunrgbd_mean_size_arr"], num_heading_bin=int(G["sunrgbd_num_heading_bin"]), scale=[float(G["sunrgbd_run%d_scale" % r])])
  pre = "%s_run%d_" % (ds, r)
  out = dr.batch(ds, [scene], G[pre + "choices"][None], bool(G[pre + "augment"]), G[pre + "flip"][None], [float(G[pre + "rot_angle"])],
                 voxel_size=float(G["voxel_size"]), point_clouds=None if point_clouds is None else point_clouds[None], **kw)
  assert not out["flags"].any()
  return scene, out


@pytest.mark.parametrize("ds", ["scannet", "sunrgbd"])
def test_golden_covers_the_cases(G, ds):
  runs = int(G[ds + "_runs"])
  assert runs == 4
  P = int(G["num_points"])
  sizes = [len(G[("scannet%d_vert" if ds == "scannet" else "sunrgbd%d_pc") % s]) for s in range(3)]
  assert min(sizes) < P < max(sizes), "one scan is smaller than num_points (replacement), one larger"
  ch = G[ds + "_run1_choices"]
  assert len(np.unique(ch)) < len(ch), "the small scan is sampled with replacement"
  flips = np.stack([G["%s_run%d_flip" % (ds, r)] for r in range(runs)])
  assert flips[:, 0].min() == 0 and flips[:, 0].max() == 1
  assert [int(G["%s_run%d_box_label_mask" % (ds, r)].sum()) for r in range(3)][2] == 0, "one scene has no box"
  assert int(G[ds + "_run3_augment"]) == 0
  if ds == "scannet":
    assert flips[:, 1].min() == 0 and flips[:, 1].max() == 1
    valid = set(G["scannet_nyu40ids"].tolist())
    sem, ins = G["scannet0_sem"], G["scannet0_ins"]
    assert any(int(sem[ins == i][0]) not in valid for i in np.unique(ins)), "an instance whose semantic label is not valid"


@pytest.mark.parametrize("r", range(4))
@pytest.mark.parametrize("ds", ["scannet", "sunrgbd"])
def test_restatement_against_reference(G, ds, r):
  pre = "%s_run%d_" % (ds, r)
  scene, out = run(G, ds, r)
  assert within_ulp(out["point_clouds"][0], G[pre + "point_clouds"]), "point_clouds beyond 1 fp32 ulp"
  assert within_ulp(out["center_label"][0], G[pre + "center_label"]), "center_label beyond 1 fp32 ulp"
  assert within_ulp(out["size_residual_label"][0], G[pre + "size_residual_label"]), "size_residual_label beyond 1 fp32 ulp"
  assert within_ulp(out["heading_residual_label"][0], G[pre + "heading_residual_label"])
  for k in INT_KEYS:
    assert out[k][0].dtype == G[pre + k].dtype and np.array_equal(out[k][0], G[pre + k]), k
  assert np.array_equal(out["vote_label_mask"][0], G[pre + "vote_label_mask"]) and out["vote_label_mask"].dtype == np.int64
  if not bool(G[pre + "augment"]):  # the reference applies nothing: every float is equal exactly
    for k in ("point_clouds", "center_label", "size_residual_label", "heading_residual_label", "vote_label"):
      assert np.array_equal(out[k][0], G[pre + k]), k
  if ds == "sunrgbd":
    bound = vote_bound(ds, G[pre + "point_clouds"], float(G[pre + "scale"]), out["vote_label"][0], G[pre + "vote_label"])
    assert (np.abs(out["vote_label"][0].astype(np.float64) - G[pre + "vote_label"].astype(np.float64)) <= bound).all(), \
        "votes beyond ulp(point) * scale + ulp(vote)"


@pytest.mark.parametrize("r", range(4))
def test_instance_votes_exact_on_reference_points(G, r):
  pre = "scannet_run%d_" % r
  _, out = run(G, "scannet", r, point_clouds=G[pre + "point_clouds"])
  want = G[pre + "vote_label"]
  assert out["vote_label"].dtype == np.float32 and want.dtype == np.float32
  assert np.array_equal(out["vote_label"][0], want), "votes differ (values; a zero's sign aside)"
  assert np.array_equal(out["vote_label_mask"][0], G[pre + "vote_label_mask"])
  assert 0 < out["vote_label_mask"].sum() < out["vote_label_mask"].size, "run %d has voted and unvoted rows" % r


@pytest.mark.parametrize("r", range(4))
@pytest.mark.parametrize("ds", ["scannet", "sunrgbd"])
def test_voxels_exact_on_reference_points(G, ds, r):
  pre = "%s_run%d_" % (ds, r)
  pc = G[pre + "point_clouds"]
  vs = float(G["voxel_size"])
  vc, vi, vf, counts, flags = dr.voxelize(pc[None], vs)
  assert not flags.any() and counts.tolist() == [len(vc)] * 2
  want_c, want_i = G[pre + "voxel_coords"], G[pre + "voxel_inds"]
  # the reference's row order is a hash-map walk's: compare as sets of (voxel, the point of the representative lies in it)
  assert sorted(map(tuple, vc[:, 1:])) == sorted(map(tuple, want_c)), "voxel sets differ"
  q = np.floor(pc / np.float32(vs)).astype(np.int32)
  assert np.array_equal(q[vi], vc[:, 1:]) and np.array_equal(q[want_i], want_c)
  assert len(vc) < len(pc), "no two points share a voxel: the case does not exercise the merge"
  # ours is the first row of every voxel: np.unique's return_index, in ascending order of that row
  _, first = np.unique(q, axis=0, return_index=True)
  assert np.array_equal(vi, np.sort(first)) and vi.dtype == np.int32 and vc.dtype == np.int32
  assert vf.shape == (len(vc), 3) and vf.dtype == np.float32 and (vf == 1).all()


@pytest.mark.parametrize("ds", ["scannet", "sunrgbd"])
def test_collated_batch(G, ds):
  """collate_fn over the three augmented runs: batch ids in scene order, the per-scene voxels concatenated."""
  pc = G[ds + "_batch_point_clouds"]
  vc, vi, vf, counts, flags = dr.voxelize(pc, float(G["voxel_size"]))
  want_c, want_i = G[ds + "_batch_voxel_coords"], G[ds + "_batch_voxel_inds"]
  assert not flags.any() and int(counts[-1]) == len(want_c) and G[ds + "_batch_voxel_feats"].shape == vf.shape
  assert np.array_equal(vc[:, 0], want_c[:, 0]), "scenes in order, the same number of voxels each"
  assert sorted(map(tuple, vc)) == sorted(map(tuple, want_c.astype(np.int32)))
  q = np.floor(pc / np.float32(float(G["voxel_size"]))).astype(np.int32)
  assert np.array_equal(q[want_c[:, 0], want_i], want_c[:, 1:]) and np.array_equal(q[vc[:, 0], vi], vc[:, 1:])
  assert (G[ds + "_batch_voxel_feats"] == 1).all()


def test_python_float_mod_rule():
  """angle2class leans on Python's float %: the result takes the divisor's sign."""
  two_pi = 2 * np.pi
  for a in (-2.5, 7.0, -1e-20, 0.0, -0.0, two_pi, -two_pi, 13.0, np.pi / 12):
    got, want = dr.py_mod(a, two_pi), a % two_pi
    assert got == want and np.signbit(got) == np.signbit(want), a
