"""The VoteNet detection head (csrc/detect.hip, pointcontrast_amd.downstream.votenet) on the MI355X against
tests/votenet_ref.py: index, count and mask outputs exactly, float outputs within 1e-4 of float64 relative to the tensor's
largest entry (the bound every kernel of this library is held to), backward passes bit-identical between two runs.  Where a
threshold decides (the loss's 0.3 / 0.6 cuts, a point on a box face, an overlap at nms_iou) the test first asserts on the
host that its inputs stay clear of the threshold by far more than float32 can move them."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_votenet as mk  # noqa: E402
import votenet_fixtures as VF  # noqa: E402
import votenet_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-4
G = np.load(mk.PATH)
KW = {"l2": {}, "l1": dict(l1=True), "huber": dict(l1smooth=True, delta=0.75)}
PCMI_ERR_INVALID, PCMI_ERR_UNSUPPORTED, PCMI_ERR_WORKSPACE = -1, -6, -7


def _dev(a, dtype=None):
  t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
  return t if dtype is None else t.to(dtype)


def _close(got, want, what, scale=None):
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  assert got.shape == want.shape, (what, got.shape, want.shape)
  if scale is None:
    scale = max(float(np.abs(want).max()) if want.size else 0.0, 1e-30)
  err = float(np.abs(got - want).max()) / scale if want.size else 0.0
  print("%s: max error %.3g of the largest entry" % (what, err))
  assert err <= TOL, "%s: %.3g > %g" % (what, err, TOL)


def _stream():
  return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _p(t):
  return None if t is None else C.c_void_p(t.data_ptr())


# ---- 1. nn_distance forward ---------------------------------------------------------------------------------------------------
FWD_SHAPES = [(1, 1, 1), (2, 63, 65), (2, 64, 64), (3, 65, 1), (2, 256, 64), (1, 1000, 1025), (8192, 1, 3), (8192, 3, 3), (5000, 3, 1)]
# the dispatch of nn_fwd_mode (flat kernel if M <= kSmallOther = 32 or B > 65535, else LDS tiles of kTile = 1024 points):
# B > 65535 with M > kSmallOther (the flat kernel walking a large other cloud), the kSmallOther edge, exactly one full kTile
FWD_SHAPES += [(65536, 1, 33), (65536, 2, 40), (3, 70, 32), (3, 70, 33), (2, 300, 1024)]


def _clouds(shape, seed):
  rng = np.random.RandomState(seed)
  B, N, M = shape
  return (rng.uniform(-2, 2, (B, N, 3)).astype(np.float32), rng.uniform(-2, 2, (B, M, 3)).astype(np.float32))


def _check_forward(p1, p2, mode, what):
  from pointcontrast_amd.downstream import votenet
  d1, i1, d2, i2 = votenet.nn_distance(_dev(p1), _dev(p2), **KW[mode])
  assert d1.dtype == torch.float32 and d2.dtype == torch.float32 and i1.dtype == torch.int64 and i2.dtype == torch.int64
  assert d1.shape == p1.shape[:2] and i1.shape == p1.shape[:2] and d2.shape == p2.shape[:2] and i2.shape == p2.shape[:2]
  assert not i1.requires_grad and not i2.requires_grad
  w1, wi1, w2, wi2 = R.nn_distance(torch.from_numpy(p1), torch.from_numpy(p2), **KW[mode])
  assert np.array_equal(i1.cpu().numpy(), wi1.numpy()), "%s: %d of idx1 differ" % (what, int((i1.cpu() != wi1).sum()))
  assert np.array_equal(i2.cpu().numpy(), wi2.numpy()), "%s: %d of idx2 differ" % (what, int((i2.cpu() != wi2).sum()))
  _close(d1.cpu().numpy(), w1.numpy(), what + " dist1")
  _close(d2.cpu().numpy(), w2.numpy(), what + " dist2")


@pytest.mark.parametrize("mode", R.MODES)
def test_nn_distance_forward(mode):
  for shape in FWD_SHAPES:
    p1, p2 = _clouds(shape, sum(shape))
    _check_forward(p1, p2, mode, "%s %s" % (mode, shape))


@pytest.mark.parametrize("mode", R.MODES)
def test_nn_distance_ties_and_identical_clouds(mode):
  from pointcontrast_amd.downstream import votenet
  rng = np.random.RandomState(3)
  base = rng.uniform(-2, 2, (2, 40, 3)).astype(np.float32)
  dup = np.concatenate([base, base], 1)  # every point of pc2 twice: the first copy wins
  p1 = rng.uniform(-2, 2, (2, 70, 3)).astype(np.float32)
  _check_forward(p1, dup, mode, mode + " duplicated")
  _, i1, _, _ = votenet.nn_distance(_dev(p1), _dev(dup), **KW[mode])
  assert int(i1.max()) < 40
  big = rng.uniform(-2, 2, (1, 1100, 3)).astype(np.float32)  # the LDS-tiled kernel, two tiles
  bigdup = np.concatenate([big, big], 1)
  _, i1, _, _ = votenet.nn_distance(_dev(big[:, :300]), _dev(bigdup), **KW[mode])
  assert int(i1.max()) < 1100
  t = _dev(base)
  d1, i1, d2, i2 = votenet.nn_distance(t, t, **KW[mode])  # pc1 is pc2
  assert float(d1.abs().max()) == 0.0 and float(d2.abs().max()) == 0.0
  ar = torch.arange(40, device=DEV).expand(2, 40)
  assert torch.equal(i1, ar) and torch.equal(i2, ar)


def test_nn_distance_refuses_other_shapes():
  from pointcontrast_amd.downstream import votenet
  with pytest.raises(ValueError):
    votenet.nn_distance(torch.zeros(1, 5, 4, device=DEV), torch.zeros(1, 6, 4, device=DEV))
  with pytest.raises(ValueError):
    votenet.nn_distance(torch.zeros(1, 0, 3, device=DEV), torch.zeros(1, 6, 3, device=DEV))
  with pytest.raises(ValueError):
    votenet.nn_distance(torch.zeros(1, 5, 3, device=DEV), torch.zeros(1, 0, 3, device=DEV))


# ---- 2. nn_distance backward --------------------------------------------------------------------------------------------------
# (1, 300, 7): many pc1 points share a nearest pc2 point; (1, 1100, 1030): both directions take the inverse lists (a cloud
# of more than 1024 points); (2, 65, 64): the LDS scan; (8192, 3, 3): the flat kernel
BWD_SHAPES = [(2, 65, 64), (8192, 3, 3), (1, 300, 7), (1, 1100, 1030)]
# the two directions in DIFFERENT forms of nn_bwd_dir (flat scan: other cloud <= kSmallOther = 32; LDS scan: <= kTile = 1024 and
# B <= 65535; else inverse lists, the second direction reusing the first one's workspace in stream order): small + lists,
# scan + lists, lists + scan, small + scan and scan + scan on the kSmallOther edge, lists forced by B > 65535 + small
BWD_SHAPES += [(2, 5, 1100), (1, 1024, 1025), (1, 1025, 1024), (3, 70, 32), (3, 70, 33), (65536, 1, 33)]


def _backward(p1, p2, g1, g2, mode):
  from pointcontrast_amd.downstream import votenet
  a, b = _dev(p1).requires_grad_(), _dev(p2).requires_grad_()
  d1, i1, d2, i2 = votenet.nn_distance(a, b, **KW[mode])
  torch.autograd.backward([d1, d2], [_dev(g1), _dev(g2)])
  return a.grad, b.grad, i1.cpu().numpy(), i2.cpu().numpy()


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", BWD_SHAPES)
def test_nn_distance_backward(shape, mode):
  rng = np.random.RandomState(7 + sum(shape))
  p1, p2 = _clouds(shape, 11 + sum(shape))
  B, N, M = shape
  g1, g2 = rng.normal(0, 1, (B, N)).astype(np.float32), rng.normal(0, 1, (B, M)).astype(np.float32)
  ga, gb, i1, i2 = _backward(p1, p2, g1, g2, mode)
  wi1, wi2 = R.nn_indices(p1, p2, mode, KW[mode].get("delta", 1.0))
  assert np.array_equal(i1, wi1) and np.array_equal(i2, wi2)
  a, b = torch.from_numpy(p1).double().requires_grad_(), torch.from_numpy(p2).double().requires_grad_()
  e1, e2 = R.nn_distance_at(a, b, wi1, wi2, mode, KW[mode].get("delta", 1.0))
  torch.autograd.backward([e1, e2], [torch.from_numpy(g1).double(), torch.from_numpy(g2).double()])
  _close(ga.cpu().numpy(), a.grad.numpy(), "%s %s grad_pc1" % (mode, shape))
  _close(gb.cpu().numpy(), b.grad.numpy(), "%s %s grad_pc2" % (mode, shape))
  ga2, gb2, _, _ = _backward(p1, p2, g1, g2, mode)
  assert torch.equal(ga, ga2) and torch.equal(gb, gb2), "two runs differ"
  # a zero grad_dist2: pc1's gradient is exactly its direct term
  ga0, _, _, _ = _backward(p1, p2, g1, np.zeros_like(g2), mode)
  a = torch.from_numpy(p1).double().requires_grad_()
  e1, _ = R.nn_distance_at(a, torch.from_numpy(p2).double(), wi1, wi2, mode, KW[mode].get("delta", 1.0))
  e1.backward(torch.from_numpy(g1).double())
  _close(ga0.cpu().numpy(), a.grad.numpy(), "%s %s direct term" % (mode, shape))
  from pointcontrast_amd.downstream import votenet
  a32, b32 = _dev(p1).requires_grad_(), _dev(p2)
  d1, _, _, _ = votenet.nn_distance(a32, b32, **KW[mode])
  d1.backward(_dev(g1))
  assert torch.equal(a32.grad, ga0), "the direct term is not exact"


# ---- 3. get_loss ----------------------------------------------------------------------------------------------------------------
LOSS_TERMS = ("vote_loss", "objectness_loss", "center_loss", "heading_cls_loss", "heading_reg_loss", "size_cls_loss", "size_reg_loss",
              "sem_cls_loss", "box_loss", "loss", "pos_ratio", "neg_ratio", "obj_acc")
LOSS_SEED = 0


def test_get_loss():
  from pointcontrast_amd.downstream import votenet
  ep, cfg = VF.loss_inputs(B=2, num_points=512, num_seed=128, K=32, K2=8, H=12, S=10, Cls=10, seed=LOSS_SEED)
  assert (ep["box_label_mask"] == 0).any() and (ep["vote_label_mask"] == 0).any()
  ep64 = VF.to_float64(ep, requires_grad=True)
  want = R.get_loss(ep64, cfg.num_heading_bin, cfg.mean_size_arr)
  eu = want["euclidean_dist1"].numpy()
  clear = np.minimum(np.abs(eu - R.NEAR_THRESHOLD), np.abs(eu - R.FAR_THRESHOLD)).min()
  assert clear >= 1e-3, "a proposal %.3g from a threshold: float32 could flip its label" % clear
  assert 0 < want["objectness_label"].sum() < want["objectness_label"].numel() and (want["objectness_mask"] == 0).any()
  want["loss"].backward()

  def on_device():
    d = {k: v.to(DEV) for k, v in ep.items()}
    for k in VF.PREDICTED:
      d[k].requires_grad_()
    return d

  votenet.get_loss(on_device(), cfg)  # the first call uploads the constants
  d = on_device()
  torch.cuda.synchronize()
  torch.cuda.set_sync_debug_mode("error")
  try:
    loss, out = votenet.get_loss(d, cfg)  # any device -> host copy or synchronisation raises
    loss.backward()
  finally:
    torch.cuda.set_sync_debug_mode("default")
  assert out is d and loss is out["loss"]
  assert out["objectness_label"].dtype == torch.int64 and out["object_assignment"].dtype == torch.int64
  assert np.array_equal(out["objectness_label"].cpu().numpy(), want["objectness_label"].numpy())
  assert np.array_equal(out["objectness_mask"].cpu().numpy(), want["objectness_mask"].numpy())
  assert np.array_equal(out["object_assignment"].cpu().numpy(), want["object_assignment"].numpy())
  for k in LOSS_TERMS:
    assert out[k].dim() == 0
    _close(out[k].detach().cpu().numpy(), want[k].detach().numpy(), k, scale=max(abs(float(want[k].detach())), 1e-30))
  for k in VF.PREDICTED:
    _close(d[k].grad.cpu().numpy(), ep64[k].grad.numpy(), "d loss / d " + k)


# ---- 4. decode --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heading", ["zero", "bins"])
@pytest.mark.parametrize("K", [1, 64, 257])
def test_box_decode(K, heading):
  from pointcontrast_amd import functional as PF
  rng = np.random.RandomState(K)
  B, H, S, Cls = 2, 12, 5, 7
  a = VF.prediction_inputs(rng, B, K, 8, H, S, Cls)
  msa = rng.uniform(0.4, 1.5, (S, 3)).astype(np.float32)
  a["heading_scores"][0, 0] = 0.0
  a["heading_scores"][0, 0, 7] = 5.0       # bin 7 of 12: 7 pi / 6 + residual wraps past pi
  a["size_scores"][1, K - 1] = 0.25        # a row of equal scores: index 0
  a["sem_cls_scores"][1, K - 1, 2:4] = 9.0  # two equal maxima: the lower index
  got = PF.box_decode(*[_dev(a[k]) for k in ("center", "heading_scores", "heading_residuals", "size_scores", "size_residuals",
                                             "sem_cls_scores", "objectness_scores")], _dev(msa), heading == "zero")
  want = R.box_decode(a["center"], a["heading_scores"], a["heading_residuals"], a["size_scores"], a["size_residuals"],
                      a["sem_cls_scores"], a["objectness_scores"], msa, heading == "zero")
  if heading == "bins":
    assert want["box_params"][0, 0, 6] < 0 and want["heading_class"][0, 0] == 7
  assert want["size_class"][1, K - 1] == 0 and want["sem_cls"][1, K - 1] == 2
  for k in ("heading_class", "size_class", "sem_cls"):
    assert got[k].dtype == torch.int32 and np.array_equal(got[k].cpu().numpy(), want[k]), k
  scale = float(np.abs(want["corners"]).max())
  _close(got["corners"].cpu().numpy(), want["corners"], "corners", scale)
  _close(got["minmax"].cpu().numpy(), want["minmax"], "minmax", scale)
  _close(got["box_params"][..., :6].cpu().numpy(), want["box_params"][..., :6], "centre and size", scale)
  dang = got["box_params"][..., 6].cpu().numpy().astype(np.float64) - want["box_params"][..., 6]
  assert np.abs(np.sin(dang / 2)).max() <= TOL  # the same angle modulo 2 pi
  _close(got["obj_prob"].cpu().numpy(), want["obj_prob"], "obj_prob")
  _close(got["sem_cls_probs"].cpu().numpy(), want["sem_cls_probs"], "sem_cls_probs")


# ---- 5. point counts ------------------------------------------------------------------------------------------------------------
def _count_case(N, K, seed):
  """(points [B, N, 4] float32, params [B, K, 7] float32), B = 2 (1 at the largest N): rotated boxes among the points; with
  room for them, box 0 holds no point, box 1 exactly 4 and box 2 exactly 5 (each far from everything else).  No point
  within 1e-3 of a face plane."""
  rng = np.random.RandomState(seed)
  B = 2 if N <= 4097 else 1
  params = np.stack([VF.clustered_params(rng, K, 4) for _ in range(B)]).astype(np.float32)
  pts = rng.uniform(-3.5, 3.5, (B, N, 3)).astype(np.float32)
  special = K >= 3 and N >= 9
  for b in range(B):
    if special:
      for k, at in ((0, 50.0), (1, 60.0), (2, 70.0)):
        params[b, k, 0:3] = at
      redraw = np.ones(9, bool)
      while redraw.any():  # the 4 + 5 points stay in their boxes and off every face plane
        for k, first, n in ((1, 0, 4), (2, 4, 5)):
          cam = params[b, k, 0:3] + rng.uniform(-0.1, 0.1, (n, 3))
          fresh = np.stack([cam[:, 0], cam[:, 2], -cam[:, 1]], -1).astype(np.float32)  # camera -> depth
          sel = redraw[first:first + n]
          pts[b, first:first + n][sel] = fresh[sel]
        redraw = R.points_near_faces(pts[b, :9], params[b], 2e-3)
    VF.clear_of_faces(pts[b, 9 if special else 0:], params[b], rng)
  return np.concatenate([pts, rng.rand(B, N, 1).astype(np.float32)], -1), params, special


@pytest.mark.parametrize("K", [1, 64, 257])
def test_box_point_counts(K):
  from pointcontrast_amd._lib import lib, check
  for N in (1, 63, 4097, 20000):
    pts, params, special = _count_case(N, K, 100 * K + N % 97)
    B = pts.shape[0]
    want, face = zip(*[R.box_point_counts(pts[b], params[b]) for b in range(B)])
    want = np.stack(want)
    assert min(f.min() for f in face) >= 1e-3, "a point within 1e-3 of a face"
    if special:
      assert (want[:, 0] == 0).all() and (want[:, 1] == 4).all() and (want[:, 2] == 5).all()
    counts = torch.full((B, K), -7, dtype=torch.int32, device=DEV)
    p, q = _dev(pts), _dev(params)
    check(lib.pcmi_box_point_counts(_p(p), 4, _p(q), B, N, K, _p(counts), _stream()))
    assert np.array_equal(counts.cpu().numpy(), want), "N %d K %d: %d counts differ" % (N, K, int((counts.cpu().numpy() != want).sum()))
    if N >= 4097:
      assert want.max() >= 5


# ---- 6. NMS -----------------------------------------------------------------------------------------------------------------------
NMS_IOU = 0.25
# seeds drawn on the host until every compared overlap is >= 1e-4 from NMS_IOU.  From 1023 boxes about a million overlaps are
# compared and random boxes always put one closer than that, so there the boxes are unit cubes on a lattice of step 0.35 in
# x and z around their cluster's centre: every overlap is one of a few known values, none within 0.01 of NMS_IOU.
# 257: the first K on the 1024-thread template (K <= 256 takes the 256-thread one), whose rows of suppression bits have 16
# words instead of 4; 1023: the last K below kNmsMaxK = 1024.
NMS_SEEDS = {1: 0, 2: 0, 64: 0, 65: 0, 256: 4, 257: 4, 1023: 0, 1024: 0}


def nms_case(K, seed):
  """Three scenes of K boxes in overlapping clusters: scene 0 with some empty boxes, scene 1 all empty, scene 2 with a
  zero-volume box.  Distinct scores.  (minmax [3, K, 6] f32, score [3, K] f32, cls [3, K] i32, counts [3, K] i32)."""
  rng = np.random.RandomState(1000 * seed + K)
  mm = np.zeros((3, K, 6), np.float32)
  for b in range(3):
    if K >= 1023:
      n_cl = K // 6
      cl = rng.randint(0, n_cl, K)
      c = np.stack([5.0 * (cl % 16) + 0.35 * rng.randint(0, 3, K), np.zeros(K), 5.0 * (cl // 16) + 0.35 * rng.randint(0, 3, K)], 1)
      p = np.concatenate([c, np.ones((K, 3))], 1)
    else:
      p = VF.clustered_params(rng, K, max(1, K // 6), rotated=False)
    mm[b] = np.concatenate([p[:, 0:3] - p[:, 3:6] / 2, p[:, 0:3] + p[:, 3:6] / 2], 1)
  mm[2, K // 2, 3:] = mm[2, K // 2, :3]
  score = np.stack([(rng.permutation(K) + 1.0) / (K + 1) for _ in range(3)]).astype(np.float32)
  cls = rng.randint(0, 3, (3, K)).astype(np.int32)
  counts = np.full((3, K), 10, np.int32)
  counts[0, rng.rand(K) < 0.2] = 4
  counts[1] = rng.randint(0, 5, K)
  return mm, score, cls, counts


def nms_expected(K, seed):
  mm, score, cls, counts = nms_case(K, seed)
  want, gap = {}, np.inf
  for mode in (0, 1, 2):
    for old in (0, 1):
      masks = []
      for b in range(3):
        m, g = R.nms(mm[b], score[b], cls[b], counts[b] >= 5, mode, bool(old), NMS_IOU)
        masks.append(m)
        gap = min(gap, g)
      want[(mode, old)] = np.stack(masks)
  return (mm, score, cls, counts), want, gap


@pytest.mark.parametrize("K", sorted(NMS_SEEDS))
def test_box_nms(K):
  from pointcontrast_amd._lib import lib, check
  (mm, score, cls, counts), want, gap = nms_expected(K, NMS_SEEDS[K])
  assert gap >= 1e-4, "an overlap %.3g from nms_iou: float32 could decide differently" % gap
  if K == 257:
    # scene 2 has no empty box, so its lowest-scored box holds rank 256: the first bit of the fifth word of the mask.  It is
    # suppressed -- by a kept box of a rank below 256, since nothing else precedes it -- so the word edge is crossed
    last = sorted(range(K), key=lambda i: (-float(score[2][i]), i))[-1]
    assert (counts[2] >= 5).all() and all(w[2][last] == 0 for w in want.values()), "no suppression crosses rank 256"
  dmm, dscore, dcls, dcounts = _dev(mm), _dev(score), _dev(cls), _dev(counts)
  for (mode, old), w in want.items():
    assert w[1].sum() == 0 and (K < 64 or 0 < w[0].sum() < (counts[0] >= 5).sum()), "the case must suppress some boxes"
    mask = torch.full((3, K), -7, dtype=torch.int32, device=DEV)
    check(lib.pcmi_box_nms(_p(dmm), _p(dscore), _p(dcls), _p(dcounts), 5, 3, K, mode, old, NMS_IOU, _p(mask), _stream()))
    assert np.array_equal(mask.cpu().numpy(), w), "K %d mode %d old %d: %d differ" % (K, mode, old, int((mask.cpu().numpy() != w).sum()))
  # without counts every box takes part
  mask = torch.empty((3, K), dtype=torch.int32, device=DEV)
  check(lib.pcmi_box_nms(_p(dmm), _p(dscore), None, None, 5, 3, K, 1, 0, NMS_IOU, _p(mask), _stream()))
  w = np.stack([R.nms(mm[b], score[b], cls[b], np.ones(K, bool), 1, False, NMS_IOU)[0] for b in range(3)])
  assert np.array_equal(mask.cpu().numpy(), w)


def test_box_nms_equal_scores_and_too_many_boxes():
  from pointcontrast_amd._lib import lib, check, PcmiError
  mm = _dev(np.array([[[0, 0, 0, 1, 1, 1], [0.1, 0, 0, 1.1, 1, 1]]], np.float32))
  score = _dev(np.array([[0.5, 0.5]], np.float32))
  for mode in (0, 1):
    mask = torch.empty((1, 2), dtype=torch.int32, device=DEV)
    check(lib.pcmi_box_nms(_p(mm), _p(score), None, None, 5, 1, 2, mode, 0, NMS_IOU, _p(mask), _stream()))
    assert mask.cpu().tolist() == [[1, 0]]  # the lower index is ranked first and suppresses the other
  K = 1025
  mm, score = torch.zeros((1, K, 6), device=DEV), torch.zeros((1, K), device=DEV)
  mask = torch.full((1, K), -7, dtype=torch.int32, device=DEV)
  rc = lib.pcmi_box_nms(_p(mm), _p(score), None, None, 5, 1, K, 1, 0, NMS_IOU, _p(mask), _stream())
  assert rc == PCMI_ERR_UNSUPPORTED
  with pytest.raises(PcmiError, match="1025 proposals"):
    check(rc)
  torch.cuda.synchronize()
  assert bool((mask == -7).all()), "a refused call wrote into its output"


# ---- 7. parse_predictions -------------------------------------------------------------------------------------------------------
PARSE_SEED = {"zero": 0, "bins": 0}


def parse_case(style, seed):
  rng = np.random.RandomState(seed + (17 if style == "bins" else 0))
  B, K, N, H, S, Cls = 2, 64, 4097, (12 if style == "bins" else 1), 6, 6
  a = VF.prediction_inputs(rng, B, K, N, H, S, Cls)
  msa = rng.uniform(0.5, 1.4, (S, 3)).astype(np.float32)
  dec = R.box_decode(a["center"], a["heading_scores"], a["heading_residuals"], a["size_scores"], a["size_residuals"],
                     a["sem_cls_scores"], a["objectness_scores"], msa, style == "zero")
  for b in range(B):
    VF.clear_of_faces(a["point_clouds"][b], dec["box_params"][b], rng)
  cfg = dict(dataset_config=VF.DatasetConfig(H, msa, Cls, style == "zero"), remove_empty_box=True, use_3d_nms=style == "zero",
             cls_nms=True, nms_iou=NMS_IOU, use_old_type_nms=False, conf_thresh=0.05, per_class_proposal=False)
  return a, msa, cfg


@pytest.mark.parametrize("per_class", [False, True])
@pytest.mark.parametrize("style", ["zero", "bins"])
def test_parse_predictions(style, per_class):
  from pointcontrast_amd.downstream import votenet
  a, msa, cfg = parse_case(style, PARSE_SEED[style])
  cfg["per_class_proposal"] = per_class
  want, wmask, stats = R.parse_predictions(a, msa, 6, style == "zero", True, votenet.nms_mode(cfg), False, NMS_IOU, 0.05, per_class)
  assert stats["min_face"] >= 1e-3 and stats["min_iou_gap"] >= 1e-4, stats
  assert all(0 < len(w) for w in want) and 0 < wmask.sum() < wmask.size
  ep = {k: _dev(v) for k, v in a.items()}
  got = votenet.parse_predictions(ep, cfg)  # the heading mode is probed from the dataset config
  assert got is ep["batch_pred_map_cls"] and len(got) == 2
  assert ep["pred_mask"].shape == (2, 64) and np.array_equal(ep["pred_mask"], wmask)
  for i in range(2):
    assert len(got[i]) == len(want[i])
    for (gc, gcorners, gscore), (wc, wcorners, wscore, j) in zip(got[i], want[i]):
      assert gc == wc and gcorners.shape == (8, 3)
      _close(gcorners, wcorners, "corners", scale=float(np.abs(wcorners).max()))
      assert abs(gscore - wscore) <= TOL
  ep2 = {k: _dev(v) for k, v in a.items()}
  votenet.parse_predictions(ep2, cfg, heading=style)  # the mode given instead of probed
  assert np.array_equal(ep2["pred_mask"], wmask)
  with pytest.raises(ValueError):
    votenet.parse_predictions(ep2, cfg, heading="other")


def test_parse_predictions_reproduces_the_reference_fixture_and_empty_scenes():
  from pointcontrast_amd.downstream import votenet
  a = {k[3:]: G[k] for k in G.files if k.startswith("pp_")}
  cfg = dict(dataset_config=VF.DatasetConfig(mk.NUM_HEADING_BIN, G["pp_mean_size_arr"], 4, False), remove_empty_box=False,
             use_3d_nms=True, cls_nms=False, nms_iou=mk.NMS_IOU, use_old_type_nms=False, conf_thresh=-1.0, per_class_proposal=False)
  ep = {k: _dev(a[k]) for k in ("center", "heading_scores", "heading_residuals", "size_scores", "size_residuals", "sem_cls_scores",
                                "objectness_scores")}
  got = votenet.parse_predictions(ep, cfg)
  assert np.array_equal(ep["pred_mask"], G["pp_pred_mask"])  # what the reference's nms_3d_faster kept
  kept = np.where(G["pp_pred_mask"][0] == 1)[0]
  assert len(got[0]) == len(kept)
  for (c, corners, score), j in zip(got[0], kept):
    _close(corners, G["pp_corners"][0, j], "corners", scale=float(np.abs(G["pp_corners"]).max()))  # get_3d_box's
    assert abs(score - G["pp_obj_prob"][0, j]) <= TOL and c == int(np.argmax(a["sem_cls_scores"][0, j]))
  # a scene without a single point keeps no box: an empty list where the reference asserts
  cfg["remove_empty_box"] = True
  ep["point_clouds"] = torch.full((1, 100, 3), 500.0, device=DEV)
  assert votenet.parse_predictions(ep, cfg) == [[]] and ep["pred_mask"].sum() == 0


# ---- 8. the C contract of the new entry points ------------------------------------------------------------------------------------
def test_c_contract_refusals_and_stream():
  from pointcontrast_amd._lib import lib, check
  st = _stream()
  B, N, M = 1, 1100, 1030
  p1, p2 = (_dev(x) for x in _clouds((B, N, M), 1))
  d1 = torch.full((B, N), -7.0, device=DEV)
  i1 = torch.full((B, N), -7, dtype=torch.int32, device=DEV)
  i2 = torch.zeros((B, M), dtype=torch.int32, device=DEV)
  g1, g2 = torch.ones((B, N), device=DEV), torch.ones((B, M), device=DEV)
  ga, gb = torch.full((B, N, 3), -7.0, device=DEV), torch.full((B, M, 3), -7.0, device=DEV)
  for args in ((None, _p(p2), B, N, M, 0, 1.0, _p(d1), _p(i1), st), (_p(p1), _p(p2), B, N, M, 0, 1.0, None, _p(i1), st),
               (_p(p1), _p(p2), B, N, M, 3, 1.0, _p(d1), _p(i1), st), (_p(p1), _p(p2), B, 0, M, 0, 1.0, _p(d1), _p(i1), st)):
    assert lib.pcmi_nn_distance_fwd(*args) == PCMI_ERR_INVALID and lib.pcmi_last_error()
  need = lib.pcmi_nn_distance_bwd_workspace_bytes(B, N, M)
  assert need > 0 and lib.pcmi_nn_distance_bwd_workspace_bytes(2, 65, 64) == 0
  ws = torch.empty(need, dtype=torch.uint8, device=DEV)
  i1.zero_()
  bwd = lambda w, nbytes, a=_p(p1): lib.pcmi_nn_distance_bwd(a, _p(p2), _p(i1), _p(i2), _p(g1), _p(g2), B, N, M, 0, 1.0, _p(ga), _p(gb),  # noqa: E731
                                                              w, nbytes, st)
  assert bwd(_p(ws), need - 1) == PCMI_ERR_WORKSPACE and bwd(None, 0) == PCMI_ERR_WORKSPACE
  assert bwd(_p(ws), need, None) == PCMI_ERR_INVALID
  torch.cuda.synchronize()
  assert bool((ga == -7).all()) and bool((gb == -7).all()) and bool((d1 == -7).all()), "a refused call wrote into an output"
  check(bwd(_p(ws), need))  # exactly the queried size
  counts = torch.full((1, 4), -7, dtype=torch.int32, device=DEV)
  params = torch.zeros((1, 4, 7), device=DEV)
  assert lib.pcmi_box_point_counts(None, 3, _p(params), 1, 10, 4, _p(counts), st) == PCMI_ERR_INVALID
  assert lib.pcmi_box_point_counts(_p(p1), 2, _p(params), 1, 10, 4, _p(counts), st) == PCMI_ERR_INVALID
  assert lib.pcmi_box_nms(None, _p(g1), None, None, 5, 1, 4, 1, 0, 0.25, _p(counts), st) == PCMI_ERR_INVALID
  assert lib.pcmi_box_nms(_p(params), _p(g1), None, None, 5, 1, 4, 2, 0, 0.25, _p(counts), st) == PCMI_ERR_INVALID  # mode 2 without classes
  nul = [None] * 8
  assert lib.pcmi_box_decode(*nul, 1, 4, 2, 2, 2, 0, *nul, st) == PCMI_ERR_INVALID
  torch.cuda.synchronize()
  assert bool((counts == -7).all())
  # a non-default stream is honoured: the work waits for what that stream holds, and the default stream does not
  side = torch.cuda.Stream(device=DEV)
  big = torch.empty(1 << 26, dtype=torch.float32, device=DEV)
  with torch.cuda.stream(side):
    for _ in range(16):
      big.fill_(1.0)  # keeps the side stream busy
    src = p1 + 3.0  # produced ON the side stream: visible only to work ordered behind it
    dist = torch.empty((B, N), device=DEV)
    idx = torch.empty((B, N), dtype=torch.int32, device=DEV)
    check(lib.pcmi_nn_distance_fwd(_p(src), _p(src), B, N, N, 0, 1.0, _p(dist), _p(idx), C.c_void_p(side.cuda_stream)))
    done = torch.cuda.Event()
    done.record(side)
  done.synchronize()
  assert float(dist.abs().max()) == 0.0 and torch.equal(idx[0].cpu(), torch.arange(N, dtype=torch.int32))
