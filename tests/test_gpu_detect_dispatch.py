"""The detection-path kernels (csrc/pointset.hip, csrc/detect.hip) at every edge of their dispatch and in the call forms of the
reference's modules.  tests/test_gpu_pointset.py and tests/test_gpu_votenet_head.py check the values; here every shape is
derived from a condition in the source -- the constant is named beside it -- so that each kernel form is launched at the
first and the last size it serves.  The rules are theirs: index, count and mask outputs exactly, float outputs within 1e-4 of
float64 relative to the tensor's largest entry, backward passes bit-identical between two runs."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pointset_ref as R  # noqa: E402
import votenet_fixtures as VF  # noqa: E402
import votenet_ref as V  # noqa: E402
from c_contract import Guarded, align256  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-4
PCMI_OK, PCMI_ERR_WORKSPACE = 0, -7
KW = {"l2": {}, "l1": dict(l1=True), "huber": dict(l1smooth=True, delta=0.75)}
MODE_CODE = {"l2": 0, "l1": 1, "huber": 2}

# the constants of the dispatch conditions, as the source has them (test_constants_are_the_sources pins them to it)
kFpsThreads = 1024                       # pointset.hip: points of the PPT = 1 tier; the tiers are 1 / 4 / 8 times this
kFpsRegCoordPoints = 8 * kFpsThreads     # pointset.hip: the largest cloud kept in registers; beyond: minima in the workspace
kSmallOther = 32                         # detect.hip: the other cloud is read straight from memory up to this size
kTile = 1024                             # detect.hip: the other cloud's indices are scanned from LDS up to this size
kGridY = 65535                           # the batch is the grid's y dimension in the tiled / scan kernels
kNmsMaxK = 1024                          # detect.hip: the 1024-thread NMS template serves 257 .. kNmsMaxK boxes
kCntThreads, kCntPointsPerThread = 256, 4  # detect.hip: points per workgroup of box_point_counts
CSRC = os.path.join(os.path.dirname(HERE), "pointcontrast_amd", "csrc")


def test_constants_are_the_sources():
  src = open(os.path.join(CSRC, "pointset.hip")).read() + open(os.path.join(CSRC, "detect.hip")).read()

  def const(name):
    return re.search(r"constexpr int %s = ([^;]+);" % name, src).group(1).strip()
  assert const("kFpsThreads") == str(kFpsThreads) and const("kFpsRegCoordPoints") == "8 * kFpsThreads"
  assert const("kSmallOther") == str(kSmallOther) and const("kNmsMaxK") == str(kNmsMaxK)
  assert set(re.findall(r"constexpr int kTile = (\d+);", src)) == {str(kTile)}
  assert const("kCntThreads") == str(kCntThreads) and const("kCntPointsPerThread") == str(kCntPointsPerThread)
  assert "PCMI_FPS_TIER(4, 0, kFpsThreads + 1, 4 * kFpsThreads)" in src and "if (K <= 256)" in src
  assert "M <= kSmallOther || B > 65535" in src and "M <= kTile && B <= 65535" in src


def _cloud(rng, n, scale=2.0):
  return ((rng.rand(n, 3).astype(np.float32) - 0.5) * scale + 1.5).astype(np.float32)  # outside the origin's 1e-3 ball


def _dev(a, dtype=None):
  t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
  return t if dtype is None else t.to(dtype)


def _p(t):
  return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
  return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _close(got, want, what):
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  assert got.shape == want.shape, (what, got.shape, want.shape)
  err = float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1e-30)
  print("%s: max error %.3g of the largest entry" % (what, err))
  assert err <= TOL, "%s: %.3g > %g" % (what, err, TOL)


def _twice(fn):
  a, b = fn(), fn()
  assert torch.equal(a, b), "two runs differ"
  return a


# ---- 1. furthest point sampling: the four tiers and their edges -----------------------------------------------------------------
# kFpsThreads / + 1: PPT 1 | PPT 4; 2500: inside PPT 4; 4 kFpsThreads: the last of PPT 4 (its last point per thread is in
# use); kFpsRegCoordPoints / + 1: PPT 8 | the global-minima form
FPS_EDGES = (kFpsThreads, kFpsThreads + 1, 2500, 4 * kFpsThreads, kFpsRegCoordPoints, kFpsRegCoordPoints + 1)


@pytest.mark.parametrize("n", FPS_EDGES)
def test_fps_dense_tier_edges(n):
  from pointcontrast_amd import pointnet2_utils as P
  rng = np.random.RandomState(n)
  xyz = np.stack([_cloud(rng, n), _cloud(rng, n)])
  m_big = n + 3 if n <= kFpsThreads + 1 else 1024  # more picks than points where that is cheap
  # tie_free: no pick with a positive running minimum shares it with another point, in the float32 the device computes in
  # (the reference is bit-exact, so any margin above equality is clear of rounding); a pick is a prefix of a longer one
  want = np.stack([R.fps(xyz[b], m_big, tie_free=True) for b in range(2)])
  for m in (1, 16, m_big):
    got = P.furthest_point_sample(_dev(xyz), m)
    assert got.dtype == torch.int32 and got.shape == (2, m)
    assert (got.cpu().numpy() == want[:, :m]).all(), "fps n=%d m=%d: %d picks differ" % (n, m, int((got.cpu().numpy() != want[:, :m]).sum()))
  if n >= 4 * kFpsThreads:
    assert want.max() >= n - n // 8  # the tail of the cloud (the last point of a thread) is picked from


# every point k times (n = 1025 k' inside PPT 4 and PPT 8, n = 8193 = 3 * 2731 in the global-minima form): every pick is a
# tie between the copies and the lowest index wins, so no pick leaves the first copy
@pytest.mark.parametrize("base,k", [(kFpsThreads + 1, 2), (kFpsThreads + 1, 5), ((kFpsRegCoordPoints + 1) // 3, 3)])
def test_fps_duplicated_cloud_in_every_tier(base, k):
  from pointcontrast_amd import pointnet2_utils as P
  n = base * k
  assert (kFpsThreads < n <= 4 * kFpsThreads, 4 * kFpsThreads < n <= kFpsRegCoordPoints, n == kFpsRegCoordPoints + 1)[(2, 5, 3).index(k)]
  rng = np.random.RandomState(100 + k)
  pts = np.tile(_cloud(rng, base), (k, 1))
  m = base + 40  # past the distinct points: all minima are zero, index 0
  got = P.furthest_point_sample(_dev(pts[None]), m).cpu().numpy()[0]
  want = R.fps(pts, m)
  assert (got == want).all(), "fps %d x %d: %d picks differ" % (base, k, int((got != want).sum()))
  assert want.max() < base and len(np.unique(want[:base])) == base and (want[base:] == 0).all()


# one launch over every tier edge at once, an empty cloud and a single point
SEG_SIZES = [kFpsThreads, kFpsThreads + 1, 4 * kFpsThreads, 0, kFpsRegCoordPoints, kFpsRegCoordPoints + 1, 1]
_SEG = {}


def _seg_case(with_rows):
  """(xyz, offs, rows, positions [7, 1024], rows of xyz [7, 1024]): computed once, never modified."""
  if with_rows not in _SEG:
    rng = np.random.RandomState(21)
    offs = np.concatenate([[0], np.cumsum(SEG_SIZES)]).astype(np.int32)
    xyz = _cloud(rng, int(offs[-1]))
    rows = rng.permutation(int(offs[-1])).astype(np.int32) if with_rows else None
    _SEG[with_rows] = (xyz, offs, rows) + R.fps_segments(xyz, offs, rows, 1024, tie_free=True)
  return _SEG[with_rows]


@pytest.mark.parametrize("with_rows", [False, True])
def test_fps_segments_tier_edges_and_bounds(with_rows):
  from pointcontrast_amd import functional as PF
  xyz, offs, rows, wpos, wrow = _seg_case(with_rows)
  N, big = len(xyz), SEG_SIZES.index(kFpsRegCoordPoints + 1)
  xyz_d, offs_d, rows_d = _dev(xyz), _dev(offs), (_dev(rows) if with_rows else None)

  def run(bound, m):
    return PF.furthest_point_sample_segments(xyz_d, _p(offs_d), _p(rows_d), len(SEG_SIZES), bound, m)
  for m in (1, 16, 1024):
    tight_pos, tight_row = run(max(SEG_SIZES), m)  # the tight bound: kFpsRegCoordPoints + 1
    assert (tight_pos.cpu().numpy() == wpos[:, :m]).all() and (tight_row.cpu().numpy() == wrow[:, :m]).all(), (with_rows, m)
    assert (tight_pos.cpu().numpy()[SEG_SIZES.index(0)] == -1).all()
    loose_pos, loose_row = run(N, m)  # a loose bound launches every tier
    assert torch.equal(loose_pos, tight_pos) and torch.equal(loose_row, tight_row)
    # a bound on the tier edge kFpsRegCoordPoints: the global-minima form is not launched, the cloud above the bound reads
    # as empty and every other cloud is what it was
    edge_pos, edge_row = run(kFpsRegCoordPoints, m)
    assert bool((edge_pos[big] == -1).all()) and bool((edge_row[big] == -1).all())
    keep = [i for i in range(len(SEG_SIZES)) if i != big]
    assert torch.equal(edge_pos[keep], tight_pos[keep]) and torch.equal(edge_row[keep], tight_row[keep])


@pytest.mark.parametrize("bound", [kFpsRegCoordPoints, kFpsRegCoordPoints + 1])
@pytest.mark.parametrize("with_rows", [False, True])
def test_fps_c_entry_with_exactly_the_queried_workspace(with_rows, bound):
  from pointcontrast_amd._lib import lib, check
  sizes = [kFpsThreads + 1, kFpsRegCoordPoints + 1, 0, 64]
  m, st = 24, _stream()
  rng = np.random.RandomState(31)
  offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
  N = int(offs[-1])
  xyz = _cloud(rng, N)
  rows = rng.permutation(N).astype(np.int32) if with_rows else None
  wpos, wrow = R.fps_segments(xyz, offs, rows, m, tie_free=True)
  if bound <= kFpsRegCoordPoints:  # the cloud beyond the caller's bound reads as empty
    wpos[1], wrow[1] = -1, -1
  need = lib.pcmi_fps_workspace_bytes(N, bound, int(with_rows))
  assert need == (align256(N * 12) if with_rows else 0) + (align256(N * 4) if bound > kFpsRegCoordPoints else 0)
  xyz_d, offs_d, rows_d = _dev(xyz), _dev(offs), (_dev(rows) if with_rows else None)
  out = torch.full((len(sizes), m), -7, dtype=torch.int32, device=DEV)
  out_rows = torch.full((len(sizes), m), -7, dtype=torch.int32, device=DEV)

  def call(ws, nbytes):
    return lib.pcmi_fps(_p(xyz_d), N, _p(rows_d), _p(offs_d), len(sizes), bound, m, _p(out), _p(out_rows), ws, C.c_size_t(nbytes), st)
  if need == 0:
    check(call(None, 0))  # nothing required: a null workspace is accepted
  else:
    g = Guarded(need)
    assert call(g.vp, need - 1) == PCMI_ERR_WORKSPACE and call(None, 0) == PCMI_ERR_WORKSPACE and call(None, need) == PCMI_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and bool((out_rows == -7).all()), "a refused call wrote into its output"
    check(call(g.vp, need))
    g.check("fps workspace")
  assert (out.cpu().numpy() == wpos).all() and (out_rows.cpu().numpy() == wrow).all()


# ---- 2. nn_distance: every form in both passes ------------------------------------------------------------------------------------
def _clouds(shape, seed):
  rng = np.random.RandomState(seed)
  B, N, M = shape
  return (rng.uniform(-2, 2, (B, N, 3)).astype(np.float32), rng.uniform(-2, 2, (B, M, 3)).astype(np.float32))


# the flat kernel keeps the lowest index of a tie at both of its conditions: M <= kSmallOther, and B > kGridY with M beyond it
@pytest.mark.parametrize("mode", V.MODES)
@pytest.mark.parametrize("shape", [(3, 70, kSmallOther), (kGridY + 1, 2, kSmallOther + 8)])
def test_nn_distance_flat_kernel_ties(shape, mode):
  from pointcontrast_amd.downstream import votenet
  B, N, M = shape
  p1, half = _clouds((B, N, M // 2), 5)
  dup = np.concatenate([half, half], 1)  # every point of pc2 twice: the first copy wins
  d1, i1, d2, i2 = votenet.nn_distance(_dev(p1), _dev(dup), **KW[mode])
  wi1, wi2 = V.nn_indices(p1, dup, mode, KW[mode].get("delta", 1.0))
  assert int(wi1.max()) < M // 2
  assert np.array_equal(i1.cpu().numpy(), wi1) and np.array_equal(i2.cpu().numpy(), wi2)


def _bwd_form(B, other):
  """The form nn_bwd_dir takes for a direction whose OTHER cloud has `other` points."""
  return "small" if other <= kSmallOther else ("scan" if other <= kTile and B <= kGridY else "lists")


# shape -> the forms of (gpc1's direction: the other cloud is pc2 with M points, gpc2's direction: N points)
NN_BWD_FORMS = {
    (2, 5, kTile + 76): ("lists", "small"),              # small + lists: the second direction needs no workspace
    (1, kTile, kTile + 1): ("lists", "scan"),            # scan + lists on the kTile edge
    (1, kTile + 1, kTile): ("scan", "lists"),            # lists + scan: the lists come second
    (3, 70, kSmallOther): ("small", "scan"),             # the kSmallOther edge
    (3, 70, kSmallOther + 1): ("scan", "scan"),
    (kGridY + 1, 1, kSmallOther + 1): ("lists", "small"),  # B beyond the grid forces the lists although M <= kTile
}


def _nn_grads64(p1, p2, i1, i2, g1, g2, mode):
  """float64 gradients for given argmins; an index outside its cloud drops its term."""
  delta = KW[mode].get("delta", 1.0)
  ok1, ok2 = (i1 >= 0) & (i1 < p2.shape[1]), (i2 >= 0) & (i2 < p1.shape[1])
  a, b = torch.from_numpy(p1).double().requires_grad_(), torch.from_numpy(p2).double().requires_grad_()
  e1, e2 = V.nn_distance_at(a, b, np.where(ok1, i1, 0), np.where(ok2, i2, 0), mode, delta)
  torch.autograd.backward([e1, e2], [torch.from_numpy(g1 * ok1).double(), torch.from_numpy(g2 * ok2).double()])
  return a.grad.numpy(), b.grad.numpy()


def _nn_bwd_c(p1, p2, i1, i2, g1, g2, mode, what, exact_ws=True):
  """pcmi_nn_distance_bwd through the C entry with a workspace of exactly the queried size between guard bands: one byte
  less is refused with the outputs untouched; the result is checked against float64, against the float32 restatement in
  the promised order (bit for bit) and against a second run."""
  from pointcontrast_amd._lib import lib, check
  B, N, M = p1.shape[0], p1.shape[1], p2.shape[1]
  delta, st = KW[mode].get("delta", 1.0), _stream()
  need = lib.pcmi_nn_distance_bwd_workspace_bytes(B, N, M)
  d = [_dev(x) for x in (p1, p2, i1.astype(np.int32), i2.astype(np.int32), g1, g2)]
  runs = []
  for _ in range(2):
    ga, gb = torch.full((B, N, 3), -7.0, device=DEV), torch.full((B, M, 3), -7.0, device=DEV)

    def call(ws, nbytes):
      return lib.pcmi_nn_distance_bwd(*[_p(x) for x in d], B, N, M, MODE_CODE[mode], delta, _p(ga), _p(gb), ws, C.c_size_t(nbytes), st)
    if need == 0:
      check(call(None, 0))
    else:
      g = Guarded(need)
      assert call(g.vp, need - 1) == PCMI_ERR_WORKSPACE and call(None, 0) == PCMI_ERR_WORKSPACE
      torch.cuda.synchronize()
      assert bool((ga == -7).all()) and bool((gb == -7).all()), "a refused call wrote into an output"
      check(call(g.vp, need))
      g.check(what)
    runs.append((ga, gb))
  # (asserted after the calls: a query that forgets a form's lists must already have surfaced above as PCMI_ERR_WORKSPACE)
  forms = (_bwd_form(B, M), _bwd_form(B, N))
  assert (need > 0) == ("lists" in forms), "%s: %d workspace bytes for the forms %s" % (what, need, forms)
  assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two runs differ"
  ga, gb = runs[0][0].cpu().numpy(), runs[0][1].cpu().numpy()
  wa, wb = _nn_grads64(p1, p2, i1, i2, g1, g2, mode)
  _close(ga, wa, what + " grad_pc1")
  _close(gb, wb, what + " grad_pc2")
  fa, fb = V.nn_backward_f32(p1, p2, i1, i2, g1, g2, mode, delta)
  assert np.array_equal(ga, fa), "%s: %d entries of grad_pc1 are not the sum in ascending index" % (what, int((ga != fa).sum()))
  assert np.array_equal(gb, fb), "%s: %d entries of grad_pc2 are not the sum in ascending index" % (what, int((gb != fb).sum()))


def _nn_fwd_c(p1, p2, mode):
  """(idx1, idx2) int64 numpy from the two pcmi_nn_distance_fwd launches."""
  from pointcontrast_amd._lib import lib, check
  B, N, M = p1.shape[0], p1.shape[1], p2.shape[1]
  a, b = _dev(p1), _dev(p2)
  out = []
  for x, y, n, m_ in ((a, b, N, M), (b, a, M, N)):
    dist, idx = torch.empty((B, n), device=DEV), torch.empty((B, n), dtype=torch.int32, device=DEV)
    check(lib.pcmi_nn_distance_fwd(_p(x), _p(y), B, n, m_, MODE_CODE[mode], KW[mode].get("delta", 1.0), _p(dist), _p(idx), _stream()))
    out.append(idx.cpu().numpy().astype(np.int64))
  return out


@pytest.mark.parametrize("mode", V.MODES)
@pytest.mark.parametrize("shape", sorted(NN_BWD_FORMS))
def test_nn_distance_backward_forms_through_the_c_entry(shape, mode):
  B, N, M = shape
  assert (_bwd_form(B, M), _bwd_form(B, N)) == NN_BWD_FORMS[shape]
  rng = np.random.RandomState(3 + sum(shape))
  p1, p2 = _clouds(shape, 17 + sum(shape))
  g1, g2 = rng.normal(0, 1, (B, N)).astype(np.float32), rng.normal(0, 1, (B, M)).astype(np.float32)
  i1, i2 = _nn_fwd_c(p1, p2, mode)
  wi1, wi2 = V.nn_indices(p1, p2, mode, KW[mode].get("delta", 1.0))
  assert np.array_equal(i1, wi1) and np.array_equal(i2, wi2)
  _nn_bwd_c(p1, p2, i1, i2, g1, g2, mode, "%s %s" % (mode, shape))


@pytest.mark.parametrize("mode", V.MODES)
def test_nn_distance_backward_long_lists(mode):
  """400 points of pc1 crowd around ONE point of pc2, both clouds beyond kTile: that point's inverse list is far longer than a
  wave (64), and the order of its sum is the promised one -- ascending index of the other cloud."""
  N, M = kTile + 476, kTile + 6
  assert (_bwd_form(1, M), _bwd_form(1, N)) == ("lists", "lists")
  rng = np.random.RandomState(41)
  p1, p2 = _clouds((1, N, M), 43)
  crowd = rng.choice(N, 400, replace=False)
  p1[0, crowd] = p2[0, 7] + rng.normal(0, 2e-3, (400, 3)).astype(np.float32)
  i1, i2 = V.nn_indices(p1, p2, mode, KW[mode].get("delta", 1.0))
  assert int((i1[0] == 7).sum()) >= 400 > 64
  g1, g2 = rng.normal(0, 1, (1, N)).astype(np.float32), rng.normal(0, 1, (1, M)).astype(np.float32)
  gi1, gi2 = _nn_fwd_c(p1, p2, mode)
  assert np.array_equal(gi1, i1) and np.array_equal(gi2, i2)
  _nn_bwd_c(p1, p2, i1, i2, g1, g2, mode, "%s crowded" % mode)
  # and through the wrapper, which hands the shared workspace over
  from pointcontrast_amd.downstream import votenet

  def run():
    a, b = _dev(p1).requires_grad_(), _dev(p2).requires_grad_()
    d1, _, d2, _ = votenet.nn_distance(a, b, **KW[mode])
    torch.autograd.backward([d1, d2], [_dev(g1), _dev(g2)])
    return torch.cat([a.grad, b.grad], 1)
  got = _twice(run).cpu().numpy()
  fa, fb = V.nn_backward_f32(p1, p2, i1, i2, g1, g2, mode, KW[mode].get("delta", 1.0))
  assert np.array_equal(got, np.concatenate([fa, fb], 1))


# An index outside its cloud.  Established by reading before this test was written: nn_bwd_small_kernel and nn_bwd_scan_kernel
# dereference idx_a only behind `t >= 0 && t < M` and only COMPARE the other cloud's indices with the row number;
# nn_bwd_lists_kernel guards idx_a the same way and reads the other cloud's indices through inverse_lists, whose
# scatter_keys_kernel sends an index outside [0, N) to the dump key B N (counted in the slot count[B N] that the workspace
# holds, sorted behind every real key, beyond start[B N] and so never read).  So the contract is the one include/pcmi.h
# states: the term is dropped, everything else is the reference gradient.  One shape per form that idx1 / idx2 pass through:
# shape -> forms of (gpc1's direction: scans idx2, gpc2's direction: scans idx1)
NN_RANGE_FORMS = {(4, 20, 50): ("scan", "small"), (2, 70, 40): ("scan", "scan"), (1, kTile + 76, 40): ("scan", "lists"),
                  (1, 40, kTile + 76): ("lists", "scan")}


@pytest.mark.parametrize("mode", V.MODES)
@pytest.mark.parametrize("shape", sorted(NN_RANGE_FORMS))
def test_nn_distance_backward_drops_an_index_outside_its_cloud(shape, mode):
  B, N, M = shape
  assert (_bwd_form(B, M), _bwd_form(B, N)) == NN_RANGE_FORMS[shape]
  rng = np.random.RandomState(sum(shape))
  p1, p2 = _clouds(shape, 23 + sum(shape))
  g1, g2 = rng.normal(0, 1, (B, N)).astype(np.float32), rng.normal(0, 1, (B, M)).astype(np.float32)
  i1, i2 = V.nn_indices(p1, p2, mode, KW[mode].get("delta", 1.0))
  f1, f2 = i1.reshape(-1), i2.reshape(-1)  # views: a handful of entries of each, below and above the range
  bad1, bad2 = rng.choice(B * N, 6, replace=False), rng.choice(B * M, 6, replace=False)
  f1[bad1[:3]], f1[bad1[3:]], f2[bad2[:3]], f2[bad2[3:]] = -1, M, -1, N
  wa, wb = _nn_grads64(p1, p2, i1, i2, g1, g2, mode)
  clean = _nn_grads64(p1, p2, *V.nn_indices(p1, p2, mode, KW[mode].get("delta", 1.0)), g1, g2, mode)
  assert np.abs(wa - clean[0]).max() > 0 and np.abs(wb - clean[1]).max() > 0  # the dropped terms are visible
  _nn_bwd_c(p1, p2, i1, i2, g1, g2, mode, "%s %s out of range" % (mode, shape))


# ---- 3. point counts on the edges of a workgroup's points ------------------------------------------------------------------------
_CNT = {}


def _count_case(N):
  """(points [2, N, 3], params [2, 64, 7], counts [2, 64]); no point within 1e-3 of a face plane (asserted)."""
  if N not in _CNT:
    rng = np.random.RandomState(N)
    params = np.stack([VF.clustered_params(rng, 64, 4) for _ in range(2)]).astype(np.float32)
    pts = rng.uniform(-3.5, 3.5, (2, N, 3)).astype(np.float32)
    for b in range(2):
      VF.clear_of_faces(pts[b], params[b], rng)
    want, face = zip(*[V.box_point_counts(pts[b], params[b]) for b in range(2)])
    assert min(f.min() for f in face) >= 1e-3, "a point within 1e-3 of a face"
    _CNT[N] = (pts, params, np.stack(want))
  return _CNT[N]


P_CNT = kCntThreads * kCntPointsPerThread  # the points of one workgroup


@pytest.mark.parametrize("point_ld", [3, 4, 7])
@pytest.mark.parametrize("N", [P_CNT - 1, P_CNT, P_CNT + 1, 2 * P_CNT])
def test_box_point_counts_block_edges_and_row_strides(N, point_ld):
  from pointcontrast_amd._lib import lib, check
  pts, params, want = _count_case(N)
  assert want.max() >= 5 and (want == 0).any()
  wide = np.full((2, N, point_ld), np.nan, np.float32)  # columns beyond the third are not coordinates
  wide[..., :3] = pts
  counts = torch.full((2, 64), -7, dtype=torch.int32, device=DEV)
  p, q = _dev(wide), _dev(params)
  check(lib.pcmi_box_point_counts(_p(p), point_ld, _p(q), 2, N, 64, _p(counts), _stream()))
  assert np.array_equal(counts.cpu().numpy(), want), "N %d ld %d: %d counts differ" % (N, point_ld, int((counts.cpu().numpy() != want).sum()))


# ---- 4. scatter-form backward passes at their extremes --------------------------------------------------------------------------
def _scatter_c(kind, gout, idx, weight, B, Cc, N, prefill=7.0):
  """The backward C entry of gather / group / interpolate with exactly the queried workspace into a pre-filled gradient."""
  from pointcontrast_amd._lib import lib, check
  L = idx.numel() // B if idx is not None else 0
  need = lib.pcmi_pointset_scatter_workspace_bytes(B * L, B * N)
  g = Guarded(need)
  gin = torch.full((B, Cc, N), prefill, device=DEV)
  st = _stream()
  if kind == "gather":
    rc = lib.pcmi_gather_points_bwd(_p(gout), _p(idx), B, Cc, N, L, _p(gin), 0, g.vp, g.size, st)
  elif kind == "group":
    rc = lib.pcmi_group_points_bwd(_p(gout), _p(idx), B, Cc, N, L // 3 if L else 0, 3, _p(gin), 0, g.vp, g.size, st)
  else:
    rc = lib.pcmi_three_interpolate_bwd(_p(gout), _p(idx), _p(weight), B, Cc, N, L // 3, _p(gin), 0, g.vp, g.size, st)
  check(rc)
  g.check(kind + " bwd workspace")
  return gin


def _scatter_want(kind, idx, weight, feat, gout):
  if kind == "gather":
    return R.grad_of(lambda x: R.gather(x, idx.cpu()), feat, gout)
  if kind == "group":
    return R.grad_of(lambda x: R.group(x, idx.cpu()), feat, gout)
  return R.grad_of(lambda x: R.interpolate(x, idx.cpu(), weight.double().cpu()), feat, gout)


# (C, N, n): the index tensor is [B, n, 3] for all three ops (gather reads it as [B, 3 n], grouping as np = n, ns = 3).
# (1, 3, 16667): 50,001 indices on three targets, three very long lists on one channel;
# (5, 20000, 13): 39 indices on 20,000 targets, almost every list empty
@pytest.mark.parametrize("kind", ["gather", "group", "interpolate"])
@pytest.mark.parametrize("Cc,N,n", [(1, 3, 16667), (5, 20000, 13)])
def test_scatter_backward_extremes(Cc, N, n, kind):
  from pointcontrast_amd import pointnet2_utils as P
  B = 2
  rng = np.random.RandomState(Cc + N + n)
  idx = _dev(rng.randint(0, N, (B, n, 3)).astype(np.int32))
  w = _dev(rng.rand(B, n, 3).astype(np.float32))
  feat = _dev(rng.randn(B, Cc, N).astype(np.float32))
  shape = {"gather": (B, Cc, 3 * n), "group": (B, Cc, n, 3), "interpolate": (B, Cc, n)}[kind]
  gout = _dev(rng.randn(*shape).astype(np.float32))
  use = idx.reshape(B, 3 * n) if kind == "gather" else idx
  want = _scatter_want(kind, use, w, feat, gout)
  got = _twice(lambda: _scatter_c(kind, gout, use, w, B, Cc, N))
  e = R.rel_err(got, want)
  print("%s bwd C %d N %d n %d: rel err %.3e" % (kind, Cc, N, n, e))
  assert e <= TOL
  hit = torch.zeros(B, N, dtype=torch.bool)
  hit[torch.arange(B)[:, None], idx.reshape(B, -1).long().cpu()] = True
  untouched = got.cpu()[~hit[:, None, :].expand(B, Cc, N)]
  assert (untouched.numel() > 0) == (N > 3 * n) and bool((untouched == 0.0).all()), "a target without sources is not exactly 0.0"
  # the autograd wrapper gives the same bits
  f = feat.clone().requires_grad_(True)
  fwd = {"gather": lambda: P.gather_operation(f, use), "group": lambda: P.grouping_operation(f, use),
         "interpolate": lambda: P.three_interpolate(f, use, w)}[kind]
  assert torch.equal(_twice(lambda: torch.autograd.grad(fwd(), f, gout)[0]), got)


@pytest.mark.parametrize("kind", ["gather", "group", "interpolate"])
def test_scatter_backward_without_indices(kind):
  """L == 0: null gout / idx / weight are not touched, PCMI_OK, the gradient is written whole as zeros."""
  got = _scatter_c(kind, None, None, None, 2, 5, 300)
  assert got.shape == (2, 5, 300) and bool((got == 0.0).all())


def test_scatter_backward_single_target():
  """The index sets "same" and "random" of test_interpolate_forward_and_all_backwards at B = 1 with N = 1: every index is 0."""
  from pointcontrast_amd import pointnet2_utils as P
  rng = np.random.RandomState(9)
  B, Cc, N = 1, 13, 1
  feat = _dev(rng.randn(B, Cc, N).astype(np.float32))
  for name, idx in (("same", np.full((B, 40, 16), 0, np.int32)), ("random", rng.randint(0, N, (B, 40, 16)).astype(np.int32))):
    it = _dev(idx)
    f = feat.clone().requires_grad_(True)
    gout = _dev(rng.randn(B, Cc, 40, 16).astype(np.float32))
    got = _twice(lambda: torch.autograd.grad(P.grouping_operation(f, it), f, gout)[0])
    assert R.rel_err(got, R.grad_of(lambda x: R.group(x, it.cpu()), feat, gout)) <= TOL, name
    flat, gflat = it.reshape(B, -1), gout.reshape(B, Cc, -1)
    got = _twice(lambda: torch.autograd.grad(P.gather_operation(f, flat), f, gflat)[0])
    assert R.rel_err(got, R.grad_of(lambda x: R.gather(x, flat.cpu()), feat, gflat)) <= TOL, name
    i3 = it.reshape(B, -1)[:, :213].reshape(B, 71, 3).contiguous()
    w = _dev(rng.rand(B, 71, 3).astype(np.float32))
    g3 = _dev(rng.randn(B, Cc, 71).astype(np.float32))
    out = _twice(lambda: P.three_interpolate(feat, i3, w))
    assert R.rel_err(out, R.interpolate(feat.double().cpu(), i3.cpu(), w.double().cpu())) <= TOL, name
    got = _twice(lambda: torch.autograd.grad(P.three_interpolate(f, i3, w), f, g3)[0])
    assert R.rel_err(got, R.grad_of(lambda x: R.interpolate(x, i3.cpu(), w.double().cpu()), feat, g3)) <= TOL, name


# ---- 5. the wrappers in the reference's call forms ---------------------------------------------------------------------------------
# Every call is made once with plain contiguous float32 / int32 tensors and then with the same VALUES presented the way the
# reference's modules present them.  A wrapper that forgot one .contiguous() or one dtype conversion reads other memory.
def _as_transposed(t):
  """The same values as a non-contiguous view: the last two dimensions swapped in memory."""
  if t.dim() < 2 or t.shape[-1] == 1 or t.shape[-2] == 1:
    return _as_sliced(t)  # a transpose of a one-wide dimension is still contiguous
  v = t.transpose(-1, -2).contiguous().transpose(-1, -2)
  assert not v.is_contiguous()
  return v


def _as_sliced(t):
  """Every other row (of dimension 0 for a matrix, else 1) of a tensor twice as long whose other rows hold garbage."""
  d = 0 if t.dim() <= 2 else 1
  shape = list(t.shape)
  shape[d] *= 2
  big = torch.full(shape, float("nan") if t.is_floating_point() else 2 ** 30, dtype=t.dtype, device=t.device)
  sl = [slice(None)] * t.dim()
  sl[d] = slice(0, None, 2)
  big[tuple(sl)] = t
  v = big[tuple(sl)]
  assert not v.is_contiguous() or t.shape[d] == 1
  return v


def _as_other_dtype(t):
  return t.double() if t.is_floating_point() else t.long()


def _as_expanded(t):
  """An upstream gradient whose last dimension has stride 0 (what .sum() / .mean() send back); its values differ from t's."""
  return t[..., :1].expand(t.shape)


FORMS = {"transposed": _as_transposed, "sliced": _as_sliced, "float64 / int64": _as_other_dtype}
GRAD_FORMS = {"transposed": _as_transposed, "sliced": _as_sliced, "expanded": _as_expanded}


def _wrapper_calls():
  """name -> (inputs: dict of plain device tensors, fn(**inputs) -> tuple of outputs, names of the differentiable inputs)."""
  from pointcontrast_amd import functional as PF, pointnet2_utils as P
  from pointcontrast_amd.downstream import votenet
  rng = np.random.RandomState(77)
  B, N, Cc, npnt, ns = 2, 300, 6, 24, 8
  f = lambda *s: _dev(rng.rand(*s).astype(np.float32))  # noqa: E731
  xyz, new_xyz, feats = f(B, N, 3), f(B, npnt, 3), _dev(rng.randn(B, Cc, N).astype(np.float32))
  i2 = _dev(rng.randint(0, N, (B, npnt)).astype(np.int32))
  i3 = _dev(rng.randint(0, N, (B, npnt, ns)).astype(np.int32))
  it = _dev(rng.randint(0, N, (B, 50, 3)).astype(np.int32))
  a = VF.prediction_inputs(rng, B, 20, 8, 12, 5, 7)
  dec = {k: _dev(a[k]) for k in ("center", "heading_scores", "heading_residuals", "size_scores", "size_residuals", "sem_cls_scores",
                                 "objectness_scores")}
  dec["mean_size_arr"] = _dev(rng.uniform(0.4, 1.5, (5, 3)).astype(np.float32))
  tup = lambda fn: (lambda **kw: tuple(fn(**kw)))  # noqa: E731
  one = lambda fn: (lambda **kw: (fn(**kw),))  # noqa: E731
  keys = ("heading_class", "size_class", "sem_cls", "box_params", "corners", "minmax", "obj_prob", "sem_cls_probs")
  return {
      "furthest_point_sample": (dict(xyz=xyz), one(lambda xyz: P.furthest_point_sample(xyz, 40)), ()),
      "ball_query": (dict(xyz=xyz, new_xyz=new_xyz), one(lambda xyz, new_xyz: P.ball_query(0.2, ns, xyz, new_xyz)), ()),
      "three_nn": (dict(unknown=xyz, known=new_xyz), tup(lambda unknown, known: P.three_nn(unknown, known)), ()),
      "gather_operation": (dict(features=feats, idx=i2), one(lambda features, idx: P.gather_operation(features, idx)), ("features",)),
      "grouping_operation": (dict(features=feats, idx=i3), one(lambda features, idx: P.grouping_operation(features, idx)), ("features",)),
      "three_interpolate": (dict(features=feats, idx=it, weight=f(B, 50, 3)),
                            one(lambda features, idx, weight: P.three_interpolate(features, idx, weight)), ("features",)),
      "QueryAndGroup": (dict(xyz=xyz, new_xyz=new_xyz, features=feats),
                        tup(lambda xyz, new_xyz, features: P.QueryAndGroup(0.2, ns, use_xyz=True, ret_grouped_xyz=True)(xyz, new_xyz, features)),
                        ("features",)),
      "GroupAll": (dict(xyz=xyz, new_xyz=new_xyz, features=feats),
                   one(lambda xyz, new_xyz, features: P.GroupAll(use_xyz=True)(xyz, new_xyz, features)), ("features",)),
      "nn_distance": (dict(pc1=xyz, pc2=new_xyz), tup(lambda pc1, pc2: votenet.nn_distance(pc1, pc2, l1smooth=True, delta=0.75)),
                      ("pc1", "pc2")),
      "box_decode": (dec, lambda **kw: tuple(PF.box_decode(zero_heading=False, **kw)[k] for k in keys), ()),
  }


def _run(fn, inputs, diff, gouts=None):
  """(outputs, gradients of the differentiable inputs); gouts: one upstream gradient per output, used for the outputs that
  depend on a differentiable input."""
  ins = {k: (v.detach().requires_grad_() if k in diff else v) for k, v in inputs.items()}
  outs = fn(**ins)
  grads = ()
  if diff:
    pairs = [(o, g) for o, g in zip(outs, gouts) if o.requires_grad]
    assert pairs, "no output depends on %s" % (diff,)
    grads = torch.autograd.grad([o for o, _ in pairs], [ins[k] for k in diff], [g for _, g in pairs])
  return tuple(o.detach() for o in outs), tuple(g.float() for g in grads)


def _same(a, b):
  """torch.equal over tuples, a float64 result compared as the float32 it was computed in."""
  return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def _bits(t):
  return t.detach().clone()


def _unchanged(before, after):
  return before.dtype == after.dtype and torch.equal(torch.nan_to_num(before.double(), nan=-12345.0), torch.nan_to_num(after.double(), nan=-12345.0))


WRAPPERS = ("furthest_point_sample", "ball_query", "three_nn", "gather_operation", "grouping_operation", "three_interpolate",
            "QueryAndGroup", "GroupAll", "nn_distance", "box_decode")


@pytest.mark.parametrize("name", WRAPPERS)
def test_wrappers_accept_the_reference_call_forms(name):
  inputs, fn, diff = _wrapper_calls()[name]
  rng = np.random.RandomState(len(name))
  probe, _ = _run(fn, inputs, ())
  gouts = [_dev(rng.randn(*o.shape).astype(np.float32)) if o.is_floating_point() else None for o in probe] if diff else None
  plain_out, plain_grad = _run(fn, inputs, diff, gouts)
  assert all(o.dtype in (torch.float32, torch.int32, torch.int64) for o in plain_out)
  for form, make in FORMS.items():
    for which in list(inputs) + ["all"]:  # one input at a time, then all of them together
      ins = {k: (make(v) if which in (k, "all") else v) for k, v in inputs.items()}
      kept = {k: _bits(v) for k, v in ins.items()}
      out, grad = _run(fn, ins, diff, gouts)
      assert _same(tuple(o.float() if o.dtype == torch.float64 else o for o in out), plain_out), (name, form, which)
      assert _same(grad, plain_grad), (name, form, which, "gradient")
      assert all(_unchanged(kept[k], ins[k]) for k in ins), (name, form, which, "an input was modified")
  if diff:
    for form, make in GRAD_FORMS.items():
      g2 = [None if g is None else make(g) for g in gouts]
      kept = [None if g is None else _bits(g) for g in g2]
      _, want = _run(fn, inputs, diff, [None if g is None else g.contiguous() for g in g2])
      _, got = _run(fn, inputs, diff, g2)
      assert _same(got, want), (name, form, "upstream gradient")
      assert all(a is None or _unchanged(a, b) for a, b in zip(kept, g2)), (name, form, "the upstream gradient was modified")


def test_wrappers_on_a_side_stream():
  """The same calls under a non-default stream on inputs produced ON that stream (visible only to work ordered behind it)."""
  calls = _wrapper_calls()
  plain = {}
  gouts = {}
  for name, (inputs, fn, diff) in calls.items():
    probe, _ = _run(fn, inputs, ())
    gouts[name] = [torch.ones_like(o) * 0.5 if o.is_floating_point() else None for o in probe] if diff else None
    plain[name] = _run(fn, inputs, diff, gouts[name])
  torch.cuda.synchronize()
  side = torch.cuda.Stream(device=DEV)
  big = torch.empty(1 << 26, dtype=torch.float32, device=DEV)
  got = {}
  with torch.cuda.stream(side):
    for _ in range(16):
      big.fill_(1.0)  # keeps the side stream busy
    for name, (inputs, fn, diff) in calls.items():
      ins = {k: ((v + 1) - 1 if not v.is_floating_point() else (v * 2.0) * 0.5) for k, v in inputs.items()}  # exact, and made here
      g = [None if x is None else x * 1.0 for x in gouts[name]] if diff else None
      got[name] = _run(fn, ins, diff, g)
    done = torch.cuda.Event()
    done.record(side)
  done.synchronize()
  for name in calls:
    assert _same(got[name][0], plain[name][0]), (name, "outputs")
    assert _same(got[name][1], plain[name][1]), (name, "gradients")
