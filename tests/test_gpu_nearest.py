"""The evaluation on the original point cloud (csrc/nearest.hip: pcmi_voxel_centers, pcmi_nearest_point, pcmi_seg_hist;
downstream.semseg.PointCloudEvaluator, SegmentationTrainer.test_original_pointcloud) against tests/nearest_ref.py, which
tests/test_nearest_ref.py holds to the reference's procedure.  The arithmetic is fixed, so every comparison is BIT-exact:
idx, dist2 (as int64 bit patterns, so NaN and +inf count), centers, hist, point_pred."""
import ctypes as C

import numpy as np
import pytest
import torch

import nearest_ref as nr
from c_contract import DEV, Guarded, PCMI_ERR_INVALID, PCMI_ERR_WORKSPACE, PCMI_OK

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def PF():
  from pointcontrast_amd import functional as pf
  return pf


def _dev(a, dtype=None):
  t = torch.from_numpy(np.ascontiguousarray(a))
  return (t if dtype is None else t.to(dtype)).to(DEV)


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def run(PF, ref, roffs, query, qoffs, cell):
  fb = torch.zeros(1, dtype=torch.int64, device=DEV)
  idx, d2 = PF.nearest_point(_dev(np.asarray(ref, np.float64).reshape(-1, 3)), _dev(np.asarray(roffs, np.int64)),
                             _dev(np.asarray(query, np.float64).reshape(-1, 3)), _dev(np.asarray(qoffs, np.int64)), cell=cell,
                             return_dist2=True, fallback_count=fb)
  return idx.cpu().numpy(), d2.cpu().numpy(), int(fb.cpu())


def check_exact(PF, ref, roffs, query, qoffs, cells, what):
  """Every cell size gives the restatement's idx and dist2 bit for bit; returns (idx, dist2, fallback counts)."""
  want_idx, want_d2 = nr.nearest_point(ref, roffs, query, qoffs)
  fbs = []
  for cell in cells:
    idx, d2, fb = run(PF, ref, roffs, query, qoffs, cell)
    bad = np.flatnonzero(idx != want_idx)
    assert len(bad) == 0, "%s, cell %r: %d of %d indices differ, first query %d: got %d want %d" % (
        what, cell, len(bad), len(idx), bad[0], idx[bad[0]], want_idx[bad[0]])
    assert np.array_equal(_bits(d2), _bits(want_d2)), "%s, cell %r: dist2 differs" % (what, cell)
    fbs.append(fb)
  return want_idx, want_d2, fbs


# ---- degenerate inputs ------------------------------------------------------------------------------------------------------
def test_single_row_and_empty_segment(PF):
  idx, d2, _ = check_exact(PF, [[0.1, 0.2, 0.3]], [0, 1], [[1.1, 0.2, 0.3]], [0, 1], [0.04, None], "m = n = 1")
  assert idx.tolist() == [0] and d2[0] == 1.0
  idx, d2, _ = check_exact(PF, np.zeros((0, 3)), [0, 0], [[1.0, 2.0, 3.0]] * 3, [0, 3], [0.04, None], "no references")
  assert idx.tolist() == [-1] * 3 and np.isposinf(d2).all()
  # a query row that belongs to no scene: as a scene without references
  idx, d2, _ = check_exact(PF, [[0.0, 0, 0]], [0, 1], [[0.0, 0, 0]] * 3, [1, 2], [0.04], "rows outside the offsets")
  assert idx.tolist() == [-1, 0, -1]


def test_no_queries_leaves_the_outputs_untouched(PF):
  from pointcontrast_amd._lib import lib
  ref, offs = _dev(np.zeros((4, 3))), _dev(np.array([0, 4], np.int64))
  qoffs = _dev(np.array([0, 0], np.int64))
  idx, d2 = Guarded(64), Guarded(64)
  ws = Guarded(lib.pcmi_nearest_point_workspace_bytes(4, 0, 1))
  st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
  rc = lib.pcmi_nearest_point(C.c_void_p(ref.data_ptr()), C.c_void_p(offs.data_ptr()), 4, None, C.c_void_p(qoffs.data_ptr()), 0, 1, 0.04,
                              None, idx.vp, d2.vp, None, ws.vp, ws.size, st)
  assert rc == PCMI_OK
  torch.cuda.synchronize()
  for g in (idx, d2, ws):
    assert bool((g.buf == 0xA5).all()), "n == 0 must enqueue nothing"
  out = PF.seg_hist(_dev(np.zeros(3, np.int32)), None, _dev(np.zeros(0, np.int32)), 5)
  assert int(out["hist"].sum()) == 0 and int(out["missing"]) == 0 and out["point_pred"].numel() == 0


# ---- the lattice: three cell sizes, identical outputs -----------------------------------------------------------------------
def test_lattice_three_cell_sizes(PF):
  coords, T, query = nr.lattice_case()
  inv = np.linalg.inv(T.reshape(4, 4)).reshape(1, 16)
  want_centers = nr.voxel_centers(coords, inv)
  centers = PF.voxel_centers(_dev(coords), torch.from_numpy(T)).cpu().numpy()
  assert np.array_equal(_bits(centers), _bits(want_centers)), "voxel_centers differs from ((X m0 + Y m1) + Z m2) + m3"
  m, n = len(centers), len(query)
  assert n == 2049  # a workgroup multiple plus one
  v = nr.VOXEL
  _, _, fbs = check_exact(PF, centers, [0, m], query, [0, n], [2 * v, 0.25 * v, 100 * v, None], "lattice")
  print("lattice: fallback queries at cell = 2, 0.25, 100 voxels and the default: %r of %d" % (fbs, n))
  assert fbs[1] > fbs[0], "quarter-voxel cells: a nearest centre beyond three cells is left to the fallback scan"
  assert fbs[2] == 0, "one cell holding the whole scene decides every query on the grid"


def test_voxel_centers_batches_and_bad_rows(PF):
  rng = np.random.RandomState(3)
  B = 37  # more than the 32 matrices one launch carries
  T = np.tile(np.eye(4), (B, 1, 1))
  T[:, :3, :3] *= rng.uniform(10, 30, (B, 1, 1))
  T[:, :3, 3] = rng.uniform(-5, 5, (B, 3))
  coords = np.concatenate([rng.randint(-2, B + 2, (1025, 1)), rng.randint(-300, 300, (1025, 3))], 1).astype(np.int32)
  want = nr.voxel_centers(coords, np.linalg.inv(T).reshape(B, 16))
  got = PF.voxel_centers(_dev(coords), torch.from_numpy(T.reshape(B, 16))).cpu().numpy()
  assert np.isnan(want).any() and np.array_equal(_bits(got), _bits(want))


# ---- the stopping rule ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("sign", [1, -1])
def test_stopping_rule(PF, axis, sign):
  """The query sits 0.99 h into its cell along one axis; A lies in a diagonal ring-1 cell at 1.7 h, B in the ring-2 cell
  straight ahead at 1.011 h.  A walk that stops after ring 1 because it has found something returns A."""
  h = 0.37
  q = np.full(3, 0.5)
  q[axis] = 0.99 if sign > 0 else 0.01
  a = q + sign * 1.7 / np.sqrt(3.0)
  b = q.copy()
  b[axis] += sign * 1.011
  ca, cb, cq = np.floor(a), np.floor(b), np.floor(q)
  assert np.abs(ca - cq).max() == 1 and np.abs(cb - cq).max() == 2  # ring 1 and ring 2 (in cells, h = 1 here)
  ref = np.stack([a, b]) * h  # A has the lower row: a tie-break cannot rescue B
  idx, _, fbs = check_exact(PF, ref, [0, 2], [q * h], [0, 1], [h], "stopping rule")
  assert idx.tolist() == [1] and fbs == [0]


# ---- exact ties and boundaries ----------------------------------------------------------------------------------------------
def test_exact_ties_and_cell_faces(PF):
  v = 0.0625
  g = np.stack(np.meshgrid(np.arange(-2, 2), np.arange(-2, 2), np.arange(-2, 2), indexing="ij"), -1).reshape(-1, 3)
  coords = np.concatenate([np.zeros((len(g), 1), np.int64), g], 1).astype(np.int32)
  T = np.diag([16.0, 16.0, 16.0, 1.0])
  T[:3, 3] = [-16.0, 32.0, 0.0]  # exact: the centres are multiples of 2^-5
  centers = PF.voxel_centers(_dev(coords), torch.from_numpy(T.reshape(1, 16))).cpu().numpy()
  assert np.array_equal(centers, (g + 0.5) * v - np.array([-1.0, 2.0, 0.0]))
  ref = np.concatenate([centers, centers[5:15], np.array([[1.0, -2.0, 0.0], [1.125, -2.125, -0.125]])])  # duplicates, cell faces
  rng = np.random.RandomState(1)
  pick = centers[rng.randint(0, len(centers), 90)]
  half = v / 2
  two = pick[:30] + [half, 0, 0]
  four = pick[30:60] + [half, half, 0]
  eight = pick[60:] + [half, half, half]
  query = np.concatenate([two, four, eight, centers[:16], ref[-2:]])  # midpoints, exact hits, points on cell faces
  m, n = len(ref), len(query)
  idx, d2, _ = check_exact(PF, ref, [0, m], query, [0, n], [2 * v, v, 0.1, None], "ties")
  ties = [(np.abs(((query[i] - ref) ** 2).sum(1) - d2[i]) == 0).sum() for i in range(90)]
  assert max(ties[60:]) >= 8 and max(ties[:30]) >= 2, "the construction must contain exact 2- and 8-way ties"
  assert all(idx[i] == np.flatnonzero(((query[i] - ref) ** 2).sum(1) == d2[i])[0] for i in range(90)), "ties go to the lowest row"


def test_unrepresentable_cell_and_negative_coordinates(PF):
  k = np.arange(-20, 21)
  pts = np.stack(np.meshgrid(k, k[::5], k[::8], indexing="ij"), -1).reshape(-1, 3) * 0.1  # k * 0.1: on or beside cell faces
  rng = np.random.RandomState(2)
  query = np.concatenate([pts, pts + rng.uniform(-0.05, 0.05, pts.shape), -pts[::3] * 1.5])
  check_exact(PF, pts, [0, len(pts)], query, [0, len(query)], [0.1, 0.3, None], "cell = 0.1")


# ---- far queries, sparse references, crowded cells -------------------------------------------------------------------------
def test_far_queries_and_sparse_references(PF):
  rng = np.random.RandomState(4)
  h = 0.04
  c0 = rng.uniform(0, 5 * h, (200, 3))
  c1 = rng.uniform(0, 5 * h, (150, 3)) + [40 * h, 0, 0]
  ref = np.concatenate([c0, c1])
  gap = np.stack([np.linspace(-2 * h, 47 * h, 257), rng.uniform(0, 5 * h, 257), rng.uniform(0, 5 * h, 257)], 1)
  dirs = rng.normal(size=(64, 3))
  dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
  far = np.array([2.5 * h] * 3) + dirs * (np.linspace(3, 50, 64)[:, None] * h + 4 * h)
  query = np.concatenate([gap, far])
  _, _, fbs = check_exact(PF, ref, [0, len(ref)], query, [0, len(query)], [h, 2 * h, None], "far queries")
  assert fbs[0] > 0, "queries more than three cells from every reference must take the fallback scan"


def test_many_references_in_one_cell(PF):
  rng = np.random.RandomState(5)
  ref = rng.uniform(0.01, 0.99, (700, 3)) * 0.2 + [0.4, -0.6, 0.2]  # one cell of side 0.2
  query = np.concatenate([rng.uniform(0, 1, (300, 3)) * 0.2 + [0.4, -0.6, 0.2], rng.uniform(-1, 1, (85, 3))])
  check_exact(PF, ref, [0, 700], query, [0, len(query)], [0.2, None], "700 references in a cell")


def test_cell_index_outside_the_key(PF):
  """|floor(x / cell)| >= 2^17 - 8 does not fit the grid key.  A reference out there sends its whole scene to the scan, a
  query out there goes itself; coordinates whose squares overflow give d2 = +inf and still the lowest row.  Scene 1 shares the
  call and stays on the grid."""
  rng = np.random.RandomState(6)
  near = rng.uniform(-1, 1, (100, 3))
  ref = np.concatenate([near, [[1e6, 0, 0], [-1e300, 0, 0]], near[:50]])
  roffs = [0, 102, 152]
  q0 = np.concatenate([rng.uniform(-1, 1, (60, 3)), [[2e6, 0, 0], [1e300, 1e300, 0], [-1e300, 5, 5]]])
  q1 = np.concatenate([near[:50] + rng.uniform(-0.1, 0.1, (50, 3)), [[1e5, 0, 0], [1e200, 0, 0]]])  # 1e5 / 0.5 does not fit either
  query = np.concatenate([q0, q1])
  qoffs = [0, len(q0), len(query)]
  idx, d2, fbs = check_exact(PF, ref, roffs, query, qoffs, [0.5, 4.0], "cells outside the key")
  assert fbs[0] == len(q0) + 2, "cell 0.5: all of scene 0 and the two far queries of scene 1 take the scan, nothing else"
  assert np.isposinf(d2[len(q0) - 2]) and idx[len(q0) - 2] == 0, "an overflowing d2 ties at +inf: the lowest row"


# ---- scenes -----------------------------------------------------------------------------------------------------------------
def _three_scenes():
  coords, T, pts, poffs, roffs = nr.three_scene_case()
  centers = nr.voxel_centers(coords, np.linalg.inv(T.reshape(3, 4, 4)).reshape(3, 16))
  return coords, T, centers, pts, poffs, roffs


def test_scene_isolation(PF):
  coords, T, centers, pts, poffs, roffs = _three_scenes()
  idx, d2, _ = check_exact(PF, centers, roffs, pts, poffs, [2 * nr.VOXEL, 0.5 * nr.VOXEL, None], "three scenes")
  glob, _ = nr.nearest_point(centers, [0, len(centers)], pts, [0, len(pts)])
  s2 = slice(poffs[2], poffs[3])
  leaks = int((glob[s2] < roffs[1]).sum())
  assert leaks > 100, "the construction: the globally nearest centre of many scene-2 vertices belongs to scene 0 (%d)" % leaks
  assert (idx[s2] >= roffs[2]).all() and (idx[poffs[1]:poffs[2]] == -1).all() and (idx[:poffs[1]] < roffs[1]).all()


def test_non_finite_rows(PF):
  rng = np.random.RandomState(8)
  ref = rng.uniform(-1, 1, (300, 3))
  ref[[0, 17, 299], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
  query = rng.uniform(-1, 1, (200, 3))
  query[[3, 64, 199], [2, 0, 1]] = [np.nan, -np.inf, np.inf]
  query[10] = [-1, -1, -1]
  nanref = np.full((4, 3), np.nan)  # scene 1: nothing but non-finite references
  refs = np.concatenate([ref, nanref])
  queries = np.concatenate([query, [[0.0, 0, 0]]])
  idx, d2, _ = check_exact(PF, refs, [0, 300, 304], queries, [0, 200, 201], [0.1, 0.01, None], "non-finite rows")
  assert (idx[[3, 64, 199]] == -1).all() and np.isnan(d2[[3, 64, 199]]).all()
  assert not np.isin(idx, [0, 17, 299]).any() and idx[200] == -1 and np.isposinf(d2[200])


# ---- seg_hist ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 20, 64])
@pytest.mark.parametrize("n", [1, 255, 257, 65537])
def test_seg_hist(PF, n, c):
  rng = np.random.RandomState(n + c)
  m = max(n // 3, 1)
  pred = rng.randint(-1, c + 1, m).astype(np.int32)  # a few outside [0, c): not counted
  idx = rng.randint(-1, m, n).astype(np.int32)
  idx[rng.rand(n) < 0.05] = -1
  labels = rng.choice(np.concatenate([np.arange(c), [255, -1, c, c + 7]]), n).astype(np.int32)
  want_hist, want_pp, want_missing = nr.seg_hist(pred, idx, labels, c)
  base = rng.randint(0, 5, (c, c)).astype(np.int64)
  hist, missing = _dev(base.copy()), _dev(np.array([7], np.int64))
  out = PF.seg_hist(_dev(pred), _dev(idx), _dev(labels), c, hist=hist, missing=missing)
  assert np.array_equal(out["hist"].cpu().numpy(), base + want_hist), "hist is accumulated"
  assert np.array_equal(out["point_pred"].cpu().numpy(), want_pp) and int(missing) == 7 + want_missing
  # idx = NULL: identity
  k = min(m, n)
  want_hist, want_pp, want_missing = nr.seg_hist(pred, None, labels[:k], c)
  out = PF.seg_hist(_dev(pred), None, _dev(labels[:k]), c)
  assert np.array_equal(out["hist"].cpu().numpy(), want_hist) and np.array_equal(out["point_pred"].cpu().numpy(), want_pp[:k])
  assert int(out["missing"]) == 0


def test_seg_hist_refuses_65_classes(PF):
  from pointcontrast_amd._lib import lib, PcmiError
  p = _dev(np.zeros(8, np.int32))
  hist = torch.zeros((65, 65), dtype=torch.int64, device=DEV)
  rc = lib.pcmi_seg_hist(C.c_void_p(p.data_ptr()), 8, None, C.c_void_p(p.data_ptr()), 8, 65, C.c_void_p(hist.data_ptr()), None, None,
                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
  assert rc == PCMI_ERR_INVALID
  torch.cuda.synchronize()
  assert int(hist.sum()) == 0
  with pytest.raises(PcmiError):
    PF.seg_hist(p, None, p, 65)


# ---- the C contract ---------------------------------------------------------------------------------------------------------
def test_c_contract():
  from pointcontrast_amd._lib import lib
  coords, T, centers, pts, poffs, roffs = _three_scenes()
  m, n, B = len(centers), len(pts), 3
  want_idx, want_d2 = nr.nearest_point(centers, roffs, pts, poffs)
  ref, query = _dev(centers), _dev(pts)
  ro, qo = _dev(roffs), _dev(poffs)
  need = lib.pcmi_nearest_point_workspace_bytes(m, n, B)
  assert need > 0 and lib.pcmi_nearest_point_workspace_bytes(-1, n, B) == 0 and lib.pcmi_nearest_point_workspace_bytes(m, n, 0) == 0
  st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
  vp = lambda t: C.c_void_p(t.data_ptr())

  def call(ws, idx, d2, ws_bytes, cell=2 * nr.VOXEL):
    return lib.pcmi_nearest_point(vp(ref), vp(ro), m, vp(query), vp(qo), n, B, cell, None, idx.vp, d2.vp, None, ws.vp,
                                  C.c_size_t(ws_bytes), st)

  ws, idx, d2 = Guarded(need), Guarded(n * 4), Guarded(n * 8)
  assert call(ws, idx, d2, need - 1) == PCMI_ERR_WORKSPACE
  assert call(ws, idx, d2, need, cell=0.0) == PCMI_ERR_INVALID and call(ws, idx, d2, need, cell=float("nan")) == PCMI_ERR_INVALID
  torch.cuda.synchronize()
  for g in (ws, idx, d2):
    assert bool((g.buf == 0xA5).all()), "a refused call enqueues nothing"
  runs = []
  for _ in range(2):
    ws, idx, d2 = Guarded(need), Guarded(n * 4), Guarded(n * 8)
    assert call(ws, idx, d2, need) == PCMI_OK
    torch.cuda.synchronize()
    for g, what in ((ws, "workspace"), (idx, "idx"), (d2, "dist2")):
      g.check(what)
    runs.append((idx.view(torch.int32, n).cpu().numpy().copy(), d2.view(torch.float64, n).cpu().numpy().copy()))
  assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(_bits(runs[0][1]), _bits(runs[1][1])), "two runs are bit-equal"
  assert np.array_equal(runs[0][0], want_idx) and np.array_equal(_bits(runs[0][1]), _bits(want_d2))


# ---- end to end -------------------------------------------------------------------------------------------------------------
def _labels_case(n, c, seed):
  """Raw dataset labels 0 .. 2 c + 3, of which the even ids below 2 c are classes (label_map), the rest ignored."""
  rng = np.random.RandomState(seed)
  raw = rng.randint(0, 2 * c + 4, n)
  label_map = {2 * k: k for k in range(c)}
  mapped = np.array([label_map.get(int(x), 255) for x in raw])
  return raw, label_map, mapped


def test_point_cloud_evaluator_two_steps():
  from pointcontrast_amd.downstream import semseg as ss
  coords, T, centers, pts, poffs, roffs = _three_scenes()
  c = 20
  rng = np.random.RandomState(12)
  pred = rng.randint(0, c, len(coords))
  perm = rng.permutation(len(coords))  # the voxels in any order: the evaluator groups them by scene itself
  raw, label_map, mapped = _labels_case(len(pts), c, 13)
  want_idx, _ = nr.nearest_point(centers, roffs, pts, poffs)
  want_hist, want_pp, want_missing = nr.seg_hist(pred, want_idx, mapped, c)
  ev = ss.PointCloudEvaluator(c, ignore_label=255, label_map=label_map)
  # every scene's vertices in two pieces (a room scored in several calls)
  halves = [[], []]
  for b in range(3):
    mid = (poffs[b] + poffs[b + 1]) // 2
    halves[0].append(np.arange(poffs[b], mid))
    halves[1].append(np.arange(mid, poffs[b + 1]))
  got_pp = np.full(len(pts), -7)
  coords_d, pred_d, T_host = _dev(coords[perm]), _dev(pred[perm]), torch.from_numpy(T)
  outs = []
  for k, part in enumerate(halves):
    rows = np.concatenate(part)
    args = (_dev(pts[rows]), _dev(raw[rows]), _dev(np.concatenate([[0], np.cumsum([len(p) for p in part])]).astype(np.int64)))
    torch.cuda.synchronize()
    if k == 1:  # everything on the device, the evaluator's state allocated: step() must not synchronise
      torch.cuda.set_sync_debug_mode("error")
    try:
      outs.append((rows, ev.step(coords_d, pred_d, T_host, *args)))
    finally:
      torch.cuda.set_sync_debug_mode("default")
  for rows, pp in outs:
    got_pp[rows] = pp.cpu().numpy()
  m = ev.compute_metrics()
  assert np.array_equal(got_pp, want_pp), "the per-vertex predictions"
  assert np.array_equal(m["hist"], want_hist) and m["missing"] == want_missing == poffs[2] - poffs[1]
  assert np.array_equal(m["ious"], nr.per_class_iu(want_hist) * 100.0, equal_nan=True)
  assert m["mIoU"] == float(np.nanmean(nr.per_class_iu(want_hist) * 100.0)) and ev.batches == 2


def test_trainer_test_original_pointcloud():
  from pointcontrast_amd.downstream import semseg as ss
  from pointcontrast_amd.lib import synthetic
  torch.manual_seed(5)
  c, v = 20, 0.05
  tr = ss.SegmentationTrainer(c, model="Res16UNet14", lr=0.05, max_iter=50)
  batches, hist, preds = [], np.zeros((c, c), np.int64), []
  for seed in (3, 8):
    b = synthetic.make_batch(seed=seed, batch_size=1, crop=0.6)
    C_, F = b["sinput0_C"], torch.from_numpy(b["sinput0_F"])
    T = np.diag([1 / v, 1 / v, 1 / v, 1.0])
    T[:3, 3] = [3.0, -1.0, 0.5]
    T = T.reshape(1, 16)
    centers = nr.voxel_centers(C_, np.linalg.inv(T.reshape(1, 4, 4)).reshape(1, 16))
    rng = np.random.RandomState(seed)
    pts = centers[rng.randint(0, len(centers), 3001)] + rng.uniform(-0.9, 0.9, (3001, 3)) * v
    raw, label_map, mapped = _labels_case(len(pts), c, seed)
    batches.append((torch.from_numpy(C_), F, torch.from_numpy(T), pts, raw))
    # the same procedure on the host, fed the trainer's own voxel predictions
    tr.model.eval()
    vox = tr.forward(torch.from_numpy(C_), F, training=False).max(1)[1].cpu().numpy()
    idx, _ = nr.nearest_point(centers, [0, len(centers)], pts, [0, len(pts)])
    h, pp, missing = nr.seg_hist(vox, idx, mapped, c)
    assert missing == 0
    hist += h
    preds.append(pp)
  mIoU, ious = tr.test_original_pointcloud(iter(batches), label_map=label_map)
  m = tr.pointcloud_evaluator.compute_metrics()
  assert np.array_equal(m["hist"], hist) and m["missing"] == 0 and hist.sum() > 0
  for got, want in zip(tr.pointcloud_predictions, preds):
    assert np.array_equal(got.cpu().numpy(), want)
  assert np.array_equal(ious, nr.per_class_iu(hist) * 100.0, equal_nan=True) and mIoU == float(np.nanmean(ious))
  assert not tr.model.training
