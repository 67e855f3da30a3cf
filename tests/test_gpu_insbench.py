"""The benchmark protocol for instance masks on the device (csrc/insbench.hip, functional.py's wrappers, downstream/insseg.py's
InstanceBenchmarkEvaluator) against tests/insbench_ref.py, which tests/test_insbench_ref.py holds to planted answers and to
the benchmark script's own spelling of the average precision.  Counts, flags and states are integers; every float64 result is
a fixed sequence of single roundings: everything is compared EXACTLY (NaN equal to NaN)."""
import ctypes as C

import numpy as np
import pytest
import torch

import insbench_ref as br
from c_contract import DEV, Guarded, PCMI_OK

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def PF():
  from pointcontrast_amd import functional as pf
  return pf


def _dev(a, dtype=None):
  t = torch.from_numpy(np.ascontiguousarray(a))
  return (t if dtype is None else t.to(dtype)).to(DEV)


def _stream():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _vp(t):
  return C.c_void_p(t.data_ptr()) if t.numel() else None


def same(a, b):
  return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


# ---- void overlap ---------------------------------------------------------------------------------------------------------------
def _void_rows(n, P, G, seed, run=1):
  rng = np.random.default_rng(seed)
  m = -(-n // run) if n else 0
  pred = np.repeat(rng.integers(-2, P + 2, m), run)[:n].astype(np.int32)  # ids outside [0, P) on both sides
  gt = np.repeat(rng.integers(-2, G + 2, m), run)[:n].astype(np.int32)
  return pred, gt, rng.integers(0, 2, G).astype(np.int32)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_void_overlap_sizes(PF, n):
  pred, gt, valid = _void_rows(n, 3, 4, 40 + n)
  got = PF.instance_void_overlap(_dev(pred), _dev(gt), _dev(valid), 3)
  assert got.dtype == torch.int32 and same(got.cpu().numpy(), br.void_overlap(pred, gt, valid, 3))


@pytest.mark.parametrize("run", [1, 64, 50], ids=["ids change inside every wave", "wave-uniform ids", "runs of 50"])
def test_void_overlap_100000_rows_against_bincount(PF, run):
  n, P, G = 100000, 37, 53
  pred, gt, valid = _void_rows(n, P, G, 7 + run, run)
  if run == 50:
    pred[::97] = (pred[::97] + 1) % P  # runs broken up here and there
  void = ~((gt >= 0) & (gt < G)) | (valid[np.clip(gt, 0, G - 1)] == 0)
  ok = (pred >= 0) & (pred < P) & void
  want = np.bincount(pred[ok], minlength=P).astype(np.int32)
  assert want.sum() > 10000 and (~ok).sum() > 10000
  got = PF.instance_void_overlap(_dev(pred), _dev(gt), _dev(valid), P)
  assert same(got.cpu().numpy(), want)


# ---- matching -------------------------------------------------------------------------------------------------------------------
def check_match(PF, case, what):
  """The device's flags, states and npos equal the restatement's; returns the restatement's."""
  want_flag, want_state, want_npos = br.bench_match(**case)
  k = {name: _dev(case[name]) for name in ("inter", "pred_size", "gt_size", "void_inter", "pred_scene", "pred_class", "pred_score", "gt_scene",
                                           "gt_class")}
  flag, state, npos = PF.instance_bench_match(k["inter"], k["pred_size"], k["gt_size"], k["void_inter"], k["pred_scene"], k["pred_class"],
                                              k["pred_score"], k["gt_scene"], k["gt_class"], case["B"], case["Cls"], case["thresholds"],
                                              case["min_region"])
  T, (P, G) = len(case["thresholds"]), case["inter"].shape
  assert flag.dtype == torch.int8 and tuple(flag.shape) == (T, P, 3) and state.dtype == torch.int32 and tuple(state.shape) == (T, G)
  flag, state = flag.cpu().numpy(), state.cpu().numpy()
  bad = np.argwhere(flag != want_flag)
  assert len(bad) == 0, "%s: %d flags differ, first at (t, p, slot) %s: got %d want %d" % (
      what, len(bad), bad[0].tolist(), flag[tuple(bad[0])], want_flag[tuple(bad[0])])
  assert same(state, want_state), "%s: gt_state" % what
  assert same(npos.cpu().numpy(), want_npos), "%s: npos" % what
  return want_flag, want_state, want_npos


@pytest.mark.parametrize("name", ["claim 0.9 0.8", "claim 0.8 0.9", "claim equal scores", "void", "small", "small only", "min region", "triple"])
def test_match_cpu_cases(PF, name):
  case = {"claim 0.9 0.8": lambda: br.two_gt_case((0.9, 0.8)), "claim 0.8 0.9": lambda: br.two_gt_case((0.8, 0.9)),
          "claim equal scores": lambda: br.two_gt_case((0.8, 0.8)), "void": lambda: br.void_case("void"),
          "small": lambda: br.void_case("small"), "small only": br.small_only_case, "min region": br.min_region_case,
          "triple": br.triple_case}[name]()
  flag, _, _ = check_match(PF, case, name)
  if name == "claim equal scores":  # the lowest p wins: p0 at g0; p1, alone at g1, is true there
    assert flag[0].tolist() == [[1, -1, -1], [0, 1, -1]]
  if name == "triple":
    assert flag[0, 3].tolist() == [1, 0, 0]


def test_match_65_predictions_and_ground_truths_in_one_unit(PF):
  """One scene, one class, P = G = 65: a prediction beyond a wave's 64 lanes, claims with two claimants in different lanes,
  T = 11."""
  case = br.chain_case()
  assert case["inter"].shape == (65, 65) and len(case["thresholds"]) == 11
  flag, state, npos = check_match(PF, case, "chain")
  assert npos.tolist() == [65] and (flag[9, 64] == [1, -1, -1]).all() and ((flag[9] >= 0).sum(1) == 2).sum() == 32
  pred, gt, psc, pcl, score, gsc, gcl = br.random_rows(1, 1, 1, 65, 65, unscored=0, foreign=0)
  case = br.match_args(pred, gt, psc, pcl, score, gsc, gcl, 1, 1, (0.5,), 100)  # T = 1
  flag, _, _ = check_match(PF, case, "random, one unit")
  assert (flag == 1).any() and (flag == 0).any()


def test_match_scenes_without_predictions_and_without_ground_truth(PF):
  """Scene 0: ground truth only.  Scene 1: a class-1 ground truth under a class-0 prediction: unit (1, 0) has predictions and
  no ground truth, unit (1, 1) ground truth and no prediction.  Scene 2: nothing.  And the two empty sides, P = 0 and G = 0."""
  gt = np.repeat([0, 1, 2], [150, 120, 200])
  pred = np.where(gt == 2, 0, -1)
  case = br.match_args(pred, gt, [1], [0], [0.6], [0, 0, 1], [0, 1, 1], 3, 2, br.BENCHMARK_THRESHOLDS, 100)
  flag, state, npos = check_match(PF, case, "lonely units")
  assert (flag[:, 0, 0] == 0).all() and (state == 0).all() and npos.tolist() == [1, 2]
  none = br.match_args(np.full(len(gt), -1), gt, [], [], [], [0, 0, 1], [0, 1, 1], 3, 2, (0.25, 0.5), 100)
  check_match(PF, none, "P = 0")
  none = br.match_args(pred, np.full(len(gt), -1), [1], [0], [0.6], [], [], 3, 2, (0.25, 0.5), 100)
  flag, _, _ = check_match(PF, none, "G = 0")
  assert (flag == -1).all(), "all rows void: ignored"


@pytest.mark.parametrize("seed", [2, 3])
def test_match_three_scenes_three_classes_sizes_around_min_region(PF, seed):
  pred, gt, psc, pcl, score, gsc, gcl = br.random_rows(seed, 3, 3, 40, 50, sizes=(90, 115))
  case = br.match_args(pred, gt, psc, pcl, score, gsc, gcl, 3, 3, br.BENCHMARK_THRESHOLDS, 100)
  assert (case["gt_size"] < 100).any() and (case["gt_size"] >= 100).any() and (case["pred_size"] == 0).any()
  flag, state, npos = check_match(PF, case, "3 x 3")
  assert (flag == 1).sum() > 10 and (flag == 0).sum() > 10 and (state == -1).any() and (state == 0).any() and npos.sum() > 5


def test_match_refuses_a_threshold_below_a_quarter(PF):
  from pointcontrast_amd._lib import PcmiError
  case = br.two_gt_case((0.9, 0.8))
  for bad in ((0.5, 0.2), (1.0,), (float("nan"),), ()):
    with pytest.raises(PcmiError):
      check_match(PF, dict(case, thresholds=bad), "refused")


# ---- average precision ----------------------------------------------------------------------------------------------------------
def _ap_case():
  """Classes of 1023, 1024, 1025 and 2049 entries, one full of -1 flags, an empty one and one with npos = 0; scores descend
  inside a class with ties, and a group of equal scores lies across positions 1023 / 1024 of the two longest; two thresholds."""
  rng = np.random.default_rng(31)
  sizes = [1023, 1024, 1025, 2049, 300, 0, 40]
  npos = np.array([700, 600, 2000, 1200, 5, 3, 0], np.int32)
  flag, score = [], []
  for n in sizes:
    s = -np.sort(-(rng.integers(0, max(n // 3, 1) + 1, n) / 1024.0))
    if n > 1024:
      s[1019:min(n, 1031)] = s[1019]
    score.append(s)
    flag.append(rng.choice(np.array([-1, 0, 1], np.int8), (2, n), p=[0.3, 0.3, 0.4]))
  flag[4][:] = -1
  flag[0][1, :] = 0  # all false at the second threshold
  flag[3][0, 1024:1031] = -1  # the straddling group ends on skipped entries
  offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
  return np.ascontiguousarray(np.concatenate(flag, 1)), np.concatenate(score), offs, npos


def test_ap_block_edges_groups_and_skipped_entries(PF):
  flag, score, offs, npos = _ap_case()
  want_ap, want_prec, want_rec = br.bench_ap(flag, score, offs, npos)
  out = PF.instance_bench_ap(_dev(flag), _dev(score), _dev(offs), _dev(npos), curves=True)
  ap, prec, rec = (out[k].cpu().numpy() for k in ("ap", "prec", "rec"))
  print("ap\n", ap, "\nwant\n", want_ap)
  assert same(ap, want_ap)
  assert same(prec, want_prec) and same(rec, want_rec)
  assert np.isnan(ap[:, 6]).all() and (ap[:, 4] == 0).all() and (ap[:, 5] == 0).all() and ap[1, 0] == 0 and (ap[0, :4] > 0).all()
  assert np.isfinite(prec).sum() > 500
  assert same(PF.instance_bench_ap(_dev(flag), _dev(score), _dev(offs), _dev(npos))["ap"].cpu().numpy(), want_ap), "without the curves"
  # no entries at all
  e = PF.instance_bench_ap(torch.zeros((2, 0), dtype=torch.int8, device=DEV), torch.zeros(0, dtype=torch.float64, device=DEV),
                           _dev(np.zeros(4, np.int32)), _dev(np.array([1, 0, 2], np.int32)), curves=True)
  assert same(e["ap"].cpu().numpy(), [[0, np.nan, 0]] * 2)


# ---- every entry point in exactly its workspace, between guard bands, twice -------------------------------------------------------
def test_entry_points_guarded_exact_workspace_and_determinism():
  from pointcontrast_amd._lib import lib
  pred, gt, psc, pcl, score, gsc, gcl = br.random_rows(5, 2, 3, 30, 40)
  case = br.match_args(pred, gt, psc, pcl, score, gsc, gcl, 2, 3, br.BENCHMARK_THRESHOLDS, 100)
  P, G, T, Cls, n = 40, 30, 10, 3, len(pred)
  want_flag, want_state, want_npos = br.bench_match(**case)
  pred_d, gt_d, valid_d = _dev(pred, torch.int32), _dev(gt, torch.int32), _dev((gcl >= 0).astype(np.int32))
  d = {k: _dev(v) for k, v in case.items() if isinstance(v, np.ndarray)}
  thr = (C.c_double * T)(*case["thresholds"])
  a_flag, a_score, a_offs, a_npos = _ap_case()
  E, aT, aC = a_flag.shape[1], 2, len(a_npos)
  want_ap, want_prec, want_rec = br.bench_ap(a_flag, a_score, a_offs, a_npos)
  af, asc, aof, anp = _dev(a_flag), _dev(a_score), _dev(a_offs), _dev(a_npos)
  need = lib.pcmi_instance_bench_ap_workspace_bytes(E, aC, aT)
  assert need > 0
  runs = []
  for _ in range(2):
    void, flag, state, npos = Guarded(P * 4), Guarded(T * P * 3), Guarded(T * G * 4), Guarded(Cls * 4)
    npos.view(torch.int32, Cls).zero_()
    rc = lib.pcmi_instance_void_overlap(_vp(pred_d), _vp(gt_d), _vp(valid_d), n, P, G, void.vp, _stream())
    assert rc == PCMI_OK, lib.pcmi_last_error()
    rc = lib.pcmi_instance_bench_match(_vp(d["inter"]), _vp(d["pred_size"]), _vp(d["gt_size"]), void.vp, _vp(d["pred_scene"]),
                                       _vp(d["pred_class"]), _vp(d["pred_score"]), _vp(d["gt_scene"]), _vp(d["gt_class"]), P, G, 2, Cls, 100,
                                       thr, T, flag.vp, state.vp, npos.vp, _stream())
    assert rc == PCMI_OK, lib.pcmi_last_error()
    ws, ap, prec, rec = Guarded(need), Guarded(aT * aC * 8), Guarded(aT * E * 8), Guarded(aT * E * 8)
    rc = lib.pcmi_instance_bench_ap(_vp(af), _vp(asc), _vp(aof), _vp(anp), E, aC, aT, ap.vp, prec.vp, rec.vp, ws.vp, ws.size, _stream())
    assert rc == PCMI_OK, lib.pcmi_last_error()
    torch.cuda.synchronize()
    for g, what in ((void, "void_inter"), (flag, "entry_flag"), (state, "gt_state"), (npos, "npos"), (ws, "bench_ap workspace"), (ap, "ap"),
                    (prec, "prec"), (rec, "rec")):
      g.check(what)
    runs.append([void.view(torch.int32, P).cpu().numpy().copy(), flag.view(torch.int8, T * P * 3).cpu().numpy().copy(),
                 state.view(torch.int32, T * G).cpu().numpy().copy(), npos.view(torch.int32, Cls).cpu().numpy().copy(),
                 ap.view(torch.float64, aT * aC).cpu().numpy().copy(), prec.view(torch.float64, aT * E).cpu().numpy().copy(),
                 rec.view(torch.float64, aT * E).cpu().numpy().copy()])
  void, flag, state, npos, ap, prec, rec = runs[0]
  assert same(void, case["void_inter"]) and same(flag, want_flag.reshape(-1)) and same(state, want_state.reshape(-1)) and same(npos, want_npos)
  assert same(ap, want_ap.reshape(-1)) and same(prec, want_prec.reshape(-1)) and same(rec, want_rec.reshape(-1))
  for a, b in zip(runs[0], runs[1]):
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "the same bits from run to run"
  small, out = Guarded(need - 1), Guarded(aT * aC * 8)
  assert lib.pcmi_instance_bench_ap(_vp(af), _vp(asc), _vp(aof), _vp(anp), E, aC, aT, out.vp, None, None, small.vp, small.size, _stream()) == -7
  # nothing to do enqueues nothing
  out = Guarded(64)
  assert lib.pcmi_instance_void_overlap(None, None, None, 0, 0, 0, None, _stream()) == PCMI_OK
  assert lib.pcmi_instance_bench_match(None, None, None, None, None, None, None, None, None, 0, 0, 1, 1, 100, thr, 1, None, None, out.vp,
                                       _stream()) == PCMI_OK
  torch.cuda.synchronize()
  assert bool((out.buf == 0xA5).all()), "P == 0 and G == 0 must enqueue nothing"


# ---- evaluator ------------------------------------------------------------------------------------------------------------------
def _batch(seed, B, P=48, G=36, Cls=5, pad=8):
  """A batch as the evaluator takes it: (pred dict of host arrays with `pad` unused slots, gt_instance, gt_class)."""
  pred, gt, psc, pcl, score, gsc, gcl = br.random_rows(seed, B, Cls, G, P, sizes=(60, 300))
  score = score.copy()
  score[1] = np.nan  # counts as 0
  n = len(pred)
  row_scene = np.where(gt >= 0, gsc[np.maximum(gt, 0)], -1)
  for i in range(n):  # the rows without instance belong to the scene of the rows before them
    if row_scene[i] < 0:
      row_scene[i] = row_scene[i - 1] if i else 0
  offs = np.searchsorted(row_scene, np.arange(B + 1))
  gt_class = np.where(gt >= 0, gcl[np.maximum(gt, 0)], 0)
  gt_class = np.where(gt_class < 0, 1, gt_class)  # an unscored instance: a stuff class
  fill = lambda a, v, dt: np.concatenate([a, np.full(pad, v)]).astype(dt)  # noqa: E731
  d = dict(instance=pred.astype(np.int32), inst_class=fill(pcl, -1, np.int32), inst_scene=fill(psc, -1, np.int32),
           inst_score=fill(score, 0.0, np.float64), inst_size=fill(np.zeros(P), 0, np.int32), scene_offsets=offs.astype(np.int64))
  return d, gt, gt_class


def _to_dev(pred):
  return {k: _dev(v) for k, v in pred.items()}


def test_evaluator_two_steps_equal_one_step_on_the_concatenated_batch():
  from pointcontrast_amd.downstream.insseg import InstanceBenchmarkEvaluator
  (p1, g1, c1), (p2, g2, c2) = _batch(11, 2), _batch(12, 3)
  two, ref = InstanceBenchmarkEvaluator(5), br.Evaluator(5)
  for p, g, c in ((p1, g1, c1), (p2, g2, c2)):
    two.step(_to_dev(p), torch.from_numpy(g), torch.from_numpy(c))
    ref.step(p, g, c)
  P1, G1, n1 = len(p1["inst_class"]), int(g1.max()) + 1, len(g1)
  cat = dict(instance=np.concatenate([p1["instance"], np.where(p2["instance"] >= 0, p2["instance"] + P1, -1)]).astype(np.int32),
             inst_scene=np.concatenate([p1["inst_scene"], np.where(p2["inst_scene"] >= 0, p2["inst_scene"] + 2, -1)]).astype(np.int32),
             scene_offsets=np.concatenate([p1["scene_offsets"], p2["scene_offsets"][1:] + n1]),
             **{k: np.concatenate([p1[k], p2[k]]) for k in ("inst_class", "inst_score", "inst_size")})
  one = InstanceBenchmarkEvaluator(5)
  one.step(_to_dev(cat), torch.from_numpy(np.concatenate([g1, np.where(g2 >= 0, g2 + G1, -1)])), torch.from_numpy(np.concatenate([c1, c2])))
  m2, m1, want = two.compute_metrics(), one.compute_metrics(), ref.compute_metrics()
  print({k: m2[k] for k in ("AP", "AP50", "AP25", "n_gt")})
  assert br.same_metrics(m2, m1), "two steps against one"
  assert br.same_metrics(m2, want), "against the restatement"
  assert 0.0 < m2["AP"] < m2["AP25"] < 1.0 and m2["n_gt"][2:].sum() > 20 and m2["n_gt"][:2].sum() == 0
  assert br.same_metrics(InstanceBenchmarkEvaluator(5).compute_metrics(), br.Evaluator(5).compute_metrics()), "no batch at all"


def test_evaluator_planted_degradation_equals_the_restatement():
  """test_gpu_insseg.py's planted case: six ground-truth instances in two scenes; the prediction merges one into another, drops
  a third, halves a fourth and frays a fifth."""
  from pointcontrast_amd.downstream.insseg import BENCHMARK_THRESHOLDS, InstanceBenchmarkEvaluator
  sizes = [400, 300, 500, 350, 450, 250]
  gt = np.repeat(np.arange(6), sizes)
  n = len(gt)
  gt_cls = np.repeat([2, 2, 3, 2, 3, 3], sizes)
  pred = gt.copy()
  pred[gt == 1] = 0
  pred[gt == 2] = -1
  pred[np.flatnonzero(gt == 3)[200:]] = -1
  pred[np.flatnonzero(gt == 5)[:30]] = -1
  ids = {0: 0, 3: 1, 4: 2, 5: 3}
  pinst = np.array([ids.get(v, -1) for v in pred], np.int32)
  M = 8
  p = dict(instance=pinst, inst_class=np.array([2, 2, 3, 3] + [-1] * 4, np.int32), inst_scene=np.array([0, 1, 1, 1] + [-1] * 4, np.int32),
           inst_score=np.array([0.9, 0.8, 0.95, 0.7] + [0.0] * 4), inst_size=np.zeros(M, np.int32), scene_offsets=np.array([0, 1200, n], np.int64))
  ev, ref = InstanceBenchmarkEvaluator(4), br.Evaluator(4)
  ev.step(_to_dev(p), torch.from_numpy(gt), torch.from_numpy(gt_cls))
  ref.step(p, gt, gt_cls)
  m, want = ev.compute_metrics(keep_curves=True), ref.compute_metrics()
  assert br.same_metrics(m, want)
  assert 0.0 < m["AP"] < m["AP50"] <= m["AP25"] < 1.0 and m["n_gt"].tolist() == [0, 0, 3, 3]
  # the merged prediction (iou 400 / 700) is true up to 0.55 and false from 0.6 on; the halved one (200 / 350) likewise
  flag, _, _ = ref.lists()
  assert ev.last_ap["prec"].shape == (len(BENCHMARK_THRESHOLDS), 3 * M) and same(ev.last_ap["order"].cpu().numpy()[:4], [0, 1, 2, 3])
  assert flag[:, 0].tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0, 1]


def _points_case(empty_scene=False):
  """Two scenes of 1000 voxels each on a 5 cm lattice (the second one empty with empty_scene), k = 1 .. 3 vertices per voxel
  jittered by less than half a voxel; predicted instances = slabs of the voxels along x, ground truth = slabs of the vertices
  cut elsewhere."""
  rng = np.random.default_rng(41)
  V = 0.05
  coords, pts, pinst, gti, gtc, sizes = [], [], [], [], [], []
  T = np.zeros((2, 16))
  for b in range(2):
    g = np.unique(rng.integers(0, 24, (1400, 3)), axis=0)
    g = g[rng.permutation(len(g))[:1000]]
    M = np.diag([1 / V, 1 / V, 1 / V, 1.0])
    M[:3, 3] = [0.3 + b, -0.2, 0.1]
    T[b] = M.reshape(-1)
    centre = (g + 0.5 - M[:3, 3]) * V
    k = rng.integers(1, 4, len(g))
    v = np.repeat(centre, k, 0) + rng.uniform(-0.49, 0.49, (k.sum(), 3)) * V
    vx = np.repeat(g[:, 0], k)
    pts.append(v)
    sizes.append(len(v))
    gti.append(np.where(vx < 22, vx // 5 + 5 * b, -1))  # five instances per scene, a void slab at the end
    gtc.append(np.where(vx < 22, 2 + (vx // 5) % 2, 0))
    if not (empty_scene and b == 1):
      coords.append(np.concatenate([np.full((len(g), 1), b), g], 1))
      pinst.append(np.where(g[:, 0] < 22, (g[:, 0] + 2) // 6 + 4 * b, -1))  # four per scene, cut 2 voxels off the ground truth's
  coords = np.concatenate(coords).astype(np.int32)
  order = rng.permutation(len(coords))  # NOT scene-major: the carry sorts
  P = 12
  pred = dict(instance=np.concatenate(pinst).astype(np.int32)[order], inst_class=np.array(([2, 3, 2, 3] * 2) + [-1] * 4, np.int32),
              inst_scene=np.array([0] * 4 + [1] * 4 + [-1] * 4, np.int32), inst_score=np.concatenate([rng.integers(1, 9, 8) / 8.0, np.zeros(4)]),
              inst_size=np.zeros(P, np.int32), scene_offsets=np.array([0, 1000, len(coords)], np.int64))
  return (coords[order], pred, T, np.concatenate(pts), np.concatenate(gti), np.concatenate(gtc),
          np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))


@pytest.mark.parametrize("empty_scene", [False, True])
def test_evaluator_step_points_equals_the_restatement(empty_scene):
  from pointcontrast_amd.downstream.insseg import InstanceBenchmarkEvaluator
  coords, pred, T, pts, gti, gtc, offs = _points_case(empty_scene)
  assert 3500 < len(pts) < 4500 and len(coords) == (1000 if empty_scene else 2000)
  ev, ref = InstanceBenchmarkEvaluator(4), br.Evaluator(4)
  got = ev.step_points(_dev(coords), _to_dev(pred), T, torch.from_numpy(pts), torch.from_numpy(gti), torch.from_numpy(gtc), torch.from_numpy(offs))
  want = ref.step_points(coords, pred, T, pts, gti, gtc, offs)
  assert got.dtype == torch.int32 and got.is_cuda and same(got.cpu().numpy(), want)
  m, m_want = ev.compute_metrics(), ref.compute_metrics()
  print({k: m[k] for k in ("AP", "AP50", "AP25", "n_gt")})
  assert br.same_metrics(m, m_want)
  assert m["n_gt"].tolist() == [0, 0, 6, 4] and 0.0 < m["AP25"] < 1.0
  if empty_scene:
    assert (want[offs[1]:] == -1).all() and (want[:offs[1]] >= 0).any(), "a scene without voxels: no prediction on its vertices"
    assert (ref.flag[0][:, 4:] == -1).all(), "and its predictions, without rows, produce nothing"


# ---- trainer --------------------------------------------------------------------------------------------------------------------
def test_trainer_benchmark_original_pointcloud_is_deterministic():
  from test_gpu_insseg import _box_scenes, _trainer
  coords, feats, target, instance = _box_scenes()
  tr = _trainer(3)
  c = coords.numpy()
  T = np.tile(np.diag([50.0, 50.0, 50.0, 1.0]).reshape(1, 16), (2, 1))
  rows = [np.flatnonzero(c[:, 0] == b) for b in range(2)]
  points = [(c[r, 1:].astype(np.float64) + 0.5) * 0.02 for r in rows]
  batch = (coords, feats, T, points, [instance.numpy()[r] for r in rows], [target.numpy()[r] for r in rows])
  a = tr.benchmark_original_pointcloud([batch])
  ids = tr.benchmark_predictions[0]
  assert ids.dtype == torch.int32 and tuple(ids.shape) == (len(coords),)
  assert same(ids.cpu().numpy(), tr.predict(coords, feats)["instance"].cpu().numpy()), "a vertex at its voxel's centre takes the voxel's id"
  b = tr.benchmark_original_pointcloud([batch])
  assert br.same_metrics(a, b)
  assert a["n_gt"].tolist() == [0, 0, 2, 2] and set(a) == {"AP", "AP50", "AP25", "ap_class", "ap50_class", "ap25_class", "n_gt", "ap"}
  assert tr.benchmark_evaluator.thresholds == br.BENCHMARK_THRESHOLDS
