"""The segmentation validation (csrc/segeval.hip, pointcontrast_amd.downstream.semseg.SegmentationEvaluator) on the MI355X
against tests/segeval_ref.py, the float64 restatement that tests/test_segeval_ref.py holds to scikit-learn, torch and the
reference's recorded outputs.

Tolerances: predictions, counts and the confusion matrix exactly (the logits are drawn so that no row's largest two entries
are equal in float32, plus one case of deliberate ties); the loss within 1e-5 relative (the bound of
test_softmax_cross_entropy_with_ignore_label); probabilities within 1e-6 absolute of the float64 softmax (they are <= 1:
about 16 float32 ulps at 1.0, which covers expf and the quotient); AP on the SAME sorted input within 1e-12 (a float64 sum of
at most n terms <= 1: n 2^-53 = 9e-13 at the n = 8193 used here); AP end to end within 1e-9 where the test has first asserted
that distinct scores of a class lie more than 1e-5 apart (then the device's float32 ranking equals the float64 one, a single
misplaced element would move AP by at least 1 / (n npos) >> 1e-9, and rounding moves it by < 1e-12)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import segeval_ref as S  # noqa: E402
from c_contract import PCMI_ERR_INVALID, PCMI_ERR_WORKSPACE, Guarded, lds, strided  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
IGNORE = 255
AP_BLOCK = 4096  # kApChunk of segeval.hip: the sorted elements one pass of the walk's workgroup covers
TOL_LOSS, TOL_PROB, TOL_AP_SORTED, TOL_AP = 1e-5, 1e-6, 1e-12, 1e-9


def _dev(a, dtype=None):
  t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
  return t if dtype is None else t.to(dtype)


def _p(t):
  return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
  return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


@functools.lru_cache(maxsize=None)
def rows_case(n, c):
  """(logits float32 [n, c] without a tie at any row's maximum, labels with about 20 % ignored, the restatement's results)."""
  rng = np.random.RandomState(1000 * c + n)
  x = (rng.randn(n, c) * 3).astype(np.float32)
  top = np.sort(x, 1)[:, -2:]
  assert (top[:, 0] < top[:, 1]).all(), "a row's two largest logits are equal in float32"
  t = rng.randint(0, c, n)
  t[rng.rand(n) < 0.2] = IGNORE
  pred = S.argmax_lowest(x)
  loss, counted = S.cross_entropy_rows(x, t, IGNORE)
  ref = dict(pred=pred, loss=loss, counted=counted, correct=S.correct_rows(pred, t, IGNORE), hist=S.fast_hist(pred, t, c),
             prob=S.softmax(x))
  for v in ref.values():
    if isinstance(v, np.ndarray):
      v.setflags(write=False)
  return x, t, ref


def _check_rows(out, ref, n, c, what):
  batch = out["batch"].cpu().numpy()
  assert np.array_equal(out["pred"].cpu().numpy(), ref["pred"]), what
  assert np.array_equal(out["hist"].cpu().numpy(), ref["hist"]), what
  assert batch[1] == ref["counted"] and batch[2] == ref["correct"] and batch[3] == n, (what, batch, ref["counted"], ref["correct"])
  if ref["counted"]:
    err = abs(batch[0] - ref["loss"]) / abs(ref["loss"])
    print("%s: loss rel err %.2e" % (what, err))
    assert err <= TOL_LOSS, (what, batch[0], ref["loss"])
  else:
    assert batch[0] == 0.0
  perr = float(np.abs(out["prob_t"].cpu().numpy().astype(np.float64) - ref["prob"].T).max())
  print("%s: prob abs err %.2e" % (what, perr))
  assert out["prob_t"].shape == (c, n) and perr <= TOL_PROB, (what, perr)


# ---- 1. the rows pass -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [2, 13, 20, 41])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1023, 1025, 5000])
def test_seg_eval_rows(n, c):
  from pointcontrast_amd import functional as PF
  x, t, ref = rows_case(n, c)
  out = PF.seg_eval_rows(_dev(x), _dev(t), IGNORE)
  _check_rows(out, ref, n, c, "n %d c %d" % (n, c))
  assert PF.seg_eval_rows(_dev(x), _dev(t), IGNORE, want_prob=False)["prob_t"] is None


def test_seg_eval_rows_ties_go_to_the_lowest_class_and_equal_rows_are_bit_equal():
  from pointcontrast_amd import functional as PF
  rng = np.random.RandomState(7)
  x, idx, pool = S.pool_rows(rng, 37, 9, 1500, spread=2)
  x[::50] = 1.5  # whole rows of equal logits
  x[1::50, [2, 5, 7]] = 4.0  # three equal maxima
  top = np.sort(x, 1)[:, -2:]
  assert (top[:, 0] == top[:, 1]).sum() >= 100
  t = rng.randint(0, 9, 1500)
  out = PF.seg_eval_rows(_dev(x), _dev(t), IGNORE)
  pred = out["pred"].cpu().numpy()
  assert np.array_equal(pred, S.argmax_lowest(x)) and (pred[::50] == 0).all() and (pred[1::50] == 2).all()
  assert np.array_equal(out["hist"].cpu().numpy(), S.fast_hist(pred, t, 9))
  p = out["prob_t"].cpu().numpy().T
  _, first, inv = np.unique(x, axis=0, return_index=True, return_inverse=True)
  assert np.array_equal(p, p[first[inv.reshape(-1)]]), "equal rows must give bit-equal probabilities"


def test_seg_eval_rows_input_forms_and_label_edges():
  from pointcontrast_amd import functional as PF
  n, c = 1025, 13
  x, t, ref = rows_case(n, c)
  # a column slice of a wider buffer, at a column offset
  wide = torch.full((n, c + 11), float("nan"), device=DEV)
  wide[:, 5:5 + c] = _dev(x)
  sl = wide[:, 5:5 + c]
  assert sl.stride(0) == c + 11 and not sl.is_contiguous()
  out = PF.seg_eval_rows(sl, _dev(t), IGNORE)
  _check_rows(out, ref, n, c, "column slice")
  packed = PF.seg_eval_rows(_dev(x), _dev(t), IGNORE)
  assert torch.equal(out["prob_t"], packed["prob_t"]) and torch.equal(out["batch"], packed["batch"])
  # hist accumulates over calls, totals too
  hist = torch.zeros((c, c), dtype=torch.int64, device=DEV)
  totals = torch.zeros(3, dtype=torch.float64, device=DEV)
  for _ in range(2):
    PF.seg_eval_rows(_dev(x), _dev(t), IGNORE, hist=hist, want_prob=False, totals=totals)
  assert np.array_equal(hist.cpu().numpy(), 2 * ref["hist"])
  tot = totals.cpu().numpy()
  want = np.array([2 * n * ref["loss"] / ref["counted"], 2 * n * 100.0 * ref["correct"] / ref["counted"], 2 * n])
  assert np.abs(tot - want).max() <= TOL_LOSS * np.abs(want).max() and tot[2] == 2 * n
  # every row ignored: nothing counted, nothing added anywhere
  before = totals.clone()
  out = PF.seg_eval_rows(_dev(x), torch.full((n,), IGNORE, device=DEV), IGNORE, hist=hist, totals=totals)
  assert out["batch"].cpu().tolist() == [0.0, 0.0, 0.0, float(n)] and torch.equal(totals, before)
  assert np.array_equal(hist.cpu().numpy(), 2 * ref["hist"])
  # a label that is neither a class nor the ignore label: the loss is NaN, the row is counted and absent from hist
  bad = t.copy()
  keep = np.flatnonzero(bad != IGNORE)
  bad[keep[3]] = c + 3
  bad[keep[4]] = -2
  out = PF.seg_eval_rows(_dev(x), _dev(bad), IGNORE)
  batch = out["batch"].cpu().numpy()
  assert np.isnan(batch[0]) and batch[1] == ref["counted"]
  assert np.array_equal(out["hist"].cpu().numpy(), S.fast_hist(ref["pred"], bad, c)) and int(out["hist"].sum()) == ref["counted"] - 2
  assert np.isnan(S.cross_entropy_rows(x, bad, IGNORE)[0])
  # host labels, int64 labels, and an empty batch
  out = PF.seg_eval_rows(_dev(x), torch.from_numpy(t), IGNORE)
  assert np.array_equal(out["hist"].cpu().numpy(), ref["hist"])
  out = PF.seg_eval_rows(torch.zeros((0, c), device=DEV), torch.zeros(0, dtype=torch.int64), IGNORE)
  assert out["pred"].shape == (0,) and int(out["hist"].sum()) == 0 and out["batch"].cpu().tolist() == [0.0] * 4
  with pytest.raises(Exception):
    PF.seg_eval_rows(torch.zeros((4, PF.SEG_EVAL_MAX_CLASSES + 1), device=DEV), torch.zeros(4, dtype=torch.int64), IGNORE)
  PF.seg_eval_rows(torch.zeros((4, PF.SEG_EVAL_MAX_CLASSES), device=DEV), torch.zeros(4, dtype=torch.int64), IGNORE)  # the limit itself


# ---- 2. average precision on a given sorted input -------------------------------------------------------------------------------
def _descending(rng, n, quantum=None):
  s = rng.rand(n)
  if quantum:
    s = np.round(s / quantum) * quantum
  return np.sort(s.astype(np.float32))[::-1].copy()


@functools.lru_cache(maxsize=None)
def ap_case(n):
  """Six classes over n rows, each with its own sorted list: 0 every score equal; 1 no positive row; 2 its only positive last;
  3 a run of equal scores across the first block boundary of the walk, positives on both sides and inside; 4 many short runs
  of ties; 5 distinct scores."""
  rng = np.random.RandomState(n)
  c = 6
  labels = rng.choice([0, 3, 4, 5, IGNORE, 77], n, p=[0.15, 0.3, 0.2, 0.15, 0.15, 0.05])
  only2 = int(rng.randint(0, n))
  labels[only2] = 2
  order = np.stack([rng.permutation(n) for _ in range(c)])
  rest = order[2][order[2] != only2]
  order[2] = np.concatenate([rest, [only2]])
  s = np.stack([_descending(rng, n, q) for q in (None, None, None, None, 0.01, None)])
  s[0] = 0.25
  if n > AP_BLOCK + 200:
    s[3, AP_BLOCK - 96:AP_BLOCK + 105] = s[3, AP_BLOCK - 96]
    run = labels[order[3, AP_BLOCK - 96:AP_BLOCK + 105]] == 3
    assert run[:96].any() and run[96:].any() and (labels[order[3, :AP_BLOCK - 96]] == 3).any() and \
        (labels[order[3, AP_BLOCK + 105:]] == 3).any()
  assert (np.diff(s, axis=1) <= 0).all()
  ref = np.array([S.ap_sorted(s[k], labels[order[k]] == k) for k in range(c)])
  return s, order, labels, ref


@pytest.mark.parametrize("n", [1, 2, 255, AP_BLOCK, AP_BLOCK + 1, 2 * AP_BLOCK + 1])
def test_seg_ap_sorted(n):
  from pointcontrast_amd import functional as PF
  s, order, labels, ref = ap_case(n)
  ap_sum = torch.full((6,), 10.0, dtype=torch.float64, device=DEV)
  ap_cnt = torch.full((6,), 3, dtype=torch.int64, device=DEV)
  ap = PF.seg_ap_sorted(_dev(s), _dev(order), _dev(labels), ap_sum, ap_cnt).cpu().numpy()
  scored = ~np.isnan(ref)
  assert not scored[1] and scored[2], "class 1 has no positive row, class 2 exactly one"
  assert np.array_equal(np.isnan(ap), ~scored), (ap, ref)
  err = float(np.abs(ap - ref)[scored].max())
  print("n %d: AP abs err %.2e" % (n, err), ap, ref)
  assert err <= TOL_AP_SORTED
  npos0 = int((labels == 0).sum())
  if npos0:
    assert abs(ap[0] - npos0 / n) <= TOL_AP_SORTED, "every score equal: one threshold, ap = npos / n"
  assert abs(ap[2] - 1.0 / n) <= TOL_AP_SORTED, "the only positive is last: ap = 1 / n"
  assert np.array_equal(ap_cnt.cpu().numpy(), 3 + scored.astype(np.int64)), "ap_cnt counts the classes that scored"
  want = 10.0 + np.where(scored, ref, 0.0)
  assert np.abs(ap_sum.cpu().numpy() - want).max() <= TOL_AP_SORTED
  again = PF.seg_ap_sorted(_dev(s), _dev(order), _dev(labels))
  assert np.array_equal(again.cpu().numpy(), ap, equal_nan=True), "two runs must agree bit for bit"


def test_seg_average_precision_sorts_on_the_device():
  from pointcontrast_amd import functional as PF
  rng = np.random.RandomState(11)
  x, _, _ = S.pool_rows(rng, 37, 7, 2 * AP_BLOCK + 1)
  t = rng.randint(0, 6, len(x))  # class 6 has no positive row
  t[rng.rand(len(x)) < 0.1] = IGNORE
  prob_t = PF.seg_eval_rows(_dev(x), _dev(t), IGNORE)["prob_t"]
  ap = PF.seg_average_precision(prob_t, _dev(t)).cpu().numpy()
  ref = S.average_precision(prob_t.cpu().numpy().T, t)  # the same float32 scores: ties are the same, their order is free
  assert np.isnan(ap[6]) and np.isnan(ref[6]) and np.abs(ap - ref)[:6].max() <= TOL_AP_SORTED


# ---- 3. the evaluator ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def evaluator_case():
  rng = np.random.RandomState(2)
  c, sizes = 7, (1300, 900, 257)
  x, idx, pool = S.pool_rows(rng, 37, c, sum(sizes))
  p = S.softmax(pool)
  gap = min(float(np.diff(np.unique(p[:, k])).min()) for k in range(c))
  print("smallest gap between distinct scores of a class: %.2e" % gap)
  assert all(len(np.unique(p[:, k])) == len(pool) for k in range(c)), "two distinct rows share a score exactly"
  assert gap > 1e-5, "distinct scores of a class must be more than 1e-5 apart for the float32 ranking to equal the float64 one"
  t = rng.randint(0, c - 1, len(x))
  t[t >= 4] += 1  # class 4 never occurs
  t[rng.rand(len(x)) < 0.1] = IGNORE
  t[sizes[0]:sizes[0] + sizes[1]][t[sizes[0]:sizes[0] + sizes[1]] == 2] = IGNORE  # class 2 has no positive row in batch 2
  acc, lo, batches = S.Accumulator(c, IGNORE), 0, []
  for n in sizes:
    batches.append((x[lo:lo + n], t[lo:lo + n]))
    acc.step(*batches[-1])
    lo += n
  return c, batches, acc.metrics()


def _run_evaluator(c, batches):
  from pointcontrast_amd.downstream import semseg as ss
  ev = ss.SegmentationEvaluator(c, IGNORE, DEV)
  for i, (x, t) in enumerate(batches):
    ev.step(_dev(x), torch.from_numpy(t) if i == 1 else _dev(t))  # (one batch with host labels)
    ev.step(torch.zeros((0, c), device=DEV), torch.zeros(0, dtype=torch.int64))  # n == 0: nothing happens
  return ev


def test_evaluator_matches_the_restatement_over_three_batches():
  c, batches, ref = evaluator_case()
  ev = _run_evaluator(c, batches)
  m = ev.compute_metrics()
  assert sorted(m) == sorted(["loss", "score", "mIoU", "mAP", "mAcc", "ious", "ap_class", "acc", "hist"]) and ev.batches == 3
  assert np.array_equal(m["hist"], ref["hist"])
  assert abs(m["loss"] - ref["loss"]) <= TOL_LOSS * abs(ref["loss"]) and abs(m["score"] - ref["score"]) <= TOL_LOSS * abs(ref["score"])
  for k in ("ious", "acc", "ap_class"):
    assert np.array_equal(np.isnan(m[k]), np.isnan(ref[k])), k
  ok = ~np.isnan(ref["ap_class"])
  assert not ok[4] and ok.sum() == c - 1
  err = float(np.abs(m["ap_class"] - ref["ap_class"])[ok].max()) / 100.0
  print("evaluator: AP abs err %.2e, loss %.6f / %.6f, score %.4f / %.4f" % (err, m["loss"], ref["loss"], m["score"], ref["score"]))
  assert err <= TOL_AP and abs(m["mAP"] - ref["mAP"]) / 100.0 <= TOL_AP
  assert np.array_equal(ev.ap_cnt.cpu().numpy(), [3, 3, 2, 3, 0, 3, 3]), "batches in which the class had a positive row"
  assert np.abs(m["ious"] - ref["ious"])[~np.isnan(ref["ious"])].max() <= 1e-9 and abs(m["mIoU"] - ref["mIoU"]) <= 1e-9
  assert np.abs(m["acc"] - ref["acc"])[~np.isnan(ref["acc"])].max() <= 1e-9 and abs(m["mAcc"] - ref["mAcc"]) <= 1e-9
  ev.reset()
  empty = ev.compute_metrics()
  assert empty["loss"] == 0.0 and int(empty["hist"].sum()) == 0 and np.isnan(empty["mAP"])


def test_evaluator_runs_are_bit_equal_and_step_does_not_synchronise():
  c, batches, _ = evaluator_case()
  a, b = _run_evaluator(c, batches), _run_evaluator(c, batches)
  for name in ("hist", "totals", "ap_sum", "ap_cnt"):
    assert torch.equal(getattr(a, name), getattr(b, name)), name
  x, t = _dev(batches[0][0]), _dev(batches[0][1])
  torch.cuda.synchronize()
  torch.cuda.set_sync_debug_mode("error")
  try:
    a.step(x, t)
  finally:
    torch.cuda.set_sync_debug_mode("default")
  assert a.batches == 4


def test_trainer_validate():
  from pointcontrast_amd.downstream import semseg as ss
  from pointcontrast_amd.lib import synthetic
  torch.manual_seed(5)
  c = 20
  tr = ss.SegmentationTrainer(c, model="Res16UNet14", lr=0.05, max_iter=50)
  batches = []
  for seed in (3, 8):
    b = synthetic.make_batch(seed=seed, batch_size=1, crop=0.6)
    C_, F = torch.from_numpy(b["sinput0_C"]), torch.from_numpy(b["sinput0_F"])
    target = torch.from_numpy(np.random.RandomState(seed).randint(0, c, len(C_)))
    target[::5] = IGNORE
    batches.append((C_, F, target))
  hist = np.zeros((c, c), np.int64)
  for C_, F, target in batches:
    hist += tr.evaluate(C_, F, target.numpy())[2]
  out = tr.validate(iter(batches))
  assert len(out) == 4 and all(isinstance(v, float) and np.isfinite(v) for v in out), out
  loss, score, mAP, mIoU = out
  m = tr.evaluator.compute_metrics()
  assert np.array_equal(m["hist"], hist), "validate() and evaluate() + fast_hist must count the same confusion matrix"
  assert abs(mIoU - float(np.nanmean(ss.per_class_iu(hist)) * 100.0)) <= 1e-9
  assert loss > 0 and 0.0 <= score <= 100.0 and 0.0 <= mAP <= 100.0 and not tr.model.training


# ---- 4. the C contract ---------------------------------------------------------------------------------------------------------
def test_c_contract():
  from pointcontrast_amd._lib import lib, check
  st = _stream()
  n, c = 1025, 13
  x, t, ref = rows_case(n, c)
  ld, off = lds(c, 0)
  xs = strided(n, c, ld, off, fill=torch.from_numpy(x))
  lb = _dev(t, torch.int32)
  need = lib.pcmi_seg_eval_rows_workspace_bytes(n)
  assert need >= (n + 255) // 256 * 16 and lib.pcmi_seg_eval_rows_workspace_bytes(-1) == 0
  ws = Guarded(need)
  pred = Guarded(n * 4)
  prob = Guarded(c * n * 4)
  hist = torch.zeros((c, c), dtype=torch.int64, device=DEV)
  batch = torch.full((4,), -7.0, dtype=torch.float64, device=DEV)
  totals = torch.full((3,), -7.0, dtype=torch.float64, device=DEV)

  def run(w=ws.vp, nbytes=None, logits=xs.vp, ld_=ld, c_=c, labels=_p(lb), p=pred.vp, h=_p(hist), b=_p(batch)):
    return lib.pcmi_seg_eval_rows(logits, ld_, n, c_, labels, IGNORE, p, prob.vp, h, b, _p(totals), w,
                                  ws.size if nbytes is None else C.c_size_t(nbytes), st)

  assert run(nbytes=need - 1) == PCMI_ERR_WORKSPACE and run(w=None, nbytes=0) == PCMI_ERR_WORKSPACE and lib.pcmi_last_error()
  assert run(logits=None) == PCMI_ERR_INVALID and run(labels=None) == PCMI_ERR_INVALID and run(p=None) == PCMI_ERR_INVALID
  assert run(h=None) == PCMI_ERR_INVALID and run(b=None) == PCMI_ERR_INVALID
  assert run(ld_=c - 1) == PCMI_ERR_INVALID and run(c_=0) == PCMI_ERR_INVALID and run(c_=65, ld_=ld + 64) == PCMI_ERR_INVALID
  torch.cuda.synchronize()
  assert bool((batch == -7).all()) and bool((totals == -7).all()) and int(hist.sum()) == 0, "a refused call wrote into an output"
  assert bool((pred.view(torch.uint8, n * 4) == 0xA5).all()) and bool((prob.view(torch.uint8, c * n * 4) == 0xA5).all())
  totals.zero_()
  check(run())  # exactly the queried size, rows at a column offset of a wider buffer
  torch.cuda.synchronize()
  for g, what in ((ws, "workspace"), (pred, "pred"), (prob, "prob_t")):
    g.check("seg_eval_rows " + what)
  xs.check("seg_eval_rows logits")
  out = dict(pred=pred.view(torch.int32, n), prob_t=prob.view(torch.float32, c * n).view(c, n), hist=hist, batch=batch)
  _check_rows(out, ref, n, c, "C call")
  assert totals.cpu().numpy()[2] == n

  # pcmi_seg_ap
  s, order, labels, ref_ap = ap_case(AP_BLOCK + 1)
  c2, n2 = s.shape
  sd, od, ld2 = _dev(s), _dev(order), _dev(labels, torch.int32)
  need = lib.pcmi_seg_ap_workspace_bytes(c2)
  assert need >= c2 * 4 and lib.pcmi_seg_ap_workspace_bytes(0) == 0 and lib.pcmi_seg_ap_workspace_bytes(65) == 0
  ws = Guarded(need)
  ap = torch.full((c2,), -7.0, dtype=torch.float64, device=DEV)
  ap_sum = torch.full((c2,), -7.0, dtype=torch.float64, device=DEV)
  ap_cnt = torch.full((c2,), -7, dtype=torch.int64, device=DEV)

  def run_ap(w=ws.vp, nbytes=None, sp=_p(sd), o=_p(od), lab=_p(ld2), a=_p(ap), n_=n2, c_=c2):
    return lib.pcmi_seg_ap(sp, o, lab, n_, c_, a, _p(ap_sum), _p(ap_cnt), w, ws.size if nbytes is None else C.c_size_t(nbytes), st)

  assert run_ap(nbytes=need - 1) == PCMI_ERR_WORKSPACE and run_ap(w=None, nbytes=0) == PCMI_ERR_WORKSPACE
  assert run_ap(sp=None) == PCMI_ERR_INVALID and run_ap(o=None) == PCMI_ERR_INVALID and run_ap(lab=None) == PCMI_ERR_INVALID
  assert run_ap(a=None) == PCMI_ERR_INVALID and run_ap(n_=-1) == PCMI_ERR_INVALID and run_ap(c_=0) == PCMI_ERR_INVALID
  assert run_ap(c_=65) == PCMI_ERR_INVALID
  torch.cuda.synchronize()
  assert bool((ap == -7).all()) and bool((ap_sum == -7).all()) and bool((ap_cnt == -7).all()), "a refused call wrote into an output"
  check(run_ap())
  torch.cuda.synchronize()
  ws.check("seg_ap workspace")
  got, scored = ap.cpu().numpy(), ~np.isnan(ref_ap)
  assert np.array_equal(np.isnan(got), ~scored) and np.abs(got - ref_ap)[scored].max() <= TOL_AP_SORTED
  check(run_ap(sp=None, o=None, lab=None, n_=0))  # no rows: every class NaN, nothing accumulated
  torch.cuda.synchronize()
  assert bool(torch.isnan(ap).all()) and np.array_equal(ap_cnt.cpu().numpy(), -7 + scored.astype(np.int64))
