"""tests/insbench_ref.py -- the numpy restatement the kernels of csrc/insbench.hip are held to -- against planted answers and
against a test-local spelling of the benchmark script's own average precision (argsort / cumsum / unique / convolve).  The
rules are restated from the script's rules and were never run against the script."""
import numpy as np
import pytest

import insbench_ref as br
from pointcontrast_amd.downstream.insseg import BENCHMARK_THRESHOLDS


def script_ap(y_true, y_score, hard_false_negatives):
  """The script's precision-recall integration for one class and threshold with ground truth and predictions."""
  y_true, y_score = np.asarray(y_true, dtype=np.float64), np.asarray(y_score, dtype=np.float64)
  order = np.argsort(y_score)
  y_score_sorted, y_true_sorted = y_score[order], y_true[order]
  cumsum = np.cumsum(y_true_sorted)
  _, unique_indices = np.unique(y_score_sorted, return_index=True)
  num = len(unique_indices) + 1
  num_examples, num_true = len(y_score_sorted), cumsum[-1]
  precision, recall = np.zeros(num), np.zeros(num)
  cumsum = np.append(cumsum, 0)
  for k, first in enumerate(unique_indices):
    below = cumsum[first - 1]
    tp = num_true - below
    fp = num_examples - first - tp
    fn = below + hard_false_negatives
    precision[k], recall[k] = float(tp) / (tp + fp), float(tp) / (tp + fn)
  precision[-1], recall[-1] = 1.0, 0.0
  conv = np.append(np.append(recall[0], recall), 0.0)
  return float(np.dot(precision, np.convolve(conv, [-0.5, 0, 0.5], "valid")))


def test_thresholds_are_the_scripts_doubles():
  assert BENCHMARK_THRESHOLDS == br.BENCHMARK_THRESHOLDS and len(BENCHMARK_THRESHOLDS) == 10
  assert BENCHMARK_THRESHOLDS[0] == 0.5 and BENCHMARK_THRESHOLDS[-1] == 0.25
  assert BENCHMARK_THRESHOLDS[2] == 0.6000000000000001 != 0.6 and BENCHMARK_THRESHOLDS[8] == 0.9000000000000004, "np.arange's values, not k / 20"


def test_closed_form_ap_equals_the_scripts_convolution():
  rng = np.random.default_rng(5)
  worst = 0.0
  for k in range(1200):
    n = int(rng.integers(1, 41))
    score = rng.integers(0, 6, n) / 5.0 if k % 2 else rng.random(n)  # every other list: tied scores
    true = np.zeros(n, np.int64) if k % 10 == 3 else rng.integers(0, 2, n)  # every tenth: all false
    hard = int(rng.integers(0, 4)) if k % 3 else 0  # hard false negatives: ground truths no prediction claimed
    npos = int(true.sum()) + hard
    if npos == 0:
      npos = hard = 1
    order = np.argsort(-score, kind="stable")
    flags = true[order].astype(np.int8)
    want = script_ap(true, score, hard)
    got = br.ap_one(flags, score[order], npos)
    pad = np.flatnonzero(rng.random(n) < 0.2)  # flags of -1 among the entries, whatever their scores, change nothing
    assert br.ap_one(np.insert(flags, pad, -1), np.insert(score[order], pad, 0.5), npos) == got
    worst = max(worst, abs(got - want))
    assert abs(got - want) <= 1e-12, (k, got, want)
  print("closed form against the convolution spelling: worst difference %.3g" % worst)


def _entries(flag, t):
  """{prediction: its entries in slot order} at threshold index t."""
  return {p: [int(f) for f in flag[t, p] if f >= 0] for p in range(flag.shape[1])}


@pytest.mark.parametrize("scores,want25", [((0.9, 0.8), {0: [1], 1: [0, 1]}), ((0.8, 0.9), {0: [0], 1: [1, 1]})])
def test_planted_claim_case(scores, want25):
  case = br.two_gt_case(scores)
  assert case["pred_size"].tolist() == [60, 80] and case["gt_size"].tolist() == [100, 100] and case["thresholds"] == (0.25, 0.5)
  flag, state, npos = br.bench_match(**case)
  assert npos.tolist() == [2]
  # at 0.25: p0 is the first claimant of g0 and becomes visited; p1, a duplicate claimant of g0, still claims g1
  assert _entries(flag, 0) == want25 and state[0].tolist() == [1, 1]
  # at 0.5: only p0 exceeds the threshold (0.6); p1 is an unmatched false positive, g1 stays unmatched
  assert _entries(flag, 1) == {0: [1], 1: [0]} and state[1].tolist() == [1, 0]


@pytest.mark.parametrize("where", ["void", "small"])
def test_void_rule(where):
  case = br.void_case(where)
  assert case["pred_size"].tolist() == [100] and case["gt_size"].tolist() == [1000, 99]
  assert case["void_inter"].tolist() == ([62] if where == "void" else [0]) and case["inter"][0, 1] == (0 if where == "void" else 62)
  thr = BENCHMARK_THRESHOLDS
  flag, state, npos = br.bench_match(**case)
  assert npos.tolist() == [1], "the 99-row ground truth is not counted"
  assert (state[:, 1] == -1).all() and (state[:, 0] == 0).all()
  for t, th in enumerate(thr):
    want = [] if th < 0.62 else [0]  # 0.62 > th: ignored at 0.25, 0.5, 0.55 and 0.6; a false positive from 0.65 on
    assert _entries(flag, t)[0] == want, (th, _entries(flag, t))
  assert _entries(flag, thr.index(0.5))[0] == [] and _entries(flag, 2)[0] == [] and _entries(flag, 3)[0] == [0]


def test_prediction_matching_only_a_small_ground_truth_emits_nothing():
  case = br.small_only_case()
  assert case["pred_size"].tolist() == [110] and case["inter"].tolist() == [[99, 11]]
  flag, state, npos = br.bench_match(**case)
  assert (flag == -1).all() and npos.tolist() == [1] and state.tolist() == [[-1, 0]] * 3


def test_minimum_region_size():
  case = br.min_region_case()
  assert case["pred_size"].tolist() == [99, 100] and case["gt_size"].tolist() == [100, 100]
  flag, state, npos = br.bench_match(**case)
  assert npos.tolist() == [2], "a 100-row ground truth is counted"
  assert _entries(flag, 0) == {0: [], 1: [1]} and state.tolist() == [[0, 1]]


def test_perfect_prediction_scores_one_at_every_threshold():
  sizes = [150, 400, 120, 300]
  gt = np.repeat(np.arange(4), sizes)
  pred = dict(instance=gt.copy(), inst_class=np.array([2, 2, 3, 3]), inst_scene=np.array([0, 0, 1, 1]), inst_score=np.array([0.9, 0.9, 0.4, 0.7]),
              scene_offsets=np.array([0, 550, 970]))
  ev = br.Evaluator(4)
  ev.step(pred, gt, np.repeat([2, 2, 3, 3], sizes))
  m = ev.compute_metrics()
  assert np.abs(m["ap"][:, 2:] - 1.0).max() <= 1e-12 and np.isnan(m["ap"][:, :2]).all()
  assert abs(m["AP"] - 1.0) <= 1e-12 and abs(m["AP50"] - 1.0) <= 1e-12 and abs(m["AP25"] - 1.0) <= 1e-12


def test_metrics_dict_nan_and_zero_classes():
  """Class 1 has no ground truth (NaN, left out of the means); class 2 has ground truth and no entry (0); class 3 is perfect."""
  sizes = [200, 300]
  gt = np.repeat(np.arange(2), sizes)
  pred = dict(instance=np.where(gt == 1, 0, -1), inst_class=np.array([3]), inst_scene=np.array([0]), inst_score=np.array([0.5]),
              scene_offsets=np.array([0, 500]))
  ev = br.Evaluator(4, stuff_classes=(0,))
  ev.step(pred, gt, np.repeat([2, 3], sizes))
  m = ev.compute_metrics()
  assert m["n_gt"].tolist() == [0, 0, 1, 1]
  assert np.isnan(m["ap"][:, :2]).all() and (m["ap"][:, 2] == 0).all() and np.abs(m["ap"][:, 3] - 1).max() <= 1e-12
  assert abs(m["AP"] - 0.5) <= 1e-12 and abs(m["AP25"] - 0.5) <= 1e-12 and np.isnan(m["ap_class"][1]) and m["ap50_class"][2] == 0
  empty = br.Evaluator(4).compute_metrics()
  assert np.isnan(empty["AP"]) and np.isnan(empty["ap"]).all() and empty["n_gt"].tolist() == [0] * 4


def test_three_claims_fill_the_three_slots_and_the_chain_of_duplicates():
  flag, state, _ = br.bench_match(**br.triple_case())
  # at 0.25 prediction 3 (60 rows of each ground truth, iou 0.27) is never the first claimant: true at g0 (0.7 against 0.5),
  # false at g1 (against 0.9) and at g2 (a tie with prediction 2, the lower index wins)
  assert _entries(flag, 0) == {0: [0], 1: [1], 2: [1], 3: [1, 0, 0]} and state[0].tolist() == [1, 1, 1]
  assert _entries(flag, 2) == {0: [0], 1: [0], 2: [0], 3: [0]} and state[2].tolist() == [0, 0, 0], "iou 0.4 and 0.27 at 0.5"
  case = br.chain_case()
  flag, state, npos = br.bench_match(**case)
  t25 = case["thresholds"].index(0.25)
  assert npos.tolist() == [65] and (state[t25] == 1).all()
  assert [_entries(flag, t25)[p] for p in range(6)] == [[1], [0, 1], [0], [1, 1], [1], [0, 1]]
