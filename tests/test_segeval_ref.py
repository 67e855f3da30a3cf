"""tests/segeval_ref.py -- the float64 restatement the device tests of the segmentation validation compare against -- held to
its sources on the CPU: scikit-learn's average_precision_score + label_binarize (what the reference's average_precision calls),
torch's cross_entropy(ignore_index), and what the reference's own precision_at_one / fast_hist / per_class_iu /
average_precision / AverageMeter returned (tests/golden/golden_segeval.npz, written by tests/golden/make_golden_segeval.py).

Tolerances: AP within 1e-12 (float64 sums of at most n = 3000 terms <= 1, n 2^-53 = 3e-13); loss within 1e-12 relative
(float64 on both sides); predictions, counts and the confusion matrix exactly."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import segeval_ref as S  # noqa: E402
import make_golden_segeval as mk  # noqa: E402

G = np.load(mk.PATH)
TOL = 1e-12


def _case(seed=3, n=3000, c=7, ignored=0.1, empty=2):
  """The issue's check: a 37-row pool of logits in multiples of 0.5, n rows, c classes, 10 % ignored, one class empty."""
  rng = np.random.RandomState(seed)
  logits, _, _ = S.pool_rows(rng, 37, c, n)
  t = rng.randint(0, c - 1, n)
  t[t >= empty] += 1
  t[rng.rand(n) < ignored] = 255
  return logits, t


def test_average_precision_equals_sklearn():
  pytest.importorskip("sklearn")
  from sklearn.metrics import average_precision_score
  from sklearn.preprocessing import label_binarize
  for seed, n, c, empty in [(3, 3000, 7, 2), (4, 501, 3, 0), (5, 64, 13, 12)]:
    logits, t = _case(seed, n, c, empty=empty)
    prob = S.softmax(logits)
    mine = S.average_precision(prob, t)
    with warnings.catch_warnings():
      warnings.simplefilter("ignore")
      ref = average_precision_score(label_binarize(t, classes=list(range(c))), prob, average=None)
    npos = np.array([(t == k).sum() for k in range(c)])
    assert npos[empty] == 0 and (npos > 0).sum() >= 2
    assert np.isnan(mine[npos == 0]).all(), "a class without a positive row scores NaN"
    err = np.abs(mine - ref)[npos > 0].max()
    print("seed %d: |restatement - sklearn| = %.2e" % (seed, err))
    assert err <= TOL
  # continuous scores (no ties), and every score equal (one threshold: ap = npos / n)
  rng = np.random.RandomState(0)
  prob, t = rng.rand(400, 3), rng.randint(0, 3, 400)
  ref = average_precision_score(label_binarize(t, classes=[0, 1, 2]), prob, average=None)
  assert np.abs(S.average_precision(prob, t) - ref).max() <= TOL
  flat = np.full((400, 3), 0.25)
  assert np.abs(S.average_precision(flat, t) - np.array([(t == k).mean() for k in range(3)])).max() <= TOL
  assert np.abs(average_precision_score(label_binarize(t, classes=[0, 1, 2]), flat, average=None) - S.average_precision(flat, t)).max() <= TOL


def test_ap_does_not_depend_on_the_order_inside_ties():
  logits, t = _case(8, 700, 5, empty=1)
  prob = S.softmax(logits)
  base = S.average_precision(prob, t)
  perm = np.random.RandomState(1).permutation(len(t))
  again = S.average_precision(prob[perm], t[perm])
  ok = ~np.isnan(base)
  assert np.array_equal(np.isnan(base), np.isnan(again)) and np.abs(base - again)[ok].max() <= TOL


def test_cross_entropy_equals_torch():
  for seed, n, c in [(3, 3000, 7), (4, 333, 13), (5, 1, 2)]:
    logits, t = _case(seed, n, c, empty=0)
    s, counted = S.cross_entropy_rows(logits, t, 255)
    if counted == 0:
      continue
    ref = float(torch.nn.functional.cross_entropy(torch.from_numpy(logits).double(), torch.from_numpy(t), ignore_index=255))
    assert counted == int((t != 255).sum()) and abs(s / counted - ref) <= TOL * abs(ref)
  assert S.cross_entropy_rows(logits, np.full(len(t), 255), 255) == (0.0, 0)
  bad = np.array([0, 9, 255])
  s, counted = S.cross_entropy_rows(np.zeros((3, 4), np.float32), bad, 255)
  assert np.isnan(s) and counted == 2
  with pytest.raises((IndexError, RuntimeError)):
    torch.nn.functional.cross_entropy(torch.zeros(3, 4), torch.from_numpy(bad), ignore_index=255)


def test_softmax_rows_and_argmax_ties():
  logits, _ = _case(6, 500, 7)
  p = S.softmax(logits)
  ref = torch.softmax(torch.from_numpy(logits).double(), 1).numpy()
  assert np.abs(p - ref).max() <= 1e-15 and np.abs(p.sum(1) - 1).max() <= 1e-15
  u, inv = np.unique(logits, axis=0, return_inverse=True)
  assert np.array_equal(p, p[[np.flatnonzero(inv.reshape(-1) == i)[0] for i in inv.reshape(-1)]]), "equal rows, bit-equal probabilities"
  x = np.array([[1.0, 3.0, 3.0, 2.0], [0.5, 0.5, 0.5, 0.5], [-1.0, -2.0, -1.0, -3.0]], np.float32)
  assert S.argmax_lowest(x).tolist() == [1, 0, 0]


def test_against_the_reference_recorded_outputs():
  logits, t, c = G["logits"], G["target"], G["logits"].shape[1]
  pred = S.argmax_lowest(logits)
  assert np.array_equal(pred, G["pred"])
  assert np.array_equal(S.fast_hist(pred, t, c), G["hist"])
  assert np.array_equal(np.isnan(S.per_class_iu(G["hist"])), np.isnan(G["iou"]))
  ok = ~np.isnan(G["iou"])
  assert np.abs(S.per_class_iu(G["hist"]) - G["iou"])[ok].max() <= TOL
  counted = int((t != 255).sum())
  # precision_at_one goes through float32 (correct.float().sum(0).mul(100.0 / n).item())
  assert abs(100.0 * S.correct_rows(pred, t, 255) / counted - float(G["score"])) <= 1e-5 * float(G["score"])
  assert np.array_equal(S.softmax(logits), G["prob"])
  mine, npos = S.average_precision(G["prob"], t), G["npos"]
  assert np.array_equal(npos, [(t == k).sum() for k in range(c)]) and (npos == 0).sum() == 1
  assert np.isnan(mine[npos == 0]).all() and np.abs(mine - G["ap"])[npos > 0].max() <= TOL


def test_accumulation_against_the_reference_recorded_outputs():
  acc, lo = S.Accumulator(G["logits"].shape[1], 255), 0
  for n in G["batches"]:
    acc.step(G["logits"][lo:lo + n], G["target"][lo:lo + n])
    lo += int(n)
  acc.step(np.zeros((0, 7), np.float32), np.zeros(0, np.int64))  # an empty batch is no batch
  m = acc.metrics()
  assert np.array_equal(m["hist"], G["acc_hist"])
  assert abs(m["loss"] - float(G["acc_loss"])) <= TOL * float(G["acc_loss"])
  assert abs(m["score"] - float(G["acc_score"])) <= 1e-5 * float(G["acc_score"])  # (float32 in precision_at_one)
  assert abs(m["mIoU"] - float(G["acc_miou"])) <= 1e-10
  scored = G["acc_npos"] > 0
  ref_aps = np.where(scored, G["acc_aps"], np.nan)  # the reference's scikit-learn gave NaN where there is no positive
  assert np.array_equal(np.isnan(acc.aps), ~scored) and np.abs(acc.aps - ref_aps)[scored].max() <= TOL
  with warnings.catch_warnings():
    warnings.simplefilter("ignore", category=RuntimeWarning)
    ref_class = np.nanmean(ref_aps, 0) * 100
  ok = ~np.isnan(ref_class)
  assert np.array_equal(np.isnan(m["ap_class"]), ~ok) and np.abs(m["ap_class"] - ref_class)[ok].max() <= 1e-10
  assert abs(m["mAP"] - np.nanmean(ref_class)) <= 1e-10
  # a batch without a counted row adds nothing to the averages; its rows still enter the histogram rule (none is a class)
  before = (acc.loss_sum, acc.score_sum, acc.count)
  acc.step(G["logits"][:5], np.full(5, 255))
  assert (acc.loss_sum, acc.score_sum, acc.count) == before and np.array_equal(acc.hist, G["acc_hist"])
