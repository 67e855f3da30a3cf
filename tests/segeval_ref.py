"""numpy float64 restatement of one validation step of the segmentation fine-tuning, in this project's own words: what test() of
the reference's downstream/semseg/lib/test.py:62-196 computes per batch (softmax, CrossEntropyLoss(ignore_index), get_prediction,
precision_at_one, fast_hist, average_precision = label_binarize + sklearn's average_precision_score(average=None)) and how it
accumulates over batches (two AverageMeters weighted by the number of rows, the summed confusion matrix, np.nanmean over the
batches' per-class AP).  tests/test_segeval_ref.py holds it to scikit-learn, to torch and to the reference's recorded outputs;
tests/test_gpu_segeval.py compares the device against it.

Where it departs from the reference, as the device code does: a class without a positive row scores NaN in
that batch; a batch without a counted row adds nothing to the loss and score averages.
"""
import numpy as np


def softmax(logits):
  """float64 softmax of the rows of logits [n, c].  Computed once per DISTINCT row, so equal rows give bit-equal probabilities
  whatever position they stand at."""
  x = np.asarray(logits, np.float64).reshape(len(logits), -1)
  if len(x) == 0:
    return x.copy()
  u, inv = np.unique(x, axis=0, return_inverse=True)
  e = np.exp(u - u.max(1, keepdims=True))
  return (e / e.sum(1, keepdims=True))[inv.reshape(-1)]


def argmax_lowest(logits):
  """get_prediction: the arg-max of every row, the lowest class among equal logits (np.argmax returns the first)."""
  return np.argmax(np.asarray(logits, np.float64), axis=1).astype(np.int64)


def cross_entropy_rows(logits, target, ignore_label):
  """(sum over the counted rows of logsumexp(x) - x[label], number of counted rows): a row counts iff label != ignore_label;
  a counted label outside [0, c) makes the sum NaN (torch raises for it)."""
  x, t = np.asarray(logits, np.float64), np.asarray(target, np.int64)
  c = x.shape[1]
  keep = t != ignore_label
  if not keep.any():
    return 0.0, 0
  if ((t[keep] < 0) | (t[keep] >= c)).any():
    return float("nan"), int(keep.sum())
  xs = x[keep]
  m = xs.max(1)
  lse = m + np.log(np.exp(xs - m[:, None]).sum(1))
  return float((lse - xs[np.arange(len(xs)), t[keep]]).sum()), int(keep.sum())


def correct_rows(pred, target, ignore_label):
  """Number of rows with label != ignore_label and pred == label (the numerator of precision_at_one)."""
  p, t = np.asarray(pred, np.int64), np.asarray(target, np.int64)
  return int(((p == t) & (t != ignore_label)).sum())


def fast_hist(pred, target, c):
  """hist[label, pred] over the rows with 0 <= label < c."""
  p, t = np.asarray(pred, np.int64), np.asarray(target, np.int64)
  k = (t >= 0) & (t < c)
  return np.bincount(c * t[k] + p[k], minlength=c * c).reshape(c, c).astype(np.int64)


def per_class_iu(hist):
  h = np.asarray(hist, np.float64)
  with np.errstate(divide="ignore", invalid="ignore"):
    return np.diag(h) / (h.sum(1) + h.sum(0) - np.diag(h))


def ap_sorted(sorted_scores, positive_sorted):
  """Average precision of ONE class from its scores in descending order and the positive flag of each sorted element: with
  tp = the positives among the first `rank` elements, at the last element of every run of equal scores P = tp / rank and
  R = tp / npos; ap = sum (R - R_prev) P.  NaN without a positive."""
  s, pos = np.asarray(sorted_scores), np.asarray(positive_sorted, bool)
  npos = int(pos.sum())
  if npos == 0:
    return float("nan")
  end = np.ones(len(s), bool)
  end[:-1] = s[1:] != s[:-1]
  tp = np.cumsum(pos)[end].astype(np.float64)
  rank = (np.flatnonzero(end) + 1).astype(np.float64)
  rec = tp / npos
  return float(np.sum((rec - np.concatenate([[0.0], rec[:-1]])) * (tp / rank)))


def average_precision(prob, target):
  """Per-class AP of prob [n, c] against target [n]: class k's positives are the rows with label k, every other row (ignored
  and out-of-range labels too) is a negative.  float64 [c], NaN for a class without a positive."""
  p, t = np.asarray(prob), np.asarray(target, np.int64)
  out = np.full(p.shape[1], np.nan)
  for k in range(p.shape[1]):
    order = np.argsort(-p[:, k], kind="stable")
    out[k] = ap_sorted(p[order, k], t[order] == k)
  return out


class Accumulator:
  """The running state of test(): step(logits, target) per batch, metrics() at the end."""

  def __init__(self, num_labels, ignore_label=255):
    self.c, self.ignore = int(num_labels), int(ignore_label)
    self.hist = np.zeros((self.c, self.c), np.int64)
    self.loss_sum = self.score_sum = self.count = 0.0
    self.aps = np.zeros((0, self.c))

  def step(self, logits, target):
    x, t = np.asarray(logits, np.float64), np.asarray(target, np.int64)
    n = len(x)
    if n == 0:
      return
    pred = argmax_lowest(x)
    loss, counted = cross_entropy_rows(x, t, self.ignore)
    if counted > 0:
      self.loss_sum += n * (loss / counted)
      self.score_sum += n * (100.0 * correct_rows(pred, t, self.ignore) / counted)
      self.count += n
    self.hist += fast_hist(pred, t, self.c)
    self.aps = np.vstack([self.aps, average_precision(softmax(x), t)])

  def metrics(self):
    import warnings
    ious = per_class_iu(self.hist) * 100.0
    with np.errstate(divide="ignore", invalid="ignore"), warnings.catch_warnings():
      warnings.simplefilter("ignore", category=RuntimeWarning)
      acc = np.diag(self.hist) / self.hist.sum(1) * 100.0
      ap_class = np.nanmean(self.aps, 0) * 100.0 if len(self.aps) else np.full(self.c, np.nan)
      means = dict(mIoU=float(np.nanmean(ious)), mAP=float(np.nanmean(ap_class)), mAcc=float(np.nanmean(acc)))
    return dict(loss=self.loss_sum / self.count if self.count else 0.0, score=self.score_sum / self.count if self.count else 0.0,
                ious=ious, ap_class=ap_class, acc=acc, hist=self.hist.copy(), **means)


def pool_rows(rng, n_pool, c, n, spread=6):
  """(logits float32 [n, c], pool index [n], pool float32 [n_pool, c]): n rows drawn from a pool of n_pool distinct rows whose
  entries are multiples of 0.5 -- exact in float32, so equal rows are equal on every side and ties between rows are exact."""
  while True:
    pool = (rng.randint(-spread, spread + 1, (n_pool, c)) * 0.5).astype(np.float32)
    if len(np.unique(pool, axis=0)) == n_pool:
      break
  idx = rng.randint(0, n_pool, n)
  return pool[idx], idx, pool
