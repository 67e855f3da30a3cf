"""numpy restatement of the benchmark protocol for instance masks (csrc/insbench.hip, downstream/insseg.py's
InstanceBenchmarkEvaluator) under exactly the rules of include/pcmi.h, as plain loops: the void overlap, the matching with
the claim rule, the entries, the average precision with its sum in the stated order, the carry of instance ids onto the
original vertices (brute-force nearest from tests/nearest_ref.py) and the metrics dict.  Like the rules themselves it is
restated from the rules of ScanNet's script and was never run against the script.  numpy never contracts a product and a
sum, so every float64 operation below is rounded on its own."""
import warnings

import numpy as np

import nearest_ref as nr

BENCHMARK_THRESHOLDS = tuple(float(t) for t in np.append(np.arange(0.5, 0.95, 0.05), 0.25))


def overlap(pred, gt, P, G):
  """-> inter int32 [P, G], pred_size [P], gt_size [G]: ids outside their range count nowhere."""
  pred, gt = np.asarray(pred).astype(np.int64), np.asarray(gt).astype(np.int64)
  pv, gv = (pred >= 0) & (pred < P), (gt >= 0) & (gt < G)
  inter = np.bincount(pred[pv & gv] * G + gt[pv & gv], minlength=P * G).reshape(P, G) if P * G else np.zeros((P, G), np.int64)
  return inter.astype(np.int32), np.bincount(pred[pv], minlength=P)[:P].astype(np.int32), np.bincount(gt[gv], minlength=G)[:G].astype(np.int32)


def void_overlap(pred, gt, gt_valid, P):
  """-> void_inter int32 [P]: the rows of each prediction whose ground-truth id is outside [0, G) or has gt_valid == 0."""
  gt_valid = np.asarray(gt_valid)
  G = len(gt_valid)
  out = np.zeros(P, np.int32)
  for p, g in zip(np.asarray(pred).tolist(), np.asarray(gt).tolist()):
    if 0 <= p < P and (not 0 <= g < G or gt_valid[g] == 0):
      out[p] += 1
  return out


def iou(inter, gs, ps):
  return np.float64(inter) / np.float64(int(gs) + int(ps) - int(inter))


def bench_match(inter, pred_size, gt_size, void_inter, pred_scene, pred_class, pred_score, gt_scene, gt_class, B, Cls, thresholds,
                min_region=100):
  """-> entry_flag int8 [T, P, 3], gt_state int32 [T, G], npos int32 [Cls]."""
  inter = np.asarray(inter)
  P, G = inter.shape
  T = len(thresholds)
  flag = np.full((T, P, 3), -1, np.int8)
  state = np.full((T, G), -1, np.int32)
  npos = np.zeros(Cls, np.int32)
  kept = [p for p in range(P) if 0 <= pred_class[p] < Cls and 0 <= pred_scene[p] < B and pred_size[p] >= min_region]
  in_unit = [g for g in range(G) if 0 <= gt_class[g] < Cls and 0 <= gt_scene[g] < B]
  counted = [g for g in in_unit if gt_size[g] >= min_region]
  for g in counted:
    npos[gt_class[g]] += 1
  same = lambda p, g: pred_scene[p] == gt_scene[g] and pred_class[p] == gt_class[g]  # noqa: E731
  for ti, th in enumerate(thresholds):
    th = np.float64(th)
    used = np.zeros(P, np.int64)
    for b in range(B):
      for c in range(Cls):
        visited = set()
        for g in counted:
          if gt_scene[g] != b or gt_class[g] != c:
            continue
          claim = [p for p in kept if same(p, g) and inter[p, g] > 0 and p not in visited and used[p] < 3 and
                   iou(inter[p, g], gt_size[g], pred_size[p]) > th]
          state[ti, g] = 1 if claim else 0
          if not claim:
            continue
          visited.add(claim[0])
          best, best_s = None, -np.inf
          for p in claim:  # ascending: a later p wins only with a strictly higher score
            if best is None and pred_score[p] == best_s or pred_score[p] > best_s:
              best, best_s = p, pred_score[p]
          for p in claim:
            flag[ti, p, used[p]] = 1 if p == best else 0
            used[p] += 1
    for p in kept:
      mine = [g for g in in_unit if same(p, g)]
      if any(inter[p, g] > 0 and iou(inter[p, g], gt_size[g], pred_size[p]) > th for g in mine):
        continue
      ignore = int(void_inter[p]) + sum(int(inter[p, g]) for g in mine if gt_size[g] < min_region)
      if np.float64(ignore) / np.float64(int(pred_size[p])) <= th:
        flag[ti, p, 0] = 0
  return flag, state, npos


def ap_one(flags, scores, npos, curve=None):
  """The closed form of one (class, threshold): flags / scores in list order (descending score), flags of -1 skipped.
  curve: (prec, rec) views of the same length, filled at the last entry of each group."""
  if npos <= 0:
    return np.nan
  npos = np.float64(npos)
  pts, ends = [(0, 0)], []  # point j = (tp, n) after group j; ends[j - 1] = the position of group j's last entry
  tp = n = 0
  prev = None
  for i, (f, s) in enumerate(zip(flags, scores)):
    if f < 0:
      continue
    if prev is not None and s != scores[prev]:
      pts.append((tp, n))
      ends.append(prev)
    tp, n, prev = tp + (f > 0), n + 1, i
  if prev is not None:
    pts.append((tp, n))
    ends.append(prev)
  m = len(pts) - 1
  P = [np.float64(1.0)] + [np.float64(t) / np.float64(k) for t, k in pts[1:]]
  R = [np.float64(t) / npos for t, _ in pts]
  if curve is not None:
    for j, e in enumerate(ends, 1):
      curve[0][e], curve[1][e] = P[j], R[j]
  ap = np.float64(0.0)
  for j in range(m + 1):
    r_prev = R[j - 1] if j > 0 else np.float64(0.0)
    r_next = R[min(j + 1, m)]
    ap = ap + P[j] * (np.float64(0.5) * (r_next - r_prev))
  return ap


def bench_ap(entry_flag, score, cls_offs, npos):
  """-> ap [T, Cls], prec, rec [T, E] (NaN where no group ends)."""
  entry_flag = np.asarray(entry_flag)
  T, E = entry_flag.shape
  Cls = len(npos)
  ap = np.full((T, Cls), np.nan)
  prec, rec = np.full((T, E), np.nan), np.full((T, E), np.nan)
  for t in range(T):
    for c in range(Cls):
      a, b = int(cls_offs[c]), int(cls_offs[c + 1])
      ap[t, c] = ap_one(entry_flag[t, a:b], np.asarray(score)[a:b], int(npos[c]), (prec[t, a:b], rec[t, a:b]))
  return ap, prec, rec


def metrics(ap, n_gt, thresholds):
  """The metrics dict from ap [T, classes] with NaN where a class has no counted ground truth."""
  ap = np.array(ap, dtype=np.float64)
  ap[:, np.asarray(n_gt) == 0] = np.nan
  thr = np.asarray(thresholds, dtype=np.float64)
  C = ap.shape[1]
  rest = ~np.isclose(thr, 0.25)

  def at(t):
    hit = np.flatnonzero(np.isclose(thr, t))
    return ap[hit[0]] if len(hit) else np.full(C, np.nan)

  with warnings.catch_warnings():
    warnings.simplefilter("ignore", category=RuntimeWarning)
    ap_class = ap[rest].mean(0) if rest.any() else np.full(C, np.nan)
    return dict(AP=float(np.nanmean(ap_class)), AP50=float(np.nanmean(at(0.5))), AP25=float(np.nanmean(at(0.25))), ap_class=ap_class,
                ap50_class=at(0.5), ap25_class=at(0.25), n_gt=np.asarray(n_gt).astype(np.int64), ap=ap)


def carry_instances(coords, voxel_instance, transformation, points, point_offsets):
  """The voxels' instance ids on the original vertices: a stable sort of the voxels by batch index, their centres, the
  nearest centre of the vertex's scene (the lowest row among equals), -1 where there is none."""
  coords, vi = np.asarray(coords), np.asarray(voxel_instance)
  T = np.asarray(transformation, dtype=np.float64).reshape(-1, 16)
  B = len(T)
  order = np.argsort(coords[:, 0], kind="stable")
  c, vi = coords[order], vi[order]
  ref_offs = np.searchsorted(c[:, 0], np.arange(B + 1))
  centers = nr.voxel_centers(c, np.linalg.inv(T.reshape(-1, 4, 4)).reshape(-1, 16))
  idx, _ = nr.nearest_point(centers, ref_offs, points, point_offsets)
  return np.where(idx >= 0, vi[np.maximum(idx, 0)] if len(vi) else -1, -1).astype(np.int32)


class Evaluator:
  """InstanceBenchmarkEvaluator in numpy: step / step_points / compute_metrics with the same arguments (host arrays)."""

  def __init__(self, num_labels, stuff_classes=(0, 1), min_region=100, thresholds=BENCHMARK_THRESHOLDS):
    self.C, self.stuff, self.min_region, self.thr = num_labels, tuple(stuff_classes), min_region, tuple(thresholds)
    self.flag, self.cls, self.score, self.npos = [], [], [], np.zeros(num_labels, np.int64)

  def step(self, pred, gt_instance, gt_class, n_instances=None):
    gi, gc = np.asarray(gt_instance).astype(np.int64), np.asarray(gt_class).astype(np.int64)
    G = int(n_instances) if n_instances is not None else (int(gi.max()) + 1 if len(gi) else 0)
    G = max(G, 0)
    offs = np.asarray(pred["scene_offsets"])
    B = len(offs) - 1
    row_scene = np.searchsorted(offs, np.arange(len(gi)), side="right") - 1
    cls, scene = np.full(G, -1, np.int64), np.full(G, -1, np.int64)
    for g in range(G):
      rows = gi == g
      if rows.any():
        cls[g], scene[g] = max(gc[rows].max(), -1), max(row_scene[rows].max(), -1)
    scored = (cls >= 0) & (cls < self.C) & ~np.isin(cls, self.stuff)
    cls = np.where(scored, cls, -1)
    P = len(pred["inst_class"])
    inter, ps, gs = overlap(pred["instance"], gi, P, G)
    void = void_overlap(pred["instance"], gi, scored, P)
    score = np.asarray(pred["inst_score"], dtype=np.float64)
    score = np.where(np.isfinite(score), score, 0.0)
    flag, self.last_state, npos = bench_match(inter, ps, gs, void, pred["inst_scene"], pred["inst_class"], score, scene, cls, B, self.C,
                                              self.thr, self.min_region)
    self.npos += npos
    self.flag.append(flag)
    self.cls.append(np.asarray(pred["inst_class"]).astype(np.int64))
    self.score.append(score)

  def step_points(self, coords, pred, transformation, points, point_instance, point_class, point_offsets):
    inst = carry_instances(coords, pred["instance"], transformation, points, point_offsets)
    self.step(dict(pred, instance=inst, scene_offsets=np.asarray(point_offsets)), point_instance, point_class)
    return inst

  def lists(self):
    """-> entry_flag [T, E], score [E], cls_offs [C + 1] in the evaluator's list order."""
    flag, cls, score = np.concatenate(self.flag, 1), np.concatenate(self.cls), np.concatenate(self.score)
    cls = np.where((cls >= 0) & (cls < self.C), cls, self.C)
    by_score = np.argsort(-score, kind="stable")
    order = by_score[np.argsort(cls[by_score], kind="stable")]
    cls_offs = 3 * np.searchsorted(cls[order], np.arange(self.C + 1))
    return flag[:, order, :].reshape(len(self.thr), -1), np.repeat(score[order], 3), cls_offs

  def compute_metrics(self):
    if not self.flag:
      return metrics(np.full((len(self.thr), self.C), np.nan), np.zeros(self.C, np.int64), self.thr)
    ap, _, _ = bench_ap(*self.lists(), self.npos)
    return metrics(ap, self.npos, self.thr)


def same_metrics(a, b):
  """Two metrics dicts hold the same bits (NaN equal to NaN)."""
  if set(a) != set(b):
    return False
  return all(np.array_equal(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64), equal_nan=True) for k in a)


# ---- the cases the CPU and the GPU tests share ------------------------------------------------------------------------------
def two_gt_case(scores):
  """Ground truths of 100 and 100 rows; prediction 0 = 60 rows of g0, prediction 1 = 40 rows of g0 and 40 of g1:
  iou(p0, g0) = 60 / 100, iou(p1, g0) = iou(p1, g1) = 40 / 140 = 0.286.  Predictions of 60 and 80 rows are scored only with a
  minimum region below them: min_region = 50.  -> the arguments of bench_match as a dict."""
  gt = np.concatenate([np.zeros(100), np.ones(100)]).astype(np.int64)
  pred = np.full(200, -1, np.int64)
  pred[:60] = 0
  pred[60:100] = 1
  pred[100:140] = 1
  return match_args(pred, gt, [0, 0], [0, 0], scores, [0, 0], [0, 0], 1, 1, (0.25, 0.5), 50)


def void_case(where, n_void=62):
  """One prediction of 100 rows without any match: n_void of its rows on `where` ('void': rows without instance; 'small': a
  99-row ground truth of its class), the rest spread thinly over a 1000-row ground truth (iou 0.04)."""
  gt = np.concatenate([np.zeros(1000), np.ones(99), np.full(100, -1)]).astype(np.int64)
  pred = np.full(len(gt), -1, np.int64)
  pred[:100 - n_void] = 0
  start = 1099 if where == "void" else 1000
  pred[start:start + n_void] = 0
  return match_args(pred, gt, [0], [0], [0.7], [0, 0], [0, 0], 1, 1, BENCHMARK_THRESHOLDS, 100)


def small_only_case():
  """A prediction of 110 rows, 99 of them a small ground truth (iou 0.9) and 11 on a 300-row one: it emits nothing."""
  gt = np.concatenate([np.zeros(99), np.ones(300)]).astype(np.int64)
  pred = np.full(len(gt), -1, np.int64)
  pred[:110] = 0
  return match_args(pred, gt, [0], [0], [0.9], [0, 0], [0, 0], 1, 1, (0.25, 0.5, 0.75), 100)


def min_region_case():
  """A 99-row prediction (dropped) on one 100-row ground truth, a 100-row prediction (kept) equal to another."""
  gt = np.concatenate([np.zeros(100), np.ones(100)]).astype(np.int64)
  pred = np.full(200, -1, np.int64)
  pred[:99] = 0
  pred[100:200] = 1
  return match_args(pred, gt, [0, 0], [0, 0], [0.9, 0.8], [0, 0], [0, 0], 1, 1, (0.5,), 100)


def match_args(pred, gt, pred_scene, pred_class, pred_score, gt_scene, gt_class, B, Cls, thresholds, min_region):
  """The arguments of bench_match from rows: overlap and void overlap (gt_valid = gt_class >= 0) computed here."""
  P, G = len(pred_scene), len(gt_scene)
  gt_class = np.asarray(gt_class, dtype=np.int32)
  inter, ps, gs = overlap(pred, gt, P, G)
  return dict(inter=inter, pred_size=ps, gt_size=gs, void_inter=void_overlap(pred, gt, gt_class >= 0, P),
              pred_scene=np.asarray(pred_scene, dtype=np.int32), pred_class=np.asarray(pred_class, dtype=np.int32),
              pred_score=np.asarray(pred_score, dtype=np.float64), gt_scene=np.asarray(gt_scene, dtype=np.int32), gt_class=gt_class, B=B,
              Cls=Cls, thresholds=tuple(thresholds), min_region=min_region)


def random_rows(seed, B, Cls, G, P, sizes=(40, 260), unscored=0.1, foreign=0.15):
  """Rows of G ground-truth instances (scene-major; a share `unscored` of class -1) cut into one to three pieces each; a piece
  goes to a new prediction of the instance's scene (of its class, or with probability `foreign` of a random one), to the
  prediction before it (which then spans two instances) or to none; some rows without instance follow each instance.  Scores
  are multiples of 1 / 8: ties.  -> pred [n], gt [n], pred_scene, pred_class, pred_score [P], gt_scene, gt_class [G]."""
  rng = np.random.default_rng(seed)
  g_scene = np.sort(rng.integers(0, B, G))
  g_class = np.where(rng.random(G) < unscored, -1, rng.integers(0, Cls, G))
  p_scene, p_class = np.full(P, -1, np.int64), np.full(P, -1, np.int64)
  pred, gt, n_p, last = [], [], 0, -1
  for g in range(G):
    size = int(rng.integers(sizes[0], sizes[1]))
    cuts = np.sort(rng.integers(0, size + 1, int(rng.integers(0, 3))))
    for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [size]])):
      r = rng.random()
      if r < 0.3 and last >= 0 and p_scene[last] == g_scene[g]:
        p = last
      elif r < 0.9 and n_p < P:
        p, n_p = n_p, n_p + 1
        p_scene[p] = g_scene[g]
        p_class[p] = g_class[g] if rng.random() >= foreign else rng.integers(-1, Cls + 1)
      else:
        p = -1
      pred += [p] * int(b - a)
      gt += [g] * int(b - a)
      last = p if p >= 0 else last
    k = int(rng.integers(0, 60))
    pred += [last if rng.random() < 0.7 else -1] * k
    gt += [-1] * k
  return (np.array(pred, np.int64), np.array(gt, np.int64), p_scene, p_class, rng.integers(0, 9, P) / 8.0, g_scene, g_class)


def chain_case(pairs=32):
  """two_gt_case `pairs` times in ONE scene and class, the score order (0.9, 0.8), (0.8, 0.9), (0.8, 0.8) in turn, then one
  exact prediction of a 100-row ground truth: P = G = 2 pairs + 1 (65: one prediction beyond a wave's 64 lanes)."""
  pred, gt, score = [], [], []
  for k in range(pairs):
    gt += [2 * k] * 100 + [2 * k + 1] * 100
    pred += [2 * k] * 60 + [2 * k + 1] * 80 + [-1] * 60
    score += [(0.9, 0.8), (0.8, 0.9), (0.8, 0.8)][k % 3]
  gt += [2 * pairs] * 100
  pred += [2 * pairs] * 100
  score += [0.5]
  z = [0] * (2 * pairs + 1)
  return match_args(np.array(pred), np.array(gt), z, z, score, z, z, 1, 1, BENCHMARK_THRESHOLDS + (0.3,), 50)


def triple_case():
  """Three 100-row ground truths; predictions 0 - 2 hold 40 rows of one each (iou 0.4), prediction 3 the other 60 rows of all
  three (iou 60 / 220 = 0.27): never the first claimant, it claims three times at 0.25 -- all three slots."""
  gt = np.repeat([0, 1, 2], 100)
  pred = np.concatenate([[k] * 40 + [3] * 60 for k in range(3)])
  return match_args(pred, gt, [0] * 4, [0] * 4, [0.5, 0.9, 0.7, 0.7], [0] * 3, [0] * 3, 1, 1, (0.25, 0.3, 0.5), 40)
