"""numpy float64 restatement of the detection scoring, in this project's own words: the oriented box overlap (box3d_iou of the
reference's lib/utils/box_util.py, without scipy), the matching rule, eval_det_cls / eval_det and both voc_ap forms of
lib/utils/eval_det.py, and the metrics dict of APCalculator.compute_metrics.  tests/test_ap_ref.py holds it to the reference's
own outputs (tests/golden/golden_ap.npz); tests/test_gpu_ap.py holds the kernels of csrc/evaldet.hip to it."""
import numpy as np

EPS64 = np.finfo(np.float64).eps


# ---- overlap ------------------------------------------------------------------------------------------------------------------
def clip_polygon(subject, clip):
  """Sutherland-Hodgman: the part of `subject` (list of (x, y)) on the strict inner side of every edge of the convex,
  counter-clockwise `clip`; None once nothing is left.  Vertex order and expressions as the reference's polygon_clip."""
  out = list(subject)
  a = clip[-1]
  for b in clip:
    src, out = out, []
    ex, ey = b[0] - a[0], b[1] - a[1]
    inside = lambda p: ex * (p[1] - a[1]) > ey * (p[0] - a[0])  # noqa: E731
    s = src[-1]
    for e in src:
      if inside(e) != inside(s):
        dcx, dcy = a[0] - b[0], a[1] - b[1]
        dpx, dpy = s[0] - e[0], s[1] - e[1]
        n1 = a[0] * b[1] - a[1] * b[0]
        n2 = s[0] * e[1] - s[1] * e[0]
        n3 = 1.0 / (dcx * dpy - dcy * dpx)
        out.append(((n1 * dpx - n2 * dcx) * n3, (n1 * dpy - n2 * dcy) * n3))
      if inside(e):
        out.append(e)
      s = e
    a = b
    if not out:
      return None
  return out


def polygon_area(p):
  x, y = np.array([v[0] for v in p], np.float64), np.array([v[1] for v in p], np.float64)
  return 0.5 * abs(np.dot(x, np.roll(y, 1)) - np.dot(y, np.roll(x, 1)))


def box_volume(c):
  return np.linalg.norm(c[0] - c[1]) * np.linalg.norm(c[1] - c[2]) * np.linalg.norm(c[0] - c[4])


def box3d_iou(c1, c2):
  """(iou3d, iou2d) of two boxes given as corners [8, 3] in get_3d_box's order."""
  c1, c2 = np.asarray(c1, np.float64), np.asarray(c2, np.float64)
  r1 = [(c1[i, 0], c1[i, 2]) for i in (3, 2, 1, 0)]
  r2 = [(c2[i, 0], c2[i, 2]) for i in (3, 2, 1, 0)]
  a1, a2 = polygon_area(r1), polygon_area(r2)
  inter = clip_polygon(r1, r2)
  ia = polygon_area(inter) if inter is not None else 0.0  # the polygon is convex: its area is its hull's
  iou2d = ia / (a1 + a2 - ia)
  iv = ia * max(0.0, min(c1[0, 1], c2[0, 1]) - max(c1[4, 1], c2[4, 1]))
  return iv / (box_volume(c1) + box_volume(c2) - iv), iou2d


def iou_matrix(A, B):
  """(iou3d [n, m], iou2d [n, m]) of corners A [n, 8, 3] against B [m, 8, 3]."""
  o3, o2 = np.zeros((len(A), len(B))), np.zeros((len(A), len(B)))
  for i in range(len(A)):
    for j in range(len(B)):
      o3[i, j], o2[i, j] = box3d_iou(A[i], B[j])
  return o3, o2


def box_corners(size, angle, center):
  """get_3d_box: the corners [8, 3] of a box of size (l, w, h), heading `angle` about y, centred at `center`."""
  l, w, h = (float(v) for v in size)
  c, s = np.cos(angle), np.sin(angle)
  x = np.array([1, 1, -1, -1, 1, 1, -1, -1], np.float64) * (l / 2)
  y = np.array([1, 1, 1, 1, -1, -1, -1, -1], np.float64) * (h / 2)
  z = np.array([1, -1, -1, 1, 1, -1, -1, 1], np.float64) * (w / 2)
  return np.stack([c * x + s * z + center[0], y + center[1], -s * x + c * z + center[2]], axis=1)


# ---- matching -----------------------------------------------------------------------------------------------------------------
def match(iou, gt_cls, gt_mask, n_cls):
  """iou [K, G] -> (best_gt int [K, n_cls], best_iou [K, n_cls], second [K, n_cls]): per box and class the largest overlap
  with the valid boxes of that class, the lowest index of equal ones (-1 / -inf without any), and the runner-up overlap."""
  K, G = iou.shape
  best_gt = np.full((K, n_cls), -1, np.int64)
  best = np.full((K, n_cls), -np.inf)
  second = np.full((K, n_cls), -np.inf)
  for k in range(K):
    for g in range(G):
      if not gt_mask[g] or not 0 <= gt_cls[g] < n_cls:
        continue
      c, o = int(gt_cls[g]), iou[k, g]
      if o > best[k, c]:
        second[k, c] = best[k, c]
        best[k, c], best_gt[k, c] = o, g
      elif o > second[k, c]:
        second[k, c] = o
  return best_gt, best, second


# ---- curves -------------------------------------------------------------------------------------------------------------------
def voc_ap(rec, prec, use_07_metric=False):
  if use_07_metric:
    ap = 0.0
    for k in range(11):
      sel = rec >= k * 0.1
      ap = ap + (np.max(prec[sel]) if np.any(sel) else 0.0) / 11.0
    return ap
  mrec = np.concatenate(([0.0], rec, [1.0]))
  env = np.concatenate(([0.0], prec, [0.0]))
  for i in range(env.size - 1, 0, -1):
    env[i - 1] = np.maximum(env[i - 1], env[i])
  i = np.where(mrec[1:] != mrec[:-1])[0]
  return float(np.sum((mrec[i + 1] - mrec[i]) * env[i + 1]))


def curves(tp, npos):
  """(rec, prec) from the true-positive flags of a class's detections in rank order."""
  tp = np.asarray(tp, np.float64)
  t, f = np.cumsum(tp), np.cumsum(1.0 - tp)
  with np.errstate(invalid="ignore", divide="ignore"):
    return t / float(npos), t / np.maximum(t + f, EPS64)


def eval_class(pred, gt, thresh=0.25, use_07_metric=False, iou_fn=None):
  """One class.  pred: {scene: [(corners, score)]}, gt: {scene: [corners]} -> dict(order, tp, ovmax, jmax, second, rec, prec,
  ap, npos): the detections in descending confidence (equal ones in accumulation order: scenes in the dict's order, a
  scene's detections in list order); a detection whose best overlap exceeds thresh is a true positive if it is the first
  to claim that box."""
  iou_fn = iou_fn or (lambda a, b: box3d_iou(a, b)[0])
  scenes, boxes, conf = [], [], []
  for sid, dets in pred.items():
    for box, score in dets:
      scenes.append(sid)
      boxes.append(box)
      conf.append(score)
  order = np.argsort(-np.asarray(conf, np.float64), kind="stable")
  npos = sum(len(v) for v in gt.values())
  claimed = {sid: [False] * len(v) for sid, v in gt.items()}
  nd = len(order)
  tp, ovmax, jmax, second = np.zeros(nd, np.int64), np.full(nd, -np.inf), np.full(nd, -1, np.int64), np.full(nd, -np.inf)
  for r, d in enumerate(order):
    for j, g in enumerate(gt.get(scenes[d], [])):
      o = iou_fn(np.asarray(boxes[d], np.float64), np.asarray(g, np.float64))
      if o > ovmax[r]:
        second[r] = ovmax[r]
        ovmax[r], jmax[r] = o, j
      elif o > second[r]:
        second[r] = o
    if ovmax[r] > thresh and not claimed[scenes[d]][jmax[r]]:
      tp[r] = 1
      claimed[scenes[d]][jmax[r]] = True
  rec, prec = curves(tp, npos)
  return dict(order=order, tp=tp, ovmax=ovmax, jmax=jmax, second=second, rec=rec, prec=prec, ap=voc_ap(rec, prec, use_07_metric),
              npos=npos)


def split_classes(pred_all, gt_all):
  """{scene: [(class, corners, score)]}, {scene: [(class, corners)]} -> ({class: {scene: [(corners, score)]}},
  {class: {scene: [corners]}}); as in the reference every scene with a detection of a class gets an (empty) ground-truth
  entry of that class, and the classes are those of either dict."""
  pred, gt = {}, {}
  for sid, dets in pred_all.items():
    for c, box, score in dets:
      pred.setdefault(c, {}).setdefault(sid, []).append((box, score))
      gt.setdefault(c, {}).setdefault(sid, [])
  for sid, boxes in gt_all.items():
    for c, box in boxes:
      gt.setdefault(c, {}).setdefault(sid, []).append(box)
  return pred, gt


def eval_det(pred_all, gt_all, thresh=0.25, use_07_metric=False, iou_fn=None):
  """{class: eval_class result}; a class with ground truth and no detection scores ap 0 with empty curves."""
  pred, gt = split_classes(pred_all, gt_all)
  return {c: eval_class(pred.get(c, {}), gt[c], thresh, use_07_metric, iou_fn) for c in gt}


def metrics(results, class2type_map=None):
  """APCalculator.compute_metrics' dict from eval_det's results."""
  name = lambda c: class2type_map[c] if class2type_map else str(c)  # noqa: E731
  out = {}
  keys = sorted(results)
  for c in keys:
    out["%s Average Precision" % name(c)] = results[c]["ap"]
  out["mAP"] = np.mean([results[c]["ap"] for c in keys])
  recs = [results[c]["rec"][-1] if len(results[c]["rec"]) else 0 for c in keys]
  for c, r in zip(keys, recs):
    out["%s Recall" % name(c)] = r
  out["AR"] = np.mean(recs)
  return out


# ---- what a float32 overlap cannot decide differently -------------------------------------------------------------------------
def assert_headings_clear(h1, h2, what):
  """Every pair of headings is parallel exactly (difference 0.0) or at least 0.05 in |sin| and |cos| away from parallel and
  perpendicular: no near-parallel edge crossing in the clipping."""
  d = np.asarray(h1, np.float64)[:, None] - np.asarray(h2, np.float64)[None, :]
  ok = (d == 0.0) | ((np.abs(np.sin(d)) >= 0.05) & (np.abs(np.cos(d)) >= 0.05))
  assert ok.all(), "%s: %d heading pairs are nearly parallel" % (what, int((~ok).sum()))


def assert_results_clear(results, thresholds, what, margin=1e-3):
  """eval_det results: every best overlap is `margin` away from every threshold, and from the runner-up unless both are 0."""
  for c, r in results.items():
    ov, sec = r["ovmax"], r["second"]
    fin = np.isfinite(ov)
    for t in thresholds:
      assert (np.abs(ov[fin] - t) >= margin).all(), "%s: class %s has an overlap within %g of %g" % (what, c, margin, t)
    both = fin & np.isfinite(sec) & ~((ov == 0) & (sec == 0))
    assert (ov[both] - sec[both] >= margin).all(), "%s: class %s has a runner-up within %g of the best overlap" % (what, c, margin)


def flags_from_matches(ovmax, gt_id, thresh):
  """The true-positive flags of one class's detections in rank order from their best overlap and the (global) index of that
  box: the first detection to claim a box with an overlap above thresh is the true positive."""
  claimed, tp = set(), np.zeros(len(ovmax), np.int64)
  for r in range(len(ovmax)):
    if gt_id[r] >= 0 and float(ovmax[r]) > thresh and int(gt_id[r]) not in claimed:
      tp[r] = 1
      claimed.add(int(gt_id[r]))
  return tp
