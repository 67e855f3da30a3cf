"""numpy float64 restatement of the instance-segmentation entry points of csrc/cluster.hip under exactly the rules of
include/pcmi.h: radius components by brute force over all pairs, compaction, fixed-point scores, overlap, matching, integer
centroids, the two offset losses with their gradients, and mask AP through tests/ap_ref.py.  tests/test_insseg_ref.py holds
it to planted answers and to independent spellings (scipy, torch.autograd); tests/test_gpu_insseg.py holds the kernels to it."""
import numpy as np

import ap_ref

CELL_LIMIT = float(1 << 20)  # kCellBias of csrc/cellgrid.h
FIX = float(1 << 30)
EPS_V, EPS_N = 1e-6, 1e-8


# ---- radius components --------------------------------------------------------------------------------------------------------
def scene_of_rows(offs, n):
  """scene [n]: b with offs[b] <= i < offs[b + 1], -1 for a row of no scene."""
  offs = np.asarray(offs, np.int64)
  rows = np.arange(n, dtype=np.int64)
  b = np.searchsorted(offs, rows, side="right") - 1
  return np.where((b >= 0) & (b < len(offs) - 1), b, -1)


def active_rows(xyz, offs, group, r):
  """(active [n] bool, scene [n], dropped): in a scene, group >= 0, finite, |floor(x / r)| < 2^20 on every axis."""
  p = np.asarray(xyz, np.float32).astype(np.float64).reshape(-1, 3)
  n = len(p)
  scene, group = scene_of_rows(offs, n), np.asarray(group, np.int64).reshape(-1)
  cand = (scene >= 0) & (group >= 0) & np.isfinite(p).all(1)
  with np.errstate(all="ignore"):
    fits = (np.abs(np.floor(p / np.float64(r))) < CELL_LIMIT).all(1)
  return cand & fits, scene, int((cand & ~fits).sum())


def radius_edges(xyz, offs, group, r, chunk=1024):
  """The edges (i < j) of the graph: (dx dx + dy dy) + dz dz <= r r with every operation rounded in float64, tested on ALL
  pairs of active rows but those more than 2 r apart in x (their d2 is at least 4 r^2 (1 - 2^-52) under any rounding): the
  rows are taken in the order of x, chunk by chunk against the window of x that reaches 2 r beyond the chunk."""
  p = np.asarray(xyz, np.float32).astype(np.float64).reshape(-1, 3)
  active, scene, _ = active_rows(xyz, offs, group, r)
  group = np.asarray(group, np.int64).reshape(-1)
  rows = np.flatnonzero(active)
  rows = rows[np.argsort(p[rows, 0], kind="stable")]
  q, s, g = p[rows], scene[rows], group[rows]
  r2 = np.float64(r) * np.float64(r)
  ei, ej = [], []
  for a in range(0, len(rows), chunk):
    b = min(a + chunk, len(rows))
    lo = np.searchsorted(q[:, 0], q[a, 0] - 2.0 * r, side="left")
    hi = np.searchsorted(q[:, 0], q[b - 1, 0] + 2.0 * r, side="right")
    d = q[a:b, None, :] - q[None, lo:hi, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    ok = (d2 <= r2) & (s[a:b, None] == s[None, lo:hi]) & (g[a:b, None] == g[None, lo:hi])
    i, j = np.nonzero(ok)
    i, j = rows[i + a], rows[j + lo]
    keep = i < j
    ei.append(i[keep])
    ej.append(j[keep])
  if not ei:
    return np.zeros(0, np.int64), np.zeros(0, np.int64)
  return np.concatenate(ei), np.concatenate(ej)


def lowest_row_labels(ei, ej, n):
  """lab [n]: the lowest row of the connected component of every row, by root hooking and pointer jumping to the fixed point.
  lab[x] <= x throughout and a fixed point has no edge between two labels, so every label is its component's minimum."""
  lab = np.arange(n, dtype=np.int64)
  while True:
    new = lab.copy()
    np.minimum.at(new, lab[ei], lab[ej])
    np.minimum.at(new, lab[ej], lab[ei])
    while True:
      nn = new[new]
      if np.array_equal(nn, new):
        break
      new = nn
    if np.array_equal(new, lab):
      return lab
    lab = new


def radius_components(xyz, offs, group, r):
  """(label int32 [n], dropped)."""
  active, _, dropped = active_rows(xyz, offs, group, r)
  ei, ej = radius_edges(xyz, offs, group, r)
  lab = lowest_row_labels(ei, ej, len(active))
  return np.where(active, lab, -1).astype(np.int32), dropped


# ---- compaction, scores, overlap, match, centroids ----------------------------------------------------------------------------
def components_compact(label, offs, group, min_points, max_inst):
  label = np.asarray(label, np.int64).reshape(-1)
  n = len(label)
  ok = (label >= 0) & (label < n)
  size = np.bincount(label[ok], minlength=n) if n else np.zeros(0, np.int64)
  roots = np.flatnonzero((label == np.arange(n)) & (size >= min_points)) if n else np.zeros(0, np.int64)
  P = len(roots)
  number = np.full(n + 1, -1, np.int64)
  number[roots[:max_inst]] = np.arange(min(P, max_inst))
  inst = np.where(ok, number[np.where(ok, label, n)], -1).astype(np.int32)
  scene = scene_of_rows(offs, n)
  out = dict(instance=inst, count=P)
  kept = roots[:max_inst]
  for name, val, fill in (("root", kept, -1), ("size", size[kept], 0), ("scene", scene[kept], -1),
                          ("group", (np.asarray(group, np.int64)[kept] if group is not None else np.full(len(kept), -1)), -1)):
    a = np.full(max_inst, fill, np.int32)
    a[:len(kept)] = val
    out[name] = a
  return out


def score_fixed(score):
  """q [n] int64 = rint(clamp(score, 0, 1) 2^30), a non-finite score counting as 0."""
  s = np.asarray(score, np.float32).astype(np.float64)
  c = np.where(np.isfinite(s), np.clip(s, 0.0, 1.0), 0.0)
  return np.rint(c * FIX).astype(np.int64)


def instance_scores(score, inst, inst_size):
  inst, size = np.asarray(inst, np.int64), np.asarray(inst_size, np.int64)
  P = len(size)
  q = score_fixed(score)
  ok = (inst >= 0) & (inst < P)
  total = np.zeros(P, np.int64)
  np.add.at(total, inst[ok], q[ok])
  with np.errstate(all="ignore"):
    return np.where(size > 0, total.astype(np.float64) / (size.astype(np.float64) * FIX), 0.0)


def instance_overlap(pred, gt, P, G):
  pred, gt = np.asarray(pred, np.int64), np.asarray(gt, np.int64)
  pv, gv = (pred >= 0) & (pred < P), (gt >= 0) & (gt < G)
  ps = np.bincount(pred[pv], minlength=P).astype(np.int32)[:P]
  gs = np.bincount(gt[gv], minlength=G).astype(np.int32)[:G]
  inter = np.zeros((P, G), np.int32)
  np.add.at(inter, (pred[pv & gv], gt[pv & gv]), 1)
  return inter, ps, gs


def iou_table(inter, ps, gs):
  """float64 inter / (ps + gs - inter), 0 where the denominator is 0."""
  it = np.asarray(inter, np.int64)
  un = np.asarray(ps, np.int64)[:, None] + np.asarray(gs, np.int64)[None, :] - it
  with np.errstate(all="ignore"):
    return np.where(un > 0, it.astype(np.float64) / un.astype(np.float64), 0.0)


def instance_match(inter, ps, gs, pred_scene, pred_class, gt_scene, gt_class):
  """(best_gt int32 [P], best_iou float32 [P]): the lowest index among equal float64 quotients; -1 / -inf without one."""
  iou = iou_table(inter, ps, gs)
  P, G = iou.shape
  best_gt, best = np.full(P, -1, np.int32), np.full(P, -np.inf)
  for p in range(P):
    for g in range(G):
      if gt_scene[g] == pred_scene[p] and gt_class[g] == pred_class[p] and iou[p, g] > best[p]:
        best[p], best_gt[p] = iou[p, g], g
  return best_gt, best.astype(np.float32)


def instance_centroids(coords, inst, G):
  coords, inst = np.asarray(coords, np.int64).reshape(-1, 4), np.asarray(inst, np.int64)
  ok = (inst >= 0) & (inst < G)
  s, c = np.zeros((G, 3), np.int64), np.zeros(G, np.int64)
  np.add.at(s, inst[ok], coords[ok, 1:4])
  np.add.at(c, inst[ok], 1)
  return s, c


# ---- offset losses ------------------------------------------------------------------------------------------------------------
def _off_parts(p, g):
  p, g = np.asarray(p, np.float32).astype(np.float64).reshape(-1, 3), np.asarray(g, np.float32).astype(np.float64).reshape(-1, 3)
  gn = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
  pn = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
  return p, g, g / (gn + EPS_N)[:, None], pn, pn + EPS_N


def offset_terms(p, g, inst):
  """(norm terms, dir terms) of the valid rows, in the header's operation order."""
  p, g, gh, _, A = _off_parts(p, g)
  v = np.asarray(inst).reshape(-1) >= 0
  e = np.abs(p - g)
  norm = (e[:, 0] + e[:, 1]) + e[:, 2]
  ph = p / A[:, None]
  direction = -((gh[:, 0] * ph[:, 0] + gh[:, 1] * ph[:, 1]) + gh[:, 2] * ph[:, 2])
  return norm[v], direction[v]


def offset_loss(p, g, inst):
  """(norm_loss, dir_loss, V), the sums by math.fsum (exact, rounded once)."""
  import math
  a, d = offset_terms(p, g, inst)
  V = float(len(a))
  return math.fsum(a) / (V + EPS_V), math.fsum(d) / (V + EPS_V), V


def offset_grad(p, g, inst, g_norm=1.0, g_dir=1.0):
  """float64 [n, 3]: d(g_norm norm_loss + g_dir dir_loss)/dp, before the rounding to float32; sign(0) = 0, d|p|/dp = 0 at 0."""
  p, g, gh, pn, A = _off_parts(p, g)
  v = np.asarray(inst).reshape(-1) >= 0
  s = float(v.sum()) + EPS_V
  gn_, gd_ = np.float64(g_norm) / s, np.float64(g_dir) / s
  dot = (gh[:, 0] * p[:, 0] + gh[:, 1] * p[:, 1]) + gh[:, 2] * p[:, 2]
  out = np.zeros_like(p)
  with np.errstate(all="ignore"):
    for a in range(3):
      dd = gh[:, a] / A
      dd = np.where(pn > 0, dd - (dot * (p[:, a] / pn)) / (A * A), dd)
      out[:, a] = gn_ * np.sign(p[:, a] - g[:, a]) + gd_ * (-dd)
  out[~v] = 0.0
  return out


# ---- mask AP through ap_ref ---------------------------------------------------------------------------------------------------
def evaluate_ap(iou32, pred_scene, pred_class, pred_score, gt_scene, gt_class, thresholds, n_classes):
  """{threshold: {class: ap_ref.eval_class result}}: instances stand in for boxes as one-element arrays holding their index,
  and the overlap is looked up in iou32 [P, G] (the float32-rounded quotients of iou_table)."""
  out = {}
  for t in thresholds:
    res = {}
    for c in range(n_classes):
      pred, gt = {}, {}
      for g in range(len(gt_scene)):
        if gt_class[g] == c:
          gt.setdefault(int(gt_scene[g]), []).append([float(g)])
      for p in range(len(pred_scene)):
        if pred_class[p] == c:
          pred.setdefault(int(pred_scene[p]), []).append(([float(p)], float(pred_score[p])))
          gt.setdefault(int(pred_scene[p]), [])
      if not gt and not pred:
        continue
      res[c] = ap_ref.eval_class(pred, gt, t, False, iou_fn=lambda a, b: float(iou32[int(a[0]), int(b[0])]))
      res[c]["pred_ids"] = [int(box[0]) for sid in pred for box, _ in pred[sid]]
    out[t] = res
  return out


# ---- the shared cases ---------------------------------------------------------------------------------------------------------
def kink_rows(n, seed):
  """(p, g, inst) float32 / int32: generic rows plus, where there is room, a row with p = 0, one with p = g, one with g = 0,
  one with a single coordinate at the kink of |.| and invalid rows."""
  rng = np.random.default_rng(seed)
  p, g = rng.normal(0, 0.4, (n, 3)).astype(np.float32), rng.normal(0, 0.4, (n, 3)).astype(np.float32)
  inst = rng.integers(-1, 6, n).astype(np.int32)
  if n >= 8:
    p[1] = 0.0
    p[2] = g[2]
    g[3] = 0.0
    p[4, 1] = g[4, 1]
    inst[1:5] = 0
    inst[5] = -1
  else:
    inst[:] = 0
  return p, g, inst



def lattice_case():
  """A 7 x 7 x 2 lattice of multiples of 0.25 thinned to 60 %: 56 points, 69 pairs at exactly r^2 for r = 0.25."""
  rng = np.random.default_rng(1)
  g = np.stack(np.meshgrid(np.arange(7), np.arange(7), np.arange(2), indexing="ij"), -1).reshape(-1, 3)
  keep = rng.random(len(g)) < 0.6
  return (g[keep] * 0.25).astype(np.float32), rng


def blob_case():
  """Three Gaussian blobs of 60 points (sigma 0.03, centres 1 m apart) and 40 uniform points; r = 0.06."""
  _, rng = lattice_case()  # default_rng(1) after the lattice draw
  centres = np.array([[0.0, 0, 0], [1.0, 0, 0], [0.0, 1.0, 0]])
  pts = [c + rng.normal(0.0, 0.03, (60, 3)) for c in centres]
  pts.append(rng.uniform(-0.5, 1.5, (40, 3)))
  return np.concatenate(pts).astype(np.float32)
