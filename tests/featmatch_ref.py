"""numpy restatement of csrc/featmatch.hip under the rules of include/pcmi.h: pcmi_feat_nn, pcmi_match_stats,
pcmi_ransac_score, pcmi_rigid_sums, and of lib/feature_match.py's evaluator on top of them.  tests/test_featmatch_ref.py holds
it to independent ground (float64 brute force, exact poses, a planted answer); tests/test_gpu_featmatch.py holds the device
to it.

numpy evaluates every float64 product, sum, quotient and square root as its own correctly rounded operation, which is the
arithmetic pcmi.h prescribes for everything but feat_nn: those results are compared BIT for bit.  feat_nn's fp32 FMA chain
is restated through float64 (the product of two fp32 numbers is exact there; the sum is rounded to fp32 once more, which in
rare cases differs from a true FMA by one ulp), so the device is held to float64 distances with a tolerance instead."""
import numpy as np

N_QUERY, N_VALID, N_MUTUAL, N_GT, HITS, HITS_GT, STAT_COLS = 0, 1, 2, 3, 4, 8, 12
LANES = 256
DEGENERATE = 1e-9


def offsets_of(lengths):
  out = np.zeros(len(lengths) + 1, dtype=np.int64)
  np.cumsum(np.asarray(lengths, dtype=np.int64), out=out[1:])
  return out


def segment_of(offs, i):
  """The segment of every position in i (-1: none)."""
  offs = np.asarray(offs, dtype=np.int64)
  s = np.searchsorted(offs, np.asarray(i, dtype=np.int64), side="right") - 1
  return np.where((s >= 0) & (s < len(offs) - 1), s, -1)


# ---- feat_nn ----------------------------------------------------------------------------------------------------------------
def dist2_f64(a, b):
  """[len(a), len(b)] squared distances in float64 from float32 features; non-finite where an operand is."""
  a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
  with np.errstate(invalid="ignore", over="ignore"):
    return ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)


def dist2_f32(a, b):
  """The device's chain: d2 = fma(a_c - b_c, a_c - b_c, d2) over ascending c in fp32 (see the module docstring)."""
  a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
  acc = np.zeros((len(a), len(b)), dtype=np.float32)
  with np.errstate(invalid="ignore", over="ignore"):
    for c in range(a.shape[1]):
      df = (a[:, None, c] - b[None, :, c]).astype(np.float64)
      acc = (df * df + acc.astype(np.float64)).astype(np.float32)
  return acc


def feat_nn(qf, q_offs, rf, r_offs, query_rows=None, query_offs=None, dist=dist2_f32):
  """(nn int32 [Q], d2 float32 [Q]) by the rules of pcmi.h; `dist` decides the arithmetic of the distances."""
  qf, rf = np.asarray(qf, dtype=np.float32), np.asarray(rf, dtype=np.float32)
  q_offs, r_offs = np.asarray(q_offs, dtype=np.int64), np.asarray(r_offs, dtype=np.int64)
  if query_rows is None:
    rows, offs = np.arange(len(qf), dtype=np.int64), q_offs
  else:
    rows, offs = np.asarray(query_rows, dtype=np.int64), np.asarray(query_offs, dtype=np.int64)
  Q = len(rows)
  nn, d2 = np.full(Q, -1, dtype=np.int32), np.full(Q, np.nan, dtype=np.float32)
  for b in range(len(q_offs) - 1):
    lo, hi = int(offs[b]), int(offs[b + 1])
    r = rows[lo:hi]
    inside = (r >= q_offs[b]) & (r < q_offs[b + 1])
    ref = rf[r_offs[b]:r_offs[b + 1]]
    if hi == lo or len(ref) == 0 or not inside.any():
      continue
    D = dist(qf[r[inside]], ref).astype(np.float64)
    D[~np.isfinite(D)] = np.inf  # never chosen
    j = D.argmin(1)  # the first among equals: the lowest row
    best = D[np.arange(len(j)), j]
    ok = np.isfinite(best)
    pos = lo + np.flatnonzero(inside)[ok]
    nn[pos] = (r_offs[b] + j[ok]).astype(np.int32)
    d2[pos] = best[ok].astype(np.float32)
  return nn, d2


# ---- match_stats ------------------------------------------------------------------------------------------------------------
def apply_rigid(T, p):
  """((R0 x + R1 y) + R2 z) + t per coordinate; T [..., 3 or 4, 4] broadcast against p [..., 3]."""
  T, p = np.asarray(T, dtype=np.float64), np.asarray(p, dtype=np.float64)
  out = np.empty(np.broadcast(T[..., 0, 0], p[..., 0]).shape + (3,))
  for r in range(3):
    out[..., r] = ((T[..., r, 0] * p[..., 0] + T[..., r, 1] * p[..., 1]) + T[..., r, 2] * p[..., 2]) + T[..., r, 3]
  return out


def residual2(y, q):
  d = np.asarray(y, dtype=np.float64) - np.asarray(q, dtype=np.float64)
  return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def match_stats(xyz0, xyz1, T_gt, query_offs, nn01, taus, query_rows=None, nn10=None, has_gt=None, counts=None):
  xyz0, xyz1 = np.asarray(xyz0, dtype=np.float64).reshape(-1, 3), np.asarray(xyz1, dtype=np.float64).reshape(-1, 3)
  T = np.asarray(T_gt, dtype=np.float64).reshape(-1, 4, 4)
  B, n0, n1 = len(T), len(xyz0), len(xyz1)
  nn01 = np.asarray(nn01, dtype=np.int64)
  Q = len(nn01)
  rows = np.arange(Q, dtype=np.int64) if query_rows is None else np.asarray(query_rows, dtype=np.int64)
  counts = np.zeros((B, STAT_COLS), dtype=np.int64) if counts is None else counts.copy()
  seg = segment_of(query_offs, np.arange(Q))
  row_ok = (rows >= 0) & (rows < n0)
  valid = (seg >= 0) & row_ok & (nn01 >= 0) & (nn01 < n1)
  r2 = np.full(Q, np.nan)
  v = np.flatnonzero(valid)
  with np.errstate(invalid="ignore", over="ignore"):
    r2[v] = residual2(apply_rigid(T[seg[v]], xyz0[rows[v]]), xyz1[nn01[v]])
  gt = np.zeros(Q, dtype=bool)
  if has_gt is not None:
    gt[row_ok] = np.asarray(has_gt)[rows[row_ok]] != 0
  for b in range(B):
    m = seg == b
    counts[b, N_QUERY] += m.sum()
    counts[b, N_VALID] += (m & valid).sum()
    counts[b, N_GT] += (m & gt).sum()
    if nn10 is not None:
      counts[b, N_MUTUAL] += (m & valid & (np.asarray(nn10, dtype=np.int64) == rows)).sum()
    for k, tau in enumerate(taus):
      with np.errstate(invalid="ignore"):
        hit = m & valid & (r2 <= np.float64(tau) * np.float64(tau))
      counts[b, HITS + k] += hit.sum()
      counts[b, HITS_GT + k] += (hit & gt).sum()
  return counts, r2


# ---- RANSAC -----------------------------------------------------------------------------------------------------------------
def _dot3(a, b):
  return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
  return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                   a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def tri_frame(a0, a1, a2):
  """(e [..., 3, 3] with rows e1, e2, e3; ok [...]) of the triangles (a0, a1, a2), in pcmi.h's operation order."""
  with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
    u = a1 - a0
    lu = np.sqrt(_dot3(u, u))
    e1 = u / lu[..., None]
    n = _cross(e1, a2 - a0)
    ln = np.sqrt(_dot3(n, n))
    e3 = n / ln[..., None]
    e2 = _cross(e3, e1)
    ok = (lu >= DEGENERATE) & (ln >= DEGENERATE)
  return np.stack([e1, e2, e3], -2), ok


def triple_transform(p, q):
  """p, q [..., 3 points, 3]: (Rt [..., 12], ok [...])."""
  p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
  e, ok_p = tri_frame(p[..., 0, :], p[..., 1, :], p[..., 2, :])
  f, ok_q = tri_frame(q[..., 0, :], q[..., 1, :], q[..., 2, :])
  with np.errstate(invalid="ignore", over="ignore"):
    R = np.empty(p.shape[:-2] + (3, 3))
    for i in range(3):
      for j in range(3):
        R[..., i, j] = (f[..., 0, i] * e[..., 0, j] + f[..., 1, i] * e[..., 1, j]) + f[..., 2, i] * e[..., 2, j]
    t = np.empty(p.shape[:-2] + (3,))
    for i in range(3):
      t[..., i] = q[..., 0, i] - ((R[..., i, 0] * p[..., 0, 0] + R[..., i, 1] * p[..., 0, 1]) + R[..., i, 2] * p[..., 0, 2])
  return np.concatenate([R.reshape(p.shape[:-2] + (9,)), t], -1), ok_p & ok_q


def match_r2(Rt, p, q):
  """|R p + t - q|^2 with Rt [..., 12] broadcast against p, q [..., 3]."""
  Rt = np.asarray(Rt, dtype=np.float64)
  T = np.concatenate([Rt[..., :9].reshape(Rt.shape[:-1] + (3, 3)), Rt[..., 9:, None]], -1)
  with np.errstate(invalid="ignore", over="ignore"):
    return residual2(apply_rigid(T, p), q)


def ransac_score(src, dst, offsets, triples, tau):
  src, dst = np.asarray(src, dtype=np.float64).reshape(-1, 3), np.asarray(dst, dtype=np.float64).reshape(-1, 3)
  tri = np.asarray(triples, dtype=np.int64)
  B, H = tri.shape[:2]
  counts, best, Rt_out = np.full((B, H), -1, dtype=np.int32), np.full(B, -1, dtype=np.int32), np.full((B, 12), np.nan)
  tau2 = np.float64(tau) * np.float64(tau)
  for b in range(B):
    lo, m = int(offsets[b]), int(offsets[b + 1] - offsets[b])
    if m < 3:
      continue
    t = tri[b]
    ok = ((t >= 0) & (t < m)).all(1) & (t[:, 0] != t[:, 1]) & (t[:, 0] != t[:, 2]) & (t[:, 1] != t[:, 2])
    tc = np.where(ok[:, None], t, 0)
    Rt, ok_f = triple_transform(src[lo + tc], dst[lo + tc])
    ok &= ok_f
    P, Qd = src[lo:lo + m], dst[lo:lo + m]
    for h in np.flatnonzero(ok):
      with np.errstate(invalid="ignore"):
        counts[b, h] = int((match_r2(Rt[h], P, Qd) <= tau2).sum())
    if ok.any():
      best[b] = int(np.argmax(counts[b]))  # the first among equals: the lowest hypothesis
      Rt_out[b] = Rt[best[b]]
  return counts, best, Rt_out


# ---- rigid_sums -------------------------------------------------------------------------------------------------------------
def _lane_fold(values, mask):
  """values [m, k], mask [m]: lane t adds rows t, t + 256, ... (where mask) in ascending order from +0, then the lanes are
  folded by halving."""
  m, k = values.shape
  rounds = -(-m // LANES)
  v = np.zeros((rounds * LANES, k))
  v[:m] = np.where(mask[:, None], values, 0.0)  # (x + 0.0 == x for every partial sum, which starts at +0 and is never -0)
  lane = np.zeros((LANES, k))
  for r in range(rounds):
    lane = lane + v[r * LANES:(r + 1) * LANES]
  s = LANES // 2
  while s >= 1:
    lane[:s] = lane[:s] + lane[s:2 * s]
    s //= 2
  return lane[0]


def rigid_sums(src, dst, offsets, best, Rt, tau):
  src, dst = np.asarray(src, dtype=np.float64).reshape(-1, 3), np.asarray(dst, dtype=np.float64).reshape(-1, 3)
  B = len(best)
  out = np.zeros((B, 16))
  tau2 = np.float64(tau) * np.float64(tau)
  for b in range(B):
    if best[b] < 0:
      continue
    P, Qd = src[offsets[b]:offsets[b + 1]], dst[offsets[b]:offsets[b + 1]]
    with np.errstate(invalid="ignore"):
      inl = match_r2(Rt[b], P, Qd) <= tau2
    first = _lane_fold(np.concatenate([np.ones((len(P), 1)), P, Qd], 1), inl)
    with np.errstate(invalid="ignore", divide="ignore"):
      pm, qm = first[1:4] / first[0], first[4:7] / first[0]
      dp, dq = P - pm, Qd - qm
      prod = (dp[:, :, None] * dq[:, None, :]).reshape(len(P), 9)
    out[b, :7], out[b, 7:] = first, _lane_fold(prod, inl)
  return out


def inliers(src, dst, offsets, best, Rt, tau, b):
  """The inlier mask of pair b's best hypothesis (for an independent Kabsch on the same set)."""
  P, Qd = np.asarray(src)[offsets[b]:offsets[b + 1]], np.asarray(dst)[offsets[b]:offsets[b + 1]]
  with np.errstate(invalid="ignore"):
    return match_r2(Rt[b], P, Qd) <= np.float64(tau) * np.float64(tau)


def kabsch_points(P, Q):
  """The least-squares rigid transform P -> Q straight from the points (numpy, centred sums in the plain order)."""
  pm, qm = P.mean(0), Q.mean(0)
  S = (P - pm).T @ (Q - qm)
  U, _, Vt = np.linalg.svd(S)
  d = np.sign(np.linalg.det(Vt.T @ U.T))
  R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
  return R, qm - R @ pm


# ---- the evaluator ----------------------------------------------------------------------------------------------------------
class EvaluatorRef:
  """lib/feature_match.py's FeatureMatchEvaluator on the functions above; `nn` replaces the nearest-neighbour search (the GPU
  tests hand over the device's nn01 / nn10, whose near-ties are decided in fp32)."""

  def __init__(self, voxel_size, hit_thresholds=(0.1,), inlier_ratio_thresh=0.05, mutual_only=False, ransac_thresh=None,
               rte_thresh=0.3, rre_thresh_deg=15.0):
    self.voxel_size, self.hit_thresholds, self.inlier_ratio_thresh = float(voxel_size), tuple(hit_thresholds), inlier_ratio_thresh
    self.mutual_only = mutual_only
    self.ransac_thresh = 2.0 * self.voxel_size if ransac_thresh is None else float(ransac_thresh)
    self.rte_thresh, self.rre_thresh_deg = rte_thresh, rre_thresh_deg
    self.records = []

  def step(self, F0, F1, C0, C1, T_gt, len_batch, correspondences, query_rows, query_offsets, triples, nn=None):
    o0, o1 = offsets_of([l[0] for l in len_batch]), offsets_of([l[1] for l in len_batch])
    B = len(len_batch)
    xyz0 = np.asarray(C0)[:, 1:4].astype(np.float64) * self.voxel_size
    xyz1 = np.asarray(C1)[:, 1:4].astype(np.float64) * self.voxel_size
    T = np.asarray(T_gt).astype(np.float64).reshape(B, 4, 4)
    moffs = o0 if query_rows is None else np.asarray(query_offsets, dtype=np.int64)
    if nn is None:
      nn01, _ = feat_nn(F0, o0, F1, o1, query_rows, None if query_rows is None else moffs)
      nn10, _ = feat_nn(F1, o1, F0, o0, nn01, moffs)
    else:
      nn01, nn10 = nn
    has_gt = None
    if correspondences is not None:
      has_gt = np.zeros(len(xyz0), dtype=np.uint8)
      has_gt[np.asarray(correspondences)[:, 0]] = 1
    counts, r2 = match_stats(xyz0, xyz1, T, moffs, nn01, self.hit_thresholds, query_rows, nn10, has_gt)
    qrow = np.arange(len(xyz0)) if query_rows is None else np.asarray(query_rows, dtype=np.int64)
    keep = nn01 >= 0
    if self.mutual_only:
      keep &= nn10 == qrow
    src = xyz0[qrow]
    dst = np.where(keep[:, None], xyz1[np.maximum(nn01, 0)], np.nan)
    hc, best, Rt = ransac_score(src, dst, moffs, triples, self.ransac_thresh)
    sums = rigid_sums(src, dst, moffs, best, Rt, self.ransac_thresh)
    self.records.append((counts, sums, T))
    return dict(nn01=nn01, nn10=nn10, counts=counts, residual2=r2, src=src, dst=dst, hyp_counts=hc, best=best, Rt=Rt, sums=sums)

  def compute_metrics(self):
    from pointcontrast_amd.lib.feature_match import metrics_from_records
    counts = np.concatenate([r[0] for r in self.records])
    sums = np.concatenate([r[1] for r in self.records])
    T = np.concatenate([r[2] for r in self.records])
    return metrics_from_records(counts, sums, T, self.hit_thresholds, self.inlier_ratio_thresh, self.rte_thresh, self.rre_thresh_deg)


# ---- the planted-answer pair ------------------------------------------------------------------------------------------------
def random_pose(rng, max_trans=1.0):
  """A proper rotation (QR of a Gaussian matrix, sign-fixed) and a translation, as a 4 x 4."""
  Qm, Rm = np.linalg.qr(rng.normal(size=(3, 3)))
  Qm = Qm * np.sign(np.diag(Rm))
  if np.linalg.det(Qm) < 0:
    Qm[:, 0] = -Qm[:, 0]
  T = np.eye(4)
  T[:3, :3], T[:3, 3] = Qm, rng.uniform(-max_trans, max_trans, 3)
  return T


def planted_pair(rng, n, c, voxel_size, clutter=0.3, feat_noise=0.02, batch_index=0):
  """Cloud 0: n distinct voxels.  Cloud 1: its rigid copy (the pose is planted), re-voxelised, with `clutter` of the rows
  replaced by unrelated voxels; corresponding rows share a random unit feature plus N(0, feat_noise) per channel, the clutter
  has features of its own.  Returns a dict with C0, C1 (int32 [n, 4]), F0, F1 (float32), T (4 x 4), corr [k, 2] (row of
  cloud 0, row of cloud 1) and len [n, n]."""
  side = int(np.ceil((4 * n) ** (1 / 3.0))) + 2
  flat = rng.choice(side ** 3, n, replace=False)
  v0 = np.stack([flat // (side * side), flat // side % side, flat % side], 1).astype(np.int64)
  T = random_pose(rng, max_trans=voxel_size * side)
  moved = apply_rigid(T, v0 * voxel_size)
  v1 = np.floor(moved / voxel_size + 0.5).astype(np.int64)  # the nearest voxel: off by at most half a voxel per axis
  n_cl = int(round(clutter * n))
  cl_rows = rng.choice(n, n_cl, replace=False)
  v1[cl_rows] = rng.randint(-3 * side, 4 * side, (n_cl, 3)) + 10 * side  # far from the copy
  # distinct voxels in cloud 1 (a collision becomes clutter)
  _, first = np.unique(v1, axis=0, return_index=True)
  dup = np.ones(n, dtype=bool)
  dup[first] = False
  is_clutter = np.zeros(n, dtype=bool)
  is_clutter[cl_rows] = True
  for r in np.flatnonzero(dup):
    v1[r] = [20 * side + r, 0, 0]
    is_clutter[r] = True
  f = rng.normal(size=(n, c))
  f /= np.linalg.norm(f, axis=1, keepdims=True)
  F0 = (f + rng.normal(0, feat_noise, f.shape)).astype(np.float32)
  g = rng.normal(size=(n, c))
  g /= np.linalg.norm(g, axis=1, keepdims=True)
  F1 = (np.where(is_clutter[:, None], g, f) + rng.normal(0, feat_noise, f.shape)).astype(np.float32)
  perm = rng.permutation(n)  # cloud 1 in its own row order
  inv = np.empty(n, dtype=np.int64)
  inv[perm] = np.arange(n)
  keep = np.flatnonzero(~is_clutter)
  corr = np.stack([keep, inv[keep]], 1)
  bcol = np.full((n, 1), batch_index, dtype=np.int64)
  return dict(C0=np.concatenate([bcol, v0], 1).astype(np.int32), C1=np.concatenate([bcol, v1[perm]], 1).astype(np.int32),
              F0=F0, F1=F1[perm], T=T, corr=corr, len=[n, n])


def collate_planted(pairs):
  """Several planted pairs as one batch (rows concatenated, correspondences shifted)."""
  o0 = offsets_of([p["len"][0] for p in pairs])
  o1 = offsets_of([p["len"][1] for p in pairs])
  cat = lambda k: np.concatenate([p[k] for p in pairs])
  C0, C1 = cat("C0"), cat("C1")
  C0[:, 0] = np.repeat(np.arange(len(pairs)), [p["len"][0] for p in pairs])
  C1[:, 0] = np.repeat(np.arange(len(pairs)), [p["len"][1] for p in pairs])
  corr = np.concatenate([p["corr"] + np.array([[o0[b], o1[b]]]) for b, p in enumerate(pairs)])
  return dict(C0=C0, C1=C1, F0=cat("F0"), F1=cat("F1"), T=np.stack([p["T"] for p in pairs]), corr=corr,
              len_batch=[p["len"] for p in pairs])
