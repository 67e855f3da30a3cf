"""numpy restatement of the three entry points of csrc/nearest.hip under exactly the rules of include/pcmi.h: the float64
operations one at a time in the stated order (numpy never contracts a product and a sum), brute force over the scene's
segment in chunks, np.argmin on d2 -- which takes the FIRST minimum, i.e. the lowest row."""
import numpy as np

NAN_BITS = np.array([np.nan]).view(np.int64)[0]


def voxel_centers(coords, inv_T):
  """coords int [n, 4] (b, x, y, z), inv_T [B, 16] -> [n, 3]: ((X m0 + Y m1) + Z m2) + m3 per output coordinate; NaN rows
  where b is outside [0, B)."""
  coords = np.asarray(coords)
  inv_T = np.asarray(inv_T, dtype=np.float64).reshape(-1, 16)
  B = inv_T.shape[0]
  b = coords[:, 0]
  ok = (b >= 0) & (b < B)
  M = inv_T[np.where(ok, b, 0)]
  X, Y, Z = (coords[:, 1].astype(np.float64) + 0.5, coords[:, 2].astype(np.float64) + 0.5, coords[:, 3].astype(np.float64) + 0.5)
  out = np.empty((len(coords), 3))
  for r in range(3):
    out[:, r] = ((X * M[:, 4 * r] + Y * M[:, 4 * r + 1]) + Z * M[:, 4 * r + 2]) + M[:, 4 * r + 3]
  out[~ok] = np.nan
  return out


def nearest_point(ref, ref_offs, query, query_offs, chunk=2048):
  """-> (idx int32 [n] global rows of ref, dist2 float64 [n])."""
  ref, query = np.asarray(ref, dtype=np.float64).reshape(-1, 3), np.asarray(query, dtype=np.float64).reshape(-1, 3)
  n = len(query)
  idx = np.full(n, -1, dtype=np.int32)
  dist2 = np.full(n, np.inf)
  qfinite = np.isfinite(query).all(1)
  dist2[~qfinite] = np.nan
  for b in range(len(ref_offs) - 1):
    r0, r1 = max(int(ref_offs[b]), 0), min(int(ref_offs[b + 1]), len(ref))
    rows = np.arange(r0, max(r1, r0))
    rows = rows[np.isfinite(ref[rows]).all(1)]  # non-finite references are never chosen
    if len(rows) == 0:
      continue
    R = ref[rows]
    for q0 in range(int(query_offs[b]), int(query_offs[b + 1]), chunk):
      q = np.arange(q0, min(q0 + chunk, int(query_offs[b + 1])))
      q = q[qfinite[q]]
      if len(q) == 0:
        continue
      with np.errstate(over="ignore"):
        d = query[q][:, None, :] - R[None, :, :]
        d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
      a = np.argmin(d2, axis=1)  # first minimum = lowest row (rows ascend)
      idx[q] = rows[a]
      dist2[q] = d2[np.arange(len(q)), a]
  return idx, dist2


def seg_hist(pred, idx, labels, c):
  """-> (hist int64 [c, c], point_pred int32 [n], missing)."""
  pred, labels = np.asarray(pred).astype(np.int64), np.asarray(labels).astype(np.int64)
  n, m = len(labels), len(pred)
  src = np.arange(n) if idx is None else np.asarray(idx).astype(np.int64)
  have = (src >= 0) & (src < m)
  pp = np.where(have, pred[np.where(have, src, 0)] if m else -1, -1)
  k = have & (labels >= 0) & (labels < c) & (pp >= 0) & (pp < c)
  hist = np.bincount(c * labels[k] + pp[k], minlength=c * c).reshape(c, c).astype(np.int64)
  return hist, pp.astype(np.int32), int((~have).sum())


def per_class_iu(hist):
  hist = np.asarray(hist, dtype=np.float64)
  with np.errstate(divide="ignore", invalid="ignore"):
    return np.diag(hist) / (hist.sum(1) + hist.sum(0) - np.diag(hist))


# ---- the cases the CPU and the GPU tests share -----------------------------------------------------------------------
VOXEL = 0.05


def lattice_case(seed=7, n_query=2049):
  """A 12 x 10 x 7 lattice at 5 cm with 30 % of the voxels removed (586 centres at seed 7), an offset transform, n_query
  vertices jittered by +-0.9 voxel around randomly chosen centres.  -> coords int32 [m, 4], T [1, 16], query [n, 3]."""
  rng = np.random.RandomState(seed)
  g = np.stack(np.meshgrid(np.arange(12), np.arange(10), np.arange(7), indexing="ij"), -1).reshape(-1, 3)
  g = g[rng.rand(len(g)) >= 0.3] - np.array([3, 2, 1])
  coords = np.concatenate([np.zeros((len(g), 1), dtype=np.int64), g], 1).astype(np.int32)
  # the voxelizer's matrix: world -> voxel units = scale 1 / VOXEL after a translation (and a rotation about z)
  a = 0.3
  R = np.array([[np.cos(a), -np.sin(a), 0, 0], [np.sin(a), np.cos(a), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
  S = np.diag([1 / VOXEL, 1 / VOXEL, 1 / VOXEL, 1.0])
  Tr = np.eye(4)
  Tr[:3, 3] = [1.37, -0.52, 0.11]
  T = (S @ R @ Tr).reshape(1, 16)
  centers = voxel_centers(coords, np.linalg.inv(T.reshape(4, 4)).reshape(1, 16))
  query = centers[rng.randint(0, len(centers), n_query)] + rng.uniform(-0.9, 0.9, (n_query, 3)) * VOXEL
  return coords, T, query


def three_scene_case(seed=11):
  """Scene 0: 300 random voxels; scene 1: EMPTY; scene 2: scene 0's voxels again under a transform shifted by 0.4 voxel, so
  that for most vertices of scene 2 the globally nearest centre belongs to scene 0.  -> coords int32 [m, 4] (sorted by
  scene), T [3, 16], points [n, 3], point_offs [4], ref_offs [4]."""
  rng = np.random.RandomState(seed)
  g = np.unique(rng.randint(-6, 7, (400, 3)), axis=0)[:300]
  c0 = np.concatenate([np.zeros((len(g), 1), dtype=np.int64), g], 1)
  c2 = c0.copy()
  c2[:, 0] = 2
  c2 = c2[: len(c2) - 37]  # a different size
  coords = np.concatenate([c0, c2]).astype(np.int32)
  S = np.diag([1 / VOXEL, 1 / VOXEL, 1 / VOXEL, 1.0])
  T0, T2 = S.copy(), S.copy()
  T2[:3, 3] = [0.4, 0.4, 0.4]  # voxel units: scene 2's centres sit 0.4 voxel away from scene 0's
  T = np.stack([T0, S, T2]).reshape(3, 16)
  inv = np.linalg.inv(T.reshape(3, 4, 4)).reshape(3, 16)
  centers = voxel_centers(coords, inv)
  ref_offs = np.array([0, len(c0), len(c0), len(coords)], dtype=np.int64)
  sizes = [513, 64, 700]
  pts = []
  for b, k in enumerate(sizes):
    lo, hi = ref_offs[b], ref_offs[b + 1]
    base = centers[rng.randint(lo, hi, k)] if hi > lo else rng.uniform(-0.3, 0.3, (k, 3))
    pts.append(base + rng.uniform(-0.9, 0.9, (k, 3)) * VOXEL)
  point_offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
  return coords, T, np.concatenate(pts), point_offs, ref_offs
