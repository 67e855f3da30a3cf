"""numpy / scipy restatement of the pair-corpus semantics (pointcontrast_amd/lib/pair_corpus.py, steps 1-5), with the
rounding order of csrc/corpus.hip made explicit: every fp64 operation below is one IEEE operation on arrays (numpy does
not contract a * b + c into an FMA), sums over the points of a voxel are sequential in ascending point order (not
np.sum, which adds pairwise).  The tests compare the device output with this bit for bit."""
import numpy as np
from scipy.spatial import cKDTree


def backproject(depth, pose, intrinsic, depth_shift=1000.0):
  """One frame: uint16 [H, W] -> world points fp64 [n, 3] in row-major pixel order (pixels with depth 0 dropped)."""
  K = np.asarray(intrinsic, dtype=np.float64)
  P = np.asarray(pose, dtype=np.float64)
  fx, fy, cx, cy, bx, by = K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[0, 3], K[1, 3]
  H, W = depth.shape
  v, u = np.divmod(np.arange(H * W, dtype=np.int64), W)
  raw = depth.reshape(-1)
  keep = raw != 0
  u, v = u[keep].astype(np.float64), v[keep].astype(np.float64)
  d = raw[keep].astype(np.float64) / np.float64(depth_shift)
  X = ((u - cx) * d) / fx + bx
  Y = ((v - cy) * d) / fy + by
  out = np.empty((len(d), 3))
  for r in range(3):
    out[:, r] = ((X * P[r, 0] + Y * P[r, 1]) + d * P[r, 2]) + P[r, 3]
  return out


def frame_reason(points, pose):
  """'' for a valid frame, else why it is left out: 'pose' (non-finite entry), 'nan' (a NaN point), 'empty'."""
  if not np.isfinite(pose).all():
    return "pose"
  if np.isnan(points).any():
    return "nan"
  if len(points) == 0:
    return "empty"
  return ""


def voxel_centroids(points, voxel):
  """open3d voxel_down_sample restated: origin = min bound - voxel / 2, index = floor((p - origin) / voxel), centroid =
  sequential sum of the voxel's points in ascending order (starting from 0.0) / count, rows by first occurrence."""
  p = np.asarray(points, dtype=np.float64)
  origin = p.min(0) - 0.5 * voxel
  idx = np.floor((p - origin) / voxel).astype(np.int64)
  m = idx.max(0) + 1 if len(idx) else np.ones(3, np.int64)
  key = (idx[:, 0] * m[1] + idx[:, 1]) * m[2] + idx[:, 2]
  _, first, inv = np.unique(key, return_index=True, return_inverse=True)
  order = np.argsort(first, kind="stable")  # unique keys -> output rows by first occurrence
  rank_of = np.empty_like(order)
  rank_of[order] = np.arange(len(order))
  vid = rank_of[inv.reshape(-1)]
  n_vox = len(first)
  # sequential sums: visit the points of every voxel level by level (the k-th point of each voxel at level k)
  srt = np.argsort(vid, kind="stable")
  sv = vid[srt]
  start = np.searchsorted(sv, np.arange(n_vox))
  level = np.arange(len(sv)) - start[sv]
  by_level = srt[np.argsort(level, kind="stable")]
  bounds = np.concatenate([[0], np.cumsum(np.bincount(level))]) if len(level) else np.zeros(1, np.int64)
  sums = np.zeros((n_vox, 3))
  for k in range(len(bounds) - 1):
    sel = by_level[bounds[k]:bounds[k + 1]]
    sums[vid[sel]] += p[sel]  # each voxel at most once per level: one rounding per addition, in point order
  cnt = np.bincount(vid, minlength=n_vox).astype(np.float64)
  return sums / cnt[:, None]


def _within(q, p, r):
  ex, ey, ez = q[:, 0] - p[:, 0], q[:, 1] - p[:, 1], q[:, 2] - p[:, 2]
  return ((ex * ex + ey * ey) + ez * ez) <= np.float64(r) * np.float64(r)


def overlap_counts(downs, r):
  """C[i, j] = #{q in D_j : some p in D_i with ((ex ex + ey ey) + ez ez) <= r r, e = q - p}, zero diagonal.  One
  cKDTree per source frame answers the nearest-neighbour query for every point of every frame; points whose distance
  is within 1e-9 of r either way get the exact rounded test against all their candidates."""
  F = len(downs)
  allq = np.concatenate(downs) if F else np.zeros((0, 3))
  frame_of = np.repeat(np.arange(F), [len(d) for d in downs])
  C = np.zeros((F, F), np.int64)
  for i in range(F):
    tree = cKDTree(downs[i])
    dist, _ = tree.query(allq, k=1, distance_upper_bound=r * (1 + 1e-6), workers=8)
    hit = dist <= r * (1 - 1e-9)
    unsure = np.flatnonzero((dist > r * (1 - 1e-9)) & (dist <= r * (1 + 1e-9)))
    if len(unsure):
      for q, cand in zip(unsure, tree.query_ball_point(allq[unsure], r * (1 + 1e-6))):
        cand = np.asarray(cand, np.int64)
        hit[q] = bool(len(cand)) and bool(_within(np.repeat(allq[q:q + 1], len(cand), 0), downs[i][cand], r).any())
    C[i] = np.bincount(frame_of[hit], minlength=F)
    C[i, i] = 0
  return C


def overlap_counts_bruteforce(downs, r):
  """The same matrix from the full distance table (small inputs only)."""
  F = len(downs)
  C = np.zeros((F, F), np.int64)
  for i in range(F):
    for j in range(F):
      if i == j:
        continue
      q, p = downs[j], downs[i]
      qq = np.repeat(q, len(p), 0)
      pp = np.tile(p, (len(q), 1))
      C[i, j] = int(_within(qq, pp, r).reshape(len(q), len(p)).any(1).sum())
  return C


def process_scene(depths, poses, intrinsic, voxel_size=0.05, depth_shift=1000.0):
  """Steps 1-5 for one scene; same keys as pair_corpus.process_scene (without timings)."""
  F = len(depths)
  pts = [backproject(depths[f], poses[f], intrinsic, depth_shift) for f in range(F)]
  reasons = [frame_reason(pts[f], np.asarray(poses[f])) for f in range(F)]
  frames = np.array([f for f in range(F) if reasons[f] == ""], np.int64)
  points = [pts[f] for f in frames]
  downs = [voxel_centroids(p, voxel_size) for p in points]
  C = overlap_counts(downs, 1.5 * voxel_size)
  nv = np.array([len(d) for d in downs], np.float64)
  M = C.astype(np.float64) / nv[None, :] if len(downs) else np.zeros((0, 0))
  return dict(valid=np.array([r == "" for r in reasons]), reasons=reasons,
              dropped={k: reasons.count(k) for k in ("pose", "nan", "empty")}, frames=frames, points=points,
              centroids=downs, C=C, M=M)


# ---- synthetic scenes ------------------------------------------------------------------------------------------------
def intrinsic_matrix(width=640, height=480, f=577.0):
  K = np.eye(4)
  K[0, 0] = K[1, 1] = f * width / 640.0
  K[0, 2], K[1, 2] = (width - 1) / 2.0, (height - 1) / 2.0
  return K


def synthetic_scene(n_frames=12, width=640, height=480, seed=0, step=0.12):
  """Depth frames (uint16 millimetres) ray-cast in a furnished room of lib/synthetic.py along a walking trajectory
  that turns the camera: nearby frames overlap a lot, distant ones little.  Returns (depths, poses, intrinsic)."""
  from pointcontrast_amd.lib import synthetic as sy
  rng = np.random.RandomState(seed)
  room, boxes = sy._make_room(rng)
  K = intrinsic_matrix(width, height)
  f = K[0, 0]
  depths, poses = [], []
  yaw0 = rng.uniform(0, 2 * np.pi)
  for k in range(n_frames):
    o = np.array([2.5 + 1.2 * np.cos(0.3 * k * step / 0.12), 2.0 + 0.9 * np.sin(0.3 * k * step / 0.12), 1.5])
    R = sy._look_at(yaw0 + k * step * 2.0, 0.3)
    # pixel (u, v) centre ray in camera space: ((u - cx) / f, (v - cy) / f, 1)
    u, v = np.meshgrid(np.arange(width), np.arange(height))
    dc = np.stack([(u - K[0, 2]) / f, (v - K[1, 2]) / f, np.ones_like(u, dtype=np.float64)], -1).reshape(-1, 3)
    dw = dc @ R.T
    t = sy._raycast(o, dw / np.linalg.norm(dw, axis=1, keepdims=True), room, boxes)
    z = t / np.linalg.norm(dc, axis=1)  # depth along the optical axis
    mm = np.round(z * 1000.0)
    mm[(mm > 65535) | ~np.isfinite(mm)] = 0
    mm[rng.rand(len(mm)) < 0.02] = 0  # sensor holes
    depths.append(mm.reshape(height, width).astype(np.uint16))
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = R, o
    poses.append(P)
  return np.stack(depths), np.stack(poses), K
