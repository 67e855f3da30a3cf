"""numpy restatement of csrc/views.hip (TEST INFRASTRUCTURE): the projection rule, the z-buffer and the visibility test of
include/pcmi.h, every fp64 operation one IEEE operation on arrays (numpy does not contract a * b + c into an FMA), plus a
scalar triple-loop spelling of the same rule for a few hundred points, the synthetic room the view tests share and the
whole process_scan through tests/pair_corpus_ref.py.  The device output is compared with this bit for bit."""
import math

import numpy as np


def project(points, M, fx, fy, cx, cy, z_near, z_far):
  """One view: (ok bool [n], px, py float64 [n] (NaN where not ok), zf float32 [n])."""
  p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
  M = np.asarray(M, dtype=np.float64).reshape(4, 4)
  x, y, z = p[:, 0], p[:, 1], p[:, 2]
  with np.errstate(all="ignore"):
    X = ((x * M[0, 0] + y * M[0, 1]) + z * M[0, 2]) + M[0, 3]
    Y = ((x * M[1, 0] + y * M[1, 1]) + z * M[1, 2]) + M[1, 3]
    Z = ((x * M[2, 0] + y * M[2, 1]) + z * M[2, 2]) + M[2, 3]
    ok = np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z) & (Z >= z_near) & (Z <= z_far)
    Zs = np.where(ok, Z, 1.0)
    u = (X * np.float64(fx)) / Zs + np.float64(cx)
    v = (Y * np.float64(fy)) / Zs + np.float64(cy)
    px = np.where(ok, np.floor(u + 0.5), np.nan)
    py = np.where(ok, np.floor(v + 0.5), np.nan)
    zf = np.where(ok, Z, 0.0).astype(np.float32)
  return ok, px, py, zf


def zbuffer(points, w2c, fx, fy, cx, cy, H, W, z_near, z_far, splat):
  """float32 [F, H, W], +inf where empty."""
  w2c = np.asarray(w2c, dtype=np.float64).reshape(-1, 4, 4)
  half = splat // 2
  out = np.full((len(w2c), H * W), np.inf, np.float32)
  for f, M in enumerate(w2c):
    ok, px, py, zf = project(points, M, fx, fy, cx, cy, z_near, z_far)
    for dy in range(-half, half + 1):
      for dx in range(-half, half + 1):
        with np.errstate(invalid="ignore"):
          qx, qy = px + dx, py + dy
          sel = ok & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
        idx = qy[sel].astype(np.int64) * W + qx[sel].astype(np.int64)
        np.minimum.at(out[f], idx, zf[sel])
  return out.reshape(len(w2c), H, W)


def visible_mask(points, w2c, fx, fy, cx, cy, H, W, z_near, z_far, rel_tol, zbuf):
  """bool [F, n]."""
  w2c = np.asarray(w2c, dtype=np.float64).reshape(-1, 4, 4)
  n = np.asarray(points).reshape(-1, 3).shape[0]
  out = np.zeros((len(w2c), n), bool)
  tol = np.float64(1.0) + np.float64(rel_tol)
  for f, M in enumerate(w2c):
    ok, px, py, zf = project(points, M, fx, fy, cx, cy, z_near, z_far)
    with np.errstate(invalid="ignore"):
      inside = ok & (px >= 0) & (px < W) & (py >= 0) & (py < H)
    k = np.flatnonzero(inside)
    zb = zbuf[f, py[k].astype(np.int64), px[k].astype(np.int64)]
    with np.errstate(all="ignore"):
      out[f, k] = zf[k].astype(np.float64) <= zb.astype(np.float64) * tol
  return out


def render(points, w2c, fx, fy, cx, cy, H, W, z_near, z_far, splat, rel_tol):
  """dict(zbuf, mask bool [F, n], rows int32 [total], offsets int64 [F + 1], pixels int64 [F])."""
  w2c = np.asarray(w2c, dtype=np.float64).reshape(-1, 4, 4)
  zb = zbuffer(points, w2c, fx, fy, cx, cy, H, W, z_near, z_far, splat)
  m = visible_mask(points, w2c, fx, fy, cx, cy, H, W, z_near, z_far, rel_tol, zb)
  rows = [np.flatnonzero(r).astype(np.int32) for r in m]
  offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
  return dict(zbuf=zb, mask=m, rows=np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32), offsets=offsets,
              pixels=np.isfinite(zb).reshape(len(w2c), -1).sum(1).astype(np.int64))


def render_scalar(points, w2c, fx, fy, cx, cy, H, W, z_near, z_far, splat, rel_tol):
  """The same rule spelled with Python scalars (float is IEEE fp64; np.float32 rounds the depth), one point, one view and
  one pixel at a time.  A few hundred points at most."""
  pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
  w2c = np.asarray(w2c, dtype=np.float64).reshape(-1, 4, 4)
  F, n, half = len(w2c), len(pts), splat // 2
  zb = np.full((F, H, W), np.inf, np.float32)
  proj = {}
  for f in range(F):
    M = [[float(a) for a in row] for row in w2c[f]]
    for i in range(n):
      x, y, z = (float(a) for a in pts[i])
      X = ((x * M[0][0] + y * M[0][1]) + z * M[0][2]) + M[0][3]
      Y = ((x * M[1][0] + y * M[1][1]) + z * M[1][2]) + M[1][3]
      Z = ((x * M[2][0] + y * M[2][1]) + z * M[2][2]) + M[2][3]
      if not (math.isfinite(X) and math.isfinite(Y) and math.isfinite(Z) and z_near <= Z <= z_far):
        continue
      u = (X * fx) / Z + cx
      v = (Y * fy) / Z + cy
      px, py, zf = math.floor(u + 0.5), math.floor(v + 0.5), np.float32(Z)
      proj[f, i] = (px, py, zf)
      for yy in range(max(py - half, 0), min(py + half, H - 1) + 1):
        for xx in range(max(px - half, 0), min(px + half, W - 1) + 1):
          if zf < zb[f, yy, xx]:
            zb[f, yy, xx] = zf
  rows, offsets = [], [0]
  for f in range(F):
    for i in range(n):
      if (f, i) in proj:
        px, py, zf = proj[f, i]
        if 0 <= px < W and 0 <= py < H and float(zf) <= float(zb[f, py, px]) * (1.0 + rel_tol):
          rows.append(i)
    offsets.append(len(rows))
  return dict(zbuf=zb, rows=np.array(rows, np.int32), offsets=np.array(offsets, np.int64),
              pixels=np.isfinite(zb).reshape(F, -1).sum(1).astype(np.int64))


def world_to_camera(poses):
  """inv of every camera-to-world pose, one at a time (scan_views.world_to_camera's rule); a non-finite pose gives NaNs."""
  poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
  out = np.full(poses.shape, np.nan)
  for f, P in enumerate(poses):
    if np.isfinite(P).all():
      out[f] = np.linalg.inv(P)
  return out


def process_scan(xyz, poses, intrinsic, H, W, z_near=0.1, z_far=10.0, splat=3, rel_tol=0.05, color=None, voxel_size=0.05,
                 min_coverage=0.5):
  """scan_views.process_scan restated; same keys (without timings)."""
  import pair_corpus_ref as pr
  xyz = np.asarray(xyz, dtype=np.float64)
  poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
  K = np.asarray(intrinsic, dtype=np.float64)
  r = render(xyz, world_to_camera(poses), K[0, 0], K[1, 1], K[0, 2], K[1, 2], H, W, z_near, z_far, splat, rel_tol)
  F = len(poses)
  coverage = r["pixels"].astype(np.float64) / np.float64(H * W)
  reasons = []
  for f in range(F):
    if not np.isfinite(poses[f]).all():
      reasons.append("pose")
    elif r["offsets"][f + 1] == r["offsets"][f]:
      reasons.append("empty")
    elif coverage[f] < min_coverage:
      reasons.append("coverage")
    else:
      reasons.append("")
  frames = np.array([f for f in range(F) if reasons[f] == ""], np.int64)
  rows = [r["rows"][r["offsets"][f]:r["offsets"][f + 1]] for f in frames]
  points = [xyz[k] for k in rows]
  downs = [pr.voxel_centroids(p, voxel_size) for p in points]
  C = pr.overlap_counts(downs, 1.5 * voxel_size) if len(downs) else np.zeros((0, 0), np.int64)
  nv = np.array([len(d) for d in downs], np.float64)
  M = C.astype(np.float64) / nv[None, :] if len(downs) else np.zeros((0, 0))
  out = dict(valid=np.array([x == "" for x in reasons]), reasons=reasons,
             dropped={k: reasons.count(k) for k in ("pose", "empty", "coverage")}, frames=frames, rows=rows, points=points,
             centroids=downs, C=C, M=M, coverage=coverage)
  if color is not None:
    out["colors"] = [np.asarray(color)[k] for k in rows]
  return out


# ---- a synthetic room --------------------------------------------------------------------------------------------------
ROOM = (5.0, 4.0, 2.6)  # x, y, z extent; the floor is z = 0
BOXES = (((0.6, 0.5, 0.0), (1.6, 1.3, 0.8)), ((3.2, 2.4, 0.0), (4.2, 3.4, 1.2)), ((2.2, 0.3, 0.0), (2.9, 0.9, 0.5)))


def _box_surface(lo, hi, n, rng, faces=range(6)):
  """n points sampled uniformly on the listed faces of an axis-aligned box (face 2 a + s: axis a at lo (s = 0) or hi)."""
  lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
  ext = hi - lo
  faces = list(faces)
  area = np.array([ext[(f // 2 + 1) % 3] * ext[(f // 2 + 2) % 3] for f in faces])
  which = rng.choice(len(faces), size=n, p=area / area.sum())
  p = lo + rng.rand(n, 3) * ext
  for k, f in enumerate(faces):
    sel = which == k
    p[sel, f // 2] = lo[f // 2] if f % 2 == 0 else hi[f // 2]
  return p


def synthetic_room(n=12000, seed=0, offset=(0.0, 0.0, 0.0)):
  """(xyz float64 [n, 3], color uint8 [n, 3]): the shell of ROOM (walls, floor, ceiling) and the surfaces of BOXES without
  their undersides, surface-sampled."""
  rng = np.random.RandomState(seed)
  n_shell = int(n * 0.7)
  parts = [_box_surface((0, 0, 0), ROOM, n_shell, rng)]
  per = (n - n_shell) // len(BOXES)
  for k, (lo, hi) in enumerate(BOXES):
    m = per if k + 1 < len(BOXES) else n - n_shell - per * (len(BOXES) - 1)
    parts.append(_box_surface(lo, hi, m, rng, faces=(0, 1, 2, 3, 5)))
  xyz = np.concatenate(parts) + np.asarray(offset, np.float64)
  xyz = xyz[rng.permutation(len(xyz))]
  color = rng.randint(0, 256, size=(len(xyz), 3)).astype(np.uint8)
  return xyz, color


def look_pose(position, yaw, pitch):
  """Camera-to-world, x right, y down, z forward, z up in the world: forward = (cos p cos y, cos p sin y, sin p) (written
  out apart from scan_views.camera_pose on purpose)."""
  cp, sp, cy, sy = math.cos(pitch), math.sin(pitch), math.cos(yaw), math.sin(yaw)
  fwd = np.array([cp * cy, cp * sy, sp])
  right = np.array([sy, -cy, 0.0])
  down = np.cross(fwd, right)
  P = np.eye(4)
  P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = right, down, fwd, position
  return P


PLANTED_YAWS = (0.0, 0.25, 0.5, 0.9, 1.3, 1.8, 2.4, 3.2)
PLANTED_DROPS = {8: "coverage", 9: "empty", 10: "pose"}


def planted_poses(offset=(0.0, 0.0, 0.0)):
  """Eleven cameras for synthetic_room: eight near its middle that turn by growing steps (near neighbours overlap a lot, far
  ones a little or not at all), then the three of PLANTED_DROPS: one 0.3 m in front of a wall (a handful of pixels), one
  outside the room looking away from it, one with a NaN in its pose."""
  off = np.asarray(offset, np.float64)
  out = []
  for k, yaw in enumerate(PLANTED_YAWS):
    pos = np.array([2.5 + 0.3 * math.cos(0.7 * k), 2.0 + 0.3 * math.sin(0.7 * k), 1.5]) + off
    out.append(look_pose(pos, yaw, math.radians(-15.0)))
  out.append(look_pose(np.array([4.7, 2.0, 1.5]) + off, 0.0, 0.0))
  out.append(look_pose(np.array([5.5, 2.0, 1.5]) + off, 0.0, 0.0))
  bad = np.eye(4)
  bad[0, 3] = np.nan
  out.append(bad)
  return np.stack(out)


def small_intrinsic(H, W, f):
  K = np.eye(4)
  K[0, 0] = K[1, 1] = f
  K[0, 2], K[1, 2] = (W - 1) / 2.0, (H - 1) / 2.0
  return K
