"""CPU restatements of the point-set ops of csrc/pointset.hip (include/pcmi.h "PointNet++ point-set ops").

Index results use numpy float32 in the library's fixed order, ((dx*dx) + (dy*dy)) + (dz*dz) with every operation rounded
on its own, so they equal the device's bit for bit.  Float results are float64; gradients come from torch autograd over
the float64 forward functions.  tests/test_pointset_ref.py pins this file against brute force and gradcheck."""
import numpy as np
import torch

F32 = np.float32


def sq_dist(pts, c):
  """float32 squared distances of pts [n, 3] to the point c [3], in the library's order."""
  pts, c = np.asarray(pts, F32).reshape(-1, 3), np.asarray(c, F32)
  dx, dy, dz = pts[:, 0] - c[0], pts[:, 1] - c[1], pts[:, 2] - c[2]
  return ((dx * dx) + (dy * dy)) + (dz * dz)


def qualifies(pts):
  pts = np.asarray(pts, F32).reshape(-1, 3)
  x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
  return (((x * x) + (y * y)) + (z * z)) > F32(1e-3)


def fps(pts, m, tie_free=False):
  """Furthest point sampling of one cloud pts [n, 3]: int32 [m] positions (-1 for an empty cloud).  tie_free: assert that
  every pick with a positive running minimum is the only point that attains it (a fixture meant to have no ties)."""
  pts = np.asarray(pts, F32).reshape(-1, 3)
  n = len(pts)
  out = np.full(m, -1, np.int32)
  if n == 0:
    return out
  ok = qualifies(pts)
  mind = np.full(n, F32(1e10), F32)
  out[0] = 0
  prev = 0
  for j in range(1, m):
    d = sq_dist(pts, pts[prev])
    mind = np.where(ok, np.minimum(mind, d), mind)
    pick = 0
    if ok.any():
      cand = np.where(ok, mind, F32(-1))
      pick = int(np.argmax(cand))  # the first maximum: the lowest index
      if tie_free and cand[pick] > 0:
        assert int((cand == cand[pick]).sum()) == 1, "fixture has a tie at pick %d" % j
    out[j] = pick
    prev = pick
  return out


def fps_segments(xyz, offs, rows, m, tie_free=False):
  """(positions [B, m], rows of xyz [B, m]) over the segments offs [B + 1] / rows (None: contiguous)."""
  xyz = np.asarray(xyz, F32).reshape(-1, 3)
  B = len(offs) - 1
  pos, row = np.full((B, m), -1, np.int32), np.full((B, m), -1, np.int32)
  for i in range(B):
    r = np.arange(offs[i], offs[i + 1]) if rows is None else np.asarray(rows)[offs[i]:offs[i + 1]]
    pos[i] = fps(xyz[r], m, tie_free)
    if len(r):
      row[i] = r[pos[i]]
  return pos, row


def ball_query(xyz, new_xyz, radius, nsample):
  """xyz [B, n, 3], new_xyz [B, np, 3] -> int32 [B, np, nsample]."""
  xyz, new_xyz = np.asarray(xyz, F32), np.asarray(new_xyz, F32)
  B, npnt = new_xyz.shape[:2]
  r2 = F32(radius) * F32(radius)
  out = np.zeros((B, npnt, nsample), np.int32)
  for b in range(B):
    for q in range(npnt):
      hits = np.nonzero(sq_dist(xyz[b], new_xyz[b, q]) < r2)[0][:nsample]
      if len(hits):
        out[b, q, :] = hits[0]
        out[b, q, :len(hits)] = hits
  return out


def three_nn(unknown, known):
  """unknown [B, n, 3], known [B, m, 3] -> (float32 SQUARED distances [B, n, 3], int32 indices [B, n, 3]); ascending scan with
  strict < == a stable sort by distance."""
  unknown, known = np.asarray(unknown, F32), np.asarray(known, F32)
  B, n = unknown.shape[:2]
  assert known.shape[1] >= 3
  d2, idx = np.zeros((B, n, 3), F32), np.zeros((B, n, 3), np.int32)
  for b in range(B):
    for u in range(n):
      d = sq_dist(known[b], unknown[b, u])
      o = np.argsort(d, kind="stable")[:3]
      d2[b, u], idx[b, u] = d[o], o
  return d2, idx


# ---- float results: torch, any dtype (the tests use float64); differentiable in the features ----------------------------------
def gather(feat, idx):
  """feat [B, C, N], idx [B, m] -> [B, C, m]."""
  B, C, _ = feat.shape
  return torch.gather(feat, 2, idx.long().unsqueeze(1).expand(B, C, idx.shape[1]))


def group(feat, idx):
  """feat [B, C, N], idx [B, np, ns] -> [B, C, np, ns]."""
  B, npnt, ns = idx.shape
  return gather(feat, idx.reshape(B, npnt * ns)).reshape(B, feat.shape[1], npnt, ns)


def interpolate(feat, idx, weight):
  """feat [B, C, M], idx / weight [B, n, 3] -> [B, C, n]."""
  B, n, _ = idx.shape
  g = gather(feat, idx.reshape(B, n * 3)).reshape(B, feat.shape[1], n, 3)
  return (g * weight.to(feat.dtype).unsqueeze(1)).sum(-1)


def grad_of(fn, feat, gout):
  """d sum(fn(feat) * gout) / d feat in float64."""
  f = feat.detach().double().cpu().requires_grad_(True)
  (fn(f) * gout.detach().double().cpu()).sum().backward()
  return f.grad


def rel_err(got, want):
  got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
  return float((got - want).abs().max() / max(float(want.abs().max()), 1e-30))
