"""float64 numpy restatement of the spatially partitioned PointInfoNCE (TEST INFRASTRUCTURE): the partition rule, the loss and
its gradients exactly as include/pcmi.h states them (csrc/nce_part.hip is held to this).  Dense: it builds the n x n partition
and logit matrices the kernels never write."""
import numpy as np


def sector(dx, dy, A):
  """The azimuth sector of integer (dx, dy) arrays in three steps (include/pcmi.h); A in {1, 2, 4, 8}."""
  dx, dy = np.asarray(dx, dtype=np.int64).copy(), np.asarray(dy, dtype=np.int64).copy()
  h = np.where((dy > 0) | ((dy == 0) & (dx > 0)), 0, 1)
  dx, dy = np.where(h == 1, -dx, dx), np.where(h == 1, -dy, dy)
  qd = np.where(dx > 0, 0, 1)
  dx, dy = np.where(qd == 1, dy, dx), np.where(qd == 1, -dx, dy)
  o = np.where(dy < dx, 0, 1)
  return {1: 0 * h, 2: h, 4: 2 * h + qd, 8: 4 * h + 2 * qd + o}[A]


def partition_matrix(xyz, scene, n_scenes, r1_sq, r2_sq, A, E):
  """part(i, j) as int8 [n, n]: row i the anchor, column j the candidate negative; -1 = in no partition."""
  xyz, scene = np.asarray(xyz, dtype=np.int64), np.asarray(scene, dtype=np.int64)
  n = len(xyz)
  d = xyz[None, :, :] - xyz[:, None, :]  # d[i, j] = xyz[j] - xyz[i]
  d2 = (d * d).sum(-1)
  ok = (scene >= 0) & (scene < n_scenes)
  none = np.eye(n, dtype=bool) | (d2 == 0) | (d2 > int(r2_sq)) | (scene[:, None] != scene[None, :]) | ~ok[:, None] | ~ok[None, :]
  shell = np.where(d2 <= int(r1_sq), 0, 1)
  el = np.where(d[..., 2] >= 0, 0, 1) if E == 2 else np.zeros_like(shell)
  part = (shell * E + el) * A + sector(d[..., 0], d[..., 1], A)
  return np.where(none, -1, part).astype(np.int8)


def loss_and_grads(q, k, xyz, scene, n_scenes, T, r1_sq, r2_sq, A, E, gscale=1.0, inv_T=None):
  """dict(loss, lse [n, P], rowlive [n, P] bool, live [B, P] counts, dq, dk, part, logits); lse of a (row, partition) that is
  not live is l_ii.  inv_T: the temperature's reciprocal if not 1 / T in float64 (the device takes it as fp32)."""
  q, k = np.asarray(q, dtype=np.float64), np.asarray(k, dtype=np.float64)
  scene = np.asarray(scene, dtype=np.int64)
  n, P, B = len(q), 2 * E * A, int(n_scenes)
  inv_T = 1.0 / float(T) if inv_T is None else float(inv_T)
  part = partition_matrix(xyz, scene, B, r1_sq, r2_sq, A, E)
  L = (q @ k.T) * inv_T
  lii = np.diag(L).copy()
  lse = np.repeat(lii[:, None], P, axis=1)
  rowlive = np.zeros((n, P), dtype=bool)
  for p in range(P):
    mask = part == p
    rowlive[:, p] = mask.any(1)
    m = np.maximum(lii, np.where(mask, L, -np.inf).max(1))
    s = np.exp(lii - m) + np.where(mask, np.exp(np.where(mask, L - m[:, None], 0.0)), 0.0).sum(1)
    lse[:, p] = np.where(rowlive[:, p], m + np.log(s), lii)
  live = np.zeros((B, P), dtype=np.int64)
  for s_ in range(B):
    live[s_] = rowlive[scene == s_].sum(0)
  Ls = (live > 0).sum(1)
  S = int((Ls > 0).sum())
  w = np.zeros((n, P))
  loss = 0.0
  for s_ in range(B):
    if Ls[s_] == 0:
      continue
    rows = scene == s_
    for p in range(P):
      if live[s_, p] == 0:
        continue
      sel = rows & rowlive[:, p]
      wt = 1.0 / (S * Ls[s_] * live[s_, p])
      w[sel, p] = wt
      loss += wt * (lse[sel, p] - lii[sel]).sum()
  G = np.zeros((n, n))
  for p in range(P):
    mask = part == p
    G += np.where(mask, w[:, p, None] * np.exp(np.where(mask, L - lse[:, p, None], 0.0)), 0.0)
  G[np.arange(n), np.arange(n)] = (w * (np.exp(lii[:, None] - lse) - 1.0)).sum(1)
  dq = float(gscale) * inv_T * (G @ k)
  dk = float(gscale) * inv_T * (G.T @ q)
  return dict(loss=float(loss), lse=lse, rowlive=rowlive, live=live, dq=dq, dk=dk, part=part, logits=L)
