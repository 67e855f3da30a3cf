"""Plain numpy / float64 torch references and input builders for tests/test_gpu_pretrain_edges.py: the pre-training
path's data-dependent kernels (coordinate manager, loader geometry, pair selection, hard-negative mining, key set,
hardest-contrastive loss) at their packing and dispatch edges.  No device code here; tests/test_pretrain_edge_ref.py
checks every function against the oracle where the two overlap, so that a wrong reference cannot hide a wrong kernel.
"""
import numpy as np
import torch

E = (1 << 17) - 1  # the largest |coordinate| of a level-0 row (include/pcmi.h)


# ---- coordinate manager ---------------------------------------------------------------------------------------------
def edge_cloud():
  """int32 [n, 4] rows (b, x, y, z) on the rim of the packable range: the corner -E and its neighbours at distance 1, 2
  and 16 (one, two and four levels of stride 2 apart), the opposite corner, mixed-sign corners and interior rows, each in
  batch indices 0 and 1022.  Every strided level of the negative corner sits at -2^17, one below what level 0 accepts."""
  xyz = [(-E, -E, -E), (-E + 1, -E, -E), (-E + 2, -E, -E), (-E + 16, -E, -E), (-E, -E + 1, -E), (-E, -E, -E + 2),
         (-E + 3, -E + 3, -E + 3), (-E + 16, -E + 16, -E + 16),
         (E, E, E), (E - 1, E, E), (E - 2, E, E), (E - 16, E, E), (E, E - 1, E - 1), (E - 16, E - 16, E - 16),
         (-E, E, -E), (E, -E, E), (-E, -E, E), (E, E, -E), (-E, E, E), (E, -E, -E), (-E + 1, E, -E + 1), (E - 1, -E, E),
         (-E, 0, 0), (0, -E, 0), (0, 0, -E), (E, 0, 0), (0, 0, E), (-E, 1, E),
         (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, -1, -1), (-1, 0, 0), (2, 2, 2), (5, 7, -3), (16, 16, 16),
         (-16, 0, 15), (-8, -8, -8), (7, 7, 7), (3, -4, 12), (-17, 16, -15)]
  assert len(set(xyz)) == len(xyz)
  rows = [(b,) + p for b in (0, 1022) for p in xyz]
  return np.asarray(rows, dtype=np.int32)


def centre_slice(region):
  """Index of the (0, 0, 0) offset of a 3^3 kernel: HYPERCUBE (0) enumerates axis 0 fastest from -1, so it is
  1 + 3 + 9 = 13; HYBRID (3) puts the centre first."""
  return {0: 13, 3: 0}[region]


def segments_ref(batch):
  """The row -> instance CSR of a key from its batch-index column: rows grouped by ascending batch index, ascending row
  inside a group (a stable sort); offs [n_inst + 1]; inst [n] = instance of every row; the distinct batch indices."""
  batch = np.asarray(batch, dtype=np.int64)
  rows = np.argsort(batch, kind="stable").astype(np.int32)
  uniq, inv, counts = np.unique(batch, return_inverse=True, return_counts=True)
  offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
  return dict(rows=rows, offs=offs, inst=inv.astype(np.int32), n_inst=len(uniq), batches=uniq.astype(np.int32))


# ---- hard-negative mining -------------------------------------------------------------------------------------------
def pdist_ref(a, b):
  """float64 D[p, s] = sqrt(|a_p - b_s|^2 + 1e-7) with its row minimum and FIRST arg-min in torch.min's order: NaN is
  below every number, so a row that holds a NaN has dmin = NaN and amin = its first NaN position."""
  a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
  with np.errstate(invalid="ignore", over="ignore"):
    D = np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(2) + 1e-7)
  nan = np.isnan(D)
  amin = np.where(nan.any(1), nan.argmax(1), np.where(nan, np.inf, D).argmin(1))
  return D, D[np.arange(len(D)), amin], amin.astype(np.int64)


# ---- hardest-contrastive loss ---------------------------------------------------------------------------------------
def hardest_ref(posF0, posF1, subF0, subF1, i01, m0, i10, m1, pos_thresh, neg_thresh):
  """include/pcmi.h's formulas in float64 autograd, given the mined rows and the masks:
    pos = mean(relu(|a - b|^2 - pt)),  neg = (mean_{m0}(relu(nt - D01)^2) + mean_{m1}(relu(nt - D10)^2)) / 2,
    D01 = sqrt(|posF0 - subF1[i01]|^2 + 1e-7), D10 = sqrt(|posF1 - subF0[i10]|^2 + 1e-7).
  Returns (pos, neg, D01, D10, [d posF0, d posF1, d subF0, d subF1] of pos + neg).  The mean over an empty mask is NaN
  (0 / 0), as torch's; its gradient is empty, i.e. zero on that side."""
  ts = [torch.as_tensor(np.asarray(t), dtype=torch.float64).clone().requires_grad_(True) for t in (posF0, posF1, subF0, subF1)]
  a, b, s0, s1 = ts
  i01, i10 = torch.as_tensor(np.asarray(i01), dtype=torch.int64), torch.as_tensor(np.asarray(i10), dtype=torch.int64)
  m0, m1 = torch.as_tensor(np.asarray(m0)).bool(), torch.as_tensor(np.asarray(m1)).bool()
  D01 = torch.sqrt((a - s1[i01]).pow(2).sum(1) + 1e-7)
  D10 = torch.sqrt((b - s0[i10]).pow(2).sum(1) + 1e-7)
  pos = torch.relu((a - b).pow(2).sum(1) - pos_thresh).mean()
  neg = (torch.relu(neg_thresh - D01[m0]).pow(2).mean() + torch.relu(neg_thresh - D10[m1]).pow(2).mean()) / 2
  grads = torch.autograd.grad(pos + neg, ts)  # (nothing flows back through the mean of an empty selection)
  return pos.detach(), neg.detach(), D01.detach(), D10.detach(), grads


# ---- key set --------------------------------------------------------------------------------------------------------
def keyset_absent_ref(pairs, M, a, b):
  """mask[i] = 1 iff a[i] + b[i] * M is not among pairs[:, 0] + pairs[:, 1] * M (int64; pc/lib/ddp_trainer.py's _hash +
  np.isin).  Distinct pairs with the same key are the same member: that is the reference's behaviour."""
  pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
  keys = pairs[:, 0] + pairs[:, 1] * np.int64(M)
  q = np.asarray(a, dtype=np.int64) + np.asarray(b, dtype=np.int64) * np.int64(M)
  return np.logical_not(np.isin(q, keys))


# ---- positive-pair selection ----------------------------------------------------------------------------------------
def pair_select_ref(pairs, uniform, sampled=None):
  """One key per run of column 0 (pairs sorted by it): the floor(float32(u) * float32(count))-th pair of the run, one
  float32 rounding; then the optional sub-sample.  A `sampled` entry outside [0, n_runs) gives (0, 0), as
  csrc/pairs.hip documents.  Returns (q, k, start, count) -- the run bounds let a caller check that the pick stays inside
  its run."""
  pairs = np.asarray(pairs, dtype=np.int64)
  starts = np.flatnonzero(np.concatenate([[True], pairs[1:, 0] != pairs[:-1, 0]]))
  counts = np.diff(np.concatenate([starts, [len(pairs)]]))
  u = np.asarray(uniform, dtype=np.float32)
  assert len(u) == len(starts)
  off = np.floor(u * counts.astype(np.float32)).astype(np.int64)
  q_all, k_all = pairs[starts, 0], pairs[np.minimum(starts + off, len(pairs) - 1), 1]
  if sampled is None:
    return q_all, k_all, starts, counts
  s = np.asarray(sampled, dtype=np.int64)
  ok = (s >= 0) & (s < len(starts))
  sc = np.where(ok, s, 0)
  return np.where(ok, q_all[sc], 0), np.where(ok, k_all[sc], 0), np.where(ok, starts[sc], 0), np.where(ok, counts[sc], 0)


def runs_of(lengths, first=0, step=3):
  """Column 0 of sorted correspondences with the given run lengths (strictly increasing query ids)."""
  lengths = np.asarray(lengths, dtype=np.int64)
  return np.repeat(first + step * np.arange(len(lengths), dtype=np.int64), lengths).astype(np.int32)


# ---- loader geometry ------------------------------------------------------------------------------------------------
def _finite_or_raise(x, what):
  if not np.isfinite(x).all():
    raise ValueError("%s: non-finite coordinate" % what)


def apply_rigid_ref(T, p):
  """((R0 x + R1 y) + R2 z) + t, every operation rounded on its own (float64 numpy does not contract)."""
  T, p = np.asarray(T, dtype=np.float64), np.asarray(p, dtype=np.float64)
  with np.errstate(invalid="ignore", over="ignore"):  # (non-finite points are the caller's to refuse)
    return np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], 1)


def match_bruteforce(src, T, dst, radius):
  """All (i, j) with ((ex ex + ey ey) + ez ez) <= r r, e = T(src_i) - dst_j, by testing EVERY pair: no cell grid, so it
  vouches for the 27-cell search that the kernel and oracle/loader_ref.py share.  Returns (int64 [P, 2] sorted by (i, j),
  the number of pairs exactly ON the radius)."""
  q, d = apply_rigid_ref(T, src), np.asarray(dst, dtype=np.float64)
  _finite_or_raise(q, "match_bruteforce src")
  _finite_or_raise(d, "match_bruteforce dst")
  r = np.float64(radius)
  ex, ey, ez = (q[:, None, k] - d[None, :, k] for k in range(3))
  d2 = (ex * ex + ey * ey) + ez * ez
  i, j = np.nonzero(d2 <= r * r)  # row-major: sorted by (i, j)
  return np.stack([i, j], 1).astype(np.int64), int((d2 == r * r).sum())


def voxelize_ref(xyz, voxel):
  """(ascending indices of the first point of every occupied voxel of floor(xyz / voxel), those voxels' coordinates).
  Rows are compared as rows (no packed key that could wrap at +-2^20)."""
  x = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
  _finite_or_raise(x, "voxelize_ref")
  q = np.floor(x / np.float64(voxel)).astype(np.int64)
  if len(q) == 0:
    return np.zeros(0, np.int64), np.zeros((0, 3), np.int32)
  _, first = np.unique(q, axis=0, return_index=True)
  first = np.sort(first).astype(np.int64)
  return first, q[first].astype(np.int32)


def lattice_points(seed, n=500, half=12, step=2.0 ** -6):
  """n distinct points on multiples of `step` in [-half, half)^3 * step: with radius 2 * step every difference, product
  and sum of the distance test is exact, so d2 == r2 happens exactly, and points lie on the faces of the radius cells."""
  rng = np.random.RandomState(seed)
  cells = rng.permutation((2 * half) ** 3)[:n]
  ijk = np.stack([cells // (2 * half) ** 2, (cells // (2 * half)) % (2 * half), cells % (2 * half)], 1) - half
  return ijk.astype(np.float64) * step


ROT_Z90 = np.array([[0.0, -1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])


def match_cases():
  """[(name, src, dst, radius)]: the exact dyadic lattice; the same moved by +-1 ulp per coordinate at random (pairs on
  the radius fall to either side, points on cell faces to either cell); a lattice of 0.025 voxels with r = 1.5 voxels
  (the loader's own geometry, where no product is exact)."""
  src, dst = lattice_points(1), lattice_points(2)
  rng = np.random.RandomState(3)
  nudge = lambda p: np.nextafter(p, np.where(rng.randint(0, 2, p.shape) == 1, np.inf, -np.inf))
  vs, vd = lattice_points(4, step=0.025), lattice_points(5, step=0.025)
  return [("exact", src, dst, 2.0 ** -5), ("ulp", nudge(src), nudge(dst), 2.0 ** -5), ("voxel", vs, vd, 0.0375)]
