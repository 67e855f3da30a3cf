"""oracle/loader_ref.py (the CPU restatement the device loader kernels are compared with) against independent
implementations: scipy's cKDTree for the radius search, the synthetic generator's own first-occurrence sub-sampling."""
from fractions import Fraction

import numpy as np
from scipy.spatial import cKDTree

from oracle import loader_ref as lf
from pointcontrast_amd.lib import synthetic


def _pair(seed, crop):
  rng = np.random.RandomState(seed)
  a, b = synthetic.make_frame_pair(rng)
  c = a[rng.randint(len(a))]
  a, b = a[np.linalg.norm(a - c, axis=1) < crop], b[np.linalg.norm(b - c, axis=1) < crop]
  T0, T1 = synthetic.sample_random_trans(a, rng), synthetic.sample_random_trans(b, rng)
  a, b = a @ T0[:3, :3].T + T0[:3, 3], b @ T1[:3, :3].T + T1[:3, 3]
  return a, b, T1 @ np.linalg.inv(T0)


def test_first_occurrence_index():
  a, _, _ = _pair(0, 0.8)
  sel = lf.sparse_quantize_index(a, 0.025)
  assert (sel == synthetic.sparse_quantize_index(a / 0.025)).all()
  q = np.floor(a / 0.025).astype(np.int64)
  assert len(np.unique(q[sel], axis=0)) == len(sel) == len(np.unique(q, axis=0)) and (np.diff(sel) > 0).all()
  for i in sel[:200]:  # really the FIRST point of its voxel
    assert not (q[:i] == q[i]).all(1).any()
  assert len(lf.sparse_quantize_index(np.zeros((0, 3)), 0.025)) == 0


def test_match_radius_against_kdtree():
  a, b, T = _pair(1, 0.7)
  a, b = a[lf.sparse_quantize_index(a, 0.025)], b[lf.sparse_quantize_index(b, 0.025)]
  r = 1.5 * 0.025
  got = lf.match_radius(a, T, b, r)
  src = a @ T[:3, :3].T + T[:3, 3]
  nb = cKDTree(b).query_ball_point(src, r)
  want = np.array([(i, j) for i, js in enumerate(nb) for j in sorted(js)], dtype=np.int64).reshape(-1, 2)
  assert len(got) > 1000
  # identical sets up to pairs whose distance is within round-off of the radius (the two sides round differently)
  gs, ws = set(map(tuple, got.tolist())), set(map(tuple, want.tolist()))
  for i, j in gs ^ ws:
    assert abs(np.linalg.norm(src[i] - b[j]) - r) < 1e-12
  assert len(gs ^ ws) <= 2
  assert (np.lexsort((got[:, 1], got[:, 0])) == np.arange(len(got))).all(), "sorted by (i, j)"
  assert lf.match_radius(a[:0], T, b, r).shape == (0, 2) and lf.match_radius(a, T, b[:0], r).shape == (0, 2)


def boundary_fixture():
  """2048 source points whose partner lies ON the radius up to round-off: q_i = T p_i + r u_i with |u_i| = 1, so the
  decision on (i, i) hangs on the last bits of d^2 -- on the order of the operations and on whether they are fused."""
  rng = np.random.RandomState(0)
  n, r = 2048, 1.5 * 0.025
  p = rng.uniform(-3.0, 3.0, (n, 3))
  T = np.eye(4)
  T[:3, :3] = np.linalg.qr(rng.normal(size=(3, 3)))[0]
  T[:3, 3] = rng.uniform(-1.0, 1.0, 3)
  u = rng.normal(size=(n, 3))
  u /= np.linalg.norm(u, axis=1, keepdims=True)
  return p, T, lf.apply_rigid(T, p) + r * u, r


def _fma(a, b, c):
  """round(a b + c), rounded once (float(Fraction) rounds to nearest even)."""
  return float(Fraction(a) * Fraction(b) + Fraction(c))


def _fused_diagonal(p, T, q, r):
  """The (i, i) decisions in the contracted order a compiler that fuses makes of the same expressions:
  t = T[k,1] p1; t = fma(T[k,0], p0, t); t = fma(T[k,2], p2, t); T[k,3] + t per row, then
  m = ey ey; m = fma(ex, ex, m); m = fma(ez, ez, m)."""
  keep = np.zeros(len(p), bool)
  for i in range(len(p)):
    s = []
    for k in range(3):
      t = float(T[k, 1] * p[i, 1])
      t = _fma(T[k, 0], p[i, 0], t)
      t = _fma(T[k, 2], p[i, 2], t)
      s.append(float(T[k, 3] + t))
    ex, ey, ez = (float(s[a] - q[i, a]) for a in range(3))
    m = _fma(ez, ez, _fma(ex, ex, ey * ey))
    keep[i] = m <= float(np.float64(r) * np.float64(r))
  return keep


def test_boundary_fixture_discriminates():
  """Conditions on the fixture alone, so that the device test on it (test_gpu_loader) cannot pass vacuously: about half
  of the on-the-radius pairs are kept, nothing else crowds a source point, and the fused order decides differently from
  the oracle on many of them."""
  p, T, q, r = boundary_fixture()
  got = lf.match_radius(p, T, q, r)
  diag = np.zeros(len(p), bool)
  diag[got[got[:, 0] == got[:, 1], 0]] = True
  per_source = np.bincount(got[:, 0], minlength=len(p))
  print("kept %d of %d (i, i) pairs, at most %d matches per source" % (diag.sum(), len(p), per_source.max()))
  assert 0.4 * len(p) <= diag.sum() <= 0.6 * len(p)
  assert per_source.max() <= 8
  differ = int((_fused_diagonal(p, T, q, r) != diag).sum())
  print("the fused order decides %d of %d (i, i) pairs differently" % (differ, len(p)))
  assert differ >= 100
