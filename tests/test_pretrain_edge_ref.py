"""tests/pretrain_edge_ref.py against the oracle wherever the two overlap (CPU only): the references that
tests/test_gpu_pretrain_edges.py holds the kernels to must themselves agree with the restatements the rest of the suite
trusts -- a wrong reference could otherwise hide a wrong kernel."""
import numpy as np
import pytest
import torch

import pretrain_edge_ref as er


def test_edge_cloud_levels_reach_minus_2_17_and_every_row_has_its_centre():
  from oracle import sparse_ref as sr
  coords = er.edge_cloud()
  assert set(coords[:, 0].tolist()) == {0, 1022} and coords[:, 1:].min() == -er.E and coords[:, 1:].max() == er.E
  for p in ((-er.E, -er.E, -er.E), (-er.E + 1, -er.E, -er.E), (-er.E + 2, -er.E, -er.E), (-er.E + 16, -er.E, -er.E), (er.E, er.E, er.E)):
    assert (coords[:, 1:] == np.asarray(p)).all(1).sum() == 2
  ref = sr.CoordsManagerRef(coords)
  key = 0
  for lvl in range(4):
    if lvl:
      assert ref.coords[key][:, 1:].min() == -(1 << 17), "level %d" % lvl
    for region in (0, 3):
      off = sr.region_offsets(3, region)
      assert (off[er.centre_slice(region)] == 0).all() and (off != 0).any(1).sum() == 26
      nbr = ref.kernel_map(key, key, 3, region).nbr
      assert (nbr[er.centre_slice(region)] == np.arange(ref.size(key))).all(), "level %d region %d" % (lvl, region)
    key = ref.stride(key, 2)


def test_segments_ref_is_the_stable_grouping():
  rng = np.random.RandomState(0)
  batch = rng.permutation(np.repeat([0, 511, 1022], [257, 1, 255]))
  seg = er.segments_ref(batch)
  want = [r for b in (0, 511, 1022) for r in range(len(batch)) if batch[r] == b]
  assert seg["rows"].tolist() == want and seg["offs"].tolist() == [0, 257, 258, 513] and seg["n_inst"] == 3
  assert seg["batches"].tolist() == [0, 511, 1022]
  assert (np.asarray([0, 511, 1022])[seg["inst"]] == batch).all()


def test_pdist_ref_is_torch_min_in_float64():
  from oracle import loss_ref  # noqa: F401  (the oracle's pdist is the same expression: sqrt(sum((a - b)^2) + 1e-7))
  torch.manual_seed(0)
  a, b = torch.randn(40, 16, dtype=torch.float64), torch.randn(70, 16, dtype=torch.float64)
  b[30] = b[3]
  a[5] = b[3]
  a[2, 0] = float("nan")
  a[6, 2] = float("inf")            # no b holds an inf in column 2: every distance of the row is +inf
  a[7, 1], b[9, 1] = float("inf"), float("inf")  # inf - inf: the row's only NaN is at column 9
  for extra_nan in (False, True):
    if extra_nan:
      b[60, 3] = float("nan")
    D, dmin, amin = er.pdist_ref(a.numpy(), b.numpy())
    Dt = torch.sqrt((a.unsqueeze(1) - b.unsqueeze(0)).pow(2).sum(2) + 1e-7)
    tmin, tind = Dt.min(1)
    # (numpy and torch add the 16 squares in different orders: the last bit may differ, nothing else)
    assert np.allclose(D, Dt.numpy(), rtol=1e-14, atol=0, equal_nan=True)
    assert np.allclose(dmin, tmin.numpy(), rtol=1e-14, atol=0, equal_nan=True) and (amin == tind.numpy()).all()
    assert amin[2] == 0 and np.isnan(dmin[2]) and amin[7] == 9 and np.isnan(dmin[7])
    if extra_nan:  # every row now has a NaN distance, at column 60 unless an earlier one exists
      assert np.isnan(dmin).all() and (np.delete(amin, [2, 7]) == 60).all()
    else:
      assert amin[5] == 3 and amin[6] == 0 and np.isinf(dmin[6]) and np.isnan(dmin).sum() == 2


@pytest.mark.parametrize("empty", [(), (0,), (0, 1)])
def test_hardest_ref_matches_the_oracle_loss(empty):
  from oracle import loss_ref as lr
  torch.manual_seed(1)
  rng = np.random.RandomState(1)
  N, P, S = 300, 120, 40
  F0 = torch.nn.functional.normalize(torch.randn(N, 16, dtype=torch.float64), dim=1)
  F1 = torch.nn.functional.normalize(F0 + 0.3 * torch.randn(N, 16, dtype=torch.float64), dim=1)
  i = np.sort(rng.choice(N, P, replace=False))
  pp = np.stack([i, np.clip(i + rng.randint(-1, 2, P), 0, N - 1)], 1)
  sel0, sel1 = rng.choice(N, S, replace=False), rng.choice(N, S, replace=False)
  F0r, F1r = F0.clone().requires_grad_(True), F1.clone().requires_grad_(True)
  pos, neg, aux = lr.hardest_contrastive_loss(F0r, F1r, pp, sel0, sel1, None)
  (pos + neg).backward()
  m0, m1 = aux["mask0"].copy(), aux["mask1"].copy()
  assert m0.any() and m1.any() and not m0.all()
  p0, p1 = torch.from_numpy(pp[:, 0]), torch.from_numpy(pp[:, 1])
  s0, s1 = torch.from_numpy(sel0), torch.from_numpy(sel1)
  if 0 in empty:
    m0[:] = False
  if 1 in empty:
    m1[:] = False
  rpos, rneg, D01, D10, g = er.hardest_ref(F0[p0], F1[p1], F0[s0], F1[s1], aux["D01ind"], m0, aux["D10ind"], m1, 0.1, 1.4)
  assert abs(float(rpos) - float(pos.detach())) <= 1e-12
  g0 = torch.zeros_like(F0).index_add_(0, p0, g[0]).index_add_(0, s0, g[2])
  g1 = torch.zeros_like(F1).index_add_(0, p1, g[1]).index_add_(0, s1, g[3])
  if not empty:
    assert abs(float(rneg) - float(neg.detach())) <= 1e-12
    assert float((g0 - F0r.grad).abs().max()) <= 1e-12 and float((g1 - F1r.grad).abs().max()) <= 1e-12
    return
  # an empty side: torch's mean over nothing is NaN, and nothing flows back through it
  assert np.isnan(float(rneg))
  if 0 in empty:
    assert float(g[3].abs().max()) == 0.0  # subF1 is reached only through side 0
  if 1 in empty:
    assert float(g[2].abs().max()) == 0.0
  if empty == (0, 1):
    only_pos = torch.autograd.grad(torch.relu((F0r[p0] - F1r[p1]).pow(2).sum(1) - 0.1).mean(), [F0r, F1r])
    assert float((g0 - only_pos[0]).abs().max()) <= 1e-12 and float((g1 - only_pos[1]).abs().max()) <= 1e-12


def test_keyset_ref_is_the_oracle_hash_and_isin():
  from oracle import loss_ref as lr
  rng = np.random.RandomState(2)
  pairs = np.stack([rng.randint(0, 50, 300), rng.randint(0, 70, 300)], 1)
  a, b = rng.randint(0, 50, 500), rng.randint(0, 70, 500)
  want = ~np.isin(lr.hash_pairs(a, b, 70), lr.hash_pairs(pairs[:, 0], pairs[:, 1], 70))
  got = er.keyset_absent_ref(pairs, 70, a, b)
  assert (got == want).all() and got.any() and not got.all()
  big = 2 ** 31 - 1
  assert not er.keyset_absent_ref([[big, big]], big, [big], [big])[0] and er.keyset_absent_ref([[big, big]], big, [big - 1], [big])[0]
  assert not er.keyset_absent_ref([[10, 0]], 10, [0], [1])[0]  # two pairs, one key: the reference's own behaviour
  assert er.keyset_absent_ref(np.zeros((0, 2)), 7, [1, 2], [3, 4]).all()


@pytest.mark.parametrize("lengths", [[1] * 500, [777], [8, 8, 16, 2016, 2048, 1, 7, 2040, 3], None])
def test_pair_select_ref_matches_the_oracle(lengths):
  from oracle import loss_ref as lr
  rng = np.random.RandomState(3)
  if lengths is None:
    lengths = rng.randint(1, 30, 2000)
  q = er.runs_of(lengths)
  pp = np.stack([q, rng.randint(0, 10 ** 6, len(q)).astype(np.int32)], 1)
  for u in (torch.rand(len(lengths), generator=torch.Generator().manual_seed(4)), torch.zeros(len(lengths)),
            torch.full((len(lengths),), float(np.nextafter(np.float32(1), np.float32(0))))):
    for sampled in (None, rng.choice(len(lengths), min(len(lengths), 64), replace=False)):
      qr, kr = lr.nce_select_pairs(pp, u, sampled)
      qg, kg, start, count = er.pair_select_ref(pp, u.numpy(), sampled)
      assert (qg == qr.numpy()).all() and (kg == kr.numpy()).all()
      assert (count >= 1).all() and (pp[start, 0] == qg).all()
  qg, kg, _, _ = er.pair_select_ref(pp, np.zeros(len(lengths), np.float32), np.array([0, -1, len(lengths)]))
  assert qg[0] == pp[0, 0] and kg[0] == pp[0, 1] and qg[1:].tolist() == [0, 0] and kg[1:].tolist() == [0, 0]


def test_match_bruteforce_equals_the_oracle_on_the_lattices():
  from oracle import loader_ref as lf
  for name, src, dst, r in er.match_cases():
    assert len(np.unique(src, axis=0)) == len(src) == 500 and len(np.unique(dst, axis=0)) == len(dst) == 500
    for T in (np.eye(4), er.ROT_Z90):
      want, n_exact = er.match_bruteforce(src, T, dst, r)
      got = lf.match_radius(src, T, dst, r)
      assert got.shape == want.shape and (got == want).all(), name
      assert len(want) > 300, name
      if name == "exact":  # pairs exactly ON the radius, points exactly ON cell faces
        assert n_exact > 50 and (np.floor(dst / r) == dst / r).any()
      assert (lf.apply_rigid(T, src) == er.apply_rigid_ref(T, src)).all()
  assert (er.apply_rigid_ref(er.ROT_Z90, src)[:, 0] == -src[:, 1]).all()  # the rotation is exact


def test_voxelize_ref_equals_the_oracle():
  from oracle import loader_ref as lf
  rng = np.random.RandomState(6)
  for n in (1, 512, 513):
    x = rng.uniform(-0.3, 0.3, (n, 3))
    first, coords = er.voxelize_ref(x, 0.025)
    assert (first == lf.sparse_quantize_index(x, 0.025)).all() and (coords == np.floor(x[first] / 0.025)).all()
  faces = np.array([[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [0.25, -0.25, 0.5], [np.nextafter(0.25, 0), -0.25, 0.5], [0.25, np.nextafter(-0.25, -1), 0.5]])
  first, coords = er.voxelize_ref(faces, 0.25)
  assert first.tolist() == lf.sparse_quantize_index(faces, 0.25).tolist() == [0, 2, 3, 4]
  assert coords.tolist() == [[0, 0, 0], [1, -1, 2], [0, -1, 2], [1, -2, 2]]


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_points_are_refused_by_reference_and_oracle(bad):
  from oracle import loader_ref as lf
  x = np.array([[0.1, 0.2, 0.3], [0.4, bad, 0.6]])
  ok = np.array([[0.1, 0.2, 0.3]])
  for f in (lambda: er.voxelize_ref(x, 0.025), lambda: lf.sparse_quantize_index(x, 0.025),
            lambda: er.match_bruteforce(x, np.eye(4), ok, 0.1), lambda: lf.match_radius(x, np.eye(4), ok, 0.1),
            lambda: er.match_bruteforce(ok, np.eye(4), x, 0.1), lambda: lf.match_radius(ok, np.eye(4), x, 0.1)):
    with pytest.raises(ValueError, match="non-finite"):
      f()
  big = np.array([[1e308, 0.0, 0.0]])  # finite, but not after the transform
  T = np.diag([10.0, 1.0, 1.0, 1.0])
  with np.errstate(over="ignore"):
    for f in (lambda: er.match_bruteforce(big, T, ok, 0.1), lambda: lf.match_radius(big, T, ok, 0.1)):
      with pytest.raises(ValueError, match="non-finite"):
        f()
