"""The pre-training path's data-dependent kernels at the edges of the packed key, at every dispatch branch and on the
inputs a diverging run produces (pytest -m gpu, on a real MI355X): coordinate manager (csrc/coords.hip), hard-negative
mining, key set and hardest-contrastive loss (csrc/loss.hip), positive-pair selection (csrc/pairs.hip), loader geometry
(csrc/loader.hip).  References: the oracle and tests/pretrain_edge_ref.py (plain numpy / float64 torch, checked against
the oracle on the CPU by tests/test_pretrain_edge_ref.py).

Tolerances are the project's: integer work bit-exact; dmin 1e-5 relative (test_pdist_argmin_and_keyset; here per row);
losses and gradients 1e-4 (the north-star tolerance); two runs bit-equal wherever the code promises reproducibility.
The non-finite cases only read outputs back and check them on the host: nothing here gathers with a mined index.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import pretrain_edge_ref as er
from test_gpu_parity import _check_maps, _device_tensor, assert_close, assert_rows_close, assert_slices_close

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
E = er.E


@pytest.fixture(scope="module")
def ME():
  import pointcontrast_amd.minkowski as me
  return me


def _dev(x, dtype=None):
  t = torch.as_tensor(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x)
  return (t if dtype is None else t.to(dtype)).contiguous().to(DEV)


# ------------------------------------------------------------------------------------------------
# A. coordinate manager
# ------------------------------------------------------------------------------------------------
def test_coords_range_edge_levels_and_maps(ME):
  """Rows at +-(2^17 - 1): every strided level of the negative corner holds -2^17 (key field 0).  Coordinates, 3^3 maps of
  both regions, stride-2 child tables and pair lists of 4 levels bit-equal to the oracle -- and, independently of the
  oracle, every row of every level is its own centre neighbour."""
  coords = er.edge_cloud()
  cm = _check_maps(ME, coords, levels=4)
  key = cm.key(0)
  for lvl in range(4):
    c = cm.get_coords(key).cpu().numpy()
    if lvl:
      assert c[:, 1:].min() == -(1 << 17) and key.tensor_stride == 1 << lvl
    for region in (0, 3):
      nbr, _, _ = cm.export_map(cm.kernel_map(key, key, 3, 1, region))
      centre = nbr.cpu().numpy()[er.centre_slice(region)]
      assert (centre == np.arange(len(c))).all(), "level %d region %d: rows %s have no centre tap" % (
          lvl, region, c[centre != np.arange(len(c))].tolist())
    key = cm.stride(key, 2)


BAD_ROWS = {"x = -2^17": (0, -(1 << 17), 0, 0), "z = -2^17": (0, 3, 4, -(1 << 17)), "y = 2^17": (0, 0, 1 << 17, 0),
            "batch 1023": (1023, 1, 2, 3), "batch -1": (-1, 1, 2, 3)}


@pytest.mark.parametrize("what", sorted(BAD_ROWS))
def test_coords_out_of_range_rows_are_refused(ME, what):
  """One row outside the packable range among valid ones: PCMI_ERR_RANGE from the synchronous insert and, for a deferred
  insert, from check(); the handle holds nothing afterwards."""
  from pointcontrast_amd._lib import PcmiError
  coords = np.concatenate([er.edge_cloud()[:20], np.asarray([BAD_ROWS[what]], np.int32), er.edge_cloud()[20:30]])
  feats = np.zeros((len(coords), 4), np.float32)
  with pytest.raises(PcmiError, match="error -5.*range"):
    _device_tensor(ME, coords, feats)
  st = ME.SparseTensor(torch.as_tensor(feats), coords=torch.as_tensor(coords)).to(DEV, defer_check=True)
  with pytest.raises(PcmiError, match="error -5.*range"):
    st.coords_man.check()
  with pytest.raises(PcmiError):
    st.coords_man.size(st.coords_man.key(0))
  _device_tensor(ME, np.delete(coords, 20, 0), np.delete(feats, 20, 0))  # the same rows without the bad one are accepted


def test_conv_on_the_edge_cloud_at_the_first_strided_level(ME):
  """3^3 HYBRID 32 -> 32 on level 1 of the edge cloud (rows at -2^17): a lost centre tap is a numerical failure of the
  output, the data gradient and the weight gradient, not only a map mismatch."""
  from oracle import model_ref as mr, sparse_ref as sr
  from pointcontrast_amd.model.modules.common import ConvType, conv
  coords = er.edge_cloud()
  g = torch.Generator().manual_seed(0)
  ref_cm = sr.CoordsManagerRef(coords)
  st0 = _device_tensor(ME, coords, np.zeros((len(coords), 4), np.float32))
  cm = st0.coords_man
  in_key, rin = cm.stride(st0.coords_key, 2), ref_cm.stride(0, 2)
  assert ref_cm.coords[rin][:, 1:].min() == -(1 << 17)
  mod = conv(32, 32, 3, conv_type=ConvType.SPATIAL_HYPERCUBE_TEMPORAL_HYPERCROSS, bias=False, D=3)
  rmod = mr.ConvRef(32, 32, 3, region=sr.HYBRID, bias=False)
  mod.load_state_dict(rmod.state_dict())
  mod = mod.to(DEV)
  x = torch.randn(ref_cm.size(rin), 32, generator=g)
  xr, xd = x.clone().requires_grad_(True), x.to(DEV).requires_grad_(True)
  yr = rmod(sr.SparseTensorRef(xr, coords_key=rin, coords_manager=ref_cm)).F
  yd = mod(ME.SparseTensor(xd, coords_key=in_key, coords_manager=cm)).F
  gy = torch.randn(yr.shape, generator=g)
  yr.backward(gy)
  yd.backward(gy.to(DEV))
  assert_rows_close(yd, yr, 1e-4, "edge conv out")
  assert_rows_close(xd.grad, xr.grad, 1e-4, "edge conv gin")
  assert_slices_close(mod.kernel.grad, rmod.kernel.grad, 1e-4, "edge conv gw")


def _read_i32(dev_ptr, n):
  """n int32 from a raw device pointer of the library's arena (the tables of pcmi_segments_t)."""
  from pointcontrast_amd._lib import lib
  out = np.empty(n, np.int32)
  if n:
    cp = lib.hipMemcpy  # (libpcmi's own HIP runtime: the one torch loaded)
    cp.restype, cp.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert cp(out.ctypes.data, dev_ptr, 4 * n, 2) == 0  # hipMemcpyDeviceToHost
  return out


@pytest.mark.parametrize("counts", [(1, 255, 256), (257, 1, 255), (256, 257, 1), (255, 256, 257)])
def test_segments_and_origin_with_sparse_batch_indices(ME, counts):
  """pcmi_coords_segments / pcmi_coords_origin with the non-contiguous batch indices {0, 511, 1022} and instance sizes
  around the 256-row block of the histogram / scatter kernels, rows interleaved: the stable grouping of numpy."""
  rng = np.random.RandomState(sum(counts))
  batch = rng.permutation(np.repeat([0, 511, 1022], counts)).astype(np.int32)
  n = len(batch)
  coords = np.stack([batch, np.arange(n, dtype=np.int32) - 300, rng.randint(-5, 5, n).astype(np.int32), np.zeros(n, np.int32)], 1)
  st = _device_tensor(ME, coords, np.zeros((n, 4), np.float32))
  cm = st.coords_man
  seg = cm.segments(st.coords_key)
  want = er.segments_ref(batch)
  assert int(seg.n) == n and int(seg.n_inst) == want["n_inst"] == 3
  assert (_read_i32(seg.rows, n) == want["rows"]).all()
  assert (_read_i32(seg.offs, 4) == want["offs"]).all()
  assert (_read_i32(seg.inst, n) == want["inst"]).all()
  okey = cm.origin_key()
  origin = cm.get_coords(okey).cpu().numpy()
  assert okey.tensor_stride == 0 and origin.tolist() == [[0, 0, 0, 0], [511, 0, 0, 0], [1022, 0, 0, 0]]


def test_segments_with_every_batch_index_in_use(ME):
  """pcmi_coords_segments with all 1023 admissible batch indices present (1 to 3 rows each, interleaved; bin 1023 is the
  one the insert refuses): every wave of the one-workgroup scan over the 1024 bins carries a count into the next."""
  rng = np.random.RandomState(7)
  batch = rng.permutation(np.repeat(np.arange(1023), rng.randint(1, 4, 1023))).astype(np.int32)
  n = len(batch)
  coords = np.stack([batch, np.arange(n, dtype=np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)], 1)
  st = _device_tensor(ME, coords, np.zeros((n, 4), np.float32))
  seg = st.coords_man.segments(st.coords_key)
  want = er.segments_ref(batch)
  assert int(seg.n) == n and int(seg.n_inst) == want["n_inst"] == 1023
  assert (_read_i32(seg.rows, n) == want["rows"]).all()
  assert (_read_i32(seg.offs, 1024) == want["offs"]).all()
  assert (_read_i32(seg.inst, n) == want["inst"]).all()


# ------------------------------------------------------------------------------------------------
# B. pdist_argmin: every instantiation, tile boundaries, exact ties, non-finite rows
# ------------------------------------------------------------------------------------------------
def _pdist_branch(c, p, s):
  """pcmi_pdist_argmin's dispatch rule (csrc/loss.hip) restated: the <C, TR, TS> instantiation a shape reaches."""
  from pointcontrast_amd._lib import lib
  ncu = C.c_int()
  assert lib.pcmi_device_info(C.byref(ncu), None, 0) == 0
  narrow = c <= 32 and (p + 63) // 64 < 2 * ncu.value and s > 64
  return (c, 16, 256) if narrow else (c, 64, 64)


# Which case reaches which instantiation of pdist_argmin_kernel<C, TR, TS> (asserted through _pdist_branch):
#   <16, 16, 256> : c = 16, s in {65, 255, 256, 257}  (narrow: s > 64 and fewer than 2 * num_cu 64-row tiles)
#   <32, 16, 256> : c = 32, s in {65, 255, 256, 257}  (narrow)
#   <16, 64, 64>  : c = 16, s in {1, 63, 64}          (wide: the candidates fit one 64-column tile)
#   <32, 64, 64>  : c = 32, s in {1, 63, 64}          (wide)
#   <64, 64, 64>  : c = 64, (p, s) in {(1, 1), (65, 63), (130, 257)}  (always wide)
PDIST_CASES = ([(c, p, s, (c, 16, 256)) for c in (16, 32) for s in (65, 255, 256, 257) for p in (1, 15, 16, 17, 257)] +
               [(c, p, s, (c, 64, 64)) for c in (16, 32) for s in (1, 63, 64) for p in (1, 63, 64, 65)] +
               [(64, p, s, (64, 64, 64)) for p, s in ((1, 1), (65, 63), (130, 257))])


def _pdist_device(a, b):
  from pointcontrast_amd import functional as PF
  dmin, amin = PF.pdist_argmin(_dev(a, torch.float32), _dev(b, torch.float32))
  return dmin.cpu().numpy().astype(np.float64), amin.cpu().numpy().astype(np.int64)


def _assert_mined(a, b, dmin, amin, what, exact_rows=()):
  """dmin within 1e-5 of float64 per row; amin = the float64 first arg-min, except at a float32 tie (the mined row's
  float64 distance exceeds the minimum by < 1e-6) -- at most 1 row in 100, and never for `exact_rows`."""
  D, rmin, rind = er.pdist_ref(a, b)
  assert ((amin >= 0) & (amin < len(b))).all(), "%s: arg-min outside [0, %d): %s" % (what, len(b), amin[(amin < 0) | (amin >= len(b))][:8])
  err = np.abs(dmin - rmin) / rmin
  print("%s: dmin worst rel err %.3e, %d of %d arg-mins differ" % (what, err.max(), int((amin != rind).sum()), len(a)))
  assert err.max() <= 1e-5, "%s: dmin rel err %.3e" % (what, err.max())
  diff = np.flatnonzero(amin != rind)
  excess = D[diff, amin[diff]] - rmin[diff]
  assert (excess < 1e-6).all(), "%s: rows %s mined a row that is not a minimum (excess %s)" % (what, diff[excess >= 1e-6][:8], excess[excess >= 1e-6][:8])
  assert len(diff) * 100 <= len(a), "%s: %d of %d rows excused as ties" % (what, len(diff), len(a))
  for r in exact_rows:
    assert amin[r] == rind[r], "%s: row %d mined %d, the first arg-min is %d" % (what, r, amin[r], rind[r])


@pytest.mark.parametrize("c,p,s,branch", PDIST_CASES)
def test_pdist_argmin_every_instantiation_at_tile_edges(c, p, s, branch):
  assert _pdist_branch(c, p, s) == branch
  torch.manual_seed(1000 * c + 7 * p + s)
  a = torch.nn.functional.normalize(torch.randn(p, c), dim=1).numpy()
  b = torch.nn.functional.normalize(torch.randn(s, c), dim=1).numpy()
  dmin, amin = _pdist_device(a, b)
  _assert_mined(a, b, dmin, amin, "pdist <%d,%d,%d> p=%d s=%d" % (branch + (p, s)))


# duplicate groups of b: copies in different 4-column lane groups, in different TS tiles, and inside one lane group
TIE_CASES = [(16, 333, ((3, 70, 300), (129, 257, 258)), (16, 16, 256)), (32, 333, ((3, 70, 300), (129, 257, 258)), (32, 16, 256)),
             (64, 333, ((3, 70, 300), (129, 257, 258)), (64, 64, 64)),
             (16, 64, ((3, 38, 63), (16, 17, 18)), (16, 64, 64)), (32, 64, ((3, 38, 63), (16, 17, 18)), (32, 64, 64))]


@pytest.mark.parametrize("c,s,groups,branch", TIE_CASES)
def test_pdist_argmin_exact_ties_go_to_the_lowest_index(c, s, groups, branch):
  """b holds exact duplicates and some rows of a equal them: identical inputs give bitwise identical sums, so the tie is
  exact and amin must be the LOWEST index (include/pcmi.h: first arg min) -- no excuse."""
  p = 40
  assert _pdist_branch(c, p, s) == branch
  torch.manual_seed(c + s)
  a = torch.nn.functional.normalize(torch.randn(p, c), dim=1).numpy()
  b = torch.nn.functional.normalize(torch.randn(s, c), dim=1).numpy()
  rows = {}
  for gi, grp in enumerate(groups):
    for j in grp[1:]:
      b[j] = b[grp[0]]
    for r in (5 + gi, 17 + gi, 38 + gi):  # (rows of different 16-row tiles)
      a[r] = b[grp[0]]
      rows[r] = grp[0]
  dmin, amin = _pdist_device(a, b)
  _assert_mined(a, b, dmin, amin, "pdist ties c=%d s=%d" % (c, s), exact_rows=rows)
  for r, first in rows.items():
    assert amin[r] == first


@pytest.mark.parametrize("c,p,s,branch", [(32, 40, 300, (32, 16, 256)), (16, 40, 300, (16, 16, 256)), (16, 70, 64, (16, 64, 64)),
                                          (32, 70, 64, (32, 64, 64)), (64, 70, 130, (64, 64, 64))])
@pytest.mark.parametrize("nan_in_b", [False, True])
def test_pdist_argmin_non_finite_rows_follow_torch_min(c, p, s, branch, nan_in_b):
  """A NaN row of a, +inf elements in a and b, optionally a NaN row of b.  amin is read back and must be a row of b for
  EVERY row (before anything could use it as an index); then torch.min's semantics: a row with a NaN distance has
  dmin = NaN and amin = its first NaN position, a row of +inf distances mines row 0."""
  assert _pdist_branch(c, p, s) == branch
  torch.manual_seed(c * p + s)
  a = torch.nn.functional.normalize(torch.randn(p, c), dim=1).numpy()
  b = torch.nn.functional.normalize(torch.randn(s, c), dim=1).numpy()
  a[2, 0] = np.nan                   # every distance of row 2 is NaN: first NaN position 0
  a[6, 2] = np.inf                   # no b has an inf in column 2: every distance is +inf, the first is 0
  a[21, 1], b[s - 20, 1] = np.inf, np.inf  # inf - inf: row 21's only NaN
  b[9, 0] = np.inf                   # a candidate at +inf from everybody
  if nan_in_b:
    b[s - 3, 3] = np.nan             # a NaN candidate: every row's distance to it is NaN
  dmin, amin = _pdist_device(a, b)
  assert ((amin >= 0) & (amin < s)).all(), "arg-min outside [0, %d) at rows %s: %s" % (
      s, np.flatnonzero((amin < 0) | (amin >= s))[:8], amin[(amin < 0) | (amin >= s)][:8])
  D, rmin, rind = er.pdist_ref(a, b)
  assert np.isnan(rmin[2]) and rind[2] == 0 and np.isnan(rmin[21]) and rind[21] == s - 20
  assert rind[6] == (s - 3 if nan_in_b else 0) and (nan_in_b or np.isinf(rmin[6]))
  special = ~np.isfinite(rmin)
  assert special.sum() == (p if nan_in_b else 3)
  assert (np.isnan(dmin) == np.isnan(rmin)).all(), "dmin is NaN at rows %s, the reference at %s" % (
      np.flatnonzero(np.isnan(dmin))[:8], np.flatnonzero(np.isnan(rmin))[:8])
  assert (np.isinf(dmin) == np.isinf(rmin)).all()
  assert (amin[special] == rind[special]).all(), "rows %s: mined %s, torch.min gives %s" % (
      np.flatnonzero(special)[:8], amin[special][:8], rind[special][:8])
  if not nan_in_b:
    fin = np.flatnonzero(~special)
    _assert_mined(a[fin], b, dmin[fin], amin[fin], "pdist finite rows beside non-finite ones")


# ------------------------------------------------------------------------------------------------
# C. hardest-contrastive loss, forward and backward
# ------------------------------------------------------------------------------------------------
PT, NT = 0.1, 1.4


def _hardest_device(posF0, posF1, subF0, subF1, d01, i01, m0, d10, i10, m1, pt=PT, nt=NT):
  from pointcontrast_amd import functional as PF
  ts = [_dev(t, torch.float32).requires_grad_(True) for t in (posF0, posF1, subF0, subF1)]
  losses = PF.HardestLossFunction.apply(ts[0], ts[1], ts[2], ts[3], _dev(d01, torch.float32), _dev(i01, torch.int32),
                                        _dev(m0, torch.uint8), _dev(d10, torch.float32), _dev(i10, torch.int32),
                                        _dev(m1, torch.uint8), pt, nt)
  (losses[0] + losses[1]).backward()
  return losses.detach().cpu().numpy().astype(np.float64), [t.grad.cpu() for t in ts]


def _hardest_case(p, s, c, seed, i01=None, i10=None):
  """Unit positives near their partners, s candidates per side; every positive mines i01 / i10 (default: i % s)."""
  g = torch.Generator().manual_seed(seed)
  norm = torch.nn.functional.normalize
  posF0 = norm(torch.randn(p, c, generator=g), dim=1)
  posF1 = norm(posF0 + 0.5 * torch.randn(p, c, generator=g), dim=1)
  # candidates of norm 1/2: distances to the unit positives lie in [0.5, 1.5], nearly all below NT = 1.4 (active)
  subF0, subF1 = 0.5 * norm(torch.randn(s, c, generator=g), dim=1), 0.5 * norm(torch.randn(s, c, generator=g), dim=1)
  i01 = np.arange(p) % s if i01 is None else i01
  i10 = np.arange(p) % s if i10 is None else i10
  return [t.numpy().copy() for t in (posF0, posF1, subF0, subF1)], np.asarray(i01), np.asarray(i10)


def _hardest_compare(F, i01, m0, i10, m1, what, pt=PT, nt=NT, runs=1):
  """Device losses and the four gradients against the float64 restatement, at 1e-4; the device takes the float32 rounding
  of the reference's own mined distances (what pdist_argmin would hand it).  Returns (device losses, device gradients,
  reference (pos, neg, D01, D10, gradients))."""
  ref = er.hardest_ref(F[0], F[1], F[2], F[3], i01, m0, i10, m1, pt, nt)
  rpos, rneg, D01, D10, rg = ref
  first = None
  for _ in range(runs):
    losses, grads = _hardest_device(F[0], F[1], F[2], F[3], D01.numpy(), i01, m0, D10.numpy(), i10, m1, pt, nt)
    if first is None:
      first = (losses, grads)
    else:
      assert np.array_equal(first[0], losses, equal_nan=True), "%s: the losses are not reproducible" % what
      for x, y, nm in zip(first[1], grads, ("dposF0", "dposF1", "dsubF0", "dsubF1")):
        assert torch.equal(x, y), "%s: %s differs between two runs" % (what, nm)
  print("%s: pos %.9g (ref %.9g) neg %.9g (ref %.9g)" % (what, losses[0], float(rpos), losses[1], float(rneg)))
  for got, want, nm in ((losses[0], float(rpos), "pos"), (losses[1], float(rneg), "neg")):
    assert np.isnan(got) == np.isnan(want), "%s: %s loss %r, the reference %r" % (what, nm, got, want)
    if not np.isnan(want):
      assert abs(got - want) <= 1e-4 * abs(want) + 1e-9, "%s: %s loss %r vs %r" % (what, nm, got, want)
  for got, want, nm in zip(grads, rg, ("dposF0", "dposF1", "dsubF0", "dsubF1")):
    if float(want.abs().max()) == 0.0:
      assert float(got.abs().max()) == 0.0, "%s: %s must be zero, max |g| = %.3e" % (what, nm, float(got.abs().max()))
    else:
      assert_close(got, want, 1e-4, "%s %s" % (what, nm))
  return losses, grads, ref


@pytest.mark.parametrize("p,c", [(255, 32), (256, 32), (257, 32), (1025, 32), (1025, 96)])
def test_hardest_everyone_mines_one_row(p, c):
  """s = 1: every positive mines row 0 -- one group across the 256-candidate steps of hardest_gsub_kernel's ownership
  scan and much longer than one step.  dsub within 1e-4 of float64; two runs bit-equal (no float atomics)."""
  F, i01, i10 = _hardest_case(p, 1, c, seed=p + c)
  m = np.ones(p, np.uint8)
  _, grads, ref = _hardest_compare(F, i01, m, i10, m, "everyone mines row 0, p=%d c=%d" % (p, c), runs=2)
  assert float((NT - ref[2]).min()) > 0 and float(grads[3].abs().max()) > 0  # every positive is active


@pytest.mark.parametrize("p,c", [(301, 16), (302, 64), (303, 96), (1027, 32)])
def test_hardest_popular_rows_with_inactive_first_miners(p, c):
  """s = 3, mined rows cycling 0, 1, 2; about a third of the positives inactive (mask 0, or the mined distance above the
  threshold), among them the FIRST miner of every row: the owner of a row's gradient is its first ACTIVE miner.  p is
  not a multiple of the 4 waves of a workgroup; c = 96 runs the channel loop twice."""
  F, i01, i10 = _hardest_case(p, 3, c, seed=p)
  rng = np.random.RandomState(p)
  m0, m1 = (rng.rand(p) > 0.15).astype(np.uint8), (rng.rand(p) > 0.15).astype(np.uint8)
  far = np.flatnonzero(rng.rand(p) < 0.15).tolist() + [1, 4]
  for i in far:  # opposite its mined row: distance 1.5 > NT
    F[0][i] = -2.0 * F[3][i01[i]]
    F[1][i] = -2.0 * F[2][i10[i]]
  m0[[0, 2, 3]] = 0  # first miners of rows 0 and 2 (and the second of row 0) masked; of row 1 (positives 1, 4) too far
  m1[[0, 2, 3]] = 0
  _, grads, ref = _hardest_compare(F, i01, m0, i10, m1, "popular rows p=%d c=%d" % (p, c), runs=2)
  active0 = (m0 != 0) & ((NT - ref[2].numpy()) > 0)
  assert not active0[:5].any() and 0.15 < 1 - active0.mean() < 0.5 and all(active0[i01 == r].any() for r in range(3))


@pytest.mark.parametrize("empty", [(0,), (1,), (0, 1)])
def test_hardest_degenerate_masks(empty):
  """One side's mask all zero, then both: the mean over an empty set is NaN (0 / 0) in the reference and on the device;
  the other side's gradients still match and every gradient through the empty side is zero."""
  p, s, c = 130, 7, 32
  F, i01, i10 = _hardest_case(p, s, c, seed=11)
  m0, m1 = np.ones(p, np.uint8), np.ones(p, np.uint8)
  if 0 in empty:
    m0[:] = 0
  if 1 in empty:
    m1[:] = 0
  losses, grads, ref = _hardest_compare(F, i01, m0, i10, m1, "empty side(s) %s" % (empty,))
  assert np.isnan(losses[1]) and np.isnan(float(ref[1])) and not np.isnan(losses[0])
  if 0 in empty:
    assert float(grads[3].abs().max()) == 0.0  # dsubF1 is reached only through side 0
  if 1 in empty:
    assert float(grads[2].abs().max()) == 0.0
  if 0 not in empty:
    assert float(grads[3].abs().max()) > 0.0


def test_hardest_hinges_exactly_at_the_threshold():
  """Row 0 sits exactly ON both hinges: |a - b|^2 == pos_thresh (dyadic values, the sums are exact) and its mined
  distance == neg_thresh (the threshold IS the float32 distance).  The strict > of the kernels and relu's subgradient 0
  agree: the row contributes nothing -- its own gradients and the row it alone mines stay exactly zero."""
  p, s, c = 9, 4, 16
  F, i01, i10 = _hardest_case(p, s, c, seed=5)
  F[0][0] = 0.0
  F[1][0] = 0.0
  F[0][0, 0] = 0.5                      # |a - b|^2 = 0.25 exactly
  F[3][0] = 0.0
  F[3][0, 1] = 1.25                     # the row that positive 0 alone mines on side 0
  i01 = np.array([0] + [1 + i % 3 for i in range(p - 1)])
  i10 = np.array([1 + i % 3 for i in range(p)])
  m0, m1 = np.ones(p, np.uint8), np.ones(p, np.uint8)
  m1[0] = 0
  D01 = er.hardest_ref(F[0], F[1], F[2], F[3], i01, m0, i10, m1, 0.25, 1.0)[2]
  nt = float(np.float32(D01[0].item()))  # the threshold is exactly what the device is handed as row 0's mined distance
  assert 1.3 < nt < 1.4
  _, grads, ref = _hardest_compare(F, i01, m0, i10, m1, "hinges at the threshold", pt=0.25, nt=nt, runs=2)
  assert float(grads[0][0].abs().max()) == 0.0 and float(grads[1][0].abs().max()) == 0.0, "row 0 is on the hinge: no gradient"
  assert float(grads[3][0].abs().max()) == 0.0, "the row mined only by the on-hinge positive has no gradient"
  assert float(grads[3][1:].abs().max()) > 0.0 and float(grads[0][1:].abs().max()) > 0.0


def test_hardest_nan_feature_row_reaches_the_losses():
  """A NaN in one row of posF0 (valid, in-range mined indices): F.relu keeps the NaN, so pos -- and neg, whose side-0 term
  holds the row's NaN distance -- are NaN; the device must not report a finite loss for a diverged step."""
  p, s, c = 300, 5, 32
  F, i01, i10 = _hardest_case(p, s, c, seed=21)
  F[0][137, 3] = np.nan
  m = np.ones(p, np.uint8)
  ref = er.hardest_ref(F[0], F[1], F[2], F[3], i01, m, i10, m, PT, NT)
  assert np.isnan(float(ref[0])) and np.isnan(float(ref[1])) and int(np.isnan(ref[2].numpy()).sum()) == 1
  from pointcontrast_amd import functional as PF
  with torch.no_grad():
    losses = PF.HardestLossFunction.apply(*[_dev(t, torch.float32) for t in F], _dev(ref[2].numpy(), torch.float32),
                                          _dev(i01, torch.int32), _dev(m, torch.uint8), _dev(ref[3].numpy(), torch.float32),
                                          _dev(i10, torch.int32), _dev(m, torch.uint8), PT, NT).cpu().numpy()
  assert np.isnan(losses[0]), "pos loss %r: the NaN row was dropped by the hinge" % losses[0]
  assert np.isnan(losses[1]), "neg loss %r: the NaN mined distance was dropped by the hinge" % losses[1]


# ------------------------------------------------------------------------------------------------
# D. key set and positive-pair selection
# ------------------------------------------------------------------------------------------------
def _keyset_check(pairs, M, qa, qb):
  from pointcontrast_amd import functional as PF
  pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
  ks = PF.PairKeySet(_dev(pairs, torch.int32), M)
  got = ks.absent(_dev(np.asarray(qa, np.int64)), _dev(np.asarray(qb, np.int64))).cpu().numpy().astype(bool)
  want = er.keyset_absent_ref(pairs, M, qa, qb)
  assert (got == want).all(), "key set: %d of %d queries differ" % (int((got != want).sum()), len(want))
  return got


@pytest.mark.parametrize("n", [0, 1, 512, 513])
def test_keyset_sizes_around_the_table_doubling(n):
  """n = 0: a query on the empty set gives all absent; 512 -> 513 keys doubles the table (pcmi_keyset_bytes)."""
  from pointcontrast_amd._lib import lib
  assert lib.pcmi_keyset_bytes(512) == 1024 * 8 and lib.pcmi_keyset_bytes(513) == 2048 * 8
  rng = np.random.RandomState(n)
  M = 1000
  flat = rng.choice(M * M, n, replace=False)
  pairs = np.stack([flat % M, flat // M], 1)
  qa = np.concatenate([pairs[:, 0], rng.randint(0, M, 300)])
  qb = np.concatenate([pairs[:, 1], rng.randint(0, M, 300)])
  got = _keyset_check(pairs, M, qa, qb)
  assert not got[:n].any() and got[n:].sum() >= 295


def test_keyset_heavy_duplicates_wide_keys_and_colliding_pairs():
  rng = np.random.RandomState(1)
  seven = np.stack([rng.randint(0, 500, 7), rng.randint(0, 500, 7)], 1)
  pairs = seven[rng.randint(0, 7, 70000)]  # 10 000 copies of each of 7 pairs, interleaved
  got = _keyset_check(pairs, 500, np.concatenate([seven[:, 0], seven[:, 0] + 1]), np.concatenate([seven[:, 1], seven[:, 1]]))
  assert not got[:7].any()
  big = 2 ** 31 - 1
  for M in (1, big):  # the largest int32 indices: the key arithmetic is int64 and must not wrap
    pairs = np.array([[big, big], [big - 1, big], [0, big], [big, 0], [0, 0]])
    qa = np.array([big, big - 1, 0, big, 0, big - 2, 1, big, big - 1])
    qb = np.array([big, big, big, 0, 0, big, big, big - 1, big - 1])
    got = _keyset_check(pairs, M, qa, qb)
    assert not got[:5].any()
  # pairs that differ but share a + b * M are one member: the reference's own behaviour
  got = _keyset_check([[10, 0]], 10, [0, 10, 1, 0], [1, 0, 1, 0])
  assert got.tolist() == [False, False, True, True]


def _select_device(pp, uniform, sampled=None):
  from pointcontrast_amd import functional as PF
  q, k = PF.pair_select(_dev(pp, torch.int32), len(uniform), _dev(np.asarray(uniform, np.float32)),
                        None if sampled is None else _dev(np.asarray(sampled, np.int64)))
  return q.cpu().numpy(), k.cpu().numpy()


def _select_check(lengths, uniform=None, sampled=None, seed=0):
  """Device selection bit-equal to the oracle (and to the plain restatement); the pick stays inside its run."""
  from oracle import loss_ref as lr
  rng = np.random.RandomState(seed)
  lengths = np.asarray(lengths)
  P = int(lengths.sum())
  pp = np.stack([er.runs_of(lengths), np.arange(P, dtype=np.int32)], 1)  # column 1 = the pair's own index
  if uniform is None:
    uniform = rng.rand(len(lengths)).astype(np.float32)
  uniform = np.asarray(uniform, np.float32)
  q, k = _select_device(pp, uniform, sampled)
  qr, kr = lr.nce_select_pairs(pp, torch.from_numpy(uniform), sampled)
  assert (q == qr.numpy()).all() and (k == kr.numpy()).all(), "pair selection differs from the oracle (%d runs, %d pairs)" % (len(lengths), P)
  qe, ke, start, count = er.pair_select_ref(pp, uniform, sampled)
  assert (q == qe).all() and (k == ke).all()
  assert ((k >= start) & (k < start + count)).all(), "a pick left its run"
  return q, k


@pytest.mark.parametrize("P", [1, 2047, 2048, 2049])
def test_pair_select_one_single_run(P):
  for u in (0.0, 0.37, float(np.nextafter(np.float32(1), np.float32(0)))):
    q, k = _select_check([P], [u])
    assert k[0] == int(np.floor(np.float32(u) * np.float32(P)))


def test_pair_select_runs_of_length_one_and_boundaries_on_thread_and_workgroup_edges():
  """Run starts exactly at multiples of 8 (one thread's items) and of 2048 (one workgroup's), and one off either side."""
  rng = np.random.RandomState(2)
  _select_check([1] * 5000)
  _select_check([1] * 5000, sampled=rng.choice(5000, 777, replace=False))
  lengths = [8, 8, 16, 2016, 2048, 1, 7, 2040, 2047, 1, 2049, 2047, 8, 3]
  assert {8, 16, 32, 2048, 4096, 4104, 6144, 8191, 8192, 10241, 12288}.issubset(set(np.cumsum(lengths).tolist()))
  for u in (None, np.zeros(len(lengths)), np.full(len(lengths), np.nextafter(np.float32(1), np.float32(0)))):
    _select_check(lengths, u)


@pytest.mark.parametrize("P", [524288, 524289])
def test_pair_select_second_pass_of_the_one_workgroup_scan(P):
  """256 workgroups of 2048 pairs fill one pass of the scan over the block counts; pair 524289 opens a second."""
  rng = np.random.RandomState(P)
  lengths = rng.randint(1, 30, P // 10)
  lengths = lengths[np.cumsum(lengths) < P - 40]
  lengths = np.concatenate([lengths, [P - 1 - lengths.sum(), 1]])  # the last pair is a run of its own, in the last block
  assert lengths.sum() == P and lengths.min() >= 1
  _select_check(lengths, seed=1)
  _select_check(lengths, sampled=rng.choice(len(lengths), 4096, replace=False), seed=2)


@pytest.mark.parametrize("u", [0.0, float(np.nextafter(np.float32(1), np.float32(0)))])
def test_pair_select_uniform_at_both_ends_of_its_range(u):
  """floor(u * count) in float32 for counts 1, 3, 30 and 2^20 at u = 0 and the largest float32 below 1: the first and the
  LAST pair of the run, never the next run's first."""
  lengths = [1, 3, 30, 1 << 20, 1, 3, 30]
  q, k = _select_check(lengths, [u] * len(lengths))
  start = np.concatenate([[0], np.cumsum(lengths)[:-1]])
  assert (k == (start if u == 0.0 else start + np.asarray(lengths) - 1)).all()


def test_pair_select_empty_selection_and_sampled_out_of_range():
  lengths = [3, 1, 4, 1, 5]
  pp = np.stack([er.runs_of(lengths), np.arange(14, dtype=np.int32)], 1)
  u = np.full(5, 0.5, np.float32)
  q, k = _select_device(pp, u, np.zeros(0, np.int64))  # n_sel = 0
  assert q.shape == k.shape == (0,)
  sampled = np.array([4, -1, 0, 5, 2, 1 << 40])
  q, k = _select_device(pp, u, sampled)  # an index outside [0, n_unique) writes (0, 0), as csrc/pairs.hip documents
  qe, ke, _, _ = er.pair_select_ref(pp, u, sampled)
  assert (q == qe).all() and (k == ke).all() and q[[1, 3, 5]].tolist() == [0, 0, 0] and k[[1, 3, 5]].tolist() == [0, 0, 0]
  assert q[[0, 2, 4]].tolist() == [12, 0, 6] and k[[0, 2, 4]].tolist() == [11, 1, 6]


# ------------------------------------------------------------------------------------------------
# E. loader geometry
# ------------------------------------------------------------------------------------------------
_MATCH_REF = {}


def _match_ref(name, tname):
  """Brute force and oracle on one lattice case, computed once."""
  from oracle import loader_ref as lf
  if not _MATCH_REF:
    for nm, src, dst, r in er.match_cases():
      for tn, T in (("identity", np.eye(4)), ("rot_z90", er.ROT_Z90)):
        brute, n_exact = er.match_bruteforce(src, T, dst, r)
        _MATCH_REF[(nm, tn)] = (src, dst, r, T, brute, n_exact, lf.match_radius(src, T, dst, r))
  return _MATCH_REF[(name, tname)]


@pytest.mark.parametrize("tname", ["identity", "rot_z90"])
@pytest.mark.parametrize("name", ["exact", "ulp", "voxel"])
def test_match_radius_on_lattices_equals_brute_force_and_oracle(name, tname):
  """Points on a dyadic lattice with radius 2^-5: every product is exact, pairs lie exactly ON the radius and points on
  cell faces; the same moved by 1 ulp; a 0.025 lattice at r = 0.0375.  The device must equal the all-pairs brute force
  (which does not share the 27-cell idea) and the oracle, under the identity and an exact rotation by 90 degrees."""
  from pointcontrast_amd.lib import device_loader as dl
  src, dst, r, T, brute, n_exact, oracle = _match_ref(name, tname)
  got = dl.get_matching_indices(src, dst, T, r)
  print("match %s %s: %d pairs, %d exactly on the radius" % (name, tname, len(brute), n_exact))
  assert (oracle == brute).all() and len(brute) > 300 and (name != "exact" or n_exact > 50)
  assert got.shape == brute.shape and (got == brute).all()


def test_match_radius_cap_of_96_matches_per_source_point():
  from pointcontrast_amd._lib import PcmiError
  from pointcontrast_amd.lib import device_loader as dl
  src = np.array([[0.1, 0.2, 0.3]])
  got = dl.get_matching_indices(src, np.repeat(src, 96, 0), np.eye(4), 0.05)
  assert got.tolist() == [[0, j] for j in range(96)]  # all of them, ascending j
  with pytest.raises(PcmiError, match="error -5.*matches"):
    dl.get_matching_indices(src, np.repeat(src, 97, 0), np.eye(4), 0.05)


def _voxelize_check(xyz, voxel):
  from pointcontrast_amd.lib import device_loader as dl
  sel, coords = dl.sparse_quantize_index(xyz, voxel, return_coords=True)
  first, rcoords = er.voxelize_ref(xyz, voxel)
  assert sel.tolist() == first.tolist() and coords.tolist() == rcoords.tolist()
  return sel, coords


@pytest.mark.parametrize("n", [1, 512, 513])
def test_voxelize_sizes_around_the_table_doubling(n):
  rng = np.random.RandomState(n)
  sel, _ = _voxelize_check(rng.uniform(-0.3, 0.3, (n, 3)), 0.025)
  assert len(sel) > 0.9 * n
  sel, coords = _voxelize_check(rng.uniform(0.0251, 0.0499, (n, 3)) * [1, -1, 1], 0.025)  # all points in ONE voxel
  assert sel.tolist() == [0] and coords.tolist() == [[1, -2, 1]]


def test_voxelize_signed_zero_voxel_faces_and_the_range_limit():
  from pointcontrast_amd._lib import PcmiError
  from pointcontrast_amd.lib import device_loader as dl
  sel, coords = _voxelize_check(np.array([[0.0, -0.0, 0.0], [-0.0, 0.0, -0.0], [-1e-300, 0.0, 0.0]]), 0.25)
  assert sel.tolist() == [0, 2] and coords.tolist() == [[0, 0, 0], [-1, 0, 0]]  # -0.0 and +0.0 are the same voxel
  below = lambda v: np.nextafter(v, -np.inf)
  faces = np.array([[0.25, -0.25, 0.5], [below(0.25), -0.25, 0.5], [0.25, below(-0.25), 0.5], [0.25, -0.25, below(0.5)],
                    [0.25, -0.25, 0.5], [-0.5, 0.75, -0.0], [below(-0.5), 0.75, 0.0]])
  sel, coords = _voxelize_check(faces, 0.25)  # a point ON a face belongs to the voxel above it
  assert sel.tolist() == [0, 1, 2, 3, 5, 6] and coords[0].tolist() == [1, -1, 2] and coords[5].tolist() == [-3, 3, 0]
  L = float((1 << 20) - 1)
  rim = np.array([[L, 0.0, 0.0], [0.0, -L, 0.0], [0.0, 0.0, L + 0.5], [-L, -L, -L], [L, L, L], [0.5 - L, 0.0, 0.0]])
  sel, coords = _voxelize_check(rim, 1.0)  # voxel indices +-(2^20 - 1) are inside
  assert len(sel) == 6 and coords[3].tolist() == [-(1 << 20) + 1] * 3 and coords[4].tolist() == [(1 << 20) - 1] * 3
  for bad in ([L + 1, 0.0, 0.0], [0.0, -L - 1, 0.0], [0.0, 0.0, -L - 0.5]):  # voxel index +-2^20
    with pytest.raises(PcmiError, match="error -5"):
      dl.sparse_quantize_index(np.array([[0.0, 0.0, 0.0], bad]), 1.0)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_points_are_refused(bad):
  """NaN / +-inf in xyz, in src (also a finite point the transform makes non-finite) and in dst: PCMI_ERR_RANGE, as a
  point outside +-2^20 cells -- an explicit finiteness test in front of the float -> integer conversion, which the
  language leaves undefined for them.  oracle/loader_ref.py raises for the same inputs (tests/test_pretrain_edge_ref.py)."""
  from pointcontrast_amd._lib import PcmiError
  from pointcontrast_amd.lib import device_loader as dl
  rng = np.random.RandomState(0)
  pts = rng.uniform(-0.2, 0.2, (300, 3))
  for axis, row in ((0, 0), (1, 150), (2, 299)):
    x = pts.copy()
    x[row, axis] = bad
    with pytest.raises(PcmiError, match="error -5"):
      dl.sparse_quantize_index(x, 0.025)
    with pytest.raises(PcmiError, match="error -5"):
      dl.get_matching_indices(x, pts, np.eye(4), 0.03)
    with pytest.raises(PcmiError, match="error -5"):
      dl.get_matching_indices(pts, x, np.eye(4), 0.03)
  big = pts.copy()
  big[7, 0] = 1e308 if bad > 0 or bad != bad else -1e308  # finite, but not behind the transform
  with pytest.raises(PcmiError, match="error -5"):
    dl.get_matching_indices(big, pts, np.diag([10.0, 1.0, 1.0, 1.0]), 0.03)
  assert len(dl.get_matching_indices(pts, pts, np.eye(4), 0.03)) >= 300  # the same calls without the bad point
