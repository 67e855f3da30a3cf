"""The convolution stack on the occupancy extremes of tests/geometry_cases.py (pytest -m gpu, on a real MI355X).

Every other GPU test of the maps, the three spconv entry points, the tile units, the unit-balanced launch, the weight
gradients and the executor builds its voxels from helpers.surface_coords: 9..27 units per tile, every offset with pairs,
only the centre offset at the bound.  Here the same code runs on isolated lattices (1 unit per tile, 26 or 7 empty
offsets), solid boxes (every stride-2 offset at the bound), axis-aligned sheets, checkerboards and a mix of solid and
isolated rows in one level (tests/test_geometry_cases.py pins those properties on the CPU).

References: the maps and the float64 convolutions come from the CPU oracle's tables (oracle.sparse_ref), never from the
device's exports, so an error of a map cannot cancel.  Criteria: none is new -- integer tables bit-exact; convolutions
at test_gpu_c_contract.py's TOL (1e-4: rows and offset slices on their own scale, a slice without pairs exactly zero);
pooling at test_gpu_pooling.py's 1e-5; the executor at test_engine_matches_autograd_path's bounds.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import geometry_cases as gc
from c_contract import DEV, GUARD_BYTE, PCMI_ERR_WORKSPACE, Guarded, conv_ref64, lds, strided
from test_gpu_c_contract import (FORM_PAIRS, FORM_TABLE, FORM_TABLE_UNITS, KERNEL_NAMES, TOL, _Maps, _conv_contract, _conv_inputs,
                                 _dev, _maps, _ok, _planned, _stream, _vp, assert_close, assert_rows_close, assert_slices_close)
from test_gpu_parity import _check_maps, _make_models
from test_gpu_pretrain_edges import _read_i32

pytestmark = pytest.mark.gpu

ALL = sorted(gc.CASES)
# the clouds with at least 4096 rows: their 3^3 maps carry the sorted order and the tile units (rows pinned in test_geometry_cases.py)
SORTED = ["checker22", "iso4224", "mixed14", "mixed14_ordered", "sheet0_66", "sheet1_66", "sheet2_66", "solid16x2"]


@pytest.fixture(scope="module")
def lib():
  from pointcontrast_amd import _lib
  return _lib.lib


@pytest.fixture(scope="module")
def ME():
  import pointcontrast_amd.minkowski as me
  return me


def _rows(name):
  """A writable copy of a named cloud (geometry_cases keeps its own read-only)."""
  return np.array(gc.rows(name))


def _oracle(coords):
  from oracle import sparse_ref as sr
  return sr.CoordsManagerRef(coords)


# ------------------------------------------------------------------------------------------------
# a. maps: coordinates of every level, neighbour tables, pair lists and counts, bit-equal to the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_maps_match_oracle(ME, name):
  _check_maps(ME, _rows(name), levels=4)


# ------------------------------------------------------------------------------------------------
# b. the mask-sorted order and the tile units (include/pcmi.h: pcmi_kmap_t; csrc/sortrows.hip)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SORTED)
def test_tile_tables_hold_their_definition(ME, name):
  """perm is a permutation that keeps every row in its XCD chunk and sorts the chunk by occupancy mask;
  nbr_perm[k][i] = nbr[k][perm[i]]; tile_mask[t] = OR of the masks at positions [128 t, 128 t + 128); tile_pref = the
  exclusive prefix of their popcounts, the total at [n_tiles].  (The order among rows of equal mask is not promised and
  not checked; tile_mask and tile_pref do not depend on it.)"""
  from oracle import sparse_ref as sr
  coords = _rows(name)
  n = len(coords)
  nbr = _oracle(coords).kernel_map(0, 0, 3, sr.HYBRID).nbr
  cm = ME.CoordsManager(torch.from_numpy(coords).to(DEV))
  key = cm.key(0)
  m = cm.kernel_map(key, key, 3, 1, sr.HYBRID)
  torch.cuda.synchronize()
  n_tiles = -(-n // gc.TILE)
  assert m.perm and m.nbr_perm and m.tile_mask and m.tile_pref and m.n_tiles == n_tiles
  perm = _read_i32(m.perm, n)
  nbr_perm = _read_i32(m.nbr_perm, 27 * n).reshape(27, n)
  tile_mask = _read_i32(m.tile_mask, n_tiles).view(np.uint32).astype(np.int64)
  tile_pref = _read_i32(m.tile_pref, n_tiles + 1)
  assert (np.sort(perm) == np.arange(n)).all(), "perm is not a permutation of the rows"
  chunk = gc.xcd_chunk_rows(n)
  pos_chunk = np.arange(n) // chunk
  assert (perm // chunk == pos_chunk).all(), "a row left its XCD chunk"
  mask = gc.row_masks(nbr)
  d = np.diff(mask[perm])
  assert (d[pos_chunk[1:] == pos_chunk[:-1]] >= 0).all(), "masks along perm decrease inside a chunk"
  assert (nbr_perm == nbr[:, perm]).all(), "nbr_perm != nbr[:, perm]"
  padded = np.zeros(n_tiles * gc.TILE, np.int64)
  padded[:n] = mask[perm]
  want_mask = np.bitwise_or.reduce(padded.reshape(n_tiles, gc.TILE), axis=1)
  assert (tile_mask == want_mask).all(), "tile_mask"
  cnt = np.array([bin(int(v)).count("1") for v in want_mask], np.int64)
  assert (tile_pref == np.concatenate([[0], np.cumsum(cnt)])).all(), "tile_pref"
  _, ref_mask, ref_pref = gc.tile_tables(nbr)  # (the stable order of the restated rule gives the same units)
  assert (tile_mask == ref_mask).all() and (tile_pref == ref_pref).all()
  # the small levels carry no sorted order (pcmi.h: "stride-1 maps of large levels, else NULL")
  k1 = cm.stride(key, 2)
  if cm.size(k1) < gc.SORT_ROWS_MIN:
    m1 = cm.kernel_map(k1, k1, 3, 1, sr.HYBRID)
    assert not m1.perm and not m1.nbr_perm and not m1.tile_mask and not m1.tile_pref and m1.n_tiles == 0


# ------------------------------------------------------------------------------------------------
# c. forward, backward-data, backward-weight against float64 from the ORACLE's pair lists
# ------------------------------------------------------------------------------------------------
class _GeoMaps(_Maps):
  """_Maps over a named cloud whose get() hands out the oracle's pair lists (the device's own are held to them bit by
  bit in (a); a convolution compared with a reference built from the device's export would forgive a wrong map)."""

  def __init__(self, name):
    coords = _rows(name)
    super().__init__(len(coords), coords=coords)
    self.ref = _oracle(coords)

  def get(self, kind):
    from oracle import sparse_ref as sr
    if kind in ("k3", "k3_cube"):
      region = sr.HYBRID if kind == "k3" else sr.HYPERCUBE
      m = self.cm.kernel_map(self.key0, self.key0, 3, 1, region)
      rm = self.ref.kernel_map(0, 0, 3, region)
    else:
      m = self.cm.kernel_map(self.key0, self.cm.stride(self.key0, 2), 2, 2, 0)
      rm = self.ref.kernel_map(0, self.ref.stride(0, 2), 2)
    assert (int(m.n_in), int(m.n_out), int(m.K)) == (rm.n_in, rm.n_out, rm.K)
    pin = torch.from_numpy(np.concatenate([p[0] for p in rm.pairs]))
    pout = torch.from_numpy(np.concatenate([p[1] for p in rm.pairs]))
    tr = kind == "up"
    n_in, n_out = (rm.n_out, rm.n_in) if tr else (rm.n_in, rm.n_out)
    return m, int(tr), n_in, n_out, pin, pout, rm.offs.tolist()


_GEO = {}


def _geo(name):
  if name not in _GEO:
    _GEO.clear()  # one manager alive at a time (the cases are ordered by cloud)
    _GEO[name] = _GeoMaps(name)
  return _GEO[name]


def _bits(t):
  return t.contiguous().view(torch.int32)


def _twice_bit_equal(lib, maps, kind, cin, cout, gbias=True):
  """Two consecutive calls of each entry point on the same operands: bit-equal (the library promises determinism; the
  last-arriver reduction of the weight gradient and the fix-up order of a split launch are what could break it)."""
  m, tr, n_in, n_out, _, _, _ = maps.get(kind)
  K = m.K
  x, W, bias, gout = _conv_inputs(n_in, n_out, cin, cout, K, 77 + n_in)
  need = lib.pcmi_spconv_workspace_bytes(n_in, n_out, cin, cout, K, m.M)
  ws = Guarded(need)
  xd, Wd, bd, gd = _dev(x), _dev(W), _dev(bias), _dev(gout)
  st = _stream()
  res = []
  for _ in range(2):
    out = torch.full((n_out, cout), float("nan"), device=DEV)
    gw = torch.full((K, cin, cout), float("nan"), device=DEV)
    gb = torch.full((cout,), float("nan"), device=DEV)
    r = [out, gw, gb]
    _ok(lib, lib.pcmi_spconv_fwd(_vp(xd), cin, n_in, cin, _vp(Wd), cout, C.byref(m), tr, _vp(bd), _vp(out), cout, n_out, ws.vp,
                                 ws.size, st), "fwd")
    gin = torch.full((n_in, cin), float("nan"), device=DEV)
    _ok(lib, lib.pcmi_spconv_bwd_data(_vp(gd), cout, n_out, cout, _vp(Wd), cin, C.byref(m), tr, _vp(gin), cin, n_in, ws.vp,
                                      ws.size, st), "bwd_data")
    r.append(gin)
    _ok(lib, lib.pcmi_spconv_bwd_weight(_vp(xd), cin, n_in, cin, _vp(gd), cout, n_out, cout, C.byref(m), tr, _vp(gw),
                                        _vp(gb) if gbias else None, ws.vp, ws.size, st), "bwd_weight")
    res.append([t.clone() for t in r])
  ws.check("workspace")
  for nm, a, b in zip(("out", "gW", "gbias", "gin"), res[0], res[1]):
    if nm == "gbias" and not gbias:
      continue
    assert bool(torch.isfinite(a).all()), "%s: an element was not written" % nm
    assert torch.equal(_bits(a), _bits(b)), "%s %d->%d %s: two consecutive calls differ" % (kind, cin, cout, nm)


# RW = 1: iso40, solid3x4x3 (36 rows).  The 16-row / split-precision range: solid8 (512 rows exactly), the sheets (576),
# iso600, checker12 (864).  Sorted order: the >= 4096-row clouds; solid16x2 has exactly 8192 rows (wgrad_x3t's default
# threshold and the slice-width threshold).
# (32, 32): spconv32r; (64, 96): the split-precision forward and an odd N / 32; (128, 64).
PAIRS = [(32, 32), (64, 96), (128, 64)]


@pytest.mark.parametrize("cin,cout", PAIRS)
@pytest.mark.parametrize("kind", ["k3", "down", "up"])
@pytest.mark.parametrize("name", ALL)
def test_conv_entry_points_against_float64(lib, name, kind, cin, cout):
  maps = _geo(name)
  wide = cin >= 64 and cout >= 64
  # the weight gradient of the wide pairs also without gbias: only then the launch may take wgrad_x3t (>= 8192 rows)
  _conv_contract(lib, maps, kind, cin, cout, also_without_gbias=wide)
  _twice_bit_equal(lib, maps, kind, cin, cout)
  if wide:
    _twice_bit_equal(lib, maps, kind, cin, cout, gbias=False)


def _stem_contract(lib, maps):
  """The 3 -> 32 HYPERCUBE stem: forward with bias, weight gradient with gbias (stem_wgrad_kernel over the pair lists) and
  without (stem_wgrad_mfma_kernel, which walks nbr); it has no input gradient.  Exact workspace, strided rows."""
  kind, cin, cout = "k3_cube", 3, 32
  m, tr, n_in, n_out, pin, pout, offs = maps.get(kind)
  K = m.K
  x, W, bias, gout = _conv_inputs(n_in, n_out, cin, cout, K, 5 + n_in)
  ref_out, _, ref_gW, ref_gb = conv_ref64(x, W, pin, pout, offs, n_out, gout=gout, bias=bias)
  need = lib.pcmi_spconv_workspace_bytes(n_in, n_out, cin, cout, K, m.M)
  Wd, bd = _dev(W), _dev(bias)
  st = _stream()
  for form in (0, 1):
    tag = "stem n=%d form %d" % (n_in, form)
    ws = Guarded(need)
    (ild, ioff), (old, ooff) = lds(cin, form), lds(cout, form)
    xin, go, out = strided(n_in, cin, ild, ioff, x), strided(n_out, cout, old, ooff, gout), strided(n_out, cout, old, ooff)
    gw, gb = Guarded(K * cin * cout * 4), Guarded(cout * 4)
    rc = lib.pcmi_spconv_fwd(xin.vp, ild, n_in, cin, _vp(Wd), cout, C.byref(m), 0, _vp(bd), out.vp, old, n_out, ws.vp, ws.size, st)
    _ok(lib, rc, tag + " fwd")
    for s_ in (ws, out, xin):
      s_.check(tag + " fwd")
    first = out.cpu()
    assert_rows_close(first, ref_out, TOL, tag + " out")
    out.view.fill_(float("nan"))  # ... and again: bit-equal
    rc = lib.pcmi_spconv_fwd(xin.vp, ild, n_in, cin, _vp(Wd), cout, C.byref(m), 0, _vp(bd), out.vp, old, n_out, ws.vp, ws.size, st)
    _ok(lib, rc, tag + " fwd")
    assert torch.equal(_bits(out.cpu()), _bits(first)), tag + " out: two calls differ"
    for with_gbias in (True, False):
      t2 = tag + (" bwd_weight" if with_gbias else " bwd_weight (no gbias)")
      gw.buf[gw.lead:gw.lead + gw.nbytes] = 0x7F
      rc = lib.pcmi_spconv_bwd_weight(xin.vp, ild, n_in, cin, go.vp, old, n_out, cout, C.byref(m), 0, gw.vp,
                                      gb.vp if with_gbias else None, ws.vp, ws.size, st)
      _ok(lib, rc, t2)
      for s_ in (ws, gw, gb, xin, go):
        s_.check(t2)
      g = gw.view(torch.float32, K * cin * cout).view(K, cin, cout).cpu()
      assert_slices_close(g, ref_gW, TOL, t2 + " gW")
      if with_gbias:
        assert_close(gb.view(torch.float32, cout).cpu(), ref_gb, TOL, t2 + " gbias")
      # ... and again: bit-equal
      rc = lib.pcmi_spconv_bwd_weight(xin.vp, ild, n_in, cin, go.vp, old, n_out, cout, C.byref(m), 0, gw.vp,
                                      gb.vp if with_gbias else None, ws.vp, ws.size, st)
      _ok(lib, rc, t2)
      assert torch.equal(_bits(gw.view(torch.float32, K * cin * cout).cpu()), _bits(g.view(-1))), t2 + ": two calls differ"


@pytest.mark.parametrize("name", ["iso40", "solid3x4x3", "sheet0_24", "mixed14"])
def test_stem_conv_against_float64(lib, name):
  _stem_contract(lib, _geo(name))


@pytest.mark.parametrize("x3p", ["1", "0"])
@pytest.mark.parametrize("name", ["iso600", "sheet1_24"])
def test_small_clouds_on_the_tile_stationary_weight_gradient(lib, name, x3p, monkeypatch):
  """PCMI_WGRAD_X3T=1 sends every 3^3 weight gradient without gbias to wgrad_x3t (both PCMI_WGRAD_X3P forms): on the
  isolated lattice 26 of its 27 slabs, on a sheet 18, sum to exactly zero."""
  monkeypatch.setenv("PCMI_WGRAD_X3T", "1")
  monkeypatch.setenv("PCMI_WGRAD_X3P", x3p)
  maps = _geo(name)
  for cin, cout in ((64, 96), (128, 64)):
    _conv_contract(lib, maps, "k3", cin, cout, forms=(0,), also_without_gbias=True)
    _twice_bit_equal(lib, maps, "k3", cin, cout, gbias=False)


# ------------------------------------------------------------------------------------------------
# d. the unit-balanced launch where run_gathered really takes it
# ------------------------------------------------------------------------------------------------
# run_gathered takes it only with ksplit == 1: ceil(rows / 128) * (N / 32 / NT) >= 2.5 workgroups per CU = 640 on this part.
#   fp32 16-row kernel (spconv16p_kernel<1, ., SK>): 224 -> 224 (NT = 1, 7 column slices, 7 chunk steps per unit) at
#     11 776 rows = 92 tiles x 7 = 644, PCMI_SPCONV_STREAMK=16; the isolated lattice has 92 units = 644 steps for the 1024
#     workgroups (per == 1, 380 of them return at once);
#   split-precision kernel (spconv16x_kernel): 64 -> 64 (NT = 2, one column slice) at 81 920 rows = 640 tiles, default
#     threshold.
def _sk_cloud(which):
  if which == "iso11776":
    return gc.isolated(11776, 32, (1, 1, 1), 2)
  if which == "mixed20":
    return gc.mixed(20, 3776, True)
  if which == "mixed20_ordered":
    return gc.mixed(20, 3776, False)
  if which == "iso81920":
    return gc.isolated(81920, 2, (1, 0, 1), 1)
  assert which == "mixed40"
  return gc.mixed(40, 17920, True)


def _fp64_from_table(nbr, x, W):
  """sum_k x[nbr_k] @ W[k] in float64 on the device, nbr = the ORACLE's table (uploaded)."""
  y = torch.zeros(nbr.shape[1], W.shape[2], dtype=torch.float64, device=x.device)
  xd, Wd = x.double(), W.double()
  for k in range(W.shape[0]):
    ok = nbr[k] >= 0
    if bool(ok.any()):
      y[ok] += xd[nbr[k][ok]] @ Wd[k]
  return y


SK_CASES = [("iso11776", 224, 224, "16"), ("mixed20", 224, 224, "16"), ("mixed20_ordered", 224, 224, "16"),
            ("iso81920", 64, 64, None), ("mixed40", 64, 64, None)]


@pytest.mark.parametrize("which,cin,cout,streamk", SK_CASES)
def test_unit_balanced_launch_on_extreme_tiles(lib, ME, which, cin, cout, streamk, monkeypatch):
  """Forward and backward-data through the unit-balanced launch against float64 from the oracle's neighbour table, rows
  at 1e-4, and against the one-tile-per-workgroup launch (PCMI_SPCONV_STREAMK=0) at
  test_full_size_streamk_matches_plain's 1e-5.  pcmi_spconv_plan reports which launch is taken: a unit-balanced kernel
  in the first mode, a table kernel in the second, no offset split in either.  A kernel trace of this test
  alone (MI355X, 256 CUs) showed the same: 20 launches of sk_fixup_kernel = 5 cases x 2 calls x (forward, backward-data), 12 of
  spconv16p_kernel<1, ., SK = true> and 16 of spconv16x_kernel<2, SK = true, ., 3> (8 per direction), against 12 + 16 of
  the SK = false forms in the plain mode and no split_reduce_kernel.  The test also holds it itself: the shapes
  are checked against plan_conv's rule with the device's CU count, and wherever a tile is cut between workgroups the two
  modes must NOT be bit-equal (another summation order).  iso81920 is the exception: 1280 chunk steps over the 768
  workgroups of spconv16x_kernel<2> are 2 each = exactly one tile, so 640 workgroups write whole tiles, 128 return at
  once, the fix-up kernel finds nothing to sum and the result is bit-equal to the plain launch (observed)."""
  from oracle import sparse_ref as sr
  from pointcontrast_amd import functional as PF
  coords = _sk_cloud(which)
  n = len(coords)
  n_tiles = -(-n // 128)
  nt = 1 if cout == 224 else 2  # plan_conv: N / 32 = 7 -> NT 1; N / 32 = 2 -> NT 2
  target = 25 * torch.cuda.get_device_properties(0).multi_processor_count // 10  # plan_conv: 2.5 workgroups per CU
  # ksplit == 1, forward and backward-data alike (on a part with more CUs the shapes must grow: this then fails)
  assert cin == cout and n_tiles * (cout // 32 // nt) >= target, (n_tiles, target)
  rm = _oracle(coords).kernel_map(0, 0, 3, sr.HYBRID)
  _, _, pref = gc.tile_tables(rm.nbr)
  units = np.diff(pref)
  if which.startswith("iso"):
    assert pref[-1] == n_tiles and rm.offs[-1] == n  # one unit per tile: centre only
    if which == "iso11776":
      assert pref[-1] * (cin // 32) == 644 < 1024  # fewer chunk steps than workgroups
  else:
    assert units.min() == 1 and units.max() == 27
  print("%s: %d rows, %d tiles, units per tile %d..%d, %d in total" % (which, n, n_tiles, units.min(), units.max(), pref[-1]))
  st = ME.SparseTensor(torch.zeros((n, 4)), coords=torch.from_numpy(coords)).to(DEV)
  cm, key = st.coords_man, st.coords_key
  m = cm.kernel_map(key, key, 3, 1, 3)
  assert m.n_tiles == n_tiles and m.tile_pref and m.perm
  assert _read_i32(m.tile_pref, n_tiles + 1)[-1] == pref[-1]
  torch.manual_seed(2)
  W = (torch.randn(27, cin, cout, device=DEV) / cin ** 0.5).requires_grad_(True)
  b = torch.randn(cout, device=DEV)
  g = torch.randn(n, cout, device=DEV)
  x0 = torch.randn(n, cin, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
  nbr = torch.from_numpy(rm.nbr).to(DEV).long()
  off = sr.region_offsets(3, sr.HYBRID)
  mirror = [int(np.nonzero((off == -off[k]).all(1))[0][0]) for k in range(27)]
  y64 = _fp64_from_table(nbr, x0, W.detach()) + b.double()
  g64 = _fp64_from_table(nbr, g, W.detach()[mirror].transpose(1, 2))  # gin[i] = sum_k gout[nbr_k(i)] @ W[mirror(k)]^T
  res = {}
  for mode in ("sk", "0"):
    if mode == "0":
      monkeypatch.setenv("PCMI_SPCONV_STREAMK", "0")
    elif streamk is not None:
      monkeypatch.setenv("PCMI_SPCONV_STREAMK", streamk)
    # forward and backward-data are one plan (cin == cout, the same rows and map)
    kernel, _, slice_, ksplit, _ = _planned(lib, n, n * cin * 4, cin, cout, 27, FORM_TABLE_UNITS)
    want = ("units_16", "units_x3") if mode == "sk" else ("table_16", "table_x3")
    assert KERNEL_NAMES[kernel] in want and ksplit == 1 and slice_ == nt, (which, mode, KERNEL_NAMES[kernel], slice_, ksplit)
    for rep in range(2):
      x = x0.clone().requires_grad_(True)
      y = PF.SparseConvFunction.apply(x, W, b, m, False, n, cm)
      y.backward(g)
      torch.cuda.synchronize()
      res[(mode, rep)] = (y.detach().clone(), x.grad.clone())
  monkeypatch.delenv("PCMI_SPCONV_STREAMK")
  for mode in ("sk", "0"):
    assert_rows_close(res[(mode, 0)][0], y64, TOL, "%s %s forward vs float64" % (which, mode))
    assert_rows_close(res[(mode, 0)][1], g64, TOL, "%s %s backward-data vs float64" % (which, mode))
    for i, nm in enumerate(("forward", "backward-data")):
      assert torch.equal(_bits(res[(mode, 0)][i]), _bits(res[(mode, 1)][i])), "%s %s %s: two calls differ" % (which, mode, nm)
  print("%s: bit-equal to the plain launch: forward %s, backward-data %s" % (
      which, torch.equal(res[("sk", 0)][0], res[("0", 0)][0]), torch.equal(res[("sk", 0)][1], res[("0", 0)][1])))
  for i, nm in enumerate(("forward", "backward-data")):
    same = torch.equal(res[("sk", 0)][i], res[("0", 0)][i])
    assert same == (which == "iso81920"), "%s %s: PCMI_SPCONV_STREAMK did not switch launches as expected" % (which, nm)
  assert_close(res[("sk", 0)][0], res[("0", 0)][0], 1e-5, which + " unit-balanced forward vs plain")
  assert_close(res[("sk", 0)][1], res[("0", 0)][1], 1e-5, which + " unit-balanced backward-data vs plain")


# ------------------------------------------------------------------------------------------------
# d2. every kernel family with exactly the workspace its plan names
# ------------------------------------------------------------------------------------------------
# (planned kernel, rows of test_gpu_c_contract's voxel set or a cloud of _sk_cloud, map, cin, cout, PCMI_SPCONV_STREAMK)
PLAN_CASES = [("pair", 530, "up", 128, 64, None), ("deep", 256, "k3", 64, 64, None), ("plain", 47, "k3", 64, 64, None),
              ("table_16", 512, "k3", 32, 64, None), ("table_x3", 512, "k3", 64, 64, None), ("32r", 8192, "k3", 32, 32, None),
              ("units_16", "iso11776", "k3", 224, 224, "16"), ("units_x3", "iso81920", "k3", 64, 64, None)]


@pytest.mark.parametrize("family,cloud,kind,cin,cout,streamk", PLAN_CASES)
def test_forward_accepts_exactly_the_planned_workspace(lib, family, cloud, kind, cin, cout, streamk, monkeypatch):
  """One forward per kernel family of plan_conv (csrc/spconv_plan.h): pcmi_spconv_plan names the family the case is meant
  for (asserted first: a wrong shape fails, it does not pass vacuously) and the smallest workspace the call accepts.  With
  exactly that many bytes between guard bands the call succeeds and matches float64 at TOL; with one byte less it returns
  PCMI_ERR_WORKSPACE and writes nothing (a refused call enqueues nothing).  The pair tiles and spconv32r use no workspace:
  their plan says 0 bytes and there is no shorter call."""
  if streamk is not None:
    monkeypatch.setenv("PCMI_SPCONV_STREAMK", streamk)
  if isinstance(cloud, str):
    coords = _sk_cloud(cloud)
    maps = _Maps(len(coords), coords=coords)
  else:
    maps = _maps(cloud)
  m, tr, n_in, n_out, pin, pout, offs = maps.get(kind)
  K = m.K
  (ild, ioff), (old, ooff) = lds(cin, 0), lds(cout, 0)
  units = bool(m.tile_pref and m.perm and m.nbr_perm) and m.n_tiles == -(-n_out // 128)
  form = FORM_PAIRS if tr else (FORM_TABLE_UNITS if units else FORM_TABLE)
  kernel, _, _, ksplit, need = _planned(lib, n_out, n_in * ild * 4, cin, cout, K, form)
  assert KERNEL_NAMES[kernel] == family, (KERNEL_NAMES[kernel], n_in, n_out, K, form)
  if family == "plain":
    assert ksplit == 27
  assert (need == 0) == (family in ("pair", "32r")), need
  x, W, bias, _ = _conv_inputs(n_in, n_out, cin, cout, K, 11 + n_in)
  ref = conv_ref64(x, W, pin, pout, offs, n_out, transpose=bool(tr), bias=bias)
  Wd, bd = _dev(W), _dev(bias)
  ws = Guarded(need)
  xin, out = strided(n_in, cin, ild, ioff, x), strided(n_out, cout, old, ooff)
  st = _stream()
  tag = "%s %s %d->%d rows %d" % (family, kind, cin, cout, n_out)

  def fwd(nbytes):
    return lib.pcmi_spconv_fwd(xin.vp, ild, n_in, cin, _vp(Wd), cout, C.byref(m), tr, _vp(bd), out.vp, old, n_out, ws.vp,
                               C.c_size_t(nbytes), st)

  if need > 0:
    rc = fwd(need - 1)
    torch.cuda.synchronize()
    assert rc == PCMI_ERR_WORKSPACE, "%s: one byte short returned %d (%s)" % (tag, rc, lib.pcmi_last_error().decode())
    assert out.untouched(), tag + ": the refused call wrote into the output"
    assert bool((ws.buf == GUARD_BYTE).all()), tag + ": the refused call wrote into the workspace"
  _ok(lib, fwd(need), tag + " fwd with the planned %d bytes" % need)
  ws.check(tag + " workspace (%d bytes planned)" % need)
  out.check(tag + " out")
  xin.check(tag + " in")
  assert_rows_close(out.cpu(), ref, TOL, tag + " out")


# ------------------------------------------------------------------------------------------------
# e. pooling on the same clouds
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("average", [False, True])
@pytest.mark.parametrize("ks,stride", [(2, 2), (3, 1)])
@pytest.mark.parametrize("C_", [13, 96])
@pytest.mark.parametrize("name", ["iso600", "solid8", "checker12"])
def test_pooling_on_occupancy_extremes(name, C_, ks, stride, average):
  """iso600: every count is 1; solid8: counts 8 (stride 2) and up to 27 (3^3); checker12: 13 of 27."""
  import test_gpu_pooling as tp
  coords = _rows(name)
  cmr = _oracle(coords)
  st, f = tp._tensor(coords, torch.randn(len(coords), C_, generator=torch.Generator().manual_seed(C_)))
  out_key = cmr.stride(0, 2) if stride == 2 else 0
  nbr = cmr.kernel_map(0, out_key, ks, 0).nbr
  counts = (nbr >= 0).sum(0)
  want = {"iso600": (1, 1), "solid8": (8, 8) if stride == 2 else (8, 27), "checker12": (4, 4) if stride == 2 else (4, 13)}[name]
  assert (int(counts.min()), int(counts.max())) == want
  tp._run_pool(st, f, cmr, 0, out_key, nbr, average, tp._pool_module(average, ks, stride, 0), C_)


@pytest.mark.parametrize("cls_name", ["MinkowskiAvgUnpooling", "MinkowskiPoolingTranspose"])
@pytest.mark.parametrize("C_", [13, 96])
@pytest.mark.parametrize("name", ["iso600", "solid8", "checker12"])
def test_unpooling_on_occupancy_extremes(ME, name, C_, cls_name):
  import pool_ref as R
  import test_gpu_pooling as tp
  coords = _rows(name)
  st, _ = tp._tensor(coords, torch.randn(len(coords), C_), requires_grad=False)
  cm = st.coords_man
  k1 = cm.stride(st.coords_key, 2)
  cmr = _oracle(coords)
  r1 = cmr.stride(0, 2)
  p1 = R.align_rows(cm.get_coords(k1).cpu().numpy(), cmr.coords[r1])
  g = torch.randn(len(p1), C_, dtype=torch.float64, generator=torch.Generator().manual_seed(C_ + 1))
  gd = torch.empty_like(g)
  gd[p1] = g
  sc, fc = tp._on_key(gd, k1, cm)
  out = getattr(ME, cls_name)(kernel_size=2, stride=2, dimension=3)(sc)
  assert out.coords_key == st.coords_key
  g64 = g.clone().requires_grad_(True)
  want = R.unpool(g64, cmr.kernel_map(0, r1, 2).nbr, len(coords))
  tp._check(out.F.detach(), want, tp.POOL_TOL, "unpool fwd")
  dy = torch.randn(want.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(C_ + 2))
  out.F.backward(dy.to(DEV, torch.float32))
  want.backward(dy)
  tp._check(fc.grad[p1.to(DEV)], g64.grad, tp.POOL_TOL, "unpool bwd")


# ------------------------------------------------------------------------------------------------
# f. the executor
# ------------------------------------------------------------------------------------------------
def _engine_clouds(which):
  if which == "isolated":  # 600 rows on all five levels, every 3^3 map centre-only, every stride-2 map one child per parent
    return [gc.isolated(600, 32, (1, 0, 1), 2), gc.isolated(600, 32, (0, 0, 0), 1)], [600] * 5
  # solid 32 x 32 x 16, two instances: every stride-2 offset exactly at the bound, 8 rows at the coarsest level
  # (pass 1 is half the box, 16 x 16 x 32: 16384 / 2048 / 256 / 32 / 4 rows -- the CPU oracles of a second full box would
  #  double the test's time)
  return [gc.solid(32, 32, 16, 2, (-32, 0, -16)), gc.solid(16, 16, 32, 2, (0, -16, -16))], [32768, 4096, 512, 64, 8]


@pytest.mark.parametrize("which", ["isolated", "solid"])
def test_engine_on_occupancy_extremes(ME, which):
  """Res16UNet14 through the native executor, training mode, pass 0 and pass 1, against the per-layer autograd path on
  the same device (features 1e-5, every gradient tensor 1e-6 of its scale -- test_engine_matches_autograd_path's bounds;
  a weight gradient that is not bit-equal because the executor sizes its chunks from the bound and the eager path from
  the counts is held slice by slice to the 1e-5 of test_grouped_weight_gradients_match_single_launches), and its
  features per row against the fp32 oracle model: max(1e-4, 10 x the fp32 oracle's own worst row error against the
  float64 oracle on the same cloud) -- an 8-row BatchNorm at the coarsest level may be ill-conditioned, which is no
  kernel error.

  Measured fp32-oracle worst row error against the float64 oracle (CPU; it moves with the thread count): isolated
  1.6e-5 .. 2.1e-5 on either pass (bounds 1.6e-4 .. 2.1e-4), solid 8e-6 .. 9e-6 (the 1e-4 floor holds).  Observed on an
  MI355X: device against the fp32 oracle 2.0e-5 / 2.4e-5 (isolated), 1.2e-5 / 1.3e-5 (solid); engine against the autograd
  path 16 / 6 of 98 gradient tensors not bit-equal, worst 4.2e-7 / 7.5e-7 (the slice-wise ceiling was never needed).  The
  solid cloud's second pass is half the box to keep the CPU oracles at a few seconds."""
  import copy
  from oracle import sparse_ref as sr
  from pointcontrast_amd.engine import NativeEngine
  from pointcontrast_amd.lib.config import get_config
  from pointcontrast_amd.lib.distributed import FlatParameters
  clouds, level_rows = _engine_clouds(which)
  cfg = get_config([])
  ref, dev = _make_models("Res16UNet14", cfg, seed=3)
  ref.train()
  dev.train()
  for c in clouds:
    r = _oracle(c)
    key, got = 0, []
    for _ in range(5):
      got.append(r.size(key))
      key = r.stride(key, 2) if len(got) < 5 else key
    assert got == level_rows or (which == "solid" and c is clouds[1] and got == [v // 2 for v in level_rows])
  gen = torch.Generator().manual_seed(9)
  Fin = [torch.randn(len(c), 3, generator=gen) for c in clouds]
  flat = FlatParameters(dev.parameters())
  eng = NativeEngine(dev, flat)
  sts = [ME.SparseTensor(Fin[i], coords=torch.from_numpy(np.array(clouds[i]))).to(DEV) for i in range(2)]
  rs = {k: v.clone() for k, v in dev.state_dict().items() if "running" in k}
  fa = [dev(st).F for st in sts]
  g = [torch.randn(f.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4 + i)) for i, f in enumerate(fa)]
  flat.zero_grad()
  (fa[0] * g[0]).sum().backward()
  (fa[1] * g[1]).sum().backward()
  ga = flat.g.clone()
  rs_after = {k: v.clone() for k, v in dev.state_dict().items() if "running" in k}
  dev.load_state_dict({**dev.state_dict(), **rs})  # rewind the BN running statistics
  fe = [eng.forward(i, sts[i]) for i in range(2)]
  for i in range(2):
    assert_close(fe[i], fa[i], 1e-5, "%s engine features pass %d" % (which, i))
  flat.zero_grad()
  eng.backward(1, g[1])
  eng.backward(0, g[0])
  torch.cuda.synchronize()
  scale = float(ga.abs().max())
  names = {id(p): n for n, p in dev.named_parameters()}
  worst, worst_name, not_equal = 0.0, "", 0
  for i, p in enumerate(flat.params):
    a, e = flat.view(ga, i), flat.view(flat.g, i)
    if torch.equal(a, e):
      continue
    not_equal += 1
    err = float((a - e).abs().max()) / max(float(a.abs().max()), 1e-4 * scale)
    if err > worst:
      worst, worst_name = err, names[id(p)]
    if err <= 1e-6:
      continue
    assert p.dim() == 3, "%s: %.2e > 1e-6 and not a convolution kernel" % (names[id(p)], err)
    assert_slices_close(e, a, 1e-5, "%s engine vs autograd %s" % (which, names[id(p)]))
  print("%s: engine vs autograd: %d of %d gradient tensors not bit-equal, worst %.2e (%s)" % (
      which, not_equal, len(flat.params), worst, worst_name))
  for k, v in dev.state_dict().items():
    if "running" in k:
      assert_close(v, rs_after[k], 1e-5, "engine " + k)
  eng._held[0] = eng._held[1] = None
  # ---- the fp32 oracle model, per row; its own error against the float64 oracle sets the bound ----
  ref64 = copy.deepcopy(ref).double()
  with torch.no_grad():
    for i in range(2):
      f32 = ref(sr.SparseTensorRef(Fin[i], coords=np.array(clouds[i]))).F
      f64 = ref64(sr.SparseTensorRef(Fin[i].double(), coords=np.array(clouds[i]))).F
      own = float(((f32.double() - f64).norm(dim=1) / f64.norm(dim=1)).max())
      bound = max(1e-4, 10 * own)
      got = fe[i].detach().double().cpu()
      e32 = float(((got - f32.double()).norm(dim=1) / f32.double().norm(dim=1)).max())
      e64 = float(((got - f64).norm(dim=1) / f64.norm(dim=1)).max())
      print("%s pass %d: fp32 oracle vs float64 oracle worst row %.2e (bound %.2e); device vs fp32 oracle %.2e, vs float64 %.2e" % (
          which, i, own, bound, e32, e64))
      assert e32 <= bound, "%s pass %d: worst row %.2e > %.2e against the fp32 oracle" % (which, i, e32, bound)
