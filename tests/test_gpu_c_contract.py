"""The C contract of include/pcmi.h, held to its word (pytest -m gpu, on a real MI355X).

The other GPU tests reach libpcmi through pointcontrast_amd/functional.py, which hands every call a shared scratch
buffer of at least 16 MiB and packed outputs (ld == channels).  The native executor (csrc/engine.hip) and any C caller
do neither: the arena is sized with exactly what the *_workspace_bytes query returns, and outputs are column slices of
wider concatenation buffers (ld > channels at a column offset).  Here the entry points are called through ctypes in
that form:
  - workspaces of EXACTLY the queried size between guard bands (tests/c_contract.py: an overrun is a failed assertion,
    never a fault, since the bands lie inside the same allocation);
  - inputs and outputs as [rows, c] slices of [rows, ld] buffers filled with a NaN sentinel: everything outside the
    slice must still hold the sentinel's bits afterwards;
  - row counts one either side of every threshold where the planners (csrc/spconv_plan.h plan_conv,
    csrc/spconv_wgrad.hip, csrc/norm.hip) change kernel, tile shape, slice width or reduction form.

Criteria: none is new.  Convolutions: test_gpu_parity.py's (max|err| <= 1e-4 * max|ref|; feature / input-gradient
matrices also per ROW, weight gradients also per offset SLICE, a slice without pairs exactly zero), against a float64
restatement on the CPU from the exported map.  BatchNorm: test_batchnorm_parity's 1e-4 (outputs, running estimates,
gradients against float64).  ReLU / add / gather: bit-exact; l2norm 1e-6 / 1e-5, scatter-add 1e-5, bn eval 1e-5
(test_bn_eval_relu_add_l2norm, test_gather_scatter_rows).  Ops with a workspace but no leading dimension: bit-identical
to the same call given a 64 MiB workspace.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import c_contract as cc
from c_contract import DEV, PCMI_ERR_INVALID, PCMI_ERR_WORKSPACE, PCMI_OK, Guarded, conv_ref64, coords_with_rows, lds, strided

pytestmark = pytest.mark.gpu

TOL = 1e-4  # the north_star's relative tolerance, as stated at the head of test_gpu_parity.py


# ------------------------------------------------------------------------------------------------
# criteria of test_gpu_parity.py, restated
# ------------------------------------------------------------------------------------------------
def rel_err(got, ref):
  got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
  return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def assert_close(got, ref, tol, what):
  assert bool(torch.isfinite(got).all()), "%s: non-finite values (an element was not written?)" % what
  e = rel_err(got, ref)
  print("%s: rel err %.3e (bound %.1e)" % (what, e, tol))
  assert e <= tol, "%s: rel err %.3e > %.1e (shape %s)" % (what, e, tol, tuple(ref.shape))


def assert_rows_close(got, ref, tol, what):
  assert_close(got, ref, tol, what)
  got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
  e = float(((got - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-30)).max())
  print("%s: worst row rel err %.3e (bound %.1e)" % (what, e, tol))
  assert e <= tol, "%s: worst row rel err %.3e > %.1e (shape %s)" % (what, e, tol, tuple(ref.shape))


def assert_slices_close(got, ref, tol, what):
  assert_close(got, ref, tol, what)
  got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
  for k in range(ref.shape[0]):
    scale = float(ref[k].abs().max())
    err = float((got[k] - ref[k]).abs().max())
    if scale == 0.0:
      assert err == 0.0, "%s: slice %d has no pairs but the device wrote %.3e" % (what, k, err)
    else:
      assert err <= tol * scale, "%s: slice %d rel err %.3e > %.1e (its max %.3e)" % (what, k, err / scale, tol, scale)


# ------------------------------------------------------------------------------------------------
# plumbing
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
  from pointcontrast_amd import _lib
  return _lib.lib


def _stream():
  return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _vp(t):
  return None if t is None else C.c_void_p(t.data_ptr())


def _ok(lib, rc, what):
  assert rc == PCMI_OK, "%s: returned %d (%s)" % (what, rc, lib.pcmi_last_error().decode())
  torch.cuda.synchronize()


def _dev(t):
  return t.to(DEV).contiguous()


# include/pcmi.h: PCMI_CONV_FORM_* and PCMI_CONV_KERNEL_*
FORM_NONE, FORM_TABLE, FORM_TABLE_UNITS, FORM_PAIRS = range(4)
KERNEL_NAMES = ("pair", "32r", "units_16", "units_x3", "table_x3", "table_16", "deep", "plain")


def _planned(lib, rows, x_bytes, c, n, k, form):
  """pcmi_spconv_plan: (kernel, row tile / 32, slice width / 32, ksplit, ws_bytes) of one forward / backward-data launch."""
  o = [C.c_int() for _ in range(4)]
  ws = C.c_size_t()
  rc = lib.pcmi_spconv_plan(rows, x_bytes, c, n, k, form, *[C.byref(v) for v in o], C.byref(ws))
  assert rc == PCMI_OK, lib.pcmi_last_error().decode()
  return tuple(v.value for v in o) + (ws.value,)


class _Maps:
  """One coordinate manager over the first n rows of the fixed voxel set (or over a given int32 [n, 4] coordinate
  array), its maps and their exported pair lists."""

  def __init__(self, n, base="mid", coords=None):
    import pointcontrast_amd.minkowski as me
    coords = coords_with_rows(n, base) if coords is None else np.ascontiguousarray(coords)
    assert len(coords) == n
    self.cm = me.CoordsManager(torch.from_numpy(coords).to(DEV))
    self.key0 = self.cm.key(0)
    self.n = n
    self._exp = {}

  def get(self, kind):
    """(map, transpose, n_in, n_out, pair_in, pair_out, offs) of 'k3' (3^3 hybrid, stride 1), 'down' (2^3, stride 2) or
    'up' (its transposed convolution)."""
    if kind == "k3":
      m = self.cm.kernel_map(self.key0, self.key0, 3, 1, 3)
    else:
      m = self.cm.kernel_map(self.key0, self.cm.stride(self.key0, 2), 2, 2, 0)
    if id(m) not in self._exp:
      _, pin, pout = self.cm.export_map(m)
      self._exp[id(m)] = (pin.cpu(), pout.cpu(), list(m.offs_host[:m.K + 1]))
    pin, pout, offs = self._exp[id(m)]
    tr = kind == "up"
    n_in, n_out = (m.n_out, m.n_in) if tr else (m.n_in, m.n_out)
    return m, int(tr), int(n_in), int(n_out), pin, pout, offs


_MAPS = {}


def _maps(n, base="mid"):
  if (n, base) not in _MAPS:
    _MAPS.clear()  # one manager alive at a time (cases are ordered by n)
    _MAPS[(n, base)] = _Maps(n, base)
  return _MAPS[(n, base)]


def _conv_inputs(n_in, n_out, cin, cout, K, seed):
  g = torch.Generator().manual_seed(seed)
  x = torch.randn(n_in, cin, generator=g)
  W = torch.randn(K, cin, cout, generator=g) / float(np.sqrt(cin))
  bias = torch.randn(cout, generator=g)
  gout = torch.randn(n_out, cout, generator=g)
  return x, W, bias, gout


def _conv_contract(lib, maps, kind, cin, cout, forms=(0, 1), also_without_gbias=False, seed=0):
  """Forward (with bias), backward-data and backward-weight (with gbias) of one convolution with the exact queried
  workspace between guard bands and every matrix a column slice of a wider buffer; the float64 reference once."""
  m, tr, n_in, n_out, pin, pout, offs = maps.get(kind)
  K = m.K
  x, W, bias, gout = _conv_inputs(n_in, n_out, cin, cout, K, seed + n_in)
  ref_out, ref_gin, ref_gW, ref_gb = conv_ref64(x, W, pin, pout, offs, n_out, transpose=bool(tr), gout=gout, bias=bias)
  need = lib.pcmi_spconv_workspace_bytes(n_in, n_out, cin, cout, K, m.M)
  Wd, bd = _dev(W), _dev(bias)
  st = _stream()
  for form in forms:
    tag = "%s n_in=%d n_out=%d %d->%d form %d" % (kind, n_in, n_out, cin, cout, form)
    ws = Guarded(need)
    (ild, ioff), (old, ooff) = lds(cin, form), lds(cout, form)
    xin = strided(n_in, cin, ild, ioff, x)
    go = strided(n_out, cout, old, ooff, gout)
    out = strided(n_out, cout, old, ooff)
    gin = strided(n_in, cin, ild, ioff)
    gw = Guarded(K * cin * cout * 4)
    gb = Guarded(cout * 4)
    rc = lib.pcmi_spconv_fwd(xin.vp, ild, n_in, cin, _vp(Wd), cout, C.byref(m), tr, _vp(bd), out.vp, old, n_out, ws.vp, ws.size, st)
    _ok(lib, rc, tag + " fwd")
    ws.check(tag + " fwd workspace (%d bytes queried)" % need)
    out.check(tag + " fwd out")
    xin.check(tag + " fwd in")
    assert_rows_close(out.cpu(), ref_out, TOL, tag + " out")
    rc = lib.pcmi_spconv_bwd_data(go.vp, old, n_out, cout, _vp(Wd), cin, C.byref(m), tr, gin.vp, ild, n_in, ws.vp, ws.size, st)
    _ok(lib, rc, tag + " bwd_data")
    ws.check(tag + " bwd_data workspace (%d bytes queried)" % need)
    gin.check(tag + " bwd_data gin")
    go.check(tag + " bwd_data gout")
    assert_rows_close(gin.cpu(), ref_gin, TOL, tag + " gin")
    for with_gbias in ((True, False) if also_without_gbias else (True,)):
      t2 = tag + (" bwd_weight" if with_gbias else " bwd_weight (no gbias)")
      gw.buf[gw.lead:gw.lead + gw.nbytes] = 0x7F  # the call overwrites: nothing of an earlier result may survive
      rc = lib.pcmi_spconv_bwd_weight(xin.vp, ild, n_in, cin, go.vp, old, n_out, cout, C.byref(m), tr, gw.vp,
                                      gb.vp if with_gbias else None, ws.vp, ws.size, st)
      _ok(lib, rc, t2)
      ws.check(t2 + " workspace (%d bytes queried)" % need)
      gw.check(t2 + " gW")
      gb.check(t2 + " gbias")
      xin.check(t2 + " in")
      go.check(t2 + " gout")
      assert_slices_close(gw.view(torch.float32, K * cin * cout).view(K, cin, cout).cpu(), ref_gW, TOL, t2 + " gW")
      if with_gbias:
        assert_close(gb.view(torch.float32, cout).cpu(), ref_gb, TOL, t2 + " gbias")


# ------------------------------------------------------------------------------------------------
# A. convolution at every plan edge
# ------------------------------------------------------------------------------------------------
# plan_conv's thresholds: 48 and 96 rows (rows per wave), 512 (PCMI_CONV16 default: the 16-row kernels and
# the split-precision form), 2048 (slice width), 4096 (tile units: the unit-balanced launch), 8192 (slice width; the
# weight gradient's wgrad_x3t), 16384 (the residency-round split).  Every row count keeps the narrow 32 -> 32 pair
# (spconv32r), one wide pair that is eligible for the split-precision kernel, and one pair with an odd N / 32 on one
# side (160 = 5, 96 = 3, 192 = 6, 224 = 7 x 32: the NT = 1 / 3 branches); both neighbours of a threshold run the same
# pairs.
_EDGE_GROUPS = [
    ((47, 48), [(32, 32), (64, 64), (96, 160)]),
    ((95, 96), [(32, 32), (256, 256), (160, 96)]),
    ((511, 512, 513), [(32, 32), (64, 64), (128, 192), (224, 64)]),
    ((2047, 2048), [(32, 32), (256, 256), (224, 64)]),
    ((4095, 4096, 4097), [(32, 32), (64, 64), (96, 160), (128, 192)]),
    ((8191, 8192, 8193), [(32, 32), (256, 256), (160, 96), (128, 192)]),
    ((16383, 16384), [(32, 32), (64, 64), (224, 64), (128, 192)]),
]
EDGE_CASES = [(n, cin, cout) for ns, pairs in _EDGE_GROUPS for n in ns for cin, cout in pairs]


@pytest.mark.parametrize("n,cin,cout", EDGE_CASES)
def test_conv_plan_edges_exact_workspace_strided(lib, n, cin, cout):
  """3^3 hybrid stride-1 convolution with exactly n rows.  The weight gradient of the wide pairs also without gbias: with
  it the launch never takes wgrad_x3t (>= 8192 rows), whose slabs come from the same workspace."""
  _conv_contract(lib, _maps(n), "k3", cin, cout, also_without_gbias=(cin >= 64 and cout >= 64))


# input rows n of coords_with_rows(n) whose stride-2 level has exactly `coarse` rows (found by a CPU search with the
# oracle's CoordsManagerRef.stride; asserted below): one row either side of 48, 96, 512 and 2048 coarse rows
STRIDED_ROWS = [(47, 47), (48, 48), (96, 95), (97, 96), (529, 511), (530, 512), (2331, 2047), (2333, 2048)]


@pytest.mark.parametrize("kind,cin,cout", [("down", 32, 32), ("down", 64, 128), ("up", 32, 32), ("up", 128, 64)])
@pytest.mark.parametrize("n,coarse", STRIDED_ROWS)
def test_strided_conv_plan_edges_exact_workspace_strided(lib, n, coarse, kind, cin, cout):
  """Stride-2 convolution (forward in table form over the coarse rows, backward-data in pair form over the fine rows) and
  its transposed counterpart (the other way round), K = 8, coarse level at a planner threshold."""
  from oracle import sparse_ref as sr
  ref = sr.CoordsManagerRef(coords_with_rows(n))
  assert ref.size(ref.stride(0, 2)) == coarse
  maps = _maps(n)
  m = maps.get(kind)[0]
  assert (m.n_in, m.n_out) == (n, coarse)
  _conv_contract(lib, maps, kind, cin, cout)


@pytest.mark.parametrize("cin,cout", [(48, 20), (40, 72), (96, 13)])
@pytest.mark.parametrize("n", [511, 512, 4096])
def test_padded_width_conv_exact_workspace_strided(lib, n, cin, cout):
  """csrc/widths.hip: channel counts that are no multiples of 32 (the widths of test_spconv_any_width) are staged
  zero-padded in buffers carved from the SAME exact workspace, in front of what the padded problem itself needs."""
  _conv_contract(lib, _maps(n), "k3", cin, cout)


# ------------------------------------------------------------------------------------------------
# B. the workspace query beyond 512 contraction channels
# ------------------------------------------------------------------------------------------------
# (kind, cin, cout, input rows, voxel set, expected output-side rows)
WIDE_CASES = [("k3", 544, 192, 12800, "mid", 12800), ("k3", 192, 544, 12800, "mid", 12800),
              ("down", 768, 128, 21263, "big", 13092), ("up", 128, 768, 21263, "big", 13092)]


@pytest.mark.parametrize("kind,cin,cout,n,base,rows", WIDE_CASES)
def test_workspace_query_covers_contractions_wider_than_512(lib, kind, cin, cout, n, base, rows):
  """The forward / backward-data term of the workspace query (csrc/spconv.hip: spconv_fwd_bwd_workspace) asks plan_conv
  for the offset split at the REAL contraction size, as run_gathered does, so the forward's own term covers these shapes:
  3^3 stride-1 544 -> 192 at 12800 rows, whose forward contracts 544 channels, and its mirror 192 -> 544, whose
  backward-data does; stride-2 768 -> 128 onto 13092 coarse rows and the transposed 128 -> 768 from them.  (It used to
  sample contraction sizes 64..512 and fell short of the planned split here -- 4 partial tensors against 7, 7 against 8 --
  and the query held only through the weight gradient's larger term.)  pcmi_spconv_workspace_bytes is the maximum of that
  term and the weight gradient's slab term (csrc/spconv_wgrad.hip: spconv_wgrad_workspace), and this test holds the
  COMBINED query to its word: every call gets exactly the queried bytes between guard bands;
  tests/test_conv_plan.py holds the query against the plan's own requirement on the CPU.

  Observed on an MI355X (256 CUs, default environment; the smallest ws_bytes each call accepts, found by bisection over
  its PCMI_ERR_WORKSPACE returns):
    3^3 544 -> 192, 12800 rows: forward needs 85 733 376 B (7 partial tensors of 9 830 400 B + 16 920 576 B of packed
      weights), the weight gradient 564 805 632 B, the query is 564 805 888 B;
      192 -> 544: the same 85 733 376 B in backward-data, query 566 247 680 B.
    2^3 stride-2 768 -> 128 onto 13092 rows: forward needs 58 343 424 B (8 partial tensors of 6 703 104 B + 4 718 592 B),
      the weight gradient 57 147 392 B, the query is 164 102 400 B (its chunk-slot bound); transposed 128 -> 768: the
      same 58 343 424 B in backward-data, query 166 723 840 B."""
  maps = _maps(n, base)
  m = maps.get(kind)[0]
  assert rows in (int(m.n_in), int(m.n_out))
  _conv_contract(lib, maps, kind, cin, cout, forms=(0,))


# ------------------------------------------------------------------------------------------------
# C. BatchNorm, elementwise ops, row gather / scatter
# ------------------------------------------------------------------------------------------------
# rows around the one-launch limits of csrc/norm.hip (backward 768, forward 1536) and the lean-statistics switch (65536)
@pytest.mark.parametrize("c", [16, 32, 96, 256])
@pytest.mark.parametrize("n", [768, 769, 1536, 1537, 65536, 65537])
def test_batchnorm_exact_workspace_all_strided(lib, n, c):
  torch.manual_seed(n + c)
  x = torch.randn(n, c) * 2.0 + 0.7
  res, dy = torch.randn(n, c), torch.randn(n, c)
  gamma, beta = torch.rand(c) + 0.5, torch.rand(c) - 0.5
  rm0, rv0 = torch.randn(c), torch.rand(c) + 0.5
  mom, eps = 0.05, 1e-5
  need = lib.pcmi_bn_workspace_bytes(n, c)
  st = _stream()
  gd, bd = _dev(gamma), _dev(beta)
  for fused in (False, True):
    tag = "bn n=%d c=%d %s" % (n, c, "fused" if fused else "plain")
    ws = Guarded(need)
    xs = strided(n, c, c + 4, 4, x)
    rs = strided(n, c, c + 8, 4, res) if fused else None
    ys = strided(n, c, c + 12, 8)
    dys = strided(n, c, c + 16, 12, dy)
    dxs = strided(n, c, c + 20, 16)
    drs = strided(n, c, 2 * c, c) if fused else None
    small = {k: Guarded(c * 4) for k in ("mean", "invstd", "rm", "rv", "dgamma", "dbeta")}
    sv = {k: g.view(torch.float32, c) for k, g in small.items()}
    sv["rm"].copy_(rm0.to(DEV))
    sv["rv"].copy_(rv0.to(DEV))
    rc = lib.pcmi_bn_fwd_train(xs.vp, xs.ld, n, c, _vp(gd), _vp(bd), small["rm"].vp, small["rv"].vp, mom, eps,
                               rs.vp if fused else None, rs.ld if fused else 0, int(fused), ys.vp, ys.ld, small["mean"].vp,
                               small["invstd"].vp, ws.vp, ws.size, st)
    _ok(lib, rc, tag + " fwd_train")
    ws.check(tag + " fwd workspace")
    for k in ("mean", "invstd", "rm", "rv"):
      small[k].check(tag + " fwd " + k)
    ys.check(tag + " y")
    xs.check(tag + " x")
    r = cc.bn_ref64(x, gamma, beta, eps, res if fused else None, fused, dy, relu_mask=(ys.cpu() > 0) if fused else None)
    assert_close(ys.cpu(), r["y"], TOL, tag + " y")
    # the device's ReLU pattern differs from float64's only within the forward tolerance of zero
    assert r["flipped_max"] <= TOL * float(r["y"].abs().max()), tag + ": ReLU pattern differs at |y| = %.3e" % r["flipped_max"]
    assert_close(sv["mean"].cpu(), r["mean"], TOL, tag + " save_mean")
    assert_close(sv["invstd"].cpu(), 1.0 / torch.sqrt(r["var"] + eps), TOL, tag + " save_invstd")
    assert_close(sv["rm"].cpu(), (1 - mom) * rm0.double() + mom * r["mean"], TOL, tag + " running mean")
    assert_close(sv["rv"].cpu(), (1 - mom) * rv0.double() + mom * r["unbiased"], TOL, tag + " running var")
    rc = lib.pcmi_bn_bwd(dys.vp, dys.ld, xs.vp, xs.ld, ys.vp if fused else None, ys.ld if fused else 0, n, c, _vp(gd),
                         small["mean"].vp, small["invstd"].vp, dxs.vp, dxs.ld, drs.vp if fused else None,
                         drs.ld if fused else 0, small["dgamma"].vp, small["dbeta"].vp, ws.vp, ws.size, st)
    _ok(lib, rc, tag + " bwd")
    ws.check(tag + " bwd workspace")
    for k, g in small.items():
      g.check(tag + " bwd " + k)
    for s_, nm in ((dxs, "dx"), (dys, "dy"), (xs, "x"), (ys, "y")) + (((drs, "dres"),) if fused else ()):
      s_.check(tag + " bwd " + nm)
    assert_close(dxs.cpu(), r["dx"], TOL, tag + " dx")
    assert_close(sv["dgamma"].cpu(), r["dgamma"], TOL, tag + " dgamma")
    assert_close(sv["dbeta"].cpu(), r["dbeta"], TOL, tag + " dbeta")
    if fused:
      # the residual gradient is dy under the ReLU mask of the forward output (pcmi.h: relu_mask_y): exactly
      assert torch.equal(drs.cpu(), dy * (ys.cpu() > 0)), tag + " dres"
    # eval mode on the same slices: the running estimates as statistics
    ye = strided(n, c, c + 12, 8)
    rc = lib.pcmi_bn_fwd_eval(xs.vp, xs.ld, n, c, _vp(gd), _vp(bd), small["rm"].vp, small["rv"].vp, eps,
                              rs.vp if fused else None, rs.ld if fused else 0, int(fused), ye.vp, ye.ld, st)
    _ok(lib, rc, tag + " fwd_eval")
    ye.check(tag + " eval y")
    rm1, rv1 = sv["rm"].cpu().double(), sv["rv"].cpu().double()
    want = (x.double() - rm1) / torch.sqrt(rv1 + eps) * gamma.double() + beta.double()
    if fused:
      want = torch.relu(want + res.double())
    assert_close(ye.cpu(), want, 1e-5, tag + " eval y")


@pytest.mark.parametrize("c", [16, 32, 96])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_elementwise_and_row_ops_strided(lib, n, c):
  torch.manual_seed(n * 131 + c)
  a, b = torch.randn(n, c), torch.randn(n, c)
  st = _stream()
  tag = "n=%d c=%d" % (n, c)
  as_, bs = strided(n, c, c + 4, 4, a), strided(n, c, 2 * c, c, b)
  y = strided(n, c, c + 8, 8)
  _ok(lib, lib.pcmi_relu_fwd(as_.vp, as_.ld, n, c, y.vp, y.ld, st), "relu_fwd " + tag)
  y.check("relu_fwd y " + tag)
  assert torch.equal(y.cpu(), torch.relu(a))
  dx = strided(n, c, c + 12, 4)
  _ok(lib, lib.pcmi_relu_bwd(bs.vp, bs.ld, y.vp, y.ld, n, c, dx.vp, dx.ld, st), "relu_bwd " + tag)
  dx.check("relu_bwd dx " + tag)
  assert torch.equal(dx.cpu(), b * (a > 0))
  s = strided(n, c, c + 16, 12)
  _ok(lib, lib.pcmi_add(as_.vp, as_.ld, bs.vp, bs.ld, n, c, s.vp, s.ld, st), "add " + tag)
  s.check("add y " + tag)
  assert torch.equal(s.cpu(), a + b)
  # l2norm: y = x / |x|, dx = (dy - y (y . dy)) / |x|
  yn, dn = strided(n, c, c + 8, 4), strided(n, c, 2 * c, c)
  norm = Guarded(n * 4)
  _ok(lib, lib.pcmi_l2norm_fwd(as_.vp, as_.ld, n, c, yn.vp, yn.ld, norm.vp, st), "l2norm_fwd " + tag)
  yn.check("l2norm_fwd y " + tag)
  norm.check("l2norm_fwd norm " + tag)
  a64 = a.double().requires_grad_(True)
  y64 = a64 / a64.norm(dim=1, keepdim=True)
  y64.backward(b.double())
  assert_close(yn.cpu(), y64.detach(), 1e-6, "l2norm_fwd " + tag)
  assert_close(norm.view(torch.float32, n).cpu(), a.double().norm(dim=1), 1e-6, "l2norm_fwd norm " + tag)
  _ok(lib, lib.pcmi_l2norm_bwd(bs.vp, bs.ld, yn.vp, yn.ld, norm.vp, n, c, dn.vp, dn.ld, st), "l2norm_bwd " + tag)
  dn.check("l2norm_bwd dx " + tag)
  assert_close(dn.cpu(), a64.grad, 1e-5, "l2norm_bwd " + tag)
  for s_ in (as_, bs):
    s_.check("inputs " + tag)
  # gather n_dst rows of the n, then scatter-add them back (duplicates: summed in increasing source-row order)
  n_dst = 2 * n + 3
  idx = torch.randint(0, n, (n_dst,))
  idx_d = _dev(idx)
  gth = strided(n_dst, c, c + 4, 4)
  _ok(lib, lib.pcmi_gather_rows(as_.vp, as_.ld, _vp(idx_d), n_dst, c, gth.vp, gth.ld, st), "gather_rows " + tag)
  gth.check("gather_rows dst " + tag)
  assert torch.equal(gth.cpu(), a[idx])
  acc = strided(n, c, c + 8, 8, torch.zeros(n, c))
  _ok(lib, lib.pcmi_scatter_add_rows(gth.vp, gth.ld, _vp(idx_d), n_dst, c, acc.vp, acc.ld, st), "scatter_add_rows " + tag)
  acc.check("scatter_add_rows dst " + tag)
  assert_close(acc.cpu(), torch.zeros(n, c, dtype=torch.float64).index_add_(0, idx, a[idx].double()), 1e-5, "scatter_add_rows " + tag)


# ------------------------------------------------------------------------------------------------
# C (continued). ops with a workspace and packed operands: a result must not depend on spare workspace
# ------------------------------------------------------------------------------------------------
BIG_WS = 64 << 20


def _twice(need, run):
  """run(ws) -> list of output tensors; once with the exact queried workspace between guard bands, once with 64 MiB:
  bit-identical."""
  assert need <= BIG_WS
  ws = Guarded(need)
  got = [t.clone() for t in run(ws)]
  ws.check("exact workspace of %d bytes" % need)
  big = Guarded(BIG_WS)
  ref = run(big)
  big.check("64 MiB workspace")
  for i, (g, r) in enumerate(zip(got, ref)):
    assert torch.equal(g.view(torch.uint8), r.view(torch.uint8)), "output %d differs between the exact and the 64 MiB workspace" % i
  return got


class _Out:
  """Packed outputs in guarded buffers."""

  def __init__(self):
    self.g = []

  def new(self, dtype, *shape):
    numel = int(np.prod(shape)) if shape else 1
    g = Guarded(max(numel, 1) * torch.empty(0, dtype=dtype).element_size())
    self.g.append(g)
    return g.view(dtype, numel).view(*shape) if shape else g.view(dtype, 1)

  def check(self, what):
    for i, g in enumerate(self.g):
      g.check("%s output %d" % (what, i))


@pytest.mark.parametrize("n,c", [(300, 32), (4097, 32), (1000, 16)])
def test_nce_exact_workspace(lib, n, c):
  torch.manual_seed(n)
  q = torch.nn.functional.normalize(torch.randn(n, c), dim=1)
  k = torch.nn.functional.normalize(q + 0.3 * torch.randn(n, c), dim=1)
  qd, kd, gs = _dev(q), _dev(k), _dev(torch.tensor([1.7]))
  st = _stream()

  def run(ws):
    o = _Out()
    lse, loss, dq, dk = o.new(torch.float32, n), o.new(torch.float32), o.new(torch.float32, n, c), o.new(torch.float32, n, c)
    _ok(lib, lib.pcmi_nce_fwd(_vp(qd), _vp(kd), n, c, 2.5, _vp(lse), _vp(loss), ws.vp, ws.size, st), "nce_fwd")
    _ok(lib, lib.pcmi_nce_bwd(_vp(qd), _vp(kd), _vp(lse), n, c, 2.5, _vp(gs), _vp(dq), _vp(dk), ws.vp, ws.size, st), "nce_bwd")
    o.check("nce n=%d" % n)
    return [lse, loss, dq, dk]

  lse, loss, dq, dk = _twice(lib.pcmi_nce_workspace_bytes(n, c), run)
  q64, k64 = q.double().requires_grad_(True), k.double().requires_grad_(True)
  logits = q64 @ k64.t() * 2.5
  l64 = (torch.logsumexp(logits, 1) - logits.diagonal()).mean()
  (l64 * 1.7).backward()
  assert abs(float(loss) - float(l64)) <= 1e-4 * max(abs(float(l64)), 0.1)  # (test_nce_parity's criteria)
  assert_close(dq.cpu(), q64.grad, TOL, "nce dq")
  assert_close(dk.cpu(), k64.grad, TOL, "nce dk")


@pytest.mark.parametrize("p,s", [(1024, 512), (4097, 1024)])
def test_hardest_loss_exact_workspace(lib, p, s):
  torch.manual_seed(p)
  c = 32
  f0 = torch.nn.functional.normalize(torch.randn(p, c), dim=1)
  f1 = torch.nn.functional.normalize(f0 + 0.2 * torch.randn(p, c), dim=1)
  s0, s1 = torch.nn.functional.normalize(torch.randn(s, c), dim=1), torch.nn.functional.normalize(torch.randn(s, c), dim=1)
  i01, i10 = torch.randint(0, s, (p,), dtype=torch.int32), torch.randint(0, s, (p,), dtype=torch.int32)
  d01 = torch.sqrt(((f0 - s1[i01.long()]) ** 2).sum(1) + 1e-7)
  d10 = torch.sqrt(((f1 - s0[i10.long()]) ** 2).sum(1) + 1e-7)
  m0, m1 = (torch.rand(p) < 0.9).to(torch.uint8), (torch.rand(p) < 0.9).to(torch.uint8)
  dv = [_dev(t) for t in (f0, f1, s0, s1, d01, i01, m0, d10, i10, m1, torch.tensor([1.0, 0.5]))]
  f0d, f1d, s0d, s1d, d01d, i01d, m0d, d10d, i10d, m1d, gl = dv
  st = _stream()

  def run(ws):
    o = _Out()
    losses, stats = o.new(torch.float32, 2), o.new(torch.float32, 8)
    g0, g1, gs0, gs1 = (o.new(torch.float32, p, c), o.new(torch.float32, p, c), o.new(torch.float32, s, c), o.new(torch.float32, s, c))
    gs0.zero_()
    gs1.zero_()
    _ok(lib, lib.pcmi_hardest_loss_fwd(_vp(f0d), _vp(f1d), p, c, _vp(d01d), _vp(m0d), _vp(d10d), _vp(m1d), 0.1, 1.4, _vp(losses),
                                      _vp(stats), ws.vp, ws.size, st), "hardest_loss_fwd")
    _ok(lib, lib.pcmi_hardest_loss_bwd(_vp(f0d), _vp(f1d), p, _vp(s0d), _vp(s1d), c, _vp(d01d), _vp(i01d), _vp(m0d), _vp(d10d),
                                      _vp(i10d), _vp(m1d), 0.1, 1.4, _vp(stats), _vp(gl), _vp(g0), _vp(g1), _vp(gs0), _vp(gs1), st),
        "hardest_loss_bwd")
    o.check("hardest p=%d" % p)
    return [losses, stats[:5], g0, g1, gs0, gs1]

  losses = _twice(lib.pcmi_hardest_workspace_bytes(p), run)[0].cpu()
  pos = torch.relu(((f0.double() - f1.double()) ** 2).sum(1) - 0.1).mean()
  neg = (torch.relu(1.4 - d01.double())[m0.bool()].pow(2).mean() + torch.relu(1.4 - d10.double())[m1.bool()].pow(2).mean()) / 2
  assert abs(float(losses[0]) - float(pos)) <= 1e-4 * abs(float(pos)) + 1e-7  # (test_hardest_loss_parity's criteria)
  assert abs(float(losses[1]) - float(neg)) <= 1e-4 * abs(float(neg))


@pytest.mark.parametrize("n,c", [(1000, 20), (70000, 20)])
def test_softmax_ce_exact_workspace_strided(lib, n, c):
  torch.manual_seed(n)
  x = torch.randn(n, c) * 3
  lb = torch.randint(0, c, (n,))
  lb[torch.rand(n) < 0.2] = 255
  lbd, gl = _dev(lb.to(torch.int32)), _dev(torch.tensor([1.3]))
  xs = strided(n, c, c + 4, 4, x)
  st = _stream()
  keep = []

  def run(ws):
    o = _Out()
    out2 = o.new(torch.float32, 2)
    dl = strided(n, c, c + 12, 8)
    keep.append(dl)
    _ok(lib, lib.pcmi_softmax_ce_fwd(xs.vp, xs.ld, n, c, _vp(lbd), 255, _vp(out2), ws.vp, ws.size, st), "softmax_ce_fwd")
    _ok(lib, lib.pcmi_softmax_ce_bwd(xs.vp, xs.ld, n, c, _vp(lbd), 255, _vp(out2), _vp(gl), dl.vp, dl.ld, st), "softmax_ce_bwd")
    o.check("softmax_ce")
    dl.check("softmax_ce dlogits")
    return [out2, dl.view.contiguous()]

  out2, dl = _twice(lib.pcmi_softmax_ce_workspace_bytes(n), run)
  xs.check("softmax_ce logits")
  x64 = x.double().requires_grad_(True)
  l64 = torch.nn.functional.cross_entropy(x64, lb, ignore_index=255)
  (l64 * 1.3).backward()
  assert abs(float(out2[0]) - float(l64)) <= 1e-5 * abs(float(l64))  # (test_softmax_cross_entropy_with_ignore_label's)
  assert float(out2[1]) == float((lb != 255).sum())
  assert_close(dl.cpu(), x64.grad, 1e-5, "dlogits")


@pytest.mark.parametrize("kind", ["k3", "down"])
@pytest.mark.parametrize("c", [32, 20])
def test_pooling_exact_workspace_strided(lib, kind, c):
  """Average pooling forward / backward (the backward's per-row counts live in the workspace) over a 3^3 stride-1 and a
  2^3 stride-2 map, strided operands; float64 restatement from the exported neighbour table."""
  n = 5000
  maps = _maps(n)
  m, _, n_in, n_out, pin, pout, offs = maps.get(kind)
  torch.manual_seed(c)
  x, go = torch.randn(n_in, c), torch.randn(n_out, c)
  xs, gs = strided(n_in, c, c + 4, 4, x), strided(n_out, c, 2 * c, c, go)
  st = _stream()
  keep = []

  def run(ws):
    out, gin = strided(n_out, c, c + 8, 8), strided(n_in, c, c + 12, 4)
    keep.extend([out, gin])
    _ok(lib, lib.pcmi_pool_fwd(xs.vp, xs.ld, c, C.byref(m), 1, out.vp, out.ld, st), "pool_fwd")
    _ok(lib, lib.pcmi_pool_bwd(gs.vp, gs.ld, c, C.byref(m), 1, gin.vp, gin.ld, ws.vp, ws.size, st), "pool_bwd")
    out.check("pool_fwd out")
    gin.check("pool_bwd gin")
    return [out.view.contiguous(), gin.view.contiguous()]

  out, gin = _twice(lib.pcmi_pool_workspace_bytes(n_out), run)
  xs.check("pool in")
  gs.check("pool gout")
  pi, po = pin.long(), pout.long()
  cnt = torch.zeros(n_out, dtype=torch.float64).index_add_(0, po, torch.ones(len(po), dtype=torch.float64)).clamp_min(1)
  ref = torch.zeros(n_out, c, dtype=torch.float64).index_add_(0, po, x.double()[pi]) / cnt[:, None]
  ref_gin = torch.zeros(n_in, c, dtype=torch.float64).index_add_(0, pi, (go.double() / cnt[:, None])[po])
  assert_close(out.cpu(), ref, 1e-5, "pool_fwd")  # (test_gpu_pooling.py's tolerance for the pooled sums)
  assert_close(gin.cpu(), ref_gin, 1e-5, "pool_bwd")


@pytest.mark.parametrize("c", [32, 20])
def test_segment_ops_exact_workspace_strided(lib, c):
  """Global average pooling and instance norm over the instances (batch indices) of a key: their fp64 chunk partials
  live in the workspace (pcmi_segments_workspace_bytes)."""
  n = 5000
  maps = _maps(n)
  seg = maps.cm.segments(maps.key0)
  ni = int(seg.n_inst)
  inst = torch.from_numpy(coords_with_rows(n)[:, 0].astype(np.int64))
  assert ni == int(inst.max()) + 1
  torch.manual_seed(c + 1)
  x, res, dy, gp = torch.randn(n, c) * 1.5 + 0.3, torch.randn(n, c), torch.randn(n, c), torch.randn(ni, c)
  w, b = torch.rand(c) + 0.5, torch.rand(c) - 0.5
  xs, rs, dys = strided(n, c, c + 4, 4, x), strided(n, c, c + 8, 4, res), strided(n, c, 2 * c, c, dy)
  gps = strided(ni, c, c + 4, 4, gp)
  wd, bd = _dev(w), _dev(b)
  st = _stream()
  keep = []

  def run(ws):
    o = _Out()
    pooled, gin = strided(ni, c, c + 8, 8), strided(n, c, c + 12, 8)
    y, dx, dres = strided(n, c, c + 12, 8), strided(n, c, c + 16, 12), strided(n, c, c + 20, 16)
    mean, invstd, dw, db = o.new(torch.float32, ni, c), o.new(torch.float32, ni, c), o.new(torch.float32, c), o.new(torch.float32, c)
    keep.extend([pooled, gin, y, dx, dres])
    _ok(lib, lib.pcmi_global_pool_fwd(xs.vp, xs.ld, c, C.byref(seg), 1, pooled.vp, pooled.ld, ws.vp, ws.size, st), "global_pool_fwd")
    _ok(lib, lib.pcmi_global_pool_bwd(gps.vp, gps.ld, c, C.byref(seg), 1, gin.vp, gin.ld, st), "global_pool_bwd")
    _ok(lib, lib.pcmi_instnorm_fwd(xs.vp, xs.ld, c, C.byref(seg), _vp(wd), _vp(bd), 1e-5, rs.vp, rs.ld, 1, y.vp, y.ld, _vp(mean),
                                  _vp(invstd), ws.vp, ws.size, st), "instnorm_fwd")
    _ok(lib, lib.pcmi_instnorm_bwd(dys.vp, dys.ld, xs.vp, xs.ld, y.vp, y.ld, c, C.byref(seg), _vp(wd), _vp(mean), _vp(invstd), dx.vp,
                                  dx.ld, dres.vp, dres.ld, _vp(dw), _vp(db), ws.vp, ws.size, st), "instnorm_bwd")
    o.check("segment ops")
    for s_, nm in ((pooled, "pooled"), (gin, "gin"), (y, "y"), (dx, "dx"), (dres, "dres")):
      s_.check("segment ops " + nm)
    return [pooled.view.contiguous(), gin.view.contiguous(), y.view.contiguous(), dx.view.contiguous(), dres.view.contiguous(),
            mean, invstd, dw, db]

  pooled, gin, y, dx, dres, mean, invstd, dw, db = _twice(lib.pcmi_segments_workspace_bytes(C.byref(seg), c), run)
  for s_ in (xs, rs, dys, gps):
    s_.check("segment ops inputs")
  cnt = torch.bincount(inst, minlength=ni).double()
  m64 = torch.zeros(ni, c, dtype=torch.float64).index_add_(0, inst, x.double()) / cnt[:, None]
  assert_close(pooled.cpu(), m64, 1e-5, "global_pool_fwd")
  assert_close(gin.cpu(), (gp.double() / cnt[:, None])[inst], 1e-6, "global_pool_bwd")
  x64, w64, b64 = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
  mu = torch.zeros(ni, c, dtype=torch.float64).index_add(0, inst, x64) / cnt[:, None]
  var = torch.zeros(ni, c, dtype=torch.float64).index_add(0, inst, (x64 - mu[inst]) ** 2) / cnt[:, None]
  pre = (x64 - mu[inst]) / torch.sqrt(var[inst] + 1e-5) * w64 + b64 + res.double()
  mask = y.cpu() > 0  # the device's ReLU pattern (cc.bn_ref64), held to float64's within the forward tolerance of zero
  differ = mask != (pre.detach() > 0)
  assert not bool(differ.any()) or float(pre.detach().abs()[differ].max()) <= TOL * float(pre.detach().abs().max())
  y64 = torch.relu(pre.detach())
  (pre * mask.double()).backward(dy.double())
  # (test_gpu_instance_norm.py's tolerances: 1e-4 against float64)
  assert_close(y.cpu(), y64, TOL, "instnorm y")
  assert_close(dx.cpu(), x64.grad, TOL, "instnorm dx")
  assert_close(dw.cpu(), w64.grad, TOL, "instnorm dweight")
  assert_close(db.cpu(), b64.grad, TOL, "instnorm dbias")
  assert torch.equal(dres.cpu(), dy * (y.cpu() > 0))


@pytest.mark.parametrize("n_queries,npos", [(3000, 1024), (70000, 4096)])
def test_pair_select_exact_workspace(lib, n_queries, npos):
  from oracle import loss_ref as lr
  rng = np.random.RandomState(n_queries)
  counts = rng.randint(1, 30, n_queries)
  q = np.repeat(np.sort(rng.choice(10 * n_queries, n_queries, replace=False)), counts).astype(np.int32)
  pp = torch.from_numpy(np.stack([q, rng.randint(0, 10 * n_queries, len(q)).astype(np.int32)], 1).copy())
  uniform = torch.rand(n_queries, generator=torch.Generator().manual_seed(3))
  sampled = np.random.RandomState(3).choice(n_queries, npos, replace=False)
  ppd, ud, sd = _dev(pp), _dev(uniform), _dev(torch.from_numpy(sampled).long())
  st = _stream()

  def run(ws):
    o = _Out()
    qi, ki = o.new(torch.int64, npos), o.new(torch.int64, npos)
    _ok(lib, lib.pcmi_pair_select(_vp(ppd), len(pp), n_queries, _vp(ud), _vp(sd), npos, _vp(qi), _vp(ki), ws.vp, ws.size, st),
        "pair_select")
    o.check("pair_select")
    return [qi, ki]

  qi, ki = _twice(lib.pcmi_pair_select_workspace_bytes(len(pp)), run)
  qr, kr = lr.nce_select_pairs(pp.numpy(), uniform, sampled)
  assert torch.equal(qi.cpu(), qr) and torch.equal(ki.cpu(), kr)


# ------------------------------------------------------------------------------------------------
# D. contract violations are errors, not faults
# ------------------------------------------------------------------------------------------------
def _refused(lib, rc, code, what):
  assert rc == code, "%s: returned %d, expected %d (%s)" % (what, rc, code, lib.pcmi_last_error().decode())
  assert lib.pcmi_last_error().decode() != "", what + ": no message"
  torch.cuda.synchronize()


def test_conv_contract_violations_are_refused(lib):
  """Arguments include/pcmi.h forbids: refused by a PCMI_REQUIRE before anything is enqueued -- an error code, a message,
  and no byte of an output, a workspace or a guard band written.  511 rows, 64 -> 64, 3^3: the launches split their
  offsets (partial sums in the workspace) and the weight gradient writes slabs, so every call needs its workspace."""
  n, cin, cout = 511, 64, 64
  m, tr, n_in, n_out, pin, pout, offs = _maps(n).get("k3")
  K = m.K
  x, W, bias, gout = _conv_inputs(n, n, cin, cout, K, 1)
  Wd = _dev(W)
  need = lib.pcmi_spconv_workspace_bytes(n, n, cin, cout, K, m.M)
  st = _stream()
  ws = Guarded(need)
  xin, go = strided(n, cin, cin + 32, 4, x), strided(n, cout, cout + 32, 4, gout)
  out, gin = strided(n, cout, cout + 32, 4), strided(n, cin, cin + 32, 4)
  gw = Guarded(K * cin * cout * 4)
  mp = C.byref(m)

  def fwd(in_p=xin.vp, in_ld=xin.ld, out_p=out.vp, out_ld=out.ld, w=ws.vp, wb=ws.size):
    return lib.pcmi_spconv_fwd(in_p, in_ld, n, cin, _vp(Wd), cout, mp, 0, None, out_p, out_ld, n, w, wb, st)

  def bwd(g_p=go.vp, g_ld=go.ld, gin_p=gin.vp, gin_ld=gin.ld, w=ws.vp, wb=ws.size):
    return lib.pcmi_spconv_bwd_data(g_p, g_ld, n, cout, _vp(Wd), cin, mp, 0, gin_p, gin_ld, n, w, wb, st)

  def wgr(in_p=xin.vp, in_ld=xin.ld, g_p=go.vp, g_ld=go.ld, w=ws.vp, wb=ws.size):
    return lib.pcmi_spconv_bwd_weight(in_p, in_ld, n, cin, g_p, g_ld, n, cout, mp, 0, gw.vp, None, w, wb, st)

  off4 = lambda s: C.c_void_p(s.view.data_ptr() + 4)
  cases = [
      ("fwd: ws = NULL", fwd(w=None), PCMI_ERR_WORKSPACE),
      ("fwd: ws_bytes = 256", fwd(wb=C.c_size_t(256)), PCMI_ERR_WORKSPACE),
      ("fwd: in_ld % 4 != 0", fwd(in_ld=xin.ld - 2), PCMI_ERR_INVALID),
      ("fwd: in offset by 4 bytes", fwd(in_p=off4(xin)), PCMI_ERR_INVALID),
      ("fwd: out_ld < cout", fwd(out_ld=cout - 4), PCMI_ERR_INVALID),
      ("fwd: out_ld % 4 != 0", fwd(out_ld=out.ld - 2), PCMI_ERR_INVALID),
      ("fwd: out offset by 4 bytes", fwd(out_p=off4(out)), PCMI_ERR_INVALID),
      ("bwd_data: ws = NULL", bwd(w=None), PCMI_ERR_WORKSPACE),
      ("bwd_data: ws_bytes = 256", bwd(wb=C.c_size_t(256)), PCMI_ERR_WORKSPACE),
      ("bwd_data: gout_ld % 4 != 0", bwd(g_ld=go.ld - 2), PCMI_ERR_INVALID),
      ("bwd_data: gout offset by 4 bytes", bwd(g_p=off4(go)), PCMI_ERR_INVALID),
      ("bwd_data: gin_ld < cin", bwd(gin_ld=cin - 4), PCMI_ERR_INVALID),
      ("bwd_weight: ws = NULL", wgr(w=None), PCMI_ERR_WORKSPACE),
      ("bwd_weight: ws_bytes = 256", wgr(wb=C.c_size_t(256)), PCMI_ERR_WORKSPACE),
      ("bwd_weight: in_ld % 4 != 0", wgr(in_ld=xin.ld - 2), PCMI_ERR_INVALID),
      ("bwd_weight: gout offset by 4 bytes", wgr(g_p=off4(go)), PCMI_ERR_INVALID),
  ]
  for what, rc, code in cases:
    _refused(lib, rc, code, what)
  ws.check("refused calls: workspace bands")
  assert bool((ws.buf == cc.GUARD_BYTE).all()), "a refused call wrote into the workspace"
  assert bool((gw.buf == cc.GUARD_BYTE).all()), "a refused call wrote into gW"
  assert out.untouched() and gin.untouched(), "a refused call wrote into an output"
  for s_ in (xin, go, out, gin):
    s_.check("refused calls")
  # and the same arguments, valid, are accepted
  _ok(lib, fwd(), "fwd")
  _ok(lib, bwd(), "bwd_data")
  _ok(lib, wgr(), "bwd_weight")
  ws.check("accepted calls")


def test_workspace_one_byte_short_is_refused(lib):
  """Ops whose requirement IS their query: one byte less is PCMI_ERR_WORKSPACE, nothing written."""
  st = _stream()
  n, c = 5000, 32
  torch.manual_seed(0)
  x = torch.randn(n, c)
  xs, y = strided(n, c, c + 4, 4, x), strided(n, c, c + 8, 8)
  gam = _dev(torch.ones(c))
  o = _Out()
  mean, invstd, dg, db = (o.new(torch.float32, c) for _ in range(4))
  need = lib.pcmi_bn_workspace_bytes(n, c)
  ws = Guarded(need)
  short = C.c_size_t(need - 1)
  rc = lib.pcmi_bn_fwd_train(xs.vp, xs.ld, n, c, _vp(gam), _vp(gam), None, None, 0.05, 1e-5, None, 0, 0, y.vp, y.ld, _vp(mean),
                             _vp(invstd), ws.vp, short, st)
  _refused(lib, rc, PCMI_ERR_WORKSPACE, "bn_fwd_train: one byte short")
  rc = lib.pcmi_bn_bwd(xs.vp, xs.ld, xs.vp, xs.ld, None, 0, n, c, _vp(gam), _vp(gam), _vp(gam), y.vp, y.ld, None, 0, _vp(dg), _vp(db),
                       ws.vp, short, st)
  _refused(lib, rc, PCMI_ERR_WORKSPACE, "bn_bwd: one byte short")
  rc = lib.pcmi_bn_fwd_train(xs.vp, xs.ld, n, c, _vp(gam), _vp(gam), None, None, 0.05, 1e-5, None, 0, 0, y.vp, y.ld, _vp(mean),
                             _vp(invstd), None, C.c_size_t(need), st)
  _refused(lib, rc, PCMI_ERR_WORKSPACE, "bn_fwd_train: ws = NULL")
  assert y.untouched() and bool((ws.buf == cc.GUARD_BYTE).all())
  for g in o.g:
    assert bool((g.buf == cc.GUARD_BYTE).all()), "a refused BatchNorm call wrote a statistic"
  # nce / softmax cross-entropy / pair selection / average-pooling backward
  q = _dev(torch.nn.functional.normalize(torch.randn(300, 32), dim=1))
  o2 = _Out()
  lse, loss, out2 = o2.new(torch.float32, 300), o2.new(torch.float32), o2.new(torch.float32, 2)
  qi, ki = o2.new(torch.int64, 64), o2.new(torch.int64, 64)
  need = lib.pcmi_nce_workspace_bytes(300, 32)
  w2 = Guarded(need)
  _refused(lib, lib.pcmi_nce_fwd(_vp(q), _vp(q), 300, 32, 2.5, _vp(lse), _vp(loss), w2.vp, C.c_size_t(need - 1), st),
           PCMI_ERR_WORKSPACE, "nce_fwd: one byte short")
  lb = _dev(torch.zeros(n, dtype=torch.int32))
  need = lib.pcmi_softmax_ce_workspace_bytes(n)
  _refused(lib, lib.pcmi_softmax_ce_fwd(xs.vp, xs.ld, n, c, _vp(lb), 255, _vp(out2), w2.vp, C.c_size_t(need - 1), st),
           PCMI_ERR_WORKSPACE, "softmax_ce_fwd: one byte short")
  pairs = _dev(torch.stack([torch.arange(64, dtype=torch.int32), torch.arange(64, dtype=torch.int32)], 1))
  need = lib.pcmi_pair_select_workspace_bytes(64)
  _refused(lib, lib.pcmi_pair_select(_vp(pairs), 64, 64, _vp(_dev(torch.rand(64))), None, 64, _vp(qi), _vp(ki), w2.vp,
                                     C.c_size_t(need - 1), st), PCMI_ERR_WORKSPACE, "pair_select: one byte short")
  m = _maps(n).get("k3")[0]
  need = lib.pcmi_pool_workspace_bytes(n)
  _refused(lib, lib.pcmi_pool_bwd(xs.vp, xs.ld, c, C.byref(m), 1, y.vp, y.ld, w2.vp, C.c_size_t(need - 1), st), PCMI_ERR_WORKSPACE,
           "pool_bwd (average): one byte short")
  assert y.untouched() and bool((w2.buf == cc.GUARD_BYTE).all())
  for g in o2.g:
    assert bool((g.buf == cc.GUARD_BYTE).all()), "a refused call wrote an output"


def test_elementwise_contract_violations_are_refused(lib):
  st = _stream()
  n, c = 65, 32
  x = strided(n, c, c + 8, 4, torch.randn(n, c))
  y = strided(n, c, c + 8, 4)
  idx = _dev(torch.arange(n))
  off4 = lambda s: C.c_void_p(s.view.data_ptr() + 4)
  cases = [
      ("relu_fwd: y_ld % 4 != 0", lib.pcmi_relu_fwd(x.vp, x.ld, n, c, y.vp, y.ld - 2, st)),
      ("relu_fwd: y_ld < c", lib.pcmi_relu_fwd(x.vp, x.ld, n, c, y.vp, c - 4, st)),
      ("relu_fwd: x offset by 4 bytes", lib.pcmi_relu_fwd(off4(x), x.ld, n, c, y.vp, y.ld, st)),
      ("relu_fwd: y offset by 4 bytes", lib.pcmi_relu_fwd(x.vp, x.ld, n, c, off4(y), y.ld, st)),
      ("relu_bwd: dx_ld % 4 != 0", lib.pcmi_relu_bwd(x.vp, x.ld, x.vp, x.ld, n, c, y.vp, y.ld - 2, st)),
      ("add: b offset by 4 bytes", lib.pcmi_add(x.vp, x.ld, off4(x), x.ld, n, c, y.vp, y.ld, st)),
      ("add: c % 4 != 0", lib.pcmi_add(x.vp, x.ld, x.vp, x.ld, n, c - 2, y.vp, y.ld, st)),
      ("l2norm_fwd: norm = NULL", lib.pcmi_l2norm_fwd(x.vp, x.ld, n, c, y.vp, y.ld, None, st)),
      ("l2norm_bwd: dx_ld < c", lib.pcmi_l2norm_bwd(x.vp, x.ld, x.vp, x.ld, _vp(idx), n, c, y.vp, c - 4, st)),
      ("bn_fwd_eval: y_ld % 4 != 0", lib.pcmi_bn_fwd_eval(x.vp, x.ld, n, c, _vp(idx), _vp(idx), _vp(idx), _vp(idx), 1e-5, None, 0, 0,
                                                          y.vp, y.ld - 2, st)),
      ("gather_rows: dst_ld % 4 != 0", lib.pcmi_gather_rows(x.vp, x.ld, _vp(idx), n, c, y.vp, y.ld - 2, st)),
      ("gather_rows: dst offset by 4 bytes", lib.pcmi_gather_rows(x.vp, x.ld, _vp(idx), n, c, off4(y), y.ld, st)),
  ]
  for what, rc in cases:
    _refused(lib, rc, PCMI_ERR_INVALID, what)
  assert y.untouched(), "a refused call wrote into its output"
  y.check("refused calls")
  x.check("refused calls")
