"""wgrad_x3p_kernel with the G rows staged by its multiplying waves (csrc/spconv_wgrad_x3.hip; pytest -m gpu, MI355X).

The producer / consumer form of the tile-stationary weight gradient (PCMI_WGRAD_X3P=1) must keep computing exactly what
the one-role form (wgrad_x3t_kernel, PCMI_WGRAD_X3P=0) computes: the same cells, fragments, products and slabs.  Every
case goes through pcmi_spconv_bwd_weight with PCMI_WGRAD_X3T=1, which sends every size to that kernel family:

  rows      65 and 200 (one ragged tile in one or two row blocks), 945 (15 tiles: seven row blocks of two tiles and a
            last one of ONE ragged tile), 1212 (a solid cube and then an isolated lattice, in that order: tiles with all
            27 offsets followed by tiles with the centre offset alone, so whole slots and whole offset groups are
            absent; three tiles per row block), 4096 (the map carries the sorted order; four or eight tiles per row
            block, the steady state of the staging schedule);
  channels  96 -> 96, 128 -> 96, 64 -> 64, 192 -> 128: the four <MTW, NTW> instances;
  operands  a wide dynamic range, as test_wgrad_x3t_split_precision_matches_fp64;
  dense     the K = 1 form (no map, identity table) at 128 -> 96.

(a) the two forms are BIT-EQUAL wherever they take the same number of row blocks (wgrad_x3t_rb: one resident workgroup
per CU for the producer / consumer form, two for the other -- restated in _row_blocks); where they do not, the slab sums
associate differently and both are held to a float64 contraction at the bounds of
test_wgrad_x3t_split_precision_matches_fp64.  (b) two runs are bit-identical.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import geometry_cases as gc
from c_contract import DEV
from test_gpu_c_contract import _Maps, _ok, _stream, _vp, rel_err
from test_gpu_wgrad_plan import _planned

pytestmark = pytest.mark.gpu

CLOUDS = {
    "solid65": (gc.solid, (5, 13, 1, 1, (-2, -6, 0))),
    "solid200": (gc.solid, (5, 5, 8, 1, (-2, -2, -4))),
    "solid945": (gc.solid, (7, 9, 15, 1, (-3, -4, -7))),
    "cube_then_lattice1212": (gc.mixed, (8, 700, False)),
    "solid4096": (gc.solid, (16, 16, 16, 1, (-8, -8, -8))),
}
ROWS = {"solid65": 65, "solid200": 200, "solid945": 945, "cube_then_lattice1212": 1212, "solid4096": 4096}
CHANNELS = [(96, 96), (128, 96), (64, 64), (192, 128)]

_CLOUD = {}


@pytest.fixture(scope="module")
def lib():
  from pointcontrast_amd import _lib
  return _lib.lib


def _cloud(name):
  """(map, nbr [27, n] on the device) of a named cloud; one coordinate manager alive at a time (cases ordered by cloud)."""
  if name not in _CLOUD:
    _CLOUD.clear()
    fn, args = CLOUDS[name]
    coords = fn(*args)
    assert len(coords) == ROWS[name]
    maps = _Maps(len(coords), coords=coords)
    m = maps.cm.kernel_map(maps.key0, maps.key0, 3, 1, 3)
    _CLOUD[name] = (maps, m, maps.cm.export_map(m)[0].long())
  return _CLOUD[name][1:]


def _tw(c):
  return 3 if c % 96 == 0 else 2


def _row_blocks(n_rows, cin, cout, per_cu, K):
  """wgrad_x3t_rb of csrc/spconv_wgrad_plan.h restated; _check holds pcmi_spconv_wgrad_plan to it."""
  gy, gz = cin // (32 * _tw(cin)), cout // (32 * _tw(cout))
  n_cu = torch.cuda.get_device_properties(DEV).multi_processor_count
  rb = per_cu * n_cu // (-(-K // 4) * gy * gz)
  rb = min(rb, -(-n_rows // 64) // 4)
  return max(8, min(128, rb // 8 * 8))


def _operands(n, cin, cout, seed):
  g_ = torch.Generator(device=DEV).manual_seed(seed)
  x = torch.randn(n, cin, device=DEV, generator=g_) * torch.exp(torch.randn(n, 1, device=DEV, generator=g_))
  g = torch.randn(n, cout, device=DEV, generator=g_) * torch.exp(0.5 * torch.randn(n, 1, device=DEV, generator=g_))
  return x, g


def _bwd_weight(lib, monkeypatch, x, g, m, K, x3t, x3p):
  monkeypatch.setenv("PCMI_WGRAD_X3T", x3t)
  monkeypatch.setenv("PCMI_WGRAD_X3P", x3p)
  n, cin, cout = x.shape[0], x.shape[1], g.shape[1]
  need = lib.pcmi_spconv_workspace_bytes(n, n, cin, cout, K, m.M if m is not None else n)
  ws = torch.empty(max(int(need), 16), dtype=torch.uint8, device=DEV)
  gw = torch.full((K, cin, cout), float("nan"), device=DEV)
  rc = lib.pcmi_spconv_bwd_weight(_vp(x), cin, n, cin, _vp(g), cout, n, cout, C.byref(m) if m is not None else None, 0, _vp(gw), None,
                                  _vp(ws), C.c_size_t(int(need)), _stream())
  _ok(lib, rc, "bwd_weight %d rows %d->%d K=%d X3T=%s X3P=%s" % (n, cin, cout, K, x3t, x3p))
  assert bool(torch.isfinite(gw).all()), "an element of gW was not written"
  return gw


def _bits(t):
  return t.contiguous().view(torch.int32)


def _check(lib, monkeypatch, x, g, m, K, g64_fn, what):
  n, cin, cout = x.shape[0], x.shape[1], g.shape[1]
  p1 = _bwd_weight(lib, monkeypatch, x, g, m, K, "1", "1")
  p2 = _bwd_weight(lib, monkeypatch, x, g, m, K, "1", "1")
  t1 = _bwd_weight(lib, monkeypatch, x, g, m, K, "1", "0")
  pair = _bwd_weight(lib, monkeypatch, x, g, m, K, "0", "1")  # the fp32 pair-list kernel
  assert not torch.equal(pair, p1) and not torch.equal(pair, t1), what + ": PCMI_WGRAD_X3T did not switch kernels"
  assert torch.equal(_bits(p1), _bits(p2)), what + ": two runs of the producer / consumer form differ"
  rb_p, rb_t = _row_blocks(n, cin, cout, 1, K), _row_blocks(n, cin, cout, 2, K)
  for x3p, kernel, rb in (("1", 1, rb_p), ("0", 2, rb_t)):  # PCMI_WGRAD_KERNEL_X3P / _X3T: the library plans the same row blocks
    monkeypatch.setenv("PCMI_WGRAD_X3T", "1")
    monkeypatch.setenv("PCMI_WGRAD_X3P", x3p)
    plan = _planned(lib, m, n, n, cin, cout, False, cin, cout)
    assert (plan[0], plan[7]) == (kernel, rb), "%s: PCMI_WGRAD_X3P=%s planned %s, restated %d row blocks" % (what, x3p, plan, rb)
  print("%s: row blocks %d (producer / consumer) and %d (one role)" % (what, rb_p, rb_t))
  if rb_p == rb_t:
    assert torch.equal(_bits(p1), _bits(t1)), what + ": the two forms differ at the same row-block count (%d)" % rb_p
    return
  g64 = g64_fn()
  e = {"fp32": rel_err(pair, g64), "x3p": rel_err(p1, g64), "x3t": rel_err(t1, g64)}
  print("%s: errors vs float64 %s" % (what, {k: "%.2e" % v for k, v in e.items()}))
  assert e["fp32"] <= 1e-5, "fp32 kernel vs float64: %s %s" % (what, e)
  for form, r in (("x3p", p1), ("x3t", t1)):
    assert e[form] <= max(4 * e["fp32"], 2e-6), "%s vs float64: %s %s" % (form, what, e)
    for k in range(K):  # every offset slice on its own scale
      assert rel_err(r[k], g64[k]) <= 1e-5, "%s offset %d: %s" % (form, k, what)


@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("name", list(CLOUDS))
def test_consumer_staged_g_equals_the_one_role_kernel(lib, name, cin, cout, monkeypatch):
  m, nbr = _cloud(name)
  n = ROWS[name]
  x, g = _operands(n, cin, cout, 1000 * cin + cout + n)

  def g64():
    out = torch.zeros(27, cin, cout, dtype=torch.float64, device=DEV)
    for k in range(27):
      ok = nbr[k] >= 0
      out[k] = x[nbr[k][ok]].double().t() @ g[ok].double()
    return out

  _check(lib, monkeypatch, x, g, m, 27, g64, "%s %d->%d" % (name, cin, cout))


@pytest.mark.parametrize("n", [65, 945, 3000])
def test_consumer_staged_g_dense_form(lib, n, monkeypatch):
  cin, cout = 128, 96
  x, g = _operands(n, cin, cout, n)
  _check(lib, monkeypatch, x, g, None, 1, lambda: (x.double().t() @ g.double())[None], "1x1 %d rows %d->%d" % (n, cin, cout))
