"""pcmi_spconv_wgrad_plan reports what pcmi_spconv_bwd_weight does (pytest -m gpu, on a real MI355X).

One weight gradient per kernel family and mode of plan_wgrad (csrc/spconv_wgrad_plan.h), each at the smallest row count
at which the planner -- asked on the CPU beforehand, tests/test_wgrad_plan.py's helpers, at every count from 1 -- first
gives that answer (or, where it gives it from the first row, at the smallest count the contract tests use):

  rows  channels  what                                    the threshold it sits on
    47  32 -> 32  pair list, direct (with gbias)          none below: direct from the first row; test_gpu_c_contract.py's smallest
   257  64 -> 64  pair list, arrive                       kWgradMinChunk = 256 pairs per chunk: the first second chunk slot of an offset
  2049  64 -> 64  pair list, slabs + wgrad_reduce_kernel  kArriveMax = 8 chunk slots per offset x 256: the ninth
  8192  64 -> 64  producer / consumer (fp32 precision),   PCMI_WGRAD_X3T's default
                  one role (bf16 precision, and PCMI_WGRAD_X3P=0)
  8192  64 -> 64  dense 1x1, producer / consumer          the same
   100   3 -> 32  both stem forms (without / with gbias)  none: from the first row; the stem's smallest case elsewhere

Each case asks the plan with slots_per_cu = 0 (the runtime's answer, as the launch takes it), then calls
pcmi_spconv_bwd_weight with EXACTLY ws_bytes between guard bands and strided operands, and holds gW (per offset slice)
and gbias to test_gpu_c_contract.py's TOL against its float64 reference.  With one byte less the call must return
PCMI_ERR_WORKSPACE and leave gW as it was.  In the bf16 precision the operands are bf16 numbers to begin with, so that
the one product per chunk of that mode is exact and the same reference and TOL hold."""
import ctypes as C

import pytest
import torch

from c_contract import PCMI_ERR_WORKSPACE, Guarded, conv_ref64, lds, strided
from test_gpu_c_contract import TOL, _conv_inputs, _maps, _ok, _stream, assert_close, assert_slices_close
from test_wgrad_plan import ARRIVE, DIRECT, MAP_NBR, MAP_PERM, NONE, PAIRS, SLABS, STEM, STEM_MFMA, X3P, X3T

pytestmark = pytest.mark.gpu

FP32, BF16 = 0, 1  # include/pcmi.h: PCMI_CONV_PRECISION_*
# (id, map or None, rows, cin, cout, gbias, environment, precision, kernel, mode or None); ordered by rows: one manager alive
CASES = [
    ("direct", "k3", 47, 32, 32, True, {}, FP32, PAIRS, DIRECT),
    ("stem_mfma", "k3", 100, 3, 32, False, {}, FP32, STEM_MFMA, None),
    ("stem_pairs", "k3", 100, 3, 32, True, {}, FP32, STEM, SLABS),
    ("arrive", "k3", 257, 64, 64, False, {}, FP32, PAIRS, ARRIVE),
    ("slabs", "k3", 2049, 64, 64, False, {}, FP32, PAIRS, SLABS),
    ("producer_consumer", "k3", 8192, 64, 64, False, {}, FP32, X3P, None),
    ("one_role_bf16", "k3", 8192, 64, 64, False, {}, BF16, X3T, None),
    ("one_role_fp32", "k3", 8192, 64, 64, False, {"PCMI_WGRAD_X3P": "0"}, FP32, X3T, None),
    ("dense_producer_consumer", None, 8192, 64, 64, False, {}, FP32, X3P, None),
]


@pytest.fixture(scope="module")
def lib():
  from pointcontrast_amd import _lib
  return _lib.lib


@pytest.fixture
def precision(lib):
  yield lambda p: lib.pcmi_set_conv_precision(p)
  lib.pcmi_set_conv_precision(FP32)


def _planned(lib, m, n_in, n_out, cin, cout, gbias, in_ld, gout_ld):
  """(kernel, tile_c, tile_n, chunk, slots_per_offset, mode, address_bits, row_blocks, groupable, ws_bytes) of the call."""
  o = [C.c_int() for _ in range(9)]
  ws = C.c_size_t()
  if m is None:
    K, ks, stride, tables, cnt = 1, 0, 0, 0, None
  else:
    K, ks, stride = m.K, m.kernel_size, m.stride
    tables = (MAP_NBR if m.nbr else 0) | (MAP_PERM if m.perm and m.nbr_perm else 0)
    cnt = (C.c_int64 * (K + 1))(*m.offs_host[:K + 1]) if m.M >= 0 else None
  rc = lib.pcmi_spconv_wgrad_plan(n_in, n_out, cin, cout, K, ks, stride, tables, 0, int(gbias), 0, n_in * in_ld * 4, n_out * gout_ld * 4, 1, cnt,
                                  0, *[C.byref(v) for v in o], C.byref(ws))
  assert rc == 0, lib.pcmi_last_error().decode()
  return tuple(v.value for v in o) + (ws.value,)


@pytest.mark.parametrize("name,kind,n,cin,cout,gbias,env,prec,kernel,mode", CASES, ids=[c[0] for c in CASES])
def test_reported_plan_is_what_the_launch_does(lib, monkeypatch, precision, name, kind, n, cin, cout, gbias, env, prec, kernel, mode):
  for k, v in env.items():
    monkeypatch.setenv(k, v)
  precision(prec)
  if kind is None:
    m, K = None, 1
    pin = pout = torch.arange(n)
    offs = [0, n]
  else:
    m, _, _, _, pin, pout, offs = _maps(n).get(kind)
    K = m.K
  x, _, _, gout = _conv_inputs(n, n, cin, cout, K, 17 + n)
  if prec == BF16:
    x, gout = x.bfloat16().float(), gout.bfloat16().float()
  W0 = torch.zeros(K, cin, cout)
  _, _, ref_gW, ref_gb = conv_ref64(x, W0, pin, pout, offs, n, gout=gout)
  (ild, ioff), (old, ooff) = lds(cin, 0), lds(cout, 1)
  plan = _planned(lib, m, n, n, cin, cout, gbias, ild, old)
  print("%s: plan %s" % (name, plan))
  assert plan[0] == kernel and (mode is None or plan[5] == mode), "%s: planned %s" % (name, plan)
  need = plan[-1]
  assert need <= lib.pcmi_spconv_workspace_bytes(n, n, cin, cout, K, m.M if m is not None else n)
  xin, go = strided(n, cin, ild, ioff, x), strided(n, cout, old, ooff, gout)
  gw, gb = Guarded(K * cin * cout * 4), Guarded(cout * 4)
  mp = C.byref(m) if m is not None else None

  def call(ws):
    gw.buf[gw.lead:gw.lead + gw.nbytes] = 0x7F  # the call overwrites: nothing of an earlier result may survive
    return lib.pcmi_spconv_bwd_weight(xin.vp, ild, n, cin, go.vp, old, n, cout, mp, 0, gw.vp, gb.vp if gbias else None, ws.vp, ws.size, _stream())

  ws = Guarded(need)
  _ok(lib, call(ws), name)
  for g, what in ((ws, "workspace (%d bytes planned)" % need), (gw, "gW"), (gb, "gbias"), (xin, "in"), (go, "gout")):
    g.check("%s %s" % (name, what))
  assert_slices_close(gw.view(torch.float32, K * cin * cout).view(K, cin, cout).cpu(), ref_gW, TOL, name + " gW")
  if gbias:
    assert_close(gb.view(torch.float32, cout).cpu(), ref_gb, TOL, name + " gbias")
  assert need > 0
  short = Guarded(need - 1)
  assert call(short) == PCMI_ERR_WORKSPACE, "%s: accepted %d bytes where the plan says %d" % (name, need - 1, need)
  torch.cuda.synchronize()
  assert bool((gw.buf[gw.lead:gw.lead + gw.nbytes] == 0x7F).all()), name + ": a refused call wrote gW"
  short.check(name + " refused call's workspace")


def test_map_without_pairs_is_planned_and_run_as_nothing(lib):
  """PCMI_WGRAD_KERNEL_NONE: a map whose counts say it has no pairs -- gW is zeroed, no workspace is asked."""
  m0 = _maps(47).get("k3")[0]
  m = type(m0).from_buffer_copy(m0)
  m.M = 0
  for k in range(m.K + 1):
    m.offs_host[k] = 0
  n, cin, cout = 47, 32, 32
  assert _planned(lib, m, n, n, cin, cout, False, cin, cout) == (NONE, 0, 0, 0, 0, 0, 0, 0, 0, 0)
  x, _, _, gout = _conv_inputs(n, n, cin, cout, m.K, 3)
  xin, go = strided(n, cin, cin, 0, x), strided(n, cout, cout, 0, gout)
  gw = Guarded(m.K * cin * cout * 4)
  gw.buf[gw.lead:gw.lead + gw.nbytes] = 0x7F
  rc = lib.pcmi_spconv_bwd_weight(xin.vp, cin, n, cin, go.vp, cout, n, cout, C.byref(m), 0, gw.vp, None, None, C.c_size_t(0), _stream())
  _ok(lib, rc, "no pairs")
  gw.check("no pairs gW")
  assert bool((gw.view(torch.float32, m.K * cin * cout) == 0).all())
