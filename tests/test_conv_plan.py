"""The plan of the gathered convolution launches (csrc/spconv_plan.h: plan_conv, reported by pcmi_spconv_plan), on the CPU.

tests/golden/conv_plans_cu256.json holds what run_gathered decided -- kernel, row tile, slice width, offset split and the
smallest workspace it accepted -- at the commit before those decisions were gathered into plan_conv, recorded there from
run_gathered itself (made to log and return in front of its launches) for 256 compute units: every (n, cin, cout) of
test_gpu_c_contract.py's EDGE_CASES, STRIDED_ROWS and WIDE_CASES and test_gpu_conv_geometry.py's SK_CASES, forward and
backward-data, each with a packed operand and one of at least 2 GiB, under the default environment and each planner
switch alone.  The planner must reproduce every line, and the workspace query must cover every plan.  Without a GPU the
library counts 256 compute units (csrc/internal.h: num_cu), as the MI355X has."""
import ctypes as C
import json
import os

import pytest

SWITCHES = ("PCMI_SPCONV_STREAMK", "PCMI_CONV16", "PCMI_CONV16_X3", "PCMI_CONV32R")
ENVS = [{}, {"PCMI_CONV16": "0"}, {"PCMI_CONV16": "8192"}, {"PCMI_CONV16_X3": "0"}, {"PCMI_SPCONV_STREAMK": "0"}, {"PCMI_CONV32R": "0"}]
NONE, TABLE, UNITS, PAIRS = range(4)  # include/pcmi.h: PCMI_CONV_FORM_*
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plans_cu256.json")


@pytest.fixture(scope="module")
def lib(built_lib):
  from pointcontrast_amd import _lib
  return _lib.lib


def _setenv(monkeypatch, env):
  for k in SWITCHES:
    monkeypatch.delenv(k, raising=False)
  for k, v in env.items():
    monkeypatch.setenv(k, v)


def _plan(lib, rows, x_bytes, c, n, k, form):
  kernel, rw, nt, ks, ws = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
  rc = lib.pcmi_spconv_plan(rows, x_bytes, c, n, k, form, C.byref(kernel), C.byref(rw), C.byref(nt), C.byref(ks), C.byref(ws))
  assert rc == 0, (rc, lib.pcmi_last_error().decode())
  return kernel.value, rw.value, nt.value, ks.value, ws.value


def test_golden_table_covers_what_it_claims():
  g = json.load(open(GOLDEN))
  assert g["compute_units"] == 256
  envs = [p["env"] for p in g["plans"]]
  for e in ENVS:
    assert e in envs
  rows = [dict(zip(g["fields"], r)) for p in g["plans"] for r in p["rows"]]
  assert sorted({r["kernel"] for r in rows}) == list(range(8))  # every kernel family is planned somewhere
  assert any(r["x_bytes"] > 0x7FFFFF00 for r in rows) and any(r["x_bytes"] <= 0x7FFFFF00 for r in rows)
  assert {r["form"] for r in rows} == {TABLE, UNITS, PAIRS}


def test_planner_reproduces_recorded_decisions_and_query_covers_them(lib, monkeypatch):
  g = json.load(open(GOLDEN))
  n = 0
  for p in g["plans"]:
    _setenv(monkeypatch, p["env"])
    for row in p["rows"]:
      r = dict(zip(g["fields"], row))
      got = _plan(lib, r["rows"], r["x_bytes"], r["C"], r["N"], r["K"], r["form"])
      want = (r["kernel"], r["rows_per_wave"], r["slice"], r["ksplit"], r["ws_bytes"])
      assert got == want, "%s %s: planned %s, recorded %s" % (p["env"], r, got, want)
      query = lib.pcmi_spconv_workspace_bytes(r["n_in"], r["n_out"], r["cin"], r["cout"], r["K"], max(r["n_in"], r["n_out"]))
      assert query >= r["ws_bytes"], "%s %s: the query gives %d bytes" % (p["env"], r, query)
      n += 1
  assert n > 3000


# every row count at which plan_conv changes its answer (48, 96: the row tile; 512: PCMI_CONV16's default; 2048, 8192: the
# slice width; 4096: tile units; 8192: spconv32r; 16384: the residency-round split; 32768 = 256 tiles: the unit-balanced
# launch), one either side, and a coarse stride between them
SWEEP_ROWS = sorted({r + d for r in (48, 96, 512, 2048, 4096, 8192, 16384, 32768) for d in (-1, 0, 1)} |
                    {1, 17, 200, 1000, 3000, 6000, 12800, 24000, 40000})
SWEEP_CHANNELS = (32, 64, 96, 128, 160, 192, 224, 256, 384, 512, 544, 768, 1024, 1536)
ALL_CHANNELS = tuple(range(32, 1537, 32))  # (the default environment: every multiple of 32 on one side, the list above on the other)


@pytest.mark.parametrize("env", ENVS, ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()) or "default")
def test_workspace_query_covers_every_plan(lib, monkeypatch, env):
  """pcmi_spconv_workspace_bytes(...) of the convolution a launch belongs to is at least what the launch requires:
  3^3 stride-1 (K = 27, table form, with tile units from 4096 rows), 2^3 stride-2 and its transposed convolution (K = 8:
  the table over the coarse rows, the pair lists over twice as many fine rows) and the dense 1x1 (K = 1), the launch as
  the forward and as the backward-data pass, the operand packed and over 2 GiB."""
  _setenv(monkeypatch, env)
  q = lib.pcmi_spconv_workspace_bytes
  wide = SWEEP_CHANNELS if env else ALL_CHANNELS
  pairs = sorted({(c, n) for c in wide for n in SWEEP_CHANNELS} | {(c, n) for c in SWEEP_CHANNELS for n in wide})
  for rows in SWEEP_ROWS:
    for c, n in pairs:
      for k, forms in ((1, (NONE,)), (8, (TABLE, PAIRS)), (27, (TABLE, UNITS) if rows >= 4096 else (TABLE,))):
        for form in forms:
          # the other side of the map: K = 8 tables run over the coarse rows of twice as many fine ones, pair lists over the fine
          other = rows if k != 8 else (2 * rows if form == TABLE else (rows + 1) // 2)
          # as the forward launch of c -> n (rows = the call's n_out) and as the backward-data launch of n -> c (rows = n_in)
          as_fwd = q(other, rows, c, n, k, max(rows, other))
          as_bwd = q(rows, other, n, c, k, max(rows, other))
          for x_bytes in (other * c * 4, 1 << 31):
            ws = _plan(lib, rows, x_bytes, c, n, k, form)[4]
            assert as_fwd >= ws and as_bwd >= ws, (env, rows, c, n, k, form, x_bytes, ws, as_fwd, as_bwd)


def test_plan_refuses_shapes_no_launch_has(lib):
  for args in ((0, 0, 64, 64, 27, TABLE), (100, 0, 48, 64, 27, TABLE), (100, 0, 64, 64, 28, TABLE), (100, 0, 64, 64, 27, 4),
               (100, 0, 64, 64, 27, NONE)):
    assert lib.pcmi_spconv_plan(*args, None, None, None, None, None) == -1, args
  assert lib.pcmi_spconv_plan(100, 0, 64, 64, 27, TABLE, None, None, None, None, None) == 0
