"""The plan of the weight-gradient calls (csrc/spconv_wgrad_plan.h: plan_wgrad, reported by pcmi_spconv_wgrad_plan), on the CPU.

tests/golden/wgrad_plans_cu256.json holds what spconv_backward_weight_m32, wgrad_x3t_run and wgrad_group_add decided --
kernel family, tile shape, chunk, chunk slots per offset, mode, addressing, row blocks, the smallest workspace accepted
and whether the layer joined a group -- at the commit before those decisions were gathered into plan_wgrad, recorded
there from the three functions themselves (made to log and return in front of their launches, on maps whose pointers are
never dereferenced) for 256 compute units.  Cases: every (n, cin, cout) of test_gpu_c_contract.py's EDGE_CASES,
STRIDED_ROWS ("down" and "up") and WIDE_CASES and test_gpu_conv_geometry.py's SK_CASES, the 3 -> 32 stem at 100 and
40 000 rows, a map without rows, the dense 1x1 form at 8191 / 8192 rows for 64 -> 64 and 128 -> 96.  Variants of a
case: with and without gbias; the map's per-offset counts absent, surface-like and all in one offset (counts());
operands packed and over 2 GiB; both conv precisions; the residency of the pair-list kernel as the HIP runtime gives it
on an MI355X (the table's "occupancy", read there once) and at the library's fallback 2.  Every combination of these is
recorded under the default environment and under each of the five switches alone (PCMI_WGRAD_X3T at 0, 1 and 16384).
The planner must reproduce every line, and the workspace query must return what it returned then and cover every plan.
Without a GPU the library counts 256 compute units (csrc/internal.h: num_cu), as the MI355X has."""
import ctypes as C
import json
import os

import pytest

from test_conv_plan import SWEEP_CHANNELS, SWEEP_ROWS

SWITCHES = ("PCMI_WGRAD_X3T", "PCMI_WGRAD_X3T_DENSE", "PCMI_WGRAD_X3P", "PCMI_WGRAD_GROUP", "PCMI_WGRAD_BUF")
ENVS = [{}, {"PCMI_WGRAD_X3T": "0"}, {"PCMI_WGRAD_X3T": "1"}, {"PCMI_WGRAD_X3T": "16384"}, {"PCMI_WGRAD_X3T_DENSE": "0"},
        {"PCMI_WGRAD_X3P": "0"}, {"PCMI_WGRAD_GROUP": "0"}, {"PCMI_WGRAD_BUF": "0"}]
# include/pcmi.h: PCMI_WGRAD_KERNEL_*, PCMI_WGRAD_MODE_*, PCMI_WGRAD_MAP_*, PCMI_ERR_*
NONE, X3P, X3T, STEM_MFMA, STEM, PAIRS = range(6)
SLABS, DIRECT, ARRIVE = range(3)
MAP_NBR, MAP_PERM = 1, 2
ERR_INVALID, ERR_UNSUPPORTED = -1, -6
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_plans_cu256.json")
CASE_FIELDS = ["n_in", "n_out", "cin", "cout", "K", "kernel_size", "stride", "map_tables", "transpose"]
VARIANT_FIELDS = ["gbias", "counts", "big", "precision", "fallback_occupancy"]
OUT_FIELDS = ["kernel", "tile_c", "tile_n", "chunk", "slots_per_offset", "mode", "address_bits", "row_blocks", "groupable", "ws_bytes"]
BUF_MAX = 0x7FFFFF00  # the largest operand the 32-bit forms address


def variants():
  """Every [gbias, counts, big, precision, fallback_occupancy]."""
  return [[g, c, b, p, o] for g in (0, 1) for c in (0, 1, 2) for b in (0, 1) for p in (0, 1) for o in (0, 1)]


def counts(which, K, n_in, n_out):
  """Host prefix [K + 1] of per-offset pair counts.  0: absent (None).  1: surface-like -- K = 27: the centre offset holds
  every row, the others 9 / 10 (faces), 6 / 10 (edges) and 4 / 10 (corners) of them, 16.8 neighbours per row; K = 8: the
  fine rows over the 8 children in the proportions 1 .. 8.  2: one offset (the middle one) holds as many pairs as an
  offset can, min(n_in, n_out), the others none."""
  if which == 0:
    return None
  bound = min(n_in, n_out)
  if which == 2:
    per = [bound if k == K // 2 else 0 for k in range(K)]
  elif K == 27:
    tenths = {0: 10, 1: 9, 2: 6, 3: 4}
    per = [bound * tenths[sum(1 for d in (k // 9 - 1, k // 3 % 3 - 1, k % 3 - 1) if d != 0)] // 10 for k in range(K)]
  else:
    per = [min(bound, max(n_in, n_out) * (k + 1) // 36) for k in range(K)]
  out = [0]
  for c in per:
    out.append(out[-1] + c)
  return out


def big_ld(n, c):
  """The smallest leading dimension (a multiple of 4, at least c) with which n rows exceed what 32-bit offsets address."""
  ld = -(-(BUF_MAX + 1) // (4 * max(n, 1)))
  return max((ld + 3) // 4 * 4, (c + 3) // 4 * 4)


def pair_tiles(c):
  return 3 if (c // 32) % 3 == 0 else (2 if (c // 32) % 2 == 0 else 1)


def slots(occupancy, case, fallback):
  """slots_per_cu of a case: the recorded answer of the HIP runtime for its pair-list variant, or the fallback."""
  if fallback or case["cin"] % 32:
    return 2
  return occupancy["%d,%d,%d" % (pair_tiles(case["cin"]), pair_tiles(case["cout"]), int(case["kernel_size"] != 0))]


def lds(case, big):
  """(in_ld, gout_ld) of a variant."""
  if not big:
    return case["cin"], case["cout"]
  return big_ld(case["n_in"], case["cin"]), big_ld(case["n_out"], case["cout"])


@pytest.fixture(scope="module")
def lib(built_lib):
  from pointcontrast_amd import _lib
  return _lib.lib


@pytest.fixture(scope="module")
def golden():
  g = json.load(open(GOLDEN))
  assert g["case_fields"] == CASE_FIELDS and g["variant_fields"] == VARIANT_FIELDS and g["out_fields"] == OUT_FIELDS + ["grouped"]
  assert g["variants"] == variants()
  return g


@pytest.fixture
def precision(lib):
  """Restores the calling thread's conv precision."""
  yield lambda p: lib.pcmi_set_conv_precision(p)
  lib.pcmi_set_conv_precision(0)


def _setenv(monkeypatch, env):
  for k in SWITCHES:
    monkeypatch.delenv(k, raising=False)
  for k, v in env.items():
    monkeypatch.setenv(k, v)


_OUT = [C.c_int() for _ in range(9)] + [C.c_size_t()]
_OUT_REFS = [C.byref(v) for v in _OUT]


def _plan_rc(lib, n_in, n_out, cin, cout, K, ks, stride, tables, transpose, gbias, accumulate, in_ld, gout_ld, cnt, slots_per_cu):
  arr = (C.c_int64 * len(cnt))(*cnt) if cnt is not None else None
  rc = lib.pcmi_spconv_wgrad_plan(n_in, n_out, cin, cout, K, ks, stride, tables, transpose, gbias, accumulate, n_in * in_ld * 4,
                                  n_out * gout_ld * 4, int(in_ld % 4 == 0 and gout_ld % 4 == 0), arr, slots_per_cu, *_OUT_REFS)
  return rc, tuple(v.value for v in _OUT)


def _plan(lib, *args):
  rc, out = _plan_rc(lib, *args)
  assert rc == 0, (rc, lib.pcmi_last_error().decode(), args)
  return out


def plan_variant(lib, occupancy, case, variant):
  """The planner's answer (OUT_FIELDS) for a recorded variant of a case; the calls are recorded accumulating."""
  gbias, cnt, big, _, fallback = variant
  in_ld, gout_ld = lds(case, big)
  return _plan(lib, *[case[f] for f in CASE_FIELDS], gbias, 1, in_ld, gout_ld, counts(cnt, case["K"], case["n_in"], case["n_out"]),
               slots(occupancy, case, fallback))


def _recorded(g):
  """(env, case, variant, recorded outputs) of every line of the table."""
  cases = [dict(zip(CASE_FIELDS, c)) for c in g["cases"]]
  for p in g["plans"]:
    vs = g["variants"]
    for case, idxs in zip(cases, p["rows"]):
      assert len(idxs) == len(vs)
      for v, i in zip(vs, idxs):
        if i >= 0:  # (-1: a dense case has no counts to vary)
          yield p["env"], case, v, g["outs"][i]


def test_golden_table_covers_what_it_claims(golden):
  g = golden
  assert g["compute_units"] == 256 and len(g["occupancy"]) == 18
  envs = [p["env"] for p in g["plans"]]
  for e in ENVS:
    assert e in envs
  assert len(g["cases"]) >= 100
  rows = [dict(zip(g["out_fields"], o)) for o in g["outs"]]
  assert sorted({r["kernel"] for r in rows}) == [NONE, X3P, X3T, STEM_MFMA, STEM, PAIRS]  # every kernel family is planned somewhere
  assert {r["mode"] for r in rows if r["kernel"] == PAIRS} == {SLABS, DIRECT, ARRIVE}
  assert {r["address_bits"] for r in rows if r["kernel"] == PAIRS} == {32, 64}
  assert {r["groupable"] for r in rows} == {0, 1}
  assert all(r["groupable"] == r["grouped"] for r in rows)
  for _, case, v, _ in _recorded(g):
    assert v[1] == 0 or case["kernel_size"] != 0


def test_planner_reproduces_recorded_decisions_and_query(lib, golden, monkeypatch, precision):
  g = golden
  cases = [dict(zip(CASE_FIELDS, c)) for c in g["cases"]]
  n = 0
  for p in g["plans"]:
    _setenv(monkeypatch, p["env"])
    for case, query in zip(cases, p["query"]):
      got = lib.pcmi_spconv_workspace_bytes(case["n_in"], case["n_out"], case["cin"], case["cout"], case["K"], max(case["n_in"], case["n_out"]))
      assert got == query, "%s %s: the query gives %d bytes, recorded %d" % (p["env"], case, got, query)
    for prec in (0, 1):
      precision(prec)
      for case, idxs, query in zip(cases, p["rows"], p["query"]):
        for v, i in zip(g["variants"], idxs):
          if i < 0 or v[3] != prec:
            continue
          want = tuple(g["outs"][i][:len(OUT_FIELDS)])
          got = plan_variant(lib, g["occupancy"], case, v)
          assert got == want, "%s %s %s: planned %s, recorded %s" % (p["env"], case, v, got, want)
          assert query >= want[-1], "%s %s %s: the query gives %d bytes" % (p["env"], case, v, query)
          n += 1
  assert n > 40000


def test_recorded_refusals(lib, golden):
  """Calls the parent commit refused, with its error codes (kernel_size 2 / stride 2 or 3 / 1 maps, gbias, aligned or not)."""
  seen = set()
  for *case, gbias, in_ld, gout_ld, rc in golden["refusals"]:
    c = dict(zip(CASE_FIELDS, case))
    got, _ = _plan_rc(lib, *case, gbias, 1, in_ld, gout_ld, None, 2)
    assert got == rc, (c, gbias, in_ld, gout_ld, got, rc)
    seen.add(rc)
  assert seen == {ERR_INVALID, ERR_UNSUPPORTED}


# one either side of 8192 (PCMI_WGRAD_X3T's default) is in SWEEP_ROWS; the chunk limits 256 (kWgradMinChunk) and 4096
# (kWgradMaxChunk, also the largest offset of a grouped layer) and eight times those (kArriveMax chunks per offset)
WGRAD_SWEEP_ROWS = sorted(set(SWEEP_ROWS) | {r + d for r in (256, 4096, 8 * 256, 8 * 4096) for d in (-1, 0, 1)})


@pytest.mark.parametrize("env", ENVS, ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()) or "default")
def test_workspace_query_covers_every_plan(lib, monkeypatch, precision, env):
  """pcmi_spconv_workspace_bytes(...) of the convolution is at least what its weight gradient requires, whatever the
  residency of the pair-list kernel (slots_per_cu 1 .. 8; it steers the chunk and with it the chunk slots): 3^3 stride-1
  (K = 27), 2^3 stride-2 and its transposed convolution (K = 8, twice as many fine rows) and the dense 1x1 (K = 1); with
  gbias (never the tile-stationary family; the column sums lie behind the slabs) and without (the tile-stationary family
  in both precisions: the one-role form has more row blocks); counts absent and all in one offset."""
  _setenv(monkeypatch, env)
  q = lib.pcmi_spconv_workspace_bytes
  n = 0
  for rows in WGRAD_SWEEP_ROWS:
    for K, ks, stride, tables, shapes in ((1, 0, 0, 0, ((rows, rows, 0),)), (8, 2, 2, MAP_NBR, ((2 * rows, rows, 0), (rows, 2 * rows, 1))),
                                          (27, 3, 1, MAP_NBR | (MAP_PERM if rows >= 4096 else 0), ((rows, rows, 0),))):
      for n_in, n_out, tr in shapes:
        for cin in SWEEP_CHANNELS:
          for cout in SWEEP_CHANNELS:
            query = q(n_in, n_out, cin, cout, K, max(n_in, n_out))
            for cnt in ((0, 2) if K > 1 else (0,)):
              ch = counts(cnt, K, n_in, n_out)
              args = (n_in, n_out, cin, cout, K, ks, stride, tables, tr)
              for gbias in (1, 0):
                for s in range(1, 9):
                  out = _plan(lib, *args, gbias, 1, cin, cout, ch, s)
                  assert query >= out[-1], (env, args, cnt, gbias, s, out, query)
                  n += 1
                  if out[0] != PAIRS:  # the residency is none of the other kernels' business
                    break
                if out[0] in (X3P, X3T):
                  precision(1)
                  out = _plan(lib, *args, gbias, 1, cin, cout, ch, 2)
                  precision(0)
                  assert out[0] == X3T and query >= out[-1], (env, args, cnt, out, query)
  assert n > 100000


def test_plan_refuses_shapes_no_launch_has(lib):
  ok = dict(n_in=100, n_out=100, cin=64, cout=64, K=27, ks=3, stride=1, tables=MAP_NBR, tr=0, gbias=0, acc=1, in_ld=64, gout_ld=64)

  def rc(**kw):
    a = dict(ok, **kw)
    return _plan_rc(lib, a["n_in"], a["n_out"], a["cin"], a["cout"], a["K"], a["ks"], a["stride"], a["tables"], a["tr"], a["gbias"], a["acc"],
                    a["in_ld"], a["gout_ld"], None, 2)[0]

  assert rc() == 0
  for bad in (dict(cin=0), dict(K=28), dict(K=0), dict(ks=5), dict(ks=3, stride=2), dict(ks=0, stride=0, tables=0),  # K = 27 without a map
              dict(ks=0, stride=0, tables=0, K=1, n_out=99), dict(n_in=-1), dict(in_ld=66)):  # (ld % 4 != 0)
    assert rc(**bad) == ERR_INVALID, bad
  for bad in (dict(cin=48), dict(cout=80), dict(cin=4, cout=32), dict(cin=3, cout=48, gbias=1)):
    assert rc(**bad) == ERR_UNSUPPORTED, bad
  # no pairs: nothing to refuse, nothing to do
  assert _plan_rc(lib, 0, 0, 48, 64, 27, 3, 1, MAP_NBR, 0, 0, 1, 48, 64, None, 2) == (0, (NONE, 0, 0, 0, 0, 0, 0, 0, 0, 0))
  # pcmi_spconv_bwd_weight overwrites (accumulate 0): wgrad_group_add takes accumulating layers only
  assert _plan(lib, 100, 100, 64, 64, 27, 3, 1, MAP_NBR, 0, 0, 1, 64, 64, None, 2)[8] == 1
  assert _plan(lib, 100, 100, 64, 64, 27, 3, 1, MAP_NBR, 0, 0, 0, 64, 64, None, 2)[8] == 0
  assert lib.pcmi_spconv_wgrad_plan(100, 100, 64, 64, 27, 3, 1, MAP_NBR, 0, 0, 1, 25600, 25600, 1, None, 0, *([None] * 10)) == 0
