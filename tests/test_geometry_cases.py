"""Pins what tests/geometry_cases.py promises (CPU, oracle only), so that the GPU tests built on these clouds
(tests/test_gpu_conv_geometry.py) cannot drift back to surface-like occupancy: rows per level, occupied 3^3 offsets,
the per-offset pair counts of the 2^3 stride-2 maps, and -- where the library sorts the rows (>= 4096) -- the units per
128-row tile of the mask-sorted order.

Everything follows from the geometry except the unit TOTALS of the shuffled solid / mixed clouds (1716, 698), which
depend on the shuffle seed of geometry_cases.py; in insertion order the mixed cloud has 585.
"""
import numpy as np
import pytest

import geometry_cases as gc
from oracle import sparse_ref as sr


def _one(k, n):
  return [n if i == k else 0 for i in range(8)]


def _iso(n, k):
  return dict(rows=[n] * 5, occupied=[1] * 5, M=n, child=[_one(k, n)] + [_one(0, n)] * 3)


def _sheet(axis, side):
  """Plane at the odd coordinate 3 of `axis`: bit `axis` of the child offset is set at level 0 (3 = 2 * 1 + 1) and level
  1 (floor(3 / 2) * 2 = 2 = 4 * 0 + 2) and clear above; the in-plane axes run from -8."""
  lv = []
  lo, hi = -8, -8 + side - 1
  for ts in (1, 2, 4, 8, 16):
    lv.append(hi // ts - lo // ts + 1)

  def counts(l):  # children of level l per in-plane offset bit: cells with a child at bit 0 / bit 1 along one axis
    ts = 1 << l
    cells = np.arange(lo // ts, hi // ts + 1)
    return [int((cells % 2 == 0).sum()), int((cells % 2 == 1).sum())]

  child = []
  for l in range(4):
    nbit = 1 if l < 2 else 0
    c = counts(l)
    row = [0] * 8
    inplane = [a for a in range(3) if a != axis]
    for bu in (0, 1):
      for bv in (0, 1):
        k = (nbit << axis) | (bu << inplane[0]) | (bv << inplane[1])
        row[k] = c[bu] * c[bv]
    child.append(row)
  return dict(rows=[v * v for v in lv], occupied=[9] * 5, M=(3 * side - 2) ** 2, child=child)


EXPECT = {
    "iso40": _iso(40, 7),
    "iso600": _iso(600, 5),
    "iso4224": dict(_iso(4224, 0), units=(1, 1, 33), masks=1),
    "solid3x4x3": dict(rows=[36, 8, 1, 1], occupied=[27, 27, 1, 1], M=7 * 10 * 7,
                       child=[[8, 4, 8, 4, 4, 2, 4, 2], [1] * 8, _one(7, 1)]),
    "solid8": dict(rows=[512, 64, 8, 1], occupied=[27, 27, 27, 1], M=22 ** 3, child=[[64] * 8, [8] * 8, [1] * 8]),
    "solid16x2": dict(rows=[8192, 1024, 128, 16, 2], occupied=[27, 27, 27, 27, 1], M=194672,
                      child=[[1024] * 8, [128] * 8, [16] * 8, [2] * 8], units=(24, 27, 1716), masks=27),
    "sheet0_24": _sheet(0, 24), "sheet1_24": _sheet(1, 24), "sheet2_24": _sheet(2, 24),
    "sheet0_66": dict(_sheet(0, 66), units=(9, 9, 315), masks=9),
    "sheet1_66": dict(_sheet(1, 66), units=(9, 9, 315), masks=9),
    "sheet2_66": dict(_sheet(2, 66), units=(9, 9, 315), masks=9),
    "checker12": dict(rows=[864, 216, 27, 8, 8], occupied=[13, 27, 27, 27, 27], M=9576,
                      child=[[216, 0, 0, 216, 0, 216, 216, 0], [27] * 8, [8, 4, 4, 2, 4, 2, 2, 1], [1] * 8]),
    "checker22": dict(rows=[5324, 1331, 216, 27, 8], occupied=[13, 27, 27, 27, 27], M=63536,
                      child=[[1331, 0, 0, 1331, 0, 1331, 1331, 0], [216, 180, 180, 150, 180, 150, 150, 125], [27] * 8,
                             [1, 2, 2, 4, 2, 4, 4, 8]], units=(13, 13, 546), masks=23),
    "mixed14": dict(rows=[4244, 2012, 1564, 1508, 1508], occupied=[27] * 5, M=65500,
                    child=[[343] * 7 + [1843], [1564] + [64] * 7, [1508] + [8] * 7, [1501] + [1] * 7],
                    units=(1, 27, 698), masks=28),
}
EXPECT["mixed14_ordered"] = dict(EXPECT["mixed14"], units=(1, 27, 585))


def test_every_case_is_pinned():
  assert set(EXPECT) == set(gc.CASES)
  # the table of the sheets is derived above, not typed: its level-0 rows as stated
  assert EXPECT["sheet0_24"]["rows"][:4] == [576, 144, 36, 9] and EXPECT["sheet0_24"]["child"][0] == [0, 144, 0, 144, 0, 144, 0, 144]
  assert EXPECT["sheet1_24"]["child"][0] == [0, 0, 144, 144, 0, 0, 144, 144]
  assert EXPECT["sheet2_66"]["rows"][0] == 4356 and EXPECT["sheet2_66"]["child"][0] == [0, 0, 0, 0, 1089, 1089, 1089, 1089]


@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_case_has_the_pinned_occupancy(name):
  want = EXPECT[name]
  c = gc.rows(name)
  assert c.dtype == np.int32 and c.ndim == 2 and c.shape[1] == 4
  assert len(np.unique(c, axis=0)) == len(c), "rows are unique"
  assert bool((c[:, 1:] < 0).any()), "some coordinates are negative"
  fn, args = gc.CASES[name]
  if name != "mixed14_ordered":
    assert not (c == np.array(sorted(map(tuple, c)), np.int32)).all(), "rows are shuffled"
  assert (fn(*args) == c).all(), "the generator is deterministic"
  ref = sr.CoordsManagerRef(c)
  key, levels = 0, len(want["rows"])
  for lvl in range(levels):
    assert ref.size(key) == want["rows"][lvl], "rows of level %d" % lvl
    m = ref.kernel_map(key, key, 3, sr.HYBRID)
    assert int((np.diff(m.offs) > 0).sum()) == want["occupied"][lvl], "occupied 3^3 offsets of level %d" % lvl
    if lvl == 0:
      assert int(m.offs[-1]) == want["M"]
      if "units" in want:
        assert len(c) >= gc.SORT_ROWS_MIN
        perm, tile_mask, tile_pref = gc.tile_tables(m.nbr)
        cnt = np.diff(tile_pref)
        assert (int(cnt.min()), int(cnt.max()), int(tile_pref[-1])) == want["units"]
        assert len(np.unique(gc.row_masks(m.nbr))) == want["masks"]
      else:
        assert len(c) < gc.SORT_ROWS_MIN
    if lvl + 1 < levels:
      ck = ref.stride(key, 2)
      assert np.diff(ref.kernel_map(key, ck, 2).offs).tolist() == want["child"][lvl], "stride-2 pair counts of level %d" % lvl
      key = ck


def test_mixed_orders_hold_the_same_voxels():
  a, b = gc.rows("mixed14"), gc.rows("mixed14_ordered")
  assert sorted(map(tuple, a)) == sorted(map(tuple, b)) and not (a == b).all()
  # insertion order: the solid cube's 14^3 rows, then the lattice
  assert (np.abs(b[:2744, 1:]) <= 7).all() and (b[2744:, 1:] > 3000).all()


def test_sort_rule_restated():
  """chunk = ceil(ceil(n / 128) / 8) * 128; inside a chunk the masks along perm are non-decreasing, ties in row order."""
  assert [gc.xcd_chunk_rows(n) for n in (4096, 4097, 4224, 8192, 81920)] == [512, 640, 640, 1024, 10240]
  nbr = sr.CoordsManagerRef(gc.rows("mixed14")).kernel_map(0, 0, 3, sr.HYBRID).nbr
  perm, tile_mask, tile_pref = gc.tile_tables(nbr)
  mask = gc.row_masks(nbr)
  chunk = gc.xcd_chunk_rows(len(perm))
  assert sorted(perm.tolist()) == list(range(len(perm)))
  assert (perm // chunk == np.arange(len(perm)) // chunk).all()
  same = (np.arange(len(perm)) // chunk)[1:] == (np.arange(len(perm)) // chunk)[:-1]
  d = np.diff(mask[perm])
  assert (d[same] >= 0).all() and (np.diff(perm)[same & (d == 0)] > 0).all()
  assert tile_pref[0] == 0 and len(tile_pref) == len(tile_mask) + 1
