"""Every pcmi_*_workspace_bytes whose entry point carves its workspace with a layout function (csrc/internal.h: Carve) returns
the number it returned before the layouts were written that way.  tests/golden/workspace_bytes.json was recorded ONCE, by
running query_all() of this file against libpcmi.so built from the commit before the change; it is never regenerated from the
code under test.  Per query: zero and one row, one below / at / one above the workgroup (256) and scan-block (1024) edges, B of 1
and the entry's maximum, a bad shape (0 bytes) and a shape near the documented row limit (a 32-bit product would show).  No GPU:
none of these queries reads the device."""
import ctypes as C
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_bytes.json")

ROWS = [0, 1, 255, 256, 257, 1023, 1024, 1025]
BIG = 1 << 29  # the row limit of the hashed entries
I31 = (1 << 31) - 1


def _rows(*more):
  return [(n,) for n in ROWS + list(more)]


def _rows_b(b_max, big, bad):
  """(n, B): every row count at B = 1, the edges at B = b_max, the large shape, the bad shapes"""
  return [(n, 1) for n in ROWS] + [(n, b_max) for n in (0, 257, 1025)] + [(big, 1), (big, b_max)] + list(bad)


# name (without pcmi_ and _workspace_bytes) -> (ctypes of the arguments: q int64, i int), argument tuples
TABLE = {
    "pair_select": ("q", _rows(BIG, I31)),
    "voxelize": ("q", _rows(BIG, I31)),
    "match_radius": ("qq", [(a, b) for a in ROWS for b in (1, 257, 1024)] + [(BIG, BIG), (I31, 1), (1, I31)]),
    "pair_transform": ("qq", _rows_b(512, I31 - 256, [(-1, 1), (1, 0), (1, 513), (I31, 1)])),
    "pair_voxelize": ("qq", _rows_b(512, BIG, [(-1, 1), (1, 0), (1, 513), (BIG + 1, 1)])),
    "pair_match": ("qq", _rows_b(512, BIG, [(-1, 1), (1, 0), (1, 513), (BIG + 1, 1)])),
    "pair_collate": ("qq", _rows_b(512, BIG, [(-1, 1), (1, 0), (1, 513)])),
    "pair_color_features": ("qq", _rows_b(512, BIG, [(-1, 1), (1, 0), (1, 513)])),
    "elastic_blur": ("qiii", [(1, 3, 3, 3), (1, 7, 6, 7), (2, 16, 17, 15), (1023, 4, 4, 4), (1, 4096, 4096, 42), (1023, 89, 89, 88),
                              (0, 3, 3, 3), (1024, 3, 3, 3), (1, 2, 3, 3), (1, 4097, 3, 3), (1, 4096, 4096, 43)]),
    "seg_transform": ("q", [(0,), (1,), (2,), (42,), (43,), (1023,), (1024,), (-1,)]),
    "seg_quantize": ("q", _rows(BIG, BIG + 1, -1)),
    "seg_color_augment": ("q", [(0,), (1,), (7,), (8,), (1023,), (1024,), (-1,)]),
    "instance_relabel": ("q", _rows(BIG, BIG + 1, -1)),
    "seg_crop_ladder": ("qq", _rows_b(1023, BIG, [(-1, 1), (1, 0), (1, 1024), (BIG + 1, 1)])),
    "det_votes_from_instances": ("q", [(0,), (1,), (2,), (1023,), (1024,), (-1,)]),
    "det_voxelize": ("qq", [(1, n) for n in ROWS[1:]] + [(1023, 1), (1023, 257), (2, 1025), (1, BIG), (1023, BIG // 1023), (0, 1),
                            (1, 0), (1024, 1), (2, BIG), (1, BIG + 1)]),
    "segment_quantile": ("q", [(0,), (1,), (2,), (1023,), (1024,), (-1,)]),
    "corpus_backproject": ("qqq", [(1, 1, n) for n in ROWS] + [(3, 16, 16), (5, 480, 640), (1, 1 << 15, (1 << 16) - 1), (0, 480, 640),
                                   (1, 0, 640)]),
    "corpus_backproject_color": ("qqq", [(1, 1, n) for n in ROWS] + [(3, 16, 16), (5, 480, 640), (1, 1 << 15, (1 << 16) - 1),
                                         (0, 480, 640), (1, 0, 640)]),
    "corpus_voxel_centroids": ("qq", [(n, 1) for n in ROWS] + [(n, 65535) for n in (0, 257, 1025)] + [(BIG - 1, 1), (BIG - 1, 65535),
                                      (1000, 0), (-5, 3)]),
    "corpus_overlap": ("qq", [(n, 1) for n in ROWS] + [(257, 65535), ((1 << 30) - 1, 1), ((1 << 30) - 1, 65535), (-5, 3)]),
    "views_visible": ("qq", [(n, 1) for n in ROWS] + [(n, 4096) for n in (0, 1, 257, 1025)] + [(I31 - 1, 1), (1 << 25, 4096), (5, 0),
                             (-1, -1)]),
    "nearest_point": ("qqq", [(m, n, 1) for m in ROWS for n in (0, 1, 257)] + [(257, n, 1) for n in ROWS] + [(257, 1025, 1024),
                              (BIG, I31, 1), (BIG, I31, 1024), (-1, 1, 1), (1, -1, 1), (1, 1, 0), (1, 1, 1025), (BIG + 1, 1, 1)]),
    "radius_components": ("qq", _rows_b(1 << 20, BIG, [(-1, 1), (1, 0), (1, (1 << 20) + 1), (BIG + 1, 1)])),
    "components_compact": ("q", _rows(BIG, I31, I31 + 1, -1)),
    "instance_scores": ("q", _rows(I31, -1)),
    "offset_loss": ("q", _rows(I31 - 256, -1)),
    "kmeans_assign": ("qi", [(1, 1), (1, 31), (1, 32), (1, 33), (2, 50), (65535, 1), (65535, 1024), (3, 1 << 20), (65535, 1 << 20), (0, 4), (4, 0),
                             (-1, -1)]),
    "kmeans_pp_step": ("q", [(0,), (1,), (2,), (255,), (256,), (257,), (65535,), (-1,)]),
    "proposal_overlap": ("q", _rows(I31, I31 + 1, -1)),
    "instance_bench_ap": ("qii", [(e, 1, 1) for e in ROWS] + [(257, 64, 16), (1025, 18, 9), ((1 << 30) - 1, 64, 16), (1 << 30, 1, 1),
                                  (5, 0, 1), (5, 65, 1), (5, 1, 0), (5, 1, 17), (-1, 1, 1)]),
    "seg_eval_rows": ("q", _rows(I31 - 256, -1)),
    "seg_ap": ("i", [(0,), (1,), (20,), (63,), (64,), (65,), (-1,)]),
    "det_ap": ("qqi", [(nd, g, 1) for nd in ROWS for g in (0, 1, 257)] + [(257, 1025, 16), (1025, 257, 9), (I31 - 1, I31, 16),
                       (1 << 28, 1 << 28, 16), (-1, 1, 1), (1, -1, 1), (1, 1, 0), (1, 1, 17), (1 << 31, 1, 1)]),
    "fps": ("qqi", [(n, m, r) for n in ROWS for m in (256, 8192, 8193) for r in (0, 1)] + [((1 << 31) // 3 - 1, 1 << 20, 1),
                    ((1 << 31) // 3 - 1, 100, 1), (-1, 9000, 1), (100, -1, 0)]),
    "pointset_scatter": ("qq", [(a, b) for a in ROWS for b in (0, 1, 257, 1024)] + [(I31, I31 - 1), (I31, 1), (1, I31 - 1), (-1, -1)]),
    "group_rows_bwd": ("qqqq", [(1, n, 16, 8) for n in ROWS] + [(1, 300, p, 16) for p in (0, 1, 16, 64, 65)] + [(2, 257, 33, 3),
                                (8, 1025, 256, 64), (1, (1 << 31) // 3 - 1, 1 << 20, 2047), (0, 5, 5, 5), (4, 0, 5, 5)]),
    "bn_maxpool": ("qii", [(r, 16, 64) for r in ROWS] + [(257, 1, 3), (257, 256, 128), (1025, 64, 256), (1 << 22, 256, 512), (5, 0, 0),
                           (-1, 16, 64)]),
    "interp_rows_bwd": ("qqq", [(1, 64, n) for n in ROWS] + [(1, m, 300) for m in ROWS] + [(2, 257, 1025), (8, 1 << 20, (1 << 26) - 1),
                                (0, 5, 5)]),
    "nn_distance_bwd": ("qqq", [(1, n, m) for n in (1, 257, 1025) for m in (1, 32, 33, 1023, 1024, 1025)] + [(2, 300, 2000),
                                (65535, 40, 40), (65536, 33, 33), (65536, 1000, 1025), (1, (1 << 31) // 3 - 1, 1025), (0, 5, 5),
                                (1, 0, 5), (1, 5, 0), (1, 1 << 31, 1)]),
    "feat_nn": ("q", _rows(I31 - 257, -1)),
}

CTYPES = {"q": C.c_int64, "i": C.c_int}


def query_all(lib_path):
  """{name: [[args..., bytes], ...]} of every query of TABLE in the library at lib_path"""
  lib = C.CDLL(lib_path)
  out = {}
  for name, (types, cases) in TABLE.items():
    fn = getattr(lib, "pcmi_%s_workspace_bytes" % name)
    fn.restype = C.c_size_t
    fn.argtypes = [CTYPES[t] for t in types]
    out[name] = [list(args) + [int(fn(*args))] for args in cases]
  return out


@pytest.fixture(scope="module")
def golden():
  with open(GOLDEN) as f:
    return json.load(f)


@pytest.fixture(scope="module")
def current(built_lib):
  return query_all(built_lib)


def test_golden_covers_the_table(golden):
  assert sorted(golden) == sorted(TABLE)
  for name, (types, cases) in TABLE.items():
    assert [row[:-1] for row in golden[name]] == [list(a) for a in cases], name
    sizes = [row[-1] for row in golden[name]]
    assert 0 in sizes or name in NO_BAD_SHAPE, "%s: no refused shape in the table" % name
    assert max(sizes) > (1 << 32) or name in SMALL, "%s: no shape whose size needs more than 32 bits" % name


# queries that have no shape guard (they size max(n, 1) rows, or nothing, instead of refusing) ...
NO_BAD_SHAPE = {"pair_select", "voxelize", "match_radius", "corpus_backproject", "corpus_backproject_color", "corpus_voxel_centroids",
                "corpus_overlap", "views_visible", "pointset_scatter", "group_rows_bwd", "bn_maxpool", "interp_rows_bwd"}
# ... and those whose largest legal workspace stays below 4 GiB
SMALL = {"pair_collate", "pair_color_features", "seg_transform", "seg_color_augment", "det_votes_from_instances", "segment_quantile",
         "kmeans_pp_step", "seg_ap", "offset_loss", "pair_transform", "seg_eval_rows", "bn_maxpool"}


@pytest.mark.parametrize("name", sorted(TABLE))
def test_query_returns_what_it_returned_before_the_layout_functions(name, golden, current):
  for want, got in zip(golden[name], current[name]):
    assert got == want, "pcmi_%s_workspace_bytes%r: %d bytes, %d before" % (name, tuple(got[:-1]), got[-1], want[-1])
