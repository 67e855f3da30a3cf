"""Voxel sets at the extremes of occupancy (numpy only): what a cropped, sparse or synthetic scene can produce and the
wavy sheets of helpers.surface_coords never do.  The host plans and the kernels of the convolution stack depend on the
occupancy pattern -- how many of the 27 offsets a row has, how many (tile, offset) units a 128-row tile has, how the
rows of a stride-2 map spread over its 8 offsets -- and these clouds sit at the ends of those ranges:

  isolated   a lattice no two points of which are neighbours: every 3^3 map is centre-only (1 unit per tile), every
             stride-2 map has all its rows in ONE of the 8 offsets, the other 7 are empty;
  solid      a full box: all 27 offsets, 24..27 units per tile, every stride-2 offset exactly at n_coarse (the bound);
  sheet      an axis-aligned plane: 9 of 27 offsets, 4 stride-2 offsets at the bound and 4 empty;
  checker    the even-parity voxels of a cube: 13 of 27 offsets, 4 of 8 stride-2 offsets;
  mixed      a solid cube and an isolated lattice in one level: tiles of 1 unit beside tiles of 27.

Every generator returns unique int32 (b, x, y, z) rows, some with negative coordinates, shuffled by a fixed seed
(mixed(..., shuffle=False) keeps insertion order: the solid rows, then the isolated ones).
tests/test_geometry_cases.py pins the properties above for every entry of CASES with the CPU oracle.
"""
import numpy as np

_SEED = 20


def _finish(arr, shuffle=True):
  arr = np.ascontiguousarray(arr, dtype=np.int32)
  assert len(np.unique(arr, axis=0)) == len(arr)
  if shuffle:
    np.random.RandomState(_SEED).shuffle(arr)
  return arr


def _lattice(n, spacing, origin):
  """n points i * spacing + origin, i over the first n cells of a cube of side ceil(cbrt(n)) centred on zero."""
  s = 1
  while s ** 3 < n:
    s += 1
  i = np.arange(n)
  idx = np.stack([i % s, i // s % s, i // (s * s)], 1) - s // 2
  return idx * spacing + np.asarray(origin)


def isolated(n, spacing=32, origin=(0, 0, 0), batch=1, shuffle=True):
  """n rows over `batch` instances, `spacing` apart on every axis.  With spacing 32 no two rows are neighbours on any
  of the five levels of a U-Net (tensor strides 1..16) and every level has n rows."""
  per = [n // batch + (b < n % batch) for b in range(batch)]
  out = [np.concatenate([np.full((m, 1), b), _lattice(m, spacing, origin)], 1) for b, m in enumerate(per)]
  return _finish(np.concatenate(out), shuffle)


def _box(sx, sy, sz, origin):
  x, y, z = np.meshgrid(np.arange(sx), np.arange(sy), np.arange(sz), indexing="ij")
  return np.stack([x.ravel(), y.ravel(), z.ravel()], 1) + np.asarray(origin)


def solid(sx, sy, sz, batch=1, origin=(0, 0, 0), shuffle=True):
  """Every voxel of a sx x sy x sz box at `origin`, in each of `batch` instances."""
  p = _box(sx, sy, sz, origin)
  return _finish(np.concatenate([np.concatenate([np.full((len(p), 1), b), p], 1) for b in range(batch)]), shuffle)


def sheet(axis, side, batch=1, origin=-8):
  """A side x side plane with its normal along `axis` (0, 1, 2 = x, y, z); the plane of instance b lies at the odd
  coordinate 3 + 2 b of that axis, the in-plane coordinates run from `origin`."""
  u, v = np.meshgrid(np.arange(side) + origin, np.arange(side) + origin, indexing="ij")
  out = []
  for b in range(batch):
    cols = [u.ravel(), v.ravel()]
    cols.insert(axis, np.full(side * side, 3 + 2 * b))
    out.append(np.stack([np.full(side * side, b)] + cols, 1))
  return _finish(np.concatenate(out))


def checker(side, batch=1, origin=-8):
  """The voxels of a side^3 cube at (origin, origin, origin) whose coordinates sum to an even number."""
  p = _box(side, side, side, (origin,) * 3)
  p = p[p.sum(1) % 2 == 0]
  return _finish(np.concatenate([np.concatenate([np.full((len(p), 1), b), p], 1) for b in range(batch)]))


def mixed(side, n_isolated, shuffle=True, spacing=16, far=4096 + 1):
  """A solid side^3 cube centred on zero and n_isolated lattice points `spacing` apart around (far, far, far), one
  instance.  shuffle=False: the cube's rows first, then the lattice's."""
  p = np.concatenate([_box(side, side, side, (-(side // 2),) * 3), _lattice(n_isolated, spacing, (far,) * 3)])
  return _finish(np.concatenate([np.zeros((len(p), 1), np.int64), p], 1), shuffle)


# name -> (generator, args).  rows(name) builds the array; the instances the GPU tests use.
CASES = {
    "iso40": (isolated, (40, 32, (1, 1, 1), 1)),
    "iso600": (isolated, (600, 32, (1, 0, 1), 2)),
    "iso4224": (isolated, (4224, 32, (0, 0, 0), 2)),
    "solid3x4x3": (solid, (3, 4, 3, 1, (-4, -4, -4))),
    "solid8": (solid, (8, 8, 8, 1, (-8, 0, -8))),
    "solid16x2": (solid, (16, 16, 16, 2, (-16, 0, -16))),
    "sheet0_24": (sheet, (0, 24)),
    "sheet1_24": (sheet, (1, 24)),
    "sheet2_24": (sheet, (2, 24)),
    "sheet0_66": (sheet, (0, 66)),
    "sheet1_66": (sheet, (1, 66)),
    "sheet2_66": (sheet, (2, 66)),
    "checker12": (checker, (12,)),
    "checker22": (checker, (22,)),
    "mixed14": (mixed, (14, 1500, True)),
    "mixed14_ordered": (mixed, (14, 1500, False)),
}

_BUILT = {}


def rows(name):
  """The (read-only) coordinate array of a named case, built once."""
  if name not in _BUILT:
    fn, args = CASES[name]
    arr = fn(*args)
    arr.setflags(write=False)
    _BUILT[name] = arr
  return _BUILT[name]


# ----------------------------------------------------------------------------------------------------------------
# the sort rule of csrc/sortrows.hip / csrc/coords.hip restated (3^3 stride-1 maps with at least 4096 rows)
# ----------------------------------------------------------------------------------------------------------------
SORT_ROWS_MIN = 4096
TILE = 128


def row_masks(nbr):
  """Bit k of mask[j] = row j has a neighbour at offset k (nbr: the oracle's [K, n] table)."""
  K = nbr.shape[0]
  return ((nbr >= 0).astype(np.int64) << np.arange(K)[:, None]).sum(0)


def xcd_chunk_rows(n):
  """Rows of the contiguous range one XCD processes: ceil(ceil(n / 128) / 8) * 128."""
  return -(-(-(-n // TILE)) // 8) * TILE


def tile_tables(nbr):
  """(perm, tile_mask, tile_pref) of the sorted order: key = (row // chunk) << K | mask, stable."""
  K, n = nbr.shape
  mask = row_masks(nbr)
  key = (np.arange(n) // xcd_chunk_rows(n)) << K | mask
  perm = np.argsort(key, kind="stable")
  n_tiles = -(-n // TILE)
  padded = np.zeros(n_tiles * TILE, np.int64)
  padded[:n] = mask[perm]
  tile_mask = np.bitwise_or.reduce(padded.reshape(n_tiles, TILE), axis=1)
  cnt = np.array([bin(int(m)).count("1") for m in tile_mask], np.int64)
  tile_pref = np.concatenate([[0], np.cumsum(cnt)])
  return perm, tile_mask, tile_pref
