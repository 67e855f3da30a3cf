"""tests/insseg_input_ref.py -- the numpy restatement the instance-input kernels are compared with bit for bit -- held to
independent spellings of the same rules: np.unique on (scene, id) pairs for the relabelling, np.bincount / np.maximum.at for
the table, a per-scene loop over Python integers for the crop; planted cases for all three; and the pipeline without a crop
against semseg_input_ref.pipeline on the outputs they share.  CPU only."""
import os
import re

import numpy as np

import insseg_input_ref as ir
import semseg_input_ref as sr


def _offs(sizes):
  return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


# ---- relabel --------------------------------------------------------------------------------------------------------------------
def relabel_by_unique(raw, offsets, keep=None):
  raw = np.asarray(raw, np.int64)
  n, B = len(raw), len(offsets) - 1
  scene = np.searchsorted(offsets, np.arange(n), side="right") - 1
  ok = (raw >= 0) & (scene >= 0) & (scene < B)
  if keep is not None:
    ok &= np.asarray(keep, bool)
  rows = np.flatnonzero(ok)
  pairs = np.stack([scene[rows], raw[rows]], 1)
  _, first, inverse = np.unique(pairs, axis=0, return_index=True, return_inverse=True)
  order = np.argsort(first, kind="stable")           # the unique pairs by their first row
  rank = np.empty(len(first), np.int64)
  rank[order] = np.arange(len(first))
  inst = np.full(n, -1, np.int32)
  inst[rows] = rank[inverse.reshape(-1)]
  first_row = rows[first[order]].astype(np.int32)
  counts = np.concatenate([np.bincount(scene[first_row], minlength=B)[:B], [len(first_row)]]).astype(np.int64)
  return inst, first_row, counts


def test_relabel_equals_np_unique_on_random_batches():
  rng = np.random.RandomState(0)
  for trial in range(20):
    sizes = rng.randint(0, 60, size=rng.randint(1, 5))
    n = int(sizes.sum())
    raw = rng.randint(-2, 9, size=n) * rng.choice([1, 1 << 20])
    keep = None if trial % 2 else (rng.rand(n) < 0.8)
    got, want = ir.instance_relabel(raw, _offs(sizes), keep), relabel_by_unique(raw, _offs(sizes), keep)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)), trial


def test_relabel_planted():
  # two scenes with the same raw ids, an empty scene between them, negative ids, the extremes of int32
  raw = [7, 7, 0, 2**31 - 1, -1, 0, -100, -2**31] + [0, 7, 7]
  inst, first, counts = ir.instance_relabel(raw, _offs([8, 0, 3]))
  assert inst.tolist() == [0, 0, 1, 2, -1, 1, -1, -1, 3, 4, 4] and first.tolist() == [0, 2, 3, 8, 9] and counts.tolist() == [3, 0, 2, 5]
  # a mask that removes an instance's lowest row: the instance is numbered by its next one, behind the instance between them
  inst, first, counts = ir.instance_relabel([5, 6, 5], _offs([3]), [0, 1, 1])
  assert inst.tolist() == [-1, 0, 1] and first.tolist() == [1, 2] and counts.tolist() == [2, 2]
  # rows beyond offsets[B] belong to no scene
  inst, _, counts = ir.instance_relabel([1, 1, 1, 1], np.array([0, 2]))
  assert inst.tolist() == [0, 0, -1, -1] and counts.tolist() == [1, 1]


# ---- table ----------------------------------------------------------------------------------------------------------------------
def table_by_bincount(instance, klass, coords, offsets, G):
  instance = np.asarray(instance, np.int64)
  n, B = len(instance), len(offsets) - 1
  scene_of = np.searchsorted(offsets, np.arange(n), side="right") - 1
  ok = (instance >= 0) & (instance < G) & (scene_of >= 0) & (scene_of < B)
  g = instance[ok]
  size = np.bincount(g, minlength=G).astype(np.int32)
  scene, cls = np.full(G, -1, np.int64), np.full(G, -1, np.int64)
  np.maximum.at(scene, g, scene_of[ok])
  np.maximum.at(cls, g, np.asarray(klass, np.int64)[ok])
  c = np.asarray(coords, np.int64)[ok][:, 1:4]
  s = np.zeros((G, 3), np.int64)
  np.add.at(s, g, c)
  lo, hi = np.full((G, 3), ir.INT32_MAX, np.int64), np.full((G, 3), ir.INT32_MIN, np.int64)
  np.minimum.at(lo, g, c)
  np.maximum.at(hi, g, c)
  return dict(size=size, scene=scene.astype(np.int32), cls=cls.astype(np.int32), sum=s, box_min=lo.astype(np.int32), box_max=hi.astype(np.int32))


def test_table_equals_bincount_on_random_batches():
  rng = np.random.RandomState(1)
  for trial in range(20):
    sizes = rng.randint(0, 80, size=rng.randint(1, 4))
    n, G = int(sizes.sum()), int(rng.randint(0, 12))
    inst = rng.randint(-1, G + 2, size=n)
    klass = rng.choice([-5, 0, 3, 2**31 - 1], size=n)
    coords = np.concatenate([np.zeros((n, 1), np.int64), rng.randint(0, 1 << 20, size=(n, 3))], 1)
    got, want = ir.instance_table(inst, klass, coords, _offs(sizes), G), table_by_bincount(inst, klass, coords, _offs(sizes), G)
    assert all(np.array_equal(got[k], want[k]) for k in want), trial


def test_table_planted():
  inst, klass = [0, 0, 2, -1, 3, 2], [-5, -7, 4, 9, 2**31 - 1, 6]
  coords = [[0, 1, 2, 3], [0, 5, 0, 1], [0, 2**20 - 1, 0, 0], [0, 9, 9, 9], [1, 7, 7, 7], [1, 2**20 - 1, 4, 0]]
  t = ir.instance_table(inst, klass, coords, _offs([4, 2]), 3)  # instance 1 has no rows, id 3 == G counts nowhere
  assert t["size"].tolist() == [2, 0, 2] and t["scene"].tolist() == [0, -1, 1] and t["cls"].tolist() == [-1, -1, 6]
  assert t["sum"].tolist() == [[6, 2, 4], [0, 0, 0], [2 * (2**20 - 1), 4, 0]]
  assert t["box_min"][1].tolist() == [ir.INT32_MAX] * 3 and t["box_max"][1].tolist() == [ir.INT32_MIN] * 3
  assert t["box_min"][0].tolist() == [1, 0, 1] and t["box_max"][0].tolist() == [5, 2, 3]
  t = ir.instance_table(inst, None, None, _offs([4, 2]), 0)
  assert t["size"].shape == (0,) and t["cls"] is None and t["sum"] is None


# ---- crop -----------------------------------------------------------------------------------------------------------------------
def crop_by_python_integers(coords, offsets, axes, sides, draws, max_voxels):
  B, S = len(offsets) - 1, len(sides)
  rows, counts, steps, flags = [], [], [], []
  for b in range(B):
    lo, hi = int(offsets[b]), int(offsets[b + 1])
    scene = [[int(coords[i][a]) for a in axes] for i in range(lo, hi)]
    kept, step, flag = list(range(lo, hi)), -1, 0
    if hi - lo > max_voxels:
      ext = [max(c[a] for c in scene) for a in range(2)]
      for s in range(S):
        side = [int(sides[s][a]) for a in range(2)]
        origin = [(int(draws[b][s][a]) * (max(ext[a] + 1 - side[a], 0) + 1)) >> 32 for a in range(2)]
        kept = [lo + k for k, c in enumerate(scene) if all(origin[a] <= c[a] < origin[a] + side[a] for a in range(2))]
        step = s
        if len(kept) <= max_voxels:
          break
      else:
        flag = ir.FLAG_CROP
    rows += kept
    counts.append(len(kept))
    steps.append(step)
    flags.append(flag)
  return np.asarray(rows, np.int64), np.asarray(counts + [sum(counts)], np.int64), np.asarray(steps, np.int32), np.asarray(flags, np.int32)


def test_crop_equals_the_python_loop_on_random_batches():
  rng = np.random.RandomState(2)
  for trial in range(20):
    sizes = rng.randint(0, 300, size=rng.randint(1, 4))
    n, S = int(sizes.sum()), int(rng.randint(1, 6))
    coords = np.concatenate([np.zeros((n, 1), np.int64), rng.randint(0, 40, size=(n, 3))], 1)
    sides = np.sort(rng.randint(1, 50, size=(S, 2)), axis=0)[::-1]
    draws = rng.randint(0, 2**32, size=(len(sizes), S, 2), dtype=np.int64)
    axes = [(1, 2), (3, 1), (2, 3)][trial % 3]
    mv = int(rng.randint(1, 200))
    got, want = ir.seg_crop_ladder(coords, _offs(sizes), axes, sides, draws, mv), crop_by_python_integers(coords, _offs(sizes), axes, sides, draws, mv)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)), trial


def lattice(w, h):
  """w x h voxels on the floor, one row each: coords [w h, 4] with x fastest."""
  y, x = np.divmod(np.arange(w * h), w)
  return np.stack([np.zeros_like(x), x, y, np.zeros_like(x)], 1)


def test_crop_planted():
  c = lattice(10, 10)  # 100 voxels, extents (9, 9)
  rows, counts, step, flags = ir.seg_crop_ladder(c, _offs([100]), (1, 2), [[5, 5]], np.zeros((1, 1, 2)), 100)
  assert step.tolist() == [-1] and np.array_equal(rows, np.arange(100)) and counts.tolist() == [100, 100] and not flags.any()
  # a ladder whose step 0 (a 10 x 9 window) counts 90 = max_voxels + 1 and whose step 1 (10 x 8) counts 80
  rows, counts, step, flags = ir.seg_crop_ladder(c, _offs([100]), (1, 2), [[10, 9], [10, 8]], np.zeros((1, 2, 2)), 89)
  assert step.tolist() == [1] and counts.tolist() == [80, 80] and not flags.any(), "step 0 counts 90 = max_voxels + 1"
  rows, counts, step, flags = ir.seg_crop_ladder(c, _offs([100]), (1, 2), [[10, 9], [10, 8]], np.zeros((1, 2, 2)), 90)
  assert step.tolist() == [0] and counts.tolist() == [90, 90], "step 0 counts exactly max_voxels"
  # no step fits: the last step and the flag
  rows, counts, step, flags = ir.seg_crop_ladder(c, _offs([100]), (1, 2), [[10, 9], [10, 8]], np.zeros((1, 2, 2)), 50)
  assert step.tolist() == [1] and counts.tolist() == [80, 80] and flags.tolist() == [ir.FLAG_CROP]
  # draws 0 and 2^32 - 1: the origin is 0 and the slack
  full = 2**32 - 1
  assert ir.crop_origin([0, full], [9, 9], [4, 4]).tolist() == [0, 6] and ir.crop_origin([full], [9], [20]).tolist() == [0]
  rows, counts, step, _ = ir.seg_crop_ladder(c, _offs([100]), (1, 2), [[4, 4]], [[[full, 0]]], 16)
  assert counts.tolist() == [16, 16] and np.array_equal(c[rows][:, 1:3].min(0), [6, 0]) and np.array_equal(c[rows][:, 1:3].max(0), [9, 3])
  assert np.all(np.diff(rows) > 0)


# ---- pipeline -------------------------------------------------------------------------------------------------------------------
def test_pipeline_without_crop_equals_the_semantic_pipeline():
  rng = np.random.RandomState(3)
  scenes = []
  for s in (400, 250):
    xyz = rng.uniform(0, 2, size=(s, 3))
    scenes.append((xyz, rng.randint(0, 256, size=(s, 3)).astype(np.float32), rng.randint(0, 5, size=s).astype(np.int32),
                   (xyz[:, 0] > 1).astype(np.int32) + 2 * (xyz[:, 1] > 1).astype(np.int32)))
  mats = np.repeat((np.eye(4) * [10.0, 10.0, 10.0, 1.0])[None], 2, 0)
  lut = np.array([0, 1, 2, 255, 3], np.int32)
  keys = rng.rand(650).astype(np.float32)
  for limit in (0, 450):
    want = sr.pipeline([s[:3] for s in scenes], mats, normalize=True, label_lut=lut, limit_numpoints=limit, dropout_keys=(keys, [True, False]))
    got = ir.pipeline(scenes, mats, normalize=True, label_lut=lut, limit_numpoints=limit, dropout_keys=(keys, [True, False]))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.int32), want[1].view(np.int32))
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[5], want[3]) and np.array_equal(got[6], want[4])
    inst, G = got[3], got[4]
    assert len(inst) == len(got[0]) and inst.max() < G and (inst[np.isin(got[2], [0, 1, 255])] == -1).all()
    assert (np.diff(np.unique(inst[inst >= 0], return_index=True)[1]) > 0).all(), "ids ascend with their first row"


def test_functional_constants_are_the_kernels_own():
  root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "pointcontrast_amd")
  scan = open(os.path.join(root, "csrc", "rowscan.h")).read()
  src = open(os.path.join(root, "csrc", "insseg_input.hip")).read()
  fn = open(os.path.join(root, "functional.py")).read()
  threads = int(re.search(r"constexpr int kThreads = (\d+);", scan).group(1))
  items = int(re.search(r"constexpr int kScanItems = (\d+),", scan).group(1))
  assert int(re.search(r"^ROW_SCAN_BLOCK = (\d+)", fn, re.M).group(1)) == threads * items
  assert eval(re.search(r"^ROW_SCAN_LEVEL = ([\d *]+)", fn, re.M).group(1)) == threads * threads * items
  assert int(re.search(r"^CROP_MAX_STEPS = (\d+)", fn, re.M).group(1)) == int(re.search(r"constexpr int kMaxSteps = (\d+);", src).group(1))
  assert "SEG_FLAG_CROP = 1, 2, 4, 8" in fn and re.search(r"#define PCMI_SEG_FLAG_CROP 8\b", open(os.path.join(root, "..", "include", "pcmi.h")).read())
