"""The instance-input kernels (csrc/insseg_input.hip: pcmi_instance_relabel, pcmi_instance_table, pcmi_seg_crop_ladder),
downstream.insseg.InstanceInputPipeline, train_iter_scenes / validate_scenes and the evaluators' table= against
tests/insseg_input_ref.py, which tests/test_insseg_input_ref.py holds to independent spellings.  Everything is integer
arithmetic, so every comparison is exact.  Shapes are the smallest that reach each path: one row, a wave +- 1, the rows of one
workgroup of the numbering scan +- 1 (PF.ROW_SCAN_BLOCK), the start of its second level +- 1 (PF.ROW_SCAN_LEVEL), 70 001 rows."""
import ctypes as C

import numpy as np
import pytest
import torch

import insseg_input_ref as ir
from c_contract import DEV, Guarded, PCMI_ERR_INVALID, PCMI_ERR_WORKSPACE, PCMI_OK

pytestmark = pytest.mark.gpu
POISON = -0x5A5A5A5B


@pytest.fixture(scope="module")
def PF():
  from pointcontrast_amd import functional as pf
  return pf


def _dev(a, dtype=None):
  t = torch.from_numpy(np.ascontiguousarray(a))
  return (t if dtype is None else t.to(dtype)).to(DEV)


def _offs(sizes):
  return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


# ---- relabel --------------------------------------------------------------------------------------------------------------------
def check_relabel(PF, raw, sizes, keep=None, what=""):
  raw, offs = np.asarray(raw, np.int32).reshape(-1), _offs(sizes)
  want = ir.instance_relabel(raw, offs, keep)
  got = PF.instance_relabel(_dev(raw), _dev(offs), None if keep is None else _dev(np.asarray(keep, np.uint8)))
  counts = got["counts"].cpu().numpy()
  assert np.array_equal(counts, want[2]), "%s: counts %s, want %s" % (what, counts, want[2])
  assert np.array_equal(got["instance"].cpu().numpy(), want[0]), "%s: instance differs" % what
  assert np.array_equal(got["first_row"][:int(counts[-1])].cpu().numpy(), want[1]), "%s: first_row differs" % what
  return want


def test_relabel_no_rows(PF):
  got = PF.instance_relabel(torch.zeros(0, dtype=torch.int32, device=DEV), _dev(_offs([0, 0])))
  assert got["counts"].tolist() == [0, 0, 0] and got["instance"].shape == (0,)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_relabel_sizes_around_the_wave(PF, n):
  rng = np.random.RandomState(n)
  check_relabel(PF, rng.randint(-1, 5, size=n), [n // 2, n - n // 2], rng.rand(n) < 0.9, what="n = %d" % n)


def test_relabel_sizes_around_the_scan_workgroup_and_its_second_level(PF):
  block, level = PF.ROW_SCAN_BLOCK, PF.ROW_SCAN_LEVEL
  assert (block, level) == (2048, 256 * 2048)
  rng = np.random.RandomState(5)
  for n in (block - 1, block, block + 1, level - 1, level, level + 1):
    # every 3rd row begins an instance of its own, the rest share 40 ids: the scan carries counts across every workgroup
    raw = np.where(np.arange(n) % 3 == 0, 1000 + np.arange(n), rng.randint(0, 40, size=n))
    inst, first, counts = check_relabel(PF, raw, [n // 3, n - n // 3], what="n = %d" % n)
    assert counts[-1] > n // 3 and inst[n - 1] >= 0


def test_relabel_70001_rows_singletons_and_two_interleaved_ids(PF):
  n = 70001
  inst, first, counts = check_relabel(PF, np.arange(n), [30001, 40000], what="singletons")
  assert counts.tolist() == [30001, 40000, n] and np.array_equal(inst, np.arange(n)) and np.array_equal(first, np.arange(n))
  inst, first, counts = check_relabel(PF, np.arange(n) % 2 * 9, [n], what="two interleaved ids")
  assert counts.tolist() == [2, 2] and first.tolist() == [0, 1] and np.array_equal(inst, np.arange(n) % 2)


def test_relabel_scenes_extreme_ids_mask_and_colliding_probes(PF):
  raw = [7, 7, 0, 2**31 - 1, -1, 0, -100, -2**31] + [0, 7, 7]
  inst, first, counts = check_relabel(PF, raw, [8, 0, 3], what="B = 3, the middle scene empty, the same ids in the outer two")
  assert inst.tolist() == [0, 0, 1, 2, -1, 1, -1, -1, 3, 4, 4] and counts.tolist() == [3, 0, 2, 5]
  inst, first, _ = check_relabel(PF, [5, 6, 5], [3], [0, 1, 1], what="keep removes an instance's lowest row")
  assert inst.tolist() == [-1, 0, 1] and first.tolist() == [1, 2]
  ids = np.arange(2048, dtype=np.int64) << 20  # every non-negative int32 multiple of 2^20, in two scenes: 4 096 keys, each twice
  inst, _, counts = check_relabel(PF, np.concatenate([ids, ids[::-1], ids[::-1], ids]), [4096, 4096], what="multiples of 2^20")
  assert counts.tolist() == [2048, 2048, 4096]


def test_relabel_rows_beyond_the_last_offset_stay_poison_and_two_runs_agree():
  from pointcontrast_amd._lib import lib
  n, used = 5000, 3333
  rng = np.random.RandomState(2)
  raw = _dev(rng.randint(-1, 30, size=n).astype(np.int32))
  raw[used:] = POISON
  offs = _dev(np.array([0, 1500, used], np.int64))
  p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
  st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
  runs = []
  for _ in range(2):
    inst, first = (torch.full((n,), POISON, dtype=torch.int32, device=DEV) for _ in range(2))
    counts = torch.empty(3, dtype=torch.int64, device=DEV)
    g = Guarded(lib.pcmi_instance_relabel_workspace_bytes(n))
    assert lib.pcmi_instance_relabel(p(raw), None, p(offs), n, 2, p(inst), p(first), p(counts), g.vp, g.size, st) == PCMI_OK
    torch.cuda.synchronize()
    g.check("instance_relabel")
    runs.append((inst.cpu().numpy(), first.cpu().numpy(), counts.cpu().numpy()))
  want = ir.instance_relabel(raw.cpu().numpy(), np.array([0, 1500, used]))
  G = int(want[2][-1])
  inst, first, counts = runs[0]
  assert np.array_equal(counts, want[2]) and np.array_equal(inst[:used], want[0][:used]) and np.array_equal(first[:G], want[1])
  assert (inst[used:] == POISON).all() and (first[G:] == POISON).all(), "rows beyond offsets[B] are not written"
  assert all(np.array_equal(a, b) for a, b in zip(*runs)), "two runs differ"


# ---- table ----------------------------------------------------------------------------------------------------------------------
def check_table(PF, inst, klass, coords, sizes, G, what=""):
  offs = _offs(sizes)
  want = ir.instance_table(inst, klass, coords, offs, G)
  got = PF.instance_table(_dev(np.asarray(inst, np.int32)), None if klass is None else _dev(np.asarray(klass, np.int32)),
                          None if coords is None else _dev(np.asarray(coords, np.int32)), _dev(offs), G)
  for k, w in want.items():
    assert (got[k] is None) == (w is None) and (w is None or np.array_equal(got[k].cpu().numpy(), w)), "%s: %s differs" % (what, k)
  return want, got


@pytest.mark.parametrize("G", [0, 1, 65])
def test_table_random_ids_outside_the_range_and_instances_without_rows(PF, G):
  rng = np.random.RandomState(G)
  n = 3000
  inst = np.sort(rng.randint(-1, G + 1, size=n))  # -1 and G count nowhere
  inst[::7] = rng.randint(-1, G + 1, size=len(inst[::7]))  # waves that hold more than one id
  if G == 65:
    inst[inst == 17] = 18                          # an instance without rows
  klass = rng.choice([-5, 0, 3, 2**31 - 1], size=n)
  coords = np.concatenate([np.zeros((n, 1), np.int64), rng.randint(0, 500, size=(n, 3))], 1)
  want, got = check_table(PF, inst, klass, coords, [1000, 0, 2000], G, what="G = %d" % G)
  if G == 65:
    assert want["size"][17] == 0 and want["scene"][17] == -1 and want["box_min"][17].tolist() == [ir.INT32_MAX] * 3
  s, cnt = PF.instance_centroids(_dev(coords.astype(np.int32)), _dev(inst.astype(np.int32)), G)
  assert torch.equal(got["sum"], s) and torch.equal(got["size"].to(torch.int64), cnt), "sum / size are instance_centroids'"
  check_table(PF, inst, None, None, [1000, 0, 2000], G, what="G = %d without klass and coords" % G)


def test_table_classes_and_sums_past_32_bits(PF):
  want, _ = check_table(PF, [0, 0, 1, 1, 2, 2], [-5, -7, 0, -3, 4, 2**31 - 1], None, [6], 3, what="klass -5, 0, 2^31 - 1; two classes in one")
  assert want["cls"].tolist() == [-1, 0, 2**31 - 1]
  n = 4096
  coords = np.zeros((n, 4), np.int64)
  coords[:, 1], coords[:, 2] = 2**20 - 1, np.arange(n) % 2 * (2**20 - 1)
  want, _ = check_table(PF, np.zeros(n, np.int64), np.ones(n), coords, [n], 1, what="4 096 rows at 2^20 - 1")
  assert want["sum"][0].tolist() == [n * (2**20 - 1), n // 2 * (2**20 - 1), 0] and want["sum"][0, 0] > 2**31, "past what an int32 holds"


# ---- crop -----------------------------------------------------------------------------------------------------------------------
def check_crop(PF, coords, sizes, axes, sides, draws, max_voxels, what=""):
  coords, offs = np.asarray(coords, np.int32).reshape(-1, 4), _offs(sizes)
  draws = np.asarray(draws, np.int64).reshape(len(sizes), -1, 2)
  want = ir.seg_crop_ladder(coords, offs, axes, sides, draws, max_voxels)
  got = PF.seg_crop_ladder(_dev(coords), _dev(offs), axes, sides, _dev(draws), max_voxels)
  counts = got["counts"].cpu().numpy()
  assert np.array_equal(counts, want[1]), "%s: counts %s, want %s" % (what, counts, want[1])
  rows = got["rows"][:int(counts[-1])].cpu().numpy()
  assert np.array_equal(rows, want[0]) and (np.diff(rows) > 0).all(), "%s: rows differ" % what
  assert np.array_equal(got["step"].cpu().numpy(), want[2]), "%s: step %s, want %s" % (what, got["step"].cpu().numpy(), want[2])
  assert np.array_equal(got["flags"].cpu().numpy(), want[3]), "%s: flags" % what
  return want


def _lattice(w, h, b=0):
  y, x = np.divmod(np.arange(w * h), w)
  return np.stack([np.full_like(x, b), x, y, np.zeros_like(x)], 1)


def test_crop_at_max_voxels_and_one_above_and_the_planted_ladder(PF):
  c = _lattice(10, 10)
  rows, counts, step, _ = check_crop(PF, c, [100], (1, 2), [[5, 5]], np.zeros((1, 1, 2)), 100, what="exactly max_voxels")
  assert step.tolist() == [-1] and np.array_equal(rows, np.arange(100))
  _, counts, step, _ = check_crop(PF, c, [100], (1, 2), [[5, 5]], np.zeros((1, 1, 2)), 99, what="max_voxels + 1")
  assert step.tolist() == [0] and counts.tolist() == [25, 25]
  _, counts, step, fl = check_crop(PF, c, [100], (1, 2), [[10, 9], [10, 8]], np.zeros((1, 2, 2)), 89, what="step 0 counts max + 1")
  assert step.tolist() == [1] and counts.tolist() == [80, 80] and not fl.any()
  _, counts, step, fl = check_crop(PF, c, [100], (1, 2), [[10, 9], [10, 8]], np.zeros((1, 2, 2)), 90, what="step 0 counts max")
  assert step.tolist() == [0] and counts.tolist() == [90, 90]


def test_crop_no_step_fits_sets_the_flag_and_the_message_names_it(PF):
  _, counts, step, fl = check_crop(PF, _lattice(10, 10), [100], (1, 2), [[10, 9], [10, 8]], np.zeros((1, 2, 2)), 50, what="no step fits")
  assert step.tolist() == [1] and counts.tolist() == [80, 80] and fl.tolist() == [PF.SEG_FLAG_CROP] and PF.SEG_FLAG_CROP == 8
  assert "scene 0" in PF.seg_flags_message(fl) and "crop ladder" in PF.seg_flags_message(fl)


def test_crop_extreme_draws_large_sides_and_ladder_lengths(PF):
  c, full = _lattice(10, 10), 2**32 - 1
  rows, counts, _, _ = check_crop(PF, c, [100], (1, 2), [[4, 4]], [[[full, 0]]], 16, what="draws 2^32 - 1 and 0")
  assert counts.tolist() == [16, 16] and c[rows][:, 1:3].min(0).tolist() == [6, 0] and c[rows][:, 1:3].max(0).tolist() == [9, 3]
  _, counts, step, _ = check_crop(PF, c, [100], (2, 1), [[50, 3]], [[[full, full]]], 30, what="a side larger than the extent")
  assert counts.tolist() == [30, 30] and step.tolist() == [0]
  rng = np.random.RandomState(4)
  n = 5000
  coords = np.concatenate([np.repeat([0, 2], [3000, 2000])[:, None], rng.randint(0, 64, size=(n, 3))], 1)
  sides32 = np.stack([np.arange(64, 0, -2), np.arange(64, 32, -1)], 1)
  for S in (1, 32):  # B = 3 with the middle scene empty; one scene below max_voxels, one above
    want = check_crop(PF, coords, [3000, 0, 2000], (1, 3), sides32[:S], rng.randint(0, 2**32, size=(3, S, 2), dtype=np.int64), 2500,
                      what="S = %d" % S)
    assert want[2][1] == -1 and want[2][2] == -1 and want[2][0] >= 0
  # scenes smaller than a wave and more scenes than a workgroup gathers in LDS
  sizes = [40, 3, 70, 0, 90, 33, 64, 200]
  coords = np.concatenate([np.repeat(np.arange(8), sizes)[:, None], rng.randint(0, 12, size=(sum(sizes), 3))], 1)
  check_crop(PF, coords, sizes, (1, 2), [[8, 8], [5, 5], [2, 2]], rng.randint(0, 2**32, size=(8, 3, 2), dtype=np.int64), 30, what="8 small scenes")


# ---- C contract -----------------------------------------------------------------------------------------------------------------
def test_c_contract_exact_workspaces_and_refusals():
  from pointcontrast_amd._lib import lib
  rng = np.random.RandomState(1)
  n, B, S = 777, 3, 3
  offs = _dev(_offs([300, 0, 477]))
  raw, coords = _dev(rng.randint(-1, 9, size=n).astype(np.int32)), _dev(rng.randint(0, 30, size=(n, 4)).astype(np.int32))
  inst, first = torch.empty(n, dtype=torch.int32, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV)
  counts, flags = torch.empty(B + 1, dtype=torch.int64, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
  rows, step = torch.zeros(n, dtype=torch.int64, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV)
  draws = _dev(rng.randint(0, 2**31, size=(B, S, 2)).astype(np.int32))
  sides = (C.c_int32 * 6)(20, 20, 10, 10, 5, 5)
  p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
  st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

  def relabel(ws, size, n_=n, B_=B):
    return lib.pcmi_instance_relabel(p(raw), None, p(offs), n_, B_, p(inst), p(first), p(counts), ws, size, st)

  def crop(ws, size, n_=n, B_=B, S_=S, a0=1, a1=2, sd=sides, mv=100):
    return lib.pcmi_seg_crop_ladder(p(coords), p(offs), n_, B_, a0, a1, sd, S_, p(draws), mv, p(rows), p(counts), p(step), p(flags), ws, size, st)

  for call, query in ((relabel, lib.pcmi_instance_relabel_workspace_bytes(n)), (crop, lib.pcmi_seg_crop_ladder_workspace_bytes(n, B))):
    assert query > 0
    g = Guarded(query)
    assert call(g.vp, g.size) == PCMI_OK, call.__name__
    torch.cuda.synchronize()
    g.check(call.__name__)
    assert call(g.vp, C.c_size_t(query - 1)) == PCMI_ERR_WORKSPACE, call.__name__
    assert call(None, g.size) == PCMI_ERR_WORKSPACE, call.__name__
    assert call(g.vp, g.size, -1) == PCMI_ERR_INVALID and call(g.vp, g.size, n, 0) == PCMI_ERR_INVALID, call.__name__
    assert call(g.vp, g.size, n, 1024) == PCMI_ERR_INVALID, call.__name__
  want = ir.seg_crop_ladder(coords.cpu().numpy(), offs.cpu().numpy(), (1, 2), [[20, 20], [10, 10], [5, 5]], draws.cpu().numpy().astype(np.uint32), 100)
  assert np.array_equal(counts.cpu().numpy(), want[1]) and np.array_equal(step.cpu().numpy(), want[2])
  g = Guarded(1 << 20)
  before = (rows.clone(), step.clone())
  assert crop(g.vp, g.size, S_=0) == PCMI_ERR_INVALID and crop(g.vp, g.size, S_=33) == PCMI_ERR_INVALID
  assert crop(g.vp, g.size, a0=2, a1=2) == PCMI_ERR_INVALID and crop(g.vp, g.size, a0=0) == PCMI_ERR_INVALID and crop(g.vp, g.size, a1=4) == PCMI_ERR_INVALID
  assert crop(g.vp, g.size, sd=(C.c_int32 * 6)(20, 20, 0, 10, 5, 5)) == PCMI_ERR_INVALID, "a side 0"
  assert crop(g.vp, g.size, sd=(C.c_int32 * 6)(20, 20, 10, 21, 5, 5)) == PCMI_ERR_INVALID, "a column that increases"
  assert crop(g.vp, g.size, mv=0) == PCMI_ERR_INVALID
  torch.cuda.synchronize()
  assert torch.equal(rows, before[0]) and torch.equal(step, before[1]), "a refused call enqueues nothing"
  assert lib.pcmi_instance_relabel_workspace_bytes(-1) == 0 and lib.pcmi_seg_crop_ladder_workspace_bytes(n, 0) == 0
  assert lib.pcmi_instance_relabel_workspace_bytes((1 << 29) + 1) == 0
  # the table has no workspace: its pairing rule and a G of 0
  size, scene = torch.empty(4, dtype=torch.int32, device=DEV), torch.empty(4, dtype=torch.int32, device=DEV)
  table = lambda kl, cl, G=4: lib.pcmi_instance_table(p(inst), kl, None, p(offs), n, B, G, p(size), p(scene), cl, None, None, None, st)  # noqa: E731
  assert table(None, None) == PCMI_OK and table(p(raw), None) == PCMI_ERR_INVALID and table(None, p(size)) == PCMI_ERR_INVALID
  assert table(None, None, 0) == PCMI_OK and table(None, None, -1) == PCMI_ERR_INVALID


# ---- pipeline -------------------------------------------------------------------------------------------------------------------
def _rooms(seed=11, sizes=(3000, 2900, 3100)):
  """Rooms of a floor (class 1, raw id 0) and 5 boxes of points (classes 2 ... 4, raw ids 3, 5, 8, 9, 12: the same in every room;
  the boxes of room 0 are larger, so it has the most voxels).
  The first two points of room 0 are planted into ONE voxel of the identity-scaled grid but belong to two instances of class 3."""
  rng = np.random.RandomState(seed)
  scenes = []
  for s in sizes:
    xyz = rng.uniform(0, 3, size=(s, 3))
    xyz[:, 2] = rng.uniform(0, 0.05, size=s)
    labels, ids = np.ones(s, np.int32), np.zeros(s, np.int32)
    for k, raw_id in enumerate((3, 5, 8, 9, 12)):
      rows = np.arange(200 + 400 * k, 200 + 400 * (k + 1))
      xyz[rows] = rng.uniform(0, 0.5 if len(scenes) == 0 else 0.3, size=(400, 3)) + [0.55 * k, 1.0, 0.1]
      labels[rows], ids[rows] = 2 + k % 3, raw_id
    scenes.append((xyz, rng.randint(0, 256, size=(s, 3)).astype(np.float32), labels, ids))
  xyz, _, labels, ids = scenes[0]
  xyz[0], xyz[1] = [2.51, 2.52, 0.53], [2.53, 2.51, 0.52]
  labels[:2], ids[:2] = 3, (5, 9)
  return scenes


def _aug(ss, **kw):
  lut = np.arange(6, dtype=np.int32)
  lut[5] = 255
  return ss.SegmentationAugmentation(voxel_size=0.05, label_map=lut, elastic_params=((0.2, 0.4),), **kw)


def _draws(ss, scenes, elastic=True):
  rng = np.random.RandomState(3)
  B, rows = len(scenes), sum(len(s[0]) for s in scenes)
  mats = np.repeat((np.eye(4) * [20.0, 20.0, 20.0, 1.0])[None], B, 0)
  d = ss.AugmentationDraws(mats, flip=[(True, False, False), None, (False, True, False)][:B], contrast=[0.4, None, 0.9][:B],
                           translation=[(10.0, -20.0, 5.0), None, (1.0, 2.0, 3.0)][:B], jitter_std=[0.05, 0.05, None][:B],
                           normals=_dev(rng.randn(rows, 3).astype(np.float32)))
  noise, keys = rng.randn(B, 20, 20, 8, 3).astype(np.float32), rng.rand(rows).astype(np.float32)
  if elastic:
    d.elastic_on, d.elastic_noise = [True, False, True][:B], [_dev(noise)]
    d.dropout_on, d.dropout_keys = [False, True, True][:B], _dev(keys)
  return d, noise, keys


CROP = ([[48, 48], [40, 40], [30, 30], [20, 20]], 2100)


def _want(PF, ss, scenes, d, noise, keys, crop, crop_draws, limit, elastic=True):
  params = PF.seg_color_params(len(scenes), d.flip, d.contrast, d.translation, d.jitter_std)
  return ir.pipeline(scenes, d.mats, None, None, params, d.normals.cpu().numpy(), True, _aug(ss).label_map, 255, limit,
                     elastic=[(0.2, 0.4, noise, [1, 0, 1])] if elastic else None, dropout_keys=(keys, d.dropout_on) if elastic else None,
                     stuff_classes=(0, 1), crop=crop, crop_draws=crop_draws)


def _same(got, want):
  coords, feats, target, instance, G, transformation = got
  assert np.array_equal(coords.cpu().numpy(), want[0]) and np.array_equal(target.cpu().numpy(), want[2]), "coords / target differ"
  assert np.array_equal(feats.cpu().numpy().view(np.int32), want[1].view(np.int32)), "feats differ"
  assert np.array_equal(instance.cpu().numpy(), want[3]) and G == want[4], "instance differs (%d instances, want %d)" % (G, want[4])
  assert np.array_equal(transformation.cpu().numpy().view(np.int64), want[5].view(np.int64)), "transformation differs"


def test_pipeline_against_the_restatement_with_elastic_dropout_crop_and_limit(PF):
  from pointcontrast_amd.downstream import insseg as iseg, semseg as ss
  scenes = _rooms()
  d, noise, keys = _draws(ss, scenes)
  crop_draws = iseg.InstanceInputPipeline.sample_crop_draws(CROP, 3, np.random.RandomState(9))
  full = _want(PF, ss, scenes, d, noise, keys, None, None, 0)
  counts = np.bincount(full[0][:, 0], minlength=3)
  assert counts[0] > CROP[1] and counts[1] <= CROP[1], "the crop bites in scene 0 only (scene 1 loses a fifth of its rows to dropout later)"
  pipe = iseg.InstanceInputPipeline(_aug(ss), DEV, crop=CROP)
  for limit in (0, None):
    if limit is None:  # the third scene exceeds the limit and is dropped, with its instances
      limit, all_instances = len(want[0]) - 10, want[4]
    want = _want(PF, ss, scenes, d, noise, keys, CROP, crop_draws, limit)
    assert not want[6].any() and want[7][0] >= 0 and (want[7][1:] == -1).all() and len(want[5]) == (3 if limit == 0 else 2)
    got = pipe(scenes, d, limit, crop_draws)
    _same(got, want)
    assert np.array_equal(pipe.last_crop_step, want[7])
    assert (got[4] > 10 if limit == 0 else got[4] == all_instances - 5) and int(got[3].max()) < got[4]
    again = pipe(scenes, d, limit, crop_draws)
    assert all(torch.equal(a, b) for a, b in zip(got[:4], again[:4])) and got[4] == again[4], "two runs differ"
  with pytest.raises(AssertionError):
    pipe(scenes, d, 0, None)
  with pytest.raises(ValueError, match="scene 0.*crop ladder"):
    iseg.InstanceInputPipeline(_aug(ss), DEV, crop=([[48, 48]], 1000))(scenes, d, 0, crop_draws[:, :1])


def test_pipeline_straddling_voxel_and_equality_with_the_semantic_pipeline(PF):
  from pointcontrast_amd.downstream import insseg as iseg, semseg as ss
  scenes = _rooms()
  aug = _aug(ss, augment=False)
  coords, feats, target, instance, G, transformation = iseg.InstanceInputPipeline(aug, DEV)(scenes)
  c = coords.cpu().numpy()
  row = np.flatnonzero((c == [0, 50, 50, 10]).all(1))
  assert len(row) == 1 and int(instance[row[0]]) == -1 and int(target[row[0]]) == 3, "two instances of one class in one voxel"
  assert G == 15 and (instance[(target == 1) | (target == 255)] == -1).all()
  d, _, _ = _draws(ss, scenes, elastic=False)
  for limit in (0, len(c) - 5):
    got = iseg.InstanceInputPipeline(_aug(ss), DEV)(scenes, d, limit)
    sem = ss.SegmentationInputPipeline(_aug(ss), DEV)([s[:3] for s in scenes], d, limit)
    assert all(torch.equal(a, b) for a, b in zip((got[0], got[1], got[2], got[5]), sem)), "limit %d" % limit
    _same(got, _want(PF, ss, scenes, d, None, None, None, None, limit, elastic=False))


def test_pipeline_reads_back_once(PF):
  """Every host-to-device copy of a batch is in stage_upload and its one device-to-host copy in stage_read_back: the stages
  between and after them run with torch's synchronisation check set to raise, so no output waits for a second read."""
  from pointcontrast_amd.downstream import insseg as iseg, semseg as ss
  scenes = _rooms()
  d, noise, keys = _draws(ss, scenes)
  crop_draws = iseg.InstanceInputPipeline.sample_crop_draws(CROP, 3, np.random.RandomState(9))
  pipe = iseg.InstanceInputPipeline(_aug(ss), DEV, crop=CROP)
  want = pipe(scenes, d, 0, crop_draws)  # (also warms the allocator)
  st = pipe.stage_upload(scenes, d, crop_draws=crop_draws)
  torch.cuda.synchronize()
  mode = torch.cuda.get_sync_debug_mode()
  try:
    torch.cuda.set_sync_debug_mode("error")
    pipe.stage_voxelize(st)
    pipe.stage_instances(st)
    torch.cuda.set_sync_debug_mode(mode)
    counts, tail = pipe.stage_read_back(st, st["read"])
    torch.cuda.set_sync_debug_mode("error")
    got = pipe.stage_finish(st, counts, tail, 0)
  finally:
    torch.cuda.set_sync_debug_mode(mode)
  assert all(torch.equal(a, b) for a, b in zip(got[:4], want[:4])) and got[4] == want[4] and torch.equal(got[5], want[5])
  with pytest.raises(RuntimeError):  # the check is live: a read inside the guarded region raises
    try:
      torch.cuda.set_sync_debug_mode("error")
      got[0].cpu()
    finally:
      torch.cuda.set_sync_debug_mode(mode)


# ---- trainer and evaluators -----------------------------------------------------------------------------------------------------
def _trainer(seed, pipe):
  from pointcontrast_amd.downstream.insseg import InstanceSegmentationTrainer
  torch.manual_seed(seed)
  return InstanceSegmentationTrainer(5, model="Res16UNet14", lr=0.05, max_iter=50, voxel_size=0.05, radius=0.08, min_points=20,
                                     input_pipeline=pipe)


def test_train_iter_scenes_is_deterministic_and_validate_scenes_equals_the_loop(PF):
  from pointcontrast_amd.downstream import insseg as iseg, semseg as ss
  scenes = _rooms()
  d, _, _ = _draws(ss, scenes)
  crop_draws = iseg.InstanceInputPipeline.sample_crop_draws(CROP, 3, np.random.RandomState(9))
  a, b = (_trainer(3, iseg.InstanceInputPipeline(_aug(ss), DEV, crop=CROP)) for _ in range(2))
  for _ in range(2):
    ra, rb = a.train_iter_scenes(scenes, d, 0, crop_draws), b.train_iter_scenes(scenes, d, 0, crop_draws)
    assert np.isfinite(float(ra["loss"])) and float(ra["loss"]) == float(rb["loss"]) and ra["transformation"].shape == (3, 16)
    assert float(ra["loss_norm"]) > 0, "the batch carries instances"
  for (name, pa), (_, pb) in zip(a.model.named_parameters(), b.model.named_parameters()):
    assert torch.equal(pa, pb), name
  batches = [scenes[:2], scenes[2:]]
  pipe = iseg.InstanceInputPipeline(_aug(ss, augment=False), DEV)
  for benchmark, cls in ((False, iseg.InstanceEvaluator), (True, iseg.InstanceBenchmarkEvaluator)):
    got = a.validate_scenes(batches, benchmark=benchmark)
    assert isinstance(a.instance_evaluator, cls)
    ev = cls(5, a.stuff_classes, device=DEV)
    for batch in batches:
      coords, feats, target, instance, G, _ = pipe(batch)
      ev.step(a.predict(coords, feats), instance, target, G)
    want = ev.compute_metrics()
    assert set(got) == set(want)
    for k in want:
      assert np.array_equal(np.asarray(got[k]), np.asarray(want[k]), equal_nan=True), (benchmark, k)
    assert benchmark or want["n_gt"].tolist() == [0, 0, 6, 6, 3]


def test_evaluators_with_and_without_the_table_are_bit_identical(PF):
  """Six ground-truth instances in two scenes, one of a stuff class and one id without rows; the prediction merges, drops and
  halves some of them."""
  from pointcontrast_amd.downstream import insseg as iseg
  sizes = [400, 300, 500, 350, 450, 250]
  gt = np.repeat([0, 1, 2, 3, 5, 6], sizes)  # id 4 has no rows
  n, G = len(gt), 7
  gt_cls = np.repeat([2, 2, 3, 1, 3, 3], sizes)
  gt_cls[:5] = 3                                 # two classes in one instance: the larger one counts
  offs = _dev(np.array([0, 1200, n], np.int64))
  pred = gt.copy()
  pred[gt == 1], pred[gt == 2] = 0, -1
  pred[np.flatnonzero(gt == 5)[::2]] = -1
  P = 8
  rng = np.random.RandomState(0)
  pd = dict(instance=_dev(pred.astype(np.int32)), inst_class=_dev(np.array([2, -1, -1, 1, -1, 3, 3, -1], np.int32)),
            inst_size=_dev(np.bincount(pred[pred >= 0], minlength=P).astype(np.int32)),
            inst_scene=_dev(np.array([0, -1, -1, 1, -1, 1, 1, -1], np.int32)), inst_score=_dev(rng.rand(P)), scene_offsets=offs)
  table = PF.instance_table(_dev(gt.astype(np.int32)), _dev(gt_cls.astype(np.int32)), None, offs, G)
  assert table["cls"].tolist() == [3, 2, 3, 1, -1, 3, 3] and table["scene"].tolist() == [0, 0, 0, 1, -1, 1, 1]
  for cls, kw in ((iseg.InstanceEvaluator, {}), (iseg.InstanceBenchmarkEvaluator, dict(min_region=100))):
    out = []
    for tb in (None, table):
      ev = cls(4, (0, 1), device=DEV, **kw)
      ev.step(pd, gt, gt_cls, G, table=tb)
      ev.step(pd, gt, gt_cls, G, table=tb)
      out.append(ev.compute_metrics())
    assert np.isfinite(out[0]["AP"]) and out[0]["n_gt"].sum() > 0
    for k in out[0]:
      a, b = np.atleast_1d(out[0][k]), np.atleast_1d(out[1][k])  # floats as their bits: a NaN equals itself
      assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (cls.__name__, k)


def test_batch_instance_ids(PF):
  from pointcontrast_amd.downstream.insseg import batch_instance_ids
  per_scene, G = batch_instance_ids([np.array([4, 4, -1, 9]), np.array([], np.int64), np.array([9, 4, 9])], DEV)
  assert [p.tolist() for p in per_scene] == [[0, 0, -1, 1], [], [2, 3, 2]] and G == 4 and per_scene[0].dtype == np.int32
