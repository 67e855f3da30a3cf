"""The segmentation input kernels (csrc/semseg_input.hip: pcmi_elastic_blur, pcmi_elastic_apply, pcmi_seg_transform,
pcmi_seg_quantize, pcmi_seg_color_augment) and
downstream.semseg.SegmentationInputPipeline against tests/semseg_input_ref.py, which tests/test_semseg_input_ref.py holds to
the reference's Voxelizer and transforms.  The arithmetic is fixed, so every comparison is BIT-exact (floats as their integer
bit patterns).  Shapes are the smallest that reach each path: one row, a partial wave, 255 / 256 / 257 rows around the
workgroup, 1023 / 1025, and 70 000 rows for the multi-workgroup scan."""
import ctypes as C

import numpy as np
import pytest
import torch

import semseg_input_ref as sr
from c_contract import DEV, Guarded, PCMI_ERR_INVALID, PCMI_ERR_WORKSPACE, PCMI_OK

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def PF():
  from pointcontrast_amd import functional as pf
  return pf


def _dev(a, dtype=None):
  t = torch.from_numpy(np.ascontiguousarray(a))
  return (t if dtype is None else t.to(dtype)).to(DEV)


def _bits(a, dtype):
  a = np.ascontiguousarray(a, dtype=dtype)
  return a.view(np.int64 if dtype == np.float64 else np.int32)


def _offs(sizes):
  return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


# ---- quantize -------------------------------------------------------------------------------------------------------------------
def check_quantize(PF, vox, sizes, labels=None, keep=None, scene_min=None, ignore=255, what=""):
  vox = np.asarray(vox, np.int32).reshape(-1, 3)
  offs = _offs(sizes)
  want = sr.seg_quantize(vox, offs, labels, keep, scene_min, ignore)
  got = PF.seg_quantize(_dev(vox), _dev(offs), None if labels is None else _dev(np.asarray(labels, np.int32)),
                        None if keep is None else _dev(np.asarray(keep, np.uint8)),
                        None if scene_min is None else _dev(np.asarray(scene_min, np.int32)), ignore)
  counts = got["counts"].cpu().numpy()
  assert np.array_equal(counts, want[3]), "%s: counts %s, want %s" % (what, counts, want[3])
  M = int(counts[-1])
  assert np.array_equal(got["coords"][:M].cpu().numpy(), want[0]), "%s: coords differ" % what
  assert np.array_equal(got["index"][:M].cpu().numpy(), want[1]), "%s: index differs" % what
  if labels is not None:
    assert np.array_equal(got["labels"][:M].cpu().numpy(), want[2]), "%s: labels differ" % what
  assert np.array_equal(got["flags"].cpu().numpy(), want[4]), "%s: flags %s, want %s" % (what, got["flags"].cpu().numpy(), want[4])
  return want


def test_quantize_one_row_and_one_voxel(PF):
  c, ix, lb, cnt, _ = check_quantize(PF, [[3, -4, 5]], [1], [7], scene_min=[[0, -4, 0]], what="n = 1")
  assert c.tolist() == [[0, 3, 0, 5]] and ix.tolist() == [0] and lb.tolist() == [7] and cnt.tolist() == [1, 1]
  c, ix, lb, cnt, _ = check_quantize(PF, [[2, 2, 2]] * 5, [5], [4] * 5, scene_min=[[2, 2, 2]], what="one voxel")
  assert c.tolist() == [[0, 0, 0, 0]] and ix.tolist() == [0] and lb.tolist() == [4]


def test_quantize_empty_scene_between_and_identical_scenes(PF):
  pts = [[0, 0, 0], [1, 0, 0], [0, 0, 0], [5, 5, 5]]
  c, ix, lb, cnt, _ = check_quantize(PF, pts + pts, [4, 0, 4], [1, 2, 1, 3] * 2, what="empty scene, identical scenes")
  assert cnt.tolist() == [3, 0, 3, 6]
  assert c[:, 0].tolist() == [0, 0, 0, 2, 2, 2] and np.array_equal(c[:3, 1:], c[3:, 1:]) and ix.tolist() == [0, 1, 3, 4, 5, 7]


def test_quantize_label_rule(PF):
  a, b, ig = 3, 9, 255
  vox = [[0, 0, 0]] * 3 + [[1, 0, 0]] * 2 + [[2, 0, 0]] * 2 + [[3, 0, 0]]
  _, _, lb, _, _ = check_quantize(PF, vox, [8], [a, b, a, a, a, ig, a, b], ignore=ig, what="label rule")
  assert lb.tolist() == [ig, a, ig, b]  # (a, b, a) -> ignore; (a, a) -> a; (ignore, a) -> ignore; a single row keeps its label
  check_quantize(PF, vox, [8], None, what="no labels")


@pytest.mark.parametrize("n", [255, 256, 257, 1023, 1025])
def test_quantize_sizes_around_the_workgroup(PF, n):
  rng = np.random.RandomState(n)
  sizes = [n // 3, n - n // 3 - 7, 7]
  vox = rng.randint(-6, 6, size=(n, 3))
  keep = (rng.rand(n) < 0.9).astype(np.uint8)
  mins = np.full((3, 3), -6)
  check_quantize(PF, vox, sizes, rng.randint(0, 3, size=n), keep, mins, what="n = %d" % n)


def test_quantize_70000_rows_cross_the_multi_workgroup_scan(PF):
  rng = np.random.RandomState(7)
  n = 70000
  vox = rng.randint(0, 40, size=(n, 3))
  _, _, _, cnt, _ = check_quantize(PF, vox, [30001, 39999], rng.randint(0, 2, size=n), what="n = 70000")
  assert cnt[-1] > 30000


def test_quantize_span_flag_and_pipeline_range_error(PF):
  from pointcontrast_amd.downstream import semseg as ss
  c, _, _, cnt, fl = check_quantize(PF, [[0, 0, 0], [1 << 18, 0, 0], [(1 << 18) - 1, 0, 0]], [3], [1, 1, 1], what="span")
  assert fl.tolist() == [sr.FLAG_SPAN] and cnt.tolist() == [2, 2]
  # a coordinate past 2^20 voxels: the transform flags the scene, the pipeline raises and names it
  aug = ss.SegmentationAugmentation(voxel_size=1.0, augment=False, normalize_color=False)
  ok = (np.zeros((2, 3)), np.zeros((2, 3), np.float32), np.zeros(2, np.int32))
  far = (np.array([[0.5, 0.5, 0.5], [float(1 << 20) + 0.5, 0.5, 0.5]]), np.zeros((2, 3), np.float32), np.zeros(2, np.int32))
  with pytest.raises(ValueError, match="scene 1.*2\\^20"):
    ss.SegmentationInputPipeline(aug, DEV)([ok, far])


# ---- transform and clip ---------------------------------------------------------------------------------------------------------
def check_transform(PF, xyz, sizes, mats, clip=None, ratio=None, what=""):
  xyz, offs = np.asarray(xyz, np.float64).reshape(-1, 3), _offs(sizes)
  want = sr.seg_transform(xyz, offs, mats, clip, ratio)
  got = PF.seg_transform(_dev(xyz), _dev(offs), _dev(np.asarray(mats, np.float64).reshape(-1, 16)), clip,
                         None if ratio is None else _dev(np.asarray(ratio, np.float64)))
  for name, w in zip(("vox", "keep", "scene_min"), want[:3]):
    assert np.array_equal(got[name].cpu().numpy(), w), "%s: %s differs" % (what, name)
  assert np.array_equal(_bits(got["aligned"].cpu().numpy(), np.float64), _bits(want[3], np.float64)), "%s: aligned differs" % what
  assert np.array_equal(got["flags"].cpu().numpy(), want[4]), "%s: flags differ" % what
  return want


def _rot_scale(theta, s, t=(0.3, -0.7, 0.2)):
  M = np.eye(4)
  M[:3, :3] = s * np.array([[np.cos(theta), -np.sin(theta), 0], [np.sin(theta), np.cos(theta), 0], [0, 0, 1]])
  M[:3, 3] = t
  return M


def test_transform_identity_and_negative_coordinates(PF):
  xyz = [[0.5, 1.5, 2.5], [-0.5, -1.25, 7.0], [-3.0, 0.0, -0.0]]
  vox, keep, mn, al, _ = check_transform(PF, xyz, [3], [np.eye(4)], what="identity")
  assert vox.tolist() == [[0, 1, 2], [-1, -2, 7], [-3, 0, 0]] and keep.tolist() == [1, 1, 1] and mn.tolist() == [[-3, -2, 0]]
  assert al.reshape(4, 4)[:3, 3].tolist() == [3.0, 2.0, 0.0]


@pytest.mark.parametrize("n", [1, 63, 257, 1025])
def test_transform_rotated_batches(PF, n):
  rng = np.random.RandomState(n)
  sizes = [n, 0, n + 5]
  xyz = rng.uniform(-4, 4, size=(sum(sizes), 3))
  mats = [_rot_scale(0.3, 20.0), np.eye(4), _rot_scale(-1.1, 50.0)]
  check_transform(PF, xyz, sizes, mats, what="no clip, n = %d" % n)
  check_transform(PF, xyz, sizes, mats, clip=2.5, ratio=rng.uniform(-0.2, 0.2, size=(3, 3)), what="numeric clip, n = %d" % n)
  check_transform(PF, xyz, sizes, mats, clip=((-1.0, 2.0), (-3.0, 0.5), (-9.0, 9.0)), ratio=rng.uniform(-0.2, 0.2, size=(3, 3)),
                  what="per-axis clip, n = %d" % n)


def test_clip_edges(PF):
  # the extent (2) is below the numeric bound 3: nothing is clipped, although a +-3 box around the shifted centre would clip
  xyz = [[0.0, 0.0, 0.0], [2.0, 2.0, 2.0], [1.0, 0.5, 1.5]]
  _, keep, _, _, _ = check_transform(PF, xyz, [3], [np.eye(4)], clip=3, ratio=[[5.0, 0, 0]], what="bound above the extent")
  assert keep.tolist() == [1, 1, 1]
  # extent 8, centre 4, bound 2: kept iff 2 <= p < 6 on every axis -- a point exactly on the upper bound is excluded
  xyz = [[0.0, 0.0, 0.0], [8.0, 8.0, 8.0], [2.0, 2.0, 2.0], [6.0, 3.0, 3.0], [5.5, 5.5, 2.0]]
  _, keep, mn, _, _ = check_transform(PF, xyz, [5], [np.eye(4)], clip=2, what="upper bound excluded")
  assert keep.tolist() == [0, 0, 1, 0, 1] and mn.tolist() == [[2, 2, 2]]
  # clipped empty (per-axis bounds that hold no point): minimum 0, the matrix unchanged, no flag; and it quantizes to nothing
  vox, keep, mn, al, fl = check_transform(PF, xyz, [2, 3], [np.eye(4)] * 2, clip=((100.0, 101.0),) * 3, what="clipped empty")
  assert keep.sum() == 0 and mn.tolist() == [[0, 0, 0]] * 2 and fl.tolist() == [0, 0]
  _, _, _, cnt, _ = check_quantize(PF, vox, [2, 3], [1] * 5, keep, mn, what="nothing kept")
  assert cnt.tolist() == [0, 0, 0]


def test_transform_flags_non_finite_and_far_points(PF):
  xyz = [[0.5, 0.5, 0.5], [np.nan, 0.0, 0.0], [1.5, 0.5, 0.5], [float(1 << 20), 0.0, 0.0], [-float(1 << 20) + 1.5, 0.0, 0.0]]
  _, keep, _, _, fl = check_transform(PF, xyz, [1, 2, 2], [np.eye(4)] * 3, what="range")
  assert keep.tolist() == [1, 0, 1, 0, 1] and fl.tolist() == [0, 1, 1]


# ---- colour, flip, label map ----------------------------------------------------------------------------------------------------
def check_color(PF, feats, coords, B, index=None, labels=None, params=None, normals=None, normalize=False, lut=None, what=""):
  want_c, want_f, want_l = sr.seg_color_augment(feats, coords, B, index, labels, params, normals, normalize, lut, 255)
  c = _dev(np.asarray(coords, np.int32))
  lb = None if labels is None else _dev(np.asarray(labels, np.int32))
  out = PF.seg_color_augment(_dev(np.asarray(feats, np.float32)), c, B, None if index is None else _dev(np.asarray(index, np.int64)), lb,
                             None if params is None else _dev(np.asarray(params, np.float64)),
                             None if normals is None else _dev(np.asarray(normals, np.float32)), normalize,
                             None if lut is None else _dev(np.asarray(lut, np.int32)), 255)
  assert np.array_equal(c.cpu().numpy(), want_c), "%s: coords differ" % what
  assert np.array_equal(_bits(out.cpu().numpy(), np.float32), _bits(want_f.astype(np.float32), np.float32)), "%s: feats differ" % what
  if labels is not None:
    assert np.array_equal(lb.cpu().numpy(), want_l), "%s: labels differ" % what
  return want_c, want_f, want_l


def _voxels(rng, sizes):
  return np.concatenate([np.concatenate([np.full((s, 1), b), rng.randint(0, 50, size=(s, 3))], 1) for b, s in enumerate(sizes)]).astype(np.int32)


@pytest.mark.parametrize("blend", [0.0, 1.0, 0.37])
def test_auto_contrast_blend(PF, blend):
  rng = np.random.RandomState(11)
  sizes = [70, 300]
  coords, feats = _voxels(rng, sizes), rng.randint(20, 200, size=(370, 3)).astype(np.float32)
  feats[:70, 1] = 88.0  # hi == lo in scene 0, channel 1: the channel is left as it is
  P = PF.seg_color_params(2, contrast=[blend, blend])
  _, f, _ = check_color(PF, feats, coords, 2, params=P, what="blend %g" % blend)
  assert np.array_equal(f[:70, 1], feats[:70, 1].astype(np.float64))
  if blend == 0.0:
    assert np.array_equal(f, feats.astype(np.float64))
  if blend == 1.0:
    assert f[70:].min() == 0.0 and abs(f[70:].max() - 255.0) < 1e-9


@pytest.mark.parametrize("m", [1, 64, 257, 1025])
def test_full_colour_chain_flip_and_label_map(PF, m):
  rng = np.random.RandomState(m)
  sizes = [m, 0, m // 2 + 1]
  n = sum(sizes)
  coords = _voxels(rng, sizes)
  src = rng.uniform(0, 255, size=(2 * n, 3)).astype(np.float32)
  index = rng.permutation(2 * n)[:n]
  labels = rng.randint(-1, 8, size=n)
  labels[0] = 255
  lut = np.array([0, 255, 1, 2, 255, 3], np.int32)  # raw 1 and 4 ignored; 6, 7, -1 and 255 fall outside the table -> ignore
  P = PF.seg_color_params(3, flip=[(True, False, False), None, (True, True, False)], contrast=[0.6, None, None],
                          translation=[(60.0, -70.0, 3.5), None, (-300.0, 300.0, 0.0)], jitter_std=[0.05, None, 0.9])
  normals = rng.randn(n, 3).astype(np.float32)
  _, f, lb = check_color(PF, src, coords, 3, index, labels, P, normals, True, lut, what="chain, m = %d" % m)
  assert f.min() >= -0.5 and f.max() <= 0.5
  if m >= 64:
    assert (f == -0.5).any() and (f == 0.5).any()  # both clips were reached
  assert lb[0] == 255 and set(np.unique(lb)) <= {0, 1, 2, 3, 255}
  check_color(PF, src, coords, 3, index, labels, None, None, False, None, what="gather only, m = %d" % m)


# ---- elastic --------------------------------------------------------------------------------------------------------------------
def check_elastic(PF, xyz, sizes, stages, caps, active=None, seed=0, what=""):
  """stages = [(granularity, magnitude)], caps = [(cx, cy, cz)] per stage: the chained stages on the device against the
  restatement -- points, the whole capacity blocks after the blur, grid dims and flags, bit for bit."""
  xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
  offs, B = _offs(sizes), len(sizes)
  rng = np.random.RandomState(seed)
  dev_xyz, dev_offs = _dev(xyz), _dev(offs)
  flags = torch.zeros(B, dtype=torch.int32, device=DEV)
  want_xyz, want_flags, all_dims = xyz, np.zeros(B, np.int32), []
  for (g, mag), cap in zip(stages, caps):
    noise = rng.randn(B, cap[0], cap[1], cap[2], 3).astype(np.float32)
    dev_noise = _dev(noise)
    want_xyz, want_noise, want_dims, f = sr.elastic_stage(want_xyz, offs, g, mag, noise, active)
    want_flags |= f
    grid = PF.elastic_blur(dev_xyz, dev_offs, g, dev_noise, None if active is None else np.asarray(active, np.int32), flags)
    PF.elastic_apply(dev_xyz, dev_offs, g, mag, dev_noise, grid)
    assert np.array_equal(grid["grid_dims"].cpu().numpy(), want_dims), "%s: dims %s, want %s" % (what, grid["grid_dims"].cpu().numpy(), want_dims)
    assert np.array_equal(_bits(dev_noise.cpu().numpy(), np.float32), _bits(want_noise, np.float32)), "%s: blurred blocks differ" % what
    assert np.array_equal(_bits(dev_xyz.cpu().numpy(), np.float64), _bits(want_xyz, np.float64)), "%s: points differ" % what
    all_dims.append(want_dims)
  assert np.array_equal(flags.cpu().numpy(), want_flags), "%s: flags %s, want %s" % (what, flags.cpu().numpy(), want_flags)
  return want_xyz, all_dims, want_flags


def test_elastic_single_point_has_dims_three_at_exact_capacity(PF):
  out, dims, _ = check_elastic(PF, [[0.3, -1.2, 2.0]], [1], [(0.2, 0.4)], [(3, 3, 3)], what="one point")
  assert dims[0].tolist() == [[3, 3, 3, 1]]


@pytest.mark.parametrize("g", [0.25, 0.2])
def test_elastic_extent_an_exact_multiple_of_the_granularity(PF, g):
  rng = np.random.RandomState(1)
  xyz = rng.uniform(0, 1, size=(300, 3)) * [3 * g, 2.5 * g, 2 * g]
  xyz[0], xyz[1] = [0, 0, 0], [3 * g, 2.5 * g, 2 * g]  # the extents are 3 g, 2.5 g and 2 g as numpy rounds them
  want = (((xyz - xyz.min(0)).max(0) // g) + 3).astype(int)
  out, dims, _ = check_elastic(PF, xyz, [300], [(g, 0.4)], [tuple(want)], what="exact multiple, capacity equal to the dims")
  assert dims[0][0, :3].tolist() == want.tolist() and not np.array_equal(out, xyz)


def test_elastic_capacity_one_too_small_flags_the_scene_and_leaves_it(PF):
  rng = np.random.RandomState(2)
  xyz = np.concatenate([rng.uniform(0, 0.5, size=(257, 3)), rng.uniform(0, 1.0, size=(300, 3))])
  # dims (5, 5, 5) and (7, 7, 7) at g = 0.2; the capacity holds the first scene and misses the second by one along y
  out, dims, flags = check_elastic(PF, xyz, [257, 300], [(0.2, 0.4)], [(7, 6, 7)], what="capacity one too small")
  assert flags.tolist() == [0, sr.FLAG_ELASTIC] and dims[0].tolist() == [[5, 5, 5, 1], [0, 0, 0, 0]]
  assert np.array_equal(out[257:], xyz[257:]) and not np.array_equal(out[:257], xyz[:257])


def test_elastic_points_on_nodes_and_on_the_last_node(PF):
  # a hand-made grid, nodes -0.25, 0, 0.25, 0.5 per axis: the last node, inner nodes, the first node, just outside
  p = np.array([[0.5, 0.5, 0.5], [0.25, 0.0, -0.25], [-0.25, -0.25, -0.25], [0.5000001, 0.0, 0.0], [0.0, -0.26, 0.0], [0.1, 0.2, 0.3]])
  noise = np.random.RandomState(3).randn(1, 5, 4, 6, 3).astype(np.float32)
  grid = dict(grid_dims=_dev(np.array([[4, 4, 4, 1]], np.int32)), grid_min=_dev(np.zeros((1, 3))))
  dev = _dev(p)
  PF.elastic_apply(dev, _dev(_offs([6])), 0.25, 2.0, _dev(noise), grid)
  want = sr.elastic_apply_scene(p, noise[0, :4, :4, :4], [0, 0, 0], [4, 4, 4], 0.25, 2.0)
  assert np.array_equal(_bits(dev.cpu().numpy(), np.float64), _bits(want, np.float64))
  assert np.array_equal(want[0], p[0] + noise[0, 3, 3, 3].astype(np.float64) * 2.0) and np.array_equal(want[3:5], p[3:5])


def test_elastic_two_chained_stages_padded_strides_empty_and_inactive_scenes(PF):
  rng = np.random.RandomState(4)
  sizes = [300, 0, 257, 64]
  xyz = rng.uniform(-1, 1, size=(sum(sizes), 3)) * [1.5, 1.0, 0.6]
  out, dims, flags = check_elastic(PF, xyz, sizes, [(0.2, 0.4), (0.8, 1.6)], [(19, 15, 11), (9, 8, 7)], active=[1, 1, 1, 0],
                                   what="two stages")
  assert not flags.any() and dims[1][:, 3].tolist() == [1, 0, 1, 0] and np.array_equal(out[557:], xyz[557:])
  assert (dims[0][0, :3] < [19, 15, 11]).all(), "the volumes are smaller than their blocks: the capacity strides are in use"


# ---- pipeline -------------------------------------------------------------------------------------------------------------------
def _rooms(seed, sizes):
  rng = np.random.RandomState(seed)
  return [(rng.uniform(0, 3, size=(s, 3)), rng.randint(0, 256, size=(s, 3)).astype(np.float32), rng.randint(0, 41, size=s).astype(np.int32))
          for s in sizes]


def _draws(ss, scenes, with_normals=True):
  rng = np.random.RandomState(3)
  B = len(scenes)
  mats = [_rot_scale(rng.uniform(-3, 3), 20.0 * rng.uniform(0.9, 1.1), (0, 0, 0)) for _ in range(B)]
  rows = sum(len(s[0]) for s in scenes)
  normals = torch.from_numpy(rng.randn(rows, 3).astype(np.float32)).to(DEV) if with_normals else None
  return ss.AugmentationDraws(mats, rng.uniform(-0.2, 0.2, size=(B, 3)), flip=[(True, False, False), (False, True, False), None][:B],
                              contrast=[0.4, None, 0.9][:B], translation=[(10.0, -20.0, 5.0), None, (1.0, 2.0, 3.0)][:B],
                              jitter_std=[0.05, 0.05, None][:B], normals=normals)


def _run_pipeline(ss, aug, scenes, draws, limit=0):
  return [t.cpu().numpy() for t in ss.SegmentationInputPipeline(aug, DEV)(scenes, draws, limit)]


@pytest.mark.parametrize("clip", [None, 1.2])
def test_pipeline_against_the_restatement(PF, clip):
  from pointcontrast_amd.downstream import semseg as ss
  aug = ss.SCANNET_5CM.replace(clip_bound=clip)
  scenes = _rooms(5, [900, 257, 1300])
  draws = _draws(ss, scenes)
  params = PF.seg_color_params(3, draws.flip, draws.contrast, draws.translation, draws.jitter_std)
  for limit in (0, None):
    want = sr.pipeline(scenes, draws.mats, clip, draws.trans_ratio if clip is not None else None, params, draws.normals.cpu().numpy(),
                       True, aug.label_map, 255, 0)
    if limit is None:  # a limit that the third scene exceeds: the batch is truncated at scene 2
      counts = np.bincount(want[0][:, 0], minlength=3)
      limit = int(counts[0] + counts[1] + counts[2] // 2)
      want = sr.pipeline(scenes, draws.mats, clip, draws.trans_ratio if clip is not None else None, params,
                         draws.normals.cpu().numpy(), True, aug.label_map, 255, limit)
      assert len(want[3]) == 2 and len(want[0]) == counts[0] + counts[1]
    got = _run_pipeline(ss, aug, scenes, draws, limit)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]), "coords / target differ (limit %d)" % limit
    assert np.array_equal(_bits(got[1], np.float32), _bits(want[1], np.float32)), "feats differ (limit %d)" % limit
    assert np.array_equal(_bits(got[3], np.float64), _bits(want[3], np.float64)), "transformation differs (limit %d)" % limit
    again = _run_pipeline(ss, aug, scenes, draws, limit)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, again)), "two runs differ"


def test_validation_path_and_sample_reproducible(PF):
  from pointcontrast_amd.downstream import semseg as ss
  scenes = _rooms(9, [300, 200])
  aug = ss.SCANNET_5CM.replace(augment=False)
  got = _run_pipeline(ss, aug, scenes, None)
  M = np.repeat((np.eye(4) * [20.0, 20.0, 20.0, 1.0])[None], 2, 0)
  want = sr.pipeline(scenes, M, None, None, None, None, True, aug.label_map, 255, 0)
  assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
  assert np.array_equal(_bits(got[1], np.float32), _bits(want[1], np.float32))
  with pytest.raises(AssertionError):
    ss.SegmentationInputPipeline(ss.SCANNET_5CM, DEV)(scenes, None)

  def sample():
    g = torch.Generator(device=DEV)
    g.manual_seed(17)
    return ss.AugmentationDraws.sample(ss.SCANNET_5CM, scenes, np.random.RandomState(4), g, DEV)
  a, b = sample(), sample()
  assert np.array_equal(a.mats, b.mats) and np.array_equal(a.trans_ratio, b.trans_ratio) and a.flip == b.flip
  assert a.contrast == b.contrast and torch.equal(a.normals, b.normals) and a.normals.shape == (500, 3)
  for M in a.mats:  # a rotation times a scale within the bounds
    s = np.linalg.norm(M[:3, 0])
    assert 0.9 * 20 <= s <= 1.1 * 20 and np.allclose(M[:3, :3] @ M[:3, :3].T, s * s * np.eye(3), atol=1e-9)
  r1, r2 = _run_pipeline(ss, ss.SCANNET_5CM, scenes, a), _run_pipeline(ss, ss.SCANNET_5CM, scenes, b)
  assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(r1, r2))


def test_pipeline_with_elastic_stages_and_dropout(PF):
  from pointcontrast_amd.downstream import semseg as ss
  aug = ss.SCANNET_5CM
  assert aug.elastic_params == ((0.2, 0.4), (0.8, 1.6)) and ss.SCANNET_2CM.elastic_params == aug.elastic_params
  scenes = _rooms(6, [900, 257, 1300])
  draws = _draws(ss, scenes)
  rng = np.random.RandomState(8)
  noise = [rng.randn(3, 19, 19, 19, 3).astype(np.float32), rng.randn(3, 12, 12, 12, 3).astype(np.float32)]
  keys = rng.rand(2457).astype(np.float32)
  keys[5] = keys[3]  # a tie: the lower row wins
  draws.elastic_on, draws.elastic_noise = [True, False, True], [_dev(v) for v in noise]
  draws.dropout_on, draws.dropout_keys = [True, False, True], _dev(keys)
  params = PF.seg_color_params(3, draws.flip, draws.contrast, draws.translation, draws.jitter_std)
  elastic = [(g, mag, v, [1, 0, 1]) for (g, mag), v in zip(aug.elastic_params, noise)]
  plain = sr.pipeline(scenes, draws.mats, None, None, params, draws.normals.cpu().numpy(), True, aug.label_map, 255, 0)
  for limit in (0, None):
    if limit is None:
      limit = int(counts[0] + counts[1] + counts[2] // 2)
    want = sr.pipeline(scenes, draws.mats, None, None, params, draws.normals.cpu().numpy(), True, aug.label_map, 255, limit,
                       elastic=elastic, dropout_keys=(keys, [True, False, True]))
    counts = np.bincount(want[0][:, 0], minlength=3)
    assert not want[4].any() and len(want[3]) == (3 if limit == 0 else 2)
    got = _run_pipeline(ss, aug, scenes, draws, limit)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]), "coords / target differ (limit %d)" % limit
    assert np.array_equal(_bits(got[1], np.float32), _bits(want[1], np.float32)), "feats differ (limit %d)" % limit
    assert np.array_equal(_bits(got[3], np.float64), _bits(want[3], np.float64)), "transformation differs (limit %d)" % limit
    again = _run_pipeline(ss, aug, scenes, draws, limit)  # the draws survive a call: the pipeline smooths a copy of the noise
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, again)), "two runs differ"
  plain_counts = np.bincount(plain[0][:, 0], minlength=3)
  assert counts[1] == plain_counts[1] and counts[0] < plain_counts[0], "dropout keeps int(0.8 m) rows of the scenes it is drawn for"

  def sample():
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    return ss.AugmentationDraws.sample(aug, scenes, np.random.RandomState(6), g, DEV)
  a, b = sample(), sample()
  assert len(a.elastic_noise) == 2 and all(torch.equal(x, y) for x, y in zip(a.elastic_noise, b.elastic_noise))
  assert a.elastic_on == b.elastic_on and a.dropout_on == b.dropout_on and torch.equal(a.dropout_keys, b.dropout_keys)
  assert a.elastic_noise[0].shape[1:4] == (18, 18, 18), "3 m // 0.2 + 4"
  r1, r2 = _run_pipeline(ss, aug, scenes, a), _run_pipeline(ss, aug, scenes, b)  # no capacity flag: the call does not raise
  assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(r1, r2))


def test_train_iter_scenes_matches_train_iter(PF):
  from pointcontrast_amd.downstream import semseg as ss
  scenes = _rooms(2, [700, 500])
  aug = ss.SCANNET_5CM
  draws = _draws(ss, scenes)
  losses = []
  for use_scenes in (True, False):
    torch.manual_seed(1)
    tr = ss.SegmentationTrainer(20, model="Res16UNet14", lr=0.05, max_iter=50, input_pipeline=ss.SegmentationInputPipeline(aug, DEV))
    if use_scenes:
      out = tr.train_iter_scenes(scenes, draws)
      assert out["transformation"].shape == (2, 16)
    else:
      coords, feats, target, _ = tr.input_pipeline(scenes, draws)
      out = tr.train_iter(coords, feats, target)
    losses.append(float(out["loss"]))
  assert np.isfinite(losses[0]) and losses[0] == losses[1], losses


# ---- C contract -----------------------------------------------------------------------------------------------------------------
def test_c_contract_exact_workspaces_and_refusals():
  from pointcontrast_amd._lib import lib
  rng = np.random.RandomState(1)
  n, B = 777, 3
  offs = _dev(_offs([300, 0, 477]))
  xyz, mats = _dev(rng.uniform(-2, 2, size=(n, 3))), _dev(np.stack([_rot_scale(0.2 * b, 20.0).reshape(16) for b in range(B)]))
  labels, feats = _dev(rng.randint(0, 3, size=n).astype(np.int32)), _dev(rng.uniform(0, 255, size=(n, 3)).astype(np.float32))
  vox, keep = torch.empty((n, 3), dtype=torch.int32, device=DEV), torch.empty(n, dtype=torch.uint8, device=DEV)
  mn, al = torch.empty((B, 3), dtype=torch.int32, device=DEV), torch.empty((B, 16), dtype=torch.float64, device=DEV)
  flags, counts = torch.zeros(B, dtype=torch.int32, device=DEV), torch.empty(B + 1, dtype=torch.int64, device=DEV)
  coords, index = torch.empty((n, 4), dtype=torch.int32, device=DEV), torch.empty(n, dtype=torch.int64, device=DEV)
  olab, out = torch.empty(n, dtype=torch.int32, device=DEV), torch.empty((n, 3), dtype=torch.float32, device=DEV)
  P = _dev(np.tile(np.array([1, 0, 1, 1, 0.5, 1, 3.0, -3.0, 0, 0, 0, 0], np.float64), (B, 1)))
  lim = (C.c_double * 6)(1.5)
  p = lambda t: C.c_void_p(t.data_ptr())
  st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

  def transform(ws, size, n_=n, B_=B, mode=1, xyz_=xyz):
    return lib.pcmi_seg_transform(p(xyz_) if xyz_ is not None else None, p(offs), n_, B_, p(mats), mode, lim, None, p(vox), p(keep), p(mn),
                                  p(al), p(flags), ws, size, st)

  def quantize(ws, size, n_=n, B_=B, ol=olab):
    return lib.pcmi_seg_quantize(p(vox), p(keep), p(labels), p(offs), p(mn), n_, B_, 255, p(coords), p(index),
                                 p(ol) if ol is not None else None, p(counts), p(flags), ws, size, st)

  def color(ws, size, m_=n, B_=B, c_=coords):
    return lib.pcmi_seg_color_augment(p(feats), n, p(index), p(c_) if c_ is not None else None, p(olab), m_, B_, p(P), None, 1, None, 0, 255,
                                      p(out), ws, size, st)

  for call, query in ((transform, lib.pcmi_seg_transform_workspace_bytes(B)), (quantize, lib.pcmi_seg_quantize_workspace_bytes(n)),
                      (color, lib.pcmi_seg_color_augment_workspace_bytes(B))):
    assert query > 0
    g = Guarded(query)
    assert call(g.vp, g.size) == PCMI_OK, call.__name__
    torch.cuda.synchronize()
    g.check(call.__name__)
    assert call(g.vp, C.c_size_t(query - 1)) == PCMI_ERR_WORKSPACE, call.__name__
    assert call(None, g.size) == PCMI_ERR_WORKSPACE, call.__name__
    assert call(g.vp, g.size, -1) == PCMI_ERR_INVALID and call(g.vp, g.size, n, 0) == PCMI_ERR_INVALID, call.__name__
    assert call(g.vp, g.size, n, 1024) == PCMI_ERR_INVALID, call.__name__
  g = Guarded(1 << 20)
  assert transform(g.vp, g.size, mode=3) == PCMI_ERR_INVALID and transform(g.vp, g.size, xyz_=None) == PCMI_ERR_INVALID
  assert quantize(g.vp, g.size, ol=None) == PCMI_ERR_INVALID and color(g.vp, g.size, c_=None) == PCMI_ERR_INVALID
  assert lib.pcmi_seg_transform_workspace_bytes(0) == 0 and lib.pcmi_seg_quantize_workspace_bytes(-1) == 0
  # the three calls above, chained, equal the restatement
  M = int(counts.cpu()[-1])
  w = sr.seg_transform(xyz.cpu().numpy(), offs.cpu().numpy(), mats.cpu().numpy(), 1.5, None)
  wq = sr.seg_quantize(w[0], offs.cpu().numpy(), labels.cpu().numpy(), w[1], w[2], 255)
  assert M == wq[3][-1] and np.array_equal(index[:M].cpu().numpy(), wq[1]) and np.array_equal(flags.cpu().numpy(), w[4] | wq[4])


def test_c_contract_elastic_exact_workspace_and_refusals():
  from pointcontrast_amd._lib import lib
  rng = np.random.RandomState(2)
  n, B, cap = 600, 2, (9, 8, 7)
  host_xyz, host_noise = rng.uniform(0, 1, size=(n, 3)), rng.randn(B, 9, 8, 7, 3).astype(np.float32)
  offs, xyz, noise = _dev(_offs([343, 257])), _dev(host_xyz), _dev(host_noise)
  dims, gmin = torch.empty((B, 4), dtype=torch.int32, device=DEV), torch.empty((B, 3), dtype=torch.float64, device=DEV)
  flags = torch.zeros(B, dtype=torch.int32, device=DEV)
  p = lambda t: C.c_void_p(t.data_ptr())
  st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

  def blur(ws, size, n_=n, B_=B, g=0.2, cx=cap[0], noise_=noise):
    return lib.pcmi_elastic_blur(p(xyz), p(offs), n_, B_, g, None, p(noise_) if noise_ is not None else None, cx, cap[1], cap[2], p(dims),
                                 p(gmin), p(flags), ws, size, st)

  def apply(n_=n, B_=B, g=0.2, mag=0.4, cx=cap[0], dims_=dims):
    return lib.pcmi_elastic_apply(p(xyz), p(offs), n_, B_, g, mag, p(noise), cx, cap[1], cap[2], p(dims_) if dims_ is not None else None,
                                  p(gmin), st)

  query = lib.pcmi_elastic_blur_workspace_bytes(B, *cap)
  assert query > 0 and lib.pcmi_elastic_blur_workspace_bytes(B, 2, 8, 7) == 0 and lib.pcmi_elastic_blur_workspace_bytes(0, *cap) == 0
  g = Guarded(query)
  assert blur(g.vp, g.size) == PCMI_OK and apply() == PCMI_OK
  torch.cuda.synchronize()
  g.check("pcmi_elastic_blur")
  want = sr.elastic_stage(host_xyz, _offs([343, 257]), 0.2, 0.4, host_noise)
  assert np.array_equal(_bits(xyz.cpu().numpy(), np.float64), _bits(want[0], np.float64)) and np.array_equal(dims.cpu().numpy(), want[2])
  assert blur(g.vp, C.c_size_t(query - 1)) == PCMI_ERR_WORKSPACE and blur(None, g.size) == PCMI_ERR_WORKSPACE
  for call in (lambda **kw: blur(g.vp, g.size, **kw), apply):
    assert call(n_=-1) == PCMI_ERR_INVALID and call(B_=0) == PCMI_ERR_INVALID and call(B_=1024) == PCMI_ERR_INVALID
    assert call(g=0.0) == PCMI_ERR_INVALID and call(g=-1.0) == PCMI_ERR_INVALID and call(cx=2) == PCMI_ERR_INVALID
  assert blur(g.vp, g.size, noise_=None) == PCMI_ERR_INVALID and apply(dims_=None) == PCMI_ERR_INVALID
  assert apply(mag=float("nan")) == PCMI_ERR_INVALID
  torch.cuda.synchronize()
  assert not flags.cpu().numpy().any()
