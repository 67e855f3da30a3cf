"""tests/detect_features_ref.py (the restatement that the GPU tests compare pcmi_segment_quantile and pcmi_det_point_features
with) held to np.sort, to np.percentile and to what the reference's own ScannetDetectionDataset and
SunrgbdDetectionVotesDataset returned with use_height / use_color on small synthetic scans:
tests/golden/golden_detfeatures.npz, recorded by tests/golden/make_golden_detfeatures.py with the draws np.random handed out.

Bounds.  The two order statistics are exact (== against np.sort).  The interpolation: numpy's own float32 path rounds hi - lo,
its product with g and the sum to float32, and ulp(hi - lo) <= 2 ulp(max(|lo|, |hi|)): the quantile is held to 3 float32 ulps
of max(|lo|, |hi|) of np.percentile.  The height column adds the one float32 rounding of the reference's float32 subtraction
(and, scaled, the scale's share of both).  xyz and the colour columns are the same operations on both sides: bit for bit.
ScannetDetectionDataset cannot run with use_color in the reference (make_golden_detfeatures.py says why); ScanNet's colour rule
is held to the reference's expression, scannet_detection_dataset.py:88, evaluated here."""
import os

import numpy as np
import pytest

import detect_features_ref as fr
import detect_input_ref as dr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_detfeatures.npz")


@pytest.fixture(scope="module")
def G():
  return np.load(GOLDEN)


def ulp32(x):
  return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def quantile_scenes():
  """(name, z float32 [m]) over sizes 1 .. 150 001, with ties, offsets and scales from 0.01 to 40."""
  rng = np.random.default_rng(20261019)
  out = []
  for m in (1, 2, 3, 4, 7, 63, 64, 65, 100, 101, 102, 255, 256, 257, 1000, 1025, 4097, 10001, 50000, 150001):
    for scale, offset in ((0.01, 0.0), (1.0, -1.5), (3.0, 0.02), (40.0, 7.0)):
      z = (rng.normal(size=m) * scale + offset).astype(np.float32)
      out.append(("normal m=%d scale=%g" % (m, scale), z))
    out.append(("ties m=%d" % m, np.round(rng.normal(size=m) * 3).astype(np.float32) * np.float32(0.25)))
    out.append(("uniform m=%d" % m, rng.uniform(-0.05, 2.6, m).astype(np.float32)))
  out.append(("all equal", np.full(777, 1.25, np.float32)))
  out.append(("signed zeros", np.array([0.0, -0.0, 0.0, -0.0, 1e-45, -1e-45] * 50, np.float32)))
  return out


def test_order_statistics_equal_a_full_sort():
  for q in (0.0, 0.99, 50.0, 99.01, 100.0):
    for name, z in quantile_scenes():
      m = len(z)
      _, stats, flags = fr.segment_quantile(z, [0, m], q)
      k, g = fr.rank_of(m, q)
      s = np.sort(z)
      assert not flags.any() and 0 <= k <= m - 1 and 0.0 <= g < 1.0, (name, q)
      assert stats[0, 0] == s[k] and stats[0, 1] == s[min(k + 1, m - 1)], (name, q)
      assert not np.signbit(stats[stats == 0]).any(), (name, q)


def test_quantile_within_3_ulp_of_numpy_percentile():
  worst = 0.0
  scenes = quantile_scenes()
  offsets = np.concatenate([[0], np.cumsum([len(z) for _, z in scenes])])
  out, stats, flags = fr.segment_quantile(np.concatenate([z for _, z in scenes]), offsets, 0.99)  # one batch: the offsets are honoured
  assert not flags.any()
  for b, (name, z) in enumerate(scenes):
    want = np.percentile(z, 0.99)
    assert want.dtype == np.float32
    lo, hi = np.float64(stats[b, 0]), np.float64(stats[b, 1])
    assert lo <= out[b] <= hi, name
    u = ulp32(max(abs(lo), abs(hi)))
    err = abs(out[b] - np.float64(want)) / u
    worst = max(worst, err)
    assert err <= 3.0, (name, err)
  print("worst difference from np.percentile over %d scenes: %.3f fp32 ulp of max(|lo|, |hi|)" % (len(scenes), worst))


def test_flags_and_zero_sign():
  z = np.array([1.0, 2.0, np.nan, 3.0, 4.0, np.inf, -0.0, -0.0, 5.0], np.float32)
  out, stats, flags = fr.segment_quantile(z, [0, 2, 2, 3, 5, 6, 8, 9], 50.0)
  assert flags.tolist() == [0, 64, 64, 0, 64, 0, 0]
  assert out.tolist() == [1.5, 0.0, 0.0, 3.5, 0.0, 0.0, 5.0] and not np.signbit(out).any() and not np.signbit(stats[stats == 0]).any()


def run(G, ds, r):
  """The restatement on run r of dataset ds, from the scans and the recorded draws: (recorded point_clouds, ours, the scan)."""
  pre = "%s_run%d_" % (ds, r)
  s = int(G[pre + "scan"])
  raw = G[("scannet%d_vert" if ds == "scannet" else "sunrgbd%d_pc") % s]
  color = ds == "sunrgbd" and bool(G[pre + "color"])
  augment = bool(G[pre + "augment"])
  choices = G[pre + "choices"][None]
  scale = [float(G[pre + "scale"])] if ds == "sunrgbd" else [1.0]
  xyz, offsets = raw[:, 0:3], np.array([0, len(raw)], np.int64)
  pc = dr.sample_transform(xyz, offsets, choices, augment=augment, flip=G[pre + "flip"][None], rot=np.stack([dr.rotz(float(G[pre + "rot_angle"]))]),
                           scale=scale)
  assert not pc["flags"].any()
  floor, stats, f = fr.segment_quantile(xyz[:, 2], offsets, 0.99)
  kw = {}
  if color and augment:  # the reference draws per raw point; the restatement takes the draws of the chosen ones
    kw = dict(color_gain=G[pre + "color_gain"][None], color_shift=G[pre + "color_shift"][None],
              color_jitter=G[pre + "color_jitter_raw"][choices[0]][None], color_keep=G[pre + "color_keep_raw"][choices[0]][None])
  out, f2 = fr.point_features(pc["point_clouds"], xyz, offsets, choices, ds, rgb=raw[:, 3:6] if color else None, floor_height=floor,
                              augment=augment, scale=scale, **kw)
  assert not f.any() and not f2.any()
  return G[pre + "point_clouds"], out[0], raw, stats[0], scale[0] if augment else 1.0


def test_golden_covers_the_cases(G):
  P = int(G["num_points"])
  assert int(G["scannet_runs"]) == 3 and int(G["sunrgbd_runs"]) == 5
  assert [int(G["sunrgbd_run%d_color" % r]) for r in range(5)] == [0, 1, 0, 1, 1]
  assert [int(G["sunrgbd_run%d_augment" % r]) for r in range(5)] == [1, 1, 0, 0, 1]
  assert [int(G["scannet_run%d_augment" % r]) for r in range(3)] == [1, 0, 1]
  assert len(G["scannet1_vert"]) < P < len(G["scannet0_vert"]) and len(G["sunrgbd1_pc"]) < P < len(G["sunrgbd0_pc"])
  assert int(G["scannet_run2_scan"]) == 1 and int(G["sunrgbd_run4_scan"]) == 1, "the small scans are run"
  keep = G["sunrgbd_run1_color_keep_raw"]
  assert 0 < keep.sum() < keep.size


@pytest.mark.parametrize("ds,r", [("scannet", r) for r in range(3)] + [("sunrgbd", r) for r in range(5)])
def test_restatement_against_reference(G, ds, r):
  want, got, raw, (lo, hi), scale = run(G, ds, r)
  assert got.shape == want.shape and got.dtype == want.dtype == np.float32
  assert np.array_equal(got[:, 0:3].view(np.uint32), want[:, 0:3].view(np.uint32)), "xyz differs"
  C = got.shape[1] - 3
  if C > 1:
    assert np.array_equal(got[:, 3:6].view(np.uint32), want[:, 3:6].view(np.uint32)), "colour columns differ"
  # the height: 3 ulp(max(|lo|, |hi|)) of the percentile and one rounding of the subtraction; times the scale, plus the
  # scaled height's own rounding, for the augmented SUN RGB-D run
  h, hw = got[:, -1].astype(np.float64), want[:, -1].astype(np.float64)
  unscaled = np.abs(hw) / scale
  bound = (3.0 * ulp32(max(abs(lo), abs(hi))) + ulp32(np.nextafter(unscaled.astype(np.float32), np.float32(np.inf)))) * scale
  if scale != 1.0:
    bound = bound + ulp32(np.maximum(np.abs(h), np.abs(hw)))
  err = np.abs(h - hw)
  print("%s run %d: worst height difference %.3g, %.3f of its bound" % (ds, r, err.max(), (err / bound).max()))
  assert (err <= bound).all(), "height beyond its bound"


def test_scannet_colour_rule_is_the_reference_expression():
  """scannet_detection_dataset.py:24,88 on a float32 [n, 6] array: the slice assignment rounds the float64 result to float32."""
  rng = np.random.default_rng(5)
  vert = np.zeros((400, 6), np.float32)
  vert[:, 0:3] = rng.uniform(-2, 2, (400, 3))
  vert[:, 3:6] = rng.integers(0, 256, (400, 3))
  raw = vert.copy()
  MEAN_COLOR_RGB = np.array([109.8, 97.2, 83.8])
  point_cloud = vert[:, 0:6]
  point_cloud[:, 3:] = (point_cloud[:, 3:] - MEAN_COLOR_RGB) / 256.0
  choices = rng.integers(0, 400, (1, 300)).astype(np.int32)
  out, flags = fr.point_features(raw[choices[0], 0:3][None], raw[:, 0:3], [0, 400], choices, "scannet", rgb=raw[:, 3:6])
  assert not flags.any() and out.shape == (1, 300, 6)
  assert np.array_equal(out[0, :, 3:6].view(np.uint32), point_cloud[choices[0], 3:6].view(np.uint32))


def test_batch_matches_the_parts(G):
  """detect_features_ref.batch (what the GPU test compares the pipeline with) is the xyz batch plus the columns."""
  raw = [G["sunrgbd0_pc"], G["sunrgbd1_pc"]]
  rng = np.random.default_rng(9)
  scenes = [(p, np.zeros((0, 8)), np.zeros((len(p), 10))) for p in raw]
  choices = np.stack([rng.integers(0, len(p), 64) for p in raw]).astype(np.int32)
  kw = dict(mean_size=np.ones((10, 3)), num_heading_bin=12)
  args = ("sunrgbd", scenes, choices, True, np.array([[1, 0], [0, 0]], np.int32), [0.2, -0.1], [1.1, 0.9], 0.2)
  wide = fr.batch(*args, use_height=True, use_color=True, color_gain=np.full((2, 3), 1.1), color_keep=rng.random((2, 64)) > 0.3, **kw)
  plain = fr.batch(*args, **kw)
  assert wide["point_clouds"].shape == (2, 64, 7) and plain["point_clouds"].shape == (2, 64, 3)
  assert np.array_equal(wide["point_clouds"][:, :, 0:3], plain["point_clouds"])
  for k in plain:
    if k != "point_clouds":
      assert np.array_equal(wide[k], plain[k]), k


def test_draws_are_the_same_with_and_without_colour(built_lib):
  from pointcontrast_amd.downstream.votenet import DetectionDraws
  sizes = [500, 120, 0, 4000]
  for ds in ("scannet", "sunrgbd"):
    a = DetectionDraws.sample(sizes, 300, ds, generator=7)
    b = DetectionDraws.sample(sizes, 300, ds, generator=7, color=True)
    for k in ("choices", "flip_x", "flip_y", "rot_angle", "scale"):
      assert np.array_equal(getattr(a, k), getattr(b, k)), (ds, k)
    assert a.color_gain is None and a.color_shift is None and a.color_jitter is None and a.color_keep is None
    if ds == "scannet":
      assert b.color_gain is None and b.color_keep is None
      continue
    assert b.color_gain.shape == (4, 3) and b.color_shift.shape == (4, 3) and b.color_jitter.shape == (4, 300) and b.color_keep.shape == (4, 300)
    assert b.color_gain.dtype == np.float64 and b.color_keep.dtype == bool
    assert (np.abs(b.color_gain - 1) <= 0.2).all() and (np.abs(b.color_shift) <= 0.05).all() and (np.abs(b.color_jitter) <= 0.025).all()
    assert 0.6 < b.color_keep.mean() < 0.8
  off = DetectionDraws.sample(sizes, 300, "sunrgbd", generator=7, augment=False, color=True)
  assert off.color_gain is None
