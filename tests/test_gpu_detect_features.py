"""The feature columns of the detection input on the device (csrc/detect_features.hip: pcmi_segment_quantile,
pcmi_det_point_features) and DetectionInputPipeline(use_height, use_color) against the numpy restatement
tests/detect_features_ref.py BIT FOR BIT (fp32 and fp64 compared as integers); through the restatement the pipeline matches
the reference's recorded dicts within the bounds of tests/test_detect_features_ref.py.  Then the consumers: decode_predictions on
a wider point cloud and DetectionTrainer(backbone="pointnet2", input_feature_dim=1) from raw scans."""
import ctypes as C

import numpy as np
import pytest
import torch

import detect_features_ref as fr
import detect_input_ref as dr
import votenet_fixtures as VF
from c_contract import DEV, Guarded, PCMI_ERR_INVALID, PCMI_ERR_WORKSPACE, PCMI_OK
from test_detect_features_ref import GOLDEN
from test_detect_features_ref import run as golden_run

pytestmark = pytest.mark.gpu

PCMI_ERR_RANGE = -5
SINGLE_MAX, CHUNK = 16384, 8192  # kSingleMax, kChunk of detect_features.hip: one workgroup per scene up to the first, then chunks
QS = (0.0, 0.99, 50.0, 99.01, 100.0)


def PF():
  import pointcontrast_amd.functional as f
  return f


def _dev(a, dtype=None):
  t = torch.as_tensor(np.ascontiguousarray(a))
  return (t if dtype is None else t.to(dtype)).to(DEV)


def bits(a):
  a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
  return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same_bits(got, want, what=""):
  g, w = bits(got), bits(want)
  assert g.dtype == w.dtype and g.shape == w.shape, "%s: %s %s against %s %s" % (what, g.dtype, g.shape, w.dtype, w.shape)
  assert np.array_equal(g, w), "%s: %d of %d elements differ in their bits" % (what, int((g != w).sum()), g.size)


# ---- pcmi_segment_quantile --------------------------------------------------------------------------------------------------------
def _last_of_a_run(rng, m, q):
  """Rank k of (m, q) is the LAST of a run of equal values: rank k + 1 is the next distinct value."""
  k, _ = fr.rank_of(m, q)
  z = np.concatenate([np.full(k + 1, 0.375, np.float32), (0.375 + np.float32(1e-3) + rng.uniform(0, 2, m - k - 1)).astype(np.float32)])
  return rng.permutation(z)


@pytest.fixture(scope="module")
def quantile_batch():
  """37 scenes in one batch: (xyz [n, 3] whose z column holds the values and whose x column is NaN, offsets, expected flags)."""
  rng = np.random.default_rng(20261019)
  normal = lambda m: (rng.normal(size=m) * 0.7 + 0.9).astype(np.float32)  # noqa: E731
  scenes = [normal(m) for m in (1, 2, 3, 63, 64, 65, 255, 256, 257, 1024, 1025, 10001, 70000, 300000)]
  # the dispatch thresholds: one workgroup <-> chunks, and the chunk borders of the smallest and of a larger chunked scene
  scenes += [normal(m) for m in (SINGLE_MAX - 1, SINGLE_MAX, SINGLE_MAX + 1, 3 * CHUNK - 1, 3 * CHUNK, 3 * CHUNK + 1)]
  for m in (5000, 40000):
    scenes.append(np.full(m, -1.625, np.float32))  # all equal
  for m in (777, 20000):
    scenes.append(rng.choice(np.array([0.25, 0.75], np.float32), m))  # two distinct values
  for m in (3000, 50000):
    scenes.append((np.float32(1.5).view(np.uint32) + rng.integers(0, 8, m).astype(np.uint32)).view(np.float32))  # last mantissa bits
  for m in (1000, 17000):  # mixed sign with +-0 and denormals
    pool = np.array([0.0, -0.0, 1e-45, -1e-45, 3e-39, -3e-39, 1.0, -1.0, 2.5e-3, -7.0], np.float32)
    scenes.append(rng.choice(pool, m))
  for m in (2048, 33000):
    scenes.append(np.sort(normal(m))[::-1].copy())  # sorted descending
  for m in (4000, 60000):
    scenes.append(np.round(rng.normal(size=m) * 3).astype(np.float32) * np.float32(0.25))  # every rank inside a run of ties
  scenes += [_last_of_a_run(rng, 5000, 0.99), _last_of_a_run(rng, 100000, 0.99)]
  flagged = {}
  scenes.append(np.zeros(0, np.float32)), flagged.update({len(scenes) - 1: "empty"})
  z = normal(500)
  z[123] = np.nan
  scenes.append(z), flagged.update({len(scenes) - 1: "nan"})
  z = normal(20000)
  z[19999] = np.inf
  scenes.append(z), flagged.update({len(scenes) - 1: "inf"})
  assert len(scenes) == 37
  order = rng.permutation(len(scenes))  # large and small, flagged and clean scenes side by side
  scenes = [scenes[i] for i in order]
  flags = np.array([64 if int(i) in flagged else 0 for i in order], np.int32)
  sizes = [len(z) for z in scenes]
  xyz = np.empty((sum(sizes), 3), np.float32)
  xyz[:, 0], xyz[:, 1], xyz[:, 2] = np.nan, rng.uniform(-3, 3, len(xyz)), np.concatenate(scenes)
  return xyz, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), flags


def _quantile_c(xyz_d, offs_d, n, B, q, ws=None):
  """The C entry point on the z column in place, with exactly the workspace it asks for between guard bands."""
  from pointcontrast_amd._lib import lib
  out = torch.full((B,), float("nan"), dtype=torch.float64, device=DEV)
  stats = torch.full((B, 2), float("nan"), dtype=torch.float32, device=DEV)
  flags = torch.zeros(B, dtype=torch.int32, device=DEV)
  need = lib.pcmi_segment_quantile_workspace_bytes(B)
  ws = Guarded(need) if ws is None else ws
  rc = lib.pcmi_segment_quantile(C.c_void_p(xyz_d.data_ptr() + 8), 3, C.c_void_p(offs_d.data_ptr()), n, B, q, C.c_void_p(out.data_ptr()),
                                 C.c_void_p(stats.data_ptr()), C.c_void_p(flags.data_ptr()), ws.vp, ws.size,
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
  torch.cuda.synchronize()
  ws.check("segment_quantile workspace")
  return rc, out, stats, flags


@pytest.mark.parametrize("q", QS)
def test_segment_quantile_37_scenes(quantile_batch, q):
  xyz, offs, want_flags = quantile_batch
  B, n = len(offs) - 1, len(xyz)
  want, want_stats, f = fr.segment_quantile(xyz[:, 2], offs, q)
  assert np.array_equal(f, want_flags) and (want[f != 0] == 0).all()
  xyz_d, offs_d = _dev(xyz), _dev(offs)
  rc, out, stats, flags = _quantile_c(xyz_d, offs_d, n, B, q)
  assert rc == PCMI_OK
  same_bits(out, want, "quantile q=%g" % q)
  same_bits(stats, want_stats, "order statistics q=%g" % q)
  assert np.array_equal(flags.cpu().numpy(), want_flags)
  if q == 0.99:  # the same bits on a second run, and through the Python wrapper
    rc2, out2, stats2, flags2 = _quantile_c(xyz_d, offs_d, n, B, q)
    assert rc2 == PCMI_OK and torch.equal(out.view(torch.int64), out2.view(torch.int64)) and torch.equal(flags, flags2)
    assert torch.equal(stats.view(torch.int32), stats2.view(torch.int32))
    r = PF().segment_quantile(xyz_d, offs_d, q, column=2, return_stats=True)
    same_bits(r["quantile"], want), same_bits(r["stats"], want_stats)
    assert np.array_equal(r["flags"].cpu().numpy(), want_flags)
    r1 = PF().segment_quantile(xyz_d[:, 2].contiguous(), offs_d, q)
    same_bits(r1["quantile"], want)
    assert r1["stats"] is None


@pytest.mark.parametrize("sizes", [[1, 100, SINGLE_MAX - 101], [SINGLE_MAX], [SINGLE_MAX + 1], [0, SINGLE_MAX + 1, 0, 5]])
def test_segment_quantile_at_the_single_launch_threshold(sizes):
  """n <= kSingleMax takes one launch, n above it the chunked launches as well."""
  rng = np.random.default_rng(sum(sizes))
  n, B = sum(sizes), len(sizes)
  xyz = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
  offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
  for q in (0.99, 50.0):
    want, want_stats, f = fr.segment_quantile(xyz[:, 2], offs, q)
    rc, out, stats, flags = _quantile_c(_dev(xyz), _dev(offs), n, B, q)
    assert rc == PCMI_OK
    same_bits(out, want), same_bits(stats, want_stats)
    assert np.array_equal(flags.cpu().numpy(), f) and f.tolist() == [64 if m == 0 else 0 for m in sizes]


def test_segment_quantile_refusals():
  from pointcontrast_amd._lib import lib
  SENT = 0x7FC0BEEF
  xyz_d, offs_d = _dev(np.zeros((8, 3), np.float32)), _dev(np.zeros(1025, np.int64))
  out = torch.full((1024,), SENT, dtype=torch.int64, device=DEV)
  flags = torch.zeros(1024, dtype=torch.int32, device=DEV)
  ws = Guarded(lib.pcmi_segment_quantile_workspace_bytes(1023))
  st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
  p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

  def call(n=8, B=2, q=0.99, stride=3, size=ws.size):
    return lib.pcmi_segment_quantile(p(xyz_d), stride, p(offs_d), n, B, q, p(out), None, p(flags), ws.vp, size, st)

  assert lib.pcmi_segment_quantile_workspace_bytes(1024) == 0 and lib.pcmi_segment_quantile_workspace_bytes(0) == 0
  assert call(B=1024) == PCMI_ERR_RANGE and call(n=1 << 29) == PCMI_ERR_RANGE
  assert call(B=0) == PCMI_ERR_INVALID and call(q=100.5) == PCMI_ERR_INVALID and call(q=-1.0) == PCMI_ERR_INVALID
  assert call(q=float("nan")) == PCMI_ERR_INVALID and call(stride=0) == PCMI_ERR_INVALID
  assert call(size=C.c_size_t(lib.pcmi_segment_quantile_workspace_bytes(2) - 1)) == PCMI_ERR_WORKSPACE
  torch.cuda.synchronize()
  assert bool((out == SENT).all()) and not bool(flags.any()), "a refused call wrote"
  ws.check("refused calls")
  assert call() == PCMI_OK


# ---- pcmi_det_point_features ------------------------------------------------------------------------------------------------------
def _feature_case(rng, ds, P=300):
  sizes = [450, 120, 333]  # the second scene is smaller than P: sampled with replacement
  n, B = sum(sizes), len(sizes)
  offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
  xyz = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
  rgb = (rng.integers(0, 256, (n, 3)) if ds == "scannet" else rng.uniform(0, 1, (n, 3))).astype(np.float32)
  choices = np.stack([rng.integers(0, m, P) for m in sizes]).astype(np.int32)
  keep = rng.random((B, P)) > 0.3
  keep[2] = False  # a keep mask of all zeros
  draws = dict(scale=rng.uniform(0.85, 1.15, B), color_gain=1 + 0.4 * rng.random((B, 3)) - 0.2, color_shift=0.1 * rng.random((B, 3)) - 0.05,
               color_jitter=0.05 * rng.random((B, P)) - 0.025, color_keep=keep)
  pc = rng.uniform(-2, 2, (B, P, 3)).astype(np.float32)
  floor = np.array([-1.9, 0.0123456789, 0.5])
  return xyz, rgb, offs, choices, pc, floor, draws


@pytest.mark.parametrize("C_", [1, 3, 4])
@pytest.mark.parametrize("augment", [False, True])
@pytest.mark.parametrize("ds", ["scannet", "sunrgbd"])
def test_point_features(ds, augment, C_):
  rng = np.random.default_rng(100 + C_)
  xyz, rgb, offs, choices, pc, floor, draws = _feature_case(rng, ds)
  kw = dict(rgb=rgb if C_ >= 3 else None, floor_height=floor if C_ != 3 else None, augment=augment, **draws)
  want, wf = fr.point_features(pc, xyz, offs, choices, ds, **kw)
  assert want.shape == (3, 300, 3 + C_) and not wf.any()
  if C_ >= 3 and ds == "sunrgbd" and augment:
    assert (want[2, :, 3:6] == -0.5).all() and (np.abs(want[:, :, 3:6]) == 0.5).any() and (np.abs(want[0, :, 3:6]) < 0.5).any(), \
        "dropped colours, clipped colours and plain ones"
  dkw = {k: (None if v is None else _dev(v)) for k, v in kw.items() if k != "augment"}
  got, flags = PF().det_point_features(_dev(pc), _dev(xyz), _dev(offs), _dev(choices), ds, augment=augment, **dkw)
  same_bits(got, want, "%s augment=%s C=%d" % (ds, augment, C_))
  assert not flags.any()
  if ds == "sunrgbd" and augment and C_ >= 3:  # absent colour draws are the identity draws
    ident = dict(kw, color_gain=None, color_shift=None, color_jitter=None, color_keep=None)
    want_i, _ = fr.point_features(pc, xyz, offs, choices, ds, **ident)
    got_i, _ = PF().det_point_features(_dev(pc), _dev(xyz), _dev(offs), _dev(choices), ds, augment=True, rgb=dkw["rgb"],
                                       floor_height=dkw["floor_height"], scale=dkw["scale"])
    same_bits(got_i, want_i, "identity colour draws")


def test_point_features_flags():
  rng = np.random.default_rng(7)
  xyz, rgb, offs, choices, pc, floor, draws = _feature_case(rng, "sunrgbd")
  rgb[offs[0] + choices[0, 5], 1] = np.inf      # a chosen colour
  rgb[offs[1] + 119, 0] = np.nan                # scene 1: chosen or not, decided below
  choices[1, choices[1] == 119] = 0             # ... not chosen: silent
  xyz[offs[2] + choices[2, 7], 2] = np.nan      # a chosen z
  choices[1, 9] = 120                           # out of the scene's rows
  want, wf = fr.point_features(pc, xyz, offs, choices, "sunrgbd", rgb=rgb, floor_height=floor, augment=True, **draws)
  assert wf.tolist() == [64, 4, 64]
  got, flags = PF().det_point_features(_dev(pc), _dev(xyz), _dev(offs), _dev(choices), "sunrgbd", rgb=_dev(rgb), floor_height=_dev(floor),
                                       augment=True, **{k: _dev(v) for k, v in draws.items()})
  same_bits(got, want)
  assert flags.cpu().numpy().tolist() == [64, 4, 64]
  assert not got[0, 5, 3:6].any() and not got[2, 7, 6].any() and not got[1, 9, 3:].any() and bool(torch.isfinite(got).all())
  from pointcontrast_amd._lib import PcmiError, check, lib
  p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
  with pytest.raises(PcmiError, match="no feature column"):
    check(lib.pcmi_det_point_features(p(_dev(pc)), p(_dev(xyz)), None, p(_dev(offs)), len(xyz), 3, 300, p(_dev(choices)), None, 1, 0, None,
                                      None, None, None, None, p(got), p(flags), C.c_void_p(torch.cuda.current_stream().cuda_stream)))


# ---- the pipeline -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def G():
  return np.load(GOLDEN)


def _golden_batch(G, ds, wide, **pipe_kw):
  """The fixture's two scans as one batch with the recorded draws of an augmented run each; labels the fixture does not hold
  (instances, boxes, stored votes) are made up here -- both sides get the same."""
  from pointcontrast_amd.downstream.votenet import DetectionDraws, DetectionInputPipeline
  rng = np.random.RandomState(3)
  P = int(G["num_points"])
  mean = rng.uniform(0.4, 1.5, (18 if ds == "scannet" else 10, 3))
  if ds == "scannet":
    nyu = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39], np.int32)
    runs, raw = [0, 2], [G["scannet0_vert"], G["scannet1_vert"]]
    scenes = [(v if wide else v[:, 0:3].copy(), rng.randint(0, 6, len(v)), np.array([0, 3, 4, 5, 1, 7])[rng.randint(0, 6, len(v))],
               np.concatenate([rng.uniform(-2, 2, (3, 3)), rng.uniform(0.3, 1.0, (3, 3)), rng.choice(nyu, (3, 1))], 1))
              for v in raw]
    kw = dict(valid_sem=nyu, label_to_class=dr.nyu40id_table(nyu), mean_size=mean)
    pipe = DetectionInputPipeline("scannet", P, 0.2, DEV, mean_size_arr=mean, **pipe_kw)
  else:
    runs, raw = [1 if wide else 0, 4], [G["sunrgbd0_pc"], G["sunrgbd1_pc"]]
    scenes = [(v if wide else v[:, 0:3].copy(), np.zeros((0, 8)), rng.uniform(-0.5, 0.5, (len(v), 10))) for v in raw]
    kw = dict(mean_size=mean, num_heading_bin=12)
    pipe = DetectionInputPipeline("sunrgbd", P, 0.2, DEV, mean_size_arr=mean, num_heading_bin=12, **pipe_kw)
  pre = ["%s_run%d_" % (ds, r) for r in runs]
  choices = np.stack([G[p + "choices"] for p in pre])
  flip = np.stack([G[p + "flip"] for p in pre])
  scale = np.array([float(G[p + "scale"]) for p in pre]) if ds == "sunrgbd" else np.ones(2)
  color = {}
  if ds == "sunrgbd" and wide:
    color = dict(color_gain=np.stack([G[p + "color_gain"] for p in pre]), color_shift=np.stack([G[p + "color_shift"] for p in pre]),
                 color_jitter=np.stack([G[p + "color_jitter_raw"][c] for p, c in zip(pre, choices)]),
                 color_keep=np.stack([G[p + "color_keep_raw"][c] for p, c in zip(pre, choices)]))
  d = DetectionDraws(choices, flip[:, 0], flip[:, 1], [float(G[p + "rot_angle"]) for p in pre], scale, **color)
  return scenes, pipe, d, kw, color, runs


KEYS = ("center_label", "heading_class_label", "heading_residual_label", "size_class_label", "size_residual_label", "sem_cls_label",
        "box_label_mask", "point_clouds", "vote_label", "vote_label_mask", "voxel_coords", "voxel_inds", "voxel_feats")


@pytest.mark.parametrize("ds,use_color", [("scannet", False), ("scannet", True), ("sunrgbd", False), ("sunrgbd", True)])
def test_pipeline_with_feature_columns(G, ds, use_color):
  scenes, pipe, d, kw, color, runs = _golden_batch(G, ds, use_color, use_height=True, use_color=use_color)
  assert pipe.feature_dim == (4 if use_color else 1)
  out = pipe(scenes, d)
  want = fr.batch(ds, scenes, d.choices, True, d.flip(), d.rot_angle, d.scale, 0.2, use_height=True, use_color=use_color, **color, **kw)
  assert not want["flags"].any() and tuple(out["point_clouds"].shape) == (2, 300, 3 + pipe.feature_dim)
  for k in KEYS:
    if k == "center_label":  # the padded slots by value: a flipped zero is -0
      assert np.array_equal(out[k].cpu().numpy(), want[k]), k
    else:
      same_bits(out[k], want[k], k)
  # the restatement on the same run, as tests/test_detect_features_ref.py holds it to the reference's recorded dict
  if ds == "sunrgbd" or not use_color:
    for b, r in enumerate(runs):
      _, got, _, _, _ = golden_run(G, ds, r)
      if got.shape[1] == out["point_clouds"].shape[2]:
        same_bits(out["point_clouds"][b], got, "scene %d against the restatement of run %d" % (b, r))


@pytest.mark.parametrize("ds", ["scannet", "sunrgbd"])
def test_pipeline_without_the_options_is_unchanged(G, ds):
  scenes, pipe_off, d, kw, _, _ = _golden_batch(G, ds, False, use_height=False, use_color=False)
  _, pipe_old, _, _, _, _ = _golden_batch(G, ds, False)
  assert pipe_off.feature_dim == 0 and pipe_old.feature_dim == 0
  a, b = pipe_off(scenes, d), pipe_old(scenes, d)
  want = dr.batch(ds, scenes, d.choices, True, d.flip(), d.rot_angle, d.scale, 0.2, **kw)
  assert sorted(a) == sorted(b) == sorted(KEYS)
  for k in KEYS:
    same_bits(a[k], b[k], k)
    if k != "center_label":
      same_bits(a[k], want[k], k)
  assert tuple(a["point_clouds"].shape) == (2, 300, 3)


def test_pipeline_raises_on_a_nan_vertex_that_is_not_chosen(G):
  scenes, pipe, d, _, _, _ = _golden_batch(G, "scannet", False, use_height=True)
  row = int(np.setdiff1d(np.arange(len(scenes[1][0])), d.choices[1])[0])
  bad = scenes[1][0].copy()
  bad[row, 2] = np.nan
  scenes[1] = (bad,) + tuple(scenes[1][1:])
  with pytest.raises(ValueError, match=r"scene 1: the scan is empty or holds a non-finite z"):
    pipe(scenes, d)
  plain = _golden_batch(G, "scannet", False)[1]
  plain(scenes, d)  # without the height the vertex is never read


# ---- the consumers ----------------------------------------------------------------------------------------------------------------
def _mean_size(n):
  return np.random.RandomState(n).uniform(0.4, 1.5, (n, 3)).astype(np.float32)


def _scans(B=2, n0=3000):
  from pointcontrast_amd.downstream.votenet import SCANNET_NYU40IDS
  rng = np.random.RandomState(21)
  out = []
  for b in range(B):
    n = n0 + 100 * b
    ins = rng.randint(0, 8, n)
    cen = rng.uniform([0.5, 0.5, 0.3], [2.5, 2.5, 1.2], (8, 3))
    xyz = (cen[ins] + rng.uniform(-0.4, 0.4, (n, 3))).astype(np.float32)
    sem = np.array([0, 3, 4, 5, 1, 7, 8, 9])[ins]
    boxes = np.concatenate([rng.uniform(0.5, 2.5, (5, 3)), rng.uniform(0.3, 0.8, (5, 3)), rng.choice(SCANNET_NYU40IDS, (5, 1))], 1)
    out.append((xyz, ins, sem, boxes))
  return out


def test_decode_predictions_reads_only_xyz_of_a_wider_cloud():
  from pointcontrast_amd.downstream import votenet
  dc = VF.DatasetConfig(1, _mean_size(18), 18, zero_heading=True)
  rng = np.random.RandomState(4)
  B, K, N = 2, 32, 2048
  pc4 = torch.as_tensor(rng.uniform(0, 1.2, (B, N, 4)).astype(np.float32)).to(DEV)
  pc4[..., 3] = 1000.0  # a height column that would move every count if it were read as a coordinate
  t = lambda *s: torch.as_tensor(rng.normal(size=s).astype(np.float32)).to(DEV)  # noqa: E731
  ep = dict(center=torch.as_tensor(rng.uniform(0.3, 2.8, (B, K, 3)).astype(np.float32)).to(DEV), heading_scores=t(B, K, 1),
            heading_residuals=t(B, K, 1), size_scores=t(B, K, 18), size_residuals=t(B, K, 18, 3) * 0.1, sem_cls_scores=t(B, K, 18),
            objectness_scores=t(B, K, 2))
  cfg = dict(remove_empty_box=True, use_3d_nms=True, nms_iou=0.25, use_old_type_nms=False, cls_nms=True, per_class_proposal=True,
             conf_thresh=0.05, dataset_config=dc)
  wide = votenet.decode_predictions(dict(ep, point_clouds=pc4), cfg)
  narrow = votenet.decode_predictions(dict(ep, point_clouds=pc4[..., 0:3].contiguous()), cfg)
  assert bool((wide["counts"] >= 5).any()) and bool((wide["counts"] < 5).any()), "boxes inside the cloud and empty ones beside it"
  assert 0 < int(wide["pred_mask"].sum()) < B * K
  for k in ("counts", "pred_mask", "sem_cls", "packed", "box_params"):
    assert torch.equal(wide[k], narrow[k]), k


def test_trainer_from_raw_scans_with_the_height_column():
  from pointcontrast_amd.downstream import votenet
  dc = VF.DatasetConfig(1, _mean_size(18), 18, zero_heading=True)
  scans, P = _scans(), 2048
  pipe = votenet.DetectionInputPipeline("scannet", P, 0.05, DEV, mean_size_arr=_mean_size(18), use_height=True)
  with pytest.raises(ValueError, match="feature columns"):
    votenet.DetectionTrainer(dc, num_proposal=32, backbone="pointnet2", input_feature_dim=1, device=DEV,
                             input_pipeline=votenet.DetectionInputPipeline("scannet", P, 0.05, DEV, mean_size_arr=_mean_size(18)))
  with pytest.raises(ValueError, match="feature columns"):
    votenet.DetectionTrainer(dc, num_proposal=32, backbone="pointnet2", input_feature_dim=0, device=DEV, input_pipeline=pipe)
  torch.manual_seed(0)
  t = votenet.DetectionTrainer(dc, num_proposal=32, backbone="pointnet2", input_feature_dim=1, device=DEV, input_pipeline=pipe)
  key = "backbone_net.sa1.mlp_module.layer0.conv.weight"
  assert tuple(t.model.state_dict()[key].shape) == (64, 4, 1, 1)
  sizes = [len(s[0]) for s in scans]
  for step in range(2):
    out = t.train_iter_scenes(scans, votenet.DetectionDraws.sample(sizes, P, "scannet", 5 + step))
    assert all(bool(torch.isfinite(out[k])) for k in ("loss", "vote_loss", "objectness_loss", "box_loss", "sem_cls_loss")), out
  # a reference-shaped state dict: sa1's first layer takes 3 + 1 channels
  state = {k: v.detach().clone() for k, v in t.model.state_dict().items()}
  state[key] = torch.arange(64 * 4, dtype=torch.float32).reshape(64, 4, 1, 1) / 256
  torch.manual_seed(1)
  fresh = votenet.DetectionTrainer(dc, num_proposal=32, backbone="pointnet2", input_feature_dim=1, device=DEV, input_pipeline=pipe)
  fresh.model.load_state_dict(state)
  assert torch.equal(fresh.model.state_dict()[key].cpu(), state[key].cpu())
  # evaluate() from the same pipeline's batches
  cfg = dict(remove_empty_box=True, use_3d_nms=True, nms_iou=0.25, use_old_type_nms=False, cls_nms=True, per_class_proposal=True,
             conf_thresh=0.05, dataset_config=dc)
  metrics = t.evaluate([pipe(scans, votenet.DetectionDraws.sample(sizes, P, "scannet", 9, augment=False))], cfg, ap_iou_thresh=0.25)
  assert isinstance(metrics, dict) and len(metrics) > 0
