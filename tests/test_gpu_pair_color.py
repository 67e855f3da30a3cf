"""Colour through the pre-training path on the device: pcmi_corpus_backproject_color and pcmi_pair_color_features against
tests/pair_color_ref.py (which tests/test_pair_color_ref.py holds to planted answers), PairInputPipeline with and without colours,
build_corpus(color=True) on a synthetic export and one step of both trainers with data.use_color.  Integers and fp64 in a stated
order with one rounding to the output: every comparison is BIT-exact."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

import pair_color_ref as cr
import pair_corpus_ref as ref
import pair_input_ref as pr
from c_contract import DEV, PCMI_ERR_INVALID, PCMI_ERR_WORKSPACE, PCMI_OK
from test_pair_color_ref import H, W, holes, intrinsic
from test_pair_input_ref import MULT, make_frames

pytestmark = pytest.mark.gpu

V = 0.05


@pytest.fixture(scope="module")
def PF():
  from pointcontrast_amd import functional as pf
  return pf


def _dev(a, dtype=None):
  t = torch.from_numpy(np.ascontiguousarray(a))
  return (t if dtype is None else t.to(dtype)).to(DEV)


def _host(t):
  return t.cpu().numpy()


def _same(got, want, what):
  got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
  assert got.dtype == want.dtype and got.shape == want.shape, "%s: %s %s, want %s %s" % (what, got.dtype, got.shape, want.dtype, want.shape)
  assert got.tobytes() == want.tobytes(), "%s differs" % what


def _d16(n):
  return (C.c_double * 16)(*np.asarray(n, np.float64).reshape(-1).tolist())


# ---- pcmi_corpus_backproject_color ----------------------------------------------------------------------------------------------
SENT = 0xA5


def backproject_color(depths, K, colors, Kc, M=None, ws_short=0, hc=None, wc=None, host_offsets=True):
  """The C entry point as a C caller drives it: a workspace of exactly the queried size (less ws_short bytes), `color` filled with
  a sentinel first.  Returns (status, color [F*H*W, 3], uncolored, offsets, offsets_host or None)."""
  from pointcontrast_amd._lib import lib
  from pointcontrast_amd.runtime import cur_stream, ptr
  depths = np.ascontiguousarray(depths, np.uint16)
  colors = np.ascontiguousarray(colors, np.uint8)
  F, h, w = depths.shape
  d_depth, d_img = _dev(depths.view(np.int16)), _dev(colors)
  col = torch.full((F * h * w, 3), SENT, dtype=torch.uint8, device=DEV)
  unc = torch.full((F,), -3, dtype=torch.int64, device=DEV)
  offs = torch.full((F + 1,), -3, dtype=torch.int64, device=DEV)
  offs_h = (C.c_int64 * (F + 1))() if host_offsets else None
  need = lib.pcmi_corpus_backproject_color_workspace_bytes(F, h, w)
  assert need > 0
  ws = torch.empty(need, dtype=torch.uint8, device=DEV)
  st = lib.pcmi_corpus_backproject_color(ptr(d_depth), F, h, w, _d16(K), 1000.0, ptr(d_img), colors.shape[1] if hc is None else hc,
                                         colors.shape[2] if wc is None else wc, _d16(Kc), _d16(np.eye(4) if M is None else M), ptr(col),
                                         ptr(unc), ptr(offs), offs_h, ptr(ws), C.c_size_t(need - ws_short), cur_stream(torch.device(DEV)))
  torch.cuda.synchronize()
  return st, _host(col), _host(unc), _host(offs), None if offs_h is None else np.frombuffer(offs_h, dtype=np.int64).copy()


def plain_offsets(depths, K):
  """offsets of pcmi_corpus_backproject for the same depth (identity poses)."""
  from pointcontrast_amd._lib import check, lib
  from pointcontrast_amd.runtime import cur_stream, ptr
  depths = np.ascontiguousarray(depths, np.uint16)
  F, h, w = depths.shape
  d_depth, poses = _dev(depths.view(np.int16)), _dev(np.tile(np.eye(4), (F, 1, 1)))
  pts = torch.empty((F * h * w, 3), dtype=torch.float64, device=DEV)
  offs, nan = torch.empty(F + 1, dtype=torch.int64, device=DEV), torch.empty(F, dtype=torch.int32, device=DEV)
  offs_h = (C.c_int64 * (F + 1))()
  need = lib.pcmi_corpus_backproject_workspace_bytes(F, h, w)
  ws = torch.empty(need, dtype=torch.uint8, device=DEV)
  check(lib.pcmi_corpus_backproject(ptr(d_depth), F, h, w, _d16(K), ptr(poses), 1000.0, ptr(pts), ptr(offs), ptr(nan), offs_h, ptr(ws),
                                    C.c_size_t(need), cur_stream(torch.device(DEV))))
  return _host(offs), np.frombuffer(offs_h, dtype=np.int64).copy()


def three_frames(seed):
  """3 frames of 20 x 26 (520 pixels: more than one 256-lane workgroup and no multiple of it; the frames' boundaries fall inside
  workgroups and waves), about 30 % zeros with a zero row and zero corners, the middle frame all zero."""
  d = holes(seed, frames=3)
  d[1] = 0
  return d


def _rigid(rng, angle, shift):
  from pointcontrast_amd.lib import synthetic
  M = np.eye(4)
  M[:3, :3] = synthetic._rotation(rng.rand(3) - 0.5, angle)
  M[:3, 3] = shift
  return M


def cases():
  rng = np.random.RandomState(0)
  K = intrinsic(23.7, 12.3, 9.1)
  K[0, 3], K[1, 3] = 0.003, -0.002  # bx, by
  big = rng.randint(0, 256, (3, 2 * H, 2 * W, 3)).astype(np.uint8)
  small = rng.randint(0, 256, (3, H, W, 3)).astype(np.uint8)
  exact = holes(3, frames=3)
  exact[exact != 0] = 1000
  exact[1] = 0
  e64 = intrinsic(64.0, 0.0, 0.0)
  flat, far = np.eye(4), np.eye(4)
  flat[2, 2], far[0, 3] = 0.0, np.inf
  return {
      # a colour camera at twice the resolution, turned and moved a little: most points coloured, some off the image
      "big_rigid": (three_frames(1), K, big, intrinsic(2 * 23.7, 2 * 12.3 + 0.4, 2 * 9.1 - 0.3), _rigid(rng, 0.05, [0.02, -0.01, 0.004])),
      "small_rigid": (three_frames(2), K, small, intrinsic(23.1, 12.9, 9.4), _rigid(rng, 0.08, [-0.03, 0.02, 0.0])),
      "small_same_camera": (three_frames(4), K, small, K, None),
      "ties_up_and_px_Wc": (exact, e64, small, intrinsic(64.0, 0.5, 0.0), None),
      "ties_down_and_px_minus_1": (exact, e64, small, intrinsic(64.0, -1.5, 0.0), None),
      "py_Hc": (exact, e64, small, intrinsic(64.0, 0.0, 0.5), None),
      "ties_on_the_big_image": (exact, e64, big, intrinsic(128.0, 0.5, 1.5), None),
      "behind_the_camera": (three_frames(5), K, small, K, np.diag([1.0, 1.0, -1.0, 1.0])),
      "q2_zero": (exact, e64, small, e64, flat),
      "uc_infinite": (exact, e64, small, e64, far),
  }


CASES = cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_backproject_color_equals_restatement(name):
  depths, K, colors, Kc, M = CASES[name]
  want_col, want_unc, want_offs = cr.backproject_color_ref(depths, K, colors, Kc, M)
  st, col, unc, offs, offs_h = backproject_color(depths, K, colors, Kc, M)
  assert st == PCMI_OK
  n = int(want_offs[-1])
  _same(col[:n], want_col, name + ": color")
  assert (col[n:] == SENT).all(), "rows behind the last point were written"
  _same(unc, want_unc, name + ": uncolored")
  _same(offs, want_offs, name + ": offsets")
  _same(offs_h, want_offs, name + ": offsets_host")
  p_offs, p_offs_h = plain_offsets(depths, K)
  _same(offs, p_offs, name + ": offsets of pcmi_corpus_backproject")
  _same(offs_h, p_offs_h, name + ": offsets_host of pcmi_corpus_backproject")
  assert offs[1] == offs[2] and unc[1] == 0  # the all-zero frame
  # what the case is there for
  total = int(unc.sum())
  if name in ("behind_the_camera", "q2_zero", "uc_infinite"):
    assert total == n > 200 and (col[:n] == 0).all()
  elif name == "small_same_camera":
    assert total == 0
  else:
    assert 0 < total < n // 2, "%s: %d of %d points uncoloured" % (name, total, n)
  # again: the same bits, and without offsets_host (the call that does not wait)
  st2, col2, unc2, offs2, none = backproject_color(depths, K, colors, Kc, M, host_offsets=False)
  assert st2 == PCMI_OK and none is None
  _same(col2, col, name + ": color of a second call")
  _same(unc2, unc, name + ": uncolored of a second call")
  _same(offs2, offs, name + ": offsets of a second call")


@pytest.mark.parametrize("depth", [0, 1])
def test_backproject_color_of_one_pixel(depth):
  d = np.array([[[depth]]], np.uint16)
  img = np.array([[[[7, 8, 9]]]], np.uint8)
  K = intrinsic(64.0, 0.0, 0.0)
  st, col, unc, offs, offs_h = backproject_color(d, K, img, K)
  want = cr.backproject_color_ref(d, K, img, K)
  assert st == PCMI_OK and offs.tolist() == offs_h.tolist() == [0, depth] == want[2].tolist() and unc.tolist() == [0]
  assert col.tolist() == ([[7, 8, 9]] if depth else [[SENT] * 3])
  _same(col[:depth], want[0], "one pixel")


def test_backproject_color_c_contract():
  depths, K, colors, Kc, M = CASES["big_rigid"]
  st, col, unc, offs, _ = backproject_color(depths, K, colors, Kc, M, ws_short=1)
  assert st == PCMI_ERR_WORKSPACE and (col == SENT).all() and (unc == -3).all() and (offs == -3).all()
  for hc, wc in ((0, 2 * W), (2 * H, 0)):
    st, col, unc, offs, _ = backproject_color(depths, K, colors, Kc, M, hc=hc, wc=wc)
    assert st == PCMI_ERR_INVALID and (col == SENT).all() and (unc == -3).all() and (offs == -3).all()
  st, col, *_ = backproject_color(depths, K, colors, Kc, M)  # the exact workspace is enough
  assert st == PCMI_OK and not (col == SENT).all()


def test_process_scene_with_colors_keeps_the_geometry():
  from pointcontrast_amd.lib import pair_corpus as pc
  depths, K, colors, Kc, M = CASES["big_rigid"]
  poses = np.tile(np.eye(4), (3, 1, 1))
  poses[2, :3, 3] = [0.03, 0.0, 0.01]
  plain = pc.process_scene(depths, poses, K)
  got = pc.process_scene(depths, poses, K, colors=colors, color_intrinsic=Kc, depth_to_color=M)
  assert set(got) == set(plain) | {"colors", "uncolored"} and list(got["frames"]) == [0, 2] and got["reasons"][1] == "empty"
  for k in ("points", "centroids"):
    assert all(np.array_equal(a, b) for a, b in zip(got[k], plain[k])) and len(got[k]) == len(plain[k]) == 2
  assert np.array_equal(got["C"], plain["C"]) and np.array_equal(got["M"], plain["M"])
  want_col, want_unc, offs = cr.backproject_color_ref(depths, K, colors, Kc, M)
  _same(got["uncolored"], want_unc, "uncolored")
  for k, f in enumerate(got["frames"]):
    _same(got["colors"][k], want_col[offs[f]:offs[f + 1]], "colors of frame %d" % f)
    assert len(got["colors"][k]) == len(got["points"][k])


# ---- pcmi_pair_color_features ---------------------------------------------------------------------------------------------------
SIZES = [0, 1, 300, 700]  # B = 2: an empty cloud, a single point, one workgroup and a bit, several workgroups


def _crowded(rng, sizes):
  """Clouds whose points crowd into few voxels (about four points per voxel): the voxel's first point is one of several."""
  return [np.stack([rng.uniform(-0.4, 0.4, n), rng.uniform(-0.2, 0.3, n), rng.normal(0, 0.003, n) - 0.2], 1) for n in sizes]


@pytest.fixture(scope="module")
def crowded(PF):
  rng = np.random.RandomState(7)
  clouds = _crowded(rng, SIZES)
  pts, offs = np.concatenate(clouds), np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
  color = rng.randint(0, 256, (len(pts), 3)).astype(np.uint8)
  noise = rng.standard_normal((len(pts), 3)).astype(np.float32)
  want_vox = pr.pair_voxelize(pts, offs, V)
  vox = PF.pair_voxelize(_dev(pts), _dev(offs), V)
  M = int(want_vox["vox_offsets"][-1])
  _same(_host(vox["first_index"])[:M], want_vox["first_index"], "first_index")
  assert want_vox["n_vox"].tolist()[:2] == [0, 1] and M < 0.5 * len(pts)
  # the colour of a voxel's first point is not that of its later points
  later = np.setdiff1d(np.arange(len(pts)), want_vox["first_index"])
  assert len(later) > 400 and len(np.unique(color[later], axis=0)) > 400
  T = np.tile(np.eye(4), (2, 1, 1))
  return dict(color=color, noise=noise, vox=vox, want_vox=want_vox, M=M, T=T, n=len(pts))


def _features(PF, c, noise, on, mu, sigma, out_rows=None):
  """pair_collate, then pair_color_features over its F: the buffers hold a sentinel where neither wrote."""
  co = PF.pair_collate(c["vox"], _dev(c["T"]), None if noise is None else _dev(noise), None if on is None else _dev(np.asarray(on, np.int32)),
                       mu, sigma, out_rows=out_rows)
  ones = {k: co[k].clone() for k in ("sinput0_F", "sinput1_F")}
  keep = {k: co[k].clone() for k in co if not k.endswith("_F")}
  for k in ones:
    co[k].fill_(-7.0)
  PF.pair_color_features(_dev(c["color"]), c["vox"], co, None if noise is None else _dev(noise), None if on is None else _dev(np.asarray(on, np.int32)),
                         mu, sigma)
  for k, v in keep.items():  # (bits: the rows behind the valid ones are whatever the allocation held)
    assert torch.equal(co[k].view(torch.int32), v.view(torch.int32)), "pair_color_features wrote %s" % k
  return co, ones


@pytest.mark.parametrize("jitter", ["mixed", "strong", "null"])
def test_color_features_equal_restatement(PF, crowded, jitter):
  c = crowded
  noise, on, mu, sigma = {"mixed": (c["noise"], [1, 0, 0, 1], 0.0, 0.01), "strong": (c["noise"], [1, 0, 0, 1], 0.25, 0.5),
                          "null": (None, None, 0.0, 0.01)}[jitter]
  rows = c["vox"]["points"].shape[0]
  co, _ = _features(PF, c, noise, on, mu, sigma)
  want = cr.color_features_ref(c["color"], c["want_vox"], noise, on, mu, sigma, out_rows=rows, sentinel=-7.0)
  for s in range(2):
    _same(_host(co["sinput%d_F" % s]), want[s], "%s: sinput%d_F" % (jitter, s))
  side = c["want_vox"]["side_offsets"]
  n0, n1 = int(side[0, 2]), int(side[1, 2])
  assert n0 > 50 and n1 > 100 and (want[0][n0:] == -7).all() and (want[1][:n1] != -7).all()
  if jitter == "null":
    assert np.abs(want[1][:n1]).max() <= 0.5
  else:  # cloud 3 (side 1 of pair 1) is jittered, cloud 2 (side 0 of pair 1) is not
    plain = cr.color_features_ref(c["color"], c["want_vox"], out_rows=rows, sentinel=-7.0)
    s1 = int(side[1, 1])
    assert (want[1][s1:n1] != plain[1][s1:n1]).any() and np.array_equal(want[0][:n0], plain[0][:n0])


def test_color_features_one_row_short(PF, crowded):
  """out_rows one short of the rows side 1 needs: its last row is not written, nor anything behind the buffers."""
  c = crowded
  side = c["want_vox"]["side_offsets"]
  n0, n1 = int(side[0, 2]), int(side[1, 2])
  assert n1 > n0
  rows = n1 - 1
  co, _ = _features(PF, c, c["noise"], [1, 0, 0, 1], 0.0, 0.01, out_rows=rows)
  want = cr.color_features_ref(c["color"], c["want_vox"], c["noise"], [1, 0, 0, 1], 0.0, 0.01, out_rows=rows, sentinel=-7.0)
  full = cr.color_features_ref(c["color"], c["want_vox"], c["noise"], [1, 0, 0, 1], 0.0, 0.01)
  for s in range(2):
    assert co["sinput%d_F" % s].shape == (rows, 3)
    _same(_host(co["sinput%d_F" % s]), want[s], "one row short: sinput%d_F" % s)
  _same(want[1], full[1][:rows], "the rows that fit")
  assert (want[0][n0:] == -7).all()
  # a buffer with the row: the same call leaves the row behind out_rows at its sentinel
  from pointcontrast_amd._lib import check, lib
  from pointcontrast_amd.runtime import cur_stream, ptr
  F0 = torch.full((n1, 3), -7.0, dtype=torch.float32, device=DEV)
  F1 = torch.full((n1, 3), -7.0, dtype=torch.float32, device=DEV)
  vox, col = c["vox"], _dev(c["color"])
  ws = torch.empty(256, dtype=torch.uint8, device=DEV)
  check(lib.pcmi_pair_color_features(ptr(col), ptr(vox["first_index"]), vox["first_index"].shape[0], ptr(vox["vox_offsets"]),
                                     ptr(vox["side_offsets"]), 2, None, c["n"], None, 0.0, 0.01, rows, ptr(F0), ptr(F1), ptr(ws),
                                     C.c_size_t(256), cur_stream(torch.device(DEV))))
  plain = cr.color_features_ref(c["color"], c["want_vox"])
  _same(_host(F1)[:rows], plain[1][:rows], "noise = NULL")
  assert (_host(F1)[rows:] == -7).all() and (_host(F0)[n0:] == -7).all()


def test_color_features_refuse_cpu_tensors(PF, crowded):
  from pointcontrast_amd._lib import PcmiError
  with pytest.raises(PcmiError, match="no CPU path"):
    PF.pair_color_features(torch.zeros((4, 3), dtype=torch.uint8), crowded["vox"], {})


# ---- pipeline -------------------------------------------------------------------------------------------------------------------
def colored_frames(seed, n_pairs=2, n=1200):
  rng = np.random.RandomState(100 + seed)
  return [(a, b, rng.randint(0, 256, a.shape).astype(np.uint8), rng.randint(0, 256, b.shape).astype(np.uint8))
          for a, b in make_frames(seed, n_pairs=n_pairs, n=n)]


def write_color_corpus(tmp_path, frames):
  from pointcontrast_amd.lib import pair_corpus as pc
  lines = []
  for i, f in enumerate(frames):
    pc.write_npz(str(tmp_path / ("f%da.npz" % i)), f[0], f[2])
    pc.write_npz(str(tmp_path / ("f%db.npz" % i)), f[1], f[3])
    lines.append("f%da.npz f%db.npz 0.5\n" % (i, i))
  (tmp_path / "pairs.txt").write_text("".join(lines))


def _config(tmp_path, extra=()):
  from pointcontrast_amd.lib.config import get_config
  return get_config(["data.dataset=ScanNetMatchPairDataset", "data.dataset_root_dir=%s" % tmp_path, "data.scannet_match_dir=pairs.txt",
                     "data.voxel_size=%r" % V, "trainer.batch_size=2"] + list(extra))


def _ref_features(frames, vox_ref, noise, on, mu, sigma):
  color = np.concatenate([c for f in frames for c in f[2:4]])
  return cr.color_features_ref(color, vox_ref, noise, on, mu, sigma)


def _vox_ref(frames, scale=None, rot=None):
  clouds = [f[s] for f in frames for s in range(2)]
  raw = np.concatenate(clouds)
  offs = np.concatenate([[0], np.cumsum([len(a) for a in clouds])]).astype(np.int64)
  tf = pr.pair_transform(raw, offs, np.ones(len(frames)) if scale is None else scale, rot)
  return pr.pair_voxelize(tf["points"], offs, V, tf["flags"])


def test_pipeline_with_and_without_colours(PF, tmp_path):
  from pointcontrast_amd.lib.ddp_data_loaders import ScanNetMatchPairDataset, default_collate_pair_fn
  from pointcontrast_amd.lib.pair_input import PairDraws, PairInputPipeline
  frames = colored_frames(3)
  bare = [f[:2] for f in frames]
  # identity draws, no jitter
  pipe = PairInputPipeline(V, MULT, random_rotation=False, jitter=None)
  got4 = pipe(frames, PairDraws.identity(2))
  assert pipe.last_readbacks == 1
  got2 = pipe(bare, PairDraws.identity(2))
  assert pipe.last_readbacks == 1
  want = _ref_features(frames, _vox_ref(frames), None, None, 0.0, 0.0)
  for s in range(2):
    _same(_host(got4["sinput%d_F" % s]), want[s], "identity draws: sinput%d_F" % s)
    assert torch.equal(got2["sinput%d_F" % s], torch.ones_like(got2["sinput%d_F" % s])), "2-tuples: the collate's ones"
  assert set(got4) == set(got2)
  for k in got2:
    if not k.endswith("_F"):
      assert got4[k] == got2[k] if k in ("len_batch", "n_queries") else torch.equal(got4[k], got2[k]), "colours changed %s" % k
  # ... which is the host loader's batch on the same files
  write_color_corpus(tmp_path, frames)
  dset = ScanNetMatchPairDataset("train", transform=None, random_rotation=False, random_scale=False,
                                 config=_config(tmp_path, ["data.use_color=True"]))
  host = default_collate_pair_fn([dset[i] for i in range(2)])
  for s in range(2):
    assert host["sinput%d_F" % s].dtype == torch.float32
    _same(_host(got4["sinput%d_F" % s]), host["sinput%d_F" % s].numpy(), "host loader: sinput%d_F" % s)
    assert torch.equal(got4["sinput%d_C" % s].cpu(), host["sinput%d_C" % s])
  # rotated, scaled and jittered draws: the restatement on the restated voxels
  rng = np.random.RandomState(8)
  from pointcontrast_amd.lib import synthetic
  rot = np.stack([synthetic._rotation(rng.rand(3) - 0.5, 2 * np.pi * (rng.rand() - 0.5)) for _ in range(4)])
  d = PairDraws(rng.uniform(0.8, 1.2, 2), rot, [1, 0, 0, 1])
  n = sum(len(f[0]) + len(f[1]) for f in frames)
  noise = rng.standard_normal((n, 3)).astype(np.float32)
  d.noise = _dev(noise)
  full = PairInputPipeline(V, MULT)
  g4, g2 = full(frames, d), full(bare, d)
  assert full.last_readbacks == 1
  want = _ref_features(frames, _vox_ref(frames, d.scale, d.rot), noise, d.jitter_on, 0.0, 0.01)
  for s in range(2):
    _same(_host(g4["sinput%d_F" % s]), want[s], "jittered draws: sinput%d_F" % s)
  ref2 = pr.pipeline(bare, d.scale, d.rot, d.jitter_on, noise, V, MULT)
  for k, w in ref2.items():
    if k in ("len_batch", "n_queries"):
      assert g2[k] == w and g4[k] == w
    else:
      _same(_host(g2[k]), w, "2-tuples: %s" % k)  # today's outputs
      if not k.endswith("_F"):
        _same(_host(g4[k]), w, "4-tuples: %s" % k)


def test_pipeline_refuses_mixed_or_misshapen_colours(PF):
  from pointcontrast_amd.lib.pair_input import PairDraws, PairInputPipeline
  frames = colored_frames(4)
  pipe = PairInputPipeline(V, MULT, random_rotation=False, jitter=None)
  with pytest.raises(ValueError, match="colours"):
    pipe([frames[0], frames[1][:2]], PairDraws.identity(2))
  with pytest.raises(ValueError, match="pair 1: rgb0"):
    pipe([frames[0], (frames[1][0], frames[1][1], frames[1][2][:-1], frames[1][3])], PairDraws.identity(2))
  with pytest.raises(ValueError, match="pair 0: rgb1"):
    pipe([(frames[0][0], frames[0][1], frames[0][2], frames[0][3].astype(np.float32)), frames[1]], PairDraws.identity(2))
  assert pipe(frames, PairDraws.identity(2))["sinput0_F"].abs().max() <= 0.5  # and works afterwards


# ---- build_corpus(color=True) and the trainers ----------------------------------------------------------------------------------
def _write_export(root, scene, depths, poses, K, colors, Kc, extrinsics=None, skip_color=()):
  from PIL import Image
  sd = os.path.join(str(root), scene)
  for sub in ("depth", "pose", "intrinsic", "color"):
    os.makedirs(os.path.join(sd, sub), exist_ok=True)
  for k, (d, P, c) in enumerate(zip(depths, poses, colors)):
    Image.fromarray(d).save(os.path.join(sd, "depth", "%d.png" % k))
    np.savetxt(os.path.join(sd, "pose", "%d.txt" % k), P)
    if k not in skip_color:
      Image.fromarray(c).save(os.path.join(sd, "color", "%d.png" % k))
  np.savetxt(os.path.join(sd, "intrinsic", "intrinsic_depth.txt"), K)
  np.savetxt(os.path.join(sd, "intrinsic", "intrinsic_color.txt"), Kc)
  if extrinsics is not None:
    np.savetxt(os.path.join(sd, "intrinsic", "extrinsic_color.txt"), extrinsics[0])
    np.savetxt(os.path.join(sd, "intrinsic", "extrinsic_depth.txt"), extrinsics[1])


def _plane_scene(seed):
  """3 frames of 24 x 32 depth of a slanted plane with holes, 48 x 64 colour, the cameras a few centimetres apart."""
  rng = np.random.RandomState(seed)
  v, u = np.mgrid[0:24, 0:32]
  depths, poses = [], []
  for k in range(3):
    d = (1500 + 9 * u + 5 * v + 20 * k + rng.randint(0, 3, u.shape)).astype(np.uint16)
    d[rng.rand(24, 32) < 0.1] = 0
    depths.append(d)
    P = np.eye(4)
    P[:3, 3] = [0.03 * k, -0.02 * k, 0.01 * k]
    poses.append(P)
  K = ref.intrinsic_matrix(32, 24)
  Kc = ref.intrinsic_matrix(64, 48)
  Kc[0, 2] += 1.7  # the last depth column projects just past the colour image
  colors = rng.randint(0, 256, (3, 48, 64, 3)).astype(np.uint8)
  return np.stack(depths), np.stack(poses), K, colors, Kc


def _tree_bytes(root):
  out = {}
  for dp, _, fs in os.walk(root):
    for f in fs:
      p = os.path.join(dp, f)
      out[os.path.relpath(p, root)] = open(p, "rb").read()
  return out


@pytest.fixture(scope="module")
def color_corpus(tmp_path_factory):
  from pointcontrast_amd.lib import pair_corpus as pc
  root = tmp_path_factory.mktemp("color_corpus")
  Ec, Ed = np.eye(4), np.eye(4)
  Ec[:3, 3], Ed[:3, 3] = [0.012, -0.004, 0.002], [0.0, 0.003, 0.0]
  scenes = {"scene0000_00": _plane_scene(1) + (None,), "scene0001_00": _plane_scene(2) + ((Ec, Ed),)}
  for s, (depths, poses, K, colors, Kc, ext) in scenes.items():
    _write_export(root / "export", s, depths, poses, K, colors, Kc, ext)
  logs, plain_logs = [], []
  out = pc.build_corpus(str(root / "export"), str(root / "color"), log=logs.append, color=True)
  pc.build_corpus(str(root / "export"), str(root / "plain"), log=plain_logs.append)
  return root, scenes, out, logs, plain_logs


def test_build_corpus_with_color(color_corpus, tmp_path):
  import zipfile
  from pointcontrast_amd.lib import pair_corpus as pc
  root, scenes, out, logs, plain_logs = color_corpus
  col, plain = _tree_bytes(str(root / "color")), _tree_bytes(str(root / "plain"))
  assert sorted(col) == sorted(plain) and len(col) == 2 * 4 + 1
  total_unc = 0
  for rel in col:
    if not rel.endswith(".npz"):
      assert col[rel] == plain[rel], "%s differs with --color" % rel  # overlap.txt and the list
      continue
    with zipfile.ZipFile(str(root / "color" / rel)) as zc, zipfile.ZipFile(str(root / "plain" / rel)) as zp:
      assert zc.namelist() == ["pcd.npy", "color.npy"] and zp.namelist() == ["pcd.npy"] and zc.read("pcd.npy") == zp.read("pcd.npy")
  for s, (depths, poses, K, colors, Kc, ext) in scenes.items():
    M = None if ext is None else np.linalg.inv(ext[0]) @ ext[1]
    want_col, want_unc, offs = cr.backproject_color_ref(depths, K, colors, Kc, M)
    for f in range(3):
      with np.load(str(root / "color" / s / "pcd" / ("%d.npz" % f))) as z:
        assert list(z.keys()) == ["pcd", "color"] and len(z["pcd"]) == len(z["color"])
        _same(z["color"], want_col[offs[f]:offs[f + 1]], "%s frame %d" % (s, f))
    summary = [x for x in out if x["scene"] == s][0]
    assert summary["uncolored"] == int(want_unc.sum()) and summary["used"] == 3
    total_unc += int(want_unc.sum())
    n = int(offs[-1])
    assert (want_col.reshape(-1, 3).any(1)).sum() > 0.8 * n  # most points found a pixel
  assert total_unc > 0
  assert all((", uncolored %d, " % s["uncolored"]) in ln for s, ln in zip(out, logs)) and not any("uncolored" in ln for ln in plain_logs)
  assert len((root / "color" / pc.LIST_NAME).read_text().splitlines()) >= 4
  # a depth frame without its image
  depths, poses, K, colors, Kc = _plane_scene(3)
  _write_export(tmp_path / "export", "scene0002_00", depths, poses, K, colors, Kc, skip_color=(1,))
  with pytest.raises(FileNotFoundError, match=r"color/1\.png"):
    pc.build_corpus(str(tmp_path / "export"), str(tmp_path / "out"), color=True)
  assert len(pc.build_corpus(str(tmp_path / "export"), str(tmp_path / "out"))) == 1  # without colours the export is complete


class _Recording:
  """The loader's pipeline, with the noise drawn here from the same generator by the same call, so that its bound is known."""

  def __init__(self, pipeline):
    self.pipeline, self.max_abs_z, self.batches = pipeline, 0.0, []

  def __call__(self, frames, draws):
    assert all(len(f) == 4 and f[2].dtype == np.uint8 for f in frames)
    n = sum(len(f[0]) + len(f[1]) for f in frames)
    g = draws.generator
    draws.noise = torch.randn((n, 3), generator=g, dtype=torch.float32, device=g.device)
    self.max_abs_z = max(self.max_abs_z, float(draws.noise.abs().max()))
    out = self.pipeline(frames, draws)
    self.batches.append(out)
    return out


def _color_step(Trainer, root):
  from pointcontrast_amd.lib import pair_corpus as pc
  from pointcontrast_amd.lib.config import get_config
  from pointcontrast_amd.lib.ddp_data_loaders import make_data_loader
  from pointcontrast_amd.lib.pair_input import DevicePairLoader
  from pointcontrast_amd.lib.timer import AverageMeter, Timer
  cfg = get_config(["data.dataset=ScanNetMatchPairDataset", "data.dataset_root_dir=%s" % (root / "color"), "data.scannet_match_dir=%s" % pc.LIST_NAME,
                    "data.val_match_dir=%s" % pc.LIST_NAME, "data.voxel_size=%r" % V, "trainer.batch_size=2", "net.model=Res16UNet14",
                    "misc.nceT=0.4", "misc.npos=256", "opt.lr=0.1", "misc.prefetch=False", "trainer.num_pos_per_batch=128",
                    "trainer.num_hn_samples_per_batch=64", "data.use_color=True", "data.device_batch=True", "misc.train_num_thread=0"])
  random.seed(0)
  np.random.seed(0)
  torch.manual_seed(0)
  loader = make_data_loader(cfg, 2, num_threads=0)
  assert isinstance(loader, DevicePairLoader)
  loader.reset_seed(0)
  rec = loader.pipeline = _Recording(loader.pipeline)
  tr = Trainer(cfg, loader)
  res = tr._train_iter(iter(loader), [AverageMeter(), Timer(), Timer()])
  torch.cuda.synchronize()
  loader.close()
  return tr, cfg, rec, {k: v.detach().cpu() for k, v in res.items()}


@pytest.mark.parametrize("which", ["PointNCELossTrainer", "HardestContrastiveLossTrainer"])
def test_trainers_step_on_the_coloured_corpus(PF, color_corpus, which):
  from pointcontrast_amd.lib import ddp_trainer
  from pointcontrast_amd.lib.ddp_data_loaders import make_val_data_loader
  root = color_corpus[0]
  Trainer = getattr(ddp_trainer, which)
  tr, cfg, rec, res = _color_step(Trainer, root)
  assert np.isfinite(float(res["loss"]))
  assert len(rec.batches) >= 1 and rec.max_abs_z > 1.0
  # |c / 255 - 0.5| <= 0.5 and |sigma z| <= 0.01 max|z| (mu = 0); one monotone rounding to float32
  bound = np.float32(0.5 + 0.01 * rec.max_abs_z)
  for b in rec.batches:
    for s in range(2):
      F = b["sinput%d_F" % s]
      assert F.is_cuda and F.shape[0] > 100 and float(F.abs().max()) <= bound and float(F.std()) > 0.1, "not colour features"
  _, _, rec2, res2 = _color_step(Trainer, root)
  assert torch.equal(res["loss"].view(torch.int32), res2["loss"].view(torch.int32)), "two runs from one seed: %r, %r" % (float(res["loss"]), float(res2["loss"]))
  assert torch.equal(rec.batches[0]["sinput0_F"], rec2.batches[0]["sinput0_F"])
  if which == "PointNCELossTrainer":  # the validation loader is the host dataset with the same option
    val = make_val_data_loader(cfg, 2)
    first = next(iter(val))
    assert float(first["sinput0_F"].abs().max()) <= 0.5 and float(first["sinput0_F"].std()) > 0.1
    m = tr.validate(val)
    assert len(m) > 0 and all(np.isfinite(v) for v in m.values() if isinstance(v, float))
