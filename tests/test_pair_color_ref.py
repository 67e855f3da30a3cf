"""The colour rules restated in tests/pair_color_ref.py (what tests/test_gpu_pair_color.py compares the kernels with) held to
planted answers, and the host side of the colour path: write_npz's second member, read_color, the calibration reader and
ScanNetMatchPairDataset with data.use_color.  No GPU."""
import os

import numpy as np
import pytest

import pair_color_ref as cr
from pointcontrast_amd.lib import pair_corpus as pc

H, W = 20, 26


def intrinsic(f, cx, cy):
  K = np.eye(4)
  K[0, 0] = K[1, 1] = f
  K[0, 2], K[1, 2] = cx, cy
  return K


def holes(seed, frames=1, h=H, w=W, lo=500, hi=4000):
  """Depth with about 30 % zeros, a whole zero row, and the first and last pixel zero."""
  rng = np.random.RandomState(seed)
  d = rng.randint(lo, hi, (frames, h, w)).astype(np.uint16)
  d[rng.rand(frames, h, w) < 0.3] = 0
  d[:, h // 2] = 0
  d[:, 0, 0] = d[:, -1, -1] = 0
  return d


def own_pixels(depth):
  v, u = np.nonzero(depth)  # row-major, as the back-projection keeps them
  return u, v


def test_image_codes_its_own_pixels():
  img = cr.self_coding_image(300, 520)
  x, y = cr.pixel_of(img)
  assert np.array_equal(x, np.tile(np.arange(520), (300, 1))) and np.array_equal(y, np.tile(np.arange(300)[:, None], (1, 520)))


def test_same_camera_gives_every_point_its_own_pixel():
  d = holes(0, frames=2)
  K = intrinsic(23.7, 12.3, 9.1)
  img = np.stack([cr.self_coding_image(H, W)] * 2)
  img[1, :, :, 2] += 100  # the second frame's image is another one
  col, unc, offs = cr.backproject_color_ref(d, K, img, K)
  assert unc.tolist() == [0, 0] and offs.tolist() == [0, (d[0] != 0).sum(), (d != 0).sum()]
  for f in range(2):
    u, v = own_pixels(d[f])
    c = col[offs[f]:offs[f + 1]].astype(np.int64)
    assert np.array_equal(c[:, 0], u) and np.array_equal(c[:, 1], v) and (c[:, 2] == 100 * f).all()


def test_colour_image_at_twice_the_resolution():
  d = holes(1)
  K = intrinsic(23.7, 12.3, 9.1)
  Kc = intrinsic(2 * 23.7, 2 * 12.3, 2 * 9.1)
  col, unc, _ = cr.backproject_color_ref(d, K, cr.self_coding_image(2 * H, 2 * W)[None], Kc)
  u, v = own_pixels(d[0])
  x, y = cr.pixel_of(col)
  assert unc.tolist() == [0] and np.array_equal(x, 2 * u) and np.array_equal(y, 2 * v)


def test_translation_along_x_shifts_by_fxc_tx_over_d():
  d = holes(2)
  d[d != 0] = np.where(np.arange((d != 0).sum()) % 2 == 0, 2000, 1000)  # 2 m and 1 m
  K = intrinsic(100.0, 12.3, 9.1)
  M = np.eye(4)
  M[0, 3] = 0.06  # 100 * 0.06 / 2 = 3 pixels at 2 m, 6 pixels at 1 m
  col, unc, _ = cr.backproject_color_ref(d, K, cr.self_coding_image(H, W)[None], K, M)
  u, v = own_pixels(d[0])
  shift = np.where(d[0][v, u] == 2000, 3, 6)
  inside = u + shift < W
  x, y = cr.pixel_of(col)
  assert np.array_equal(x[inside], (u + shift)[inside]) and np.array_equal(y[inside], v[inside])
  assert (col[~inside] == 0).all() and unc.tolist() == [int((~inside).sum())] and 0 < unc[0] < len(u)


# fx = fxc = 64, cx = cy = 0 and d = 1 make every step exact: uc = u + cxc, vc = v + cyc
def _exact(cxc, cyc, M=None, seed=3):
  d = holes(seed)
  d[d != 0] = 1000
  col, unc, _ = cr.backproject_color_ref(d, intrinsic(64.0, 0.0, 0.0), cr.self_coding_image(H, W)[None], intrinsic(64.0, cxc, cyc), M)
  u, v = own_pixels(d[0])
  uc = cr.project(d[0], intrinsic(64.0, 0.0, 0.0), intrinsic(64.0, cxc, cyc), M)[0]
  return d[0], u, v, uc, col, int(unc[0])


def test_half_pixel_ties_go_to_floor_of_uc_plus_half():
  d, u, v, uc, col, unc = _exact(0.5, 0.0)
  assert np.array_equal(uc, u + 0.5)  # exact half-integers
  x, y = cr.pixel_of(col)
  inside = u + 1 < W
  assert np.array_equal(x[inside], u[inside] + 1) and np.array_equal(y[inside], v[inside])
  assert (col[~inside] == 0).all() and unc == (u == W - 1).sum() > 0  # px = Wc: not coloured
  d, u, v, uc, col, unc = _exact(-1.5, 0.0)  # negative half-integers: floor, not truncation
  assert np.array_equal(uc, u - 1.5)
  x, y = cr.pixel_of(col)
  inside = u >= 1
  assert np.array_equal(x[inside], u[inside] - 1) and unc == (u == 0).sum() > 0 and (col[~inside] == 0).all()  # px = -1


def test_points_that_no_pixel_covers_are_black_and_counted():
  d, u, v, _, col, unc = _exact(0.0, 0.5)  # py = Hc for the last row
  assert unc == (v == H - 1).sum() > 0 and (col[v == H - 1] == 0).all() and np.array_equal(cr.pixel_of(col)[1][v < H - 1], v[v < H - 1] + 1)
  flip = np.diag([1.0, 1.0, -1.0, 1.0])  # q2 = -d < 0: behind the colour camera, although (uc, vc) may fall inside the image
  d, u, v, _, col, unc = _exact(0.0, 0.0, flip)
  assert unc == len(u) > 100 and (col == 0).all()
  flat = np.eye(4)
  flat[2, 2] = 0.0  # q2 = 0: uc is infinite, or NaN on the principal column
  d, u, v, uc, col, unc = _exact(0.0, 0.0, flat)
  assert not np.isfinite(uc).any() and np.isnan(uc).any() and unc == len(u) and (col == 0).all()
  far = np.eye(4)
  far[0, 3] = np.inf  # q2 > 0, uc not finite
  d, u, v, uc, col, unc = _exact(0.0, 0.0, far)
  assert np.isinf(uc).all() and unc == len(u) and (col == 0).all()
  # planted one by one in a frame that is coloured otherwise: a huge principal point for a few rows cannot be done per pixel, so
  # three one-pixel frames instead, each with its own count
  one = np.array([[[1000]], [[1000]], [[0]]], np.uint16)
  img = np.full((3, 1, 1, 3), 9, np.uint8)
  col, unc, offs = cr.backproject_color_ref(one, intrinsic(64.0, 0.0, 0.0), img, intrinsic(64.0, 0.0, 0.0))
  assert col.tolist() == [[9, 9, 9], [9, 9, 9]] and unc.tolist() == [0, 0, 0] and offs.tolist() == [0, 1, 2, 2]
  col, unc, offs = cr.backproject_color_ref(one, intrinsic(64.0, 0.0, 0.0), img, intrinsic(64.0, 1.0, 0.0))
  assert col.tolist() == [[0, 0, 0], [0, 0, 0]] and unc.tolist() == [1, 1, 0]


def test_features_restated_by_hand():
  vox = dict(vox_offsets=np.array([0, 2, 3]), side_offsets=np.array([[0, 2], [0, 1]]), first_index=np.array([0, 2, 3], np.int32))
  color = np.array([[0, 255, 51], [9, 9, 9], [102, 153, 204], [255, 0, 1]], np.uint8)
  F0, F1 = cr.color_features_ref(color, vox)
  assert F0.dtype == np.float32 and F0.tolist() == np.array([[-0.5, 0.5, 0.2 - 0.5], [0.4 - 0.5, 0.6 - 0.5, 0.8 - 0.5]], np.float32).tolist()
  assert F1.tolist() == [[0.5, -0.5, np.float32(1 / 255 - 0.5)]]
  z = np.arange(12, dtype=np.float32).reshape(4, 3)
  F0, F1 = cr.color_features_ref(color, vox, z, [0, 1], 0.25, 0.5, out_rows=2, sentinel=-7.0)
  assert F0.tolist() == np.array([[-0.5, 0.5, 0.2 - 0.5], [0.4 - 0.5, 0.6 - 0.5, 0.8 - 0.5]], np.float32).tolist()  # jitter off on side 0
  assert F1.tolist() == [[np.float32(0.5 + (0.25 + 0.5 * 9)), np.float32(-0.5 + (0.25 + 0.5 * 10)), np.float32((1 / 255 - 0.5) + (0.25 + 0.5 * 11))],
                         [-7.0, -7.0, -7.0]]
  F0, _ = cr.color_features_ref(color, vox, out_rows=1, sentinel=-7.0)  # one row short: the second row is not written
  assert F0.tolist() == [[-0.5, 0.5, np.float32(0.2 - 0.5)]]


# ---- the host side ------------------------------------------------------------------------------------------------------------
def test_write_npz_with_a_colour(tmp_path):
  rng = np.random.RandomState(3)
  p, c = rng.normal(size=(100, 3)), rng.randint(0, 256, (100, 3)).astype(np.uint8)
  pc.write_npz(str(tmp_path / "plain.npz"), p)
  pc.write_npz(str(tmp_path / "a.npz"), p, c)
  pc.write_npz(str(tmp_path / "b.npz"), p, color=c)
  assert (tmp_path / "a.npz").read_bytes() == (tmp_path / "b.npz").read_bytes()
  with np.load(str(tmp_path / "a.npz")) as z:
    assert list(z.keys()) == ["pcd", "color"] and z["color"].dtype == np.uint8 and np.array_equal(z["color"], c)
    assert z["pcd"].tobytes() == np.load(str(tmp_path / "plain.npz"))["pcd"].tobytes()
  import zipfile
  with zipfile.ZipFile(str(tmp_path / "a.npz")) as za, zipfile.ZipFile(str(tmp_path / "plain.npz")) as zp:
    assert za.read("pcd.npy") == zp.read("pcd.npy") and zp.namelist() == ["pcd.npy"]
  with pytest.raises(ValueError, match="color"):
    pc.write_npz(str(tmp_path / "c.npz"), p, c[:-1])


def test_read_color_and_calibration(tmp_path):
  from PIL import Image
  rng = np.random.RandomState(4)
  a = rng.randint(0, 256, (6, 8, 4)).astype(np.uint8)
  sd = tmp_path / "scene"
  os.makedirs(sd / "color")
  os.makedirs(sd / "intrinsic")
  Image.fromarray(a[:, :, :3]).save(str(sd / "color" / "0.png"))
  Image.fromarray(a).save(str(sd / "color" / "1.png"))  # RGBA: the alpha channel is dropped
  Image.fromarray(a[:, :, 0]).save(str(sd / "color" / "2.png"))  # greyscale
  Image.fromarray(a[:, :, :3]).save(str(sd / "color" / "3.jpg"))
  for n in ("0", "1"):
    got = pc.read_color(pc.color_path(str(sd), n))
    assert got.dtype == np.uint8 and got.flags.c_contiguous and np.array_equal(got, a[:, :, :3])
  with pytest.raises(ValueError, match="RGB"):
    pc.read_color(pc.color_path(str(sd), "2"))
  assert pc.color_path(str(sd), "3").endswith("3.jpg") and pc.read_color(pc.color_path(str(sd), "3")).shape == (6, 8, 3)
  with pytest.raises(FileNotFoundError, match=r"color/7\.png.*7\.png"):
    pc.color_path(str(sd), "7")
  with pytest.raises(FileNotFoundError, match="intrinsic_color.txt"):
    pc.read_color_calibration(str(sd))
  Kc = intrinsic(1170.0, 647.75, 483.75)
  np.savetxt(str(sd / "intrinsic" / "intrinsic_color.txt"), Kc)
  got_K, M = pc.read_color_calibration(str(sd))
  assert np.array_equal(got_K, Kc) and np.array_equal(M, np.eye(4))  # no extrinsics: the identity
  Ec, Ed = np.eye(4), np.eye(4)
  Ec[:3, 3], Ed[0, 3] = [0.01, -0.02, 0.003], 0.5
  Ec[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
  np.savetxt(str(sd / "intrinsic" / "extrinsic_color.txt"), Ec)
  np.savetxt(str(sd / "intrinsic" / "extrinsic_depth.txt"), Ed)
  assert np.array_equal(pc.read_color_calibration(str(sd))[1], np.linalg.inv(Ec) @ Ed)


def _two_file_corpus(tmp_path, with_color=True):
  """Two frames whose voxels hold several points of different colours: the first point of a voxel is not the first of the file's
  points with that colour, so a wrong selection shows."""
  rng = np.random.RandomState(5)
  frames = []
  for k in range(2):
    base = np.stack([rng.uniform(0.0, 0.6, 400), rng.uniform(-0.3, 0.3, 400), rng.normal(0, 0.004, 400)], 1) + [0.01 * k, 0, 0]
    xyz = np.concatenate([base, base + rng.uniform(0, 0.004, base.shape)])[rng.permutation(800)]  # most voxels hold >= 2 points
    rgb = rng.randint(0, 256, (800, 3)).astype(np.uint8)
    frames.append((xyz, rgb))
    if with_color:
      pc.write_npz(str(tmp_path / ("f%d.npz" % k)), xyz, rgb)
    else:
      pc.write_npz(str(tmp_path / ("f%d.npz" % k)), xyz)
  (tmp_path / "pairs.txt").write_text("f0.npz f1.npz 0.5\n")
  return frames


def _cfg(tmp_path, extra=()):
  from pointcontrast_amd.lib.config import get_config
  return get_config(["data.dataset=ScanNetMatchPairDataset", "data.dataset_root_dir=%s" % tmp_path, "data.scannet_match_dir=pairs.txt",
                     "data.voxel_size=0.05"] + list(extra))


def test_dataset_takes_the_colour_of_every_voxels_first_point(tmp_path, built_lib):
  from oracle import loader_ref
  from pointcontrast_amd.lib.ddp_data_loaders import ScanNetMatchPairDataset
  frames = _two_file_corpus(tmp_path)
  plain = ScanNetMatchPairDataset("train", transform=None, random_rotation=False, random_scale=False, config=_cfg(tmp_path))[0]
  item = ScanNetMatchPairDataset("train", transform=None, random_rotation=False, random_scale=False,
                                 config=_cfg(tmp_path, ["data.use_color=True"]))[0]
  for s in range(2):
    xyz, rgb = frames[s]
    sel = loader_ref.sparse_quantize_index(xyz, 0.05)
    assert len(sel) < 0.8 * len(xyz) and np.array_equal(item[s], xyz[sel])
    want = rgb[sel].astype(np.float64) / 255.0 - 0.5
    assert item[4 + s].dtype == np.float64 and np.array_equal(item[4 + s], want)
    assert np.abs(item[4 + s]).max() <= 0.5 and len(np.unique(item[4 + s])) > 100
    assert np.array_equal(plain[4 + s], np.ones((len(sel), 3)))  # without the option: the reference's ones
  for k in (0, 1, 2, 3, 6, 7):  # the geometry does not depend on the option
    assert np.array_equal(plain[k], item[k])


def test_dataset_without_the_option_ignores_the_colours(tmp_path, built_lib):
  from pointcontrast_amd.lib.ddp_data_loaders import ScanNetMatchPairDataset
  _two_file_corpus(tmp_path)
  os.makedirs(tmp_path / "plain")
  _two_file_corpus(tmp_path / "plain", with_color=False)
  a = ScanNetMatchPairDataset("train", transform=None, random_rotation=False, random_scale=False, config=_cfg(tmp_path))[0]
  b = ScanNetMatchPairDataset("train", transform=None, random_rotation=False, random_scale=False, config=_cfg(tmp_path / "plain"))[0]
  assert len(a) == len(b) == 8
  for x, y in zip(a, b):
    assert x.dtype == y.dtype and np.array_equal(x, y)


def test_missing_colour_member_and_synthetic_dataset_raise(tmp_path, built_lib):
  from pointcontrast_amd.lib.config import get_config
  from pointcontrast_amd.lib.ddp_data_loaders import ScanNetMatchPairDataset, SyntheticScanNetPairDataset, make_data_loader
  _two_file_corpus(tmp_path, with_color=False)
  d = ScanNetMatchPairDataset("train", transform=None, random_rotation=False, random_scale=False, config=_cfg(tmp_path, ["data.use_color=True"]))
  with pytest.raises(ValueError, match=r"f0\.npz.*make_pair_corpus --color"):
    d[0]
  with pytest.raises(ValueError, match="use_color"):
    SyntheticScanNetPairDataset(config=get_config(["data.use_color=True"]))
  with pytest.raises(ValueError, match="use_color"):
    make_data_loader(get_config(["data.use_color=True", "misc.num_gpus=1"]), 2)
  assert len(SyntheticScanNetPairDataset(config=get_config([]))) == 64  # the default is untouched


def test_raw_pair_files_hand_the_colours_on(tmp_path, built_lib):
  from pointcontrast_amd.lib.pair_input import RawPairFiles
  frames = _two_file_corpus(tmp_path)
  item = RawPairFiles(_cfg(tmp_path, ["data.use_color=True"]))[0]
  assert len(item) == 4 and all(np.array_equal(item[s], frames[s][0]) and np.array_equal(item[2 + s], frames[s][1]) for s in range(2))
  assert item[2].dtype == np.uint8
  plain = RawPairFiles(_cfg(tmp_path))[0]
  assert len(plain) == 2 and np.array_equal(plain[0], frames[0][0])
