"""The view kernels (csrc/views.hip through functional.view_zbuffer / view_visible and lib/scan_views.py) on the device:
bit-identical to the numpy restatement (tests/views_ref.py) on a synthetic room and at every edge of the rule, the refused
arguments, and a corpus built from two synthetic scans that ScanNetMatchPairDataset and pair_match consume as is.
Criteria: none is a tolerance -- the arithmetic is fp64 with a fixed order and integer atomics, so everything is np.array_equal."""
import os

import numpy as np
import pytest
import torch

import views_ref as vr
from pointcontrast_amd import functional as PF
from pointcontrast_amd._lib import PcmiError
from pointcontrast_amd.lib import pair_corpus as pc
from pointcontrast_amd.lib import scan_views as sv

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMALL = dict(fx=30.0, fy=30.0, cx=15.5, cy=11.5, H=24, W=32, z_near=0.5, z_far=4.0)


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(points, w2c, cam, splat, rel_tol, d_points=None):
  """(device result as numpy, restatement)."""
  w2c = np.asarray(w2c, dtype=np.float64).reshape(-1, 4, 4)
  p = _dev(np.asarray(points, dtype=np.float64).reshape(-1, 3)) if d_points is None else d_points
  zbuf = PF.view_zbuffer(p, _dev(w2c), cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["H"], cam["W"], z_near=cam["z_near"],
                         z_far=cam["z_far"], splat=splat)
  rows, offs, offs_h, pixels, mask = PF.view_visible(p, _dev(w2c), cam["fx"], cam["fy"], cam["cx"], cam["cy"], zbuf, z_near=cam["z_near"],
                                                     z_far=cam["z_far"], rel_tol=rel_tol)
  got = dict(zbuf=zbuf.cpu().numpy(), rows=rows.cpu().numpy(), offsets=offs.cpu().numpy(), offsets_host=offs_h, pixels=pixels.cpu().numpy(),
             mask=mask.cpu().numpy())
  want = vr.render(points, w2c, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["H"], cam["W"], cam["z_near"], cam["z_far"], splat, rel_tol)
  return got, want


def _assert_same(got, want, what=""):
  for k in ("zbuf", "rows", "offsets", "pixels"):
    assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)
  assert np.array_equal(got["offsets_host"], want["offsets"]), what
  F, n = want["mask"].shape
  bits = np.zeros((F, (n + 63) // 64 * 64), bool)
  bits[:, :n] = want["mask"]
  words = (bits.reshape(F, -1, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)
  assert np.array_equal(got["mask"].view(np.uint64), words), what


@pytest.fixture(scope="module")
def room():
  xyz, color = vr.synthetic_room(20000)
  return xyz, color, vr.planted_poses(), vr.small_intrinsic(60, 80, 72.0)


@pytest.mark.parametrize("splat", [1, 3, 7])
@pytest.mark.parametrize("rel_tol", [0.0, 0.05])
def test_room_is_bit_identical_to_the_restatement(room, splat, rel_tol):
  xyz, _, poses, K = room
  cam = dict(fx=72.0, fy=72.0, cx=K[0, 2], cy=K[1, 2], H=60, W=80, z_near=0.1, z_far=10.0)
  got, want = _run(xyz, vr.world_to_camera(poses), cam, splat, rel_tol)  # 11 views: two groups of eight, the last one NaN
  _assert_same(got, want)
  sizes = np.diff(got["offsets"])
  assert (sizes[:8] > 0).all() and sizes[9] == 0 and sizes[10] == 0 and got["pixels"][9] == 0 and got["pixels"][10] == 0
  for f in range(11):
    assert (np.diff(got["rows"][got["offsets"][f]:got["offsets"][f + 1]]) > 0).all()
  if splat == 1 and rel_tol == 0.0:  # one pixel per point, no tolerance: what is visible is every pixel's nearest point
    assert (sizes >= got["pixels"]).all() and (sizes[:8] <= got["pixels"][:8] + 5).all() and (sizes[:8] > 700).all()
  if splat == 3:  # occlusion does something: the tolerance lets the surface behind the nearest point through, not the room behind it
    assert (sizes[:8] < 0.5 * got["pixels"][:8]).all()


def _edge_points():
  """Identity camera of SMALL, so Z = z exactly and u = 30 x / z + 15.5."""
  z = 1.0
  at = lambda px, py, zz=z: [(px - 15.5) * zz / 30.0, (py - 11.5) * zz / 30.0, zz]
  pts = [[0.0, 0.0, -1.0], [0.0, 0.0, 0.0],                       # behind the camera, in its centre
         at(16, 6, 0.5), at(24, 6, 4.0),                            # exactly z_near and z_far: projectable
         at(7, 3, np.nextafter(0.5, 0)), at(9, 3, np.nextafter(4.0, 5)),  # one ulp outside: not
         [np.nan, 0.0, 1.0], [0.0, np.nan, 1.0], [0.0, 0.0, np.nan], [np.inf, 0.0, 1.0], [0.0, -np.inf, 1.0], [0.0, 0.0, np.inf],
         [1e308, 0.0, 1.0],                                        # X fx overflows: a pixel at infinity
         at(-1, 5), at(32, 5), at(5, -1), at(5, 24), at(-1, -1), at(32, 24),  # the pixel just outside every border and corner
         at(-4, 18), at(35, 18), at(9, -4), at(9, 27),              # too far outside even for splat 7
         at(0, 0), at(31, 0), at(0, 23), at(31, 23), at(0, 12), at(31, 12), at(16, 0), at(16, 23),  # windows clipped at every border
         at(20, 15, 2.0), [(20 - 15.5) * 2.0 / 30.0, (15 - 11.5) * 2.0 / 30.0, 2.0 + 1e-12],  # equal float32 depth, one pixel
         at(12, 15, 2.0), at(12, 15, 2.05), at(12, 15, 2.2),       # behind one another: inside and outside rel_tol 0.05
         at(13, 16, 3.0)]                                          # hidden by its neighbour's window at splat >= 3 only
  return np.array(pts, dtype=np.float64)


@pytest.mark.parametrize("splat", [1, 3, 7])
@pytest.mark.parametrize("rel_tol", [0.0, 0.05])
def test_edges_of_the_rule(splat, rel_tol):
  pts = _edge_points()
  got, want = _run(pts, np.eye(4)[None], SMALL, splat, rel_tol)
  _assert_same(got, want)
  vis = set(got["rows"].tolist())
  assert {2, 3} <= vis and not vis & set(range(0, 2)) and not vis & set(range(4, 23))  # range ends in, everything outside out
  assert set(range(23, 31)) <= vis  # border pixels
  assert {31, 32} <= vis  # both of the equal float32 depths, also at rel_tol 0
  assert np.float32(pts[31, 2]) == np.float32(pts[32, 2]) and pts[31, 2] != pts[32, 2]
  assert 33 in vis and (34 in vis) == (rel_tol > 0) and 35 not in vis
  assert (36 in vis) == (splat == 1)
  zb = got["zbuf"][0]
  half = splat // 2
  if half:  # the points one pixel outside reach into the image with their windows
    assert zb[5, 0] == 1.0 and zb[5, 31] == 1.0 and zb[0, 5] == 1.0 and zb[23, 5] == 1.0
  assert np.isinf(zb[18, 0]) and np.isinf(zb[18, 31])  # the far-outside ones never do
  assert np.isfinite(zb[:half + 1, :half + 1]).all() and np.isfinite(zb[23 - half:, 31 - half:]).all()  # corner windows, clipped


def test_camera_looking_away_gives_an_empty_view_with_repeated_offsets(room):
  xyz, _, poses, K = room
  cam = dict(fx=72.0, fy=72.0, cx=K[0, 2], cy=K[1, 2], H=60, W=80, z_near=0.1, z_far=10.0)
  got, want = _run(xyz[:5000], vr.world_to_camera(poses[[0, 9, 1]]), cam, 3, 0.05)
  _assert_same(got, want)
  assert got["offsets"][1] == got["offsets"][2] > 0 and got["offsets"][3] > got["offsets"][2] and got["pixels"][1] == 0
  assert np.isinf(got["zbuf"][1]).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000])
def test_point_counts_around_the_word_and_block_sizes(n):
  rng = np.random.RandomState(n)
  pts = rng.uniform(-1.0, 1.0, (n, 3)) * [1.2, 0.9, 1.0] + [0.0, 0.0, 2.0]
  w2c = np.stack([np.eye(4), vr.world_to_camera(vr.look_pose([0.0, -2.0, 2.0], np.pi / 2, 0.0)[None])[0]][:1 + (n % 2)])  # F = 1 and 2
  got, want = _run(pts, w2c, SMALL, 3, 0.05)
  _assert_same(got, want, n)
  assert got["offsets"][-1] > 0 and got["mask"].shape == (len(w2c), (n + 63) // 64)


def test_more_views_than_one_group_and_f_equal_one(room):
  xyz, _, poses, K = room
  cam = dict(fx=36.0, fy=36.0, cx=19.5, cy=14.5, H=30, W=40, z_near=0.1, z_far=10.0)
  many = np.concatenate([poses[:8], poses[:8][::-1], poses[2:3]])  # 17 views: three groups, the last of one
  got, want = _run(xyz[:3000], vr.world_to_camera(many), cam, 3, 0.05)
  _assert_same(got, want)
  one, want1 = _run(xyz[:3000], vr.world_to_camera(many[16:]), cam, 3, 0.05)
  _assert_same(one, want1)
  assert np.array_equal(one["zbuf"][0], got["zbuf"][16]) and np.array_equal(one["rows"], got["rows"][got["offsets"][16]:])


def test_strided_rows():
  rng = np.random.RandomState(9)
  wide8 = rng.uniform(-1.0, 1.0, (700, 8)) + [0, 0, 2.0, 0, 0, 0, 2.0, 0]
  wide7 = rng.uniform(-1.0, 1.0, (700, 7)) + [0, 0, 0, 0, 2.0, 0, 0]
  d8, d7 = _dev(wide8), _dev(wide7)
  # row strides of 8 and 16 doubles are read in place; 7 is packed by the wrapper first
  for view, host in ((d8[:, :3], wide8[:, :3]), (d8[::2, 4:7], wide8[::2, 4:7]), (d7[:, 2:5], wide7[:, 2:5])):
    assert not view.is_contiguous()
    got, want = _run(host, np.eye(4)[None], SMALL, 3, 0.0, d_points=view)
    _assert_same(got, want)
    assert got["offsets"][-1] > 50


def test_empty_inputs_succeed():
  cam = SMALL
  w2c = _dev(np.eye(4)[None].repeat(2, 0))
  none = torch.zeros((0, 3), dtype=torch.float64, device=DEV)
  zbuf = PF.view_zbuffer(none, w2c, 30.0, 30.0, 15.5, 11.5, 24, 32)
  assert zbuf.shape == (2, 24, 32) and torch.isinf(zbuf).all()
  rows, offs, offs_h, pixels, mask = PF.view_visible(none, w2c, 30.0, 30.0, 15.5, 11.5, zbuf)
  assert rows.shape == (0,) and offs.tolist() == [0, 0, 0] and offs_h.tolist() == [0, 0, 0] and pixels.tolist() == [0, 0] and mask.shape == (2, 0)
  pts = _dev(np.array([[0.0, 0.0, 1.0]]))
  zbuf = PF.view_zbuffer(pts, w2c[:0], 30.0, 30.0, 15.5, 11.5, 24, 32)
  assert zbuf.shape == (0, 24, 32)
  rows, offs, offs_h, pixels, mask = PF.view_visible(pts, w2c[:0], 30.0, 30.0, 15.5, 11.5, zbuf)
  assert rows.shape == (0,) and offs.tolist() == [0] and offs_h.tolist() == [0] and pixels.shape == (0,)


def test_refused_arguments():
  from pointcontrast_amd._lib import check, lib
  pts = _dev(np.array([[0.0, 0.0, 1.0], [0.1, 0.0, 1.0]]))
  w2c = _dev(np.eye(4)[None])
  ok = dict(fx=30.0, fy=30.0, cx=15.5, cy=11.5, height=24, width=32)
  for splat in (0, 2, 4, 9, -1):
    with pytest.raises(PcmiError, match="splat"):
      PF.view_zbuffer(pts, w2c, splat=splat, **ok)
  for hw in ((0, 32), (24, 0), (-1, 32)):
    with pytest.raises(PcmiError, match="pixels"):
      PF.view_zbuffer(pts, w2c, 30.0, 30.0, 15.5, 11.5, hw[0], hw[1])
  for bad in (dict(fx=0.0), dict(fy=-1.0), dict(cx=np.nan), dict(z_near=0.0), dict(z_near=2.0, z_far=1.0), dict(z_far=np.inf)):
    with pytest.raises(PcmiError, match="camera"):
      PF.view_zbuffer(pts, w2c, **{**ok, **bad})
  zbuf = PF.view_zbuffer(pts, w2c, **ok)
  for tol in (-0.1, np.nan, np.inf):
    with pytest.raises(PcmiError, match="rel_tol"):
      PF.view_visible(pts, w2c, 30.0, 30.0, 15.5, 11.5, zbuf, rel_tol=tol)
  # the limits on n and F are refused before anything is read
  st = torch.cuda.current_stream().cuda_stream
  args = (30.0, 30.0, 15.5, 11.5, 24, 32, 0.1, 10.0)
  assert lib.pcmi_views_zbuffer(pts.data_ptr(), 3, 1 << 31, w2c.data_ptr(), 1, *args, 3, zbuf.data_ptr(), st) == lib.pcmi_views_zbuffer(
      pts.data_ptr(), 3, 2, w2c.data_ptr(), 4097, *args, 3, zbuf.data_ptr(), st) != 0
  assert lib.pcmi_views_rows(None, None, 1 << 31, 1, None, st) == lib.pcmi_views_rows(None, None, 2, 4097, None, st) != 0
  assert lib.pcmi_views_zbuffer(pts.data_ptr(), 2, 2, w2c.data_ptr(), 1, *args, 3, zbuf.data_ptr(), st) != 0  # row stride < 3
  big = (30.0, 30.0, 15.5, 11.5, 1 << 16, 1 << 15, 0.1, 10.0)  # F H W = 2^31
  with pytest.raises(PcmiError, match="2\\^31"):
    check(lib.pcmi_views_zbuffer(pts.data_ptr(), 3, 2, w2c.data_ptr(), 1, *big, 3, zbuf.data_ptr(), st))
  with pytest.raises(PcmiError, match="no CPU path"):
    PF.view_zbuffer(pts.cpu(), w2c, **ok)
  with pytest.raises(AssertionError, match="float64"):
    PF.view_zbuffer(pts.float(), w2c, **ok)
  with pytest.raises(AssertionError, match="w2c"):
    PF.view_zbuffer(pts, w2c.cpu(), **ok)
  with pytest.raises(AssertionError, match="zbuf"):
    PF.view_visible(pts, w2c, 30.0, 30.0, 15.5, 11.5, zbuf.double())
  got, want = _run(pts.cpu().numpy(), np.eye(4)[None], SMALL, 3, 0.0)  # the device is fine afterwards
  _assert_same(got, want)


def test_exact_workspace_and_one_byte_short(room):
  """pcmi_views_visible as a C caller uses it: a workspace of exactly the queried size, guarded behind, and one byte less."""
  import ctypes as C
  from pointcontrast_amd._lib import check, lib
  xyz, _, poses, K = room
  n, F, H, W = 4097, 3, 60, 80
  pts, w2c_h = xyz[:n], vr.world_to_camera(poses[:F])
  d_pts, w2c = _dev(pts), _dev(w2c_h)
  cam = (72.0, 72.0, K[0, 2], K[1, 2], H, W, 0.1, 10.0)
  zbuf = PF.view_zbuffer(d_pts, w2c, *cam[:6], z_near=0.1, z_far=10.0, splat=3)
  need = lib.pcmi_views_visible_workspace_bytes(n, F)
  assert 0 < need < 1 << 20
  buf = torch.full((need + 256,), 0x5a, dtype=torch.uint8, device=DEV)
  nw = (n + 63) // 64
  mask, start = (torch.empty((F, nw), dtype=torch.int64, device=DEV) for _ in range(2))
  offs, pixels = torch.empty(F + 1, dtype=torch.int64, device=DEV), torch.empty(F, dtype=torch.int64, device=DEV)
  offs_h = (C.c_int64 * (F + 1))()
  st = torch.cuda.current_stream().cuda_stream
  args = (d_pts.data_ptr(), 3, n, w2c.data_ptr(), F, *cam, 0.05, zbuf.data_ptr(), mask.data_ptr(), start.data_ptr(), offs.data_ptr(), offs_h,
          pixels.data_ptr(), buf.data_ptr())
  with pytest.raises(PcmiError, match="workspace too small"):
    check(lib.pcmi_views_visible(*args, need - 1, st))
  check(lib.pcmi_views_visible(*args, need, st))
  assert (buf[need:] == 0x5a).all()  # nothing written behind the workspace
  want = vr.render(pts, w2c_h, *cam, 3, 0.05)
  assert np.array_equal(np.frombuffer(offs_h, dtype=np.int64), want["offsets"]) and np.array_equal(pixels.cpu().numpy(), want["pixels"])
  rows = torch.empty(int(offs_h[F]), dtype=torch.int32, device=DEV)
  check(lib.pcmi_views_rows(mask.data_ptr(), start.data_ptr(), n, F, rows.data_ptr(), st))
  assert np.array_equal(rows.cpu().numpy(), want["rows"])


def test_two_runs_give_identical_bytes(room):
  xyz, _, poses, K = room
  cam = dict(fx=72.0, fy=72.0, cx=K[0, 2], cy=K[1, 2], H=60, W=80, z_near=0.1, z_far=10.0)
  a, _ = _run(xyz, vr.world_to_camera(poses[:8]), cam, 3, 0.05)
  b, _ = _run(xyz, vr.world_to_camera(poses[:8]), cam, 3, 0.05)
  for k in a:
    assert a[k].tobytes() == b[k].tobytes(), k


# ---- process_scan and the corpus ---------------------------------------------------------------------------------------------
def test_process_scan_equals_the_restatement_and_drops_as_planted(room):
  xyz, color, poses, K = room
  got = sv.process_scan(xyz, poses, K, 60, 80, color=color)
  want = vr.process_scan(xyz, poses, K, 60, 80, color=color)
  assert got["reasons"] == want["reasons"] == [""] * 8 + ["coverage", "empty", "pose"]
  assert got["dropped"] == want["dropped"] == {"pose": 1, "empty": 1, "coverage": 1}
  assert list(got["frames"]) == list(want["frames"]) == list(range(8)) and np.array_equal(got["valid"], want["valid"])
  assert np.array_equal(got["coverage"], want["coverage"])
  for k in range(8):
    assert got["rows"][k].dtype == np.int32 and np.array_equal(got["rows"][k], want["rows"][k])
    assert got["points"][k].dtype == np.float64 and np.array_equal(got["points"][k], xyz[want["rows"][k]])
    assert np.array_equal(got["centroids"][k], want["centroids"][k])
    assert got["colors"][k].dtype == np.uint8 and np.array_equal(got["colors"][k], color[want["rows"][k]])
  assert np.array_equal(got["C"], want["C"]) and np.array_equal(got["M"], want["M"])
  M = got["M"]
  ov = np.array([max(M[i, j], M[j, i]) for i in range(8) for j in range(i + 1, 8)])
  assert (ov >= 0.3).sum() >= 3 and ((ov > 0) & (ov < 0.3)).sum() >= 3
  assert set(got["gpu_s"]) >= {"views", "voxel_centroids", "overlap_counts"}
  plain = sv.process_scan(xyz, poses, K, 60, 80)
  assert "colors" not in plain and np.array_equal(plain["C"], got["C"])
  r = sv.render_views(xyz, poses, K, 60, 80)
  assert np.array_equal(r["coverage"], want["coverage"]) and np.array_equal(np.concatenate(want["rows"]), r["rows"][:r["offsets"][8]])
  none = sv.process_scan(xyz, poses[9:], K, 60, 80, color=color)  # nothing kept
  assert none["reasons"] == ["empty", "pose"] and none["points"] == [] and none["colors"] == [] and none["C"].shape == (0, 0)


def _tree_bytes(root):
  out = {}
  for dp, _, fs in os.walk(root):
    for f in fs:
      p = os.path.join(dp, f)
      out[os.path.relpath(p, root)] = open(p, "rb").read()
  return out


VIEW_ARGS = dict(n_views=8, height=60, width=80, focal=72.0, min_coverage=0.25)  # (20 000 points are sparse for the default 0.5)


@pytest.fixture(scope="module")
def scan_corpus(tmp_path_factory):
  """Two synthetic scans, one with colours (.npz) and one without (.npy), built twice with one seed and once with another."""
  root = tmp_path_factory.mktemp("scans")
  os.makedirs(root / "scans")
  xyz_a, col_a = vr.synthetic_room(20000, seed=1)
  xyz_b, _ = vr.synthetic_room(16000, seed=2, offset=(10.0, -3.0, 0.5))
  np.savez(str(root / "scans" / "room_a.npz"), xyz=xyz_a, color=col_a)
  np.save(str(root / "scans" / "room_b.npy"), xyz_b)
  logs = []
  out = sv.build_corpus_from_scans(str(root / "scans"), str(root / "a"), seed=0, log=logs.append, **VIEW_ARGS)
  sv.build_corpus_from_scans(str(root / "scans"), str(root / "b"), seed=0, **VIEW_ARGS)
  sv.build_corpus_from_scans(str(root / "scans"), str(root / "c"), seed=1, **VIEW_ARGS)
  return root, dict(room_a=(xyz_a, col_a), room_b=(xyz_b, None)), out, logs


def test_corpus_files_equal_the_restatement_and_are_deterministic(scan_corpus):
  root, scans, out, logs = scan_corpus
  assert [s["scene"] for s in out] == ["room_a", "room_b"] and len(logs) == 2 and "8 views" in logs[0] and "coverage" in logs[0]
  a, b, c = (_tree_bytes(str(root / d)) for d in "abc")
  assert a == b and set(a) >= {"room_a/views.npz", "room_b/views.npz", "room_a/pcd/overlap.txt", pc.LIST_NAME}
  assert a["room_a/views.npz"] != c["room_a/views.npz"] and a["room_b/views.npz"] != c["room_b/views.npz"]
  assert {k: v for k, v in a.items() if k.endswith("pcd/0.npz")} != {k: v for k, v in c.items() if k.endswith("pcd/0.npz")}
  all_lines = []
  for s in ("room_a", "room_b"):
    xyz, color = scans[s]
    with np.load(str(root / "a" / s / "views.npz")) as z:
      v = {k: z[k] for k in z.files}
    draws = sv.ViewDraws.from_members(v)
    assert np.array_equal(draws.poses(xyz), v["poses"])  # views.npz rebuilds its cameras
    assert np.array_equal(sv.ViewDraws.sample(sv.scene_rng(0, s), xyz, 8).poses(xyz), v["poses"])
    assert np.array_equal(v["intrinsic"], vr.small_intrinsic(60, 80, 72.0)) and v["image_size"].tolist() == [60, 80]
    assert (v["splat"], v["rel_tol"], v["min_coverage"], v["voxel_size"], v["seed"]) == (3, 0.05, 0.25, 0.05, 0)
    want = vr.process_scan(xyz, v["poses"], v["intrinsic"], 60, 80, color=color, min_coverage=0.25)
    assert v["reasons"].tolist() == want["reasons"] and np.array_equal(v["coverage"], want["coverage"])
    names = [str(f) for f in want["frames"]]
    assert sorted(os.listdir(root / "a" / s / "pcd")) == sorted([n + ".npz" for n in names] + ["overlap.txt"])
    for k, n in enumerate(names):
      with np.load(str(root / "a" / s / "pcd" / (n + ".npz"))) as z:
        assert np.array_equal(z["pcd"], want["points"][k])
        assert z.files == (["pcd", "color"] if color is not None else ["pcd"])
        if color is not None:
          assert np.array_equal(z["color"], want["colors"][k])
    M = want["M"]
    lines = ["%s/pcd/%s.npz %s/pcd/%s.npz %s" % (s, names[i], s, names[j], "{}".format(max(M[i, j], M[j, i])))
             for i in range(len(names)) for j in range(i + 1, len(names))]
    assert (root / "a" / s / "pcd" / "overlap.txt").read_text() == "".join(ln + "\n" for ln in lines)
    all_lines += lines
  kept = [ln for ln in all_lines if float(ln.split()[2]) >= 0.3]
  assert len(kept) >= 2 and any(ln.startswith("room_a") for ln in kept)
  assert (root / "a" / pc.LIST_NAME).read_text() == "".join(ln + "\n" for ln in kept)
  only = sv.build_corpus_from_scans(str(root / "scans"), str(root / "d"), seed=0, scenes=["room_b"], **VIEW_ARGS)
  assert [s["scene"] for s in only] == ["room_b"]
  assert {k: v for k, v in _tree_bytes(str(root / "d")).items() if k.startswith("room_b")} == {k: v for k, v in a.items() if k.startswith("room_b")}


def test_corpus_feeds_the_dataset_and_pair_match(scan_corpus):
  import random
  from pointcontrast_amd.lib.config import get_config
  from pointcontrast_amd.lib.ddp_data_loaders import ScanNetMatchPairDataset
  root = scan_corpus[0]
  target = str(root / "a")
  listed = (root / "a" / pc.LIST_NAME).read_text().splitlines()
  first_a = next(i for i, ln in enumerate(listed) if ln.startswith("room_a"))  # room_a has colours
  for extra in ([], ["data.use_color=True"]):
    cfg = get_config(["data.dataset=ScanNetMatchPairDataset", "data.dataset_root_dir=%s" % target, "data.scannet_match_dir=%s" % pc.LIST_NAME,
                      "data.voxel_size=0.05"] + extra)
    d = ScanNetMatchPairDataset("train", transform=None, random_rotation=False, random_scale=False, config=cfg)
    assert len(d) == len(listed)
    random.seed(0)
    np.random.seed(0)
    item = d[first_a]
    assert len(item) == 8 and len(item[0]) > 100 and len(item[1]) > 100 and len(item[6]) > 0
    if extra:
      assert np.abs(item[4]).max() <= 0.5 and len(np.unique(item[4])) > 50  # the scan's colours, not the reference's ones
  fa, fb, _ = listed[first_a].split()
  with np.load(os.path.join(target, fa)) as z:
    p0 = z["pcd"]
  with np.load(os.path.join(target, fb)) as z:
    p1 = z["pcd"]
  vox = PF.pair_voxelize(_dev(np.concatenate([p0, p1])), torch.tensor([0, len(p0), len(p0) + len(p1)]), 0.05)
  m = PF.pair_match(vox, torch.eye(4, dtype=torch.float64)[None], torch.tensor([0.075], dtype=torch.float64), 200000)
  totals = m["totals"].cpu().numpy()
  assert totals[2] == 0 and totals[0] > 50  # the two views share scan vertices: correspondences at distance 0 among them
