"""CPU tests of the virtual views (pointcontrast_amd/lib/scan_views.py, csrc/views.hip's rule restated in tests/views_ref.py):
the restatement against its own scalar spelling and against planted answers, the round trip with the other half of the corpus
code, the camera formula, the PLY reader, the scan readers and the command line.  Nothing here needs a device."""
import math
import os

import numpy as np
import pytest

import pair_corpus_ref as pr
import views_ref as vr
from pointcontrast_amd.lib import scan_views as sv


# ---- the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splat", [1, 3, 5])
def test_vectorised_equals_scalar(splat):
  rng = np.random.RandomState(splat)
  pts = rng.uniform(-2.0, 2.0, (300, 3)) + [0.0, 0.0, 2.5]
  pts[5], pts[6] = [np.nan, 0, 1], [0, np.inf, 1]
  w2c = np.stack([np.eye(4), vr.world_to_camera(vr.look_pose([0.5, -3.0, 2.5], 1.4, -0.2)[None])[0]])
  cam = dict(fx=20.0, fy=22.0, cx=11.5, cy=8.5, H=18, W=24, z_near=0.5, z_far=4.0)
  for tol in (0.0, 0.05):
    a = vr.render(pts, w2c, splat=splat, rel_tol=tol, **cam)
    b = vr.render_scalar(pts, w2c, splat=splat, rel_tol=tol, **cam)
    for k in ("zbuf", "rows", "offsets", "pixels"):
      assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (k, tol)
    assert 0 < a["offsets"][1] < 300 and a["offsets"][2] > a["offsets"][1]  # both views see some, neither sees all


def _plane(z, ext):
  a = np.arange(-ext, ext + 1e-9, 0.03)
  x, y = np.meshgrid(a, a)
  return np.stack([x.ravel(), y.ravel(), np.full(x.size, z)], 1)


@pytest.mark.parametrize("splat", [1, 3])
@pytest.mark.parametrize("rel_tol", [0.0, 0.02])
def test_two_parallel_planes_the_front_one_hides_the_back_one(splat, rel_tol):
  cam = dict(fx=30.0, fy=30.0, cx=15.5, cy=11.5, H=24, W=32, z_near=0.1, z_far=10.0)
  front, back = _plane(2.0, 1.5), _plane(3.0, 2.5)
  eye = np.eye(4)[None]
  r = vr.render(np.concatenate([front, back]), eye, splat=splat, rel_tol=rel_tol, **cam)
  vis = r["mask"][0]
  ok, px, py, _ = vr.project(front, eye[0], 30.0, 30.0, 15.5, 11.5, 0.1, 10.0)
  in_image = ok & (px >= 0) & (px < 32) & (py >= 0) & (py < 24)
  assert not vis[len(front):].any()  # no back point
  assert np.array_equal(vis[:len(front)], in_image) and in_image.sum() == 3763  # every front point inside the image
  alone = vr.render(back, eye, splat=splat, rel_tol=rel_tol, **cam)
  ok, px, py, _ = vr.project(back, eye[0], 30.0, 30.0, 15.5, 11.5, 0.1, 10.0)
  in_image = ok & (px >= 0) & (px < 32) & (py >= 0) & (py < 24)
  assert np.array_equal(alone["mask"][0], in_image) and in_image.sum() == 8480
  assert r["pixels"][0] == alone["pixels"][0] == 24 * 32


def test_round_trip_with_back_projection():
  """The points pair_corpus_ref back-projects from a depth frame, rendered from that frame's own pose and intrinsic at splat
  1, rel_tol 0: every point lands in the pixel it came from (one point per pixel, so each is its pixel's minimum) and the
  occupied pixels are the frame's non-zero ones.  Exact here: |u - pixel| after the two fp64 transforms is ~1e-12, far from
  the 0.5 at which floor(u + 0.5) would move."""
  depths, poses, K = pr.synthetic_scene(2, width=64, height=48)
  for f in range(2):
    pts = pr.backproject(depths[f], poses[f], K)
    r = vr.render(pts, np.linalg.inv(poses[f])[None], K[0, 0], K[1, 1], K[0, 2], K[1, 2], 48, 64, 0.01, 100.0, 1, 0.0)
    assert len(pts) > 2500 and r["mask"].all() and np.array_equal(r["rows"], np.arange(len(pts)))
    assert np.array_equal(np.isfinite(r["zbuf"][0]), depths[f] != 0) and r["pixels"][0] == (depths[f] != 0).sum()


@pytest.fixture(scope="module")
def room_scan():
  xyz, color = vr.synthetic_room(20000)
  poses = vr.planted_poses()
  K = vr.small_intrinsic(60, 80, 72.0)
  return xyz, color, poses, K, vr.process_scan(xyz, poses, K, 60, 80, color=color)


def test_planted_cameras_give_pairs_on_both_sides_of_the_threshold(room_scan):
  xyz, color, poses, K, r = room_scan
  assert r["reasons"] == [""] * 8 + ["coverage", "empty", "pose"] and r["dropped"] == {"pose": 1, "empty": 1, "coverage": 1}
  assert list(r["frames"]) == list(range(8))
  M = r["M"]
  ov = np.array([max(M[i, j], M[j, i]) for i in range(8) for j in range(i + 1, 8)])
  assert (ov >= 0.3).sum() >= 3 and ((ov > 0) & (ov < 0.3)).sum() >= 3
  for k in range(8):
    assert np.array_equal(r["points"][k], xyz[r["rows"][k]]) and np.array_equal(r["colors"][k], color[r["rows"][k]])
    assert (np.diff(r["rows"][k]) > 0).all() and 400 < len(r["rows"][k]) < 5000


# ---- cameras -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up_axis", [0, 1, 2])
def test_camera_formula(up_axis):
  rng = np.random.RandomState(7 + up_axis)
  xyz = rng.uniform(-3.0, 4.0, (500, 3)) * [1.0, 2.0, 0.5]
  d = sv.ViewDraws.sample(rng, xyz, 40, up_axis=up_axis, height=(0.4, 0.9), pitch_deg=(-40, 10))
  assert d.index.min() >= 0 and d.index.max() < 500 and len(np.unique(d.index)) > 20
  for u in (d.u_height, d.u_yaw, d.u_pitch):
    assert u.shape == (40,) and (u >= 0).all() and (u < 1).all() and len(np.unique(u)) == 40
  P = d.poses(xyz)
  lo, hi = xyz.min(0), xyz.max(0)
  for f in range(40):
    R, t = P[f, :3, :3], P[f, :3, 3]
    assert np.allclose(R.T @ R, np.eye(3), atol=1e-14) and abs(np.linalg.det(R) - 1.0) < 1e-14
    assert np.array_equal(P[f, 3], [0, 0, 0, 1])
    assert (t >= lo).all() and (t <= hi).all()
    for a in range(3):
      if a != up_axis:
        assert lo[a] + sv.INSET <= t[a] <= hi[a] - sv.INSET
        assert t[a] == min(max(xyz[d.index[f], a], lo[a] + sv.INSET), hi[a] - sv.INSET)
    assert t[up_axis] == lo[up_axis] + 0.4 + d.u_height[f] * 0.5
    pitch = math.radians(-40 + d.u_pitch[f] * 50)
    assert abs(R[up_axis, 2] - math.sin(pitch)) < 1e-15  # forward's up component
    assert R[up_axis, 0] == 0.0 and R[up_axis, 1] <= 0.0  # right is level, down points down (|pitch| < 90 degrees)
  again = sv.ViewDraws.from_members(d.members())
  assert np.array_equal(again.poses(xyz), P)
  assert np.array_equal(sv.ViewDraws.sample(np.random.RandomState(3), xyz, 5).poses(xyz), sv.ViewDraws.sample(np.random.RandomState(3), xyz, 5).poses(xyz))


def test_camera_pose_agrees_with_the_tests_own_formula_and_inverts():
  for yaw, pitch in ((0.0, 0.0), (1.1, -0.4), (4.0, 0.2)):
    assert np.allclose(sv.camera_pose([1.0, 2.0, 3.0], yaw, pitch), vr.look_pose([1.0, 2.0, 3.0], yaw, pitch), atol=1e-15)
  poses = vr.planted_poses()
  w = sv.world_to_camera(poses)
  assert np.isnan(w[10]).all() and np.array_equal(w[:10], vr.world_to_camera(poses)[:10])
  assert np.allclose(w[0] @ poses[0], np.eye(4), atol=1e-14)
  with pytest.raises(ValueError, match="pose 0 is singular"):
    sv.world_to_camera(np.zeros((1, 4, 4)))


# ---- scans on disk -----------------------------------------------------------------------------------------------------
def _write_ply(path, xyz, color, binary, extra=True, fmt=None):
  """x y z [nx] [red green blue] [alpha], then a face element with a list property."""
  props = [("x", "float", "<f4"), ("y", "float", "<f4"), ("z", "double", "<f8")]
  if extra:
    props.append(("nx", "short", "<i2"))
  if color is not None:
    props += [("red", "uchar", "u1"), ("green", "uchar", "u1"), ("blue", "uchar", "u1")]
  if extra:
    props.append(("alpha", "uchar", "u1"))
  n = len(xyz)
  fmt = fmt or ("binary_little_endian 1.0" if binary else "ascii 1.0")
  head = ["ply", "format " + fmt, "comment written by the test", "element vertex %d" % n]
  head += ["property %s %s" % (t, p) for p, t, _ in props]
  head += ["element face 1", "property list uchar int vertex_indices", "end_header"]
  v = np.zeros(n, dtype=[(p, d) for p, _, d in props])
  v["x"], v["y"], v["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
  if extra:
    v["nx"], v["alpha"] = np.arange(n) - 3, 255
  if color is not None:
    v["red"], v["green"], v["blue"] = color[:, 0], color[:, 1], color[:, 2]
  with open(path, "wb") as f:
    f.write(("\n".join(head) + "\n").encode("ascii"))
    if binary:
      f.write(v.tobytes())
      f.write(np.array([3], "u1").tobytes() + np.array([0, 1, 2], "<i4").tobytes())
    else:
      for row in v:
        f.write((" ".join(repr(x.item()) for x in row) + "\n").encode("ascii"))
      f.write(b"3 0 1 2\n")


@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("with_color", [True, False])
def test_ply_reader(tmp_path, binary, with_color):
  rng = np.random.RandomState(11)
  xyz = rng.uniform(-5, 5, (37, 3))
  color = rng.randint(0, 256, (37, 3)).astype(np.uint8) if with_color else None
  path = str(tmp_path / "scan.ply")
  _write_ply(path, xyz, color, binary)
  got_xyz, got_color = sv.read_ply_vertices(path)
  want = np.stack([xyz[:, 0].astype(np.float32), xyz[:, 1].astype(np.float32), xyz[:, 2]], 1).astype(np.float64)
  assert got_xyz.dtype == np.float64 and np.array_equal(got_xyz, want)  # x, y float, z double, the short and alpha skipped
  if with_color:
    assert got_color.dtype == np.uint8 and np.array_equal(got_color, color)
  else:
    assert got_color is None
  _write_ply(path, xyz, color, binary, extra=False)
  assert np.array_equal(sv.read_ply_vertices(path)[0], want)


def test_ply_reader_refuses_what_it_does_not_read(tmp_path):
  xyz = np.zeros((3, 3))
  path = str(tmp_path / "bad.ply")
  _write_ply(path, xyz, None, True, fmt="binary_big_endian 1.0")
  with pytest.raises(ValueError, match="binary_big_endian 1.0"):
    sv.read_ply_vertices(path)
  with open(path, "wb") as f:
    f.write(b"ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nend_header\n0 0\n0 0\n")
  with pytest.raises(ValueError, match=r"\['x', 'y'\]"):
    sv.read_ply_vertices(path)
  with open(path, "wb") as f:
    f.write(b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nproperty list uchar int k\nend_header\n")
  with pytest.raises(ValueError, match="list property 'k'"):
    sv.read_ply_vertices(path)
  with open(path, "wb") as f:
    f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nend_header\n" + b"\0" * 40)
  with pytest.raises(ValueError, match="40 bytes after the header"):
    sv.read_ply_vertices(path)
  with open(path, "wb") as f:
    f.write(b"ply\nformat ascii 1.0\nelement vertex 1\nproperty half x\nend_header\n")
  with pytest.raises(ValueError, match="property half x"):
    sv.read_ply_vertices(path)
  with open(path, "wb") as f:
    f.write(b"not a ply")
  with pytest.raises(ValueError, match="not a PLY file"):
    sv.read_ply_vertices(path)


def test_scan_readers_and_listing(tmp_path):
  rng = np.random.RandomState(2)
  xyz = rng.uniform(0, 3, (20, 3))
  color = rng.randint(0, 256, (20, 3)).astype(np.uint8)
  np.savez(str(tmp_path / "a.npz"), xyz=xyz, color=color)
  np.savez(str(tmp_path / "b.npz"), xyz=xyz.astype(np.float32))
  np.save(str(tmp_path / "c.npy"), np.concatenate([xyz, color.astype(np.float64)], 1))
  np.save(str(tmp_path / "d.npy"), xyz)
  _write_ply(str(tmp_path / "e.ply"), xyz, color, True)
  os.makedirs(tmp_path / "scene0000_00")
  _write_ply(str(tmp_path / "scene0000_00" / "scene0000_00_vh_clean_2.ply"), xyz, color, True)
  os.makedirs(tmp_path / "not_a_scan")
  (tmp_path / "notes.txt").write_text("x")
  found = sv.list_scans(str(tmp_path))
  assert list(found) == ["a", "b", "c", "d", "e", "scene0000_00"] and found["scene0000_00"].endswith("scene0000_00_vh_clean_2.ply")
  for s, has_color in (("a", True), ("b", False), ("c", True), ("d", False), ("e", True), ("scene0000_00", True)):
    x, c = sv.read_scan(found[s])
    assert x.dtype == np.float64 and x.shape == (20, 3) and (c is not None) == has_color
    if has_color:
      assert c.dtype == np.uint8 and np.array_equal(c, color)
  assert np.array_equal(sv.read_scan(found["a"])[0], xyz) and np.array_equal(sv.read_scan(found["b"])[0], xyz.astype(np.float32).astype(np.float64))
  np.save(str(tmp_path / "f.npy"), np.zeros((4, 5)))
  with pytest.raises(ValueError, match=r"\(4, 5\)"):
    sv.read_scan(str(tmp_path / "f.npy"))
  np.savez(str(tmp_path / "g.npz"), points=xyz)
  with pytest.raises(ValueError, match="no member 'xyz'"):
    sv.read_scan(str(tmp_path / "g.npz"))
  np.save(str(tmp_path / "a.npy"), xyz)
  with pytest.raises(ValueError, match="scene a is there twice"):
    sv.list_scans(str(tmp_path))


def test_scene_rng_depends_on_seed_and_scene_only():
  a = sv.scene_rng(0, "room1").random_sample(4)
  assert np.array_equal(a, sv.scene_rng(0, "room1").random_sample(4))
  assert not np.array_equal(a, sv.scene_rng(1, "room1").random_sample(4)) and not np.array_equal(a, sv.scene_rng(0, "room2").random_sample(4))


# ---- command line --------------------------------------------------------------------------------------------------------
def test_cli_takes_exactly_one_source(capsys):
  from pointcontrast_amd import make_pair_corpus as cli
  for argv in (["--target", "t"], ["--export", "e", "--scans", "s", "--target", "t"]):
    with pytest.raises(SystemExit) as e:
      cli.parse_args(argv)
    assert e.value.code == 2
  err = capsys.readouterr().err
  assert "one of the arguments --export --scans is required" in err and "not allowed with argument" in err
  a = cli.parse_args(["--export", "e", "--target", "t", "--voxel-size", "0.025", "--threshold", "0.4", "--frame-skip", "5", "--scenes", "s1", "s2",
                      "--color"])
  assert (a.export, a.scans, a.target, a.voxel_size, a.threshold, a.frame_skip, a.scenes, a.color) == ("e", None, "t", 0.025, 0.4, 5, ["s1", "s2"], True)
  a = cli.parse_args(["--export", "e", "--target", "t"])
  assert (a.voxel_size, a.threshold, a.frame_skip, a.scenes, a.color) == (0.05, 0.3, 1, None, False)
  a = cli.parse_args(["--scans", "s", "--target", "t"])
  assert (a.export, a.scans, a.views, a.seed, a.width, a.height, a.focal, a.splat, a.rel_tol, a.min_coverage) == \
      (None, "s", 64, 0, 320, 240, 288.0, 3, 0.05, 0.5)
  a = cli.parse_args(["--scans", "s", "--target", "t", "--views", "8", "--seed", "3", "--width", "80", "--height", "60", "--focal", "72", "--splat", "5",
                      "--rel-tol", "0.1", "--min-coverage", "0.2"])
  assert (a.views, a.seed, a.width, a.height, a.focal, a.splat, a.rel_tol, a.min_coverage) == (8, 3, 80, 60, 72.0, 5, 0.1, 0.2)
