"""CPU tests of the pair-corpus builder: the numpy restatement against brute force, the export layout reader and the
list writer (pointcontrast_amd/lib/pair_corpus.py; the device side is tests/test_gpu_pair_corpus.py)."""
import os

import numpy as np
import pytest

import pair_corpus_ref as ref
from pointcontrast_amd.lib import pair_corpus as pc


def test_restated_counts_equal_brute_force():
  rng = np.random.RandomState(0)
  downs = [rng.uniform(0, 0.6, (n, 3)) for n in (40, 55, 1, 70)]
  downs.append(downs[0][:10] + 0.075)  # exact-ish ties along one axis
  for r in (0.075, 0.15):
    C = ref.overlap_counts(downs, r)
    assert (C == ref.overlap_counts_bruteforce(downs, r)).all()
    assert (np.diag(C) == 0).all() and C.sum() > 0


def test_restated_centroids_equal_a_per_voxel_loop():
  rng = np.random.RandomState(1)
  p = rng.normal(0, 0.3, (4000, 3)) + np.array([3.0, -2.0, 1.0])
  voxel = 0.05
  got = ref.voxel_centroids(p, voxel)
  origin = p.min(0) - 0.5 * voxel
  groups = {}
  for i, key in enumerate(map(tuple, np.floor((p - origin) / voxel).astype(np.int64))):
    groups.setdefault(key, []).append(i)  # dict order = first occurrence
  want = []
  for ids in groups.values():
    s = np.zeros(3)
    for i in ids:
      s = s + p[i]
    want.append(s / len(ids))
  assert got.shape == (len(groups), 3) and np.array_equal(got, np.asarray(want))


def test_restated_backprojection_follows_the_reference_formula():
  depth = np.array([[0, 1000], [2500, 65535]], np.uint16)
  K = np.array([[500.0, 0, 0.5, 0.01], [0, 400.0, 0.25, -0.02], [0, 0, 1, 0], [0, 0, 0, 1]])
  P = np.array([[0.0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]])
  got = ref.backproject(depth, P, K)
  rows = []
  for v in range(2):
    for u in range(2):
      if depth[v, u]:
        d = depth[v, u] / 1000.0
        x, y = (u - 0.5) * d / 500.0 + 0.01, (v - 0.25) * d / 400.0 - 0.02
        rows.append(P[:3, :3] @ [x, y, d] + P[:3, 3])
  assert got.shape == (3, 3) and np.allclose(got, rows, rtol=0, atol=1e-12)


def _write_png(path, a):
  from PIL import Image
  Image.fromarray(np.asarray(a, np.uint16)).save(path)


def _export(root, scene, names, shape=(4, 5), pose_missing=(), intrinsic=True):
  sd = os.path.join(root, scene)
  for sub in ("depth", "pose", "intrinsic"):
    os.makedirs(os.path.join(sd, sub), exist_ok=True)
  for n in names:
    _write_png(os.path.join(sd, "depth", "%s.png" % n), np.full(shape, 1000 + int(n), np.uint16))
    if n not in pose_missing:
      np.savetxt(os.path.join(sd, "pose", "%s.txt" % n), np.eye(4))
  if intrinsic:
    np.savetxt(os.path.join(sd, "intrinsic", "intrinsic_depth.txt"), ref.intrinsic_matrix(shape[1], shape[0]))
  return sd


def test_frames_come_in_numeric_order_with_frame_skip(tmp_path):
  sd = _export(str(tmp_path), "scene0000_00", ["0", "2", "10", "1", "25", "3"])
  open(os.path.join(sd, "depth", "notes.txt"), "w").close()
  assert pc.list_frames(sd) == ["0", "1", "2", "3", "10", "25"]
  assert pc.list_frames(sd, frame_skip=2) == ["0", "2", "10"]
  assert pc.list_frames(sd, frame_skip=4) == ["0", "10"]
  with pytest.raises(ValueError, match="frame_skip"):
    pc.list_frames(sd, frame_skip=0)


def test_16bit_png_depth_round_trips_through_pil(tmp_path):
  a = np.random.RandomState(2).randint(0, 65536, (48, 64)).astype(np.uint16)
  a[0, 0], a[0, 1] = 0, 65535
  _write_png(str(tmp_path / "7.png"), a)
  got = pc.read_depth(str(tmp_path / "7.png"))
  assert got.dtype == np.uint16 and np.array_equal(got, a)


def test_missing_pose_or_intrinsic_give_clear_errors(tmp_path):
  sd = _export(str(tmp_path), "s_pose", ["0", "1"], pose_missing=("1",))
  assert np.array_equal(pc.read_pose(sd, "0"), np.eye(4))
  with pytest.raises(FileNotFoundError, match=r"pose.*1\.txt.*1\.png"):
    pc.read_pose(sd, "1")
  sd = _export(str(tmp_path), "s_intr", ["0"], intrinsic=False)
  with pytest.raises(FileNotFoundError, match="intrinsic_depth.txt"):
    pc.read_intrinsic(sd)
  with pytest.raises(FileNotFoundError, match="depth"):
    pc.list_frames(str(tmp_path / "nowhere"))
  # build_corpus stops at the same errors before any GPU work
  with pytest.raises(FileNotFoundError, match="intrinsic_depth.txt"):
    pc.build_corpus(str(tmp_path), str(tmp_path / "out"), scenes=["s_intr"])


def test_list_writing_is_inclusive_relative_and_formatted(tmp_path):
  M = np.array([[0.0, 0.3, 0.1, 1 / 3], [0.2, 0.0, 0.29999999999999999, 0.0], [0.05, 0.31, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
  lines = pc.pair_lines("scene0001_00", ["0", "5", "10", "20"], M)
  assert lines[0] == "scene0001_00/pcd/0.npz scene0001_00/pcd/5.npz 0.3"
  assert lines[2] == "scene0001_00/pcd/0.npz scene0001_00/pcd/20.npz %s" % "{}".format(1 / 3)
  assert lines[3] == "scene0001_00/pcd/5.npz scene0001_00/pcd/10.npz 0.31"
  assert len(lines) == 6 and all(not ln.split()[0].startswith("/") for ln in lines)
  kept = pc.select_lines(lines, 0.3)
  assert [ln.split()[2] for ln in kept] == ["0.3", "{}".format(1 / 3), "0.31"]  # 0.3 itself is kept
  # the written list loads through ScanNetMatchPairDataset's parsing, paths joined to the target root
  root = tmp_path / "target"
  os.makedirs(root / "scene0001_00" / "pcd")
  for n in ("0", "5", "10", "20"):
    pc.write_npz(str(root / "scene0001_00" / "pcd" / ("%s.npz" % n)), np.full((3, 3), float(n)))
  pc._write_lines(str(root / pc.LIST_NAME), kept)
  from pointcontrast_amd.lib.config import get_config
  from pointcontrast_amd.lib.ddp_data_loaders import ScanNetMatchPairDataset
  cfg = get_config(["data.dataset=ScanNetMatchPairDataset", "data.dataset_root_dir=%s" % root,
                    "data.scannet_match_dir=%s" % pc.LIST_NAME])
  d = ScanNetMatchPairDataset("train", config=cfg)
  assert d.files == [ln.split()[:2] for ln in kept]
  for a, b in d.files:
    assert np.load(os.path.join(d.root, a))["pcd"].shape == (3, 3) and os.path.exists(os.path.join(d.root, b))


def test_npz_files_are_deterministic_and_load(tmp_path):
  p = np.random.RandomState(3).normal(size=(100, 3))
  pc.write_npz(str(tmp_path / "a.npz"), p)
  pc.write_npz(str(tmp_path / "b.npz"), p)
  assert (tmp_path / "a.npz").read_bytes() == (tmp_path / "b.npz").read_bytes()
  with np.load(str(tmp_path / "a.npz")) as z:
    assert list(z.keys()) == ["pcd"] and np.array_equal(z["pcd"], p)
