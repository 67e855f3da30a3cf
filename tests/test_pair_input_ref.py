"""tests/pair_input_ref.py (the restatement that tests/test_gpu_pair_input.py compares the kernels with) held to the host
loader it replaces -- ScanNetMatchPairDataset.__getitem__ + default_collate_pair_fn (lib/ddp_data_loaders.py) -- and PairDraws
to the dataset's consumption of the random streams.  No GPU."""
import random

import numpy as np
import pytest
import torch

import pair_input_ref as pr

VOXEL, MULT = 0.05, 1.5


def make_frames(seed, n_pairs=2, n=2500, dtype=np.float64):
  """Small overlapping frame pairs: a noisy floor and wall patch seen twice (the second frame a shifted subset)."""
  rng = np.random.RandomState(seed)
  frames = []
  for _ in range(n_pairs):
    floor = np.stack([rng.uniform(-0.7, 0.7, n), rng.uniform(-0.6, 0.6, n), rng.normal(0, 0.004, n)], 1)
    wall = np.stack([rng.uniform(-0.7, 0.7, n // 2), 0.6 + rng.normal(0, 0.004, n // 2), rng.uniform(0, 0.8, n // 2)], 1)
    a = np.concatenate([floor, wall])[rng.permutation(n + n // 2)] + np.array([1.3, -0.4, 0.9])
    b = a[rng.rand(len(a)) < 0.8] + rng.normal(0, 0.002, (1, 3))
    frames.append((a.astype(dtype), b[rng.permutation(len(b))].astype(dtype)))
  return frames


def write_corpus(tmp_path, frames):
  lines = []
  for i, (a, b) in enumerate(frames):
    np.savez(tmp_path / ("f%da.npz" % i), pcd=a)
    np.savez(tmp_path / ("f%db.npz" % i), pcd=b)
    lines.append("f%da.npz f%db.npz 0.5\n" % (i, i))
  (tmp_path / "pairs.txt").write_text("".join(lines))


def config(tmp_path, extra=()):
  from pointcontrast_amd.lib.config import get_config
  return get_config(["data.dataset=ScanNetMatchPairDataset", "data.dataset_root_dir=%s" % tmp_path, "data.scannet_match_dir=pairs.txt",
                     "data.voxel_size=%r" % VOXEL, "trainer.batch_size=2"] + list(extra))


def test_identity_draws_equal_the_host_loader_bit_for_bit(tmp_path, built_lib):
  from pointcontrast_amd.lib.ddp_data_loaders import dataset_str_mapping, default_collate_pair_fn
  from pointcontrast_amd.lib.pair_input import PairDraws
  frames = make_frames(1, n_pairs=3)
  write_corpus(tmp_path, frames)
  cfg = config(tmp_path)
  dset = dataset_str_mapping["ScanNetMatchPairDataset"](phase="train", transform=None, random_rotation=False, random_scale=False, config=cfg)
  want = default_collate_pair_fn([dset[i] for i in range(3)])
  d = PairDraws.identity(3)
  got = pr.pipeline(frames, d.scale, d.rot, d.jitter_on, None, VOXEL, MULT, random_rotation=False, jitter=None)
  assert set(want) <= set(got)
  for k, v in want.items():
    if k == "len_batch":
      assert got[k] == v
    else:
      assert got[k].dtype == v.numpy().dtype and np.array_equal(got[k], v.numpy()), k
  assert got["n_queries"] == len(np.unique(want["correspondences"][:, 0].numpy()))


def _numpy_route(frames, scale, rot):
  """The dataset's own arithmetic on the draws: np.mean, np.linalg.inv, @."""
  out = []
  for b, (a0, a1) in enumerate(frames):
    T = []
    xs = [scale[b] * a0, scale[b] * a1]
    for s in range(2):
      M = np.eye(4)
      M[:3, :3] = rot[2 * b + s]
      M[:3, 3] = rot[2 * b + s].dot(-np.mean(xs[s], axis=0))
      T.append(M)
    out.append((T[0], T[1], T[1] @ np.linalg.inv(T[0]), xs[0] @ T[0][:3, :3].T + T[0][:3, 3], xs[1] @ T[1][:3, :3].T + T[1][:3, 3]))
  return out


def test_rotated_scaled_case_agrees_with_numpy_route(built_lib):
  from oracle import loader_ref
  from pointcontrast_amd.lib import synthetic
  frames = make_frames(7, n_pairs=2)
  rng = np.random.RandomState(11)
  scale = np.array([0.9137, 1.1462])
  rot = np.stack([synthetic._rotation(rng.rand(3) - 0.5, 2 * np.pi * (rng.rand() - 0.5)) for _ in range(4)])
  raw = np.concatenate([a for f in frames for a in f])
  offsets = np.concatenate([[0], np.cumsum([len(a) for f in frames for a in f])])
  tf = pr.pair_transform(raw, offsets, scale, rot)
  vx = pr.pair_voxelize(tf["points"], offsets, VOXEL, tf["flags"])
  assert not vx["flags"].any()
  for b, (T0, T1, trans, x0, x1) in enumerate(_numpy_route(frames, scale, rot)):
    for got, want in ((tf["T"][2 * b], T0), (tf["T"][2 * b + 1], T1), (tf["trans"][b], trans)):
      assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    r = VOXEL * MULT * scale[b]
    sel, pts = [], []
    for s, x in enumerate((x0, x1)):
      # no coordinate / voxel_size within 1e-9 of an integer: the two routes cannot disagree on a floor
      q = x / VOXEL
      assert np.abs(q - np.rint(q)).min() > 1e-9
      lo, hi = offsets[2 * b + s], offsets[2 * b + s + 1]
      assert np.abs(tf["points"][lo:hi] - x).max() < 1e-12
      first = loader_ref.sparse_quantize_index(x, VOXEL)
      vlo, vhi = vx["vox_offsets"][2 * b + s], vx["vox_offsets"][2 * b + s + 1]
      assert np.array_equal(vx["first_index"][vlo:vhi], first + lo), "voxel sets"
      sel.append(first)
      pts.append(x[first])
    src = pts[0] @ trans[:3, :3].T + trans[:3, 3]
    dist = np.linalg.norm(src[:, None] - pts[1][None], axis=2)
    assert np.abs(dist - r).min() > 1e-9, "a distance within 1e-9 of the radius"
    want = np.argwhere(dist <= r)
    m, flag = pr._match_one(vx["points"][vx["vox_offsets"][2 * b]:vx["vox_offsets"][2 * b + 1]], tf["trans"][b],
                            vx["points"][vx["vox_offsets"][2 * b + 1]:vx["vox_offsets"][2 * b + 2]], np.float64(VOXEL * MULT) * scale[b], 0)
    assert flag == 0 and len(want) > 500 and np.array_equal(m, want), "match sets"


def test_batch_entry_points_agree_with_the_collated_pipeline(built_lib):
  """pair_match + pair_collate (what the kernels are compared with) against pipeline (built on synthetic.collate_pairs)."""
  from pointcontrast_amd.lib import synthetic
  frames = make_frames(3, n_pairs=3, dtype=np.float32)
  far = frames[1][1] + np.float32(50.0)  # pair 1: no match
  frames[1] = (frames[1][0], far)
  rng = np.random.RandomState(5)
  scale = np.array([1.0, 0.83, 1.17])
  rot = np.stack([synthetic._rotation(rng.rand(3) - 0.5, 2 * np.pi * (rng.rand() - 0.5)) for _ in range(6)])
  on = np.array([1, 0, 1, 1, 0, 1], bool)
  n = sum(len(a) for f in frames for a in f)
  noise = rng.standard_normal((n, 3)).astype(np.float32)
  want = pr.pipeline(frames, scale, rot, on, noise, VOXEL, MULT)
  raw = np.concatenate([a for f in frames for a in f])
  offsets = np.concatenate([[0], np.cumsum([len(a) for f in frames for a in f])])
  tf = pr.pair_transform(raw, offsets, scale, rot)
  vx = pr.pair_voxelize(tf["points"], offsets, VOXEL, tf["flags"])
  mt = pr.pair_match(vx, tf["trans"], np.float64(VOXEL * MULT) * scale, vx["flags"])
  co = pr.pair_collate(vx, tf["trans"], noise, on, 0.0, 0.01)
  for k in co:
    assert co[k].dtype == want[k].dtype and np.array_equal(co[k], want[k]), k
  assert np.array_equal(mt["pairs"], want["correspondences"]) and mt["totals"][1] == want["n_queries"]
  # the placeholder row of the matchless pair, and column 0 never decreases
  c = want["correspondences"]
  s0, s1 = vx["side_offsets"][0, 1], vx["side_offsets"][1, 1]
  assert mt["pair_counts"][1] == 1 and (c[mt["pair_counts"][0]] == [s0, s1]).all()
  assert (np.diff(c[:, 0]) >= 0).all()
  assert (want["sinput0_F"][:want["len_batch"][0][0]] != 1).any() and (want["sinput1_F"][:want["len_batch"][0][1]] == 1).all()


def test_flags_drop_the_pair_and_leave_the_neighbours(built_lib):
  frames = make_frames(9, n_pairs=3)
  bad = frames[1][0].copy()
  bad[17, 1] = np.nan
  raw = np.concatenate([a for f in frames for a in f])
  offsets = np.concatenate([[0], np.cumsum([len(a) for f in frames for a in f])])
  clean = pr.pair_voxelize(pr.pair_transform(raw, offsets, np.ones(3))["points"], offsets, VOXEL)
  raw2 = raw.copy()
  raw2[offsets[2] + 17, 1] = np.nan
  tf = pr.pair_transform(raw2, offsets, np.ones(3))
  vx = pr.pair_voxelize(tf["points"], offsets, VOXEL, tf["flags"])
  assert vx["flags"].tolist() == [0, pr.FLAG_NONFINITE, 0]
  assert vx["n_vox"].tolist() == clean["n_vox"][:2].tolist() + [0, 0] + clean["n_vox"][4:].tolist()
  mt = pr.pair_match(vx, tf["trans"], np.full(3, VOXEL * MULT), vx["flags"])
  assert mt["pair_counts"][1] == 0 and mt["pair_counts"][0] > 1 and mt["pair_counts"][2] > 1
  with pytest.raises(ValueError, match="pair 1"):
    pr.pipeline([frames[0], (bad, frames[1][1]), frames[2]], np.ones(3), None, np.zeros(6, bool), None, VOXEL, MULT, random_rotation=False)


def test_pair_draws_consume_the_streams_in_the_datasets_order(tmp_path, built_lib):
  from pointcontrast_amd.lib.ddp_data_loaders import FeatureJitter, dataset_str_mapping
  from pointcontrast_amd.lib.pair_input import PairDraws
  frames = make_frames(2, n_pairs=3)
  write_corpus(tmp_path, frames)
  cfg = config(tmp_path, ["trainer.use_random_scale=True", "trainer.use_random_rotation=True"])
  dset = dataset_str_mapping["ScanNetMatchPairDataset"](phase="train", transform=FeatureJitter(), random_rotation=True, random_scale=True,
                                                       manual_seed=True, config=cfg)
  random.seed(4)
  np.random.seed(4)
  items = [dset[i] for i in range(3)]
  random.seed(4)
  randg = np.random.RandomState()
  randg.seed(0)
  d = PairDraws.sample(cfg, 3, randg)
  assert d.scale.shape == (3,) and d.rot.shape == (6, 3, 3) and d.jitter_on.shape == (6,)
  assert (d.scale != 1).any()
  for b, (T0, T1, trans, x0, x1) in enumerate(_numpy_route(frames, d.scale, d.rot)):
    assert np.array_equal(items[b][7], trans), "pair %d: the dataset drew another scale or rotation" % b
    assert np.array_equal(d.jitter_on[2 * b:2 * b + 2], [(items[b][4] != 1).any(), (items[b][5] != 1).any()])
  i = PairDraws.identity(2)
  assert (i.scale == 1).all() and (i.rot == np.eye(3)).all() and not i.jitter_on.any()
  assert torch.is_tensor(torch.as_tensor(i.rot))
