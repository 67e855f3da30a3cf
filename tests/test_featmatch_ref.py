"""tests/featmatch_ref.py held to independent ground on the CPU: the nearest neighbour against a float64 brute force, the
frame construction against exact poses, Kabsch against a known transform, and the evaluator's metrics against a planted
answer.  tests/test_gpu_featmatch.py then holds the device to the restatement."""
import numpy as np
import pytest

import featmatch_ref as fr


def test_nearest_neighbour_is_the_float64_brute_force():
  rng = np.random.RandomState(0)
  lens_q, lens_r = [5, 0, 40], [7, 9, 33]
  qo, ro = fr.offsets_of(lens_q), fr.offsets_of(lens_r)
  qf, rf = rng.normal(size=(qo[-1], 16)).astype(np.float32), rng.normal(size=(ro[-1], 16)).astype(np.float32)
  nn, d2 = fr.feat_nn(qf, qo, rf, ro)
  for b in range(3):
    for i in range(qo[b], qo[b + 1]):
      best, arg = np.inf, -1
      for j in range(ro[b], ro[b + 1]):  # the plainest possible loop, float64
        d = float(((qf[i].astype(np.float64) - rf[j].astype(np.float64)) ** 2).sum())
        if d < best:
          best, arg = d, j
      assert nn[i] == arg and abs(d2[i] - best) <= 1e-5 * best
  # rows as queries: repeats, descending order, and the rules for what cannot be matched
  rows = np.array([4, 4, 3, 0, 44, 6, 5], dtype=np.int32)
  nn2, d22 = fr.feat_nn(qf, qo, rf, ro, rows, np.array([0, 4, 4, 7]))
  assert np.array_equal(nn2[:4], nn[[4, 4, 3, 0]]) and nn2[4] == nn[44] and np.array_equal(nn2[5:], nn[[6, 5]])
  bad = np.array([4, 5, -1], dtype=np.int32)  # row 5 lies in pair 2's segment, not pair 0's
  nn3, d23 = fr.feat_nn(qf, qo, rf, ro, bad, np.array([0, 3, 3, 3]))
  assert nn3.tolist() == [nn[4], -1, -1] and np.isnan(d23[1:]).all()
  rf2 = rf.copy()
  rf2[nn[0]] = np.nan  # a non-finite reference row is never chosen
  qf2 = qf.copy()
  qf2[1, 3] = np.inf   # a non-finite query matches nothing
  nn4, d24 = fr.feat_nn(qf2, qo, rf2, ro)
  assert nn4[0] != nn[0] and nn4[0] >= 0 and nn4[1] == -1 and np.isnan(d24[1])
  nn5, _ = fr.feat_nn(qf, qo, rf[:0], np.zeros(4, dtype=np.int64))
  assert (nn5 == -1).all()
  # exact ties go to the lowest row
  rf3 = np.concatenate([rf[:7], rf[:7]])
  nn6, _ = fr.feat_nn(qf[:5], [0, 5], rf3, [0, 14])
  assert (nn6 < 7).all()


def test_frame_construction_returns_the_exact_transform():
  rng = np.random.RandomState(1)
  for _ in range(50):
    T = fr.random_pose(rng, 3.0)
    p = rng.uniform(-2, 2, (3, 3))
    q = p @ T[:3, :3].T + T[:3, 3]
    Rt, ok = fr.triple_transform(p, q)
    assert ok
    assert np.abs(Rt[:9].reshape(3, 3) - T[:3, :3]).max() <= 1e-12 and np.abs(Rt[9:] - T[:3, 3]).max() <= 1e-12
  # degenerate triangles are refused: a repeated point, three collinear points
  p = rng.uniform(-2, 2, (3, 3))
  assert not fr.triple_transform(np.stack([p[0], p[0], p[2]]), p)[1]
  assert not fr.triple_transform(np.stack([p[0], p[0] + (p[1] - p[0]), p[0] + 2 * (p[1] - p[0])]), p)[1]


def test_kabsch_recovers_a_known_transform():
  from pointcontrast_amd.lib.feature_match import kabsch, pose_errors
  rng = np.random.RandomState(2)
  for reflect in (False, True):
    T = fr.random_pose(rng, 2.0)
    P = rng.uniform(-1, 1, (300, 3))
    if reflect:
      P[:, 2] *= 1e-9  # an almost planar set: the reflection fix decides the sign of the third axis
    Q = P @ T[:3, :3].T + T[:3, 3]
    m = len(P)
    best, Rt = np.array([0], dtype=np.int32), np.concatenate([T[:3, :3].reshape(-1), T[:3, 3]])[None]
    sums = fr.rigid_sums(P, Q, [0, m], best, Rt, 0.1)
    assert sums[0, 0] == m
    R, t = kabsch(sums[0])
    assert np.abs(R - T[:3, :3]).max() <= 1e-6 and np.abs(t - T[:3, 3]).max() <= 1e-6 and np.linalg.det(R) > 0
    R2, t2 = fr.kabsch_points(P, Q)
    assert np.abs(R - R2).max() <= 1e-6 and np.abs(t - t2).max() <= 1e-6
    rte, rre = pose_errors(R, t, T)
    assert rte <= 1e-6 and rre <= 1e-3
  assert kabsch(np.zeros(16)) is None


def test_ransac_and_stats_rules():
  rng = np.random.RandomState(3)
  T = fr.random_pose(rng, 1.0)
  P = rng.uniform(-1, 1, (40, 3))
  Q = fr.apply_rigid(T, P)
  Q[30:] += 5.0  # ten outliers
  tri = np.array([[[0, 1, 2], [0, 0, 2], [0, 1, 40], [30, 31, 32], [3, 4, 5]]], dtype=np.int32)
  counts, best, Rt = fr.ransac_score(P, Q, [0, 40], tri, 0.01)
  assert counts[0].tolist() == [30, -1, -1, 10, 30] and best[0] == 0  # the tie goes to the lowest hypothesis
  assert np.abs(Rt[0, :9].reshape(3, 3) - T[:3, :3]).max() <= 1e-12
  c2, b2, _ = fr.ransac_score(P[:2], Q[:2], [0, 2], tri, 0.01)
  assert (c2 == -1).all() and b2[0] == -1
  # match_stats: a threshold placed exactly on a residual counts it
  Pi = rng.randint(-5, 5, (40, 3)).astype(np.float64)
  Qi = Pi + np.array([3.0, 4.0, 0.0])  # every residual is exactly 25
  cnt, r2 = fr.match_stats(Pi, Qi, np.eye(4)[None], [0, 40], np.arange(40), [5.0, np.nextafter(5.0, 0.0)])
  assert (r2 == 25.0).all() and cnt[0, fr.HITS] == 40 and cnt[0, fr.HITS + 1] == 0
  assert cnt[0, fr.N_QUERY] == 40 and cnt[0, fr.N_VALID] == 40


PLANT = dict(n=400, c=32, voxel_size=0.05)


def planted_batch(seeds=(10, 11)):
  return fr.collate_planted([fr.planted_pair(np.random.RandomState(s), **PLANT) for s in seeds])


def test_planted_pair_is_recovered():
  """Cloud 1 is a rigid copy of cloud 0, snapped to voxels, with 30 % clutter; features are shared unit vectors plus
  N(0, 0.02) noise per channel (two unrelated unit vectors in 32 dimensions are sqrt(2) apart, corresponding ones about
  0.02 sqrt(64) = 0.16: the nearest neighbour of a kept row is its partner).  The restatement alone must recover the planted
  pose to one voxel and 1 degree and match at least 90 % of the rows that have a partner."""
  from pointcontrast_amd.lib.feature_match import MatchDraws
  batch = planted_batch()
  draws = MatchDraws.sample(batch["len_batch"], None, 256, np.random.RandomState(5))
  ev = fr.EvaluatorRef(PLANT["voxel_size"], hit_thresholds=(0.1, 0.05))
  ev.step(batch["F0"], batch["F1"], batch["C0"], batch["C1"], batch["T"], batch["len_batch"], batch["corr"], None, None,
          draws.triples)
  m = ev.compute_metrics()
  assert m["n_pairs"] == 2
  assert m["hit_ratio_overlap@0.1"] >= 0.9
  assert 0.6 <= m["hit_ratio@0.1"] <= 0.75  # 70 % of the rows have a partner
  assert m["feature_match_recall@0.1"] == 1.0 and m["registration_recall"] == 1.0
  assert m["mutual_ratio"] >= 0.6
  assert (m["pairs"]["rte"] <= PLANT["voxel_size"]).all() and (m["pairs"]["rre_deg"] <= 1.0).all()
  # sampled queries: the same answer from a subset
  draws = MatchDraws.sample(batch["len_batch"], 150, 256, np.random.RandomState(6))
  assert draws.query_offsets.tolist() == [0, 150, 300] and (np.diff(draws.query_rows[:150]) > 0).all()
  assert (np.sort(draws.triples, 2)[:, :, 1:] != np.sort(draws.triples, 2)[:, :, :-1]).all() and draws.triples.max() < 150
  ev = fr.EvaluatorRef(PLANT["voxel_size"])
  ev.step(batch["F0"], batch["F1"], batch["C0"], batch["C1"], batch["T"], batch["len_batch"], batch["corr"], draws.query_rows,
          draws.query_offsets, draws.triples)
  m = ev.compute_metrics()
  assert m["hit_ratio_overlap@0.1"] >= 0.9 and m["registration_recall"] == 1.0


def test_validation_loader_is_repeatable_and_leaves_the_global_generators_alone(built_lib, tmp_path):
  """data.val_match_dir: the training dataset class over a second list, in list order, without scale or jitter, rotations
  re-seeded per pass -- and no draw from `random`, numpy's or torch's global generator, which belong to the training run."""
  import random
  import torch
  from pointcontrast_amd.lib.config import get_config
  from pointcontrast_amd.lib.ddp_data_loaders import make_val_data_loader
  rng = np.random.RandomState(0)
  names = []
  for k in range(3):
    pts = rng.uniform(0, 1, (400, 3)) * [1.0, 1.0, 0.02]  # a slab: a few hundred 5 cm voxels
    np.savez(tmp_path / ("f%d.npz" % k), pcd=pts)
    names.append("f%d.npz" % k)
  (tmp_path / "val.txt").write_text("f0.npz f1.npz 0.5\nf1.npz f2.npz 0.4\nf2.npz f0.npz 0.6\n")
  over = ["data.dataset=ScanNetMatchPairDataset", "data.dataset_root_dir=%s" % tmp_path, "data.voxel_size=0.05"]
  with pytest.raises(ValueError, match="val_match_dir"):
    make_val_data_loader(get_config(over), 2)
  loader = make_val_data_loader(get_config(over + ["data.val_match_dir=val.txt", "trainer.use_random_scale=True"]), 2)
  random.seed(1), np.random.seed(1), torch.manual_seed(1)
  before = (random.getstate(), np.random.get_state()[1].copy(), torch.get_rng_state().clone())
  passes = []
  for _ in range(2):
    loader.dataset.reset_seed()  # what ContrastiveLossTrainer.validate does in front of every pass
    passes.append(list(loader))
  assert random.getstate() == before[0] and np.array_equal(np.random.get_state()[1], before[1])
  assert torch.equal(torch.get_rng_state(), before[2])
  assert [len(b["len_batch"]) for b in passes[0]] == [2, 1], "three pairs in list order, batches of two, nothing dropped"
  for a, b in zip(*passes):
    assert a.keys() == b.keys()
    for k in a:
      assert (torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k]), k
  first = passes[0][0]
  assert (first["sinput0_F"] == 1).all(), "no feature jitter"
  assert not torch.equal(first["T_gt"][:4], torch.eye(4)), "the rotations are on"


def test_too_few_matches_is_a_registration_failure_not_an_error():
  batch = fr.collate_planted([fr.planted_pair(np.random.RandomState(4), n=2, c=16, voxel_size=0.05, clutter=0.0)])
  ev = fr.EvaluatorRef(0.05)
  ev.step(batch["F0"], batch["F1"], batch["C0"], batch["C1"], batch["T"], batch["len_batch"], None, None, None,
          np.zeros((1, 8, 3), dtype=np.int32))
  m = ev.compute_metrics()
  assert m["registration_recall"] == 0.0 and m["n_pairs"] == 1 and m["rte"] == 0.0
  assert m["hit_ratio_overlap@0.1"] == 0.0  # no correspondences were given
