"""CPU: tests/nearest_ref.py -- the restatement the GPU tests of csrc/nearest.hip compare with bit for bit -- held to the
reference's own procedure: np.linalg.inv(T) @ xyz of save_predictions (downstream/semseg/lib/utils.py:322-327),
scipy.spatial.KDTree(leafsize=500).query of test_pointcloud (lib/datasets/scannet.py:154-155), fast_hist / per_class_iu
(lib/utils.py:131-138)."""
import numpy as np
import pytest

import nearest_ref as nr


def test_voxel_centers_match_the_reference_expression():
  coords, T, _ = nr.lattice_case()
  inv = np.linalg.inv(T.reshape(4, 4))
  got = nr.voxel_centers(coords, inv.reshape(1, 16))
  xyz = np.hstack((coords[:, 1:].astype(np.float64) + 0.5, np.ones((len(coords), 1))))
  want = (inv @ xyz.T).T[:, :3]
  scale = np.abs(want).max()
  assert np.abs(got - want).max() <= 1e-12 * scale
  # a batch index outside [0, B): NaN, the other rows unchanged
  c2 = coords.copy()
  c2[5, 0] = 1
  c2[9, 0] = -1
  got2 = nr.voxel_centers(c2, inv.reshape(1, 16))
  assert np.isnan(got2[[5, 9]]).all()
  keep = np.ones(len(coords), bool)
  keep[[5, 9]] = False
  assert np.array_equal(got2[keep], got[keep])


def test_nearest_point_matches_the_kd_tree():
  spatial = pytest.importorskip("scipy.spatial")
  coords, T, query = nr.lattice_case()
  assert len(query) == 2049
  centers = nr.voxel_centers(coords, np.linalg.inv(T.reshape(4, 4)).reshape(1, 16))
  m, n = len(centers), len(query)
  idx, dist2 = nr.nearest_point(centers, [0, m], query, [0, n])
  d, tree_idx = spatial.KDTree(centers, leafsize=500).query(query)
  # the two nearest distances of every query, to set aside near-ties the KD-tree may resolve either way
  two = np.sort(np.linalg.norm(query[:, None, :] - centers[None, :, :], axis=2), axis=1)[:, :2]
  gap = (two[:, 1] - two[:, 0]) / two[:, 1]
  clear = gap > 1e-9
  print("centres %d, smallest relative gap %.3e, excluded %d of %d" % (m, gap.min(), int((~clear).sum()), n))
  assert (~clear).mean() <= 0.01
  assert np.array_equal(idx[clear], tree_idx[clear])
  assert np.allclose(np.sqrt(dist2), d, rtol=1e-12, atol=0)


def test_nearest_point_rules():
  ref = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [np.nan, 0, 0], [5, 5, 5.0]])
  query = np.array([[0.5, 0, 0], [0.9, 0, 0], [np.inf, 0, 0], [4, 4, 4], [0, 0, 0.0]])
  # scene 0: rows 0-3 of ref, queries 0-2; scene 1: EMPTY, query 3; scene 2: row 4, query 4
  idx, d2 = nr.nearest_point(ref, [0, 4, 4, 5], query, [0, 3, 4, 5])
  assert idx.tolist() == [0, 1, -1, -1, 4]  # tie -> lowest row; duplicate -> lowest row; non-finite query; empty scene; isolation
  assert d2[0] == 0.25 and np.isnan(d2[2]) and d2[3] == np.inf and d2[4] == 75.0
  assert d2[2:3].view(np.int64)[0] == nr.NAN_BITS


def test_seg_hist_matches_fast_hist():
  rng = np.random.RandomState(0)
  c, m, n = 20, 300, 1000
  pred = rng.randint(0, c, m)
  idx = rng.randint(-1, m, n)
  labels = rng.choice(np.concatenate([np.arange(c), [255, -3, c]]), n)
  hist, pp, missing = nr.seg_hist(pred, idx, labels, c)
  have = idx >= 0
  # fast_hist(pred[idx], label) of lib/utils.py:131-133 on the rows that have a neighbour
  p, l = pred[idx[have]], labels[have]
  k = (l >= 0) & (l < c)
  want = np.bincount(c * l[k].astype(int) + p[k], minlength=c ** 2).reshape(c, c)
  assert np.array_equal(hist, want) and missing == int((~have).sum())
  assert np.array_equal(pp[have], p) and (pp[~have] == -1).all()
  hist_id, pp_id, miss_id = nr.seg_hist(pred, None, labels[:m], c)
  assert miss_id == 0 and np.array_equal(pp_id, pred)
  with np.errstate(divide="ignore", invalid="ignore"):
    iu = np.diag(want) / (want.sum(1) + want.sum(0) - np.diag(want))  # per_class_iu, lib/utils.py:136-138
  assert np.array_equal(nr.per_class_iu(hist), iu, equal_nan=True)
