"""Pins tests/pointset_ref.py (the CPU reference the GPU point-set tests compare against) and the import surface of
pointcontrast_amd.pointnet2_utils.  No GPU needed."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointset_ref as R  # noqa: E402


def _cloud(n, seed, scale=2.0):
  return (np.random.RandomState(seed).rand(n, 3).astype(np.float32) - 0.5) * scale + 1.5  # away from the origin's 1e-3 ball


def test_fps_picks_maximise_the_minimum_distance():
  """Every pick is, in float64, a point whose distance to the set chosen so far is the largest (up to float32 round-off of
  the squared distances: three roundings of 2^-24 each, bound 1e-6 relative)."""
  for n, m, seed in ((50, 20, 0), (700, 64, 1), (3000, 40, 2)):
    pts = _cloud(n, seed)
    got = R.fps(pts, m, tie_free=True)
    assert got[0] == 0 and len(set(got.tolist())) == m
    p64 = pts.astype(np.float64)
    mind = np.full(n, np.inf)
    for j in range(1, m):
      mind = np.minimum(mind, ((p64 - p64[got[j - 1]]) ** 2).sum(1))
      assert mind[got[j]] >= mind.max() * (1 - 1e-6), (n, j)


def test_fps_padding_ties_and_repeats():
  pts = _cloud(10, 3)
  pts[4] = pts[7] = (0.01, 0.01, 0.01)  # inside the 1e-3 ball: never chosen after pick 0
  got = R.fps(pts, 8)
  assert 4 not in got[1:] and 7 not in got[1:]
  dup = np.repeat(_cloud(3, 4), 2, axis=0)  # exact duplicates: the lower index of a pair wins
  assert R.fps(dup, 3).tolist() in ([0, 2, 4], [0, 4, 2])
  rep = R.fps(_cloud(3, 5), 7).tolist()  # m > n: every point once, then repeats
  assert sorted(rep[:3]) == [0, 1, 2] and set(rep[3:]) <= {0, 1, 2}
  assert R.fps(np.zeros((0, 3)), 4).tolist() == [-1] * 4
  assert R.fps(np.zeros((5, 3)), 3).tolist() == [0, 0, 0]  # no point qualifies


def test_ball_query_against_brute_force():
  rng = np.random.RandomState(6)
  xyz, new_xyz = rng.rand(2, 300, 3).astype(np.float32), rng.rand(2, 40, 3).astype(np.float32)
  for radius, nsample in ((0.01, 4), (0.2, 16), (0.6, 8)):
    d = ((xyz[:, None].astype(np.float64) - new_xyz[:, :, None].astype(np.float64)) ** 2).sum(-1)  # [B, np, n]
    r2 = float(np.float32(radius) * np.float32(radius))
    assert (np.abs(d - r2) > 1e-5 * r2).all(), "fixture: a distance too close to the radius for float32 / float64 to agree"
    got = R.ball_query(xyz, new_xyz, radius, nsample)
    for b in range(2):
      for q in range(40):
        hits = sorted(i for i in range(300) if d[b, q, i] < r2)[:nsample]
        want = (hits + [hits[0]] * (nsample - len(hits))) if hits else [0] * nsample
        assert got[b, q].tolist() == want, (radius, b, q)


def test_three_nn_against_brute_force():
  rng = np.random.RandomState(7)
  unknown, known = rng.rand(2, 60, 3).astype(np.float32), rng.rand(2, 90, 3).astype(np.float32)
  d = ((known[:, None].astype(np.float64) - unknown[:, :, None].astype(np.float64)) ** 2).sum(-1)  # [B, n, m]
  srt = np.sort(d, axis=-1)
  assert (np.diff(srt[..., :4], axis=-1) > 1e-5 * srt[..., 1:4]).all(), "fixture: near-tied neighbours"
  d2, idx = R.three_nn(unknown, known)
  assert (idx == np.argsort(d, axis=-1)[..., :3]).all()
  assert np.allclose(d2, srt[..., :3], rtol=1e-5)
  known[:, 5] = known[:, 2]  # a duplicated known point: the lower index comes first
  _, idx = R.three_nn(known[:, 2:3], known)
  assert idx[:, 0, :2].tolist() == [[2, 5], [2, 5]]


def test_gather_group_interpolate_gradients():
  torch.manual_seed(0)
  feat = torch.randn(2, 3, 7, dtype=torch.float64, requires_grad=True)
  idx = torch.randint(0, 7, (2, 5))
  idx3 = torch.randint(0, 7, (2, 4, 3))
  w = torch.rand(2, 4, 3, dtype=torch.float64)
  assert torch.equal(R.gather(feat, idx)[1, 2], feat[1, 2][idx[1]])
  assert torch.equal(R.group(feat, idx3)[0, 1, 3], feat[0, 1][idx3[0, 3]])
  want = sum(w[1, 2, k] * feat[1, 0, idx3[1, 2, k]] for k in range(3))
  assert abs(float((R.interpolate(feat, idx3, w)[1, 0, 2] - want).detach())) < 1e-12
  assert torch.autograd.gradcheck(lambda f: R.gather(f, idx), (feat,))
  assert torch.autograd.gradcheck(lambda f: R.group(f, idx3), (feat,))
  assert torch.autograd.gradcheck(lambda f: R.interpolate(f, idx3, w), (feat,))
  g = R.grad_of(lambda f: R.gather(f, idx), feat, torch.ones(2, 3, 5))
  assert float(g.sum()) == 2 * 3 * 5


def test_pointnet2_utils_imports_without_a_gpu(built_lib):
  from pointcontrast_amd import pointnet2_utils as P
  for name in ("furthest_point_sample", "gather_operation", "three_nn", "three_interpolate", "grouping_operation", "ball_query",
               "QueryAndGroup", "GroupAll"):
    assert hasattr(P, name), name
  import pytest
  with pytest.raises(NotImplementedError):
    P.QueryAndGroup(0.2, 16, sample_uniformly=True)
  from pointcontrast_amd._lib import PcmiError
  with pytest.raises(PcmiError, match="no CPU path"):
    P.furthest_point_sample(torch.zeros(1, 8, 3), 4)
  from pointcontrast_amd.downstream import votenet
  assert callable(votenet.sample_seeds)
  xyz, feats = torch.rand(2, 6, 3), torch.rand(2, 4, 6)
  out = P.GroupAll()(xyz, None, feats)
  assert out.shape == (2, 7, 1, 6)
