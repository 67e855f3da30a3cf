"""Seeded inputs of the detection-head tests (tests/test_votenet_ref.py, tests/test_gpu_votenet_head.py)."""
import types

import numpy as np
import torch

PREDICTED = ("vote_xyz", "center", "objectness_scores", "heading_scores", "heading_residuals_normalized", "size_scores",
             "size_residuals_normalized", "sem_cls_scores")


def loss_inputs(B, num_points, num_seed, K, K2, H, S, Cls, seed, vote_factor=1):
  """(end_points of float32 / int64 CPU tensors with the reference's keys, config).  Some box_label_mask and vote_label_mask
  entries are zero.  aggregated_vote_xyz is placed so that sqrt(dist1 + 1e-6) stays clear of the 0.3 / 0.6 thresholds."""
  rng = np.random.RandomState(seed)
  f = lambda a: torch.from_numpy(np.asarray(a, np.float32))  # noqa: E731
  gt = rng.uniform(-3, 3, (B, K2, 3))
  # proposals at a chosen distance from a ground-truth centre: near (< 0.3), grey zone, far (> 0.6)
  radius = rng.choice([0.05, 0.15, 0.25, 0.4, 0.5, 0.8, 1.5], (B, K))
  direction = rng.normal(0, 1, (B, K, 3))
  direction /= np.linalg.norm(direction, axis=-1, keepdims=True)
  owner = rng.randint(0, K2, (B, K))
  agg = np.take_along_axis(gt, owner[..., None].repeat(3, -1), 1) + direction * radius[..., None]
  seed_xyz = rng.uniform(-3, 3, (B, num_seed, 3))
  mean_size_arr = rng.uniform(0.4, 1.5, (S, 3)).astype(np.float32)
  box_label_mask = (rng.rand(B, K2) > 0.25).astype(np.float32)
  box_label_mask[:, 0] = 1
  ep = dict(
      seed_xyz=f(seed_xyz), seed_inds=torch.from_numpy(np.stack([rng.choice(num_points, num_seed, replace=False) for _ in range(B)])),
      vote_xyz=f(np.repeat(seed_xyz, vote_factor, 1) + rng.normal(0, 0.3, (B, num_seed * vote_factor, 3))),
      aggregated_vote_xyz=f(agg), center=f(agg + rng.normal(0, 0.1, (B, K, 3))),
      objectness_scores=f(rng.normal(0, 1, (B, K, 2))), heading_scores=f(rng.normal(0, 1, (B, K, H))),
      heading_residuals_normalized=f(rng.normal(0, 1, (B, K, H))), size_scores=f(rng.normal(0, 1, (B, K, S))),
      size_residuals_normalized=f(rng.normal(0, 1, (B, K, S, 3))), sem_cls_scores=f(rng.normal(0, 1, (B, K, Cls))),
      center_label=f(gt), heading_class_label=torch.from_numpy(rng.randint(0, H, (B, K2))),
      heading_residual_label=f(rng.uniform(-0.2, 0.2, (B, K2))), size_class_label=torch.from_numpy(rng.randint(0, S, (B, K2))),
      size_residual_label=f(rng.uniform(-0.3, 0.3, (B, K2, 3))), sem_cls_label=torch.from_numpy(rng.randint(0, Cls, (B, K2))),
      box_label_mask=f(box_label_mask), vote_label=f(rng.normal(0, 0.5, (B, num_points, 9))),
      vote_label_mask=torch.from_numpy((rng.rand(B, num_points) > 0.4).astype(np.int64)))
  cfg = types.SimpleNamespace(num_heading_bin=H, num_size_cluster=S, num_class=Cls, mean_size_arr=mean_size_arr)
  return ep, cfg


def to_float64(ep, requires_grad=False):
  out = {}
  for k, v in ep.items():
    if v.is_floating_point():
      v = v.double()
      if requires_grad and k in PREDICTED:
        v = v.requires_grad_()
    out[k] = v
  return out


class DatasetConfig:
  """A dataset config as parse_predictions uses it: ScanNet style (zero_heading: class2angle is constantly 0) or SUN RGB-D
  style heading bins."""

  def __init__(self, num_heading_bin, mean_size_arr, num_class, zero_heading):
    self.num_heading_bin, self.mean_size_arr, self.num_class = num_heading_bin, np.asarray(mean_size_arr, np.float32), num_class
    self.num_size_cluster = self.mean_size_arr.shape[0]
    self.zero_heading = zero_heading

  def class2angle(self, pred_cls, residual, to_label_format=True):
    if self.zero_heading:
      return 0
    angle = pred_cls * (2 * np.pi / float(self.num_heading_bin)) + residual
    return angle - 2 * np.pi if to_label_format and angle > np.pi else angle

  def class2size(self, pred_cls, residual):
    return self.mean_size_arr[int(pred_cls)] + residual


def clustered_params(rng, K, n_clusters, rotated=True):
  """[K, 7] box parameters (camera centre, size, angle) jittered around n_clusters centres."""
  cen = rng.uniform(-2.5, 2.5, (n_clusters, 3))
  c = cen[rng.randint(0, n_clusters, K)] + rng.normal(0, 0.15, (K, 3))
  size = rng.uniform(0.5, 1.3, (K, 3))
  angle = rng.uniform(-np.pi, np.pi, (K, 1)) if rotated else np.zeros((K, 1))
  return np.concatenate([c, size, angle], 1)


def prediction_inputs(rng, B, K, N, H, S, Cls, n_clusters=6):
  """float32 arrays of a parse_predictions call (the reference's end_points keys) with clustered centres, and points placed
  so that some boxes hold many, some few and some none."""
  cen = rng.uniform(-2.5, 2.5, (B, n_clusters, 3))
  pick = rng.randint(0, n_clusters, (B, K))
  center = np.take_along_axis(cen, pick[..., None].repeat(3, -1), 1) + rng.normal(0, 0.12, (B, K, 3))
  pts = rng.uniform(-3.5, 3.5, (B, N, 3))
  dense = cen[:, : n_clusters // 2]  # half of the clusters sit in dense regions
  k = N // 2
  pts[:, :k] = np.take_along_axis(dense, rng.randint(0, dense.shape[1], (B, k))[..., None].repeat(3, -1), 1) + rng.normal(0, 0.3, (B, k, 3))
  return dict(
      center=center.astype(np.float32), heading_scores=rng.normal(0, 1, (B, K, H)).astype(np.float32),
      heading_residuals=rng.uniform(-0.25, 0.25, (B, K, H)).astype(np.float32), size_scores=rng.normal(0, 1, (B, K, S)).astype(np.float32),
      size_residuals=rng.uniform(-0.1, 0.1, (B, K, S, 3)).astype(np.float32), sem_cls_scores=rng.normal(0, 1, (B, K, Cls)).astype(np.float32),
      objectness_scores=rng.normal(0, 2, (B, K, 2)).astype(np.float32),
      point_clouds=np.concatenate([pts, rng.rand(B, N, 1)], -1).astype(np.float32))


def clear_of_faces(points, box_params, rng, tol=2e-3):
  """Moves (in place) every point of points [N, >= 3] that is closer than tol to a face plane of a box far away from all
  boxes, until none is left: a float32 in / out decision then cannot differ from the float64 one."""
  import votenet_ref as R
  for _ in range(50):
    near = R.points_near_faces(points, box_params, tol)
    if not near.any():
      return
    points[near, :3] = rng.uniform(100.0, 200.0, (int(near.sum()), 3)).astype(points.dtype)
  raise AssertionError("points keep landing on box faces")
