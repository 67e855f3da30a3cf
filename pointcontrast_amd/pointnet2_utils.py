"""Drop-in for the reference's models/backbone/pointnet2/pointnet2_utils.py (downstream/votenet_det_new): the same names,
argument orders, shapes and dtypes, on the HIP kernels of csrc/pointset.hip instead of the reference's CUDA extension.

  from pointcontrast_amd import pointnet2_utils

Differences, both deliberate: furthest_point_sample breaks ties towards the lowest index (the reference's tie order depends
on its block size), and QueryAndGroup refuses sample_uniformly / ret_unique_cnt (the reference's per-region Python loop with
host random numbers, which VoteNet leaves off).  The backward passes use no float atomics: a repeated run is bit-identical.
"""
import torch
import torch.nn as nn

from . import functional as PF

furthest_point_sample = PF.FurthestPointSampleFunction.apply
gather_operation = PF.GatherOperationFunction.apply
three_nn = PF.ThreeNNFunction.apply
three_interpolate = PF.ThreeInterpolateFunction.apply
grouping_operation = PF.GroupingOperationFunction.apply
ball_query = PF.BallQueryFunction.apply


class QueryAndGroup(nn.Module):
  """Groups with a ball query of `radius`: new_features [B, 3 + C, npoint, nsample] (pointnet2_utils.py:294-376)."""

  def __init__(self, radius, nsample, use_xyz=True, ret_grouped_xyz=False, normalize_xyz=False, sample_uniformly=False,
               ret_unique_cnt=False):
    super().__init__()
    if sample_uniformly or ret_unique_cnt:
      raise NotImplementedError("QueryAndGroup: sample_uniformly / ret_unique_cnt (a per-region host loop with host random "
                                "numbers in the reference) are not supported")
    self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz
    self.ret_grouped_xyz, self.normalize_xyz = ret_grouped_xyz, normalize_xyz
    self.sample_uniformly, self.ret_unique_cnt = False, False

  def forward(self, xyz, new_xyz, features=None):
    idx = ball_query(self.radius, self.nsample, xyz, new_xyz)
    xyz_trans = xyz.transpose(1, 2).contiguous()
    grouped_xyz = grouping_operation(xyz_trans, idx)  # (B, 3, npoint, nsample)
    grouped_xyz = grouped_xyz - new_xyz.transpose(1, 2).unsqueeze(-1)
    if self.normalize_xyz:
      grouped_xyz = grouped_xyz / self.radius
    if features is not None:
      grouped_features = grouping_operation(features, idx)
      new_features = torch.cat([grouped_xyz, grouped_features], dim=1) if self.use_xyz else grouped_features
    else:
      assert self.use_xyz, "Cannot have not features and not use xyz as a feature!"
      new_features = grouped_xyz
    return (new_features, grouped_xyz) if self.ret_grouped_xyz else new_features


class GroupAll(nn.Module):
  """Groups all features: [B, 3 + C, 1, N] (pointnet2_utils.py:379-425)."""

  def __init__(self, use_xyz=True, ret_grouped_xyz=False):
    super().__init__()
    self.use_xyz, self.ret_grouped_xyz = use_xyz, ret_grouped_xyz

  def forward(self, xyz, new_xyz, features=None):
    grouped_xyz = xyz.transpose(1, 2).unsqueeze(2)
    if features is not None:
      grouped_features = features.unsqueeze(2)
      new_features = torch.cat([grouped_xyz, grouped_features], dim=1) if self.use_xyz else grouped_features
    else:
      new_features = grouped_xyz
    return (new_features, grouped_xyz) if self.ret_grouped_xyz else new_features
