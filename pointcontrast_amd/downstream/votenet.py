"""The seed sampling of the detection fine-tuning's sparse backbone: what SparseConvBackbone.forward of the reference
(downstream/votenet_det_new/models/backbone_module.py:159-177) does after the network -- there a Python loop over the
scenes with boolean masks and one furthest_point_sample call each, here one segmented launch over the coordinate manager's
row -> scene tables.  The modules behind it (set abstraction, feature propagation, proposal) take their ops from
pointcontrast_amd.pointnet2_utils."""
import ctypes as C

import torch

from .. import functional as PF


def sample_seeds(sparse_out, points, inds, num_seed):
  """sparse_out: the backbone's output SparseTensor (features [N, C], one row per voxel); points [B, num_points, 3]; inds
  [N]: the point of its scene every voxel stands for (the quantisation's return_index).  Returns
  (fp2_xyz [B, num_seed, 3], fp2_features [B, C, num_seed], fp2_inds [B, num_seed] int64): per scene, num_seed furthest
  point samples of its voxels' points, in the scene's row order.  fp2_features is differentiable into sparse_out.F
  (a deterministic scatter-add)."""
  feats, cm = sparse_out.F, sparse_out.coords_man
  PF.require_cuda(feats, "sample_seeds")
  assert points.dim() == 3 and points.shape[2] == 3 and inds.dim() == 1 and inds.shape[0] == feats.shape[0], \
      "sample_seeds: points [B, num_points, 3], inds [N] with one entry per row of the sparse tensor"
  B, num_points, _ = points.shape
  dev = feats.device
  seg = cm.segments(sparse_out.coords_key)
  if seg.n_inst != B:
    raise ValueError("sample_seeds: %d scenes in `points` but %d batch indices with voxels" % (B, seg.n_inst))
  inds = inds.to(device=dev, dtype=torch.int64)
  batch_ids = sparse_out.C[:, 0].to(torch.int64)
  row_xyz = points.to(dev).reshape(-1, 3)[inds + batch_ids * num_points].float().contiguous()  # [N, 3]
  _, rows = PF.furthest_point_sample_segments(row_xyz, C.c_void_p(seg.offs), C.c_void_p(seg.rows), B,
                                              min(int(seg.n), int(num_points)), int(num_seed))
  rows = rows.reshape(-1).to(torch.int64)
  fp2_xyz = row_xyz[rows].reshape(B, num_seed, 3)
  fp2_inds = inds[rows].reshape(B, num_seed)
  fp2_features = PF.GatherRowsFunction.apply(feats, rows).reshape(B, num_seed, -1).transpose(1, 2)
  return fp2_xyz, fp2_features, fp2_inds
