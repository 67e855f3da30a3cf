"""The detection fine-tuning path (downstream/votenet_det_new of the reference) beyond the backbone's ops: the seed sampling,
the loss (models/loss_helper.py over lib/utils/nn_distance.py) and the decoding of the predictions (models/ap_helper.py).

The seed sampling of the detection fine-tuning's sparse backbone: what SparseConvBackbone.forward of the reference
(downstream/votenet_det_new/models/backbone_module.py:159-177) does after the network -- there a Python loop over the
scenes with boolean masks and one furthest_point_sample call each, here one segmented launch over the coordinate manager's
row -> scene tables.  The modules behind it (set abstraction, feature propagation, proposal) take their ops from
pointcontrast_amd.pointnet2_utils."""
import ctypes as C
import math

import numpy as np
import torch
import torch.nn.functional as F

from .. import functional as PF

FAR_THRESHOLD = 0.6
NEAR_THRESHOLD = 0.3
GT_VOTE_FACTOR = 3  # ground-truth votes per point
OBJECTNESS_CLS_WEIGHTS = (0.2, 0.8)
MIN_POINTS_IN_BOX = 5  # remove_empty_box keeps a box holding at least this many points (pcmi_box_point_counts)


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


# ---- the loss -------------------------------------------------------------------------------------------------------
def huber_loss(error, delta=1.0):
  """0.5 q^2 + delta (|x| - q), q = min(|x|, delta), elementwise (nn_distance.py:15-32)."""
  abs_error = torch.abs(error)
  quadratic = torch.clamp(abs_error, max=delta)
  return 0.5 * quadratic ** 2 + delta * (abs_error - quadratic)


def nn_distance(pc1, pc2, l1smooth=False, delta=1.0, l1=False):
  """pc1 [B, N, 3], pc2 [B, M, 3] -> (dist1 float32 [B, N], idx1 int64 [B, N], dist2 float32 [B, M], idx2 int64 [B, M]):
  for every point its distance to, and the index of, the nearest point of the other cloud (nn_distance.py:34-61) -- squared
  L2, L1 with l1, Huber per component with l1smooth (which takes precedence, as there).  One HIP launch per direction and no
  [B, N, M] tensor; differentiable in both clouds.  The lowest index wins a tie."""
  if pc1.dim() != 3 or pc2.dim() != 3 or pc1.shape[0] != pc2.shape[0]:
    raise ValueError("nn_distance: pc1 [B, N, C] and pc2 [B, M, C], got %s and %s" % (tuple(pc1.shape), tuple(pc2.shape)))
  if pc1.shape[2] != 3 or pc2.shape[2] != 3:
    raise ValueError("nn_distance: only C == 3 is supported, got C = %d / %d" % (pc1.shape[2], pc2.shape[2]))
  if pc1.shape[1] == 0 or pc2.shape[1] == 0:
    raise ValueError("nn_distance: empty cloud (N = %d, M = %d)" % (pc1.shape[1], pc2.shape[1]))
  mode = PF.NN_DISTANCE_MODES["huber" if l1smooth else ("l1" if l1 else "l2")]
  return PF.NNDistanceFunction.apply(pc1, pc2, mode, float(delta))


_CONSTANTS = {}


def _constant(key, device, make):
  """A small constant tensor kept on `device` (the reference uploads these with .cuda() on every step)."""
  k = (key, str(device))
  t = _CONSTANTS.get(k)
  if t is None:
    t = _CONSTANTS[k] = make().to(device)
  return t


def _mean_size(config, device):
  arr = np.ascontiguousarray(np.asarray(config.mean_size_arr, dtype=np.float32))
  return _constant(("mean_size", arr.shape, arr.tobytes()), device, lambda: torch.from_numpy(arr.copy()))


def _masked_mean(values, weights):
  return torch.sum(values * weights) / (torch.sum(weights) + 1e-6)


def compute_vote_loss(end_points):
  """loss_helper.py:18-63: every seed inside an object votes for one of its (up to three) ground-truth centres."""
  seed_xyz = end_points["seed_xyz"]
  B, num_seed = seed_xyz.shape[0], seed_xyz.shape[1]
  seed_inds = end_points["seed_inds"].long()
  mask = torch.gather(end_points["vote_label_mask"], 1, seed_inds).float()
  gt_votes = torch.gather(end_points["vote_label"], 1, seed_inds.view(B, num_seed, 1).expand(B, num_seed, 3 * GT_VOTE_FACTOR))
  gt_votes = gt_votes + seed_xyz.repeat(1, 1, GT_VOTE_FACTOR)
  votes = end_points["vote_xyz"].reshape(B * num_seed, -1, 3)
  _, _, dist2, _ = nn_distance(votes, gt_votes.reshape(B * num_seed, GT_VOTE_FACTOR, 3), l1=True)
  votes_dist = torch.min(dist2, dim=1)[0].view(B, num_seed)
  return _masked_mean(votes_dist, mask)


def compute_objectness_loss(end_points):
  """loss_helper.py:65-105 -> (loss, objectness_label int64 [B, K], objectness_mask float [B, K], object_assignment)."""
  gt_center = end_points["center_label"][:, :, 0:3]
  dist1, ind1, _, _ = nn_distance(end_points["aggregated_vote_xyz"], gt_center)
  euclidean = torch.sqrt(dist1.detach() + 1e-6)
  near = euclidean < NEAR_THRESHOLD
  objectness_label = near.long()
  objectness_mask = (near | (euclidean > FAR_THRESHOLD)).float()
  scores = end_points["objectness_scores"]
  weights = _constant("objectness_weights", scores.device, lambda: torch.tensor(OBJECTNESS_CLS_WEIGHTS, dtype=torch.float32))
  loss = F.cross_entropy(scores.transpose(2, 1), objectness_label, weight=weights.to(scores.dtype), reduction="none")
  return _masked_mean(loss, objectness_mask), objectness_label, objectness_mask, ind1


def compute_box_and_sem_cls_loss(end_points, config):
  """loss_helper.py:107-181 -> (center, heading_cls, heading_reg, size_cls, size_reg, sem_cls) losses.  The one-hot products
  of the reference are gathers here (the same values and gradients)."""
  assignment = end_points["object_assignment"]
  gt_center = end_points["center_label"][:, :, 0:3]
  dist1, _, dist2, _ = nn_distance(end_points["center"], gt_center)
  obj = end_points["objectness_label"].float()
  center_loss = _masked_mean(dist1, obj) + _masked_mean(dist2, end_points["box_label_mask"].float())

  def picked(key):
    return torch.gather(end_points[key], 1, assignment)

  heading_class_label = picked("heading_class_label")
  heading_class_loss = _masked_mean(F.cross_entropy(end_points["heading_scores"].transpose(2, 1), heading_class_label, reduction="none"), obj)
  heading_residual_label = picked("heading_residual_label") / (math.pi / config.num_heading_bin)
  heading_pred = torch.gather(end_points["heading_residuals_normalized"], 2, heading_class_label.unsqueeze(-1)).squeeze(-1)
  heading_reg_loss = _masked_mean(huber_loss(heading_pred - heading_residual_label, delta=1.0), obj)

  size_class_label = picked("size_class_label")
  size_class_loss = _masked_mean(F.cross_entropy(end_points["size_scores"].transpose(2, 1), size_class_label, reduction="none"), obj)
  size_residual_label = torch.gather(end_points["size_residual_label"], 1, assignment.unsqueeze(-1).expand(-1, -1, 3))
  size_pred = torch.gather(end_points["size_residuals_normalized"], 2,
                           size_class_label.view(*size_class_label.shape, 1, 1).expand(-1, -1, 1, 3)).squeeze(2)
  mean_size_label = _mean_size(config, size_pred.device)[size_class_label]
  size_reg_loss = _masked_mean(torch.mean(huber_loss(size_pred - size_residual_label / mean_size_label, delta=1.0), -1), obj)

  sem_cls_loss = _masked_mean(F.cross_entropy(end_points["sem_cls_scores"].transpose(2, 1), picked("sem_cls_label"), reduction="none"), obj)
  return center_loss, heading_class_loss, heading_reg_loss, size_class_loss, size_reg_loss, sem_cls_loss


def get_loss(end_points, config):
  """The VoteNet loss (loss_helper.py:183-247): end_points with the reference's keys (seed_xyz, seed_inds, vote_xyz,
  aggregated_vote_xyz, center, objectness_scores, heading_scores, heading_residuals_normalized, size_scores,
  size_residuals_normalized, sem_cls_scores and the labels) -> (loss, end_points) with the nine loss terms, objectness_label /
  objectness_mask, object_assignment, pos_ratio, neg_ratio and obj_acc added.  config: num_heading_bin, num_size_cluster,
  num_class, mean_size_arr.  The three matchings are libpcmi's nn_distance; the cross-entropies and masked means on the
  [B, K, .] tensors are torch ops.  Constants stay on the inputs' device and nothing synchronises with the host."""
  vote_loss = compute_vote_loss(end_points)
  end_points["vote_loss"] = vote_loss
  objectness_loss, objectness_label, objectness_mask, object_assignment = compute_objectness_loss(end_points)
  end_points["objectness_loss"] = objectness_loss
  end_points["objectness_label"] = objectness_label
  end_points["objectness_mask"] = objectness_mask
  end_points["object_assignment"] = object_assignment
  total = float(objectness_label.shape[0] * objectness_label.shape[1])
  end_points["pos_ratio"] = torch.sum(objectness_label.float()) / total
  end_points["neg_ratio"] = torch.sum(objectness_mask) / total - end_points["pos_ratio"]
  center_loss, heading_cls_loss, heading_reg_loss, size_cls_loss, size_reg_loss, sem_cls_loss = \
      compute_box_and_sem_cls_loss(end_points, config)
  end_points["center_loss"] = center_loss
  end_points["heading_cls_loss"] = heading_cls_loss
  end_points["heading_reg_loss"] = heading_reg_loss
  end_points["size_cls_loss"] = size_cls_loss
  end_points["size_reg_loss"] = size_reg_loss
  end_points["sem_cls_loss"] = sem_cls_loss
  box_loss = center_loss + 0.1 * heading_cls_loss + heading_reg_loss + 0.1 * size_cls_loss + size_reg_loss
  end_points["box_loss"] = box_loss
  loss = (vote_loss + 0.5 * objectness_loss + box_loss + 0.1 * sem_cls_loss) * 10
  end_points["loss"] = loss
  obj_pred_val = torch.argmax(end_points["objectness_scores"], 2)
  end_points["obj_acc"] = _masked_mean((obj_pred_val == objectness_label).float(), objectness_mask)
  return loss, end_points


# ---- the predictions --------------------------------------------------------------------------------------------------
def heading_mode(dataset_config):
  """"zero" for a dataset whose class2angle is constantly 0 (ScanNet's axis-aligned boxes), else "bins"."""
  return "zero" if dataset_config.class2angle(1, 0.0) == 0 else "bins"


def nms_mode(config_dict):
  """pcmi_box_nms's mode: 0 = 2D (use_3d_nms off), 1 = 3D, 2 = 3D within a class (cls_nms)."""
  if not config_dict["use_3d_nms"]:
    return 0
  return 2 if config_dict.get("cls_nms", False) else 1


def decode_predictions(end_points, config_dict, heading=None):
  """The device half of parse_predictions: decode, empty-box counts (remove_empty_box) and NMS.  Returns
  functional.box_decode's dict of device tensors; nothing synchronises."""
  dc = config_dict["dataset_config"]
  if heading is None:
    heading = heading_mode(dc)
  if heading not in ("bins", "zero"):
    raise ValueError('heading must be "bins" or "zero", got %r' % (heading,))
  center = end_points["center"]
  PF.require_cuda(center, "parse_predictions")
  return PF.box_decode(center.detach(), end_points["heading_scores"].detach(), end_points["heading_residuals"].detach(),
                       end_points["size_scores"].detach(), end_points["size_residuals"].detach(),
                       end_points["sem_cls_scores"].detach(), end_points["objectness_scores"].detach(),
                       _mean_size(dc, center.device), heading == "zero",
                       with_counts_of=end_points["point_clouds"].detach() if config_dict["remove_empty_box"] else None,
                       nms=(nms_mode(config_dict), config_dict["use_old_type_nms"], config_dict["nms_iou"]), min_points=MIN_POINTS_IN_BOX)


def parse_predictions(end_points, config_dict, heading=None):
  """parse_predictions of the reference (ap_helper.py:40-177): batch_pred_map_cls, a list over the scenes of lists of
  (class, corners [8, 3] in upright-camera coordinates, score); also stored, with pred_mask (numpy [B, K]), in end_points.
  Decoding, the empty-box test and the NMS run on the device (decode_predictions); ONE copy then reads back pred_mask, the
  corners, obj_prob, sem_cls_probs and pred_sem_cls, and the lists are built on the host.  heading: "bins" / "zero", by
  default probed from dataset_config.class2angle.  A scene that keeps no box gives an empty list (the reference asserts)."""
  out = decode_predictions(end_points, config_dict, heading)
  B, K = out["obj_prob"].shape
  Cls = out["sem_cls_probs"].shape[2]
  host = out["packed"].cpu().numpy()
  n = B * K
  o = 0
  corners = host[o:o + n * 24].reshape(B, K, 8, 3).astype(np.float64); o += n * 24
  obj_prob = host[o:o + n].reshape(B, K); o += n
  sem_probs = host[o:o + n * Cls].reshape(B, K, Cls); o += n * Cls
  sem_cls = host[o:o + n].view(np.int32).reshape(B, K); o += n
  pred_mask = host[o:o + n].view(np.int32).reshape(B, K)
  end_points["pred_mask"] = pred_mask.astype(np.float64)
  conf = config_dict["conf_thresh"]
  batch_pred_map_cls = []
  for i in range(B):
    kept = [j for j in range(K) if pred_mask[i, j] == 1 and obj_prob[i, j] > conf]
    if config_dict["per_class_proposal"]:
      cur = [(ii, corners[i, j], sem_probs[i, j, ii] * obj_prob[i, j])
             for ii in range(config_dict["dataset_config"].num_class) for j in kept]
    else:
      cur = [(int(sem_cls[i, j]), corners[i, j], obj_prob[i, j]) for j in kept]
    batch_pred_map_cls.append(cur)
  end_points["batch_pred_map_cls"] = batch_pred_map_cls
  return batch_pred_map_cls


def box_corners(size, heading_angle, center):
  """The 8 corners [8, 3] of a box of size (l, w, h) rotated by heading_angle about the camera's y axis around center, in
  get_3d_box's corner order (box_util.py:210-225); float64 on the host."""
  l, w, h = (float(v) for v in size)
  c, s = math.cos(heading_angle), math.sin(heading_angle)
  x = np.array([1, 1, -1, -1, 1, 1, -1, -1], np.float64) * (l / 2)
  y = np.array([1, 1, 1, 1, -1, -1, -1, -1], np.float64) * (h / 2)
  z = np.array([1, -1, -1, 1, 1, -1, -1, 1], np.float64) * (w / 2)
  return np.stack([c * x + s * z + center[0], y + center[1], -s * x + c * z + center[2]], axis=1)


def parse_groundtruths(end_points, config_dict):
  """parse_groundtruths of the reference (ap_helper.py:179-221): per scene the list of (class, corners [8, 3]) of the
  labelled boxes (box_label_mask == 1); also stored in end_points['batch_gt_map_cls'].  Host-side list building on labels."""
  dc = config_dict["dataset_config"]
  lab = {k: end_points[k].detach().cpu().numpy() for k in ("center_label", "heading_class_label", "heading_residual_label",
                                                          "size_class_label", "size_residual_label", "sem_cls_label",
                                                          "box_label_mask")}
  centers = lab["center_label"][:, :, 0:3]
  cam = np.stack([centers[..., 0], -centers[..., 2], centers[..., 1]], axis=-1)
  batch_gt_map_cls = []
  for i in range(cam.shape[0]):
    cur = []
    for j in range(cam.shape[1]):
      if lab["box_label_mask"][i, j] != 1:
        continue
      angle = dc.class2angle(lab["heading_class_label"][i, j], lab["heading_residual_label"][i, j])
      size = dc.class2size(int(lab["size_class_label"][i, j]), lab["size_residual_label"][i, j])
      cur.append((lab["sem_cls_label"][i, j].item(), box_corners(size, angle, cam[i, j])))
    batch_gt_map_cls.append(cur)
  end_points["batch_gt_map_cls"] = batch_gt_map_cls
  return batch_gt_map_cls
