"""The detection fine-tuning path (downstream/votenet_det_new of the reference) beyond the backbone's ops: the seed sampling,
the loss (models/loss_helper.py over lib/utils/nn_distance.py) and the decoding of the predictions (models/ap_helper.py).

The seed sampling of the detection fine-tuning's sparse backbone: what SparseConvBackbone.forward of the reference
(downstream/votenet_det_new/models/backbone_module.py:159-177) does after the network -- there a Python loop over the
scenes with boolean masks and one furthest_point_sample call each, here one segmented launch over the coordinate manager's
row -> scene tables.  The modules behind it (set abstraction, feature propagation, proposal) take their ops from
pointcontrast_amd.pointnet2_utils.

The network and the training step (models/voting_module.py, proposal_module.py, votenet.py with the sparse backbone, lib/train.py)
are at the end of the file: VotingModule, ProposalModule, VoteNet on row-major activations (csrc/votehead.hip) and
DetectionTrainer."""
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


# ---- the scoring ----------------------------------------------------------------------------------------------------
def ground_truth_boxes(end_points, config_dict, heading=None):
  """The device half of parse_groundtruths: (corners float32 [B, K2, 8, 3] in upright-camera coordinates and get_3d_box's
  corner order, class int64 [B, K2], mask bool [B, K2]) from the label tensors, with decode_predictions' heading modes.  The
  corners are computed in float64, as parse_groundtruths does on the host, and rounded once.  A handful of torch ops on
  [B, K2] tensors; nothing is read back."""
  dc = config_dict["dataset_config"]
  if heading is None:
    heading = heading_mode(dc)
  if heading not in ("bins", "zero"):
    raise ValueError('heading must be "bins" or "zero", got %r' % (heading,))
  center = end_points["center_label"]
  PF.require_cuda(center, "ground_truth_boxes")
  dev = center.device
  c = center[:, :, 0:3].detach().double()
  cx, cy, cz = c[..., 0], -c[..., 2], c[..., 1]
  size_class = end_points["size_class_label"].long()
  size = (_mean_size(dc, dev)[size_class] + end_points["size_residual_label"].detach().float()).double()  # class2size's float32 sum
  if heading == "zero":
    angle = torch.zeros_like(cx)
  else:
    angle = end_points["heading_class_label"].double() * (2 * math.pi / float(dc.num_heading_bin)) + \
        end_points["heading_residual_label"].detach().double()
    angle = torch.where(angle > math.pi, angle - 2 * math.pi, angle)
  sign = _constant("corner_signs", dev, lambda: torch.tensor([[1, 1, -1, -1, 1, 1, -1, -1], [1, 1, 1, 1, -1, -1, -1, -1],
                                                              [1, -1, -1, 1, 1, -1, -1, 1]], dtype=torch.float64))
  x = sign[0] * (size[..., 0:1] / 2)
  y = sign[1] * (size[..., 2:3] / 2)
  z = sign[2] * (size[..., 1:2] / 2)
  co, si = torch.cos(angle)[..., None], torch.sin(angle)[..., None]
  corners = torch.stack([co * x + si * z + cx[..., None], y + cy[..., None], -si * x + co * z + cz[..., None]], dim=-1)
  return corners.float(), end_points["sem_cls_label"].long(), end_points["box_label_mask"] == 1


class APCalculator(object):
  """APCalculator of the reference (models/ap_helper.py:223-276) on the device: the oriented overlaps, the matching and the
  precision / recall curves are libpcmi's (pcmi_det_match, pcmi_det_ap); the confidence ordering is a stable torch.sort.

  step() takes the host lists of parse_predictions / parse_groundtruths, step_decoded() the device tensors of
  decode_predictions and the labels; both run the match at once and keep device records, and only compute_metrics() reads
  anything back.  ap_iou_thresh may be a sequence: compute_metrics() then returns {threshold: dict}, all scored from the one
  match.  Differences from the reference: equal confidences keep accumulation order; overlaps are float32; a class with
  ground truth and no prediction scores AP 0 and recall 0 (eval_det raises KeyError, eval_det_multiprocessing misaligns the
  classes); corners must be in get_3d_box's order."""

  def __init__(self, ap_iou_thresh=0.25, class2type_map=None, device=None):
    self.ap_iou_thresh = ap_iou_thresh
    self.class2type_map = class2type_map
    self.device = None if device is None else torch.device(device)  # None: the current device at the first use
    self.reset()

  def reset(self):
    self._dense = {}    # class id -> dense index, in order of first appearance
    self._records = []  # (score float64 [n], dense class int64 [n], gt id int64 [n], overlap float32 [n])
    self._npos = []     # int64 [dense classes at the time]
    self._n_gt = 0      # ground-truth slots handed out so far
    self.scan_cnt = 0

  def _device(self):
    if self.device is None:
      self.device = torch.device("cuda", torch.cuda.current_device())
    return self.device

  # -- accumulation --
  def _register(self, ids):
    for i in ids:
      if i not in self._dense:
        self._dense[i] = len(self._dense)

  def _append(self, score, cls, best_gt, best_iou, gt_base, gt_cls, gt_mask, n_slots):
    """best_gt / best_iou [n]: the match entry of every detection; gt_base [n]: the first slot of its scene's boxes."""
    gid = torch.where(best_gt >= 0, best_gt.long() + gt_base, torch.full_like(gt_base, -1))
    self._records.append((score, cls, gid, best_iou))
    n_cls = len(self._dense)
    hit = (gt_cls.reshape(-1, 1) == torch.arange(n_cls, device=gt_cls.device)) & gt_mask.reshape(-1, 1)
    self._npos.append(hit.sum(0))
    self._n_gt += n_slots

  def step(self, batch_pred_map_cls, batch_gt_map_cls):
    """Accumulates one batch: lists over the scenes of (class, corners [8, 3], score) and of (class, corners [8, 3]).  One
    upload of the padded arrays, one match.  A scene with more than 1024 detections is matched in rows of 1024."""
    bsize = len(batch_pred_map_cls)
    assert bsize == len(batch_gt_map_cls)
    self.scan_cnt += bsize
    self._register(c for scene in batch_pred_map_cls for c, _, _ in scene)
    self._register(c for scene in batch_gt_map_cls for c, _ in scene)
    if not self._dense:
      return
    G = max(max((len(s) for s in batch_gt_map_cls), default=0), 1)
    KM = PF.DET_MATCH_MAX_K
    rows = []  # (scene, first detection, detections)
    for i, scene in enumerate(batch_pred_map_cls):
      for s in range(0, len(scene), KM):
        rows.append((i, s, min(KM, len(scene) - s)))
    gt_c = np.zeros((bsize, G, 8, 3), np.float32)
    gt_k = np.zeros((bsize, G), np.int64)
    gt_m = np.zeros((bsize, G), bool)
    for i, scene in enumerate(batch_gt_map_cls):
      for j, (c, box) in enumerate(scene):
        gt_c[i, j], gt_k[i, j], gt_m[i, j] = box, self._dense[c], True
    K = max(max((r[2] for r in rows), default=0), 1)
    R = max(len(rows), 1)
    pr_c = np.zeros((R, K, 8, 3), np.float32)
    row_scene = np.zeros(R, np.int64)
    n_det = sum(r[2] for r in rows)
    score, cls, at_row, at_k = np.zeros(n_det, np.float64), np.zeros(n_det, np.int64), np.zeros(n_det, np.int64), np.zeros(n_det, np.int64)
    o = 0
    for r, (i, s, n) in enumerate(rows):
      row_scene[r] = i
      for k in range(n):
        c, box, sc = batch_pred_map_cls[i][s + k]
        pr_c[r, k] = box
        score[o], cls[o], at_row[o], at_k[o] = sc, self._dense[c], r, k
        o += 1
    dev = self._device()
    up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    gt_cls, gt_mask, rs = up(gt_k), up(gt_m), up(row_scene)
    best_gt, best_iou = PF.det_match(up(pr_c), up(gt_c)[rs], gt_cls[rs], gt_mask[rs], len(self._dense))
    cls_d, row_d, k_d = up(cls), up(at_row), up(at_k)
    self._append(up(score), cls_d, best_gt[row_d, k_d, cls_d], best_iou[row_d, k_d, cls_d], self._n_gt + rs[row_d] * G,
                 gt_cls, gt_mask, bsize * G)

  def step_decoded(self, decoded, end_points, config_dict, heading=None):
    """Accumulates one batch from decode_predictions' dict and the label tensors: pred_mask, conf_thresh and
    per_class_proposal are applied on the device (a box that is not kept stays in the record as a detection of no class),
    the match runs at once.  No device-to-host copy and no synchronisation."""
    dc = config_dict["dataset_config"]
    num_class = int(dc.num_class)
    corners, obj_prob = decoded["corners"], decoded["obj_prob"]
    B, K = obj_prob.shape
    dev = obj_prob.device
    self.scan_cnt += B
    self._register(range(num_class))
    ids = tuple(self._dense[c] for c in range(num_class))
    lut = _constant(("dense_classes", ids), dev, lambda: torch.tensor(ids, dtype=torch.int64))
    gt_corners, gt_cls, gt_mask = ground_truth_boxes(end_points, config_dict, heading)
    gt_mask = gt_mask & (gt_cls >= 0) & (gt_cls < num_class)
    gt_cls = lut[gt_cls.clamp(0, num_class - 1)]
    G = gt_cls.shape[1]
    best_gt, best_iou = PF.det_match(corners, gt_corners, gt_cls, gt_mask, len(self._dense))
    keep = obj_prob > config_dict["conf_thresh"]
    if decoded.get("pred_mask") is not None:
      keep = keep & (decoded["pred_mask"] == 1)
    if config_dict["per_class_proposal"]:
      score = (decoded["sem_cls_probs"] * obj_prob.unsqueeze(-1)).double()  # the float32 product, as parse_predictions
      cls = lut.expand(B, K, num_class)
      keep = keep.unsqueeze(-1).expand(B, K, num_class)
      pick = cls
    else:
      score = obj_prob.double()
      cls = lut[decoded["sem_cls"].long()]
      pick = cls.unsqueeze(-1)
    bg = torch.gather(best_gt, 2, pick).reshape(B, K, -1)
    bo = torch.gather(best_iou, 2, pick).reshape(B, K, -1)
    cls = torch.where(keep, cls, torch.full_like(cls, _NO_CLASS)).reshape(B, K, -1)
    bg = torch.where(keep.reshape(B, K, -1), bg, torch.full_like(bg, -1))
    base = (self._n_gt + torch.arange(B, device=dev) * G).reshape(B, 1, 1).expand_as(bg)
    self._append(score.reshape(-1), cls.reshape(-1), bg.reshape(-1), bo.reshape(-1), base.reshape(-1), gt_cls, gt_mask, B * G)

  # -- scoring --
  def evaluate(self, thresholds=None, use_07_metric=False, curves=False):
    """Scores what has been accumulated: a dict with class_ids (the original ids in dense order), and device tensors ap /
    last_rec [T, classes], nd / npos [classes] and, with curves, rec / prec / tp [T, nd] with order (the detection of every
    position, as an index into the accumulation order) and cls_offs.  No synchronisation."""
    if thresholds is None:
      thresholds = self._thresholds()
    n_cls = max(len(self._dense), 1)
    dev = self._device()
    if self._records:
      score, cls, gid, iou = (torch.cat([r[k] for r in self._records]) for k in range(4))
      npos = torch.stack([F.pad(n, (0, n_cls - n.shape[0])) for n in self._npos]).sum(0)
    else:
      score, cls, gid = torch.zeros(0, dtype=torch.float64, device=dev), torch.zeros(0, dtype=torch.int64, device=dev), \
          torch.zeros(0, dtype=torch.int64, device=dev)
      iou, npos = torch.zeros(0, dtype=torch.float32, device=dev), torch.zeros(n_cls, dtype=torch.int64, device=dev)
    # descending confidence, then class: both sorts are stable, so equal confidences keep accumulation order
    by_score = torch.sort(score, descending=True, stable=True)[1]
    cls_sorted, by_cls = torch.sort(cls[by_score], stable=True)
    order = by_score[by_cls]
    offs = torch.searchsorted(cls_sorted, torch.arange(n_cls + 1, device=cls.device))
    out = PF.det_ap(iou[order], gid[order], offs, npos, self._n_gt, list(thresholds), use_07_metric, curves)
    out.update(class_ids=sorted(self._dense, key=self._dense.get), nd=offs[1:] - offs[:-1], npos=npos, order=order, cls_offs=offs)
    return out

  def _thresholds(self):
    t = self.ap_iou_thresh
    return [float(x) for x in t] if isinstance(t, (list, tuple, np.ndarray)) else [float(t)]

  def compute_metrics(self):
    """The reference's dict -- '<name> Average Precision', 'mAP', '<name> Recall', 'AR' over the classes that have a
    detection or a ground-truth box -- or, for a sequence of thresholds, {threshold: dict}.  The one read-back."""
    thr = self._thresholds()
    res = self.evaluate(thr)
    host = torch.cat([res["ap"].reshape(-1), res["last_rec"].reshape(-1), res["nd"].double(), res["npos"].double()]).cpu().numpy()
    n_cls, T = res["npos"].shape[0], len(thr)
    ap, rec = host[:T * n_cls].reshape(T, n_cls), host[T * n_cls:2 * T * n_cls].reshape(T, n_cls)
    nd, npos = host[2 * T * n_cls:2 * T * n_cls + n_cls], host[2 * T * n_cls + n_cls:]
    seen = [(cid, d) for d, cid in enumerate(res["class_ids"]) if nd[d] > 0 or npos[d] > 0]
    seen.sort(key=lambda e: e[0])
    out = {}
    for t in range(T):
      ret = {}
      name = lambda cid: self.class2type_map[cid] if self.class2type_map else str(cid)  # noqa: E731
      for cid, d in seen:
        ret["%s Average Precision" % name(cid)] = ap[t, d]
      ret["mAP"] = np.mean([ap[t, d] for _, d in seen]) if seen else float("nan")
      for cid, d in seen:
        ret["%s Recall" % name(cid)] = rec[t, d]
      ret["AR"] = np.mean([rec[t, d] for _, d in seen]) if seen else float("nan")
      out[thr[t]] = ret
    return out if isinstance(self.ap_iou_thresh, (list, tuple, np.ndarray)) else out[thr[0]]


_NO_CLASS = 1 << 30  # the class of a detection that was not kept: sorted behind every class, scored by none


# ---- the input side: raw scans -> the batch dict, on the device (csrc/detect_input.hip) --------------------------------------------
MAX_NUM_OBJ = PF.DET_MAX_NUM_OBJ
SCANNET_NYU40IDS = (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39)  # model_util_scannet.py:25
DET_ROT_RANGE = {"scannet": np.pi / 18, "sunrgbd": np.pi / 3}  # the full width of the rotation draw: +-5 and +-30 degrees


def rotz(t):
  """pc_util.rotz of the reference: the rotation about z from numpy's cos and sin (the kernels take the matrix as data)."""
  c, s = np.cos(t), np.sin(t)
  return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float64)


class DetectionDraws:
  """Every random quantity of one detection batch, on the host: choices int32 [B, num_points] (the row within the scene),
  flip_x, flip_y bool [B], rot_angle float64 [B], scale float64 [B]; augment False = the reference's augment=False (only
  the choice is applied).  The colour augmentation of SUN RGB-D (use_color): color_gain, color_shift float64 [B, 3],
  color_jitter float64 [B, num_points], color_keep bool [B, num_points] -- per CHOSEN point, where the reference draws per raw
  point before it samples; each None = the identity (1, 0, 0, keep)."""

  def __init__(self, choices, flip_x=None, flip_y=None, rot_angle=None, scale=None, augment=True, color_gain=None, color_shift=None,
               color_jitter=None, color_keep=None):
    self.choices = np.ascontiguousarray(choices, dtype=np.int32)
    B = self.choices.shape[0]
    self.flip_x = np.zeros(B, bool) if flip_x is None else np.asarray(flip_x, dtype=bool)
    self.flip_y = np.zeros(B, bool) if flip_y is None else np.asarray(flip_y, dtype=bool)
    self.rot_angle = np.zeros(B, np.float64) if rot_angle is None else np.asarray(rot_angle, dtype=np.float64)
    self.scale = np.ones(B, np.float64) if scale is None else np.asarray(scale, dtype=np.float64)
    self.augment = bool(augment)
    P = self.choices.shape[1]
    self.color_gain = None if color_gain is None else np.asarray(color_gain, dtype=np.float64).reshape(B, 3)
    self.color_shift = None if color_shift is None else np.asarray(color_shift, dtype=np.float64).reshape(B, 3)
    self.color_jitter = None if color_jitter is None else np.asarray(color_jitter, dtype=np.float64).reshape(B, P)
    self.color_keep = None if color_keep is None else np.asarray(color_keep, dtype=bool).reshape(B, P)

  @staticmethod
  def sample(sizes, num_points, dataset, generator=None, augment=True, color=False):
    """Draws by the reference's distributions (scannet_detection_dataset.py:103-104,115-126, sunrgbd_detection_dataset.py:
    104-112,139,193, pc_util.py:35-43): a choice of num_points rows without replacement where the scan has at least that many,
    with replacement otherwise; flips with probability 1/2 (u > 0.5; no y flip for SUN RGB-D); the angle u w - w / 2 with w =
    pi / 18 (ScanNet) or pi / 3 (SUN RGB-D); the scale u 0.3 + 0.85 for SUN RGB-D only.  generator: a numpy Generator or a
    seed; the same seed gives the same draws.  augment False: identity draws apart from the choice.  color (SUN RGB-D with
    augment; sunrgbd_detection_dataset.py:130-135): gain 1 + 0.4 u - 0.2 and shift 0.1 u - 0.05 per scene and channel, jitter
    0.05 u - 0.025 and keep u > 0.3 per chosen point -- taken from the generator AFTER every draw above, so that a seed gives
    the same choices, flips, angles and scales with and without it."""
    assert dataset in DET_ROT_RANGE, "dataset: 'scannet' or 'sunrgbd'"
    rng = generator if isinstance(generator, np.random.Generator) else np.random.default_rng(generator)
    B, w = len(sizes), DET_ROT_RANGE[dataset]
    choices = np.zeros((B, num_points), np.int32)
    d = DetectionDraws(choices, augment=augment)
    for b, n in enumerate(sizes):
      if n > 0:
        choices[b] = rng.choice(int(n), num_points, replace=int(n) < num_points)
      if not augment:
        continue
      d.flip_x[b] = rng.random() > 0.5
      if dataset == "scannet":
        d.flip_y[b] = rng.random() > 0.5
      d.rot_angle[b] = (rng.random() * w) - w / 2
      if dataset == "sunrgbd":
        d.scale[b] = rng.random() * 0.3 + 0.85
    if color and augment and dataset == "sunrgbd":
      d.color_gain = 1 + 0.4 * rng.random((B, 3)) - 0.2
      d.color_shift = 0.1 * rng.random((B, 3)) - 0.05
      d.color_jitter = 0.05 * rng.random((B, num_points)) - 0.025
      d.color_keep = rng.random((B, num_points)) > 0.3
    return d

  def rot(self):
    """float64 [B, 9]: rotz(rot_angle) per scene."""
    return np.stack([rotz(t).reshape(9) for t in self.rot_angle])

  def flip(self):
    return np.stack([self.flip_x, self.flip_y], 1).astype(np.int32)


def _upload(arrays, device):
  """ONE host -> device copy for a dict of numpy arrays: they are packed, 16-byte aligned, into one byte buffer; returns the
  dict of device tensors, views of the copy."""
  spans, total = {}, 0
  for k, a in arrays.items():
    a = np.ascontiguousarray(a)
    arrays[k] = a
    spans[k] = (total, a.nbytes)
    total += (a.nbytes + 15) // 16 * 16
  host = np.zeros(max(total, 16), np.uint8)
  for k, a in arrays.items():
    o, nb = spans[k]
    host[o:o + nb] = a.reshape(-1).view(np.uint8)
  dev = torch.from_numpy(host).to(device)
  out = {}
  for k, a in arrays.items():
    o, nb = spans[k]
    out[k] = dev[o:o + nb].view(getattr(torch, a.dtype.name)).reshape(a.shape)
  return out


class DetectionInputPipeline:
  """Raw scans -> the batch dict of the reference's detection fine-tuning (VoxelizationDataset over ScannetDetectionDataset or
  SunrgbdDetectionVotesDataset, then collate_fn) as device tensors: ONE upload, pcmi_det_sample_transform /
  pcmi_det_votes_transform, pcmi_det_votes_from_instances, pcmi_det_box_labels, pcmi_det_voxelize, ONE read-back (the flags
  and the voxel counts).  use_height / use_color (the reference's dataset options) widen point_clouds to [B, P, 3 + C] --
  xyz, then rgb, then the height above the floor, feature_dim = C -- with pcmi_segment_quantile over every scan's z and
  pcmi_det_point_features; votes, box labels and voxels are computed from xyz as without them.  Differences from the reference
  (INTEGRATION.md B2): voxel rows leave in the order of first occurrence; the choices are data; a flagged scene raises; the
  colour jitter and dropout are drawn per chosen point."""

  def __init__(self, dataset, num_points, voxel_size, device=None, valid_sem=None, label_to_class=None, mean_size_arr=None,
               num_heading_bin=None, use_height=False, use_color=False):
    assert dataset in PF.DET_MODES, "dataset: 'scannet' or 'sunrgbd'"
    assert mean_size_arr is not None, "mean_size_arr [n_class, 3]: the dataset config's mean sizes"
    self.dataset, self.num_points, self.voxel_size = dataset, int(num_points), float(voxel_size)
    self.use_height, self.use_color = bool(use_height), bool(use_color)
    self.feature_dim = (3 if self.use_color else 0) + (1 if self.use_height else 0)
    self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    self.num_heading_bin = int(num_heading_bin) if num_heading_bin is not None else (1 if dataset == "scannet" else 12)
    ids = SCANNET_NYU40IDS if valid_sem is None else [int(v) for v in valid_sem]
    if label_to_class is None:  # nyu40id2class: the position of the id in nyu40ids
      label_to_class = np.full(max(ids) + 1, -1, np.int32)
      label_to_class[np.asarray(ids)] = np.arange(len(ids))
    const = _upload(dict(valid_sem=np.asarray(ids, dtype=np.int32), label_to_class=np.asarray(label_to_class, dtype=np.int32),
                         mean_size=np.asarray(mean_size_arr, dtype=np.float64).reshape(-1, 3)), self.device)
    self._valid, self._lut, self._mean = const["valid_sem"], const["label_to_class"], const["mean_size"]

  def host_inputs(self, scenes, draws):
    """The numpy arrays that one batch uploads (what tests feed the restatement with)."""
    B, scannet = len(scenes), self.dataset == "scannet"
    sizes = [len(s[0]) for s in scenes]
    width = 6 if self.use_color else 3
    for s in scenes:
      p = np.asarray(s[0])
      assert p.dtype == np.float32 and p.ndim == 2 and p.shape[1] == width, \
          "points: float32 [n, %d], as the arrays on disk are%s" % (width, " (xyz, then rgb: use_color)" if self.use_color else "")
    a = dict(offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
             xyz=np.concatenate([np.asarray(s[0], dtype=np.float32)[:, 0:3] for s in scenes]),
             choices=draws.choices)
    if self.use_color:
      a["rgb"] = np.concatenate([np.asarray(s[0], dtype=np.float32)[:, 3:6] for s in scenes])
      if draws.augment and not scannet:
        for k in ("color_gain", "color_shift", "color_jitter"):
          if getattr(draws, k) is not None:
            a[k] = getattr(draws, k)
        if draws.color_keep is not None:
          a["color_keep"] = draws.color_keep.astype(np.uint8)
    boxes = np.zeros((B, MAX_NUM_OBJ, 8), np.float64)
    n_boxes = np.zeros(B, np.int32)
    for b, s in enumerate(scenes):
      bx = np.asarray(s[3] if scannet else s[1], dtype=np.float64)
      k = bx.shape[0]
      assert k <= MAX_NUM_OBJ, "scene %d: %d boxes, at most %d" % (b, k, MAX_NUM_OBJ)
      n_boxes[b] = k
      if k and scannet:
        boxes[b, :k, 0:6], boxes[b, :k, 7] = bx[:, 0:6], bx[:, -1]
      elif k:
        boxes[b, :k] = bx[:, 0:8]
    a["boxes"], a["n_boxes"] = boxes, n_boxes
    if scannet:
      a["instance"] = np.concatenate([np.asarray(s[1]).reshape(-1) for s in scenes]).astype(np.int32)
      a["semantic"] = np.concatenate([np.asarray(s[2]).reshape(-1) for s in scenes]).astype(np.int32)
    else:
      a["votes"] = np.concatenate([np.asarray(s[2], dtype=np.float64).reshape(-1, 10) for s in scenes])
      h = boxes[:, :, 6].copy()  # the final heading, as pcmi_det_box_labels computes it; its cos and sin are numpy's
      if draws.augment:
        h = np.where(draws.flip_x[:, None], np.pi - h, h) - draws.rot_angle[:, None]
      h = np.where((np.arange(MAX_NUM_OBJ)[None] < n_boxes[:, None]) & np.isfinite(h), h, 0.0)
      a["heading_cs"] = np.stack([np.cos(-1 * h), np.sin(-1 * h)], -1)
    if draws.augment:
      a.update(flip=draws.flip(), rot=draws.rot(), rot_angle=draws.rot_angle, scale=draws.scale)
    return a

  def __call__(self, scenes, draws=None):
    """scenes: a list of raw scans -- ScanNet (vertices float32 [n, 3], instance_labels [n], semantic_labels [n],
    instance_bboxes [k, 7]), SUN RGB-D (points float32 [n, 3], bboxes [k, 8], point_votes float64 [n, 10]); with use_color
    the vertices / points are [n, 6]: xyz, then the raw rgb (0..255 for ScanNet, 0..1 for SUN RGB-D).  draws: a
    DetectionDraws; None draws with DetectionDraws.sample(augment=False) from a fresh generator.  Returns the batch dict as
    device tensors: point_clouds, center_label, heading_class_label, heading_residual_label, size_class_label,
    size_residual_label, sem_cls_label, box_label_mask, vote_label, vote_label_mask, voxel_coords int32 [M, 4], voxel_inds int32
    [M], voxel_feats float32 [M, 3]."""
    B, dev, P = len(scenes), self.device, self.num_points
    assert B >= 1, "at least one scene"
    if draws is None:
      draws = DetectionDraws.sample([len(s[0]) for s in scenes], P, self.dataset, augment=False)
    assert draws.choices.shape == (B, P), "draws: choices [B, num_points]"
    d = _upload(self.host_inputs(scenes, draws), dev)
    aug = dict(augment=draws.augment, flip=d.get("flip"), rot=d.get("rot"), scale=d.get("scale"))
    flags = torch.zeros(B, dtype=torch.int32, device=dev)
    if self.dataset == "scannet":
      s = PF.det_sample_transform(d["xyz"], d["offsets"], d["choices"], instance=d["instance"], semantic=d["semantic"], flags=flags, **aug)
      v = PF.det_votes_from_instances(s["point_clouds"], s["out_instance"], s["out_semantic"], self._valid, flags=flags)
    else:
      s = v = PF.det_votes_transform(d["xyz"], d["votes"], d["offsets"], d["choices"], flags=flags, **aug)
    out = PF.det_box_labels(d["boxes"], d["n_boxes"], self.dataset, self._mean, rot_angle=d.get("rot_angle"), heading_cs=d.get("heading_cs"),
                            label_to_class=self._lut if self.dataset == "scannet" else None, num_heading_bin=self.num_heading_bin,
                            flags=flags, **aug)
    x = PF.det_voxelize(s["point_clouds"], self.voxel_size, flags=flags)
    point_clouds = s["point_clouds"]
    if self.feature_dim:
      floor = PF.segment_quantile(d["xyz"], d["offsets"], 0.99, column=2, flags=flags)["quantile"] if self.use_height else None
      point_clouds, _ = PF.det_point_features(point_clouds, d["xyz"], d["offsets"], d["choices"], self.dataset, rgb=d.get("rgb"),
                                              floor_height=floor, augment=draws.augment, scale=d.get("scale"),
                                              color_gain=d.get("color_gain"), color_shift=d.get("color_shift"),
                                              color_jitter=d.get("color_jitter"), color_keep=d.get("color_keep"), flags=flags)
    host = torch.cat([x["counts"], flags.to(torch.int64)]).cpu().numpy()  # the batch's one read-back
    msg = PF.det_flags_message(host[B + 1:])
    if msg:
      raise ValueError(msg)
    M = int(host[B])
    del out["flags"]
    out.update(point_clouds=point_clouds, vote_label=v["vote_label"], vote_label_mask=v["vote_label_mask"],
               voxel_coords=x["voxel_coords"][:M], voxel_inds=x["voxel_inds"][:M], voxel_feats=x["voxel_feats"][:M])
    return out


# ---- the network: voting, vote aggregation, proposals (csrc/votehead.hip) ----------------------------------------------------
# Every head activation is a row-major fp32 matrix [rows, ld] (rows = B num_seed, B num_seed vote_factor, B num_proposal
# nsample or B num_proposal): feature columns first, geometric columns behind them, zero columns up to a multiple of 32 -- the
# layout the dense GEMM (SparseConvFunction with kmap None) and the fused BatchNorm + ReLU already work on, so nothing is
# ever transposed.  Parameters are stored in the GEMM's layout, [Cin_pad, Cout_pad], transposed, zero-padded and with the
# columns permuted to "features, then xyz"; state_dict() / load_state_dict() speak the reference's names and shapes.
VOTE_AGGREGATION_RADIUS = 0.3
VOTE_AGGREGATION_NSAMPLE = 16
VOTE_AGGREGATION_MLP = (128, 128, 128)


def features_then_xyz(C, blocks=1, block_width=None):
  """Native column of every reference channel of `blocks` groups of (3 geometric + C feature) channels: the reference puts
  xyz first, the rows put the C features first and xyz behind them; block b starts at column b * block_width."""
  width = C + 3 if block_width is None else block_width
  one = torch.cat([torch.arange(C, C + 3), torch.arange(0, C)])
  return torch.cat([one + b * width for b in range(blocks)])


def to_native_weight(ref, in_map, out_map, cin_pad, cout_pad):
  """A reference convolution weight [Cout, Cin, 1(, 1)] in the GEMM's layout [cin_pad, cout_pad]: native[in_map[j],
  out_map[i]] = ref[i, j], zeros elsewhere."""
  ref2 = ref.reshape(ref.shape[0], ref.shape[1])
  out = torch.zeros((cin_pad, cout_pad), dtype=ref.dtype, device=ref.device)
  out[in_map.to(ref.device).unsqueeze(1), out_map.to(ref.device).unsqueeze(0)] = ref2.t()
  return out


def to_reference_weight(native, in_map, out_map, ref_shape):
  native = native.reshape(native.shape[-2], native.shape[-1])
  return native[in_map.to(native.device).unsqueeze(1), out_map.to(native.device).unsqueeze(0)].t().reshape(ref_shape).contiguous()


class RowConv(torch.nn.Module):
  """A 1x1 convolution (the reference's Conv1d / Conv2d with kernel size 1) on rows: y [rows, cout_pad] = x [rows, cin_pad]
  W + b through the dense GEMM.  in_map / out_map: the native column of every reference input / output channel (None:
  the identity).  Padded weights and biases start at zero and receive exactly zero gradient -- their input columns are zero
  and so are the gradients of their output columns -- so they stay zero.  The state dict holds the reference's tensors."""

  def __init__(self, cin, cout, bias=True, in_map=None, out_map=None, cin_pad=None, cout_pad=None, conv_dims=1):
    super().__init__()
    self.cin, self.cout = int(cin), int(cout)
    self.cin_pad = int(cin_pad) if cin_pad is not None else PF.pad_width(cin)
    self.cout_pad = int(cout_pad) if cout_pad is not None else PF.pad_width(cout)
    self.register_buffer("in_map", torch.arange(cin) if in_map is None else in_map.clone(), persistent=False)
    self.register_buffer("out_map", torch.arange(cout) if out_map is None else out_map.clone(), persistent=False)
    self.ref_shape = (self.cout, self.cin) + (1,) * conv_dims
    ref = torch.empty(self.ref_shape)
    torch.nn.init.kaiming_uniform_(ref, a=math.sqrt(5))  # Conv1d / Conv2d's own initialisation
    self.weight = torch.nn.Parameter(to_native_weight(ref, self.in_map, self.out_map, self.cin_pad, self.cout_pad))
    self.bias = None
    if bias:
      bound = 1.0 / math.sqrt(self.cin)
      b = torch.zeros((1, self.cout_pad))
      b[0, self.out_map] = torch.empty(self.cout).uniform_(-bound, bound)
      self.bias = torch.nn.Parameter(b)

  def forward(self, x):
    assert x.dim() == 2 and x.shape[1] == self.cin_pad, "RowConv: expected rows of width %d, got %s" % (self.cin_pad, tuple(x.shape))
    return PF.SparseConvFunction.apply(x, self.weight, self.bias, None, False, x.shape[0])

  def reference_tensors(self):
    out = {"weight": to_reference_weight(self.weight.detach(), self.in_map, self.out_map, self.ref_shape)}
    if self.bias is not None:
      out["bias"] = self.bias.detach()[0, self.out_map].contiguous()
    return out

  def _save_to_state_dict(self, destination, prefix, keep_vars):
    for k, v in self.reference_tensors().items():
      destination[prefix + k] = v

  def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
    for k, param in (("weight", self.weight), ("bias", self.bias)):
      key = prefix + k
      if param is None:
        if key in state_dict and strict:
          unexpected_keys.append(key)
        continue
      if key not in state_dict:
        if strict:
          missing_keys.append(key)
        continue
      v = state_dict[key]
      want = self.ref_shape if k == "weight" else (self.cout,)
      if tuple(v.shape) != tuple(want):
        error_msgs.append("size mismatch for %s: the reference's shape is %s, got %s" % (key, tuple(want), tuple(v.shape)))
        continue
      with torch.no_grad():
        v = v.to(device=param.device, dtype=param.dtype)
        if k == "weight":
          param.copy_(to_native_weight(v, self.in_map, self.out_map, self.cin_pad, self.cout_pad))
        else:
          param.zero_()
          param[0, self.out_map] = v


class RowBatchNorm(torch.nn.BatchNorm1d):
  """BatchNorm1d / BatchNorm2d of the reference over rows [rows, C], fused with the ReLU behind it (pcmi_bn_*).  A
  BatchNorm1d by type, so that whatever sets `.momentum` on the reference's model (BNMomentumScheduler) finds it."""

  def __init__(self, num_features):
    super().__init__(num_features)
    self._untracked = 0
    self.register_state_dict_pre_hook(RowBatchNorm._flush_tracked)

  @staticmethod
  def _flush_tracked(module, prefix, keep_vars):
    if module._untracked:
      with torch.no_grad():
        module.num_batches_tracked += module._untracked
      module._untracked = 0

  def forward(self, x, relu=True):
    if self.training:
      self._untracked += 1
      return PF.BatchNormFunction.apply(x, self.weight, self.bias, self.running_mean, self.running_var, self.momentum, self.eps,
                                        None, relu)
    return PF.batch_norm_eval(x, self.weight, self.bias, self.running_mean, self.running_var, self.eps, None, relu)

  def forward_maxpool(self, x, ns, return_arg=False):
    """BatchNorm + ReLU + the maximum over every ns consecutive rows in one pass (pcmi_bn_maxpool_*): x [R ns, C] -> [R, C],
    the same statistics, running estimates and decision rule as rows_maxpool(forward(x)); the full output is never stored.
    return_arg: also the uint8 rows [R, C] that hold the maxima."""
    if self.training:
      self._untracked += 1
      out, arg = PF.BatchNormMaxPoolFunction.apply(x, self.weight, self.bias, self.running_mean, self.running_var, self.momentum,
                                                   self.eps, ns)
    else:
      out, arg = PF.batch_norm_maxpool_eval(x, self.weight, self.bias, self.running_mean, self.running_var, self.eps, ns, want_arg=True)
    return (out, arg) if return_arg else out


class VotingModule(torch.nn.Module):
  """models/voting_module.py on rows: (seed_xyz [B, S, 3], seed rows [B S, C]) -> (vote_xyz [B S vf, 3], vote rows [B S vf, C]),
  the vote features already L2-normalised (models/votenet.py:120-121; pcmi_vote_fwd does both)."""

  def __init__(self, vote_factor, seed_feature_dim):
    super().__init__()
    self.vote_factor, self.in_dim = int(vote_factor), int(seed_feature_dim)
    C = self.in_dim
    assert C % 32 == 0, "the seed feature width must be a multiple of 32 (the dense GEMM's granularity)"
    self.block_width = PF.pad_width(C + 3)
    self.conv1, self.conv2 = RowConv(C, C), RowConv(C, C)
    self.conv3 = RowConv(C, (3 + C) * self.vote_factor, out_map=features_then_xyz(C, self.vote_factor, self.block_width),
                         cout_pad=self.vote_factor * self.block_width)
    self.bn1, self.bn2 = RowBatchNorm(C), RowBatchNorm(C)

  def forward(self, seed_xyz, seed_rows):
    net = self.bn1(self.conv1(seed_rows))
    net = self.bn2(self.conv2(net))
    net = self.conv3(net)
    return PF.VoteFunction.apply(net, seed_xyz.reshape(-1, 3), seed_rows, self.vote_factor)


class _ConvBN(torch.nn.Module):
  """One layer of the reference's SharedMLP: `conv` (no bias) and `bn.bn`, named as there."""

  def __init__(self, cin, cout, in_map=None):
    super().__init__()
    self.conv = RowConv(cin, cout, bias=False, in_map=in_map, conv_dims=2)
    self.bn = torch.nn.Module()
    self.bn.bn = RowBatchNorm(cout)

  def forward(self, x):
    return self.bn.bn(self.conv(x))


class VoteAggregation(torch.nn.Module):
  """PointnetSAModuleVotes(npoint, radius 0.3, nsample 16, mlp [C, 128, 128, 128], use_xyz, normalize_xyz) on rows: the
  sampled votes' neighbourhoods written straight into rows (pcmi_group_rows_fwd), three GEMM + BatchNorm + ReLU layers, and the
  maximum over nsample (pcmi_rows_maxpool_fwd)."""

  def __init__(self, npoint, seed_feat_dim, radius=VOTE_AGGREGATION_RADIUS, nsample=VOTE_AGGREGATION_NSAMPLE, mlp=VOTE_AGGREGATION_MLP):
    super().__init__()
    self.npoint, self.radius, self.nsample, self.C = int(npoint), float(radius), int(nsample), int(seed_feat_dim)
    self.mlp_module = torch.nn.Module()
    cin = self.C + 3
    for i, cout in enumerate(mlp):
      self.mlp_module.add_module("layer%d" % i, _ConvBN(cin, cout, in_map=features_then_xyz(self.C) if i == 0 else None))
      cin = cout
    self.n_layers = len(mlp)

  def forward(self, xyz, rows, inds):
    """xyz [B, K, 3], rows [B K, C], inds int32 [B, npoint] -> (new_xyz [B, npoint, 3], pooled rows [B npoint, 128], idx)."""
    B, K, _ = xyz.shape
    flat = (inds.to(torch.int64) + torch.arange(B, device=inds.device, dtype=torch.int64).unsqueeze(1) * K).reshape(-1)
    # through the row gather, so that the gradient of the centres flows back into the votes as a deterministic scatter-add
    xyz4 = F.pad(xyz.reshape(B * K, 3), (0, 1))
    new_xyz = PF.GatherRowsFunction.apply(xyz4, flat)[:, :3].reshape(B, self.npoint, 3)
    idx = PF.BallQueryFunction.apply(self.radius, self.nsample, xyz.detach(), new_xyz.detach())
    x = PF.GroupRowsFunction.apply(xyz, new_xyz, rows, idx, self.radius, PF.pad_width(self.C + 3), False)
    for i in range(self.n_layers):
      x = getattr(self.mlp_module, "layer%d" % i)(x)
    return new_xyz, PF.RowsMaxPoolFunction.apply(x, self.nsample), idx


# ---- the PointNet++ backbone on rows (csrc/rowspool.hip beside votehead.hip and pointset.hip) ---------------------------------
POINTNET2_NPOINTS = (2048, 1024, 512, 256)
POINTNET2_RADII = (0.2, 0.4, 0.8, 1.2)
POINTNET2_NSAMPLES = (64, 32, 16, 16)
POINTNET2_SA_MLPS = ((64, 64, 128), (128, 128, 256), (128, 128, 256), (128, 128, 256))  # behind each level's input width
POINTNET2_FP_MLPS = ((256, 256), (256, 256))


def _check_widths(who, widths):
  for w in widths:
    if w % 32:
      raise ValueError("%s: layer width %d is not a multiple of 32 (the dense GEMM's granularity)" % (who, w))


class PointnetSAModuleVotes(torch.nn.Module):
  """PointnetSAModuleVotes(npoint, radius, nsample, mlp, use_xyz=True, normalize_xyz) of the reference on rows: furthest point
  sampling, the ball query, the neighbourhoods written straight into rows (pcmi_group_rows_fwd), the SharedMLP as GEMM +
  BatchNorm + ReLU layers, and the last layer's BatchNorm + ReLU fused with the maximum over nsample (pcmi_bn_maxpool_*).
  mlp = [C, c1, ..., cL] WITHOUT the three coordinate channels, as the reference's argument; c1 .. cL multiples of 32.
  fused_pool=False keeps the composition RowBatchNorm -> RowsMaxPoolFunction (A/B measurements and tests)."""

  def __init__(self, *, mlp, npoint, radius, nsample, use_xyz=True, normalize_xyz=True, fused_pool=True):
    super().__init__()
    if not use_xyz:
      raise NotImplementedError("PointnetSAModuleVotes on rows: use_xyz=False is not provided")
    self.npoint, self.radius, self.nsample, self.C = int(npoint), float(radius), int(nsample), int(mlp[0])
    self.normalize_xyz, self.fused_pool = bool(normalize_xyz), bool(fused_pool)
    _check_widths("PointnetSAModuleVotes", mlp[1:])
    self.mlp_module = torch.nn.Module()
    cin = self.C + 3
    for i, cout in enumerate(mlp[1:]):
      self.mlp_module.add_module("layer%d" % i, _ConvBN(cin, cout, in_map=features_then_xyz(self.C) if i == 0 else None))
      cin = cout
    self.n_layers = len(mlp) - 1
    # the last forward's picks, neighbourhoods and (fused pool) pooling rows, for inspection
    self.last_inds = self.last_idx = self.last_arg = None

  def forward(self, xyz, rows=None, inds=None):
    """xyz [B, N, 3], rows [B N, C] (None with C == 0), inds int [B, npoint] or None -> (new_xyz [B, npoint, 3], pooled rows
    [B npoint, cL], inds int32 [B, npoint])."""
    B = xyz.shape[0]
    if inds is None:
      inds = PF.FurthestPointSampleFunction.apply(xyz.detach(), self.npoint)
    inds = inds.to(device=xyz.device, dtype=torch.int32)
    assert tuple(inds.shape) == (B, self.npoint), "inds: [B, npoint]"
    new_xyz = torch.gather(xyz, 1, inds.to(torch.int64).unsqueeze(-1).expand(B, self.npoint, 3))
    idx = PF.BallQueryFunction.apply(self.radius, self.nsample, xyz.detach(), new_xyz.detach())
    x = PF.GroupRowsFunction.apply(xyz, new_xyz, rows if self.C else None, idx, self.radius if self.normalize_xyz else 1.0,
                                   PF.pad_width(self.C + 3), False)
    for i in range(self.n_layers - 1):
      x = getattr(self.mlp_module, "layer%d" % i)(x)
    last = getattr(self.mlp_module, "layer%d" % (self.n_layers - 1))
    self.last_inds, self.last_idx = inds, idx
    if self.fused_pool:
      pooled, self.last_arg = last.bn.bn.forward_maxpool(last.conv(x), self.nsample, return_arg=True)
    else:
      pooled, self.last_arg = PF.RowsMaxPoolFunction.apply(last(x), self.nsample), None
    return new_xyz, pooled, inds


class PointnetFPModule(torch.nn.Module):
  """PointnetFPModule(mlp) of the reference on rows: the three nearest known points (pcmi_three_nn), the reference's weights
  1 / (dist + 1e-8) normalised over the three, the interpolation and the concatenation with the unknown points' own features
  written into rows in one pass (pcmi_interp_rows_fwd), then the SharedMLP.  mlp = [C2 + C1, c1, ..., cL]."""

  def __init__(self, *, mlp):
    super().__init__()
    _check_widths("PointnetFPModule", mlp[1:])
    self.cin = int(mlp[0])
    self.mlp = torch.nn.Module()
    cin = self.cin
    for i, cout in enumerate(mlp[1:]):
      self.mlp.add_module("layer%d" % i, _ConvBN(cin, cout))
      cin = cout
    self.n_layers = len(mlp) - 1
    self.last_idx = None

  def forward(self, unknown, known, unknown_rows, known_rows):
    """unknown [B, n, 3], known [B, m, 3], unknown_rows [B n, C1] or None, known_rows [B m, C2] -> rows [B n, cL]."""
    dist, idx = PF.ThreeNNFunction.apply(unknown.detach(), known.detach())
    dist_recip = 1.0 / (dist + 1e-8)
    weight = dist_recip / torch.sum(dist_recip, dim=2, keepdim=True)
    C1 = unknown_rows.shape[1] if unknown_rows is not None else 0
    assert known_rows.shape[1] + C1 == self.cin, "PointnetFPModule: %d + %d feature columns, the first layer takes %d" % (
        known_rows.shape[1], C1, self.cin)
    self.last_idx = idx
    x = PF.InterpRowsFunction.apply(known_rows, idx, weight, unknown_rows, PF.pad_width(self.cin), False)
    for i in range(self.n_layers):
      x = getattr(self.mlp, "layer%d" % i)(x)
    return x


class Pointnet2Backbone(torch.nn.Module):
  """models/backbone_module.py Pointnet2Backbone on rows: four set-abstraction levels and two feature propagations; the
  defaults are the reference's numbers.  forward(pointcloud [B, N, 3 + input_feature_dim]) returns the reference's end_points:
  saK_xyz [B, npoint, 3], saK_features [B, C, npoint] (views of the rows), sa1_inds, sa2_inds, fp2_inds (int32), fp2_xyz and
  fp2_features [B, 256, 1024].  Differences from the reference: fp2_inds = sa1_inds taken at sa2_inds --
  the reference's sa1_inds[:, :num_seed] wherever its comment "this fps_inds is just 0, 1, ..., 1023" holds, and the seeds'
  true points where it does not; ties of the sampling and of the pooling go to the lowest index / row."""

  def __init__(self, input_feature_dim=0, npoints=POINTNET2_NPOINTS, radii=POINTNET2_RADII, nsamples=POINTNET2_NSAMPLES,
               sa_mlps=None, fp_mlps=None, fused_pool=True):
    super().__init__()
    F_ = int(input_feature_dim)
    if sa_mlps is None:
      cins = (F_,) + tuple(m[-1] for m in POINTNET2_SA_MLPS[:-1])
      sa_mlps = tuple((c,) + tuple(m) for c, m in zip(cins, POINTNET2_SA_MLPS))
    if fp_mlps is None:
      fp_mlps = ((sa_mlps[3][-1] + sa_mlps[2][-1],) + POINTNET2_FP_MLPS[0], (POINTNET2_FP_MLPS[0][-1] + sa_mlps[1][-1],) + POINTNET2_FP_MLPS[1])
    assert len(sa_mlps) == 4 and len(fp_mlps) == 2 and len(npoints) == 4 and len(radii) == 4 and len(nsamples) == 4
    assert sa_mlps[0][0] == F_, "the first level takes the input's %d feature columns" % F_
    self.input_feature_dim = F_
    for k in range(4):
      self.add_module("sa%d" % (k + 1), PointnetSAModuleVotes(npoint=npoints[k], radius=radii[k], nsample=nsamples[k], mlp=list(sa_mlps[k]),
                                                             use_xyz=True, normalize_xyz=True, fused_pool=fused_pool))
    self.fp1 = PointnetFPModule(mlp=list(fp_mlps[0]))
    self.fp2 = PointnetFPModule(mlp=list(fp_mlps[1]))
    self.num_seed, self.out_dim = int(npoints[1]), int(fp_mlps[1][-1])

  def forward(self, pointcloud, end_points=None):
    if not end_points:
      end_points = {}
    PF.require_cuda(pointcloud, "Pointnet2Backbone")
    assert pointcloud.dim() == 3 and pointcloud.shape[2] == 3 + self.input_feature_dim, \
        "pointcloud: [B, N, 3 + %d], got %s" % (self.input_feature_dim, tuple(pointcloud.shape))
    B, N, W = pointcloud.shape
    pointcloud = pointcloud.float()
    xyz = pointcloud[..., 0:3].contiguous()
    rows = pointcloud.reshape(B * N, W)[:, 3:] if W > 3 else None
    saved = {}
    for k in (1, 2, 3, 4):
      xyz, rows, inds = getattr(self, "sa%d" % k)(xyz, rows)
      saved[k] = (xyz, rows)
      end_points["sa%d_xyz" % k] = xyz
      end_points["sa%d_features" % k] = rows.reshape(B, xyz.shape[1], rows.shape[1]).transpose(1, 2)
      if k <= 2:
        end_points["sa%d_inds" % k] = inds
    rows = self.fp1(saved[3][0], saved[4][0], saved[3][1], saved[4][1])
    rows = self.fp2(saved[2][0], saved[3][0], saved[2][1], rows)
    S = saved[2][0].shape[1]
    end_points["fp2_features"] = rows.reshape(B, S, rows.shape[1]).transpose(1, 2)
    end_points["fp2_xyz"] = saved[2][0]
    end_points["fp2_inds"] = torch.gather(end_points["sa1_inds"], 1, end_points["sa2_inds"].to(torch.int64))
    return end_points


def decode_scores(net, end_points, num_class, num_heading_bin, num_size_cluster, mean_size_arr):
  """decode_scores of models/proposal_module.py:18-44 on net [B, num_proposal, 2 + 3 + 2 NH + 4 NS + num_class] (the
  reference's net_transposed): views of the rows under the reference's keys."""
  B, P = net.shape[0], net.shape[1]
  H, S = num_heading_bin, num_size_cluster
  end_points["objectness_scores"] = net[:, :, 0:2]
  end_points["center"] = end_points["aggregated_vote_xyz"] + net[:, :, 2:5]
  end_points["heading_scores"] = net[:, :, 5:5 + H]
  end_points["heading_residuals_normalized"] = net[:, :, 5 + H:5 + 2 * H]
  end_points["heading_residuals"] = end_points["heading_residuals_normalized"] * (np.pi / H)
  end_points["size_scores"] = net[:, :, 5 + 2 * H:5 + 2 * H + S]
  end_points["size_residuals_normalized"] = net[:, :, 5 + 2 * H + S:5 + 2 * H + 4 * S].reshape(B, P, S, 3)
  arr = np.ascontiguousarray(np.asarray(mean_size_arr, dtype=np.float32))
  msa = _constant(("mean_size", arr.shape, arr.tobytes()), net.device, lambda: torch.from_numpy(arr.copy()))
  end_points["size_residuals"] = end_points["size_residuals_normalized"] * msa.reshape(1, 1, S, 3)
  end_points["sem_cls_scores"] = net[:, :, 5 + 2 * H + 4 * S:]
  return end_points


PROPOSAL_SAMPLINGS = ("vote_fps", "seed_fps", "random")


class ProposalModule(torch.nn.Module):
  """models/proposal_module.py on rows.  sampling: "vote_fps" (furthest point sampling of the votes), "seed_fps" (of the
  seeds; the picks index the votes, as in the reference) or "random" (uniform over the seeds -- or the caller's
  sample_inds: the draw is data)."""

  def __init__(self, num_class, num_heading_bin, num_size_cluster, mean_size_arr, num_proposal, sampling, seed_feat_dim=256):
    super().__init__()
    if sampling not in PROPOSAL_SAMPLINGS:
      raise ValueError("Unknown sampling strategy: %r (one of %s)" % (sampling, ", ".join(PROPOSAL_SAMPLINGS)))
    self.num_class, self.num_heading_bin, self.num_size_cluster = int(num_class), int(num_heading_bin), int(num_size_cluster)
    self.mean_size_arr = np.asarray(mean_size_arr, np.float32)
    assert self.mean_size_arr.shape == (self.num_size_cluster, 3)
    self.num_proposal, self.sampling, self.seed_feat_dim = int(num_proposal), sampling, int(seed_feat_dim)
    self.num_outputs = 2 + 3 + self.num_heading_bin * 2 + self.num_size_cluster * 4 + self.num_class
    self.vote_aggregation = VoteAggregation(self.num_proposal, self.seed_feat_dim)
    self.conv1, self.conv2, self.conv3 = RowConv(128, 128), RowConv(128, 128), RowConv(128, self.num_outputs)
    self.bn1, self.bn2 = RowBatchNorm(128), RowBatchNorm(128)

  def forward(self, xyz, rows, end_points, sample_inds=None, generator=None):
    """xyz [B, K, 3] and rows [B K, C]: the votes.  sample_inds (int [B, num_proposal], optional): the sampled votes."""
    B = xyz.shape[0]
    if sample_inds is None:
      if self.sampling == "vote_fps":
        sample_inds = PF.FurthestPointSampleFunction.apply(xyz.detach(), self.num_proposal)
      elif self.sampling == "seed_fps":
        sample_inds = PF.FurthestPointSampleFunction.apply(end_points["seed_xyz"].detach(), self.num_proposal)
      else:
        num_seed = end_points["seed_xyz"].shape[1]
        sample_inds = torch.randint(0, num_seed, (B, self.num_proposal), dtype=torch.int32, device=xyz.device, generator=generator)
    sample_inds = sample_inds.to(device=xyz.device, dtype=torch.int32)
    assert tuple(sample_inds.shape) == (B, self.num_proposal), "sample_inds: [B, num_proposal]"
    new_xyz, pooled, idx = self.vote_aggregation(xyz, rows, sample_inds)
    end_points["aggregated_vote_xyz"] = new_xyz
    end_points["aggregated_vote_inds"] = sample_inds
    self.last_idx = idx  # the ball query's neighbourhoods of the last forward, for inspection (not one of the reference's keys)
    net = self.bn1(self.conv1(pooled))
    net = self.bn2(self.conv2(net))
    net = self.conv3(net)[:, :self.num_outputs].reshape(B, self.num_proposal, self.num_outputs)
    return decode_scores(net, end_points, self.num_class, self.num_heading_bin, self.num_size_cluster, self.mean_size_arr)


class SparseConvBackbone(torch.nn.Module):
  """models/backbone_module.py:134-180: Res16UNet34C (3 -> output_feature_dim, no feature normalisation) and the seed
  sampling behind it (sample_seeds)."""

  def __init__(self, input_feature_dim=3, output_feature_dim=256, num_seed=1024, model="Res16UNet34C", bn_momentum=0.02):
    super().__init__()
    from ..lib.config import get_config
    from ..model import load_model
    cfg = get_config(["net.normalize_feature=False", "net.conv1_kernel_size=3", "opt.bn_momentum=%g" % bn_momentum])
    self.net = load_model(model)(input_feature_dim, output_feature_dim, cfg, D=3)
    self.num_seed = int(num_seed)


class VoteNet(torch.nn.Module):
  """models/votenet.py.  backbone="sparseconv": forward(inputs) takes the input pipeline's batch dict (point_clouds,
  voxel_coords, voxel_feats, voxel_inds); backbone="pointnet2" (the reference's default, Pointnet2Backbone on rows): it needs
  only point_clouds [B, N, 3 + input_feature_dim], and the backbone's end_points (saK_*, fp2_*) are returned too.  Either way
  the result is end_points with the reference's keys, shapes and dtypes, as [B, K, ...] views of the rows (vote_features and
  seed_features as [B, C, K] views); get_loss and decode_predictions consume it unchanged."""

  def __init__(self, num_class, num_heading_bin, num_size_cluster, mean_size_arr, input_feature_dim=0, num_proposal=128,
               vote_factor=1, sampling="vote_fps", backbone="sparseconv", num_seed=1024, seed_feature_dim=256):
    super().__init__()
    if backbone not in ("sparseconv", "pointnet2"):
      raise NotImplementedError("VoteNet: backbone is 'sparseconv' or 'pointnet2' (backbone=%r)" % (backbone,))
    mean_size_arr = np.asarray(mean_size_arr, np.float32)
    assert mean_size_arr.shape[0] == num_size_cluster
    self.num_class, self.num_heading_bin, self.num_size_cluster, self.mean_size_arr = num_class, num_heading_bin, num_size_cluster, mean_size_arr
    self.input_feature_dim, self.num_proposal, self.vote_factor, self.sampling = input_feature_dim, num_proposal, vote_factor, sampling
    self.backbone = backbone
    if backbone == "pointnet2":
      self.backbone_net = Pointnet2Backbone(input_feature_dim=input_feature_dim)
      if (self.backbone_net.num_seed, self.backbone_net.out_dim) != (num_seed, seed_feature_dim):
        raise ValueError("VoteNet: the pointnet2 backbone gives %d seeds of %d features (num_seed=%r, seed_feature_dim=%r)" % (
            self.backbone_net.num_seed, self.backbone_net.out_dim, num_seed, seed_feature_dim))
    else:
      self.backbone_net = SparseConvBackbone(input_feature_dim + 3, seed_feature_dim, num_seed)
    self.vgen = VotingModule(vote_factor, seed_feature_dim)
    self.pnet = ProposalModule(num_class, num_heading_bin, num_size_cluster, mean_size_arr, num_proposal, sampling,
                               seed_feat_dim=seed_feature_dim)

  def head_parameters(self):
    return list(self.vgen.parameters()) + list(self.pnet.parameters())

  def forward_head(self, seed_xyz, seed_rows, seed_inds=None, sample_inds=None):
    """The head on seed_xyz [B, S, 3] and seed rows [B S, C]: everything behind the backbone."""
    B, S, _ = seed_xyz.shape
    C = seed_rows.shape[1]
    end_points = {"seed_xyz": seed_xyz, "seed_features": seed_rows.reshape(B, S, C).transpose(1, 2)}
    if seed_inds is not None:
      end_points["seed_inds"] = seed_inds
    vote_xyz, vote_rows = self.vgen(seed_xyz, seed_rows)
    K = S * self.vote_factor
    vote_xyz = vote_xyz.reshape(B, K, 3)
    end_points["vote_xyz"] = vote_xyz
    end_points["vote_features"] = vote_rows.reshape(B, K, C).transpose(1, 2)
    return self.pnet(vote_xyz, vote_rows, end_points, sample_inds=sample_inds)

  def forward(self, inputs, sparse_out=None):
    """sparse_out: the backbone's output SparseTensor when something else ran the backbone (DetectionTrainer: the native
    executor); None runs self.backbone_net.net eagerly."""
    points = inputs["point_clouds"]
    dev = self.vgen.conv1.weight.device
    if self.backbone == "pointnet2":
      end_points = self.backbone_net(points.to(dev))
      B, C, S = end_points["fp2_features"].shape
      seed_rows = end_points["fp2_features"].transpose(1, 2).reshape(B * S, C)  # the rows themselves: the view of a view
      end_points.update(self.forward_head(end_points["fp2_xyz"], seed_rows, end_points["fp2_inds"], inputs.get("sample_inds")))
      return end_points
    from .. import minkowski as ME
    if sparse_out is None:
      st = ME.SparseTensor(inputs["voxel_feats"].float(), coords=inputs["voxel_coords"].int()).to(dev)
      sparse_out = self.backbone_net.net(st)
    fp2_xyz, fp2_features, fp2_inds = sample_seeds(sparse_out, points[:, :, 0:3], inputs["voxel_inds"], self.backbone_net.num_seed)
    B, C, S = fp2_features.shape
    seed_rows = fp2_features.transpose(1, 2).reshape(B * S, C)
    return self.forward_head(fp2_xyz, seed_rows, fp2_inds, inputs.get("sample_inds"))


class BNMomentumScheduler:
  """BNMomentumScheduler of the reference (pytorch_utils.py:271-296): step(epoch) sets the momentum bn_lambda(epoch) on
  every BatchNorm of `model` -- the head's RowBatchNorm and the backbone's MinkowskiBatchNorm containers are BatchNorm1d --
  and, through `engine` (a NativeEngine, optional), on the executor's program, which holds its own copy."""

  def __init__(self, model, bn_lambda, last_epoch=-1, engine=None):
    if not isinstance(model, torch.nn.Module):
      raise RuntimeError("Class '%s' is not a PyTorch nn Module" % type(model).__name__)
    self.model, self.lmbd, self.engine = model, bn_lambda, engine
    self.step(last_epoch + 1)
    self.last_epoch = last_epoch

  def step(self, epoch=None):
    if epoch is None:
      epoch = self.last_epoch + 1
    self.last_epoch = epoch
    momentum = float(self.lmbd(epoch))
    for m in self.model.modules():
      if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d, torch.nn.BatchNorm3d)):
        m.momentum = momentum
    if self.engine is not None:
      self.engine.set_bn_momentum(momentum)
    return momentum


def detection_lr(epoch, learning_rate=1e-3, lr_decay_steps=(80, 120, 160), lr_decay_rates=(0.1, 0.1, 0.1)):
  """get_current_lr of lib/train.py:44-50."""
  lr = learning_rate
  for step, rate in zip(lr_decay_steps, lr_decay_rates):
    if epoch >= step:
      lr *= rate
  return lr


def detection_bn_momentum(epoch, init=0.5, decay_rate=0.5, decay_step=20, floor=0.001):
  """bn_lbmd of lib/train.py:184-188."""
  return max(init * decay_rate ** int(epoch / decay_step), floor)


LOSS_TERMS = ("loss", "vote_loss", "objectness_loss", "box_loss", "sem_cls_loss", "center_loss", "heading_cls_loss",
              "heading_reg_loss", "size_cls_loss", "size_reg_loss", "obj_acc", "pos_ratio", "neg_ratio")


class DetectionTrainer:
  """One process, one GPU (the reference's detection fine-tuning is single-GPU): `train_iter(batch)` = forward, get_loss,
  backward, Adam step (lib/train.py train_one_epoch's body).  The backbone (Res16UNet34C, 3 -> 256) runs under
  NativeEngine(n_passes=1), the head eagerly through autograd; one FlatParameters covers both.  start_epoch(epoch) applies
  the epoch's learning rate and BatchNorm momentum.  Mirrors SegmentationTrainer.

  backbone="pointnet2" (the from-scratch VoteNet baseline): no executor -- the whole model goes through autograd, all of its
  parameters lie in the one FlatParameters, FlatAdam and the schedules are the same; the batch needs only point_clouds
  [B, N, 3 + input_feature_dim] beside the labels; state_dict / load_state_dict hold no sparse kernels to convert; pretrained=
  is refused (a pre-training checkpoint holds a sparse backbone)."""

  def __init__(self, dataset_config, num_proposal=256, vote_factor=1, sampling="vote_fps", num_seed=1024, input_feature_dim=0,
               seed_feature_dim=256, lr=1e-3, weight_decay=0.0, lr_decay_steps=(80, 120, 160), lr_decay_rates=(0.1, 0.1, 0.1),
               bn_decay_step=20, bn_decay_rate=0.5, pretrained=None, kernel_order="hybrid", device=None, conv_precision="fp32",
               input_pipeline=None, backbone="sparseconv"):
    from ..lib.distributed import FlatParameters
    from ..lib.solver import FlatAdam
    assert torch.cuda.is_available(), "the fine-tuning step runs on a gfx950 GPU (no CPU path)"
    self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    self.config, self.backbone = dataset_config, backbone
    if backbone == "pointnet2" and pretrained is not None:
      raise ValueError("DetectionTrainer: pretrained= holds a sparse backbone; the pointnet2 backbone trains from scratch "
                       "(load a VoteNet checkpoint with load_state_dict)")
    self.model = VoteNet(dataset_config.num_class, dataset_config.num_heading_bin, dataset_config.num_size_cluster,
                         dataset_config.mean_size_arr, input_feature_dim=input_feature_dim, num_proposal=num_proposal,
                         vote_factor=vote_factor, sampling=sampling, num_seed=num_seed, seed_feature_dim=seed_feature_dim,
                         backbone=backbone).to(self.device)
    self.kernel_order = kernel_order
    if backbone == "pointnet2":
      self.flat, self.engine = FlatParameters(list(self.model.parameters())), None
    else:
      self._init_sparse_backbone(pretrained, kernel_order, input_feature_dim, conv_precision)
    self.optimizer = FlatAdam(self.flat, lr=lr, weight_decay=weight_decay)
    self.base_lr, self.lr_decay_steps, self.lr_decay_rates = lr, tuple(lr_decay_steps), tuple(lr_decay_rates)
    self.bn_scheduler = BNMomentumScheduler(self.model, lambda e: detection_bn_momentum(e, decay_rate=bn_decay_rate, decay_step=bn_decay_step),
                                            engine=self.engine)
    self.input_pipeline = input_pipeline  # a DetectionInputPipeline, for train_iter_scenes
    if backbone == "pointnet2" and input_pipeline is not None and getattr(input_pipeline, "feature_dim", 0) != input_feature_dim:
      raise ValueError("DetectionTrainer: the input pipeline makes %d feature columns (use_height, use_color) and the pointnet2 backbone "
                       "takes input_feature_dim=%d" % (getattr(input_pipeline, "feature_dim", 0), input_feature_dim))
    self.epoch, self.curr_iter = 0, 0
    self.start_epoch(0)

  def _init_sparse_backbone(self, pretrained, kernel_order, input_feature_dim, conv_precision):
    from ..engine import NativeEngine
    from ..lib import checkpoint as ck
    from ..lib.distributed import FlatParameters
    backbone = self.model.backbone_net.net
    if pretrained is not None:  # a pre-training checkpoint: every backbone tensor whose name and shape match
      state = torch.load(pretrained, map_location="cpu", weights_only=False) if isinstance(pretrained, str) else pretrained
      weights = ck.convert_kernel_order(backbone, ck.strip_prefixes(state.get("state_dict", state)), kernel_order)
      own = backbone.state_dict()
      own.update(ck.load_state_with_same_shape(backbone, weights))
      backbone.load_state_dict(own)
    # the backbone's parameters first: the executor's program addresses them by their offsets in the flat buffer
    self.flat = FlatParameters(list(backbone.parameters()) + self.model.head_parameters())
    self.engine = NativeEngine(backbone, self.flat, in_channels=input_feature_dim + 3, n_passes=1, conv_precision=conv_precision)

  def start_epoch(self, epoch):
    """The epoch's learning rate (adjust_learning_rate) and BatchNorm momentum (bnm_scheduler.step) of lib/train.py:56-59."""
    self.epoch = int(epoch)
    lr = detection_lr(epoch, self.base_lr, self.lr_decay_steps, self.lr_decay_rates)
    for g in self.optimizer.param_groups:
      g["lr"] = lr
    return lr, self.bn_scheduler.step(epoch)

  def _to_device(self, batch):
    return {k: (v.to(self.device) if torch.is_tensor(v) else v) for k, v in batch.items()}

  def forward(self, batch, training=True):
    """batch: the input pipeline's dict, on the device.  Returns (end_points with the batch's labels merged in, the
    backbone's output features -- a leaf whose .grad the backward pass hands to the executor; None with the pointnet2
    backbone, which autograd covers)."""
    from .. import minkowski as ME
    if self.engine is None:
      end_points = self.model(batch)
      for k, v in batch.items():
        if k not in end_points:
          end_points[k] = v
      return end_points, None
    st = ME.SparseTensor(batch["voxel_feats"].float(), coords=batch["voxel_coords"].int()).to(self.device)
    feats = self.engine.forward(0, st, training=training)
    if training:
      feats.requires_grad_(True)
    sparse_out = ME.SparseTensor(feats, coords_key=st.coords_key, coords_manager=st.coords_man)
    end_points = self.model(batch, sparse_out=sparse_out)
    for k, v in batch.items():
      if k not in end_points:
        end_points[k] = v
    return end_points, feats

  def train_iter(self, batch):
    """Forward, get_loss, backward through the head and then the executor, Adam step.  Returns the loss terms as device
    tensors; nothing synchronises."""
    self.model.train()
    self.optimizer.zero_grad()
    batch = self._to_device(batch)
    end_points, feats = self.forward(batch, training=True)
    loss, end_points = get_loss(end_points, self.config)
    loss.backward()
    if self.engine is not None:
      self.engine.backward(0, feats.grad)
    self.optimizer.step()
    self.curr_iter += 1
    return {k: end_points[k].detach() for k in LOSS_TERMS if k in end_points}

  def train_iter_scenes(self, scenes, draws=None):
    """One iteration from raw scans through self.input_pipeline (a DetectionInputPipeline, the constructor's argument)."""
    assert self.input_pipeline is not None, "construct the trainer with input_pipeline=DetectionInputPipeline(...)"
    return self.train_iter(self.input_pipeline(scenes, draws))

  @torch.no_grad()
  def evaluate(self, batches, config_dict, ap_iou_thresh=(0.25, 0.5)):
    """evaluate_one_epoch of lib/train.py over an iterable of batch dicts: eval-mode forward (running BatchNorm estimates),
    the loss, decode_predictions and APCalculator.step_decoded per batch -- one match scores every threshold -- and ONE
    read-back, in compute_metrics().  Returns the APCalculator's dict ({threshold: metrics} for a sequence of thresholds);
    the calculator stays on self.ap_calculator, the mean loss terms (device tensors) on self.eval_losses."""
    self.model.eval()
    thresholds = list(ap_iou_thresh) if isinstance(ap_iou_thresh, (list, tuple, np.ndarray)) else ap_iou_thresh
    self.ap_calculator = APCalculator(thresholds, getattr(self.config, "class2type", None), device=self.device)
    sums, n = {}, 0
    for batch in batches:
      batch = self._to_device(batch)
      end_points, _ = self.forward(batch, training=False)
      _, end_points = get_loss(end_points, self.config)
      for k in LOSS_TERMS:
        if k in end_points:
          sums[k] = sums.get(k, 0) + end_points[k].detach()
      n += 1
      self.ap_calculator.step_decoded(decode_predictions(end_points, config_dict), end_points, config_dict)
    self.eval_losses = {k: v / max(n, 1) for k, v in sums.items()}
    return self.ap_calculator.compute_metrics()

  def state_dict(self):
    """The reference's checkpoint form (lib/train.py: epoch, optimizer_state_dict, model_state_dict under the reference's
    names and shapes); the backbone's kernels in the file enumeration given by kernel_order."""
    from ..lib import checkpoint as ck
    sd = self.model.state_dict()
    if self.engine is not None:
      prefix = "backbone_net.net."
      inner = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
      inner = ck.convert_kernel_order(self.model.backbone_net.net, inner, self.kernel_order, inverse=True)
      for k, v in inner.items():
        sd[prefix + k] = v
    return {"epoch": self.epoch, "optimizer_state_dict": self.optimizer.state_dict(), "model_state_dict": sd}

  def load_state_dict(self, state, load_optimizer=True):
    """A checkpoint of state_dict(), or of the reference (its model_state_dict loads; its Adam state does not: the
    parameters differ in layout, so pass load_optimizer=False)."""
    from ..lib import checkpoint as ck
    sd = dict(state.get("model_state_dict", state.get("state_dict", state)))
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
    if self.engine is not None:
      prefix = "backbone_net.net."
      inner = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
      inner = ck.convert_kernel_order(self.model.backbone_net.net, inner, self.kernel_order)
      for k, v in inner.items():
        sd[prefix + k] = v
    self.model.load_state_dict(sd)
    if load_optimizer and "optimizer_state_dict" in state:
      self.optimizer.load_state_dict(state["optimizer_state_dict"])
    if "epoch" in state:
      self.start_epoch(int(state["epoch"]))
