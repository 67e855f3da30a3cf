"""Semantic-segmentation fine-tuning step on the pre-training backbone.

What the reference's downstream/semseg does per iteration (downstream/semseg/lib/train.py:46-232), on libpcmi:
  model      Res16UNet34C with out_channels = number of classes and no feature normalisation
             (downstream/semseg/models/res16unet.py:202-260) -- the SAME backbone kernels; the head's odd width goes
             through csrc/widths.hip
  weights    pre-trained checkpoint loaded by name and shape (downstream/semseg/lib/utils.py:19-43), the head stays random
  loss       nn.CrossEntropyLoss(ignore_index=ignore_label) on model(x).F (train.py:64,124) -> pcmi_softmax_ce_fwd/bwd
  optimiser  SGD(lr, sgd_momentum, dampening, weight_decay) + PolyLR (lib/solvers.py:27-31,50-59,75-76) -> FlatSGD + PolyLR
  metrics    precision_at_one (lib/utils.py:117-128), fast_hist / per_class_iu -> mIoU (:131-138)
  validation test() of lib/test.py:62-196 per batch -- loss, precision@1, confusion matrix, per-class average precision ->
             SegmentationEvaluator (pcmi_seg_eval_rows, pcmi_seg_ap), SegmentationTrainer.validate
  full eval  save_predictions + dataset.test_pointcloud (lib/utils.py:304-344, lib/datasets/scannet.py:131-171): the voxel
             predictions carried onto the ORIGINAL vertices of the scan through the nearest voxel centre, and their mIoU ->
             PointCloudEvaluator (pcmi_voxel_centers, pcmi_nearest_point, pcmi_seg_hist),
             SegmentationTrainer.test_original_pointcloud
  input      Voxelizer.voxelize + sparse_quantize with labels, flip and the chromatic transforms, colour normalisation, label
             map and collation (lib/dataset.py:289-298, lib/voxelizer.py, lib/transforms.py) for a batch of raw scans ->
             SegmentationInputPipeline (pcmi_seg_transform, pcmi_seg_quantize, pcmi_seg_color_augment),
             SegmentationTrainer.train_iter_scenes; every random draw is data (AugmentationDraws)
  limited    the data-efficient setting of Hou et al. (no code in the reference): which `budget` voxels of a scene carry a label
             is decided by k-means on features -> AnnotationSelector (csrc/kmeans.hip), limited_annotation_target,
             SegmentationTrainer.train_iter(annotated=rows)
Dataset classes, the elastic distortion and random dropout, PLY / txt files and colour maps, tensorboard and checkpoint
bookkeeping of the downstream trainer are not provided.
"""
import warnings

import numpy as np
import torch
from torch.optim.lr_scheduler import LambdaLR

from .. import functional as PF
from .. import minkowski as ME
from ..engine import NativeEngine
from ..lib import checkpoint as ck
from ..lib.config import get_config
from ..lib.distributed import FlatParameters
from ..lib.solver import FlatSGD
from ..model import load_model


class PolyLR(LambdaLR):
  """DeepLab learning-rate policy lr * (1 - step / (max_iter + 1)) ** power (downstream/semseg/lib/solvers.py:12-31)."""

  def __init__(self, optimizer, max_iter, power=0.9, last_step=-1):
    super().__init__(optimizer, lambda s: (1 - s / (max_iter + 1)) ** power, last_step)

  @property
  def last_step(self):
    return self.last_epoch


def precision_at_one(pred, target, ignore_label=255):
  """Percentage of correctly labelled points among those whose label is not ignored (lib/utils.py:117-128)."""
  pred, target = pred.reshape(-1), target.reshape(-1)
  keep = target != ignore_label
  if int(keep.sum()) == 0:
    return float("nan")
  return float((pred[keep] == target[keep]).float().mean() * 100.0)


def fast_hist(pred, label, n):
  """n x n confusion matrix of the points with a valid label (lib/utils.py:131-133)."""
  pred, label = np.asarray(pred), np.asarray(label)
  k = (label >= 0) & (label < n)
  return np.bincount(n * label[k].astype(int) + pred[k], minlength=n ** 2).reshape(n, n)


def per_class_iu(hist):
  """Intersection over union per class; mIoU = nanmean (lib/utils.py:136-138)."""
  with np.errstate(divide="ignore", invalid="ignore"):
    return np.diag(hist) / (hist.sum(1) + hist.sum(0) - np.diag(hist))


class SegmentationEvaluator:
  """The accumulators of the reference's validation loop (test() of downstream/semseg/lib/test.py:62-196) on the device.

  step(logits, target) adds one batch: cross-entropy and precision@1 into the two AverageMeters (weighted by the number of
  rows, ignored ones included), fast_hist into the confusion matrix (pcmi_seg_eval_rows), and the per-class average precision
  of the softmax scores into nanmean's sum and count (torch.sort per class + pcmi_seg_ap).  Nothing is read back until
  compute_metrics().  Differences from the reference: arg-max ties go to the lowest class; a class without
  a positive row in a batch scores NaN there whatever scikit-learn is installed; a batch without a counted row adds nothing
  to the loss and score averages; the ranking uses float32 probabilities."""

  def __init__(self, num_labels, ignore_label=255, device=None):
    self.num_labels, self.ignore_label = int(num_labels), int(ignore_label)
    self.device = None if device is None else torch.device(device)  # None: the current device at the first use
    self.reset()

  def reset(self):
    self.hist = self.totals = self.ap_sum = self.ap_cnt = None
    self.batches = 0

  def _state(self):
    if self.hist is None:
      if self.device is None:
        self.device = torch.device("cuda", torch.cuda.current_device())
      c, dev = self.num_labels, self.device
      self.hist = torch.zeros((c, c), dtype=torch.int64, device=dev)
      self.totals = torch.zeros(3, dtype=torch.float64, device=dev)  # sum n loss, sum n score, sum n
      self.ap_sum = torch.zeros(c, dtype=torch.float64, device=dev)
      self.ap_cnt = torch.zeros(c, dtype=torch.int64, device=dev)

  def step(self, logits, target):
    """logits [n, num_labels] on the device, target [n] (a host tensor or array is copied once).  No synchronisation."""
    assert logits.dim() == 2 and logits.shape[1] == self.num_labels, "logits [n, num_labels]"
    if logits.shape[0] == 0:
      return
    self._state()
    tgt = torch.as_tensor(target).reshape(-1).to(device=self.device, dtype=torch.int32)
    out = PF.seg_eval_rows(logits, tgt, self.ignore_label, hist=self.hist, totals=self.totals)
    PF.seg_average_precision(out["prob_t"], tgt, self.ap_sum, self.ap_cnt)
    self.batches += 1

  def compute_metrics(self):
    """One read-back.  loss / score: the AverageMeters' averages; ious, acc, ap_class (per class, in %), their nanmeans mIoU,
    mAcc, mAP, and hist -- the values test() logs and returns."""
    c = self.num_labels
    if self.hist is None:
      flat = np.zeros(3 + 2 * c + c * c)
    else:  # (every count is far below 2^53: float64 carries it exactly)
      flat = torch.cat([self.totals, self.ap_sum, self.ap_cnt.double(), self.hist.reshape(-1).double()]).cpu().numpy()
    totals, ap_sum, ap_cnt = flat[:3], flat[3:3 + c], flat[3 + c:3 + 2 * c]
    hist = np.rint(flat[3 + 2 * c:]).astype(np.int64).reshape(c, c)
    ious = per_class_iu(hist) * 100.0
    with np.errstate(divide="ignore", invalid="ignore"):
      acc = np.diag(hist) / hist.sum(1) * 100.0
      ap_class = ap_sum / ap_cnt * 100.0
    with warnings.catch_warnings():  # a class that never occurred: nanmean of nothing but NaN
      warnings.simplefilter("ignore", category=RuntimeWarning)
      means = dict(mIoU=float(np.nanmean(ious)), mAP=float(np.nanmean(ap_class)), mAcc=float(np.nanmean(acc)))
    n = totals[2]
    return dict(loss=float(totals[0] / n) if n > 0 else 0.0, score=float(totals[1] / n) if n > 0 else 0.0, ious=ious,
                ap_class=ap_class, acc=acc, hist=hist, **means)


class PointCloudEvaluator:
  """mIoU on the ORIGINAL point cloud, on the device: what the reference does between save_predictions (downstream/semseg/
  lib/utils.py:304-344) and dataset.test_pointcloud (lib/datasets/scannet.py:131-171, stanford.py:41-72) through .npy files,
  a scipy KD-tree per room and fast_hist on the host.

  step(coords, pred, transformation, points, point_labels, point_offsets) adds one batch of scenes -- or one PIECE of them:
  a room that was evaluated in pieces (the Stanford rooms) is scored by one call per piece, each with the vertices that belong
  to the piece, or by one call with the pieces' voxels concatenated into one segment.  Nothing is read back until
  compute_metrics().  Differences from the reference: equidistant voxel centres go to the lowest row (the
  KD-tree's choice is arbitrary), a scene without voxels and a vertex with a non-finite coordinate get the prediction -1 and
  are counted in `missing` instead of raising."""

  def __init__(self, num_labels, ignore_label=255, label_map=None, device=None):
    self.num_labels, self.ignore_label = int(num_labels), int(ignore_label)
    self.device = None if device is None else torch.device(device)  # None: the current device at the first use
    # label_map: raw dataset id -> class (a dict, or a sequence indexed by the raw id); ids it does not contain -> ignore_label
    self._lut_host = None
    if label_map is not None:
      if isinstance(label_map, dict):
        lut = np.full(max([int(k) for k in label_map] + [0]) + 1, self.ignore_label, dtype=np.int64)
        for k, v in label_map.items():
          if int(k) >= 0:
            lut[int(k)] = int(v)
      else:
        lut = np.asarray(label_map, dtype=np.int64).reshape(-1)
      self._lut_host = lut
    self._lut = None
    self.reset()

  def reset(self):
    self.hist = self.missing = None
    self.batches = 0

  def _state(self):
    if self.device is None:
      self.device = torch.device("cuda", torch.cuda.current_device())
    if self.hist is None:
      self.hist = torch.zeros((self.num_labels, self.num_labels), dtype=torch.int64, device=self.device)
      self.missing = torch.zeros(1, dtype=torch.int64, device=self.device)
    if self._lut is None and self._lut_host is not None:
      self._lut = torch.from_numpy(self._lut_host).to(self.device)

  def map_labels(self, raw):
    """Raw dataset labels -> classes through label_map (a device gather); ignored rows become -1, which no class equals."""
    lb = torch.as_tensor(np.asarray(raw) if not torch.is_tensor(raw) else raw).reshape(-1).to(self.device).long()
    if self._lut is not None:
      inside = (lb >= 0) & (lb < self._lut.shape[0])
      lb = torch.where(inside, self._lut[lb.clamp(0, self._lut.shape[0] - 1)], torch.full_like(lb, self.ignore_label))
    return torch.where(lb == self.ignore_label, torch.full_like(lb, -1), lb).to(torch.int32)

  def step(self, coords, pred, transformation, points, point_labels, point_offsets):
    """coords int32 [nv, 4] (b, x, y, z) and pred [nv] (the voxels' predicted classes) on the device; transformation [B, 16]:
    the voxelizer matrices as the loader returns them (host); points float64 [n, 3]: the original vertices, scene b at rows
    [point_offsets[b], point_offsets[b + 1]); point_labels [n]: raw dataset labels.  Returns the predicted class per vertex
    (int32 [n] on the device, -1 where there is none) -- what the reference writes to <room>.txt.  No synchronisation."""
    self._state()
    dev = self.device
    T = np.asarray(transformation.cpu() if torch.is_tensor(transformation) else transformation, dtype=np.float64)
    T = T[:, :16] if T.ndim == 2 else T.reshape(-1, 16)
    B = T.shape[0]
    c = torch.as_tensor(coords).to(dev).to(torch.int32)
    # the voxels scene by scene (a stable sort by batch index: rows of a scene keep their order), and the scenes' offsets
    order = torch.sort(c[:, 0], stable=True)[1]
    c, vp = c[order].contiguous(), torch.as_tensor(pred).reshape(-1).to(dev).to(torch.int32)[order]
    ref_offs = torch.searchsorted(c[:, 0].contiguous(), torch.arange(B + 1, dtype=torch.int32, device=dev)).to(torch.int64)
    centers = PF.voxel_centers(c, T)
    # two voxels: the world-space voxel edge is the length of a column of the inverse's linear part (host arithmetic)
    edge = float(max(np.linalg.norm(np.linalg.inv(T.reshape(-1, 4, 4))[:, :3, 0], axis=1).max(), 0.0))
    cell = 2.0 * edge if np.isfinite(edge) and edge > 0 else None
    pts = torch.as_tensor(points)
    assert pts.dtype == torch.float64, "points: float64 [n, 3] (the original vertices, unrounded)"
    idx = PF.nearest_point(centers, ref_offs, pts.to(dev), point_offsets, cell=cell)
    out = PF.seg_hist(vp, idx, self.map_labels(point_labels), self.num_labels, hist=self.hist, missing=self.missing)
    self.batches += 1
    return out["point_pred"]

  def compute_metrics(self):
    """One read-back.  ious and acc per class in %, their nanmeans mIoU and mAcc (scannet.py:169-170), hist, and missing: the
    vertices that received no prediction."""
    c = self.num_labels
    flat = np.zeros(c * c + 1, dtype=np.int64) if self.hist is None else torch.cat([self.hist.reshape(-1), self.missing]).cpu().numpy()
    hist = flat[:c * c].reshape(c, c)
    ious = per_class_iu(hist) * 100.0
    with np.errstate(divide="ignore", invalid="ignore"):
      acc = np.diag(hist) / hist.sum(1) * 100.0
    with warnings.catch_warnings():  # a class that never occurred: nanmean of nothing but NaN
      warnings.simplefilter("ignore", category=RuntimeWarning)
      return dict(ious=ious, mIoU=float(np.nanmean(ious)), acc=acc, mAcc=float(np.nanmean(acc)), hist=hist, missing=int(flat[-1]))


class SegmentationTrainer:
  """One process per GPU; `train_iter(coords, feats, target)` = forward, cross-entropy, backward, SGD + PolyLR step."""

  def __init__(self, num_labels, in_channels=3, model="Res16UNet34C", lr=0.1, momentum=0.9, dampening=0.1,
               weight_decay=1e-4, max_iter=60000, poly_power=0.9, ignore_label=255, bn_momentum=0.02, pretrained=None,
               kernel_order="hybrid", device=None, conv_precision="fp32", input_pipeline=None):
    assert torch.cuda.is_available(), "the fine-tuning step runs on a gfx950 GPU (no CPU path)"
    self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    cfg = get_config(["net.normalize_feature=False", "opt.bn_momentum=%g" % bn_momentum])
    self.model = load_model(model)(in_channels, num_labels, cfg, D=3).to(self.device)
    if pretrained is not None:  # a pre-training checkpoint: everything whose name and shape match (not the head)
      state = torch.load(pretrained, map_location="cpu", weights_only=False) if isinstance(pretrained, str) else pretrained
      weights = ck.convert_kernel_order(self.model, ck.strip_prefixes(state.get("state_dict", state)), kernel_order)
      own = self.model.state_dict()
      own.update(ck.load_state_with_same_shape(self.model, weights))
      self.model.load_state_dict(own)
    self.flat = FlatParameters(self.model.parameters())
    # conv_precision "bf16": the opt-in bf16 matrix-core mode of the convolutions
    self.engine = NativeEngine(self.model, self.flat, in_channels=in_channels, n_passes=1, conv_precision=conv_precision)
    # downstream/semseg/lib/solvers.py:52-60: SGD(lr, momentum=sgd_momentum 0.9, dampening=sgd_dampening 0.1, weight_decay)
    self.optimizer = FlatSGD(self.flat, lr=lr, momentum=momentum, weight_decay=weight_decay, dampening=dampening)
    self.scheduler = PolyLR(self.optimizer, max_iter=max_iter, power=poly_power)
    self.ignore_label, self.num_labels, self.curr_iter = ignore_label, num_labels, 0
    self.input_pipeline = input_pipeline  # a SegmentationInputPipeline, for train_iter_scenes

  def forward(self, coords, feats, training=True):
    st = ME.SparseTensor(feats, coords=coords).to(self.device)
    return self.engine.forward(0, st, training=training)

  def train_iter(self, coords, feats, target, annotated=None):
    """annotated: rows int32 [B, budget] (AnnotationSelector's result; -1 entries are skipped) -- the limited-annotation
    setting: every label but those of these rows becomes ignore_label (limited_annotation_target) where the target lies: on
    the device for a device target; a host target is masked on the host, so the range check below still sees the labels
    that count -- exactly train_iter on the masked target."""
    self.model.train()
    self.optimizer.zero_grad()
    if annotated is not None:
      target = limited_annotation_target(torch.as_tensor(target), annotated, self.ignore_label)
    if torch.is_tensor(target) and not target.is_cuda and target.numel():  # free on the host; as torch's CrossEntropyLoss
      bad = (target != self.ignore_label) & ((target < 0) | (target >= self.num_labels))
      if bool(bad.any()):
        raise IndexError("Target %d is out of bounds (classes 0..%d, ignore label %d)" %
                         (int(target[bad][0]), self.num_labels - 1, self.ignore_label))
    logits = self.forward(coords, feats).requires_grad_(True)
    tgt = target.to(self.device)
    loss = PF.SoftmaxCrossEntropyFunction.apply(logits, tgt, self.ignore_label)
    loss.backward()
    self.engine.backward(0, logits.grad)
    self.optimizer.step()
    self.scheduler.step()
    self.curr_iter += 1
    pred = logits.detach().max(1)[1]
    return {"loss": loss.detach(), "score": precision_at_one(pred, tgt, self.ignore_label), "pred": pred}

  @torch.no_grad()
  def evaluate(self, coords, feats, target):
    """(mIoU in %, per-class IoU, confusion matrix) of one batch in eval mode (running BN estimates)."""
    self.model.eval()
    pred = self.forward(coords, feats, training=False).max(1)[1].cpu().numpy()
    hist = fast_hist(pred, np.asarray(target), self.num_labels)
    ious = per_class_iu(hist) * 100.0
    return float(np.nanmean(ious)), ious, hist

  @torch.no_grad()
  def validate(self, batches):
    """test() of downstream/semseg/lib/test.py:62-196 over an iterable of (coords, feats, target): eval mode, one forward
    and one SegmentationEvaluator.step per batch, one read-back at the end.  Returns the reference's (loss average, score
    average, mAP, mIoU); the evaluator with every other metric stays on self.evaluator."""
    self.model.eval()
    self.evaluator = SegmentationEvaluator(self.num_labels, self.ignore_label, self.device)
    for coords, feats, target in batches:
      self.evaluator.step(self.forward(coords, feats, training=False), target)
    m = self.evaluator.compute_metrics()
    return m["loss"], m["score"], m["mAP"], m["mIoU"]

  @torch.no_grad()
  def test_original_pointcloud(self, batches, label_map=None):
    """The full-resolution evaluation of downstream/semseg/lib/test.py:85-93,122-123,190-192 over an iterable of (coords,
    feats, transformation, points, point_labels): eval mode, one forward per batch, the voxels' arg-max carried onto the
    original vertices by PointCloudEvaluator.step, one read-back at the end.  points / point_labels: one array per scene of the
    batch (a list), or a single array for a batch of one scene.  Returns (mIoU, ious); the evaluator stays on
    self.pointcloud_evaluator and the per-vertex predictions of every batch (device tensors) on self.pointcloud_predictions."""
    self.model.eval()
    self.pointcloud_evaluator = PointCloudEvaluator(self.num_labels, self.ignore_label, label_map, self.device)
    self.pointcloud_predictions = []
    for coords, feats, transformation, points, point_labels in batches:
      if isinstance(points, (list, tuple)):
        sizes = [len(p) for p in points]
        points = torch.cat([torch.as_tensor(p).reshape(-1, 3) for p in points])
        point_labels = torch.cat([torch.as_tensor(np.asarray(l)).reshape(-1) for l in point_labels])
      else:
        sizes = [len(points)]
      offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64)
      pred = self.forward(coords, feats, training=False).max(1)[1]
      self.pointcloud_predictions.append(
          self.pointcloud_evaluator.step(coords, pred, transformation, points, point_labels, offsets))
    m = self.pointcloud_evaluator.compute_metrics()
    return m["mIoU"], m["ious"]

  def train_iter_scenes(self, scenes, draws=None, limit_numpoints=0):
    """One iteration from raw scans: self.input_pipeline (a SegmentationInputPipeline, the constructor's argument) on (scenes,
    draws, limit_numpoints), then train_iter on its device tensors (the coordinates never visit the host).  The result
    carries the batch's `transformation` too."""
    assert self.input_pipeline is not None, "construct the trainer with input_pipeline=SegmentationInputPipeline(aug, device)"
    coords, feats, target, transformation = self.input_pipeline(scenes, draws, limit_numpoints)
    out = self.train_iter(coords, feats, target)
    out["transformation"] = transformation
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Limited annotations (the data-efficient benchmark of Hou et al., "Contrastive Scene Contexts"): a scene gets `budget`
# annotated voxels, chosen by active labelling -- k-means with K = budget on per-voxel features, the voxel nearest to each
# centre (csrc/kmeans.hip, PF.kmeans_select).  The paper's procedure is restated in INTEGRATION.md; the reference has no code.
# ---------------------------------------------------------------------------------------------------------------------
def limited_annotation_target(target, rows, ignore_label=255):
  """target [n] with every label replaced by ignore_label except at rows (any shape; entries < 0 are skipped): what
  SegmentationTrainer.train_iter takes.  Stays on target's device."""
  target = torch.as_tensor(target)
  r = torch.as_tensor(rows).to(device=target.device, dtype=torch.int64).reshape(-1)
  r = r[r >= 0]
  out = torch.full_like(target, ignore_label)
  out[r] = target[r]
  return out


def scene_offsets(coords):
  """int64 [B + 1] (host) from the batch column of coords [n, 4]; the rows of a scene must stand together, scenes ascending."""
  b = torch.as_tensor(coords)[:, 0].cpu().to(torch.int64)
  if b.numel() == 0:
    return torch.zeros(2, dtype=torch.int64)
  assert bool((b[1:] >= b[:-1]).all()) and int(b[0]) >= 0, "the rows of a batch must be grouped by scene, scenes ascending"
  counts = torch.bincount(b, minlength=int(b[-1]) + 1)
  return torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)])


class AnnotationSelector:
  """Chooses the `budget` voxels of every scene of a batch that get a label.  features:
    "net"     k-means on the output of the pre-training network (inference forward, normalised 32-channel features);
              pretrained: its checkpoint (path or state dict), None keeps the random initialisation
    "xyzrgb"  k-means on the voxel coordinates in metres (coords * voxel_size) and the colour columns of feats
    "random"  budget distinct rows per scene, drawn without replacement from the draws
  __call__(coords [n, 4] (b, x, y, z), feats [n, 3], draws=None) -> rows int32 [B, budget] on the host: global rows, -1 where
  the scene has fewer voxels than the budget or a cluster stayed empty.  draws: PF.KMeansDraws [B, budget] (None: sampled).
  `last` keeps kmeans_select's whole result of the last call."""

  def __init__(self, budget, features="net", pretrained=None, model="Res16UNet34C", iters=10, device=None, in_channels=3,
               voxel_size=0.05, kernel_order="hybrid"):
    assert features in ("net", "xyzrgb", "random"), "features: 'net', 'xyzrgb' or 'random'"
    assert 1 <= int(budget) <= PF.KMEANS_MAX_K, "budget: 1 .. %d annotated voxels per scene" % PF.KMEANS_MAX_K
    self.budget, self.features, self.iters, self.voxel_size, self.last = int(budget), features, int(iters), float(voxel_size), None
    if features == "random":
      self.device = None
      return
    assert torch.cuda.is_available(), "the selection runs on a gfx950 GPU (no CPU path)"
    self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if features == "net":
      cfg = get_config(["net.normalize_feature=True"])
      self.model = load_model(model)(in_channels, cfg.net.model_n_out, cfg, D=3).to(self.device)
      if pretrained is not None:
        state = torch.load(pretrained, map_location="cpu", weights_only=False) if isinstance(pretrained, str) else pretrained
        weights = ck.convert_kernel_order(self.model, ck.strip_prefixes(state.get("state_dict", state)), kernel_order)
        own = self.model.state_dict()
        own.update(ck.load_state_with_same_shape(self.model, weights))
        self.model.load_state_dict(own)
      self.model.eval()
      self.flat = FlatParameters(self.model.parameters())
      self.engine = NativeEngine(self.model, self.flat, in_channels=in_channels, n_passes=1)

  @torch.no_grad()
  def point_features(self, coords, feats):
    """float32 [n, C] on the device: what the k-means runs on."""
    if self.features == "net":
      st = ME.SparseTensor(torch.as_tensor(feats).float(), coords=torch.as_tensor(coords)).to(self.device)
      return self.engine.forward(0, st, training=False)
    xyz = torch.as_tensor(coords)[:, 1:4].to(self.device).float() * self.voxel_size
    return torch.cat([xyz, torch.as_tensor(feats).to(self.device).float()], 1)

  def __call__(self, coords, feats, draws=None):
    offs = scene_offsets(coords)
    B = offs.shape[0] - 1
    if draws is None:
      draws = PF.KMeansDraws.sample(B, self.budget)
    elif not isinstance(draws, PF.KMeansDraws):
      draws = PF.KMeansDraws(draws)
    assert tuple(draws.bits.shape) == (B, self.budget), "draws [B, budget]"
    if self.features == "random":
      return random_rows(offs, draws)
    self.last = PF.kmeans_select(self.point_features(coords, feats), offs, self.budget, draws, iters=self.iters)
    return self.last["rows"]


def random_rows(offsets, draws):
  """int32 [B, K] (host): K distinct rows per scene, a partial Fisher-Yates shuffle whose step k takes position
  k + floor((m - k) draw[b, k] / 2^64) of the scene's m rows; -1 from the m-th on."""
  bits = (draws.bits if isinstance(draws, PF.KMeansDraws) else PF.KMeansDraws(draws).bits).cpu().numpy().view(np.uint64)
  offs = np.asarray(offsets, dtype=np.int64)
  B, K = bits.shape
  rows = np.full((B, K), -1, dtype=np.int32)
  for b in range(B):
    lo, m, moved = int(offs[b]), int(offs[b + 1] - offs[b]), {}
    for k in range(min(K, m)):
      j = k + (((m - k) * int(bits[b, k])) >> 64)
      rows[b, k] = lo + moved.get(j, j)
      moved[j] = moved.get(k, k)
  return torch.from_numpy(rows)


# ---------------------------------------------------------------------------------------------------------------------
# The input side on the device (csrc/semseg_input.hip): what dataset.py:289-298 of the reference runs per scan on the host.
# ---------------------------------------------------------------------------------------------------------------------
_SCANNET_VALID = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39)


def make_label_map(num_labels, ignore_labels, ignore_label=255):
  """The lookup table of dataset.py:249-259: raw label -> its rank among the labels that are not ignored; the ignored ones,
  and (in pcmi_seg_color_augment) every label outside the table, -> ignore_label."""
  lut, used = np.full(num_labels, ignore_label, dtype=np.int32), 0
  for l in range(num_labels):
    if l not in ignore_labels:
      lut[l], used = used, used + 1
  return lut


class SegmentationAugmentation:
  """The dataset constants of the reference's VoxelizationDataset subclasses and of config/default.yaml:86-90."""

  def __init__(self, voxel_size=0.05, clip_bound=None, scale_bound=(0.9, 1.1),
               rotation_bound=((-np.pi / 6, np.pi / 6), (-np.pi, np.pi), (-np.pi / 6, np.pi / 6)),
               translation_ratio_bound=((-0.2, 0.2), (-0.05, 0.05), (-0.2, 0.2)), rotation_axis="z", ignore_label=255,
               label_map=None, color_trans_ratio=0.10, color_jitter_std=0.05, normalize_color=True, augment=True,
               elastic_params=None, dropout_ratio=0.2):
    self.voxel_size, self.clip_bound, self.scale_bound = float(voxel_size), clip_bound, scale_bound
    self.rotation_bound, self.translation_ratio_bound = rotation_bound, translation_ratio_bound
    self.rotation_axis, self.ignore_label = rotation_axis, int(ignore_label)
    self.label_map = None if label_map is None else np.asarray(label_map, dtype=np.int32)
    self.color_trans_ratio, self.color_jitter_std = float(color_trans_ratio), float(color_jitter_std)
    self.normalize_color, self.augment = bool(normalize_color), bool(augment)
    # ((granularity, magnitude), ...) of ElasticDistortion in the units of the raw points, or None; RandomDropout's ratio
    self.elastic_params, self.dropout_ratio = elastic_params, float(dropout_ratio)

  def replace(self, **kw):
    new = SegmentationAugmentation.__new__(SegmentationAugmentation)
    new.__dict__.update(self.__dict__)
    new.__dict__.update(kw)
    return new

  @property
  def horizontal_axes(self):
    return [a for a in range(3) if a != "xyz".index(self.rotation_axis.lower())]


_SCANNET = dict(clip_bound=None, rotation_bound=((-np.pi / 64, np.pi / 64), (-np.pi / 64, np.pi / 64), (-np.pi, np.pi)),
                translation_ratio_bound=((-0.2, 0.2), (-0.2, 0.2), (0, 0)), rotation_axis="z",
                label_map=make_label_map(41, set(range(41)) - set(_SCANNET_VALID)),
                elastic_params=((0.2, 0.4), (0.8, 1.6)))  # ELASTIC_DISTORT_PARAMS, scannet.py:76
# lib/datasets/scannet.py:68-78,176 and lib/datasets/stanford.py:98-106 (the training phase: Stanford clips at 4 m)
SCANNET_2CM = SegmentationAugmentation(voxel_size=0.02, **_SCANNET)
SCANNET_5CM = SegmentationAugmentation(voxel_size=0.05, **_SCANNET)
STANFORD_5CM = SegmentationAugmentation(
    voxel_size=0.05, clip_bound=4, rotation_bound=((-np.pi / 32, np.pi / 32), (-np.pi / 32, np.pi / 32), (-np.pi, np.pi)),
    translation_ratio_bound=((-0.2, 0.2), (-0.2, 0.2), (-0.05, 0.05)), rotation_axis="z", label_map=make_label_map(14, {10}))


def axis_rotation(axis, theta):
  """The rotation by theta about coordinate axis `axis`: M(axis, theta) of lib/voxelizer.py:14-15 in closed form."""
  c, s = np.cos(theta), np.sin(theta)
  i, j = (axis + 1) % 3, (axis + 2) % 3
  R = np.eye(3)
  R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
  return R


class AugmentationDraws:
  """Every random quantity of one batch, as data.  Host, per scene: mats [B, 4, 4] (M_r M_v of voxelizer.py:49-79,128-132),
  trans_ratio [B, 3], flip [B] of (fx, fy, fz) or None, contrast [B] of the blend factor or None, translation [B] of (r, g, b)
  in colour units or None, jitter_std [B] of std or None, elastic_on [B] and dropout_on [B] of booleans or None.  Device:
  normals float32 [rows, 3] for the jitter and dropout_keys float32 [rows], both read by VOXEL row (rows >= the number of
  voxels; the number of points always suffices); elastic_noise: per stage of aug.elastic_params one float32 [B, cx, cy, cz, 3]
  block of standard normals (the pipeline smooths a copy, so the draws can be used again)."""

  # the largest |value| a blurred grid of float32 normals can take: the filter's weights sum to at most 1, and a float32 normal
  # drawn from 24 uniform bits stays below sqrt(2 * 24 * ln 2) = 5.77
  NOISE_BOUND = 6.0

  def __init__(self, mats, trans_ratio=None, flip=None, contrast=None, translation=None, jitter_std=None, normals=None,
               elastic_on=None, elastic_noise=None, dropout_on=None, dropout_keys=None):
    self.mats = np.asarray(mats, dtype=np.float64).reshape(-1, 4, 4)
    B = len(self.mats)
    self.trans_ratio = np.zeros((B, 3)) if trans_ratio is None else np.asarray(trans_ratio, dtype=np.float64).reshape(B, 3)
    self.flip, self.contrast, self.translation, self.jitter_std, self.normals = flip, contrast, translation, jitter_std, normals
    self.elastic_on, self.elastic_noise, self.dropout_on, self.dropout_keys = elastic_on, elastic_noise, dropout_on, dropout_keys

  @staticmethod
  def identity(aug, n_scenes):
    """No augmentation: the validation path (M_v alone)."""
    M = np.eye(4)
    np.fill_diagonal(M[:3, :3], 1 / aug.voxel_size)
    return AugmentationDraws(np.repeat(M[None], n_scenes, 0))

  @staticmethod
  def sample(aug, scenes, rng, generator=None, device=None):
    """Draws with the reference's probabilities (transforms.py: flip 0.95 then 0.5 per horizontal axis, auto-contrast 0.2,
    translation 0.95, jitter 0.95, elastic distortion 0.95, dropout aug.dropout_ratio) -- the scalars from rng (numpy.random.RandomState), the normals from `generator` (a
    torch.Generator of `device`).  The streams are not numpy's of the reference; the distributions are.  The capacity of a
    stage's noise blocks comes from the scenes' raw bounding boxes (host arithmetic on the arrays as loaded) widened by what
    the earlier stages can add, NOISE_BOUND * magnitude on either side."""
    B = len(scenes)
    mats, ratio, flip, contrast, translation, jitter, elastic_on, dropout_on = [], [], [], [], [], [], [], []
    for _ in range(B):
      rots = [axis_rotation(a, rng.uniform(*bound) if bound is not None else 0.0) for a, bound in enumerate(aug.rotation_bound)]
      order = rng.permutation(3)  # "use random order" (voxelizer.py:67-69)
      M_r, M_v = np.eye(4), np.eye(4)
      M_r[:3, :3] = rots[order[0]] @ rots[order[1]] @ rots[order[2]]
      np.fill_diagonal(M_v[:3, :3], 1 / aug.voxel_size * rng.uniform(*aug.scale_bound))
      mats.append(M_r @ M_v)
      ratio.append([rng.uniform(*bound) for bound in aug.translation_ratio_bound])
      f = [False] * 3
      if rng.random_sample() < 0.95:
        for a in aug.horizontal_axes:
          f[a] = bool(rng.random_sample() < 0.5)
      flip.append(tuple(f))
      contrast.append(float(rng.random_sample()) if rng.random_sample() < 0.2 else None)
      translation.append((rng.random_sample(3) - 0.5) * 255 * 2 * aug.color_trans_ratio if rng.random_sample() < 0.95 else None)
      jitter.append(aug.color_jitter_std if rng.random_sample() < 0.95 else None)
      elastic_on.append(bool(rng.random_sample() < 0.95))
      dropout_on.append(bool(rng.random_sample() < aug.dropout_ratio))
    rows = sum(len(s[0]) for s in scenes)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    normals = torch.randn((rows, 3), dtype=torch.float32, device=dev, generator=generator)
    keys = torch.rand(rows, dtype=torch.float32, device=dev, generator=generator)
    noise = None
    if aug.elastic_params:
      extent = np.max([np.ptp(np.asarray(s[0], dtype=np.float64).reshape(-1, 3), axis=0) if len(s[0]) else np.zeros(3)
                       for s in scenes], axis=0)
      noise, grown = [], 0.0
      for g, mag in aug.elastic_params:
        cap = [int((e + grown) // g) + 4 for e in extent]  # dims = extent // g + 3, and one more against round-off
        noise.append(torch.randn((B, cap[0], cap[1], cap[2], 3), dtype=torch.float32, device=dev, generator=generator))
        grown += 2 * AugmentationDraws.NOISE_BOUND * mag
    return AugmentationDraws(mats, ratio, flip, contrast, translation, jitter, normals, elastic_on, noise, dropout_on, keys)


class SegmentationInputPipeline:
  """scenes -> (coords, feats, target, transformation) on the device: pcmi_seg_transform, pcmi_seg_quantize, ONE read-back
  (counts, flags), pcmi_seg_color_augment.  Differences from the reference: rows leave in the order of first
  occurrence, scenes in order; colour arithmetic in float64 with one rounding; a channel with hi == lo is not contrasted."""

  def __init__(self, aug, device=None):
    self.aug = aug
    self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    self.last_scene_min = None  # int64 [B, 3]: the voxel minima of the last batch, from its read-back
    self._lut = None if aug.label_map is None else torch.from_numpy(aug.label_map).to(self.device)

  def __call__(self, scenes, draws=None, limit_numpoints=0):
    """scenes: a list of (xyz float64 [n, 3], feats [n, 3] in 0..255, labels [n]).  draws None: AugmentationDraws.identity
    (requires aug.augment False).  Returns coords int32 [M, 4], feats float32 [M, 3], target int32 [M], transformation float64
    [B', 16]; limit_numpoints > 0 keeps the leading scenes whose voxels fit (cfl_collate_fn, transforms.py:251-283)."""
    st = self.stage_upload(scenes, draws)
    self.stage_voxelize(st)
    counts, _ = self.stage_read_back(st)
    pick, nb, total = self.stage_select(st, counts, limit_numpoints)
    return self.stage_colour(st, pick, nb, total)

  # The stages of a call, in order (downstream.insseg.InstanceInputPipeline runs the same ones with its own in between).  Every
  # host-to-device copy of a batch is in stage_upload, its ONE device-to-host copy in stage_read_back; the others only enqueue.
  def stage_upload(self, scenes, draws=None, extra_labels=()):
    """The batch on the device: a dict with B, draws, offs (host) / offs_dev, xyz, feats, labels, flags, mats, trans_ratio,
    elastic_on, params ([B, 12] or None) and, per index k of extra_labels, extra[k] = column k of the scenes as int32 [n]."""
    aug, dev, B = self.aug, self.device, len(scenes)
    assert B >= 1, "at least one scene"
    if draws is None:
      assert not aug.augment, "an augmenting pipeline needs its draws (AugmentationDraws.sample)"
      draws = AugmentationDraws.identity(aug, B)
    assert len(draws.mats) == B, "one set of draws per scene"
    sizes = [len(s[0]) for s in scenes]
    offs = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64)
    for s in scenes:
      assert torch.as_tensor(s[0]).dtype == torch.float64, "xyz: float64 [n, 3]"

    def column(k):
      return torch.cat([torch.as_tensor(np.asarray(s[k])).reshape(-1).to(torch.int32) for s in scenes]).to(dev)
    st = dict(B=B, draws=draws, offs=offs, offs_dev=offs.to(dev),
              xyz=torch.cat([torch.as_tensor(s[0]).reshape(-1, 3) for s in scenes]).to(dev),
              feats=torch.cat([torch.as_tensor(s[1]).reshape(-1, 3).float() for s in scenes]).to(dev), labels=column(2),
              extra={k: column(k) for k in extra_labels}, flags=torch.zeros(B, dtype=torch.int32, device=dev),
              mats=torch.from_numpy(draws.mats.reshape(B, 16)).to(dev),
              trans_ratio=torch.from_numpy(draws.trans_ratio).to(dev) if aug.clip_bound is not None else None,
              elastic_on=None, params=None)
    if draws.elastic_noise is not None and draws.elastic_on is not None:
      st["elastic_on"] = torch.tensor([int(bool(v)) for v in draws.elastic_on], dtype=torch.int32).to(dev)
    if any(x is not None for x in (draws.flip, draws.contrast, draws.translation, draws.jitter_std)):
      st["params"] = torch.from_numpy(PF.seg_color_params(B, draws.flip, draws.contrast, draws.translation, draws.jitter_std)).to(dev)
    return st

  def stage_voxelize(self, st):
    """Elastic distortion, pcmi_seg_transform and pcmi_seg_quantize: st["t"], st["q"]."""
    aug, draws, xyz, flags = self.aug, st["draws"], st["xyz"], st["flags"]
    if draws.elastic_noise is not None:  # the stages chain on the device: each reads the extents the one before left in xyz
      assert aug.elastic_params and len(draws.elastic_noise) == len(aug.elastic_params), "one noise block per elastic stage"
      for (g, mag), noise in zip(aug.elastic_params, draws.elastic_noise):
        noise = noise.clone()  # smoothed in place
        grid = PF.elastic_blur(xyz, st["offs_dev"], g, noise, st["elastic_on"], flags)
        PF.elastic_apply(xyz, st["offs_dev"], g, mag, noise, grid)
    st["t"] = PF.seg_transform(xyz, st["offs_dev"], st["mats"], aug.clip_bound, st["trans_ratio"], flags=flags)
    st["q"] = PF.seg_quantize(st["t"]["vox"], st["offs_dev"], st["labels"], st["t"]["keep"], st["t"]["scene_min"], aug.ignore_label,
                              flags=flags)

  def stage_read_back(self, st, extra=()):
    """The batch's one read-back: counts [B + 1], flags [B], per-scene minima [3 B], then the int64 device tensors of `extra`.
    Raises on a flagged scene.  Returns (the voxels per scene as a list, the host values of `extra` as one array)."""
    B, t = st["B"], st["t"]
    host = torch.cat([st["q"]["counts"], st["flags"].to(torch.int64), t["scene_min"].reshape(-1).to(torch.int64)] +
                     [e.reshape(-1).to(torch.int64) for e in extra]).cpu().numpy()
    msg = PF.seg_flags_message(host[B + 1:2 * B + 1])
    if msg:
      raise ValueError(msg)
    self.last_scene_min = host[2 * B + 1:5 * B + 1].reshape(B, 3)
    return [int(c) for c in host[:B]], host[5 * B + 1:]

  def stage_select(self, st, counts, limit_numpoints=0):
    """RandomDropout and the batch limit on the voxel rows, from the counts on the host.  Returns (pick, nb, total): pick(t) =
    the surviving rows of a row array t, nb the scenes kept, total their rows."""
    aug, dev, B, draws = self.aug, self.device, st["B"], st["draws"]
    counts, kept = list(counts), None
    if draws.dropout_on is not None and any(draws.dropout_on):
      # RandomDropout on the voxel rows (transforms.py:153-158): the int(m (1 - ratio)) rows of the scene with the smallest keys,
      # in row order (a stable sort of the keys, then a sort of the winners); the counts are already on the host
      assert draws.dropout_keys is not None, "dropout needs its keys"
      kept, start = [], 0
      for b in range(B):
        rows = torch.arange(start, start + counts[b], device=dev)
        if draws.dropout_on[b]:
          k = int(counts[b] * (1 - aug.dropout_ratio))
          order = torch.sort(draws.dropout_keys[start:start + counts[b]], stable=True).indices[:k]
          rows = rows[torch.sort(order).values]
        kept.append(rows)
        start += counts[b]
        counts[b] = len(rows)
      kept = torch.cat(kept)
    nb, total = B, 0
    for b in range(B):  # cfl_collate_fn: stop before the scene that would exceed the limit
      if limit_numpoints and total + counts[b] > limit_numpoints:
        nb = b
        break
      total += counts[b]

    def pick(t):
      return (t if kept is None else t[kept].contiguous())[:total]
    return pick, nb, total

  def stage_colour(self, st, pick, nb, total, coords=None, index=None, target=None):
    """pcmi_seg_color_augment on the surviving rows of the quantizer's arrays (or of the ones given) -> the call's result."""
    aug, draws, q = self.aug, st["draws"], st["q"]
    coords = pick(q["coords"] if coords is None else coords)
    index, target = pick(q["index"] if index is None else index), pick(q["labels"] if target is None else target)
    params = None if st["params"] is None else st["params"][:max(nb, 1)]
    normals = None if draws.normals is None else draws.normals[:total]
    out = PF.seg_color_augment(st["feats"], coords, max(nb, 1), index, target, params, normals, aug.normalize_color,
                               self._lut, aug.ignore_label)
    return coords, out, target, st["t"]["aligned"][:nb]
