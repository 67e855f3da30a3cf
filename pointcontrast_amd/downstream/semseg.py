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
Datasets, augmentation, the transfer of predictions onto the original point cloud, tensorboard and checkpoint bookkeeping
of the downstream trainer are outside the hot path and not provided.
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


class SegmentationTrainer:
  """One process per GPU; `train_iter(coords, feats, target)` = forward, cross-entropy, backward, SGD + PolyLR step."""

  def __init__(self, num_labels, in_channels=3, model="Res16UNet34C", lr=0.1, momentum=0.9, dampening=0.1,
               weight_decay=1e-4, max_iter=60000, poly_power=0.9, ignore_label=255, bn_momentum=0.02, pretrained=None,
               kernel_order="hybrid", device=None, conv_precision="fp32"):
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

  def forward(self, coords, feats, training=True):
    st = ME.SparseTensor(feats, coords=coords).to(self.device)
    return self.engine.forward(0, st, training=training)

  def train_iter(self, coords, feats, target):
    self.model.train()
    self.optimizer.zero_grad()
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
