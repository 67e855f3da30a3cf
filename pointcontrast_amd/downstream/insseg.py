"""Instance-segmentation fine-tuning on the pre-training backbone: the third downstream task of Hou et al., "Exploring
Data-Efficient 3D Scene Understanding with Contrastive Scene Contexts", in PointGroup's recipe (Jiang et al., "PointGroup:
Dual-Set Point Grouping for 3D Instance Segmentation").  The reference has no counterpart; the rules are include/pcmi.h's.

  model       the SAME sparse U-Net with num_labels + 3 outputs: a class and a 3-vector offset to the instance centre per voxel
  loss        cross-entropy on logits[:, :C] (pcmi_softmax_ce_*) + PointGroup's two offset losses on logits[:, C:C + 3]
              (pcmi_offset_loss_*) against centroid - voxel in metres (pcmi_instance_centroids: exact integer sums)
  clustering  voxels shifted by their offsets; shifted voxels of one class within `radius` of each other are one instance:
              connected components of a radius graph (pcmi_radius_components, a lock-free union-find over a cell hash grid),
              pcmi_components_compact, pcmi_instance_scores -> cluster_instances
  metrics     mask AP at IoU 0.25, 0.5 and 0.5:0.95:0.05 (pcmi_instance_overlap, pcmi_instance_match, pcmi_det_ap)
              -> InstanceEvaluator

  proposals   PointGroup's dual set: BOTH coordinate sets clustered (the voxels where they are, and shifted), the union reduced by
              non-maximum suppression on mask IoU (pcmi_proposal_overlap, pcmi_proposal_nms) -> cluster_proposals: overlapping
              masks as a membership matrix member [n, S], which both evaluators take; the trainer's dual_set=True

Stated differences from PointGroup: no cap on the neighbours of a row (theirs: 50, which makes the result
depend on the row order), <= radius where they have <, and no ScoreNet (an instance's score is the mean softmax probability of
its rows for their class, and the non-maximum suppression ranks by it); cluster_instances alone (dual_set=False, the default)
is moreover ONE clustering on the shifted coordinates with disjoint masks.  nms_iou, min_score and max_per_scene are untuned.
The AP is VOC-style -- each prediction is matched to its best ground truth, the rule of APCalculator -- and NOT ScanNet's
benchmark script, which has void-overlap and minimum-region rules.

  benchmark   those rules -- minimum region size, void and small-region overlap, the script's claim rule and its integration
              of the curve -- on the voxels or on the original vertices (pcmi_instance_void_overlap,
              pcmi_instance_bench_match, pcmi_instance_bench_ap) -> InstanceBenchmarkEvaluator.  Restated from the script's
              rules, never run against the script (INTEGRATION.md lists the differences).
  input       raw scans (xyz, colours, labels, per-scene instance ids) -> a batch with instance indices that are unique across
              its scenes: SegmentationInputPipeline's stages, the voxel's instance id by a second pcmi_seg_quantize, an optional
              per-scene crop (pcmi_seg_crop_ladder: this project's own rule, untuned), pcmi_instance_relabel
              -> InstanceInputPipeline, train_iter_scenes, validate_scenes
"""
import warnings

import numpy as np
import torch

from .. import functional as PF
from .semseg import SegmentationInputPipeline, SegmentationTrainer, precision_at_one

# 0.25, then 0.50, 0.55, ... 0.95
AP_THRESHOLDS = (0.25,) + tuple((10 + k) / 20.0 for k in range(10))
# the benchmark script's own doubles: np.arange(0.5, 0.95, 0.05) (nine values, several a few bits away from k / 20), then 0.25
BENCHMARK_THRESHOLDS = tuple(float(t) for t in np.append(np.arange(0.5, 0.95, 0.05), 0.25))


def scene_offsets_of(coords):
  """int64 [B + 1] on coords' device: the row offsets of the scenes of coords [n, 4] (batch index first, rows scene-major as
  the collate functions leave them).  B comes from the last row: free for a host tensor, one read-back for a device one."""
  b = coords[:, 0].contiguous()
  B = int(b[-1]) + 1 if b.numel() else 1
  return torch.searchsorted(b, torch.arange(B + 1, dtype=b.dtype, device=b.device)).to(torch.int64)


def cluster_instances(coords, offsets, logits, scene_offsets, voxel_size, radius=0.03, min_points=50, stuff_classes=(0, 1),
                      max_instances=4096, shifted=True):
  """Instances from a network's output, on the device without a read-back.  coords int32 [n, 4] (b, x, y, z; rows scene-major),
  offsets float32 [n, 3] (predicted offsets in metres; may be a column slice), logits float32 [n, C] (may be a column slice),
  scene_offsets [B + 1].  The semantic arg-max (the lowest class of equal logits) is the row's group, -1 for stuff_classes;
  xyz = coords[:, 1:4] voxel_size (+ offsets if shifted) in float32; then radius_components -> components_compact (at least
  min_points rows, numbered by lowest row) -> instance_scores of the row's softmax probability of its own class.
  radius 0.03, min_points 50 and the two stuff classes (ScanNet's wall and floor) are PointGroup's numbers, untuned here.
  Returns device tensors: instance int32 [n] (-1: in none), count int32 [1] (the true number, also beyond max_instances),
  inst_class, inst_size, inst_scene int32 [max_instances] (-1 / 0 from the count on), inst_score float64 [max_instances], and
  scene_offsets int64 [B + 1] as given."""
  PF.require_cuda(logits, "cluster_instances")
  xyz, offs, group, score = _semantic_rows(coords, logits, scene_offsets, voxel_size, stuff_classes)
  if shifted:
    xyz = xyz + offsets.to(device=logits.device, dtype=torch.float32)
  label = PF.radius_components(xyz, offs, group, radius)
  out = PF.components_compact(label, offs, group, min_points, max_instances)
  return dict(instance=out["instance"], count=out["count"], inst_class=out["group"], inst_size=out["size"], inst_scene=out["scene"],
              inst_score=PF.instance_scores(score, out["instance"], out["size"]), scene_offsets=offs)


def _semantic_rows(coords, logits, scene_offsets, voxel_size, stuff_classes):
  """The semantic pass both clusterings share -> (xyz float32 [n, 3] unshifted, scene_offsets int64 [B + 1] on the device,
  group int32 [n]: the arg-max class, -1 for stuff_classes; score float32 [n]: the row's softmax probability of that class)."""
  dev = logits.device
  n = logits.shape[0]
  c = coords.to(device=dev, dtype=torch.int32)
  offs = torch.as_tensor(scene_offsets).to(device=dev, dtype=torch.int64).contiguous()
  rows = PF.seg_eval_rows(logits, torch.full((n,), -1, dtype=torch.int32, device=dev), -1)
  pred = rows["pred"]
  score = rows["prob_t"].gather(0, pred.long().reshape(1, n)).reshape(n) if n else torch.zeros(0, dtype=torch.float32, device=dev)
  group = pred
  for s in stuff_classes:
    group = torch.where(pred == int(s), torch.full_like(pred, -1), group)
  return c[:, 1:4].to(torch.float32) * float(voxel_size), offs, group, score


PROPOSAL_SETS = ("unshifted", "shifted")  # PointGroup's P and Q


def cluster_proposals(coords, offsets, logits, scene_offsets, voxel_size, radius=0.03, min_points=50, stuff_classes=(0, 1),
                      max_instances=4096, sets=PROPOSAL_SETS, nms_iou=0.3, min_score=0.0, max_per_scene=1024):
  """PointGroup's dual-set grouping: OVERLAPPING proposals from a network's output, on the device without a read-back.  The
  arguments of cluster_instances; sets: 1 to 4 of "unshifted" (the voxels where they are: PointGroup's set P, which keeps
  objects whose offsets are poor) and "shifted" (where their offsets send them: set Q, which separates objects that touch).
  The semantic pass runs once; per set radius_components -> components_compact -> instance_scores as in cluster_instances; then
  pcmi_proposal_overlap and pcmi_proposal_nms over the union (per scene, descending score, a kept proposal clears every later
  one with mask IoU > nms_iou; classes are not looked at).  With M = max_instances and S = len(sets), set s owns the proposal
  slots [s M, (s + 1) M) of every per-proposal array [P = S M]; the sets are never packed together.
  nms_iou 0.3 is PointGroup's number, untuned here; min_score 0 because PointGroup's 0.09 belongs to ScoreNet's scores, not
  to a mean softmax probability; max_per_scene (<= 1024) bounds the proposals of ONE scene over all sets: the first in slot
  order stay, the rest are counted in `dropped` and never kept.  All three are untuned.
  Returns cluster_instances' keys --
    instance int32 [n]        the kept proposal of the highest rank (score, then lowest slot) among the row's columns, -1: none
    count int32 [S]           components_compact's count per set (the true number, also beyond max_instances)
    inst_class int32 [P]      -1 for an unused AND for a suppressed slot (what the evaluators skip)
    inst_size int32 [P]       the size BEFORE suppression;  inst_scene int32 [P], inst_score float64 [P], scene_offsets
  -- plus member int32 [n, S] (the row's proposal per set, -1 none or suppressed), keep int32 [P] (pcmi_proposal_nms's) and
  dropped int64 [1]."""
  PF.require_cuda(logits, "cluster_proposals")
  sets = tuple(sets)
  assert 1 <= len(sets) <= PF.PROPOSAL_MAX_SETS and all(s in PROPOSAL_SETS for s in sets), \
      "cluster_proposals: sets: 1 to %d of %s" % (PF.PROPOSAL_MAX_SETS, PROPOSAL_SETS)
  dev, M = logits.device, int(max_instances)
  xyz, offs, group, score = _semantic_rows(coords, logits, scene_offsets, voxel_size, stuff_classes)
  moved = xyz + offsets.to(device=dev, dtype=torch.float32) if "shifted" in sets else None
  parts = []
  for s, name in enumerate(sets):
    label = PF.radius_components(moved if name == "shifted" else xyz, offs, group, radius)
    out = PF.components_compact(label, offs, group, min_points, M)
    out["score"] = PF.instance_scores(score, out["instance"], out["size"])
    out["member"] = torch.where(out["instance"] >= 0, out["instance"] + s * M, out["instance"])
    parts.append(out)
  cat = lambda k: torch.cat([p[k] for p in parts])  # noqa: E731
  member = torch.stack([p["member"] for p in parts], 1)
  cls, scene, inst_score = cat("group"), cat("scene"), cat("score")
  dropped = torch.zeros(1, dtype=torch.int64, device=dev)
  ov = PF.proposal_overlap(member, scene, offs.shape[0] - 1, max_per_scene, dropped)
  keep = PF.proposal_nms(ov, scene, cls, inst_score, nms_iou, min_score)
  kept = keep > 0
  if member.numel():
    member = torch.where((member >= 0) & kept[member.clamp(min=0).long()], member, torch.full_like(member, -1))
  best, best_score = member[:, 0], inst_score[member[:, 0].clamp(min=0).long()] if member.numel() else inst_score[:0]
  for s in range(1, len(sets)):  # a later column has the higher slots: it wins only with a strictly higher score
    m = member[:, s]
    sc = inst_score[m.clamp(min=0).long()]
    take = (m >= 0) & ((best < 0) | (sc > best_score))
    best, best_score = torch.where(take, m, best), torch.where(take, sc, best_score)
  return dict(instance=best.contiguous(), count=cat("count"), inst_class=torch.where(kept, cls, torch.full_like(cls, -1)), inst_size=cat("size"),
              inst_scene=scene, inst_score=inst_score, scene_offsets=offs, member=member, keep=keep, dropped=dropped)


class InstanceInputPipeline(SegmentationInputPipeline):
  """scenes of (xyz, colours, labels, instance_ids) -> (coords, feats, target, instance, n_instances, transformation) on the
  device, with ONE read-back per batch: the parent's stages, and between its quantizer and its read-back

    the voxel's raw instance id   the common id of all its points, else -1: a second pcmi_seg_quantize with the ids as labels
                                  and -1 as the ignore label (the same voxels in the same order)
    the crop, if any              crop = (sides, max_voxels): pcmi_seg_crop_ladder on the two horizontal axes; every row array
                                  is gathered by its rows.  THIS PROJECT'S OWN RULE, in the spirit of PointGroup's crop, not a
                                  restatement of it; the ladder and max_voxels are untuned.  Coordinates are not shifted again,
                                  so `transformation` stays valid.  A scene that no step brings within max_voxels raises.
    pcmi_instance_relabel         over the voxels whose target after aug.label_map is neither the ignore label nor one of
                                  stuff_classes: those are in no instance

  Dropout and limit_numpoints only remove rows afterwards: the ids stay unique and ordered, some may be left without rows
  (legal for the loss and both evaluators).  n_instances counts the instances of the scenes that survive limit_numpoints.
  dropout_keys and normals of the draws are read by voxel row AFTER the crop.  Without crop, and with the same draws, coords,
  feats, target and transformation are SegmentationInputPipeline's bit for bit.  last_crop_step: step int64 [B] of the last
  batch (-1: the scene was not cropped), from its read-back."""

  def __init__(self, aug, device=None, stuff_classes=(0, 1), crop=None):
    super().__init__(aug, device)
    self.stuff_classes = tuple(int(s) for s in stuff_classes)
    self.crop = None if crop is None else (np.asarray(crop[0], dtype=np.int64).reshape(-1, 2), int(crop[1]))
    self.last_crop_step = None

  @staticmethod
  def sample_crop_draws(crop, n_scenes, rng):
    """uint32-valued int64 [B, S, 2] from rng (numpy.random.RandomState): one draw per scene, step and axis."""
    return rng.randint(0, 2**32, size=(int(n_scenes), len(np.asarray(crop[0]).reshape(-1, 2)), 2), dtype=np.int64)

  def __call__(self, scenes, draws=None, limit_numpoints=0, crop_draws=None):
    st = self.stage_upload(scenes, draws, crop_draws=crop_draws)
    self.stage_voxelize(st)
    self.stage_instances(st)
    counts, tail = self.stage_read_back(st, st["read"])
    return self.stage_finish(st, counts, tail, limit_numpoints)

  def stage_upload(self, scenes, draws=None, extra_labels=(3,), crop_draws=None):
    st = super().stage_upload(scenes, draws, extra_labels)
    st["crop_draws"] = None
    if self.crop is not None:
      assert crop_draws is not None, "a cropping pipeline needs its draws (InstanceInputPipeline.sample_crop_draws)"
      st["crop_draws"] = torch.as_tensor(np.asarray(crop_draws, dtype=np.int64)).reshape(st["B"], len(self.crop[0]), 2).to(self.device)
    return st

  def stage_instances(self, st):
    """The voxel's raw id, the crop, the relabelling: st["rows"] (coords, index, target), st["instance"], st["read"]."""
    aug, dev, B, t, q = self.aug, self.device, st["B"], st["t"], st["q"]
    raw = PF.seg_quantize(t["vox"], st["offs_dev"], st["extra"][3], t["keep"], t["scene_min"], -1, flags=st["flags"])["labels"]
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    voffs = torch.cat([zero, q["counts"][:B].cumsum(0)])
    coords, index, target, read = q["coords"], q["index"], q["labels"], []
    if self.crop is not None:
      cr = PF.seg_crop_ladder(coords, voffs, [1 + a for a in aug.horizontal_axes], self.crop[0], st["crop_draws"], self.crop[1], st["flags"])
      rows = cr["rows"]
      coords, index, target, raw = coords[rows].contiguous(), index[rows].contiguous(), target[rows].contiguous(), raw[rows].contiguous()
      voffs = torch.cat([zero, cr["counts"][:B].cumsum(0)])
      read += [cr["counts"], cr["step"]]
    mapped = target
    if self._lut is not None:  # pcmi_seg_color_augment's rule, which the target itself meets after the read-back
      L = self._lut.shape[0]
      mapped = torch.where((target >= 0) & (target < L), self._lut[target.clamp(0, L - 1).long()], torch.full_like(target, aug.ignore_label))
    keep = mapped != aug.ignore_label
    for s in self.stuff_classes:
      keep = keep & (mapped != s)
    rl = PF.instance_relabel(raw, voffs, keep)
    st["rows"], st["instance"], st["read"] = (coords, index, target), rl["instance"], read + [rl["counts"]]

  def stage_finish(self, st, counts, tail, limit_numpoints=0):
    """Dropout, the batch limit and the colour stage from the read-back -> the call's result."""
    B = st["B"]
    if self.crop is not None:
      counts, self.last_crop_step, tail = [int(c) for c in tail[:B]], tail[B + 1:2 * B + 1].copy(), tail[2 * B + 1:]
    else:
      self.last_crop_step = None
    pick, nb, total = self.stage_select(st, counts, limit_numpoints)
    coords, feats, target, transformation = self.stage_colour(st, pick, nb, total, *st["rows"])
    return coords, feats, target, pick(st["instance"]), int(tail[:nb].sum()), transformation


def batch_instance_ids(per_scene_raw_ids, device=None):
  """The point_instance numbering benchmark_original_pointcloud asks its caller for, from the raw per-scene instance ids of a
  batch's vertices (a list of integer arrays; < 0: no instance): PF.instance_relabel over the concatenated vertices, so the
  indices are unique across the scenes and ordered by first occurrence.  Returns (one int32 array per scene on the host, the
  number of instances); one read-back."""
  dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
  sizes = [len(r) for r in per_scene_raw_ids]
  offs = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64)
  raw = torch.cat([torch.as_tensor(np.asarray(r)).reshape(-1).to(torch.int32) for r in per_scene_raw_ids]).to(dev)
  out = PF.instance_relabel(raw, offs.to(dev))
  host = torch.cat([out["instance"].to(torch.int64), out["counts"][-1:]]).cpu().numpy()
  inst = host[:-1].astype(np.int32)
  return [inst[int(offs[b]):int(offs[b + 1])] for b in range(len(sizes))], int(host[-1])


class InstanceSegmentationTrainer(SegmentationTrainer):
  """SegmentationTrainer with a head of num_labels + 3 outputs.  train_iter(coords, feats, target, instance) = forward,
  cross-entropy + the two offset losses, ONE backward, SGD + PolyLR step; predict(coords, feats) = cluster_instances of the
  inference forward -- with dual_set=True cluster_proposals (PointGroup's dual set: overlapping masks after mask NMS at nms_iou,
  0.3 being PointGroup's number, untuned here), which validate_scenes and benchmark_original_pointcloud then score.  An inference forward returns the num_labels class columns, so evaluate / validate /
  test_original_pointcloud of the parent score the semantic head unchanged.  A pre-training checkpoint loads as in the parent:
  by name and shape, so the head stays random.  **Nobody has trained a network with this head to a benchmark number yet.**"""

  def __init__(self, num_labels, voxel_size=0.02, radius=0.03, min_points=50, stuff_classes=(0, 1), max_instances=4096, dual_set=False,
               nms_iou=0.3, **kw):
    super().__init__(num_labels + 3, **kw)
    self.dual_set, self.nms_iou = bool(dual_set), float(nms_iou)
    self.num_labels = num_labels  # the classes; the model has num_labels + 3 outputs
    self.voxel_size, self.radius, self.min_points = float(voxel_size), float(radius), int(min_points)
    self.stuff_classes, self.max_instances = tuple(stuff_classes), int(max_instances)
    self._full_width = False

  def forward(self, coords, feats, training=True):
    out = super().forward(coords, feats, training)
    return out if (training or self._full_width) else out[:, :self.num_labels]

  def offset_targets(self, coords, instance, n_instances):
    """float32 [n, 3]: centroid of the row's instance - the row's voxel, in metres (rows with instance < 0: unused)."""
    c = coords.to(device=self.device, dtype=torch.int32).contiguous()
    inst = instance.to(device=self.device, dtype=torch.int32)
    s, cnt = PF.instance_centroids(c, inst, n_instances)
    centre = s.double() / cnt.clamp(min=1).double().reshape(-1, 1)
    picked = centre[inst.clamp(min=0).long()] if n_instances else torch.zeros((c.shape[0], 3), dtype=torch.float64, device=self.device)
    return ((picked - c[:, 1:4].double()) * self.voxel_size).float()

  def train_iter(self, coords, feats, target, instance, n_instances=None):
    """instance [n]: the row's ground-truth instance as an index into the batch's instances (unique across its scenes), -1 for
    none; n_instances: their number (None: instance.max() + 1, free for a host tensor)."""
    self.model.train()
    self.optimizer.zero_grad()
    C = self.num_labels
    if torch.is_tensor(target) and not target.is_cuda and target.numel():  # free on the host; as torch's CrossEntropyLoss
      bad = (target != self.ignore_label) & ((target < 0) | (target >= C))
      if bool(bad.any()):
        raise IndexError("Target %d is out of bounds (classes 0..%d, ignore label %d)" % (int(target[bad][0]), C - 1, self.ignore_label))
    if n_instances is None:
      n_instances = int(instance.max()) + 1 if instance.numel() else 0
    logits = self.forward(coords, feats).requires_grad_(True)
    tgt = target.to(self.device)
    inst = instance.to(device=self.device, dtype=torch.int32)
    goal = self.offset_targets(coords, inst, max(int(n_instances), 0))
    loss_sem = PF.SoftmaxCrossEntropyFunction.apply(logits[:, :C], tgt, self.ignore_label)
    loss_norm, loss_dir = PF.OffsetLossFunction.apply(logits[:, C:C + 3], goal, inst)
    loss = loss_sem + loss_norm + loss_dir
    loss.backward()
    self.engine.backward(0, logits.grad)
    self.optimizer.step()
    self.scheduler.step()
    self.curr_iter += 1
    pred = logits.detach()[:, :C].max(1)[1]
    return {"loss": loss.detach(), "loss_sem": loss_sem.detach(), "loss_norm": loss_norm.detach(), "loss_dir": loss_dir.detach(),
            "score": precision_at_one(pred, tgt, self.ignore_label), "pred": pred}

  @torch.no_grad()
  def predict(self, coords, feats):
    """cluster_instances of the inference forward (eval mode): its dict.  With dual_set: cluster_proposals' dict (overlapping
    masks after non-maximum suppression at nms_iou), which both evaluators and step_points take as well."""
    self.model.eval()
    self._full_width = True
    try:
      out = self.forward(coords, feats, training=False)
    finally:
      self._full_width = False
    C = self.num_labels
    if self.dual_set:
      return cluster_proposals(coords, out[:, C:C + 3], out[:, :C], scene_offsets_of(coords), self.voxel_size, self.radius, self.min_points,
                               self.stuff_classes, self.max_instances, nms_iou=self.nms_iou)
    return cluster_instances(coords, out[:, C:C + 3], out[:, :C], scene_offsets_of(coords), self.voxel_size, self.radius, self.min_points,
                             self.stuff_classes, self.max_instances)

  def train_iter_scenes(self, scenes, draws=None, limit_numpoints=0, crop_draws=None):
    """One iteration from raw scans of (xyz, colours, labels, instance_ids): self.input_pipeline (an InstanceInputPipeline, the
    constructor's argument), then train_iter on its device tensors.  The result carries the batch's `transformation` too."""
    assert isinstance(self.input_pipeline, InstanceInputPipeline), "construct the trainer with input_pipeline=InstanceInputPipeline(aug, device)"
    coords, feats, target, instance, n_instances, transformation = self.input_pipeline(scenes, draws, limit_numpoints, crop_draws)
    out = self.train_iter(coords, feats, target, instance, n_instances)
    out["transformation"] = transformation
    return out

  @torch.no_grad()
  def validate_scenes(self, batches, benchmark=False):
    """Mask AP over an iterable of scene lists (each a batch of (xyz, colours, labels, instance_ids)): a non-augmenting, non-
    cropping InstanceInputPipeline on self.input_pipeline's constants, predict, PF.instance_table (the ground truth's class and
    scene per instance, which the evaluator then does not derive), InstanceEvaluator.step -- InstanceBenchmarkEvaluator.step
    with benchmark=True -- and compute_metrics().  Returns its dict; the evaluator stays on self.instance_evaluator."""
    assert isinstance(self.input_pipeline, InstanceInputPipeline), "construct the trainer with input_pipeline=InstanceInputPipeline(aug, device)"
    pipe = InstanceInputPipeline(self.input_pipeline.aug.replace(augment=False), self.device, self.input_pipeline.stuff_classes)
    ev = (InstanceBenchmarkEvaluator if benchmark else InstanceEvaluator)(self.num_labels, self.stuff_classes, device=self.device)
    self.instance_evaluator = ev
    for scenes in batches:
      coords, feats, target, instance, n_instances, _ = pipe(scenes)
      pred = self.predict(coords, feats)
      table = PF.instance_table(instance, target, None, pred["scene_offsets"], n_instances)
      ev.step(pred, instance, target, n_instances, table=table)
    return ev.compute_metrics()

  def benchmark_original_pointcloud(self, batches, min_region=100):
    """The benchmark protocol on the ORIGINAL vertices (InstanceBenchmarkEvaluator: restated from the rules of ScanNet's
    script, never run against the script) over an iterable of (coords, feats, transformation, points, point_instance,
    point_class): predict per batch, the voxels' instance ids carried onto the vertices by step_points, one read-back at the
    end.  points / point_instance / point_class: one array per scene of the batch (a list), or a single array for a batch of
    one scene, as test_original_pointcloud takes them; point_instance numbers the batch's instances (-1: none).  Returns the
    metrics dict; the evaluator stays on self.benchmark_evaluator and the per-vertex instance ids of every batch (device
    tensors) on self.benchmark_predictions."""
    self.benchmark_evaluator = InstanceBenchmarkEvaluator(self.num_labels, self.stuff_classes, min_region, device=self.device)
    self.benchmark_predictions = []
    for coords, feats, transformation, points, point_instance, point_class in batches:
      if isinstance(points, (list, tuple)):
        sizes = [len(p) for p in points]
        points = torch.cat([torch.as_tensor(p).reshape(-1, 3) for p in points])
        point_instance = torch.cat([torch.as_tensor(np.asarray(i)).reshape(-1) for i in point_instance])
        point_class = torch.cat([torch.as_tensor(np.asarray(c)).reshape(-1) for c in point_class])
      else:
        sizes = [len(points)]
      offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64)
      pred = self.predict(coords, feats)
      self.benchmark_predictions.append(
          self.benchmark_evaluator.step_points(coords, pred, transformation, points, point_instance, point_class, offsets))
    return self.benchmark_evaluator.compute_metrics()


def _member_overlap(member, gi, P, G):
  """instance_overlap for overlapping masks: member int32 [n, S] (cluster_proposals'), gi int64 [n] -> (inter [P, G], pred_size
  [P], gt_size [G]).  The predictions' side is taken over the n S ENTRIES -- member.reshape(-1) against the ground truth repeated
  per column -- and the ground truth's sizes over the n ROWS: every row stands S times among the entries, so the entry count
  is exactly S times the row count, and a row in two masks does not count its ground truth twice."""
  S = member.shape[1]
  inter, ps, gs = PF.instance_overlap(member.reshape(-1), gi.repeat_interleave(S), P, G)
  return inter, ps, torch.div(gs, S, rounding_mode="floor")


def _table_cls_scene(table, G):
  """(cls, scene) int64 [G] of PF.instance_table's dict: what the evaluators' scatter_reduce derivation gives."""
  assert table["cls"] is not None and table["cls"].shape[0] == G and table["scene"].shape[0] == G, "table: instance_table's dict with klass, for G"
  return table["cls"].to(torch.int64), table["scene"].to(torch.int64)


class InstanceEvaluator:
  """Mask AP of predicted instances (cluster_instances' dict) against ground-truth instances, accumulated on the device.

  step(pred, gt_instance, gt_class) adds one batch: pcmi_instance_overlap and pcmi_instance_match (per prediction its best
  ground-truth instance of the same scene and class).  compute_metrics() sorts every prediction by (class, descending score)
  with a stable torch.sort, runs PF.det_ap ONCE for all thresholds and reads back once.  This is VOC-style matching, the rule
  APCalculator already uses -- NOT ScanNet's benchmark script, which has void-overlap and minimum-region rules."""

  def __init__(self, num_labels, stuff_classes=(0, 1), thresholds=AP_THRESHOLDS, device=None):
    self.num_labels, self.stuff_classes = int(num_labels), tuple(int(s) for s in stuff_classes)
    self.thresholds = tuple(float(t) for t in thresholds)
    self.device = None if device is None else torch.device(device)
    self.reset()

  def reset(self):
    self._iou, self._gid, self._cls, self._score, self.npos, self.n_gt = [], [], [], [], None, 0

  def step(self, pred, gt_instance, gt_class, n_instances=None, table=None):
    """pred: cluster_instances' dict; gt_instance [n]: the row's ground-truth instance as an index into the batch's instances,
    -1 for none; gt_class [n]: the row's ground-truth class (an instance takes the largest class among its rows; instances of
    stuff_classes or of a class outside [0, num_labels) are not scored).  n_instances None: gt_instance.max() + 1.  table:
    PF.instance_table's dict for (gt_instance, gt_class, pred["scene_offsets"], n_instances) -- its cls and scene are then taken
    instead of being derived here; the metrics are the same bits.  A pred with `member` [n, S] (cluster_proposals' dict:
    overlapping masks) is scored on its entries instead of `instance`: _member_overlap."""
    dev = pred["instance"].device
    if self.device is None:
      self.device = dev
    gi_any = torch.as_tensor(gt_instance).reshape(-1)
    G = int(n_instances) if n_instances is not None else (int(gi_any.max()) + 1 if gi_any.numel() else 0)
    G = max(G, 0)
    gi = gi_any.to(device=dev, dtype=torch.int64)
    gc = torch.as_tensor(gt_class).reshape(-1).to(device=dev, dtype=torch.int64)
    n, C = gi.shape[0], self.num_labels
    if table is not None:
      cls, scene = _table_cls_scene(table, G)
    else:
      row_scene = torch.searchsorted(pred["scene_offsets"], torch.arange(n, device=dev), right=True) - 1
      ok = (gi >= 0) & (gi < G)
      cls = torch.full((G,), -1, dtype=torch.int64, device=dev).scatter_reduce(0, gi[ok], gc[ok], "amax", include_self=True)
      scene = torch.full((G,), -1, dtype=torch.int64, device=dev).scatter_reduce(0, gi[ok], row_scene[ok], "amax", include_self=True)
    scored = (cls >= 0) & (cls < C)
    for s in self.stuff_classes:
      scored = scored & (cls != s)
    cls = torch.where(scored, cls, torch.full_like(cls, -1))
    P = pred["inst_size"].shape[0]
    if "member" in pred:
      inter, ps, gs = _member_overlap(pred["member"], gi, P, G)
    else:
      inter, ps, gs = PF.instance_overlap(pred["instance"], gi, P, G)
    best_gt, best_iou = PF.instance_match(inter, ps, gs, pred["inst_scene"], pred["inst_class"], scene, cls)
    self._iou.append(best_iou)
    self._gid.append(torch.where(best_gt >= 0, best_gt + self.n_gt, best_gt))
    self._cls.append(pred["inst_class"])
    self._score.append(pred["inst_score"])
    npos = torch.bincount(cls[scored], minlength=C)[:C]
    self.npos = npos if self.npos is None else self.npos + npos
    self.n_gt += G

  def compute_metrics(self, keep_curves=False):
    """One read-back.  AP (the mean over 0.50:0.95:0.05), AP50, AP25: nanmeans over the classes with ground truth of
    ap_class / ap50_class / ap25_class (per class, NaN without ground truth); ap [T, classes]; n_gt per class.  keep_curves:
    self.last_ap keeps det_ap's device tensors (rec, prec, tp [T, nd]) and `order`, the accumulated predictions in list order."""
    C, T = self.num_labels, len(self.thresholds)
    if not self._iou:
      nan = np.full(C, np.nan)
      return dict(AP=float("nan"), AP50=float("nan"), AP25=float("nan"), ap_class=nan, ap50_class=nan.copy(), ap25_class=nan.copy(),
                  n_gt=np.zeros(C, np.int64), ap=np.full((T, C), np.nan))
    iou, gid, cls, score = torch.cat(self._iou), torch.cat(self._gid), torch.cat(self._cls).long(), torch.cat(self._score)
    cls = torch.where((cls >= 0) & (cls < C), cls, torch.full_like(cls, C))  # unused slots and foreign classes: behind every range
    by_score = torch.sort(score, descending=True, stable=True).indices
    order = by_score[torch.sort(cls[by_score], stable=True).indices]
    cls_offs = torch.searchsorted(cls[order].contiguous(), torch.arange(C + 1, device=cls.device)).to(torch.int32)
    out = PF.det_ap(iou[order], gid[order].to(torch.int32), cls_offs, self.npos.to(torch.int32), self.n_gt, self.thresholds,
                    curves=keep_curves)
    self.last_ap = dict(out, order=order) if keep_curves else None
    flat = torch.cat([out["ap"].reshape(-1), self.npos.double()]).cpu().numpy()
    ap, n_gt = flat[:T * C].reshape(T, C), np.rint(flat[T * C:]).astype(np.int64)
    ap[:, n_gt == 0] = np.nan
    thr = np.asarray(self.thresholds)
    coco = thr >= 0.5 - 1e-9

    def at(t):
      hit = np.flatnonzero(np.abs(thr - t) < 1e-9)
      return ap[hit[0]] if len(hit) else np.full(C, np.nan)

    with warnings.catch_warnings():  # a class that never occurred: nanmean of nothing but NaN
      warnings.simplefilter("ignore", category=RuntimeWarning)
      ap_class = ap[coco].mean(0) if coco.any() else np.full(C, np.nan)
      ap50, ap25 = at(0.5), at(0.25)
      return dict(AP=float(np.nanmean(ap_class)), AP50=float(np.nanmean(ap50)), AP25=float(np.nanmean(ap25)), ap_class=ap_class,
                  ap50_class=ap50, ap25_class=ap25, n_gt=n_gt, ap=ap)


class InstanceBenchmarkEvaluator:
  """Mask AP by the protocol of ScanNet's benchmark script (evaluate_semantic_instance.py), accumulated on the device --
  **restated from the script's rules, never run against the script** (include/pcmi.h states them; INTEGRATION.md lists the
  differences).  Beside InstanceEvaluator's VOC-style matching it drops predictions of fewer than min_region rows, does not
  count ground truths that small, ignores an unmatched prediction that lies mostly on void (no instance, or an instance of an
  unscored class) or on small ground truths, lets duplicate predictions claim by the script's rule and integrates the
  precision-recall curve as the script does.  Figures of the two evaluators are not comparable.

  step(pred, gt_instance, gt_class) adds one batch on the rows it is given; step_points(...) carries the voxels' instance ids
  onto the original vertices first, as PointCloudEvaluator.step carries classes, which is where published numbers are taken.
  compute_metrics() sorts the predictions once by descending score and once by class (stable torch.sorts), runs
  PF.instance_bench_ap ONCE for all thresholds and reads back once."""

  def __init__(self, num_labels, stuff_classes=(0, 1), min_region=100, thresholds=BENCHMARK_THRESHOLDS, device=None):
    self.num_labels, self.stuff_classes = int(num_labels), tuple(int(s) for s in stuff_classes)
    self.min_region = int(min_region)
    self.thresholds = tuple(float(t) for t in thresholds)
    self.device = None if device is None else torch.device(device)
    self.reset()

  def reset(self):
    self._flag, self._cls, self._score, self.npos = [], [], [], None

  def step(self, pred, gt_instance, gt_class, n_instances=None, table=None):
    """pred: cluster_instances' dict (instance [n], inst_class, inst_scene, inst_score [P], scene_offsets [B + 1] over the n
    rows); gt_instance [n]: the row's ground-truth instance as an index into the batch's instances, -1 for none; gt_class [n]:
    the row's ground-truth class (an instance takes the largest class among its rows and the scene of its last row; instances of
    stuff_classes or of a class outside [0, num_labels) are not scored: their rows are void).  n_instances None:
    gt_instance.max() + 1.  The size of a prediction is its rows among the n given, NOT pred["inst_size"]; a score that is not
    finite counts as 0.  table: PF.instance_table's dict for (gt_instance, gt_class, pred["scene_offsets"], n_instances) -- its
    cls and scene are then taken instead of being derived here; the metrics are the same bits.  A pred with `member` [n, S]
    (cluster_proposals' dict: overlapping masks) is scored on its entries instead of `instance`: overlaps, sizes and void
    overlaps of the predictions over the n S entries, the ground truth's sizes over the n rows.  Nothing is read back."""
    dev = pred["instance"].device
    if self.device is None:
      self.device = dev
    gi_any = torch.as_tensor(gt_instance).reshape(-1)
    G = int(n_instances) if n_instances is not None else (int(gi_any.max()) + 1 if gi_any.numel() else 0)
    G = max(G, 0)
    gi = gi_any.to(device=dev, dtype=torch.int64)
    gc = torch.as_tensor(gt_class).reshape(-1).to(device=dev, dtype=torch.int64)
    n, C = gi.shape[0], self.num_labels
    offs = pred["scene_offsets"].to(device=dev, dtype=torch.int64)
    B = offs.shape[0] - 1
    if table is not None:
      cls, scene = _table_cls_scene(table, G)
    else:
      row_scene = torch.searchsorted(offs, torch.arange(n, device=dev), right=True) - 1
      ok = (gi >= 0) & (gi < G)
      cls = torch.full((G,), -1, dtype=torch.int64, device=dev).scatter_reduce(0, gi[ok], gc[ok], "amax", include_self=True)
      scene = torch.full((G,), -1, dtype=torch.int64, device=dev).scatter_reduce(0, gi[ok], row_scene[ok], "amax", include_self=True)
    scored = (cls >= 0) & (cls < C)
    for s in self.stuff_classes:
      scored = scored & (cls != s)
    cls = torch.where(scored, cls, torch.full_like(cls, -1))
    P = pred["inst_class"].shape[0]
    if "member" in pred:
      inter, ps, gs = _member_overlap(pred["member"], gi, P, G)
      S = pred["member"].shape[1]
      void = PF.instance_void_overlap(pred["member"].reshape(-1), gi.repeat_interleave(S), scored, P)
    else:
      inter, ps, gs = PF.instance_overlap(pred["instance"], gi, P, G)
      void = PF.instance_void_overlap(pred["instance"], gi, scored, P)
    score = pred["inst_score"].to(device=dev, dtype=torch.float64)
    score = torch.where(torch.isfinite(score), score, torch.zeros_like(score))
    if self.npos is None:
      self.npos = torch.zeros(C, dtype=torch.int32, device=dev)
    flag, _, _ = PF.instance_bench_match(inter, ps, gs, void, pred["inst_scene"], pred["inst_class"], score, scene, cls, B, C,
                                         self.thresholds, self.min_region, npos=self.npos)
    self._flag.append(flag)
    self._cls.append(pred["inst_class"])
    self._score.append(score)

  def step_points(self, coords, pred, transformation, points, point_instance, point_class, point_offsets):
    """coords int32 [nv, 4] (b, x, y, z) and pred (cluster_instances' dict on those voxels); transformation [B, 16]: the
    voxelizer matrices as the loader returns them (host); points float64 [n, 3]: the original vertices, scene b at rows
    [point_offsets[b], point_offsets[b + 1]); point_instance / point_class [n]: their ground truth as step takes it.  A vertex
    takes the instance id of the voxel whose centre is nearest (voxel_centers, nearest_point with a cell of two voxel edges,
    after a stable sort of the voxels by batch index: PointCloudEvaluator.step's carry), -1 where there is none (a scene
    without voxels, a non-finite vertex); then step on the vertices.  Returns the per-vertex instance id (int32 [n], device)."""
    dev = pred["instance"].device
    T = np.asarray(transformation.cpu() if torch.is_tensor(transformation) else transformation, dtype=np.float64)
    T = T[:, :16] if T.ndim == 2 else T.reshape(-1, 16)
    B = T.shape[0]
    c = torch.as_tensor(coords).to(dev).to(torch.int32)
    order = torch.sort(c[:, 0], stable=True)[1]
    c, vi = c[order].contiguous(), pred["instance"].reshape(-1).to(torch.int32)[order]
    ref_offs = torch.searchsorted(c[:, 0].contiguous(), torch.arange(B + 1, dtype=torch.int32, device=dev)).to(torch.int64)
    centers = PF.voxel_centers(c, T)
    edge = float(max(np.linalg.norm(np.linalg.inv(T.reshape(-1, 4, 4))[:, :3, 0], axis=1).max(), 0.0))
    cell = 2.0 * edge if np.isfinite(edge) and edge > 0 else None
    pts = torch.as_tensor(points)
    assert pts.dtype == torch.float64, "points: float64 [n, 3] (the original vertices, unrounded)"
    offs = torch.as_tensor(point_offsets).to(device=dev, dtype=torch.int64)
    idx = PF.nearest_point(centers, ref_offs, pts.to(dev), offs, cell=cell).long()
    if vi.numel():
      inst = torch.where(idx >= 0, vi[idx.clamp(min=0)], torch.full_like(idx, -1, dtype=torch.int32))
    else:
      inst = torch.full((idx.shape[0],), -1, dtype=torch.int32, device=dev)
    carried = dict(pred, instance=inst, scene_offsets=offs)
    if "member" in pred:  # overlapping masks: every column of the voxel's row, by the same gather
      vm = pred["member"].to(torch.int32)[order]
      none = torch.full((idx.shape[0], vm.shape[1]), -1, dtype=torch.int32, device=dev)
      carried["member"] = torch.where((idx >= 0).reshape(-1, 1), vm[idx.clamp(min=0)], none) if vm.shape[0] else none
    self.step(carried, point_instance, point_class)
    return inst

  def compute_metrics(self, keep_curves=False):
    """One read-back.  The keys of InstanceEvaluator.compute_metrics: AP (the mean over the thresholds not close to 0.25, the
    script's all_ap), AP50, AP25: nanmeans over the classes with counted ground truth of ap_class / ap50_class / ap25_class
    (per class, NaN without ground truth, 0 with ground truth and no entry); ap [T, classes]; n_gt per class.  keep_curves:
    self.last_ap keeps instance_bench_ap's device tensors (prec, rec [T, 3 nd]) and `order`, the accumulated predictions in
    list order: entry 3 k + s is slot s of prediction order[k]."""
    C, T = self.num_labels, len(self.thresholds)
    if not self._flag:
      nan = np.full(C, np.nan)
      return dict(AP=float("nan"), AP50=float("nan"), AP25=float("nan"), ap_class=nan, ap50_class=nan.copy(), ap25_class=nan.copy(),
                  n_gt=np.zeros(C, np.int64), ap=np.full((T, C), np.nan))
    flag, cls, score = torch.cat(self._flag, 1), torch.cat(self._cls).long(), torch.cat(self._score)
    cls = torch.where((cls >= 0) & (cls < C), cls, torch.full_like(cls, C))  # unused slots and foreign classes: behind every range
    by_score = torch.sort(score, descending=True, stable=True).indices
    order = by_score[torch.sort(cls[by_score], stable=True).indices]
    cls_offs = (3 * torch.searchsorted(cls[order].contiguous(), torch.arange(C + 1, device=cls.device))).to(torch.int32)
    out = PF.instance_bench_ap(flag[:, order, :].reshape(T, -1), score[order].repeat_interleave(3), cls_offs, self.npos,
                               curves=keep_curves)
    self.last_ap = dict(out, order=order) if keep_curves else None
    flat = torch.cat([out["ap"].reshape(-1), self.npos.double()]).cpu().numpy()
    ap, n_gt = flat[:T * C].reshape(T, C), np.rint(flat[T * C:]).astype(np.int64)
    ap[:, n_gt == 0] = np.nan
    return metrics_from_ap(ap, n_gt, self.thresholds)


def metrics_from_ap(ap, n_gt, thresholds):
  """The metrics dict of InstanceBenchmarkEvaluator from ap [T, classes] (NaN: a class without counted ground truth)."""
  C = ap.shape[1]
  thr = np.asarray(thresholds, dtype=np.float64)
  rest = ~np.isclose(thr, 0.25)

  def at(t):
    hit = np.flatnonzero(np.isclose(thr, t))
    return ap[hit[0]] if len(hit) else np.full(C, np.nan)

  with warnings.catch_warnings():  # a class that never occurred: nanmean of nothing but NaN
    warnings.simplefilter("ignore", category=RuntimeWarning)
    ap_class = ap[rest].mean(0) if rest.any() else np.full(C, np.nan)
    ap50, ap25 = at(0.5), at(0.25)
    return dict(AP=float(np.nanmean(ap_class)), AP50=float(np.nanmean(ap50)), AP25=float(np.nanmean(ap25)), ap_class=ap_class,
                ap50_class=ap50, ap25_class=ap25, n_gt=n_gt, ap=ap)
