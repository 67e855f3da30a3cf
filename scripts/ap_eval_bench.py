"""Times the on-device detection scoring (csrc/evaldet.hip, pointcontrast_amd.downstream.votenet.APCalculator) on a synthetic
evaluation at the reference's ScanNet shape: 312 scenes in batches of 8, 256 proposals, 18 classes with per_class_proposal,
up to 64 labelled boxes per scene, thresholds 0.25 and 0.5 scored from one match.
  * step_decoded per batch (label decode, match, record building): device events, median after warm-up;
  * compute_metrics() over the whole evaluation (sorts, true positives, curves, AP, the one read-back): wall clock with a
    synchronise, median;
  * the host path it replaces, restated in tests/ap_ref.py (numpy float64, one thread; the reference itself is absent where
    this runs): the time per box pair measured on a slice, and the whole evaluation's overlap calls scaled from it -- the
    reference evaluates each threshold separately, so its cost doubles for two.
One JSON line per measurement.

  python scripts/ap_eval_bench.py [--warmup 2] [--repeats 7] [--host-pairs 2000] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SCENES, B, K, K2, CLS = 312, 8, 256, 64, 18
THRESHOLDS = (0.25, 0.5)


class AxisAlignedConfig:
  """ScanNet style: no heading, size = mean size of the class + residual."""
  num_heading_bin, num_class, num_size_cluster = 1, CLS, CLS

  def __init__(self, rng):
    self.mean_size_arr = rng.uniform(0.4, 1.5, (CLS, 3)).astype(np.float32)

  def class2angle(self, pred_cls, residual, to_label_format=True):
    return 0

  def class2size(self, pred_cls, residual):
    return self.mean_size_arr[int(pred_cls)] + residual


def make_batch(rng, dc, dev):
  """(decoded, end_points): labelled boxes (a random number up to 64 per scene) and proposals scattered around them."""
  n_gt = rng.randint(4, K2 + 1, B)
  mask = (np.arange(K2)[None] < n_gt[:, None]).astype(np.float32)
  center = rng.uniform(-4, 4, (B, K2, 3)) * (1, 1, 0.3)
  size_class = rng.randint(0, CLS, (B, K2))
  ep = dict(center_label=center.astype(np.float32), heading_class_label=np.zeros((B, K2), np.int64),
            heading_residual_label=np.zeros((B, K2), np.float32), size_class_label=size_class,
            size_residual_label=rng.uniform(-0.1, 0.1, (B, K2, 3)).astype(np.float32), sem_cls_label=size_class, box_label_mask=mask)
  owner = rng.randint(0, K2, (B, K)) % n_gt[:, None]
  c = np.take_along_axis(center, owner[..., None].repeat(3, -1), 1) + rng.normal(0, 0.15, (B, K, 3))
  size = dc.mean_size_arr[np.take_along_axis(size_class, owner, 1)] * rng.uniform(0.8, 1.2, (B, K, 3))
  sign = np.array([[1, 1, -1, -1, 1, 1, -1, -1], [1, 1, 1, 1, -1, -1, -1, -1], [1, -1, -1, 1, 1, -1, -1, 1]], np.float64)
  cam = np.stack([c[..., 0], -c[..., 2], c[..., 1]], -1)
  corners = np.stack([sign[0] * size[..., 0:1] / 2 + cam[..., 0:1], sign[1] * size[..., 2:3] / 2 + cam[..., 1:2],
                      sign[2] * size[..., 1:2] / 2 + cam[..., 2:3]], -1)
  probs = rng.dirichlet(np.ones(CLS), (B, K))
  up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
  decoded = dict(corners=up(corners.astype(np.float32)), obj_prob=up(rng.rand(B, K).astype(np.float32)),
                 sem_cls_probs=up(probs.astype(np.float32)), sem_cls=up(probs.argmax(-1).astype(np.int32)),
                 pred_mask=up((rng.rand(B, K) > 0.3).astype(np.int32)))
  return decoded, {k: up(v) for k, v in ep.items()}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--warmup", type=int, default=2)
  ap.add_argument("--repeats", type=int, default=7)
  ap.add_argument("--host-pairs", type=int, default=2000)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  from pointcontrast_amd.downstream import votenet
  import ap_ref as A
  dev = torch.device("cuda:0")
  rng = np.random.RandomState(0)
  dc = AxisAlignedConfig(rng)
  cfg = dict(dataset_config=dc, conf_thresh=0.05, per_class_proposal=True)
  batches = [make_batch(rng, dc, dev) for _ in range(SCENES // B)]
  results = []

  def emit(name, **kw):
    results.append(dict(name=name, **kw))
    print(json.dumps(results[-1]), flush=True)

  calc = votenet.APCalculator(list(THRESHOLDS))
  for _ in range(args.warmup):
    calc.step_decoded(*batches[0], cfg)
  calc.reset()
  torch.cuda.synchronize()
  ms = []
  for decoded, ep in batches:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    calc.step_decoded(decoded, ep, cfg)
    b.record()
    b.synchronize()
    ms.append(a.elapsed_time(b))
  emit("step_decoded_per_batch", batch=B, proposals=K, classes=CLS, median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms),
       batches=len(ms))
  wall = []
  for _ in range(args.warmup + args.repeats):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    metrics = calc.compute_metrics()
    wall.append((time.perf_counter() - t0) * 1e3)
  wall = wall[args.warmup:]
  emit("compute_metrics", scenes=SCENES, detections=SCENES * K * CLS, thresholds=list(THRESHOLDS), median_ms=statistics.median(wall),
       min_ms=min(wall), max_ms=max(wall), mAP_025=float(metrics[0.25]["mAP"]), mAP_05=float(metrics[0.5]["mAP"]))
  # the host path: seconds per box pair on a slice, and the evaluation's pair count (a detection of class c meets every
  # labelled box of class c in its scene)
  decoded, ep = batches[0]
  pc = decoded["corners"].cpu().numpy().astype(np.float64).reshape(-1, 8, 3)
  gc = votenet.ground_truth_boxes(ep, cfg)[0].cpu().numpy().astype(np.float64).reshape(-1, 8, 3)
  n = args.host_pairs
  t0 = time.perf_counter()
  for i in range(n):
    A.box3d_iou(pc[i % len(pc)], gc[(7 * i) % len(gc)])
  per_pair = (time.perf_counter() - t0) / n
  pairs = 0
  for decoded, ep in batches:
    kept = ((decoded["pred_mask"] == 1) & (decoded["obj_prob"] > cfg["conf_thresh"])).sum(1).cpu().numpy()
    pairs += int((kept * ep["box_label_mask"].sum(1).cpu().numpy()).sum())
  emit("host_restatement", us_per_pair=per_pair * 1e6, pairs_per_threshold=pairs, thresholds=len(THRESHOLDS),
       scaled_seconds=per_pair * pairs * len(THRESHOLDS))
  if args.out:
    with open(args.out, "w") as f:
      for r in results:
        f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
  main()
