"""Times the VoteNet detection head (csrc/detect.hip, pointcontrast_amd.downstream.votenet) at the reference's ScanNet shapes
(downstream/votenet_det_new: batch_size 8, num_target 256, vote_factor 1 from config/default.yaml, 40000 points and 1024
seeds as its ScanNet runs use, MAX_NUM_OBJ 64, 1 heading bin, 18 size clusters, 18 classes):
  * the three nn_distance calls of a training step, forward + backward, against the reference's spelling of the same
    formula in torch ops on the same GPU (repeat, subtract, reduce, two torch.min; written out below);
  * parse_predictions with remove_empty_box on and off, split into decode / count / NMS / read-back + list building,
    against the host path it replaces (tests/votenet_ref.py: numpy decode and NMS, one scipy Delaunay + find_simplex per
    box as the reference's extract_pc_in_box3d; one thread), timed once on a slice of the boxes and scaled.
Median of repeated launches after warm-up, device events, one process; one JSON line per measurement.

  python scripts/votenet_head_bench.py [--warmup 3] [--repeats 15] [--host-boxes 64] [--out FILE]
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

B, NUM_POINTS, NUM_SEED, K, K2, H, S, CLS, VOTE_FACTOR = 8, 40000, 1024, 256, 64, 1, 18, 18, 1
NMS_IOU, CONF = 0.25, 0.05


def timed(fn, warmup, repeats):
  for _ in range(warmup):
    fn()
  torch.cuda.synchronize()
  ms = []
  for _ in range(repeats):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    ms.append(a.elapsed_time(b))
  return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))


def nn_distance_torch(pc1, pc2, l1=False):
  """nn_distance as the reference spells it (lib/utils/nn_distance.py:47-61)."""
  N, M = pc1.shape[1], pc2.shape[1]
  diff = pc1.unsqueeze(2).repeat(1, 1, M, 1) - pc2.unsqueeze(1).repeat(1, N, 1, 1)
  dist = torch.sum(torch.abs(diff), dim=-1) if l1 else torch.sum(diff ** 2, dim=-1)
  d1, i1 = torch.min(dist, dim=2)
  d2, i2 = torch.min(dist, dim=1)
  return d1, i1, d2, i2


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--repeats", type=int, default=15)
  ap.add_argument("--host-boxes", type=int, default=64, help="boxes of the first scene the host path's empty-box test is timed on")
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  from pointcontrast_amd import functional as PF
  from pointcontrast_amd.downstream import votenet
  import votenet_fixtures as VF
  import votenet_ref as R
  dev = torch.device("cuda:0")
  rng = np.random.RandomState(0)
  results = []

  def report(name, **kw):
    rec = dict(name=name, **kw)
    results.append(rec)
    print(json.dumps(rec), flush=True)

  # ---- the three matchings of a step ----
  calls = [("votes", (B * NUM_SEED, VOTE_FACTOR, 3), True), ("objectness", (B, K, K2), False), ("center", (B, K, K2), False)]
  clouds = [(torch.from_numpy(rng.uniform(-3, 3, (b, n, 3)).astype(np.float32)).to(dev).requires_grad_(),
             torch.from_numpy(rng.uniform(-3, 3, (b, m, 3)).astype(np.float32)).to(dev).requires_grad_(), l1) for _, (b, n, m), l1 in calls]

  def step(fn):
    def run():
      total = 0
      for p1, p2, l1 in clouds:
        d1, _, d2, _ = fn(p1, p2, l1=l1)
        total = total + d1.sum() + d2.sum()
      total.backward()
      for p1, p2, _ in clouds:
        p1.grad = p2.grad = None
    return run

  ours = timed(step(votenet.nn_distance), args.warmup, args.repeats)
  theirs = timed(step(nn_distance_torch), args.warmup, args.repeats)
  report("nn_distance_x3_fwd_bwd", shapes=[c[1] for c in calls], libpcmi=ours, torch_ops=theirs,
         speedup=theirs["median_ms"] / ours["median_ms"])
  for (name, shape, l1), (p1, p2, _) in zip(calls, clouds):
    a, b = p1.detach(), p2.detach()
    o = timed(lambda: votenet.nn_distance(a, b, l1=l1), args.warmup, args.repeats)
    t = timed(lambda: nn_distance_torch(a, b, l1=l1), args.warmup, args.repeats)
    report("nn_distance_fwd_" + name, shape=shape, libpcmi=o, torch_ops=t, speedup=t["median_ms"] / o["median_ms"])

  # ---- parse_predictions ----
  arrays = VF.prediction_inputs(rng, B, K, NUM_POINTS, H, S, CLS, n_clusters=24)
  msa = rng.uniform(0.4, 1.5, (S, 3)).astype(np.float32)
  dc = VF.DatasetConfig(H, msa, CLS, True)
  ep = {k: torch.from_numpy(v).to(dev) for k, v in arrays.items()}
  cfg = dict(dataset_config=dc, remove_empty_box=True, use_3d_nms=True, cls_nms=True, nms_iou=NMS_IOU, use_old_type_nms=False,
             conf_thresh=CONF, per_class_proposal=True)
  msa_d = torch.from_numpy(msa).to(dev)
  ins = [ep[k] for k in ("center", "heading_scores", "heading_residuals", "size_scores", "size_residuals", "sem_cls_scores",
                         "objectness_scores")]
  for remove in (True, False):
    cfg["remove_empty_box"] = remove
    pts = ep["point_clouds"] if remove else None
    nms = (2, False, NMS_IOU)
    t_decode = timed(lambda: PF.box_decode(*ins, msa_d, True), args.warmup, args.repeats)
    t_count = timed(lambda: PF.box_decode(*ins, msa_d, True, with_counts_of=pts), args.warmup, args.repeats) if remove else None
    t_nms = timed(lambda: PF.box_decode(*ins, msa_d, True, with_counts_of=pts, nms=nms), args.warmup, args.repeats)
    wall = []
    for _ in range(args.warmup + args.repeats):
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      out = votenet.parse_predictions(ep, cfg, heading="zero")
      wall.append((time.perf_counter() - t0) * 1e3)
    wall = statistics.median(wall[args.warmup:])
    dev_ms = t_nms["median_ms"]
    report("parse_predictions", remove_empty_box=remove, decode_ms=t_decode["median_ms"],
           count_ms=(t_count["median_ms"] - t_decode["median_ms"]) if remove else 0.0,
           nms_ms=dev_ms - (t_count["median_ms"] if remove else t_decode["median_ms"]), device_ms=dev_ms,
           readback_and_lists_ms=wall - dev_ms, wall_ms=wall, detections=[len(o) for o in out])

  # ---- the host path it replaces, one thread ----
  from scipy.spatial import Delaunay
  torch.set_num_threads(1)
  t0 = time.perf_counter()
  dec = R.box_decode(*[arrays[k] for k in ("center", "heading_scores", "heading_residuals", "size_scores", "size_residuals",
                                            "sem_cls_scores", "objectness_scores")], msa, True)
  host_decode = (time.perf_counter() - t0) * 1e3
  nb = min(args.host_boxes, K)
  pc = arrays["point_clouds"][0, :, :3].astype(np.float64)
  corners = dec["corners"][0]
  depth = np.stack([corners[..., 0], corners[..., 2], -corners[..., 1]], -1)
  t0 = time.perf_counter()
  host_counts = [int((Delaunay(depth[j]).find_simplex(pc) >= 0).sum()) for j in range(nb)]
  host_count = (time.perf_counter() - t0) * 1e3 * (B * K / nb)
  dev_counts = PF.box_decode(*ins, msa_d, True, with_counts_of=ep["point_clouds"])["counts"][0, :nb].cpu().tolist()
  t0 = time.perf_counter()
  for i in range(B):
    R.nms(dec["minmax"][i], dec["obj_prob"][i], dec["sem_cls"][i], np.ones(K, bool), 2, False, NMS_IOU)
  host_nms = (time.perf_counter() - t0) * 1e3
  report("parse_predictions_host_path", decode_ms=host_decode, count_ms_scaled=host_count, count_boxes_timed=nb, nms_ms=host_nms,
         total_with_empty_box_ms=host_decode + host_count + host_nms, total_without_ms=host_decode + host_nms,
         counts_differing_from_device=int(sum(a != b for a, b in zip(host_counts, dev_counts))))
  if args.out:
    with open(args.out, "w") as f:
      json.dump(results, f, indent=1)


if __name__ == "__main__":
  main()
