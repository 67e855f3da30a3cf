"""Times the benchmark-protocol evaluation of instance masks (csrc/insbench.hip, InstanceBenchmarkEvaluator) on a ScanNet-sized
batch, beside the existing InstanceEvaluator.step on the same batch and the numpy restatement on this machine's CPU.

The batch is insseg_bench.py's SYNTHETIC one: 8 scenes of about 150 000 occupied 2 cm voxels, 30 box "instances" each (240 in
all) -- the sizes of ScanNet scans, not their geometry.  The prediction is the ground truth DEGRADED: every fifth instance is
merged into its neighbour, every seventh dropped, every third loses a random 30 % of its rows, and 2 % of the floor joins the
instance before it; scores are random.  The original cloud is one vertex per voxel at the voxel's centre plus a jitter of
less than half a voxel.  Device times are HIP events around each call on warm kernels, the median of --runs with the variants
ALTERNATING inside one loop of one process.  The protocol is restated from the rules of ScanNet's script and was never run
against the script; nothing here says anything about accuracy.  Prints one JSON line.

  python scripts/insbench_bench.py [--scenes 8] [--voxels 150000] [--runs 25] [--no-host]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from insseg_bench import CLASSES, VOXEL, batch  # noqa: E402

MAX_INSTANCES = 4096


def degrade(inst, cls, n_boxes, rng):
  """-> predicted instance per row (numbered 0 .. P - 1 in order of first row), its class per prediction."""
  pred = inst.copy()
  G = int(inst.max()) + 1
  for g in range(G):
    if g % 5 == 4 and g % n_boxes:
      pred[inst == g] = g - 1
    elif g % 7 == 6:
      pred[inst == g] = -1
    elif g % 3 == 2:
      rows = np.flatnonzero(inst == g)
      pred[rows[rng.random(len(rows)) < 0.3]] = -1
  floor = np.flatnonzero(inst < 0)
  take = floor[rng.random(len(floor)) < 0.02]
  prev = np.maximum.accumulate(np.where(inst >= 0, np.arange(len(inst)), 0))  # the last instance row before each row
  pred[take] = pred[prev[take]]
  ids, first, inv = np.unique(pred[pred >= 0], return_index=True, return_inverse=True)
  rank = np.argsort(np.argsort(first))
  out = np.full(len(pred), -1, np.int32)
  out[pred >= 0] = rank[inv]
  pcls = np.zeros(len(ids), np.int32)
  pcls[rank] = [cls[np.flatnonzero(pred == k)[0]] for k in ids]
  return out, pcls


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--scenes", type=int, default=8)
  ap.add_argument("--voxels", type=int, default=150000)
  ap.add_argument("--boxes", type=int, default=30)
  ap.add_argument("--runs", type=int, default=25)
  ap.add_argument("--no-host", action="store_true")
  a = ap.parse_args()
  assert torch.cuda.is_available(), "insbench_bench measures the device path: it needs the GPU"
  from pointcontrast_amd import functional as PF
  from pointcontrast_amd.downstream.insseg import BENCHMARK_THRESHOLDS, InstanceBenchmarkEvaluator, InstanceEvaluator
  dev = torch.device("cuda", 0)
  coords, cls, inst, offs, rng = batch(a.scenes, a.voxels, a.boxes)
  n, G = len(coords), a.scenes * a.boxes
  pinst, pcls = degrade(inst, cls, a.boxes, rng)
  P = len(pcls)
  row_scene = coords[:, 0]
  pscene = np.array([row_scene[np.flatnonzero(pinst == k)[0]] for k in range(P)], np.int32)
  pad = lambda v, fill, dt: np.concatenate([v, np.full(MAX_INSTANCES - P, fill)]).astype(dt)  # noqa: E731
  host_pred = dict(instance=pinst, inst_class=pad(pcls, -1, np.int32), inst_scene=pad(pscene, -1, np.int32),
                   inst_score=pad(rng.random(P), 0.0, np.float64), inst_size=pad(np.bincount(pinst[pinst >= 0], minlength=P), 0, np.int32),
                   scene_offsets=offs)
  pred = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in host_pred.items()}
  gi, gc = torch.from_numpy(inst).to(dev), torch.from_numpy(cls).to(dev)
  T = np.tile(np.diag([1 / VOXEL, 1 / VOXEL, 1 / VOXEL, 1.0]).reshape(1, 16), (a.scenes, 1))
  points = (coords[:, 1:].astype(np.float64) + 0.5 + rng.uniform(-0.45, 0.45, (n, 3))) * VOXEL
  coords_d, points_d, offs_d = torch.from_numpy(coords).to(dev), torch.from_numpy(points).to(dev), torch.from_numpy(offs).to(dev)
  res = dict(scenes=a.scenes, rows=n, instances=G, predictions=P, slots=MAX_INSTANCES, thresholds=len(BENCHMARK_THRESHOLDS), synthetic=True)

  # the pieces of one step, on the tensors the evaluator derives
  gt_class = torch.full((G,), -1, dtype=torch.int64, device=dev).scatter_reduce(0, gi[gi >= 0], gc[gi >= 0], "amax")
  gt_scene = torch.from_numpy(np.repeat(np.arange(a.scenes), a.boxes)).to(dev)
  gt_class = torch.where(gt_class >= 2, gt_class, torch.full_like(gt_class, -1))
  inter, ps, gs = PF.instance_overlap(pred["instance"], gi, MAX_INSTANCES, G)
  void = PF.instance_void_overlap(pred["instance"], gi, gt_class >= 0, MAX_INSTANCES)
  match = lambda: PF.instance_bench_match(inter, ps, gs, void, pred["inst_scene"], pred["inst_class"], pred["inst_score"], gt_scene,  # noqa: E731
                                          gt_class, a.scenes, CLASSES, BENCHMARK_THRESHOLDS)
  ev = InstanceBenchmarkEvaluator(CLASSES)
  ev.step(pred, gi, gc, G)
  flag, score, order_cls = torch.cat(ev._flag, 1), torch.cat(ev._score), torch.cat(ev._cls).long()
  order_cls = torch.where(order_cls >= 0, order_cls, torch.full_like(order_cls, CLASSES))
  by_score = torch.sort(score, descending=True, stable=True).indices
  order = by_score[torch.sort(order_cls[by_score], stable=True).indices]
  cls_offs = (3 * torch.searchsorted(order_cls[order].contiguous(), torch.arange(CLASSES + 1, device=dev))).to(torch.int32)
  e_flag, e_score = flag[:, order, :].reshape(len(BENCHMARK_THRESHOLDS), -1).contiguous(), score[order].repeat_interleave(3)

  def bench_step():
    e = InstanceBenchmarkEvaluator(CLASSES)
    e.step(pred, gi, gc, G)

  def bench_step_points():
    e = InstanceBenchmarkEvaluator(CLASSES)
    e.step_points(coords_d, pred, T, points_d, gi, gc, offs_d)

  def voc_step():
    e = InstanceEvaluator(CLASSES)
    e.step(pred, gi, gc, G)

  variants = dict(instance_overlap=lambda: PF.instance_overlap(pred["instance"], gi, MAX_INSTANCES, G),
                  void_overlap=lambda: PF.instance_void_overlap(pred["instance"], gi, gt_class >= 0, MAX_INSTANCES),
                  bench_match=match, bench_ap=lambda: PF.instance_bench_ap(e_flag, e_score, cls_offs, ev.npos),
                  step=bench_step, step_points=bench_step_points, compute_metrics=ev.compute_metrics, voc_evaluator_step=voc_step)
  for fn in variants.values():  # warm-up: code objects, the workspace, torch's sort plans
    for _ in range(2):
      fn()
  torch.cuda.synchronize()
  ms = {k: [] for k in variants}
  for _ in range(a.runs):  # the variants alternate inside one loop
    for k, fn in variants.items():
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      fn()
      e1.record()
      e1.synchronize()
      ms[k].append(e0.elapsed_time(e1))
  res["device_ms"] = {k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), runs=a.runs) for k, v in ms.items()}
  res["metrics"] = {k: ev.compute_metrics()[k] for k in ("AP", "AP50", "AP25")}

  if not a.no_host:
    import insbench_ref as br
    t0 = time.perf_counter()
    ref = br.Evaluator(CLASSES)
    ref.step(host_pred, inst, cls, G)
    t1 = time.perf_counter()
    m = ref.compute_metrics()
    t2 = time.perf_counter()
    res["host_numpy_ms"] = dict(step=(t1 - t0) * 1e3, compute_metrics=(t2 - t1) * 1e3)
    res["host_agrees"] = bool(br.same_metrics(m, ev.compute_metrics()))
  print(json.dumps(res))


if __name__ == "__main__":
  main()
