"""Times the on-device segmentation validation (csrc/segeval.hip, pointcontrast_amd.downstream.semseg.SegmentationEvaluator) on
one synthetic batch at the shape of a 2 cm ScanNet scene: N = 200 000 rows, C = 20 classes, 10 % ignored labels, uniform random
logits.
  * SegmentationEvaluator.step (rows pass, per-class sort, AP walk): device events, median after warm-up; and its three stages
    on their own -- pcmi_seg_eval_rows, torch.sort of prob_t [C, N], pcmi_seg_ap -- the same way;
  * compute_metrics() (the one read-back): wall clock with a synchronise, median;
  * the host path it replaces, measured separately from the device step: softmax(...).cpu() (wall clock, synchronised), then
    the reference's average_precision (label_binarize + scikit-learn's average_precision_score if importable, else the numpy
    restatement of tests/segeval_ref.py) and fast_hist on the host.
One JSON line per measurement.

  python scripts/semseg_eval_bench.py [--rows 200000] [--classes 20] [--warmup 3] [--repeats 15] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def device_ms(fn, warmup, repeats):
  """Median / min / max stream time of fn() in ms (HIP events), after `warmup` untimed calls."""
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


def wall_ms(fn, warmup, repeats):
  out = []
  for i in range(warmup + repeats):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    if i >= warmup:
      out.append((time.perf_counter() - t0) * 1e3)
  return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rows", type=int, default=200000)
  ap.add_argument("--classes", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--repeats", type=int, default=15)
  ap.add_argument("--host-repeats", type=int, default=3)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  from pointcontrast_amd import functional as PF
  from pointcontrast_amd.downstream import semseg as ss
  import segeval_ref as S
  dev = torch.device("cuda:0")
  n, c = args.rows, args.classes
  rng = np.random.RandomState(0)
  logits = torch.from_numpy(rng.uniform(-3, 3, (n, c)).astype(np.float32)).to(dev)
  target_np = rng.randint(0, c, n)
  target_np[rng.rand(n) < 0.1] = 255
  target = torch.from_numpy(target_np).to(device=dev, dtype=torch.int32)
  shape = dict(rows=n, classes=c, ignored=float((target_np == 255).mean()))
  results = []

  def emit(name, **kw):
    results.append(dict(name=name, **shape, **kw))
    print(json.dumps(results[-1]), flush=True)

  ev = ss.SegmentationEvaluator(c, 255, dev)
  emit("evaluator_step", **device_ms(lambda: ev.step(logits, target), args.warmup, args.repeats))
  hist = torch.zeros((c, c), dtype=torch.int64, device=dev)
  emit("stage_rows_pass", **device_ms(lambda: PF.seg_eval_rows(logits, target, 255, hist=hist), args.warmup, args.repeats))
  prob_t = PF.seg_eval_rows(logits, target, 255)["prob_t"]
  emit("stage_sort", **device_ms(lambda: torch.sort(prob_t, dim=1, descending=True), args.warmup, args.repeats))
  sorted_prob, order = torch.sort(prob_t, dim=1, descending=True)
  emit("stage_ap_walk", **device_ms(lambda: PF.seg_ap_sorted(sorted_prob, order, target), args.warmup, args.repeats))
  metrics = {}
  timing = wall_ms(lambda: metrics.update(ev.compute_metrics()), args.warmup, args.repeats)
  emit("compute_metrics", **timing, batches=ev.batches, mAP=metrics["mAP"], mIoU=metrics["mIoU"])
  # the host path: the probabilities leave the device, scikit-learn and numpy do the rest
  holder = {}
  emit("host_softmax_cpu", **wall_ms(lambda: holder.update(prob=torch.softmax(logits, 1).cpu().numpy()), 1, args.host_repeats))
  try:
    from sklearn.metrics import average_precision_score
    from sklearn.preprocessing import label_binarize

    def host_ap(prob, t):
      with np.errstate(divide="ignore", invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return average_precision_score(label_binarize(t, classes=list(range(c))), prob, average=None)
    how = "sklearn"
  except ImportError:
    host_ap, how = S.average_precision, "numpy restatement"
  pred = holder["prob"].argmax(1)
  sec_ap, sec_hist = [], []
  for _ in range(args.host_repeats):
    t0 = time.perf_counter()
    host = host_ap(holder["prob"], target_np)
    sec_ap.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    ss.fast_hist(pred, target_np, c)
    sec_hist.append(time.perf_counter() - t0)
  emit("host_average_precision", how=how, median_ms=statistics.median(sec_ap) * 1e3, min_ms=min(sec_ap) * 1e3, max_ms=max(sec_ap) * 1e3)
  emit("host_fast_hist", median_ms=statistics.median(sec_hist) * 1e3, min_ms=min(sec_hist) * 1e3, max_ms=max(sec_hist) * 1e3)
  dev_ap = PF.seg_ap_sorted(sorted_prob, order, target).cpu().numpy()
  emit("device_vs_host_ap", max_abs_diff=float(np.nanmax(np.abs(dev_ap - np.asarray(host, np.float64)))))
  if args.out:
    with open(args.out, "w") as f:
      for r in results:
        f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
  main()
