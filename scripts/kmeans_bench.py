"""Times the active labelling (csrc/kmeans.hip) on a ScanNet-sized batch against the composition it replaces and the host.

The batch is SYNTHETIC: 8 scenes of 150 000 rows of 32 unit-norm channels drawn around 40 directions per scene -- the sizes of
a ScanNet training batch of pre-trained features, not their distribution.  For K in {20, 200}, on warm kernels, device events,
the variants ALTERNATING inside one process and one loop, the median of --runs:
  step         one kmeans_step (assignment + fixed-point sums in one pass, new centroids)
  composition  the same iteration from existing parts: feature_nn against the centroids, then torch.index_add_ of the rows and
               a count (float32 sums: not the same bits, the same work)
  seeding      kmeans_pp_init: K kmeans_pp_step calls
  select       the whole kmeans_select (seeding, --iters iterations, final pass, one read-back)
  host         scipy.cluster.vq.kmeans2(minit="++", iter=--iters) on ONE scene on this machine's CPU, if scipy imports
Prints one JSON line.

  python scripts/kmeans_bench.py [--scenes 8] [--rows 150000] [--runs 25] [--iters 10] [--no-host]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def batch(n_scenes, rows, c, seed=0):
  rng = np.random.default_rng(seed)
  out = []
  for _ in range(n_scenes):
    dirs = rng.normal(size=(40, c))
    x = dirs[rng.integers(0, 40, rows)] + rng.normal(0, 0.35, (rows, c))
    out.append((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))
  return np.concatenate(out), np.arange(n_scenes + 1, dtype=np.int64) * rows


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--scenes", type=int, default=8)
  ap.add_argument("--rows", type=int, default=150000)
  ap.add_argument("--channels", type=int, default=32)
  ap.add_argument("--runs", type=int, default=25)
  ap.add_argument("--iters", type=int, default=10)
  ap.add_argument("--no-host", action="store_true")
  a = ap.parse_args()
  assert torch.cuda.is_available(), "kmeans_bench measures the device path: it needs the GPU"
  from pointcontrast_amd import functional as PF
  dev = torch.device("cuda", 0)
  feat, offs = batch(a.scenes, a.rows, a.channels)
  feat_d, B, C = torch.from_numpy(feat).to(dev), a.scenes, a.channels
  offs_d = torch.from_numpy(offs).to(dev)
  res = dict(scenes=B, rows_per_scene=a.rows, channels=C, iters=a.iters, runs=a.runs, synthetic=True)

  def timed_alternating(fns, runs):
    """{name: fn} -> {name: stats}: every run times each variant once, in turn."""
    for fn in fns.values():
      fn()
      fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(runs):
      for k, fn in fns.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms[k].append(e0.elapsed_time(e1))
    return {k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for k, v in ms.items()}

  for K in (20, 200):
    draws = PF.KMeansDraws.sample(B, K, torch.Generator().manual_seed(K))
    init = PF.kmeans_pp_init(feat_d, offs_d, K, draws, a.rows)
    cen, live, _ = PF.kmeans_init(feat_d, offs_d, init, a.rows)
    k_offs = torch.arange(B + 1, dtype=torch.int64, device=dev) * K
    scene_base = (torch.arange(B, device=dev) * K).repeat_interleave(a.rows)

    def step():
      return PF.kmeans_step(feat_d, offs_d, cen, live, None, a.rows)

    def composition():
      nn, _ = PF.feature_nn(feat_d, offs_d, cen.reshape(B * K, C), k_offs)
      idx = nn.long()
      s = torch.zeros((B * K, C), dtype=torch.float32, device=dev).index_add_(0, idx, feat_d)
      cnt = torch.zeros(B * K, dtype=torch.float32, device=dev).index_add_(0, idx, torch.ones_like(idx, dtype=torch.float32))
      return torch.where(cnt[:, None] > 0, s / cnt[:, None].clamp(min=1), cen.reshape(B * K, C)), nn

    st, (cc, nn) = step(), composition()
    agree = float((st["assign"] + scene_base == nn).float().mean())
    out = dict(assignments_equal_fraction=agree,
               centroid_max_abs_diff=float((st["centroid"].reshape(B * K, C) - cc).abs().max()))
    out.update(timed_alternating(dict(step_ms=step, composition_ms=composition), a.runs))
    out.update(timed_alternating(dict(seeding_ms=lambda: PF.kmeans_pp_init(feat_d, offs_d, K, draws, a.rows),
                                      select_ms=lambda: PF.kmeans_select(feat_d, offs_d, K, draws, iters=a.iters, max_scene_rows=a.rows)),
                                 a.runs))
    if not a.no_host:
      try:
        from scipy.cluster.vq import kmeans2
        t0 = time.perf_counter()
        kmeans2(feat[:a.rows].astype(np.float64), K, iter=a.iters, minit="++", seed=0)
        out["host_kmeans2_one_scene_ms"] = (time.perf_counter() - t0) * 1e3
      except ImportError:
        out["host_kmeans2_one_scene_ms"] = None
    res["K%d" % K] = out
  print(json.dumps(res))


if __name__ == "__main__":
  main()
