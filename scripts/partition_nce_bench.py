"""Times the spatially partitioned PointInfoNCE (csrc/nce_part.hip) beside the plain one (csrc/nce_x3.hip):
  * forward + backward of the loss at n = 4096, c = 32, 4 scenes, P in {2, 8, 32}, and PF.NCELossFunction at the same n in the
    same process -- the variants alternate round by round, device events, warm-up, median of 25;
  * one training step of PointNCELossTrainer and of PartitionPointNCELossTrainer on the synthetic dataset, alternating likewise.
Queries: uniform in a room of 160 x 160 x 100 voxels per scene (4 m x 4 m x 2.5 m at 2.5 cm), the default radii (20 and 80
voxels).  There is no target; the numbers go to DESIGN.md 3.24 with the commit they were taken on.  One JSON line per measurement.

  python scripts/partition_nce_bench.py [--warmup 5] [--repeats 25] [--no-trainers] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, C, SCENES, T = 4096, 32, 4, 0.4
R1_SQ, R2_SQ = 400, 6400


def alternate(variants, warmup, repeats):
  """variants: {name: fn}.  Every round runs each variant once, in turn; one pair of device events per run."""
  for _ in range(warmup):
    for fn in variants.values():
      fn()
  torch.cuda.synchronize()
  ms = {name: [] for name in variants}
  for _ in range(repeats):
    for name, fn in variants.items():
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      fn()
      b.record()
      b.synchronize()
      ms[name].append(a.elapsed_time(b))
  return {name: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), repeats=len(v)) for name, v in ms.items()}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--repeats", type=int, default=25)
  ap.add_argument("--no-trainers", action="store_true")
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  out_path = os.path.abspath(args.out) if args.out else None  # (the trainer part changes the working directory)
  assert torch.cuda.is_available(), "a timing needs the GPU"
  from pointcontrast_amd import functional as PF
  dev = torch.device("cuda:0")
  rng = np.random.default_rng(0)
  results = []

  def report(name, **kw):
    rec = dict(name=name, **kw)
    results.append(rec)
    print(json.dumps(rec), flush=True)

  q = rng.standard_normal((N, C))
  q /= np.linalg.norm(q, axis=1, keepdims=True)
  k = q + 0.3 * rng.standard_normal((N, C))
  k /= np.linalg.norm(k, axis=1, keepdims=True)
  qd = torch.from_numpy(q.astype(np.float32)).to(dev).requires_grad_(True)
  kd = torch.from_numpy(k.astype(np.float32)).to(dev).requires_grad_(True)
  xyz = torch.from_numpy(np.stack([rng.integers(0, 160, N), rng.integers(0, 160, N), rng.integers(0, 100, N)], 1).astype(np.int32)).to(dev)
  scene = torch.from_numpy(rng.permutation(np.arange(N) % SCENES).astype(np.int32)).to(dev)

  def step(loss_of):
    def run():
      loss_of().backward()
      qd.grad = kd.grad = None
    return run

  variants = {"nce": step(lambda: PF.NCELossFunction.apply(qd, kd, T))}
  for A, E in ((1, 1), (2, 2), (8, 2)):
    variants["partition_P%d" % (2 * E * A)] = step(
        lambda A=A, E=E: PF.PartitionNCELossFunction.apply(qd, kd, xyz, scene, T, R1_SQ, R2_SQ, A, E, SCENES))
  live = {}
  for A, E in ((1, 1), (2, 2), (8, 2)):
    _, _, lv = PF.partition_nce_forward(qd, kd, xyz, scene, T, R1_SQ, R2_SQ, A, E, SCENES)
    live["partition_P%d" % (2 * E * A)] = int(lv.min())
  for name, t in alternate(variants, args.warmup, args.repeats).items():
    report("loss_fwd_bwd", variant=name, n=N, c=C, scenes=SCENES, min_live_rows=live.get(name), **t)

  if not args.no_trainers:
    import tempfile
    from pointcontrast_amd.lib import ddp_trainer
    from pointcontrast_amd.lib.config import get_config
    from pointcontrast_amd.lib.ddp_data_loaders import FixedBatchLoader, SyntheticScanNetPairDataset, default_collate_pair_fn
    from pointcontrast_amd.lib.timer import AverageMeter, Timer
    os.chdir(tempfile.mkdtemp())  # (a trainer looks for weights/ in the working directory)
    ds = SyntheticScanNetPairDataset(config=get_config([]), num_pairs=4)
    batch = default_collate_pair_fn([ds[i] for i in range(4)])
    steps, shapes = {}, None
    for name in ("PointNCELossTrainer", "PartitionPointNCELossTrainer"):
      cfg = get_config(["trainer.trainer=" + name, "misc.nceT=0.4", "net.model=Res16UNet34C"])
      torch.manual_seed(0)
      np.random.seed(0)
      tr = getattr(ddp_trainer, name)(cfg, FixedBatchLoader([batch], batch_size=4))
      timers = [AverageMeter(), Timer(), Timer()]
      steps[name] = lambda tr=tr, timers=timers: tr._train_iter(iter(tr.data_loader), timers)
      shapes = [int(batch["sinput0_C"].shape[0]), int(batch["sinput1_C"].shape[0])]
    for name, t in alternate(steps, args.warmup, args.repeats).items():
      report("train_step", trainer=name, model="Res16UNet34C", pairs=4, voxels=shapes, npos=4096, **t)
  if out_path:
    with open(out_path, "w") as f:
      json.dump(results, f, indent=1)


if __name__ == "__main__":
  main()
