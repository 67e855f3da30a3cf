"""Digest of three training iterations through the network executor, one JSON line per configuration: the losses as hex
floats, a sha256 each of the flat weights, the momentum buffer and the BatchNorm buffers and, under time_all, the launch
counts of set 1.  Two builds of the library (PCMI_LIB=<other libpcmi.so>) that enqueue the same work print the same lines,
byte for byte -- the check for a change to csrc/engine.hip that must not change what a step computes.  The trainer is that
of tests/test_gpu_timing.py (Res16UNet34C, 2 synthetic pairs, crop 0.9, seed 3, injected draws).

  python scripts/engine_step_digest.py > new.txt; PCMI_LIB=/path/to/old/libpcmi.so python scripts/engine_step_digest.py > old.txt"""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

SWITCHES = ("PCMI_FWD_BRANCH", "PCMI_X3_PACK_SIDE", "PCMI_X3_PREPACK")
CONFIGS = [("defaults", [], None, False), ("two_passes", ["misc.joint_pair=False"], None, False)] + \
          [("%s=0" % s, [], s, False) for s in SWITCHES] + [("time_all", [], None, True)]


def sha(t):
  return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def run(name, extra, switch_off, timed, seed=3, pairs=2, crop=0.9, steps=3):
  from pointcontrast_amd.lib import synthetic
  from pointcontrast_amd.lib.config import get_config
  from pointcontrast_amd.lib.ddp_data_loaders import FixedBatchLoader, default_collate_pair_fn
  from pointcontrast_amd.lib.ddp_trainer import PointNCELossTrainer
  from pointcontrast_amd.lib.timer import AverageMeter, Timer
  for s in SWITCHES:  # read per pass by the executor
    os.environ.pop(s, None)
  if switch_off:
    os.environ[switch_off] = "0"
  cfg = get_config(["net.model=Res16UNet34C", "misc.nceT=0.4", "misc.npos=512", "opt.lr=0.1", "misc.engine=native"] + extra)
  rng = np.random.RandomState(seed)
  batch = default_collate_pair_fn([synthetic.make_pair_item(rng, 0.025, crop=crop) for _ in range(pairs)])
  loader = FixedBatchLoader([batch], batch_size=pairs)
  torch.manual_seed(seed)
  trainer = PointNCELossTrainer(cfg, loader)
  if timed:
    trainer.engine.time_all(steps)
  nq = len(np.unique(batch["correspondences"].numpy()[:, 0]))
  it, timers, losses = iter(loader), [AverageMeter(), Timer(), Timer()], []
  for step in range(steps):
    draws = dict(uniform=torch.rand(nq, generator=torch.Generator().manual_seed(step)),
                 sampled_inds=np.random.RandomState(step).choice(nq, min(512, nq), replace=False))
    losses.append(float(trainer._train_iter(it, timers, draws=draws)["loss"]).hex())
  torch.cuda.synchronize()
  out = dict(config=name, losses=losses, weights=sha(trainer.flat.w), momentum=sha(trainer.flat.v),
             bn_buffers=sha(torch.cat([b.detach().flatten().float() for b in trainer.model.buffers()])))
  if timed:
    fwd, bwd, wgrad, groups = trainer.engine.timed_launches(steps)[1]
    out.update(fwd_launches=list(map(int, fwd)), bwd_launches=list(map(int, bwd)), wgrad_launches=list(map(int, wgrad)),
               group_launches=list(map(int, groups)))
    trainer.engine.time_all(0)
  return out


if __name__ == "__main__":
  assert torch.cuda.is_available(), "engine_step_digest.py needs the GPU"
  for cfg in CONFIGS:
    print(json.dumps(run(*cfg), sort_keys=True), flush=True)
