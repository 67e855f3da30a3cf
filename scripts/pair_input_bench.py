"""What one pre-training batch costs to BUILD, at the shape of BASELINE configs[1]: 4 pairs of raw ScanNet-shaped frames (640x480
depth frames, ~300k points each, as the pair corpus writes them) at 2.5 cm, random scale and rotation on.  In one process:
  stages    the four entry points of csrc/pair_input.hip between device events (upload excluded), ms
  device    the whole PairInputPipeline call -- pack, one upload, the kernels, one read-back -- wall clock, ms
  host      ScanNetMatchPairDataset.__getitem__ x 4 + default_collate_pair_fn + the uploads the trainer makes (coordinates,
            features, correspondences), data.device_geometry off and on, wall clock, ms
The figure to hold the device call against is the training step it has to hide behind (13.7 ms for this batch).
--color: every raw point gets an RGB (as a corpus built with make_pair_corpus --color stores it); the whole call with 4-tuples
(the colours in the same upload) is timed beside the call without, and pcmi_pair_color_features as a stage of its own.
Usage: python scripts/pair_input_bench.py [repetitions] [--color]"""
import json
import os
import random
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pointcontrast_amd import functional as PF
from pointcontrast_amd.lib import synthetic
from pointcontrast_amd.lib.config import get_config
from pointcontrast_amd.lib.ddp_data_loaders import FeatureJitter, dataset_str_mapping, default_collate_pair_fn
from pointcontrast_amd.lib.pair_input import PairDraws, PairInputPipeline

color = "--color" in sys.argv[1:]
argv = [a for a in sys.argv[1:] if a != "--color"]
reps = int(argv[0]) if argv else 10
B, voxel, mult = 4, 0.025, 1.5
dev = torch.device("cuda", 0)
rng = np.random.RandomState(0)
frames = [synthetic.make_frame_pair(rng) for _ in range(B)]
n = sum(len(a) for f in frames for a in f)
print("frames: %d pairs, %d raw points" % (B, n), flush=True)

with tempfile.TemporaryDirectory() as root:
  lines = []
  for i, (a, b) in enumerate(frames):
    np.savez(os.path.join(root, "f%da.npz" % i), pcd=a)
    np.savez(os.path.join(root, "f%db.npz" % i), pcd=b)
    lines.append("f%da.npz f%db.npz 0.5\n" % (i, i))
  with open(os.path.join(root, "pairs.txt"), "w") as f:
    f.write("".join(lines))
  base = ["data.dataset=ScanNetMatchPairDataset", "data.dataset_root_dir=%s" % root, "data.scannet_match_dir=pairs.txt",
          "trainer.use_random_scale=True", "trainer.use_random_rotation=True"]
  cfg = get_config(base)
  out = {"pairs": B, "raw_points": n, "voxel_size": voxel, "repetitions": reps}

  # ---- the device pipeline: whole call ----
  gen = torch.Generator(device=dev)
  gen.manual_seed(0)
  randg = np.random.RandomState(0)
  pipe = PairInputPipeline(voxel, mult, device=dev)
  random.seed(0)
  batch = pipe(frames, PairDraws.sample(cfg, B, randg, gen))  # warm-up: allocator, staging buffer, match capacity
  batch = pipe(frames, PairDraws.sample(cfg, B, randg, gen))
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(reps):
    batch = pipe(frames, PairDraws.sample(cfg, B, randg, gen))
  torch.cuda.synchronize()
  out["device_call_ms"] = (time.perf_counter() - t0) / reps * 1e3
  out["voxels"] = [int(batch["sinput0_C"].shape[0]), int(batch["sinput1_C"].shape[0])]
  out["correspondences"] = int(batch["correspondences"].shape[0])
  print("device    %8.2f ms per batch (%d + %d voxels, %d correspondences, %d read-back)" %
        (out["device_call_ms"], out["voxels"][0], out["voxels"][1], out["correspondences"], pipe.last_readbacks), flush=True)
  if color:
    frames4 = [(a, b, rng.randint(0, 256, a.shape).astype(np.uint8), rng.randint(0, 256, b.shape).astype(np.uint8)) for a, b in frames]
    saved = (random.getstate(), randg.get_state(), gen.get_state())  # the legs below see the draws they see without --color
    for _ in range(2):
      batch = pipe(frames4, PairDraws.sample(cfg, B, randg, gen))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
      batch = pipe(frames4, PairDraws.sample(cfg, B, randg, gen))
    torch.cuda.synchronize()
    out["device_call_color_ms"] = round((time.perf_counter() - t0) / reps * 1e3, 3)
    print("device    %8.2f ms per batch with colours (%d read-back)" % (out["device_call_color_ms"], pipe.last_readbacks), flush=True)
    random.setstate(saved[0])
    randg.set_state(saved[1])
    gen.set_state(saved[2])

  # ---- the stages between device events ----
  d = PairDraws.sample(cfg, B, randg, gen)
  raw = torch.from_numpy(np.concatenate([a for f in frames for a in f])).to(dev)
  offs = torch.from_numpy(np.concatenate([[0], np.cumsum([len(a) for f in frames for a in f])]).astype(np.int64)).to(dev)
  scale, rot = torch.from_numpy(d.scale).to(dev), torch.from_numpy(d.rot).to(dev)
  radius = torch.from_numpy(np.float64(voxel * mult) * d.scale).to(dev)
  on = torch.from_numpy(d.jitter_on.astype(np.int32)).to(dev)
  cap = int(out["correspondences"] * 1.25) + 1024
  acc = {k: 0.0 for k in ("noise", "transform", "voxelize", "match", "collate") + (("color_features",) if color else ())}
  rgb = torch.from_numpy(np.concatenate([c for f in frames4 for c in f[2:]])).to(dev) if color else None
  for it in range(reps + 1):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(acc) + 1)]
    flags = torch.zeros(B, dtype=torch.int32, device=dev)
    ev[0].record()
    noise = torch.randn((n, 3), generator=gen, dtype=torch.float32, device=dev)
    ev[1].record()
    tf = PF.pair_transform(raw, offs, scale, rot, flags)
    ev[2].record()
    vx = PF.pair_voxelize(tf["points"], offs, voxel, flags)
    ev[3].record()
    mt = PF.pair_match(vx, tf["trans"], radius, cap, flags)
    ev[4].record()
    co = PF.pair_collate(vx, tf["trans"], noise, on, 0.0, 0.01)
    ev[5].record()
    if color:
      PF.pair_color_features(rgb, vx, co, noise, on, 0.0, 0.01)
      ev[6].record()
    torch.cuda.synchronize()
    if it:  # (the first round warms up)
      for k, name in enumerate(acc):
        acc[name] += ev[k].elapsed_time(ev[k + 1]) / reps
  assert not int(flags.any()) and not int(mt["totals"][2])
  out["stage_ms"] = {k: round(v, 3) for k, v in acc.items()}
  print("stages    " + ", ".join("%s %.3f ms" % kv for kv in out["stage_ms"].items()) +
        "  (sum %.3f ms)" % sum(out["stage_ms"].values()), flush=True)

  # ---- the host loader: items, collate, the trainer's uploads ----
  for name, devgeo in (("host_ms", False), ("host_device_geometry_ms", True)):
    c = get_config(base + ["data.device_geometry=%s" % devgeo, "misc.train_num_thread=0"])
    dset = dataset_str_mapping["ScanNetMatchPairDataset"](phase="train", transform=FeatureJitter(), random_scale=True, random_rotation=True,
                                                         manual_seed=True, config=c)
    n_host = max(1, min(reps, 3))
    for it in range(n_host + 1):
      if it == 1:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
      hb = default_collate_pair_fn([dset[i] for i in range(B)])
      up = [hb[k].to(dev) for k in ("sinput0_C", "sinput0_F", "sinput1_C", "sinput1_F", "correspondences")]
      torch.cuda.synchronize()
    out[name] = (time.perf_counter() - t0) / n_host * 1e3
    print("%-24s %8.2f ms per batch (%d correspondences)" % (name, out[name], hb["correspondences"].shape[0]), flush=True)

out["device_call_ms"] = round(out["device_call_ms"], 3)
out["host_ms"], out["host_device_geometry_ms"] = round(out["host_ms"], 2), round(out["host_device_geometry_ms"], 2)
print(json.dumps(out))
