"""Times the point-set ops of csrc/pointset.hip against the same algorithms written in torch ops on the same GPU -- what a
user of the library would have written without them (the reference's extension is CUDA and does not run here):
furthest point sampling as an m-step loop of distance / minimum / argmax, ball query as cdist + masked top-k, the grouping
backward as index_add_.  Median of repeated launches after warm-up, device events; one JSON line per (shape, op).

  python scripts/pointset_bench.py [--warmup 2] [--repeats 7] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [  # name, B, n, m (centres), nsample, radius, channels
    ("votenet_seeds", 8, 40000, 1024, 0, 0.0, 0),
    ("proposal", 8, 1024, 256, 16, 0.3, 128),
    ("set_abstraction", 8, 20000, 2048, 64, 0.2, 64),
]


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
  return statistics.median(ms), min(ms), max(ms)


def fps_torch(xyz, m):
  B, n, _ = xyz.shape
  ok = (xyz * xyz).sum(-1) > 1e-3
  mind = torch.full((B, n), 1e10, device=xyz.device)
  idx = torch.zeros((B, m), dtype=torch.int64, device=xyz.device)
  far = torch.zeros(B, dtype=torch.int64, device=xyz.device)
  ar = torch.arange(B, device=xyz.device)
  for j in range(1, m):
    d = ((xyz - xyz[ar, far].unsqueeze(1)) ** 2).sum(-1)
    mind = torch.where(ok, torch.minimum(mind, d), mind)
    far = torch.where(ok, mind, mind.new_tensor(-1.0)).argmax(1)
    idx[:, j] = far
  return idx


def ball_query_torch(radius, nsample, xyz, new_xyz):
  n = xyz.shape[1]
  hit = torch.cdist(new_xyz, xyz) ** 2 < radius * radius  # [B, np, n]
  key = torch.where(hit, torch.arange(n, device=xyz.device), n)
  idx = key.topk(nsample, dim=-1, largest=False, sorted=True).values
  first = torch.where(idx[..., :1] == n, 0, idx[..., :1])
  return torch.where(idx == n, first, idx)


def group_bwd_torch(gout, idx, N):
  B, C = gout.shape[:2]
  flat = (idx.long() + (torch.arange(B, device=idx.device) * N).view(B, 1, 1)).reshape(-1)
  g = torch.zeros((B * N, C), device=gout.device)
  g.index_add_(0, flat, gout.permute(0, 2, 3, 1).reshape(-1, C))
  return g.view(B, N, C).permute(0, 2, 1)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--warmup", type=int, default=2)
  ap.add_argument("--repeats", type=int, default=7)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), "pointset_bench needs the GPU: a timing taken elsewhere says nothing"
  from pointcontrast_amd import pointnet2_utils as P
  dev = torch.device("cuda:0")
  rows = []

  def report(shape, op, native, torch_fn):
    nat = timed(native, args.warmup, args.repeats)
    ref = timed(torch_fn, args.warmup, args.repeats) if torch_fn is not None else (None, None, None)
    row = dict(shape=shape, op=op, native_ms=round(nat[0], 4), native_min_ms=round(nat[1], 4), native_max_ms=round(nat[2], 4),
               torch_ms=None if ref[0] is None else round(ref[0], 4), torch_min_ms=None if ref[1] is None else round(ref[1], 4),
               torch_max_ms=None if ref[2] is None else round(ref[2], 4))
    rows.append(row)
    print(json.dumps(row), flush=True)

  for name, B, n, m, nsample, radius, C in SHAPES:
    g = torch.Generator(device="cpu").manual_seed(0)
    xyz = (torch.rand(B, n, 3, generator=g) + 0.5).to(dev)
    report(name, "fps", lambda: P.furthest_point_sample(xyz, m), lambda: fps_torch(xyz, m))
    same = bool((P.furthest_point_sample(xyz, m).long() == fps_torch(xyz, m)).all())
    print(json.dumps(dict(shape=name, op="fps", picks_equal_torch_loop=same)), flush=True)
    if nsample == 0:
      continue
    sel = P.furthest_point_sample(xyz, m).long()
    new_xyz = torch.gather(xyz, 1, sel.unsqueeze(-1).expand(B, m, 3)).contiguous()
    report(name, "ball_query", lambda: P.ball_query(radius, nsample, xyz, new_xyz), lambda: ball_query_torch(radius, nsample, xyz, new_xyz))
    idx = P.ball_query(radius, nsample, xyz, new_xyz)
    feat = torch.randn(B, C, n, device=dev)
    gout = torch.randn(B, C, m, nsample, device=dev)
    il = idx.long()
    report(name, "group_fwd", lambda: P.grouping_operation(feat, idx),
           lambda: torch.gather(feat, 2, il.view(B, 1, -1).expand(B, C, m * nsample)).view(B, C, m, nsample))
    f = feat.clone().requires_grad_(True)
    out = P.grouping_operation(f, idx)
    report(name, "group_bwd", lambda: torch.autograd.grad(out, f, gout, retain_graph=True), lambda: group_bwd_torch(gout, idx, n))
    dist, i3 = P.three_nn(xyz, new_xyz)
    w = 1.0 / (dist + 1e-8)
    w = w / w.sum(-1, keepdim=True)
    fm = torch.randn(B, C, m, device=dev)
    report(name, "three_nn", lambda: P.three_nn(xyz, new_xyz), lambda: (torch.cdist(xyz, new_xyz) ** 2).topk(3, dim=-1, largest=False))
    i3l = i3.long()
    report(name, "three_interpolate_fwd", lambda: P.three_interpolate(fm, i3, w),
           lambda: (torch.gather(fm, 2, i3l.view(B, 1, -1).expand(B, C, n * 3)).view(B, C, n, 3) * w.unsqueeze(1)).sum(-1))
  if args.out:
    with open(args.out, "w") as fh:
      json.dump(rows, fh, indent=1)


if __name__ == "__main__":
  main()
