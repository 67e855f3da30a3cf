"""Times VoteNet's PointNet++ backbone on rows (pointcontrast_amd.downstream.votenet.Pointnet2Backbone, csrc/rowspool.hip):
  (a) the fused BatchNorm + ReLU + max-pool (BatchNormMaxPoolFunction), forward + backward, against the composition
      BatchNormFunction(relu) + RowsMaxPoolFunction on the same tensors, at the last-layer shapes of the four set-abstraction
      levels at batch size 8.  The bytes the fused algorithm needs are computed from the shapes (x read three times, dx written
      once, the pooled tensors); reported: achieved bytes/s and the share of the HBM peak.  GATE (exit status 1 otherwise): the
      fused path must beat the composition by more than the run-to-run spread measured here.  The four shapes run together in
      every step of the backbone and one flag (fused_pool) switches them together, so the gate is on the four together: the sum
      of the median differences must exceed the sum of the spreads, a shape's spread being the larger of its two variants'
      (slowest - fastest window).  Each shape's own verdict is reported beside it (fused_wins_beyond_spread).
  (b) the backbone, forward + backward, at B = 8 with N = 40000 (the ScanNet recipe) and N = 20000 (SUN RGB-D), one extra
      feature column, against the same network restated channel-first in torch ops -- Conv2d / BatchNorm2d / max_pool2d over
      pointcontrast_amd.pointnet2_utils, the way the reference's model code spells it -- with the same parameters;
  (c) DetectionTrainer.train_iter with each backbone on the same synthetic batch.
Device events; every shape is warmed up; median of 7 windows of about 250 ms; the variants of a comparison alternate inside one
process.  One JSON
line per measurement.

  python scripts/pointnet2_backbone_bench.py [--parts abc] [--warmup 2] [--repeats 7] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12  # bytes/s, the MI355X's HBM3E specification (a float4 copy reaches 6.29e12)
B = 8
# (R ns, ns, C): the last SharedMLP layer of sa1 .. sa4 at B = 8
POOL_SHAPES = ((1048576, 64, 128), (262144, 32, 256), (65536, 16, 256), (32768, 16, 256))
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def window(fn, inner):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  for _ in range(inner):
    fn()
  b.record()
  b.synchronize()
  return a.elapsed_time(b) / inner


WINDOW_MS = 250.0  # a timed window repeats its call until it is about this long: a shorter one measures the clock and the host


def alternated(variants, warmup, repeats):
  """variants: {name: fn}.  Every variant is warmed up, then the variants take turns, `repeats` windows each; a window is
  `calls_per_window` calls (the same number for every variant, from the slowest one's warm time).  Returns
  {name: dict(median_ms, min_ms, max_ms per call, spread = (max - min) / median), "calls_per_window": n}."""
  for fn in variants.values():
    for _ in range(warmup):
      fn()
  torch.cuda.synchronize()
  slowest = max(window(fn, 2) for fn in variants.values())
  inner = max(1, min(4096, int(WINDOW_MS / slowest)))
  ms = {k: [] for k in variants}
  for _ in range(repeats):
    for k, fn in variants.items():
      ms[k].append(window(fn, inner))
  out = {}
  for k, v in ms.items():
    med = statistics.median(v)
    out[k] = dict(median_ms=med, min_ms=min(v), max_ms=max(v), spread=(max(v) - min(v)) / med)
  out["calls_per_window"] = inner
  return out


def fused_pool_bytes(n, ns, C):
  """Bytes the fused algorithm needs, forward + backward: x three times and dx once ([n, C] fp32); out written and read twice,
  gout read twice ([n / ns, C] fp32); the argument rows written and read twice (uint8)."""
  R = n // ns
  return 4 * n * C * 4 + 5 * R * C * 4 + 3 * R * C


def part_a(args, report):
  from pointcontrast_amd import functional as PF
  dev = torch.device("cuda:0")
  gain = spread = 0.0
  verdicts = []
  for n, ns, C in POOL_SHAPES:
    g = torch.Generator(device=dev).manual_seed(n + C)
    x = torch.randn(n, C, device=dev, generator=g).requires_grad_(True)
    gamma = (torch.rand(C, device=dev, generator=g) + 0.5).requires_grad_(True)
    beta = (torch.randn(C, device=dev, generator=g) * 0.3).requires_grad_(True)
    gout = torch.randn(n // ns, C, device=dev, generator=g)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)

    def fused(want_arg=False):
      out, arg = PF.BatchNormMaxPoolFunction.apply(x, gamma, beta, rm, rv, BN_MOMENTUM, BN_EPS, ns)
      grads = torch.autograd.grad(out, [x, gamma, beta], gout)
      return (grads, out.detach(), arg) if want_arg else grads

    def composed(want_arg=False):
      y = PF.BatchNormFunction.apply(x, gamma, beta, rm, rv, BN_MOMENTUM, BN_EPS, None, True)
      out = PF.RowsMaxPoolFunction.apply(y, ns)
      grads = torch.autograd.grad(out, [x, gamma, beta], gout)
      return (grads, out.detach(), PF.rows_maxpool(y.detach(), ns)[1]) if want_arg else grads

    # Faster and different is not faster: the two agree at the size that is timed.  The two paths round y differently, so
    # among millions of windows a few pick another row where two values lie within rounding of each other; dx moves by
    # a whole gout there (a decision, not an error), so dx is compared on the windows whose rows agree and the others are counted.
    (ga, oa, aa), (gb, ob, ab) = fused(True), composed(True)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())  # noqa: E731
    same = (aa == ab).reshape(n // ns, 1, C).expand(n // ns, ns, C).reshape(n, C)
    err = dict(out=rel(oa, ob), dgamma=rel(ga[1], gb[1]), dbeta=rel(ga[2], gb[2]),
               dx_where_rows_agree=float(((ga[0] - gb[0]).abs() * same).max() / gb[0].abs().max()),
               windows_with_another_row=int((aa != ab).sum()), windows=int(aa.numel()))
    t = alternated(dict(fused=fused, composed=composed), args.warmup, args.repeats)
    need = fused_pool_bytes(n, ns, C)
    rate = need / (t["fused"]["median_ms"] * 1e-3)
    noise = max(t["fused"]["max_ms"] - t["fused"]["min_ms"], t["composed"]["max_ms"] - t["composed"]["min_ms"])
    wins = t["composed"]["median_ms"] - t["fused"]["median_ms"] > noise
    gain += t["composed"]["median_ms"] - t["fused"]["median_ms"]
    spread += noise
    verdicts.append(wins)
    report("bn_maxpool_fwd_bwd", shape=dict(rows=n, ns=ns, C=C), fused=t["fused"], composed=t["composed"],
           speedup=t["composed"]["median_ms"] / t["fused"]["median_ms"], bytes_needed=need, fused_bytes_per_s=rate,
           fused_share_of_hbm_peak=rate / HBM_PEAK, agreement=err, calls_per_window=t["calls_per_window"], fused_wins_beyond_spread=wins)
    del x, gout, ga, gb, oa, ob, aa, ab, same
  report("bn_maxpool_gate", fused_gain_ms=gain, spread_ms=spread, per_shape=verdicts, fused_wins_beyond_spread=gain > spread)
  return gain > spread


class ChannelFirstBackbone(nn.Module):
  """Pointnet2Backbone as the reference's model code spells it: channel-first tensors through torch's Conv2d / BatchNorm2d /
  max_pool2d and this package's drop-in pointnet2_utils.  Built from a native backbone's state dict."""

  def __init__(self, native):
    super().__init__()
    self.cfg = [(getattr(native, "sa%d" % k).npoint, getattr(native, "sa%d" % k).radius, getattr(native, "sa%d" % k).nsample) for k in (1, 2, 3, 4)]
    sd = native.state_dict()
    self.convs, self.bns = nn.ModuleDict(), nn.ModuleDict()
    for k in sd:
      if k.endswith(".conv.weight"):
        key = k[:-len(".conv.weight")].replace(".", "_")
        cout, cin = sd[k].shape[:2]
        self.convs[key] = nn.Conv2d(cin, cout, 1, bias=False)
        self.bns[key] = nn.BatchNorm2d(cout)
        self.convs[key].load_state_dict({"weight": sd[k]})
        prefix = k[:-len(".conv.weight")] + ".bn.bn."
        self.bns[key].load_state_dict({n[len(prefix):]: v for n, v in sd.items() if n.startswith(prefix)})

  def _mlp(self, x, prefix):
    i = 0
    while "%s_layer%d" % (prefix, i) in self.convs:
      key = "%s_layer%d" % (prefix, i)
      x = F.relu(self.bns[key](self.convs[key](x)))
      i += 1
    return x

  def _sa(self, k, xyz, features):
    from pointcontrast_amd import pointnet2_utils as pu
    npoint, radius, ns = self.cfg[k - 1]
    xyz_t = xyz.transpose(1, 2).contiguous()
    inds = pu.furthest_point_sample(xyz, npoint)
    new_xyz = pu.gather_operation(xyz_t, inds).transpose(1, 2).contiguous()
    idx = pu.ball_query(radius, ns, xyz, new_xyz)
    grouped = (pu.grouping_operation(xyz_t, idx) - new_xyz.transpose(1, 2).unsqueeze(-1)) / radius
    if features is not None:
      grouped = torch.cat([grouped, pu.grouping_operation(features, idx)], dim=1)
    x = self._mlp(grouped, "sa%d_mlp_module" % k)
    return new_xyz, F.max_pool2d(x, kernel_size=[1, x.size(3)]).squeeze(-1)

  def _fp(self, k, unknown, known, unknown_feats, known_feats):
    from pointcontrast_amd import pointnet2_utils as pu
    dist, idx = pu.three_nn(unknown, known)
    r = 1.0 / (dist + 1e-8)
    x = torch.cat([pu.three_interpolate(known_feats, idx, r / torch.sum(r, dim=2, keepdim=True)), unknown_feats], dim=1)
    return self._mlp(x.unsqueeze(-1), "fp%d_mlp" % k).squeeze(-1)

  def forward(self, pc):
    xyz = pc[..., 0:3].contiguous()
    features = pc[..., 3:].transpose(1, 2).contiguous() if pc.size(-1) > 3 else None
    lv = []
    for k in (1, 2, 3, 4):
      xyz, features = self._sa(k, xyz, features)
      lv.append((xyz, features))
    f = self._fp(1, lv[2][0], lv[3][0], lv[2][1], lv[3][1])
    return self._fp(2, lv[1][0], lv[2][0], lv[1][1], f)


def synthetic_cloud(rng, n_scenes, n_points, n_feat):
  """Points on the objects of a room of 8 m x 8 m x 2.4 m, as the step benchmark's scans."""
  out = np.zeros((n_scenes, n_points, 3 + n_feat), np.float32)
  for b in range(n_scenes):
    ins = rng.randint(0, 30, n_points)
    cen = rng.uniform(0.5, 7.5, (30, 3)) * np.array([1.0, 1.0, 0.3])
    out[b, :, 0:3] = cen[ins] + rng.uniform(-0.6, 0.6, (n_points, 3))
    out[b, :, 3:] = rng.uniform(0, 2.4, (n_points, n_feat))
  return out


def part_b(args, report):
  from pointcontrast_amd.downstream import votenet
  dev = torch.device("cuda:0")
  rng = np.random.RandomState(0)
  torch.manual_seed(0)
  for n_points in (40000, 20000):
    native = votenet.Pointnet2Backbone(input_feature_dim=1).to(dev).train()
    composed = votenet.Pointnet2Backbone(input_feature_dim=1, fused_pool=False).to(dev).train()
    composed.load_state_dict(native.state_dict())
    ref = ChannelFirstBackbone(native).to(dev).train()
    pc = torch.from_numpy(synthetic_cloud(rng, B, n_points, 1)).to(dev)
    nat_params, cmp_params, ref_params = list(native.parameters()), list(composed.parameters()), list(ref.parameters())

    def rows(net, params):
      def fn():
        ep = net(pc)
        torch.autograd.grad(ep["fp2_features"].sum(), params)
        return ep["fp2_features"]
      return fn

    def channel_first():
      out = ref(pc)
      torch.autograd.grad(out.sum(), ref_params)
      return out

    with torch.no_grad():
      want = ref(pc)
      err = float((native(pc)["fp2_features"] - want).abs().max() / want.abs().max())
    t = alternated(dict(rows=rows(native, nat_params), rows_composed_pool=rows(composed, cmp_params), channel_first_torch=channel_first),
                   args.warmup, args.repeats)
    report("backbone_fwd_bwd", shape=dict(B=B, N=n_points, F=1), **t, speedup=t["channel_first_torch"]["median_ms"] / t["rows"]["median_ms"],
           fused_pool_speedup=t["rows_composed_pool"]["median_ms"] / t["rows"]["median_ms"], largest_relative_difference=err)
    del native, composed, ref


def part_c(args, report):
  from pointcontrast_amd.downstream import votenet
  import votenet_fixtures as VF
  from votenet_step_bench import synthetic_scans
  dev = torch.device("cuda:0")
  rng = np.random.RandomState(0)
  torch.manual_seed(0)
  msa = rng.uniform(0.4, 1.5, (18, 3)).astype(np.float32)
  dc = VF.DatasetConfig(1, msa, 18, True)
  pipe = votenet.DetectionInputPipeline("scannet", 40000, 0.025, dev, mean_size_arr=msa)
  scans = synthetic_scans(rng, B, 50000)
  batch = pipe(scans, votenet.DetectionDraws.sample([len(s[0]) for s in scans], 40000, "scannet", 1))
  trainers = {name: votenet.DetectionTrainer(dc, num_proposal=256, backbone=name, device=dev) for name in ("pointnet2", "sparseconv")}
  t = alternated({name: (lambda tr=tr: tr.train_iter(batch)) for name, tr in trainers.items()}, args.warmup, args.repeats)
  report("train_iter", shape=dict(B=B, N=40000, num_proposal=256), voxels=int(batch["voxel_coords"].shape[0]), **t)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--parts", default="abc")
  ap.add_argument("--warmup", type=int, default=2)
  ap.add_argument("--repeats", type=int, default=7)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), "the measurements are taken on the GPU (no CPU path)"
  results = []

  def report(name, **kw):
    rec = dict(name=name, **kw)
    results.append(rec)
    print(json.dumps(rec), flush=True)
    if args.out:
      with open(args.out, "w") as f:
        json.dump(results, f, indent=1)

  ok = True
  if "a" in args.parts:
    ok = part_a(args, report)
  if "b" in args.parts:
    part_b(args, report)
  if "c" in args.parts:
    part_c(args, report)
  sys.exit(0 if ok else 1)


if __name__ == "__main__":
  sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
  main()
