"""Times the VoteNet head and the detection training step at the ScanNet recipe's shape (downstream/votenet_det_new of the
reference: batch_size 8, 40000 points, 1024 seeds, 256 proposals, nsample 16, vote_factor 1, 1 heading bin, 18 size clusters,
18 classes):
  * the head, forward + backward, on rows (pointcontrast_amd.downstream.votenet.VoteNet.forward_head: the dense GEMM, the fused
    BatchNorm + ReLU and csrc/votehead.hip) against the same head restated channel-first in torch ops -- Conv1d / Conv2d /
    BatchNorm1d / BatchNorm2d / max_pool2d over pointcontrast_amd.pointnet2_utils, the way the reference's model code spells
    it -- on the same GPU, with the same parameters;
  * the whole step (DetectionTrainer.train_iter: backbone under the native executor, head, loss, backward, Adam) and the
    backbone's share of it (the executor's forward + backward alone on the same batch).
Median of 7 after 2 warm-ups, device events, one process; one JSON line per measurement.

  python scripts/votenet_step_bench.py [--warmup 2] [--repeats 7] [--out FILE]
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

B, NUM_POINTS, NUM_SEED, NUM_PROPOSAL, NSAMPLE, C, H, S, CLS = 8, 40000, 1024, 256, 16, 256, 1, 18, 18
RADIUS, VOXEL = 0.3, 0.025


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


class ChannelFirstHead(nn.Module):
  """The head as the reference's model code spells it: channel-first [B, C, N] tensors through torch's Conv1d / Conv2d /
  BatchNorm and this package's drop-in pointnet2_utils.  Built from a native VoteNet's state dict."""

  def __init__(self, nout):
    super().__init__()
    self.v1, self.v2, self.v3 = nn.Conv1d(C, C, 1), nn.Conv1d(C, C, 1), nn.Conv1d(C, 3 + C, 1)
    self.vb1, self.vb2 = nn.BatchNorm1d(C), nn.BatchNorm1d(C)
    dims = (C + 3, 128, 128, 128)
    self.mlp = nn.ModuleList([nn.Conv2d(dims[i], dims[i + 1], 1, bias=False) for i in range(3)])
    self.mbn = nn.ModuleList([nn.BatchNorm2d(d) for d in dims[1:]])
    self.p1, self.p2, self.p3 = nn.Conv1d(128, 128, 1), nn.Conv1d(128, 128, 1), nn.Conv1d(128, nout, 1)
    self.pb1, self.pb2 = nn.BatchNorm1d(128), nn.BatchNorm1d(128)

  def load_reference(self, sd):
    pairs = [("vgen.conv1", self.v1), ("vgen.conv2", self.v2), ("vgen.conv3", self.v3), ("vgen.bn1", self.vb1), ("vgen.bn2", self.vb2),
             ("pnet.conv1", self.p1), ("pnet.conv2", self.p2), ("pnet.conv3", self.p3), ("pnet.bn1", self.pb1), ("pnet.bn2", self.pb2)]
    for i in range(3):
      pairs += [("pnet.vote_aggregation.mlp_module.layer%d.conv" % i, self.mlp[i]),
                ("pnet.vote_aggregation.mlp_module.layer%d.bn.bn" % i, self.mbn[i])]
    for prefix, mod in pairs:
      mod.load_state_dict({k[len(prefix) + 1:]: v for k, v in sd.items() if k.startswith(prefix + ".")})

  def forward(self, seed_xyz, seed_features):
    from pointcontrast_amd import pointnet2_utils as pu
    Bn, _, N = seed_features.shape
    net = F.relu(self.vb1(self.v1(seed_features)))
    net = F.relu(self.vb2(self.v2(net)))
    net = self.v3(net).transpose(2, 1).view(Bn, N, 1, 3 + C)
    vote_xyz = (seed_xyz.unsqueeze(2) + net[:, :, :, 0:3]).contiguous().view(Bn, N, 3)
    feats = (seed_features.transpose(2, 1).unsqueeze(2) + net[:, :, :, 3:]).contiguous().view(Bn, N, C).transpose(2, 1).contiguous()
    feats = feats.div(torch.norm(feats, p=2, dim=1).unsqueeze(1))
    inds = pu.furthest_point_sample(vote_xyz, NUM_PROPOSAL)
    new_xyz = pu.gather_operation(vote_xyz.transpose(1, 2).contiguous(), inds).transpose(1, 2).contiguous()
    idx = pu.ball_query(RADIUS, NSAMPLE, vote_xyz, new_xyz)
    grouped_xyz = pu.grouping_operation(vote_xyz.transpose(1, 2).contiguous(), idx) - new_xyz.transpose(1, 2).unsqueeze(-1)
    x = torch.cat([grouped_xyz / RADIUS, pu.grouping_operation(feats, idx)], dim=1)
    for conv, bn in zip(self.mlp, self.mbn):
      x = F.relu(bn(conv(x)))
    x = F.max_pool2d(x, kernel_size=[1, x.size(3)]).squeeze(-1)
    net = F.relu(self.pb1(self.p1(x)))
    net = F.relu(self.pb2(self.p2(net)))
    return vote_xyz, feats, new_xyz, self.p3(net).transpose(2, 1)


def synthetic_scans(rng, n_scenes, n_vertices):
  from pointcontrast_amd.downstream.votenet import SCANNET_NYU40IDS
  out = []
  for _ in range(n_scenes):
    ins = rng.randint(0, 30, n_vertices)
    cen = rng.uniform(0.5, 7.5, (30, 3)) * np.array([1.0, 1.0, 0.3])
    xyz = (cen[ins] + rng.uniform(-0.6, 0.6, (n_vertices, 3))).astype(np.float32)
    sem = rng.choice(SCANNET_NYU40IDS, 30)[ins]
    boxes = np.concatenate([rng.uniform(0.5, 7.5, (20, 3)) * np.array([1.0, 1.0, 0.3]), rng.uniform(0.3, 1.5, (20, 3)),
                            rng.choice(SCANNET_NYU40IDS, (20, 1))], 1)
    out.append((xyz, ins, sem, boxes))
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--warmup", type=int, default=2)
  ap.add_argument("--repeats", type=int, default=7)
  ap.add_argument("--vertices", type=int, default=50000, help="vertices of every synthetic scan")
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  from pointcontrast_amd.downstream import votenet
  import votenet_fixtures as VF
  dev = torch.device("cuda:0")
  rng = np.random.RandomState(0)
  torch.manual_seed(0)
  results = []

  def report(name, **kw):
    rec = dict(name=name, **kw)
    results.append(rec)
    print(json.dumps(rec), flush=True)

  msa = rng.uniform(0.4, 1.5, (S, 3)).astype(np.float32)
  dc = VF.DatasetConfig(H, msa, CLS, True)
  pipe = votenet.DetectionInputPipeline("scannet", NUM_POINTS, VOXEL, dev, mean_size_arr=msa)
  trainer = votenet.DetectionTrainer(dc, num_proposal=NUM_PROPOSAL, num_seed=NUM_SEED, input_pipeline=pipe, device=dev)
  model = trainer.model
  model.train()

  # ---- the head alone, forward + backward, on the same seeds and parameters ----
  seed_xyz = torch.from_numpy(rng.uniform(0.5, 7.5, (B, NUM_SEED, 3)).astype(np.float32) * np.array([1, 1, 0.3], np.float32)).to(dev)
  seed_rows = torch.randn(B * NUM_SEED, C, device=dev)
  nout = 2 + 3 + 2 * H + 4 * S + CLS
  ref = ChannelFirstHead(nout).to(dev)
  ref.load_reference({k: v for k, v in model.state_dict().items() if k.startswith(("vgen.", "pnet."))})
  ref.train()
  head_params = model.head_parameters()

  def native():
    sx, rows = seed_xyz.clone().requires_grad_(True), seed_rows.clone().requires_grad_(True)
    ep = model.forward_head(sx, rows)
    total = ep["vote_xyz"].sum() + ep["vote_features"].sum() + ep["center"].sum() + ep["objectness_scores"].sum() + \
        ep["heading_scores"].sum() + ep["size_scores"].sum() + ep["size_residuals_normalized"].sum() + ep["sem_cls_scores"].sum()
    torch.autograd.grad(total, [sx, rows] + head_params, allow_unused=True)

  feats_cf = seed_rows.reshape(B, NUM_SEED, C).transpose(1, 2).contiguous()
  ref_params = list(ref.parameters())

  def channel_first():
    sx, sf = seed_xyz.clone().requires_grad_(True), feats_cf.clone().requires_grad_(True)
    vote_xyz, feats, new_xyz, net = ref(sx, sf)
    total = vote_xyz.sum() + feats.sum() + new_xyz.sum() + net.sum()
    torch.autograd.grad(total, [sx, sf] + ref_params, allow_unused=True)

  ours, theirs = timed(native, args.warmup, args.repeats), timed(channel_first, args.warmup, args.repeats)
  report("head_fwd_bwd", shape=dict(B=B, num_seed=NUM_SEED, num_proposal=NUM_PROPOSAL, nsample=NSAMPLE, C=C), rows=ours,
         channel_first_torch=theirs, speedup=theirs["median_ms"] / ours["median_ms"])

  # ---- the whole step and the backbone's share ----
  scans = synthetic_scans(rng, B, args.vertices)
  batch = pipe(scans, votenet.DetectionDraws.sample([len(s[0]) for s in scans], NUM_POINTS, "scannet", 1))
  step = timed(lambda: trainer.train_iter(batch), args.warmup, args.repeats)
  import pointcontrast_amd.minkowski as ME
  st = ME.SparseTensor(batch["voxel_feats"].float(), coords=batch["voxel_coords"].int()).to(dev)
  d_out = torch.randn(st.F.shape[0], C, device=dev)

  def backbone():
    trainer.flat.zero_grad()
    trainer.engine.forward(0, st, training=True)
    trainer.engine.backward(0, d_out)

  bb = timed(backbone, args.warmup, args.repeats)
  report("train_iter", voxels=int(st.F.shape[0]), step=step, backbone_fwd_bwd=bb, backbone_share=bb["median_ms"] / step["median_ms"])
  if args.out:
    with open(args.out, "w") as f:
      json.dump(results, f, indent=1)


if __name__ == "__main__":
  main()
