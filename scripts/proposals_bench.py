"""Times the dual-set proposals (csrc/proposals.hip, downstream/insseg.py's cluster_proposals) on a ScanNet-sized batch, beside
cluster_instances, beside an evaluator step on disjoint masks, and beside PointGroup's dense spelling of the same suppression.

The batch is insseg_bench.py's SYNTHETIC one: 8 scenes of about 150 000 occupied 2 cm voxels, 30 box "instances" each (240 in
all) -- the sizes of ScanNet scans, not their geometry -- in its two states of the offset head:
  untrained  offsets of 5 mm noise: both sets find nearly the same masks
  trained    offsets to the instance's centroid: the shifted set separates what touches, and the two clusters of one object
             share thousands of consecutive rows -- the state pcmi_proposal_overlap's wave aggregation is written for
Per state, with the variants ALTERNATING inside one loop of one process, HIP events around each on warm kernels, the median of
--runs with the minimum beside it:
  second_clustering   radius_components + components_compact + instance_scores on the unshifted coordinates: what the second
                      set costs
  proposal_overlap, proposal_nms
  cluster_proposals | cluster_instances        the whole calls
  step_overlapping | step_disjoint             InstanceBenchmarkEvaluator.step on cluster_proposals' / cluster_instances' dict
  dense_baseline      per scene, in torch on the same device: the [proposals of the scene, rows of the scene] float32 indicator,
                      torch.mm with its transpose, the quotients, then the greedy loop on the host (PointGroup runs it there);
                      a scene whose matrix does not fit in free memory is REPORTED, not shrunk
Nothing here says anything about accuracy.  Prints one JSON line.

  python scripts/proposals_bench.py [--scenes 8] [--voxels 150000] [--runs 25]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from insseg_bench import CLASSES, MIN_POINTS, RADIUS, VOXEL, batch  # noqa: E402

MAX_INSTANCES, NMS_IOU = 4096, 0.3


def dense_keep(member, scene, cls, score, offs_host, nms_iou):
  """PointGroup's spelling, scene by scene -> (keep int32 [P] on the host, the scenes whose matrix did not fit)."""
  P, dev = scene.shape[0], member.device
  keep, skipped = np.zeros(P, np.int32), []
  for b in range(len(offs_host) - 1):
    lo, hi = int(offs_host[b]), int(offs_host[b + 1])
    used = torch.nonzero(scene == b).reshape(-1)
    K, nb = used.shape[0], hi - lo
    if K == 0 or nb == 0:
      continue
    if K * nb * 4 > 0.8 * torch.cuda.mem_get_info(dev)[0]:
      skipped.append(b)
      continue
    lut = torch.full((P,), -1, dtype=torch.int64, device=dev)
    lut[used] = torch.arange(K, device=dev)
    A = torch.zeros((K, nb), dtype=torch.float32, device=dev)
    rows = torch.arange(nb, device=dev)
    for s in range(member.shape[1]):
      m = member[lo:hi, s].long()
      idx = torch.where((m >= 0) & (m < P), lut[m.clamp(0, P - 1)], torch.full_like(m, -1))
      ok = idx >= 0
      A[idx[ok], rows[ok]] = 1.0
    inter = torch.mm(A, A.t())
    size = A.sum(1)
    iou = (inter / (size[:, None] + size[None, :] - inter)).cpu().numpy()
    sc, cl, sz = score[used].cpu().numpy(), cls[used].cpu().numpy(), size.cpu().numpy()
    ok = (sz >= 1) & (cl >= 0) & np.isfinite(sc)
    gone = ~ok
    used_h = used.cpu().numpy()
    for i in np.argsort(-sc, kind="stable"):
      if gone[i]:
        continue
      keep[used_h[i]] = 1
      over = iou[i] > nms_iou
      over[i] = False
      gone |= over
  return keep, skipped


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--scenes", type=int, default=8)
  ap.add_argument("--voxels", type=int, default=150000)
  ap.add_argument("--boxes", type=int, default=30)
  ap.add_argument("--runs", type=int, default=25)
  a = ap.parse_args()
  assert torch.cuda.is_available(), "proposals_bench measures the device path: it needs the GPU"
  from pointcontrast_amd import functional as PF
  from pointcontrast_amd.downstream.insseg import InstanceBenchmarkEvaluator, cluster_instances, cluster_proposals
  dev = torch.device("cuda", 0)
  coords, cls, inst, offs, rng = batch(a.scenes, a.voxels, a.boxes)
  n, G = len(coords), a.scenes * a.boxes
  xyz0 = coords[:, 1:].astype(np.float64) * VOXEL
  centre = np.zeros((G, 3))
  np.add.at(centre, inst[inst >= 0], xyz0[inst >= 0])
  centre /= np.maximum(np.bincount(inst[inst >= 0], minlength=G), 1)[:, None]
  noise = rng.normal(0, 0.005, (n, 3))
  offsets = dict(untrained=noise.astype(np.float32),
                 trained=np.where(inst[:, None] >= 0, centre[np.maximum(inst, 0)] - xyz0 + noise, noise).astype(np.float32))
  logits = np.full((n, CLASSES), -4.0, np.float32)
  logits[np.arange(n), cls] = 4.0
  logits += rng.normal(0, 0.5, logits.shape).astype(np.float32)
  coords_d, logits_d, offs_d = torch.from_numpy(coords).to(dev), torch.from_numpy(logits).to(dev), torch.from_numpy(offs).to(dev)
  gi, gc = torch.from_numpy(inst).to(dev), torch.from_numpy(cls).to(dev)
  group_d = torch.from_numpy(np.where(cls < 2, -1, cls).astype(np.int32)).to(dev)
  score_d = torch.rand(n, device=dev)
  xyz_d = (coords_d[:, 1:4].to(torch.float32) * VOXEL).contiguous()
  res = dict(scenes=a.scenes, rows=n, instances=G, slots=2 * MAX_INSTANCES, nms_iou=NMS_IOU, max_per_scene=1024, synthetic=True)

  for state in ("untrained", "trained"):
    off_d = torch.from_numpy(offsets[state]).to(dev)
    args = (coords_d, off_d, logits_d, offs_d, VOXEL, RADIUS, MIN_POINTS)
    full = cluster_proposals(*args, max_instances=MAX_INSTANCES, nms_iou=1.0)  # the union before suppression: the calls' input
    prop = cluster_proposals(*args, max_instances=MAX_INSTANCES, nms_iou=NMS_IOU)
    single = cluster_instances(*args, max_instances=MAX_INSTANCES)
    member, scene, pcls, pscore = full["member"], full["inst_scene"], full["inst_class"], full["inst_score"]
    ov = PF.proposal_overlap(member, scene, a.scenes, 1024)

    def second_clustering():
      label = PF.radius_components(xyz_d, offs_d, group_d, RADIUS)
      comp = PF.components_compact(label, offs_d, group_d, MIN_POINTS, MAX_INSTANCES)
      PF.instance_scores(score_d, comp["instance"], comp["size"])

    def step(pred):
      InstanceBenchmarkEvaluator(CLASSES).step(pred, gi, gc, G)

    variants = dict(second_clustering=second_clustering,
                    proposal_overlap=lambda: PF.proposal_overlap(member, scene, a.scenes, 1024),
                    proposal_nms=lambda: PF.proposal_nms(ov, scene, pcls, pscore, NMS_IOU),
                    cluster_proposals=lambda: cluster_proposals(*args, max_instances=MAX_INSTANCES, nms_iou=NMS_IOU),
                    cluster_instances=lambda: cluster_instances(*args, max_instances=MAX_INSTANCES),
                    step_overlapping=lambda: step(prop), step_disjoint=lambda: step(single),
                    dense_baseline=lambda: dense_keep(member, scene, pcls, pscore, offs, NMS_IOU))
    for fn in variants.values():  # warm-up: code objects, the workspace, the allocator
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
    out = {k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), runs=a.runs) for k, v in ms.items()}
    keep = prop["keep"].cpu().numpy()
    dense, skipped = dense_keep(member, scene, pcls, pscore, offs, NMS_IOU)
    out.update(proposals_per_set=[int(c) for c in prop["count"].cpu()], kept=int(keep.sum()), dropped=int(prop["dropped"].cpu()),
               rows_in_two_proposals=int(((member >= 0).sum(1) == 2).sum().cpu()),
               proposals_per_scene_max=int(ov["scene_count"].max().cpu()), dense_scenes_that_did_not_fit=skipped,
               dense_agrees=bool(not skipped and np.array_equal(dense, keep)))
    res[state] = out
  print(json.dumps(res))


if __name__ == "__main__":
  main()
