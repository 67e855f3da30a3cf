"""Times the validation by feature matching (csrc/featmatch.hip, lib/feature_match.py) at the shape of BASELINE configs[1]:
4 pairs, about 87 000 voxels per cloud, 32-channel features.

The pairs are SYNTHETIC: voxels on the surfaces of a room at 2.5 cm, cloud 1 a rigid copy of cloud 0 snapped to voxels, unit
features shared by corresponding rows plus noise -- the sizes of the pre-training batches, not their geometry.  Device times
are HIP events around warm calls, the median of --runs after --warmup:
  * one PF.feature_nn call over the batch against B calls of PF.pdist_argmin on the same data (every row a query);
  * PF.feature_nn, PF.match_stats, PF.ransac_score (H hypotheses) and PF.rigid_sums at --queries sampled rows per pair;
  * a whole FeatureMatchEvaluator.step at --queries;
  * the same metrics on the host (numpy, this machine's CPU): matrix-product nearest neighbours both ways, the geometric
    check, the same RANSAC hypotheses scored in blocks, Kabsch.
Prints one JSON line.

  python scripts/feature_match_bench.py [--pairs 4] [--voxels 87000] [--channels 32] [--queries 5000] [--hypotheses 4096]
                                        [--runs 25] [--no-host]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VOXEL = 0.025


def room_voxels(n, rng):
  """n distinct occupied voxels on the walls and floor of an 8 x 6 x 3 m room."""
  L = np.array([8.0, 6.0, 3.0])
  pts = []
  for axis in range(3):
    for side in (0.0, 1.0):
      p = rng.uniform(0, 1, (n, 3)) * L
      p[:, axis] = side * L[axis]
      pts.append(p)
  vox = np.unique(np.floor(np.concatenate(pts) / VOXEL).astype(np.int64), axis=0)
  return vox[rng.permutation(len(vox))[:n]]


def random_pose(rng):
  Q, R = np.linalg.qr(rng.normal(size=(3, 3)))
  Q = Q * np.sign(np.diag(R))
  if np.linalg.det(Q) < 0:
    Q[:, 0] = -Q[:, 0]
  T = np.eye(4)
  T[:3, :3], T[:3, 3] = Q, rng.uniform(-1, 1, 3)
  return T


def make_batch(pairs, voxels, channels, seed=0):
  rng = np.random.RandomState(seed)
  C0, C1, F0, F1, T, lens, corr = [], [], [], [], [], [], []
  s0 = s1 = 0
  for b in range(pairs):
    v0 = room_voxels(voxels, rng)
    Tb = random_pose(rng)
    moved = (v0 * VOXEL) @ Tb[:3, :3].T + Tb[:3, 3]
    v1, first = np.unique(np.floor(moved / VOXEL + 0.5).astype(np.int64), axis=0, return_index=True)
    f = rng.normal(size=(len(v0), channels))
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    F0.append((f + rng.normal(0, 0.02, f.shape)).astype(np.float32))
    F1.append((f[first] + rng.normal(0, 0.02, (len(first), channels))).astype(np.float32))
    C0.append(np.concatenate([np.full((len(v0), 1), b), v0], 1).astype(np.int32))
    C1.append(np.concatenate([np.full((len(v1), 1), b), v1], 1).astype(np.int32))
    corr.append(np.stack([first + s0, np.arange(len(first)) + s1], 1))
    T.append(Tb)
    lens.append([len(v0), len(v1)])
    s0, s1 = s0 + len(v0), s1 + len(v1)
  corr = np.concatenate(corr)
  return dict(C0=np.concatenate(C0), C1=np.concatenate(C1), F0=np.concatenate(F0), F1=np.concatenate(F1), T=np.stack(T),
              len_batch=lens, corr=corr[np.argsort(corr[:, 0], kind="stable")])


def timed(fn, runs, warmup):
  for _ in range(warmup):
    fn()
  torch.cuda.synchronize()
  ms = []
  for _ in range(runs):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    ms.append(e0.elapsed_time(e1))
  return dict(median=float(np.median(ms)), min=float(np.min(ms)), max=float(np.max(ms)))


def host_metrics(batch, draws, taus, ransac_tau):
  """The evaluator's quantities with numpy on the host, pair by pair."""
  from pointcontrast_amd.lib.feature_match import kabsch, offsets_of
  o0, o1 = offsets_of([l[0] for l in batch["len_batch"]]), offsets_of([l[1] for l in batch["len_batch"]])
  out = []
  for b in range(len(batch["len_batch"])):
    rows = draws.query_rows[draws.query_offsets[b]:draws.query_offsets[b + 1]].astype(np.int64)
    f0, f1 = batch["F0"][o0[b]:o0[b + 1]], batch["F1"][o1[b]:o1[b + 1]]
    a = batch["F0"][rows]
    n1 = (f1 * f1).sum(1)
    nn01 = np.concatenate([(n1[None] - 2.0 * (a[i:i + 1024] @ f1.T)).argmin(1) for i in range(0, len(a), 1024)])
    n0 = (f0 * f0).sum(1)
    m = f1[nn01]
    nn10 = np.concatenate([(n0[None] - 2.0 * (m[i:i + 1024] @ f0.T)).argmin(1) for i in range(0, len(m), 1024)])
    x0 = batch["C0"][rows, 1:4] * VOXEL
    x1 = batch["C1"][o1[b] + nn01, 1:4] * VOXEL
    T = batch["T"][b]
    r2 = ((x0 @ T[:3, :3].T + T[:3, 3] - x1) ** 2).sum(1)
    hits = [(r2 <= t * t).mean() for t in taus]
    mutual = (nn10 + o0[b] == rows).mean()
    tri = draws.triples[b].astype(np.int64)
    p, q = x0[tri], x1[tri]  # [H, 3, 3]

    def frames(a3):
      e1 = a3[:, 1] - a3[:, 0]
      e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
      n = np.cross(e1, a3[:, 2] - a3[:, 0])
      e3 = n / np.linalg.norm(n, axis=1, keepdims=True)
      return np.stack([e1, np.cross(e3, e1), e3], 1)
    with np.errstate(invalid="ignore", divide="ignore"):
      E, Fq = frames(p.copy()), frames(q.copy())
      R = np.einsum("hki,hkj->hij", Fq, E)
      t = q[:, 0] - np.einsum("hij,hj->hi", R, p[:, 0])
      counts = np.zeros(len(tri), dtype=np.int64)
      for i in range(0, len(tri), 256):
        y = np.einsum("hij,mj->hmi", R[i:i + 256], x0) + t[i:i + 256, None]
        counts[i:i + 256] = (((y - x1[None]) ** 2).sum(2) <= ransac_tau ** 2).sum(1)
    best = int(counts.argmax())
    inl = ((x0 @ R[best].T + t[best] - x1) ** 2).sum(1) <= ransac_tau ** 2
    P, Qd = x0[inl], x1[inl]
    pm, qm = P.mean(0), Qd.mean(0)
    fit = kabsch(np.concatenate([[len(P)], pm * len(P), qm * len(P), ((P - pm).T @ (Qd - qm)).reshape(-1)]))
    out.append(dict(hits=hits, mutual=float(mutual), inliers=int(inl.sum()), fit=fit is not None))
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--pairs", type=int, default=4)
  ap.add_argument("--voxels", type=int, default=87000)
  ap.add_argument("--channels", type=int, default=32)
  ap.add_argument("--queries", type=int, default=5000)
  ap.add_argument("--hypotheses", type=int, default=4096)
  ap.add_argument("--runs", type=int, default=25)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--no-host", action="store_true")
  a = ap.parse_args()
  assert torch.cuda.is_available(), "feature_match_bench measures the device path: it needs the GPU"
  from pointcontrast_amd import build, functional as PF
  from pointcontrast_amd.lib.feature_match import FeatureMatchEvaluator, MatchDraws, offsets_of
  dev = torch.device("cuda", 0)
  batch = make_batch(a.pairs, a.voxels, a.channels)
  lens = batch["len_batch"]
  B = len(lens)
  o0, o1 = offsets_of([l[0] for l in lens]), offsets_of([l[1] for l in lens])
  up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
  F0, F1, C0, C1, T, corr = (up(batch[k]) for k in ("F0", "F1", "C0", "C1", "T", "corr"))
  o0d, o1d = up(o0), up(o1)
  res = dict(pairs=B, rows_cloud0=int(o0[-1]), rows_cloud1=int(o1[-1]), channels=a.channels, queries_per_pair=a.queries,
             hypotheses=a.hypotheses, runs=a.runs, synthetic=True, variant="plain fp32 FMA", build=build.sources_digest()[:12])

  # 1. every row a query: one segmented call against B unsegmented ones
  res["feature_nn_all_rows_ms"] = timed(lambda: PF.feature_nn(F0, o0d, F1, o1d), a.runs, a.warmup)
  if a.channels in (16, 32, 64):
    parts = [(F0[o0[b]:o0[b + 1]].contiguous(), F1[o1[b]:o1[b + 1]].contiguous()) for b in range(B)]
    res["pdist_argmin_B_calls_ms"] = timed(lambda: [PF.pdist_argmin(x, y) for x, y in parts], a.runs, a.warmup)
    nn, _ = PF.feature_nn(F0, o0d, F1, o1d)
    amin = torch.cat([PF.pdist_argmin(x, y)[1].long() + int(o1[b]) for b, (x, y) in enumerate(parts)])
    res["nn_disagreements_with_pdist_argmin"] = int((nn.long() != amin).sum())

  # 2. the pieces at the evaluator's sampled queries
  draws = MatchDraws.sample(lens, a.queries, a.hypotheses, np.random.RandomState(0))
  rows, qoffs, tri = up(draws.query_rows), up(draws.query_offsets), up(draws.triples)
  res["feature_nn_sampled_ms"] = timed(lambda: PF.feature_nn(F0, o0d, F1, o1d, query_rows=rows, query_offsets=qoffs), a.runs, a.warmup)
  nn01, _ = PF.feature_nn(F0, o0d, F1, o1d, query_rows=rows, query_offsets=qoffs)
  res["feature_nn_reverse_ms"] = timed(lambda: PF.feature_nn(F1, o1d, F0, o0d, query_rows=nn01, query_offsets=qoffs), a.runs, a.warmup)
  nn10, _ = PF.feature_nn(F1, o1d, F0, o0d, query_rows=nn01, query_offsets=qoffs)
  xyz0, xyz1 = C0[:, 1:4].double() * VOXEL, C1[:, 1:4].double() * VOXEL
  taus = (0.1,)
  res["match_stats_ms"] = timed(lambda: PF.match_stats(xyz0, xyz1, T, qoffs, nn01, taus, query_rows=rows, nn10=nn10), a.runs, a.warmup)
  src, dst = xyz0[rows.long()], xyz1[nn01.clamp(min=0).long()]
  tau = 2 * VOXEL
  res["ransac_score_ms"] = timed(lambda: PF.ransac_score(src, dst, qoffs, tri, tau), a.runs, a.warmup)
  _, best, Rt = PF.ransac_score(src, dst, qoffs, tri, tau)
  res["rigid_sums_ms"] = timed(lambda: PF.rigid_sums(src, dst, qoffs, best, Rt, tau), a.runs, a.warmup)

  # 3. a whole step, and the metrics it leads to
  ev = FeatureMatchEvaluator(VOXEL, num_queries=a.queries, ransac_hypotheses=a.hypotheses)
  ddev = MatchDraws(rows, qoffs, tri)

  def step():
    ev.reset()
    ev.step(F0, F1, C0, C1, T, lens, correspondences=corr, draws=ddev)
  res["step_ms"] = timed(step, a.runs, a.warmup)
  t0 = time.perf_counter()
  m = ev.compute_metrics()
  res["compute_metrics_host_ms"] = (time.perf_counter() - t0) * 1e3
  res["metrics"] = {k: v for k, v in m.items() if k != "pairs"}

  # 4. the host path
  if not a.no_host:
    ts = []
    for _ in range(3):
      t0 = time.perf_counter()
      host = host_metrics(batch, draws, taus, tau)
      ts.append((time.perf_counter() - t0) * 1e3)
    res["host_numpy_ms"] = dict(median=float(np.median(ts)), min=float(np.min(ts)), threads=torch.get_num_threads())
    res["host_hit_ratio"] = float(np.mean([h["hits"][0] for h in host]))
  print(json.dumps(res))


if __name__ == "__main__":
  main()
