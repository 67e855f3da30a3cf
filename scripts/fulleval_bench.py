"""Times the evaluation on the original point cloud (csrc/nearest.hip) for one ScanNet-like scene against the host path of
the reference (downstream/semseg/lib/datasets/scannet.py:154-168: scipy KD-tree query + fast_hist after a read-back).

The scene is SYNTHETIC: about 150 000 occupied 2 cm voxels on the walls, floor and a few boxes of a 8 x 6 x 3 m room, and as
many vertices jittered around them -- the sizes of a ScanNet scan, not its geometry.  Device times are HIP events around
voxel_centers + nearest_point + seg_hist on warm kernels, the median of --runs; the host baselines run on this machine's CPU
and include the read-back of the voxel predictions they need.  Prints one JSON line.

  python scripts/fulleval_bench.py [--voxels 150000] [--points 150000] [--runs 30] [--no-host]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VOXEL = 0.02


def room(n_voxels, n_points, seed=0):
  """Occupied voxels on the surfaces of a room, and vertices around them.  -> coords int32 [m, 4], T [1, 16], points [n, 3]."""
  rng = np.random.RandomState(seed)
  L = np.array([8.0, 6.0, 3.0])
  pts = []
  k = n_voxels * 3
  for axis in range(3):  # the two faces normal to `axis`, sampled by area
    for side in (0.0, 1.0):
      p = rng.uniform(0, 1, (k // 6, 3)) * L
      p[:, axis] = side * L[axis]
      pts.append(p)
  for _ in range(12):  # furniture: boxes on the floor
    lo = rng.uniform(0, 0.8, 3) * L * [1, 1, 0]
    size = rng.uniform(0.3, 1.5, 3)
    p = lo + rng.uniform(0, 1, (k // 24, 3)) * size
    face = rng.randint(0, 3, len(p))
    p[np.arange(len(p)), face] = lo[face] + size[face] * rng.randint(0, 2, len(p))
    pts.append(p)
  pts = np.concatenate(pts)
  vox = np.unique(np.floor(pts / VOXEL).astype(np.int64), axis=0)
  vox = vox[rng.permutation(len(vox))[:n_voxels]]
  coords = np.concatenate([np.zeros((len(vox), 1), np.int64), vox], 1).astype(np.int32)
  T = np.diag([1 / VOXEL, 1 / VOXEL, 1 / VOXEL, 1.0]).reshape(1, 16)
  centers = (vox + 0.5) * VOXEL
  points = centers[rng.randint(0, len(centers), n_points)] + rng.uniform(-0.9, 0.9, (n_points, 3)) * VOXEL
  return coords, T, points


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--voxels", type=int, default=150000)
  ap.add_argument("--points", type=int, default=150000)
  ap.add_argument("--classes", type=int, default=20)
  ap.add_argument("--runs", type=int, default=30)
  ap.add_argument("--no-host", action="store_true")
  a = ap.parse_args()
  assert torch.cuda.is_available(), "fulleval_bench measures the device path: it needs the GPU"
  assert a.runs >= 20
  from pointcontrast_amd import functional as PF
  dev = torch.device("cuda", 0)
  coords, T, points = room(a.voxels, a.points)
  m, n, c = len(coords), len(points), a.classes
  rng = np.random.RandomState(1)
  pred = rng.randint(0, c, m).astype(np.int32)
  labels = rng.randint(0, c, n).astype(np.int32)
  coords_d, pred_d = torch.from_numpy(coords).to(dev), torch.from_numpy(pred).to(dev)
  points_d, labels_d = torch.from_numpy(points).to(dev), torch.from_numpy(labels).to(dev)
  ro = torch.tensor([0, m], dtype=torch.int64, device=dev)
  qo = torch.tensor([0, n], dtype=torch.int64, device=dev)
  Tt = torch.from_numpy(T)
  fb = torch.zeros(1, dtype=torch.int64, device=dev)

  def device_path(cell, fallback=None):
    centers = PF.voxel_centers(coords_d, Tt)
    idx = PF.nearest_point(centers, ro, points_d, qo, cell=cell, fallback_count=fallback)
    return PF.seg_hist(pred_d, idx, labels_d, c), idx

  def timed(cell):
    for _ in range(3):
      device_path(cell)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.runs):
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      device_path(cell)
      e1.record()
      e1.synchronize()
      ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))

  out, idx = device_path(2 * VOXEL, fb)
  torch.cuda.synchronize()
  res = dict(voxels=m, points=n, classes=c, runs=a.runs, synthetic=True, fallback_queries=int(fb.cpu()),
             fallback_share=float(int(fb.cpu()) / n))
  for name, cell in (("cell_2_voxels", 2 * VOXEL), ("cell_default", None)):
    med, lo, hi = timed(cell)
    res["device_ms_" + name] = dict(median=med, min=lo, max=hi)
  if not a.no_host:
    from scipy import spatial
    hist_d = out["hist"].cpu().numpy()
    idx_d = idx.cpu().numpy()

    def host_path(query_fn):
      t0 = time.perf_counter()
      torch.cuda.synchronize()
      p = pred_d.cpu().numpy()  # the read-back the host path starts with
      centers = (coords[:, 1:] + 0.5) * VOXEL
      result = query_fn(centers)
      pp = p[result]
      k = (labels >= 0) & (labels < c)
      hist = np.bincount(c * labels[k].astype(int) + pp[k], minlength=c * c).reshape(c, c)
      return (time.perf_counter() - t0) * 1e3, result, hist

    t1, r1, h1 = host_path(lambda ctr: spatial.KDTree(ctr, leafsize=500).query(points)[1])
    res["host_ms_KDTree_leafsize500_1thread"] = t1
    t16 = []
    for _ in range(5):
      t, r16, h16 = host_path(lambda ctr: spatial.cKDTree(ctr).query(points, workers=16)[1])
      t16.append(t)
    res["host_ms_cKDTree_workers16"] = dict(median=float(np.median(t16)), min=float(np.min(t16)))
    # same answer (ties aside: the KD-tree's choice among equidistant centres is arbitrary)
    res["index_mismatches_vs_KDTree"] = int((r1 != idx_d).sum())
    res["hist_equal_KDTree"] = bool(np.array_equal(h1, hist_d))
  print(json.dumps(res))


if __name__ == "__main__":
  main()
