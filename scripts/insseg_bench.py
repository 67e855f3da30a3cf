"""Times the instance clustering (csrc/cluster.hip) on a ScanNet-sized batch against the host path it replaces.

The batch is SYNTHETIC: 8 scenes of about 150 000 occupied 2 cm voxels -- the hollow boxes of about 30 "instances" in a 8 x 6 x 3 m
room plus its floor and two walls (stuff) -- the sizes of ScanNet scans, not their geometry.  Two states of the offset head:
  untrained  the offsets are noise of 5 mm: the rows stay on their surfaces (many cells, short lists)
  trained    the offsets point to the instance's centroid, 5 mm of noise left: every instance lies within the radius of its centre
             (few cells, long lists, every pair an edge) -- the state that decides the kernel's shape
Device times are HIP events around pcmi_radius_components, pcmi_components_compact, pcmi_instance_scores and the whole
cluster_instances call on warm kernels, the median of --runs in one process.  The host baseline is
scipy.spatial.cKDTree.query_pairs + scipy.sparse.csgraph.connected_components per scene and class on this machine's CPU; in the
trained state an instance of k rows has k (k - 1) / 2 pairs, so the baseline is run on the first --host-instances instances only
and reported with that scope.  Prints one JSON line.

  python scripts/insseg_bench.py [--scenes 8] [--voxels 150000] [--runs 25] [--no-host]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VOXEL, RADIUS, MIN_POINTS, CLASSES = 0.02, 0.03, 50, 20


def scene(n_voxels, n_boxes, rng):
  """-> vox int64 [m, 3], cls [m], inst [m] (0 .. n_boxes - 1, -1 for stuff) of one room, rows grouped by instance."""
  L = np.array([8.0, 6.0, 3.0])
  per_box = int(n_voxels * 0.8 / n_boxes)
  vox, cls, inst = [], [], []
  for k in range(n_boxes):
    size = rng.uniform(0.5, 1.3, 3)
    lo = rng.uniform(0, 1, 3) * (L - size)
    p = lo + rng.uniform(0, 1, (per_box * 3, 3)) * size
    face = rng.integers(0, 3, len(p))
    p[np.arange(len(p)), face] = lo[face] + size[face] * rng.integers(0, 2, len(p))
    v = np.unique(np.floor(p / VOXEL).astype(np.int64), axis=0)
    v = v[rng.permutation(len(v))[:per_box]]
    vox.append(v)
    cls.append(np.full(len(v), 2 + k % (CLASSES - 2)))
    inst.append(np.full(len(v), k))
  rest = n_voxels - sum(len(v) for v in vox)
  p = rng.uniform(0, 1, (rest * 2, 3)) * L
  which = rng.integers(0, 3, len(p))  # floor, wall x = 0, wall y = 0
  p[which == 0, 2] = 0.0
  p[which == 1, 0] = 0.0
  p[which == 2, 1] = 0.0
  v, first = np.unique(np.floor(p / VOXEL).astype(np.int64), axis=0, return_index=True)
  keep = rng.permutation(len(v))[:rest]
  vox.append(v[keep])
  cls.append(np.where(which[first][keep] == 0, 1, 0))
  inst.append(np.full(len(keep), -1))
  vox, cls, inst = np.concatenate(vox), np.concatenate(cls), np.concatenate(inst)
  # a voxel two boxes share stays with the first
  _, first = np.unique(vox, axis=0, return_index=True)
  first.sort()
  return vox[first], cls[first], inst[first]


def batch(n_scenes, n_voxels, n_boxes, seed=0):
  rng = np.random.default_rng(seed)
  coords, cls, inst, offs, base = [], [], [], [0], 0
  for b in range(n_scenes):
    v, c, i = scene(n_voxels, n_boxes, rng)
    coords.append(np.concatenate([np.full((len(v), 1), b), v], 1))
    cls.append(c)
    inst.append(np.where(i >= 0, i + base, -1))
    base += n_boxes
    offs.append(offs[-1] + len(v))
  return np.concatenate(coords).astype(np.int32), np.concatenate(cls), np.concatenate(inst), np.array(offs, np.int64), rng


def host_components(xyz, rows):
  """The number of components with at least MIN_POINTS rows among `rows`, by scipy; the time in ms and the pairs."""
  from scipy.sparse import coo_matrix
  from scipy.sparse.csgraph import connected_components
  from scipy.spatial import cKDTree
  t0 = time.perf_counter()
  p = xyz[rows].astype(np.float64)
  pairs = cKDTree(p).query_pairs(RADIUS, output_type="ndarray")
  graph = coo_matrix((np.ones(len(pairs), np.int8), (pairs[:, 0], pairs[:, 1])), shape=(len(p), len(p)))
  comp = connected_components(graph, directed=False)[1]
  kept = int((np.bincount(comp) >= MIN_POINTS).sum()) if len(p) else 0
  return kept, (time.perf_counter() - t0) * 1e3, len(pairs)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--scenes", type=int, default=8)
  ap.add_argument("--voxels", type=int, default=150000)
  ap.add_argument("--boxes", type=int, default=30)
  ap.add_argument("--runs", type=int, default=25)
  ap.add_argument("--host-instances", type=int, default=3)
  ap.add_argument("--no-host", action="store_true")
  a = ap.parse_args()
  assert torch.cuda.is_available(), "insseg_bench measures the device path: it needs the GPU"
  from pointcontrast_amd import functional as PF
  from pointcontrast_amd.downstream.insseg import cluster_instances
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
  group = np.where(cls < 2, -1, cls).astype(np.int32)
  group_d = torch.from_numpy(group).to(dev)
  score_d = torch.rand(n, device=dev)
  res = dict(scenes=a.scenes, rows=n, instances=G, radius=RADIUS, min_points=MIN_POINTS, synthetic=True)

  def timed(fn, runs):
    for _ in range(2):
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
    return dict(median=float(np.median(ms)), min=float(np.min(ms)), max=float(np.max(ms)), runs=runs)

  for state in ("untrained", "trained"):
    off_d = torch.from_numpy(offsets[state]).to(dev)
    xyz_d = (coords_d[:, 1:4].to(torch.float32) * VOXEL + off_d).contiguous()
    t0 = time.perf_counter()
    label = PF.radius_components(xyz_d, offs_d, group_d, RADIUS)
    torch.cuda.synchronize()
    first_ms = (time.perf_counter() - t0) * 1e3
    runs = a.runs if first_ms < 2000 else 3  # a pathological time still ends
    comp = PF.components_compact(label, offs_d, group_d, MIN_POINTS, 4096)
    out = dict(first_call_ms=first_ms, instances_found=int(comp["count"].cpu()))
    out["radius_components_ms"] = timed(lambda: PF.radius_components(xyz_d, offs_d, group_d, RADIUS), runs)
    out["components_compact_ms"] = timed(lambda: PF.components_compact(label, offs_d, group_d, MIN_POINTS, 4096), runs)
    out["instance_scores_ms"] = timed(lambda: PF.instance_scores(score_d, comp["instance"], comp["size"]), runs)
    out["cluster_instances_ms"] = timed(lambda: cluster_instances(coords_d, off_d, logits_d, offs_d, VOXEL, RADIUS, MIN_POINTS), runs)
    if not a.no_host:
      xyz = xyz_d.cpu().numpy()
      lab = label.cpu().numpy()
      if state == "untrained":  # every scene and class: the pairs are few
        total, pairs, kept = 0.0, 0, 0
        for b in range(a.scenes):
          for c in range(2, CLASSES):
            rows = np.flatnonzero((group == c) & (np.arange(n) >= offs[b]) & (np.arange(n) < offs[b + 1]))
            if len(rows):
              k, ms, npairs = host_components(xyz, rows)
              total, pairs, kept = total + ms, pairs + npairs, kept + k
        out["host_ms_all_scenes_and_classes"] = total
        out["host_pairs"], out["host_instances_found"] = pairs, kept
      else:  # an instance of k rows has k (k - 1) / 2 pairs: the first few instances only
        total, pairs, agree = 0.0, 0, True
        for k in range(min(a.host_instances, G)):
          rows = np.flatnonzero(inst == k)
          kept, ms, npairs = host_components(xyz, rows)
          total, pairs = total + ms, pairs + npairs
          agree = agree and kept == 1 and len(np.unique(lab[rows])) == 1
        out["host_ms_first_instances"] = total
        out["host_instances_timed"], out["host_pairs"], out["host_agrees"] = min(a.host_instances, G), pairs, agree
    res[state] = out
  print(json.dumps(res))


if __name__ == "__main__":
  main()
