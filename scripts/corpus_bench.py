"""Times the pair-corpus builder (lib/pair_corpus.py, csrc/corpus.hip) on one synthetic scene of ScanNet shape.

  python scripts/corpus_bench.py [--frames 80] [--width 640] [--height 480] [--reps 3] [--out FILE]

The scene: --frames depth frames ray-cast in a furnished room of lib/synthetic.py (tests/pair_corpus_ref.py:
synthetic_scene).  Reported, as one JSON line:
  * GPU seconds per stage (back-projection incl. the depth upload, voxel centroids, all-pairs overlap counts, the
    download of points and centroids), the median of --reps runs after one warm-up; frames/s and ordered pairs/s;
  * the same scene through the tests' numpy/scipy restatement (cKDTree): seconds, pairs/s, and whether every point,
    centroid, count and ratio is bit-identical;
  * host I/O of the same frames: PNG decoding with PIL and npz writing on the builder's thread pool, which on real
    data may cost more than the GPU work."""
import argparse
import concurrent.futures
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--frames", type=int, default=80)
  ap.add_argument("--width", type=int, default=640)
  ap.add_argument("--height", type=int, default=480)
  ap.add_argument("--voxel-size", type=float, default=0.05)
  ap.add_argument("--reps", type=int, default=3)
  ap.add_argument("--no-ref", action="store_true", help="skip the numpy/scipy path")
  ap.add_argument("--out", default=None, help="also write the JSON line here")
  args = ap.parse_args()
  import torch
  if not torch.cuda.is_available():
    sys.exit("corpus_bench: no GPU")
  import pair_corpus_ref as ref
  from pointcontrast_amd.lib import pair_corpus as pc

  t = time.perf_counter()
  depths, poses, K = ref.synthetic_scene(args.frames, width=args.width, height=args.height, step=0.12 * 12 / args.frames * 2)
  gen_s = time.perf_counter() - t
  F = args.frames
  pc.process_scene(depths[:4], poses[:4], K, voxel_size=args.voxel_size)  # warm-up: code objects, workspace
  runs = []
  for _ in range(max(args.reps, 1)):
    torch.cuda.synchronize()
    t = time.perf_counter()
    got = pc.process_scene(depths, poses, K, voxel_size=args.voxel_size)
    total = time.perf_counter() - t
    runs.append(dict(got["gpu_s"], total=total))
  stages = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
  V = len(got["frames"])
  res = dict(frames=F, width=args.width, height=args.height, voxel_size=args.voxel_size, valid_frames=V,
             points=int(sum(len(p) for p in got["points"])), centroids=int(sum(len(c) for c in got["centroids"])),
             pairs_over_0_3=int(sum(max(got["M"][i, j], got["M"][j, i]) >= 0.3 for i in range(V) for j in range(i + 1, V))),
             gpu_s=stages, gpu_frames_per_s=F / stages["total"], gpu_ordered_pairs_per_s=V * (V - 1) / stages["total"],
             scene_generation_s=gen_s)

  if not args.no_ref:
    t = time.perf_counter()
    want = ref.process_scene(depths, poses, K, voxel_size=args.voxel_size)
    ref_s = time.perf_counter() - t
    same = (list(got["frames"]) == list(want["frames"]) and np.array_equal(got["C"], want["C"]) and
            np.array_equal(got["M"], want["M"]) and
            all(np.array_equal(a, b) for a, b in zip(got["points"], want["points"])) and
            all(np.array_equal(a, b) for a, b in zip(got["centroids"], want["centroids"])))
    res.update(ref_s=ref_s, ref_ordered_pairs_per_s=V * (V - 1) / ref_s, speedup_vs_ref=ref_s / stages["total"],
               bit_identical=bool(same))

  with tempfile.TemporaryDirectory() as tmp:  # host I/O of the same frames on the builder's pool
    from PIL import Image
    paths = [os.path.join(tmp, "%d.png" % k) for k in range(F)]
    for p, d in zip(paths, depths):
      Image.fromarray(d).save(p)
    with concurrent.futures.ThreadPoolExecutor(pc.IO_THREADS) as pool:
      t = time.perf_counter()
      dec = list(pool.map(pc.read_depth, paths))
      res["png_decode_s"] = time.perf_counter() - t
      assert all(np.array_equal(a, b) for a, b in zip(dec, depths))
      t = time.perf_counter()
      list(pool.map(lambda kp: pc.write_npz(os.path.join(tmp, "%d.npz" % kp[0]), kp[1]), enumerate(got["points"])))
      res["npz_write_s"] = time.perf_counter() - t
      res["npz_bytes"] = int(sum(os.path.getsize(os.path.join(tmp, "%d.npz" % k)) for k in range(V)))
    res["io_threads"] = pc.IO_THREADS
  line = json.dumps(res)
  print(line, flush=True)
  if args.out:
    with open(args.out, "w") as f:
      f.write(line + "\n")
  if not args.no_ref and not res["bit_identical"]:
    sys.exit("corpus_bench: the device output differs from the restatement")


if __name__ == "__main__":
  main()
