"""Times the pair-corpus builder (lib/pair_corpus.py, csrc/corpus.hip) on one synthetic scene of ScanNet shape.

  python scripts/corpus_bench.py [--frames 80] [--width 640] [--height 480] [--reps 3] [--out FILE] [--color]

The scene: --frames depth frames ray-cast in a furnished room of lib/synthetic.py (tests/pair_corpus_ref.py:
synthetic_scene).  Reported, as one JSON line:
  * GPU seconds per stage (back-projection incl. the depth upload, voxel centroids, all-pairs overlap counts, the
    download of points and centroids), the median of --reps runs after one warm-up; frames/s and ordered pairs/s;
  * the same scene through the tests' numpy/scipy restatement (cKDTree): seconds, pairs/s, and whether every point,
    centroid, count and ratio is bit-identical;
  * host I/O of the same frames: PNG decoding with PIL and npz writing on the builder's thread pool, which on real
    data may cost more than the GPU work;
  * --color: the same runs with a synthetic colour image per frame (--color-width x --color-height, ScanNet's 1296 x 968) --
    the stage backproject_color (image upload, pcmi_corpus_backproject_color, the read-back of the counts) beside the others,
    its output against tests/pair_color_ref.py, and the host decode of --color-decode-frames such images from JPEG."""
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
  ap.add_argument("--color", action="store_true", help="also colour the points (pcmi_corpus_backproject_color)")
  ap.add_argument("--color-width", type=int, default=1296)
  ap.add_argument("--color-height", type=int, default=968)
  ap.add_argument("--color-decode-frames", type=int, default=16, help="colour frames whose JPEG decode is timed")
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
  ckw = {}
  if args.color:  # a smooth image with noise on it, one per frame; the colour camera looks along the depth camera, 2 cm beside it
    rng = np.random.RandomState(0)
    Hc, Wc = args.color_height, args.color_width
    yy, xx = np.mgrid[0:Hc, 0:Wc]
    base = np.stack([xx * 255 // max(Wc - 1, 1), yy * 255 // max(Hc - 1, 1), (xx + yy) % 256], -1).astype(np.uint8)
    colors = np.stack([base ^ rng.randint(0, 16, base.shape).astype(np.uint8) for _ in range(F)])
    Kc = ref.intrinsic_matrix(Wc, Hc)
    M = np.eye(4)
    M[0, 3] = 0.02
    ckw = dict(colors=colors, color_intrinsic=Kc, depth_to_color=M)
  pc.process_scene(depths[:4], poses[:4], K, voxel_size=args.voxel_size, **{k: (v[:4] if k == "colors" else v) for k, v in ckw.items()})  # warm-up
  runs = []
  for _ in range(max(args.reps, 1)):
    torch.cuda.synchronize()
    t = time.perf_counter()
    got = pc.process_scene(depths, poses, K, voxel_size=args.voxel_size, **ckw)
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
    if args.color:
      import pair_color_ref as cr
      t = time.perf_counter()
      want_col, want_unc, offs = cr.backproject_color_ref(depths, K, colors, Kc, M)
      res["color_ref_s"] = time.perf_counter() - t
      same_c = np.array_equal(got["uncolored"], want_unc) and all(
          np.array_equal(c, want_col[offs[f]:offs[f + 1]]) for c, f in zip(got["colors"], got["frames"]))
      res["bit_identical"] = bool(same and same_c)
  if args.color:
    res.update(color_width=args.color_width, color_height=args.color_height, color_image_bytes=int(colors.nbytes),
               uncolored=int(got["uncolored"].sum()))

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
      if args.color:
        t = time.perf_counter()
        list(pool.map(lambda kp: pc.write_npz(os.path.join(tmp, "c%d.npz" % kp[0]), kp[1][0], kp[1][1]), enumerate(zip(got["points"], got["colors"]))))
        res["npz_write_color_s"] = time.perf_counter() - t
        nd = max(1, min(args.color_decode_frames, F))
        cpaths = [os.path.join(tmp, "c%d.jpg" % k) for k in range(nd)]
        for p, c in zip(cpaths, colors):
          Image.fromarray(c).save(p, quality=90)
        t = time.perf_counter()
        dec = list(pool.map(pc.read_color, cpaths))
        res["color_jpeg_decode_s_per_frame"] = (time.perf_counter() - t) / nd  # wall clock on the pool / frames
        res["color_decode_frames"] = nd
        assert all(a.shape == colors[0].shape for a in dec)
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
