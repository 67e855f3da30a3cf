"""Times the virtual views of one synthetic scan (lib/scan_views.py, csrc/views.hip).

  python scripts/scan_views_bench.py [--points 1500000] [--views 64] [--width 320] [--height 240] [--focal 288] [--splat 3]
                                     [--rel-tol 0.05] [--reps 25] [--scan-reps 3] [--no-ref] [--out FILE]

The scan: --points surface samples of tests/views_ref.py's room (shell plus boxes); the cameras: ViewDraws.sample with seed 0.
Reported, as one JSON line:
  * kernel_ms: device events around pcmi_views_zbuffer (the fill of the buffer and the splat kernel), pcmi_views_visible (the
    verdict kernel, the scan of the popcounts, the pixel counts and its one wait for the offsets) and pcmi_views_rows (the
    compaction), the median and the minimum of --reps runs after two warm-up runs, uploads excluded;
  * process_scan_s: the whole call -- uploads, the three above, the gather of the kept views' points, voxel centroids, overlap
    counts, downloads -- by the host clock (the call ends in downloads, so it has waited for the device), the median of
    --scan-reps runs after one warm-up, with its gpu_s stages;
  * ref_s: tests/views_ref.py's numpy restatement of the z-buffer and the visibility test on the same data on this machine's
    CPU, once, and whether zbuf, rows, offsets and pixels are bit-identical (--no-ref skips it).  The restatement of the
    centroid and overlap stages is not timed here (scripts/corpus_bench.py does that for the same kernels)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--points", type=int, default=1500000)
  ap.add_argument("--views", type=int, default=64)
  ap.add_argument("--width", type=int, default=320)
  ap.add_argument("--height", type=int, default=240)
  ap.add_argument("--focal", type=float, default=288.0)
  ap.add_argument("--splat", type=int, default=3)
  ap.add_argument("--rel-tol", type=float, default=0.05)
  ap.add_argument("--reps", type=int, default=25)
  ap.add_argument("--scan-reps", type=int, default=3)
  ap.add_argument("--no-ref", action="store_true", help="skip the numpy restatement")
  ap.add_argument("--out", default=None, help="also write the JSON line here")
  args = ap.parse_args()
  import torch
  if not torch.cuda.is_available():
    sys.exit("scan_views_bench: no GPU")
  import views_ref as vr
  from pointcontrast_amd._lib import check, lib
  from pointcontrast_amd.lib import scan_views as sv
  from pointcontrast_amd.runtime import cur_stream, ptr, ws_args

  t = time.perf_counter()
  xyz, color = vr.synthetic_room(args.points, seed=0)
  poses = sv.ViewDraws.sample(np.random.RandomState(0), xyz, args.views).poses(xyz)
  gen_s = time.perf_counter() - t
  K = sv.pinhole_intrinsic(args.height, args.width, args.focal)
  cam = (K[0, 0], K[1, 1], K[0, 2], K[1, 2], args.height, args.width, 0.1, 10.0)
  n, F, H, W = len(xyz), args.views, args.height, args.width
  nw = (n + 63) // 64
  dev = torch.device("cuda", torch.cuda.current_device())
  w2c = sv.world_to_camera(poses)
  d_xyz, d_w2c = torch.from_numpy(xyz).to(dev), torch.from_numpy(w2c).to(dev)
  zbuf = torch.empty((F, H, W), dtype=torch.float32, device=dev)
  mask = torch.empty((F, nw), dtype=torch.int64, device=dev)
  start = torch.empty((F, nw), dtype=torch.int64, device=dev)
  offsets = torch.empty(F + 1, dtype=torch.int64, device=dev)
  pixels = torch.empty(F, dtype=torch.int64, device=dev)
  offs_h = (C.c_int64 * (F + 1))()
  rows = torch.empty(0, dtype=torch.int32, device=dev)
  st = cur_stream(dev)
  ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
  times = []
  for rep in range(args.reps + 2):
    ws, wsb = ws_args(lib.pcmi_views_visible_workspace_bytes(n, F), dev)
    ev[0].record()
    check(lib.pcmi_views_zbuffer(ptr(d_xyz), 3, n, ptr(d_w2c), F, *cam, args.splat, ptr(zbuf), st))
    ev[1].record()
    check(lib.pcmi_views_visible(ptr(d_xyz), 3, n, ptr(d_w2c), F, *cam, args.rel_tol, ptr(zbuf), ptr(mask), ptr(start), ptr(offsets), offs_h,
                                 ptr(pixels), ws, wsb, st))
    ev[2].record()
    total = int(offs_h[F])
    if rows.shape[0] != total:
      rows = torch.empty(total, dtype=torch.int32, device=dev)
    check(lib.pcmi_views_rows(ptr(mask), ptr(start), n, F, ptr(rows), st))
    ev[3].record()
    torch.cuda.synchronize()
    if rep >= 2:
      times.append([ev[k].elapsed_time(ev[k + 1]) for k in range(3)])
  tm = np.array(times)
  kernel_ms = {name: dict(median=float(np.median(tm[:, k])), min=float(tm[:, k].min())) for k, name in enumerate(("zbuffer", "visible", "rows"))}
  kernel_ms["sum"] = dict(median=float(np.median(tm.sum(1))), min=float(tm.sum(1).min()))
  res = dict(points=n, views=F, width=W, height=H, focal=args.focal, splat=args.splat, rel_tol=args.rel_tol, reps=args.reps,
             visible_rows=total, occupied_pixels=int(pixels.sum()), kernel_ms=kernel_ms, projections_per_s=F * n / (kernel_ms["sum"]["median"] * 1e-3),
             scan_generation_s=gen_s)
  got = dict(zbuf=zbuf.cpu().numpy(), rows=rows.cpu().numpy(), offsets=np.frombuffer(offs_h, dtype=np.int64).copy(), pixels=pixels.cpu().numpy())

  sv.process_scan(xyz, poses[:4], K, H, W, splat=args.splat, rel_tol=args.rel_tol, color=color)  # warm-up
  runs = []
  for _ in range(max(args.scan_reps, 1)):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = sv.process_scan(xyz, poses, K, H, W, splat=args.splat, rel_tol=args.rel_tol, color=color)
    runs.append(dict(r["gpu_s"], total=time.perf_counter() - t))
  V = len(r["frames"])
  res.update(process_scan_s={k: float(np.median([x[k] for x in runs])) for k in runs[0]}, kept_views=V, dropped=r["dropped"],
             kept_points=int(sum(len(p) for p in r["points"])), centroids=int(sum(len(c) for c in r["centroids"])),
             pairs_over_0_3=int(sum(max(r["M"][i, j], r["M"][j, i]) >= 0.3 for i in range(V) for j in range(i + 1, V))))

  if not args.no_ref:
    t = time.perf_counter()
    want = vr.render(xyz, w2c, K[0, 0], K[1, 1], K[0, 2], K[1, 2], H, W, 0.1, 10.0, args.splat, args.rel_tol)
    res["ref_s"] = time.perf_counter() - t
    res["bit_identical"] = bool(all(np.array_equal(got[k], want[k]) for k in got))
    res["ref_over_kernels"] = res["ref_s"] / (kernel_ms["sum"]["median"] * 1e-3)
  line = json.dumps(res)
  print(line, flush=True)
  if args.out:
    with open(args.out, "w") as f:
      f.write(line + "\n")
  if not args.no_ref and not res["bit_identical"]:
    sys.exit("scan_views_bench: the device output differs from the restatement")


if __name__ == "__main__":
  main()
