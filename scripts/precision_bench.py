"""fp32 against the opt-in bf16 conv precision mode (pcmi_set_conv_precision).

Stand-alone (HIP events on the launch stream, bench.time_kernel): the level-1 96->96 and 128->96 3^3 forward and
backward-data and the level-1 96->96 3^3 weight gradient at the configs[1] row count (both clouds of the bench batch as
one tensor, as the training step launches them), in both modes.  The step: `bench.py --set misc.conv_precision=MODE` in
child processes, PROCS per mode, interleaved; with --families one `--full` run per mode for families[] as well.
Prints one JSON line.  Usage on the GPU box:  python scripts/precision_bench.py [--procs 3] [--steps 60] [--families]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernels():
  import torch
  import bench
  import pointcontrast_amd.minkowski as ME
  from pointcontrast_amd._lib import lib, check
  from pointcontrast_amd.runtime import ptr, cur_stream, ws_args
  dev = torch.device("cuda:0")
  st = bench.level1_tensor(bench.get_batch(0, 4, 0.025), dev)
  cm, key = st.coords_man, st.coords_key
  m = cm.kernel_map(key, key, 3, 1, 3)
  n = cm.size(key)
  s = cur_stream(dev)
  out = {"rows": int(n)}
  for cin, cout in ((96, 96), (128, 96)):
    torch.manual_seed(0)
    x, g = torch.randn(n, cin, device=dev), torch.randn(n, cout, device=dev)
    W = torch.randn(27, cin, cout, device=dev) / (27 * cin) ** 0.5
    y, gin, gw = torch.empty(n, cout, device=dev), torch.empty(n, cin, device=dev), torch.empty_like(W)
    ws, wsb = ws_args(lib.pcmi_spconv_workspace_bytes(n, n, cin, cout, 27, m.M if m.M >= 0 else 27 * n), dev)
    legs = {
        "fwd": lambda: check(lib.pcmi_spconv_fwd(ptr(x), cin, n, cin, ptr(W), cout, C.byref(m), 0, None, ptr(y), cout, n,
                                                 ws, wsb, s)),
        "bwd_data": lambda: check(lib.pcmi_spconv_bwd_data(ptr(g), cout, n, cout, ptr(W), cin, C.byref(m), 0, ptr(gin), cin,
                                                           n, ws, wsb, s)),
    }
    if (cin, cout) == (96, 96):
      legs["wgrad"] = lambda: check(lib.pcmi_spconv_bwd_weight(ptr(x), cin, n, cin, ptr(g), cout, n, cout, C.byref(m), 0,
                                                               ptr(gw), None, ws, wsb, s))
    for leg, fn in legs.items():
      row = {}
      for mode in ("fp32", "bf16"):
        with ME.conv_precision(mode):
          row[mode + "_ms"] = round(bench.time_kernel(fn, iters=30, warm=5) * 1e3, 4)
      row["speedup"] = round(row["fp32_ms"] / row["bf16_ms"], 3)
      out["%d->%d %s" % (cin, cout, leg)] = row
      print("%-20s %s" % ("%d->%d %s" % (cin, cout, leg), row), file=sys.stderr, flush=True)
  return out


def bench_line(mode, steps, warmup, extra=()):
  cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
         "--set", "misc.conv_precision=%s" % mode] + list(extra)
  r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
  lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
  if r.returncode != 0 or not lines:
    raise RuntimeError("bench.py (%s) failed, rc %d: %s" % (mode, r.returncode, r.stderr[-2000:]))
  return json.loads(lines[-1])


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--procs", type=int, default=3, help="bench.py processes per mode (interleaved)")
  ap.add_argument("--steps", type=int, default=60)
  ap.add_argument("--warmup", type=int, default=10)
  ap.add_argument("--families", action="store_true", help="one bench.py --full per mode: families[]")
  ap.add_argument("--no-kernels", action="store_true")
  args = ap.parse_args()
  out = {"what": "conv precision fp32 vs bf16 (configs[1])"}
  if not args.no_kernels:
    out["kernels"] = kernels()
  step = {"fp32": [], "bf16": []}
  for _ in range(args.procs):
    for mode in ("fp32", "bf16"):
      d = bench_line(mode, args.steps, args.warmup)
      step[mode].append(d["value"])
      print("step %s: %s pairs/s" % (mode, d["value"]), file=sys.stderr, flush=True)
  out["step_pairs_per_s"] = step
  if all(step.values()):
    out["step_speedup_median"] = round(sorted(step["bf16"])[len(step["bf16"]) // 2] / sorted(step["fp32"])[len(step["fp32"]) // 2], 4)
  if args.families:
    fam = {}
    for mode in ("fp32", "bf16"):
      d = bench_line(mode, args.steps, args.warmup, ["--full", "--no-cpu-baseline", "--no-extra"])
      fam[mode] = [{"family": f.get("family"), "ms_per_step": f.get("ms_per_step")} for f in (d.get("families") or [])]
    out["families"] = fam
  print(json.dumps(out), flush=True)


if __name__ == "__main__":
  main()
