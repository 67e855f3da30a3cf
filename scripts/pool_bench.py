"""Micro-benchmark of the pooling / per-instance kernels (csrc/pool.hip) on the real maps of the bench batch, with
BatchNorm on the same shape for comparison (HIP events on the launch stream).  Prints achieved GB/s of algorithmic
bytes (every input read once, every output written once) against the ~6.3 TB/s achievable HBM rate.  Usage on the GPU
box:  python scripts/pool_bench.py"""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
import pointcontrast_amd.minkowski as ME
from pointcontrast_amd._lib import lib, check
from pointcontrast_amd.runtime import ptr, cur_stream, ws_args

HBM = 6.3e12
dev = torch.device("cuda:0")
batch = bench.get_batch(0, 4, 0.025)
st = bench.level1_tensor(batch, dev)  # as the training step: both clouds of the pair, 8 instances
cm = st.coords_man
keys = [st.coords_key]
for _ in range(2):
  keys.append(cm.stride(keys[-1], 2))
s = cur_stream(dev)
print("rows", [cm.size(k) for k in keys], flush=True)


def row(label, fn, nbytes):
  t = bench.time_kernel(fn, iters=20, warm=3)
  print("%-40s %8.1f us  %7.0f GB/s  %5.1f %% of HBM" % (label, t * 1e6, nbytes / t * 1e-9, 100 * nbytes / t / HBM),
        flush=True)
  return t


def pool_rows(lvl_in, lvl_out, ks, stride, region, c):
  m = cm.kernel_map(keys[lvl_in], keys[lvl_out], ks, stride, region)
  x, g = torch.randn(m.n_in, c, device=dev), torch.randn(m.n_out, c, device=dev)
  y, gin = torch.empty(m.n_out, c, device=dev), torch.empty(m.n_in, c, device=dev)
  ws, wsb = ws_args(lib.pcmi_pool_workspace_bytes(m.n_out), dev)
  mb = (m.n_in + m.n_out) * c * 4 + 4 * m.K * m.n_out
  tag = "ts%d->%d k%d/s%d C=%d" % (2 ** lvl_in, 2 ** lvl_out, ks, stride, c)
  for avg in (0, 1):
    name = ("avg " if avg else "sum ") + tag
    row(name + " fwd", lambda: check(lib.pcmi_pool_fwd(ptr(x), c, c, C.byref(m), avg, ptr(y), c, s)), mb)
    row(name + " bwd", lambda: check(lib.pcmi_pool_bwd(ptr(g), c, c, C.byref(m), avg, ptr(gin), c, ws, wsb, s)), mb)


pool_rows(0, 1, 2, 2, 0, 96)
pool_rows(1, 2, 2, 2, 0, 96)
pool_rows(0, 0, 3, 1, 3, 96)

c = 96
n = cm.size(keys[0])
seg = cm.segments(keys[0])
print("instances", seg.n_inst, "chunks", seg.n_chunks, flush=True)
x, dy, res = (torch.randn(n, c, device=dev) for _ in range(3))
y, dx, dres = (torch.empty(n, c, device=dev) for _ in range(3))
w, b = torch.rand(c, device=dev) + 0.5, torch.randn(c, device=dev)
gout = torch.empty(seg.n_inst, c, device=dev)
mean, invstd = torch.empty(seg.n_inst, c, device=dev), torch.empty(seg.n_inst, c, device=dev)
dw, db = torch.empty(c, device=dev), torch.empty(c, device=dev)
sr = C.byref(seg)
ws, wsb = ws_args(max(lib.pcmi_segments_workspace_bytes(sr, c), lib.pcmi_bn_workspace_bytes(n, c)), dev)
nb = n * c * 4
row("global avg pool fwd C=96", lambda: check(lib.pcmi_global_pool_fwd(ptr(x), c, c, sr, 1, ptr(gout), c, ws, wsb, s)), nb)
row("global avg pool bwd C=96", lambda: check(lib.pcmi_global_pool_bwd(ptr(gout), c, c, sr, 1, ptr(dx), c, s)), nb)
row("broadcast mul fwd C=96", lambda: check(lib.pcmi_broadcast_fwd(ptr(x), c, ptr(gout), c, c, sr, 1, ptr(y), c, s)), 2 * nb)
row("broadcast mul bwd C=96", lambda: check(lib.pcmi_broadcast_bwd(ptr(dy), c, ptr(x), c, ptr(gout), c, c, sr, 1, ptr(dx), c,
                                                                    ptr(mean), c, ws, wsb, s)), 4 * nb)
# fused residual + ReLU, as in a block: fwd reads x, res, writes y; bwd reads dy, x, y, writes dx, dres
t_in_f = row("instance norm fwd (+res, relu) C=96", lambda: check(lib.pcmi_instnorm_fwd(
    ptr(x), c, c, sr, ptr(w), ptr(b), 1e-5, ptr(res), c, 1, ptr(y), c, ptr(mean), ptr(invstd), ws, wsb, s)), 3 * nb)
t_in_b = row("instance norm bwd (+res, relu) C=96", lambda: check(lib.pcmi_instnorm_bwd(
    ptr(dy), c, ptr(x), c, ptr(y), c, c, sr, ptr(w), ptr(mean), ptr(invstd), ptr(dx), c, ptr(dres), c, ptr(dw), ptr(db),
    ws, wsb, s)), 5 * nb)
rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
bm, bi = torch.empty(c, device=dev), torch.empty(c, device=dev)
t_bn_f = row("batch norm fwd (+res, relu) C=96", lambda: check(lib.pcmi_bn_fwd_train(
    ptr(x), c, n, c, ptr(w), ptr(b), ptr(rm), ptr(rv), 0.1, 1e-5, ptr(res), c, 1, ptr(y), c, ptr(bm), ptr(bi), ws, wsb, s)),
    3 * nb)
t_bn_b = row("batch norm bwd (+res, relu) C=96", lambda: check(lib.pcmi_bn_bwd(
    ptr(dy), c, ptr(x), c, ptr(y), c, n, c, ptr(w), ptr(bm), ptr(bi), ptr(dx), c, ptr(dres), c, ptr(dw), ptr(db), ws, wsb,
    s)), 5 * nb)
print("instance norm / batch norm: fwd %.2fx, bwd %.2fx" % (t_in_f / t_bn_f, t_in_b / t_bn_b), flush=True)
