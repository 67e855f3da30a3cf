"""Pooling, unpooling, global pooling, broadcast and instance norm on the MI355X against the fp64 references of
tests/pool_ref.py (themselves pinned against dense torch by tests/test_pooling_surface.py), forward and every gradient;
a small eager network built from them; bit-reproducibility at full level-1 size."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pool_ref as R  # noqa: E402
from helpers import random_coords  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
POOL_TOL = 1e-5
NORM_TOL = 1e-4


def _coords(n=900, extent=12, seed=0, batches=(0, 3, 7)):
  """Shuffled rows, negative coordinates, non-contiguous batch indices."""
  c = random_coords(n, extent=extent, batch=len(batches), seed=seed)
  c[:, 0] = np.asarray(batches, dtype=np.int32)[c[:, 0]]
  return c


def _tensor(coords, feats, requires_grad=True):
  import pointcontrast_amd.minkowski as ME
  f = feats.to(DEV, torch.float32).requires_grad_(requires_grad)
  return ME.SparseTensor(f, coords=torch.from_numpy(coords).to(DEV)), f


def _on_key(feats, key, cm, requires_grad=True):
  import pointcontrast_amd.minkowski as ME
  f = feats.to(DEV, torch.float32).requires_grad_(requires_grad)
  return ME.SparseTensor(f, coords_key=key, coords_manager=cm), f


def _check(got, want, tol, what):
  e = R.rel_err(got, want)
  assert e <= tol, "%s: rel err %.3e > %.0e" % (what, e, tol)


def _pool_module(average, ks, stride, region):
  import pointcontrast_amd.minkowski as ME
  gen = ME.KernelGenerator(ks, stride, 1, region_type=ME.RegionType(region), dimension=3)
  cls = ME.MinkowskiAvgPooling if average else ME.MinkowskiSumPooling
  return cls(kernel_size=ks, stride=stride, kernel_generator=gen, dimension=3)


def _run_pool(st, f, cmr, ref_key, ref_out_key, nbr, average, mod, seed):
  """Device pooling of (st, f) against the reference; rows are matched by coordinates."""
  C = f.shape[1]
  out = mod(st)
  got_c, want_c = out.C.cpu().numpy(), cmr.coords[ref_out_key]
  p = R.align_rows(got_c, want_c)
  x64 = f.detach().double().cpu().requires_grad_(True)
  ref = R.pool(x64, nbr, average)
  _check(out.F.detach()[p.to(DEV)], ref, POOL_TOL, "pool fwd C=%d" % C)
  g = torch.randn(ref.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))
  gdev = torch.empty_like(out.F)
  gdev[p.to(DEV)] = g.to(DEV, torch.float32)
  out.F.backward(gdev)
  ref.backward(g)
  _check(f.grad, x64.grad, POOL_TOL, "pool bwd C=%d" % C)
  return out


@pytest.mark.parametrize("average", [False, True])
@pytest.mark.parametrize("ks, stride, region", [(2, 2, 0), (3, 1, 0), (3, 1, 3)])
@pytest.mark.parametrize("C", [1, 13, 32, 96, 256])
def test_pooling_matches_reference(average, ks, stride, region, C):
  from oracle.sparse_ref import CoordsManagerRef
  coords = _coords(seed=C + ks)
  gen = torch.Generator().manual_seed(C)
  st, f = _tensor(coords, torch.randn(len(coords), C, generator=gen))
  cmr = CoordsManagerRef(coords)
  out_key = cmr.stride(0, 2) if stride == 2 else 0
  nbr = cmr.kernel_map(0, out_key, ks, region).nbr
  _run_pool(st, f, cmr, 0, out_key, nbr, average, _pool_module(average, ks, stride, region), C)
  if stride == 2:  # level 2 -> 4, on the device's strided key
    cm = st.coords_man
    k1 = cm.stride(st.coords_key, 2)
    p1 = R.align_rows(cm.get_coords(k1).cpu().numpy(), cmr.coords[out_key])
    x1 = torch.randn(len(p1), C, generator=gen)
    xd = torch.empty_like(x1)
    xd[p1] = x1  # device row order
    st1, f1 = _on_key(xd, k1, cm)
    k2 = cmr.stride(out_key, 2)
    nbr2 = cmr.kernel_map(out_key, k2, 2).nbr
    out = _pool_module(average, 2, 2, 0)(st1)
    want = R.pool(x1.double(), nbr2, average)
    p2 = R.align_rows(out.C.cpu().numpy(), cmr.coords[k2])
    _check(out.F.detach()[p2.to(DEV)], want, POOL_TOL, "pool 2->4 fwd C=%d" % C)
    assert out.tensor_stride == [4, 4, 4]


def test_stride2_pooling_shares_the_conv_key():
  import pointcontrast_amd.minkowski as ME
  coords = _coords(seed=11)
  st, _ = _tensor(coords, torch.randn(len(coords), 8), requires_grad=False)
  pooled = ME.MinkowskiSumPooling(kernel_size=2, stride=2, dimension=3)(st)
  conv = ME.MinkowskiConvolution(8, 16, kernel_size=2, stride=2, dimension=3).to(DEV)
  y = conv(st)
  assert pooled.coords_key == y.coords_key
  cat = ME.cat(pooled, y)
  assert cat.F.shape == (len(pooled), 24) and cat.coords_key == y.coords_key


@pytest.mark.parametrize("cls_name", ["MinkowskiAvgUnpooling", "MinkowskiPoolingTranspose"])
@pytest.mark.parametrize("C", [13, 96])
def test_unpooling_onto_the_finer_key(cls_name, C):
  import pointcontrast_amd.minkowski as ME
  from oracle.sparse_ref import CoordsManagerRef
  coords = _coords(seed=5)
  st, _ = _tensor(coords, torch.randn(len(coords), C), requires_grad=False)
  cm = st.coords_man
  k1 = cm.stride(st.coords_key, 2)
  cmr = CoordsManagerRef(coords)
  r1 = cmr.stride(0, 2)
  p1 = R.align_rows(cm.get_coords(k1).cpu().numpy(), cmr.coords[r1])
  g = torch.randn(len(p1), C, dtype=torch.float64)
  gd = torch.empty_like(g)
  gd[p1] = g
  sc, fc = _on_key(gd, k1, cm)
  out = getattr(ME, cls_name)(kernel_size=2, stride=2, dimension=3)(sc)
  assert out.coords_key == st.coords_key
  g64 = g.clone().requires_grad_(True)
  want = R.unpool(g64, cmr.kernel_map(0, r1, 2).nbr, len(coords))
  _check(out.F.detach(), want, POOL_TOL, "unpool fwd")
  dy = torch.randn(want.shape, dtype=torch.float64)
  out.F.backward(dy.to(DEV, torch.float32))
  want.backward(dy)
  _check(fc.grad[p1.to(DEV)], g64.grad, POOL_TOL, "unpool bwd")


def _instance_coords(rng, n_rows_per_batch):
  rows = []
  for b, n in n_rows_per_batch.items():
    c = random_coords(n, extent=14, batch=1, seed=int(rng.randint(1 << 30)))
    c[:, 0] = b
    rows.append(c)
  c = np.concatenate(rows)
  return c[rng.permutation(len(c))]  # rows of the instances interleaved


def _full_level1_coords():
  import bench
  batch = bench.get_batch(0, 4, 0.025)
  C0, C1 = batch["sinput0_C"].numpy(), batch["sinput1_C"].numpy().copy()
  C1[:, 0] += int(C0[:, 0].max()) + 1
  c = np.concatenate([C0, C1, np.array([[1000, 0, 0, 0]], dtype=np.int32)])  # plus a one-row instance
  return c[np.random.RandomState(0).permutation(len(c))]


@pytest.mark.parametrize("case", ["small", "full"])
@pytest.mark.parametrize("C", [13, 96])
def test_global_pooling_and_broadcast(case, C):
  import pointcontrast_amd.minkowski as ME
  if case == "small":
    coords = _instance_coords(np.random.RandomState(C), {0: 1, 3: 500, 7: 37, 9: 2})
  else:
    coords = _full_level1_coords()
  b = coords[:, 0]
  gen = torch.Generator().manual_seed(C)
  x = torch.randn(len(coords), C, generator=gen, dtype=torch.float64)
  uniq = np.unique(b)
  for average in (True, False):
    st, f = _tensor(coords, x)
    out = ME.MinkowskiGlobalPooling(average=average)(st)
    oc = out.C.cpu().numpy()
    assert (oc[:, 0] == uniq).all() and (oc[:, 1:] == 0).all() and out.tensor_stride == [0, 0, 0]
    x64 = x.clone().requires_grad_(True)
    want = R.global_pool(x64, b, average)
    _check(out.F.detach(), want, POOL_TOL, "global pool fwd (average=%s)" % average)
    dy = torch.randn(want.shape, dtype=torch.float64, generator=gen)
    out.F.backward(dy.to(DEV, torch.float32))
    want.backward(dy)
    _check(f.grad, x64.grad, POOL_TOL, "global pool bwd (average=%s)" % average)
  for op, cls in (("add", ME.MinkowskiBroadcastAddition), ("mul", ME.MinkowskiBroadcastMultiplication)):
    st, f = _tensor(coords, x)
    cm = st.coords_man
    gv = torch.randn(len(uniq), C, generator=gen, dtype=torch.float64)
    sg, fg = _on_key(gv, cm.origin_key(), cm)
    out = cls(dimension=3)(st, sg)
    assert out.coords_key == st.coords_key
    x64, g64 = x.clone().requires_grad_(True), gv.clone().requires_grad_(True)
    want = R.broadcast(x64, g64, b, op)
    _check(out.F.detach(), want, POOL_TOL, "broadcast %s fwd" % op)
    dy = torch.randn(want.shape, dtype=torch.float64, generator=gen)
    out.F.backward(dy.to(DEV, torch.float32))
    want.backward(dy)
    _check(f.grad, x64.grad, POOL_TOL, "broadcast %s dx" % op)
    _check(fg.grad, g64.grad, POOL_TOL, "broadcast %s dg" % op)


def test_cpu_tensor_raises_on_the_device_path():
  from pointcontrast_amd import functional as PF
  from pointcontrast_amd._lib import PcmiError
  import pointcontrast_amd.minkowski as ME
  coords = _coords(seed=2)
  st, _ = _tensor(coords, torch.randn(len(coords), 4), requires_grad=False)
  seg = st.coords_man.segments(st.coords_key)
  with pytest.raises(PcmiError):
    PF.GlobalPoolFunction.apply(torch.randn(len(coords), 4), seg, True)
  assert isinstance(seg.n_inst, int) and seg.n_inst == 3
  assert ME.MinkowskiGlobalPooling()(st).C.shape == (3, 4)


def test_small_eager_network_matches_fp64_oracle():
  """conv -> IN + ReLU -> sum_pool(2, 2) -> conv -> global average pool, forward and every parameter gradient."""
  import pointcontrast_amd.minkowski as ME
  from oracle.sparse_ref import CoordsManagerRef, sparse_conv
  torch.manual_seed(0)
  coords = _instance_coords(np.random.RandomState(4), {0: 700, 2: 400, 5: 1})
  b = coords[:, 0]
  x = torch.randn(len(coords), 3, dtype=torch.float64)
  conv1 = ME.MinkowskiConvolution(3, 32, kernel_size=3, stride=1, dimension=3).to(DEV)
  norm = ME.MinkowskiInstanceNorm(32, D=3).to(DEV)
  with torch.no_grad():
    norm.weight.uniform_(0.5, 1.5)
    norm.bias.uniform_(-0.2, 0.2)
  pool = ME.MinkowskiSumPooling(kernel_size=2, stride=2, dimension=3)
  conv2 = ME.MinkowskiConvolution(32, 16, kernel_size=3, stride=1, dimension=3).to(DEV)
  gpool = ME.MinkowskiGlobalPooling(average=True)
  st, _ = _tensor(coords, x, requires_grad=False)
  out = gpool(conv2(pool(norm(conv1(st), relu=True))))
  G = torch.randn(out.F.shape, dtype=torch.float64)
  (out.F * G.to(DEV, torch.float32)).sum().backward()

  cmr = CoordsManagerRef(coords)
  k1 = cmr.stride(0, 2)
  P = {n: p.detach().double().cpu().requires_grad_(True) for n, p in
       (("w1", conv1.kernel), ("nw", norm.weight), ("nb", norm.bias), ("w2", conv2.kernel))}
  h = sparse_conv(x, P["w1"], cmr.kernel_map(0, 0, 3))
  h = R.instance_norm(h, b, P["nw"], P["nb"], relu=True)
  h = R.pool(h, cmr.kernel_map(0, k1, 2).nbr, False)
  h = sparse_conv(h, P["w2"], cmr.kernel_map(k1, k1, 3))
  ref = R.global_pool(h, cmr.coords[k1][:, 0], True)
  (ref * G).sum().backward()
  _check(out.F.detach(), ref, NORM_TOL, "network output")
  for n, p in (("w1", conv1.kernel), ("nw", norm.weight), ("nb", norm.bias), ("w2", conv2.kernel)):
    _check(p.grad, P[n].grad, NORM_TOL, "network grad %s" % n)


def test_every_new_op_is_bit_reproducible_at_full_size():
  import pointcontrast_amd.minkowski as ME
  coords = _full_level1_coords()
  C = 96
  x = torch.randn(len(coords), C, generator=torch.Generator().manual_seed(0))
  norm = ME.MinkowskiInstanceNorm(C, D=3).to(DEV)
  with torch.no_grad():
    norm.weight.uniform_(0.5, 1.5)

  def run():
    st, f = _tensor(coords, x)
    cm = st.coords_man
    a = _pool_module(True, 3, 1, 3)(st)
    s2 = ME.MinkowskiSumPooling(kernel_size=2, stride=2, dimension=3)(st)
    u = ME.MinkowskiAvgUnpooling(kernel_size=2, stride=2, dimension=3)(s2)
    g = ME.MinkowskiGlobalPooling(average=True)(st)
    m = ME.MinkowskiBroadcastMultiplication(dimension=3)(a, g)
    y = norm(m, residual=u, relu=True)
    gs = ME.MinkowskiGlobalPooling(average=False)(y)
    loss = (y.F * y.F).sum() + (gs.F * torch.linspace(-1, 1, C, device=DEV)).sum()
    norm.weight.grad = norm.bias.grad = None
    loss.backward()
    torch.cuda.synchronize()
    del cm
    return [t.detach().clone() for t in (a.F, s2.F, u.F, g.F, m.F, y.F, gs.F, f.grad, norm.weight.grad, norm.bias.grad)]

  r0, r1 = run(), run()
  for i, (p, q) in enumerate(zip(r0, r1)):
    assert torch.equal(p, q), "output %d differs between two runs" % i
