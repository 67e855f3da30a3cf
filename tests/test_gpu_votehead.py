"""The row-major VoteNet head kernels (csrc/votehead.hip) and pcmi_net_set_bn_momentum on the MI355X: group_rows, rows_maxpool,
vote, adam.  Forward results that are individually rounded fp32 operations are compared exactly with numpy float32; float
results within 1e-4 of float64 relative to the tensor's largest entry (pointset_ref.rel_err, the bound every kernel of this
library is held to); backward passes bit-identical between two runs."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointset_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-4
F32 = np.float32
RADIUS = 0.3
PCMI_ERR_INVALID, PCMI_ERR_RANGE, PCMI_ERR_UNSUPPORTED, PCMI_ERR_WORKSPACE = -1, -5, -6, -7


def _dev(a, dtype=None):
  t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
  return t if dtype is None else t.to(dtype)


def _pad4(c):
  return (c + 3) // 4 * 4


# ---- group_rows ---------------------------------------------------------------------------------------------------------
B, N, NP = 2, 40, 5


def _group_geometry():
  """xyz [2, 40, 3] and centres [2, 5, 3].  Scene 0: point 0 lies within the radius of centres 0..3 (their first hit), six
  more points lie near them (fewer than 16 hits: the first hit is repeated), the rest is far away, and centre 4 is far from
  everything (no hit: zeros, i.e. point 0 again) -- so point 0 is the first hit of EVERY centre and has the longest inverse
  list.  Scene 1: a random cloud with centres on some of its points."""
  rng = np.random.RandomState(11)
  xyz = np.zeros((B, N, 3), F32)
  ctr = np.zeros((B, NP, 3), F32)
  p0 = np.array([1.5, 1.5, 1.5], F32)
  xyz[0, 0] = p0
  ctr[0, :4] = p0 + rng.uniform(-0.05, 0.05, (4, 3)).astype(F32)
  xyz[0, 1:7] = p0 + rng.uniform(-0.12, 0.12, (6, 3)).astype(F32)
  xyz[0, 7:] = p0 + 2.0 + rng.uniform(0, 1, (N - 7, 3)).astype(F32)
  ctr[0, 4] = p0 - 3.0
  xyz[1] = (1.5 + rng.uniform(-0.4, 0.4, (N, 3))).astype(F32)
  ctr[1] = xyz[1, [3, 9, 17, 25, 39]] + F32(0.01)
  return xyz, ctr


XYZ, CTR = _group_geometry()


def _idx(ns):
  from pointcontrast_amd import functional as PF
  got = PF.BallQueryFunction.apply(RADIUS, ns, _dev(XYZ), _dev(CTR))
  want = R.ball_query(XYZ, CTR, RADIUS, ns)
  assert np.array_equal(got.cpu().numpy(), want)
  return want


def _group_fwd_ref(feat, idx, radius_div, out_ld):
  """numpy float32, each operation rounded on its own; an index outside [0, N) gives a zero row."""
  ns = idx.shape[2]
  Cc = feat.shape[1]
  out = np.zeros((B * NP * ns, out_ld), F32)
  for b in range(B):
    for q in range(NP):
      for s in range(ns):
        t, r = idx[b, q, s], (b * NP + q) * ns + s
        if 0 <= t < N:
          out[r, :Cc] = feat[b * N + t]
          out[r, Cc:Cc + 3] = (XYZ[b, t] - CTR[b, q]) / F32(radius_div)
  return out


def _group_bwd_ref(gout, idx, Cc, radius_div):
  """float64: (gfeat [B N, C], gxyz [B, N, 3], gcentre [B, NP, 3])."""
  ns = idx.shape[2]
  g = gout.astype(np.float64)
  gfeat, gxyz, gctr = np.zeros((B * N, Cc)), np.zeros((B, N, 3)), np.zeros((B, NP, 3))
  for b in range(B):
    for q in range(NP):
      for s in range(ns):
        t, r = idx[b, q, s], (b * NP + q) * ns + s
        if 0 <= t < N:
          gfeat[b * N + t] += g[r, :Cc]
          gxyz[b, t] += g[r, Cc:Cc + 3] / radius_div
          gctr[b, q] -= g[r, Cc:Cc + 3] / radius_div
  return gfeat, gxyz, gctr


@pytest.mark.parametrize("C_", [0, 5, 32, 256])
@pytest.mark.parametrize("ns", [1, 3, 16])
def test_group_rows_forward_exact_and_backward(C_, ns):
  from pointcontrast_amd import functional as PF
  rng = np.random.RandomState(100 * ns + C_)
  idx = _idx(ns)
  if ns == 16:
    uniq = [len(set(r)) for r in idx.reshape(-1, ns)]
    assert min(uniq) == 1 and 1 < sorted(uniq)[1] < ns  # a centre without a hit, centres with fewer than ns hits
    assert (idx[0, :, 0] == 0).all()  # point 0 is the first hit of every centre of scene 0
  feat = rng.normal(0, 1, (B * N, C_)).astype(F32)
  for out_ld, radius_div in ((_pad4(C_ + 3), RADIUS), (_pad4(C_ + 3) + 8, 1.0), ((C_ + 3 + 31) // 32 * 32, RADIUS)):
    xyz, ctr = _dev(XYZ).requires_grad_(True), _dev(CTR).requires_grad_(True)
    f = _dev(feat).requires_grad_(True) if C_ else None
    out = PF.GroupRowsFunction.apply(xyz, ctr, f, _dev(idx), radius_div, out_ld)
    assert out.shape == (B * NP * ns, out_ld)
    want = _group_fwd_ref(feat, idx, radius_div, out_ld)
    assert np.array_equal(out.detach().cpu().numpy(), want), "forward differs (C %d, ns %d, ld %d)" % (C_, ns, out_ld)
    assert not out.detach()[:, C_ + 3:].any()  # the pad columns
    gout = rng.normal(0, 1, (B * NP * ns, out_ld)).astype(F32)
    grads = torch.autograd.grad(out, [xyz, ctr] + ([f] if C_ else []), _dev(gout))
    again = torch.autograd.grad(PF.GroupRowsFunction.apply(xyz, ctr, f, _dev(idx), radius_div, out_ld), [xyz, ctr] + ([f] if C_ else []),
                                _dev(gout))
    gfeat, gxyz, gctr = _group_bwd_ref(gout, idx, C_, radius_div)
    assert R.rel_err(grads[0], gxyz) <= TOL and R.rel_err(grads[1], gctr) <= TOL
    if C_:
      assert grads[2].shape == (B * N, C_) and R.rel_err(grads[2], gfeat) <= TOL
    for a, b in zip(grads, again):
      assert torch.equal(a, b), "the backward pass is not bit-identical between two runs"


@pytest.mark.parametrize("C_", [5, 32])
def test_group_rows_out_of_range_index(C_):
  from pointcontrast_amd import functional as PF
  from pointcontrast_amd._lib import PcmiError
  rng = np.random.RandomState(C_)
  ns, out_ld = 3, _pad4(C_ + 3)
  idx = _idx(ns).copy()
  idx[0, 1, 2], idx[1, 4, 0], idx[1, 0, 1] = -1, N, 2 ** 31 - 1
  feat = rng.normal(0, 1, (B * N, C_)).astype(F32)
  with pytest.raises(PcmiError):
    PF.GroupRowsFunction.apply(_dev(XYZ), _dev(CTR), _dev(feat), _dev(idx), RADIUS, out_ld)  # validate: refused
  xyz, ctr, f = _dev(XYZ).requires_grad_(True), _dev(CTR).requires_grad_(True), _dev(feat).requires_grad_(True)
  out = PF.GroupRowsFunction.apply(xyz, ctr, f, _dev(idx), RADIUS, out_ld, False)  # no validation: no error
  want = _group_fwd_ref(feat, idx, RADIUS, out_ld)
  assert np.array_equal(out.detach().cpu().numpy(), want)
  for r in ((0 * NP + 1) * ns + 2, (1 * NP + 4) * ns + 0, (1 * NP + 0) * ns + 1):
    assert not want[r].any() and not out.detach()[r].any()  # a zero row
  gout = rng.normal(0, 1, out.shape).astype(F32)
  gxyz, gctr, gfeat = torch.autograd.grad(out, [xyz, ctr, f], _dev(gout))
  wf, wx, wc = _group_bwd_ref(gout, idx, C_, RADIUS)  # the three rows are dropped from all three gradients
  assert R.rel_err(gfeat, wf) <= TOL and R.rel_err(gxyz, wx) <= TOL and R.rel_err(gctr, wc) <= TOL


def test_group_rows_c_entry_exact_workspace_and_refusals():
  from pointcontrast_amd._lib import lib
  from c_contract import Guarded
  rng = np.random.RandomState(5)
  ns, C_ = 16, 32
  out_ld = 64
  idx = _dev(_idx(ns))
  rows = B * NP * ns
  gout = _dev(rng.normal(0, 1, (rows, out_ld)).astype(F32))
  need = lib.pcmi_group_rows_bwd_workspace_bytes(B, N, NP, ns)
  assert need > 0
  ws = Guarded(need)
  gfeat = torch.full((B * N, C_), float("nan"), device=DEV)
  gxyz = torch.full((B, N, 3), float("nan"), device=DEV)
  gctr = torch.full((B, NP, 3), float("nan"), device=DEV)
  st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
  p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
  # one byte short: refused, nothing enqueued
  rc = lib.pcmi_group_rows_bwd(p(gout), out_ld, p(idx), B, N, NP, ns, C_, RADIUS, p(gfeat), C_, p(gxyz), p(gctr), ws.vp, C.c_size_t(need - 1), st)
  torch.cuda.synchronize()
  assert rc == PCMI_ERR_WORKSPACE and bool(torch.isnan(gfeat).all()) and bool(torch.isnan(gxyz).all()) and bool(torch.isnan(gctr).all())
  rc = lib.pcmi_group_rows_bwd(p(gout), out_ld, p(idx), B, N, NP, ns, C_, RADIUS, p(gfeat), C_, p(gxyz), p(gctr), ws.vp, ws.size, st)
  torch.cuda.synchronize()
  assert rc == 0
  ws.check("group_rows_bwd")
  wf, wx, wc = _group_bwd_ref(gout.cpu().numpy(), idx.cpu().numpy(), C_, RADIUS)
  assert R.rel_err(gfeat, wf) <= TOL and R.rel_err(gxyz, wx) <= TOL and R.rel_err(gctr, wc) <= TOL
  # out_ld below C + 3, or not a multiple of 4: PCMI_ERR_INVALID, the output untouched
  out = torch.full((rows, out_ld), float("nan"), device=DEV)
  feat = _dev(rng.normal(0, 1, (B * N, C_)).astype(F32))
  for bad_ld in (C_, C_ + 3, C_ + 6):
    rc = lib.pcmi_group_rows_fwd(p(_dev(XYZ)), p(_dev(CTR)), p(feat), C_, p(idx), B, N, NP, ns, C_, RADIUS, p(out), bad_ld, 0, st)
    assert rc == PCMI_ERR_INVALID
  torch.cuda.synchronize()
  assert bool(torch.isnan(out).all())


# ---- rows_maxpool -------------------------------------------------------------------------------------------------------
def _maxpool_ref(x, ns):
  """(values, arguments): the lowest row among equals; a NaN wins, the lowest NaN row is the argument."""
  R_, C_ = x.shape[0] // ns, x.shape[1]
  w = x.reshape(R_, ns, C_)
  out, arg = np.zeros((R_, C_), F32), np.zeros((R_, C_), np.uint8)
  for r in range(R_):
    for c in range(C_):
      col = w[r, :, c]
      nan = np.isnan(col)
      a = int(np.argmax(nan)) if nan.any() else int(np.argmax(col))  # argmax returns the first maximum
      out[r, c], arg[r, c] = col[a], a
  return out, arg


@pytest.mark.parametrize("C_", [1, 128, 130])
@pytest.mark.parametrize("ns", [1, 3, 16, 256])
@pytest.mark.parametrize("R_", [1, 7])
def test_rows_maxpool(R_, ns, C_):
  from pointcontrast_amd import functional as PF
  rng = np.random.RandomState(R_ * 1000 + ns * 10 + C_)
  x = np.maximum(rng.normal(0, 1, (R_ * ns, C_)), 0).astype(F32)  # ReLU output: many exact zeros
  w = x.reshape(R_, ns, C_)
  if ns > 1:
    w[:, ns // 2:] = w[:, :1]  # ball-query padding: the first row repeated
    w[:, :, 0] = 0  # an all-zero column
    if C_ > 1:
      w[0, 1:, C_ - 1] = np.nan  # NaNs: the lowest NaN row is the argument
      w[R_ - 1, ns - 1, 1] = np.nan
  xt = _dev(x).requires_grad_(True)
  out, arg = PF.rows_maxpool(xt.detach(), ns)
  wv, wa = _maxpool_ref(x, ns)
  assert arg.dtype == torch.uint8 and np.array_equal(arg.cpu().numpy(), wa)
  assert np.array_equal(out.cpu().numpy(), wv, equal_nan=True)
  y = PF.RowsMaxPoolFunction.apply(xt, ns)
  assert np.array_equal(y.detach().cpu().numpy(), wv, equal_nan=True)
  gout = rng.normal(0, 1, (R_, C_)).astype(F32)
  (gx,) = torch.autograd.grad(y, [xt], _dev(gout))
  want = np.zeros((R_, ns, C_), F32)
  np.put_along_axis(want, wa[:, None, :].astype(np.int64), gout[:, None, :], 1)
  assert np.array_equal(gx.cpu().numpy(), want.reshape(R_ * ns, C_))


def test_rows_maxpool_refuses_more_than_256_rows():
  from pointcontrast_amd import functional as PF
  from pointcontrast_amd._lib import lib, PcmiError
  x = torch.zeros((257, 4), device=DEV)
  with pytest.raises(PcmiError):
    PF.rows_maxpool(x, 257)
  out, arg = torch.full((1, 4), float("nan"), device=DEV), torch.full((1, 4), 7, dtype=torch.uint8, device=DEV)
  st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
  for ns in (0, 257):
    rc = lib.pcmi_rows_maxpool_fwd(C.c_void_p(x.data_ptr()), 4, 1, ns, 4, C.c_void_p(out.data_ptr()), 4, C.c_void_p(arg.data_ptr()), st)
    assert rc == PCMI_ERR_UNSUPPORTED
    rc = lib.pcmi_rows_maxpool_bwd(C.c_void_p(out.data_ptr()), 4, C.c_void_p(arg.data_ptr()), 1, ns, 4, C.c_void_p(x.data_ptr()), 4, st)
    assert rc == PCMI_ERR_UNSUPPORTED
  torch.cuda.synchronize()
  assert bool(torch.isnan(out).all()) and bool((arg == 7).all())


# ---- vote -----------------------------------------------------------------------------------------------------------------
def _vote_ref(net, seed_xyz, seed_feat, vf, Cc, Wb):
  """float64 torch: (vote_xyz [R vf, 3], vote_feat [R vf, C])."""
  R_ = net.shape[0]
  blocks = net[:, :vf * Wb].reshape(R_, vf, Wb)
  u = seed_feat.unsqueeze(1) + blocks[:, :, :Cc]
  y = u / u.norm(dim=2, keepdim=True)
  return (seed_xyz.unsqueeze(1) + blocks[:, :, Cc:Cc + 3]).reshape(R_ * vf, 3), y.reshape(R_ * vf, Cc)


@pytest.mark.parametrize("R_", [1, 65])
@pytest.mark.parametrize("C_", [5, 32, 256])
@pytest.mark.parametrize("vf", [1, 2])
def test_vote_forward_and_backward(vf, C_, R_):
  from pointcontrast_amd import functional as PF
  rng = np.random.RandomState(vf * 7 + C_ + R_)
  Wb = (C_ + 3 + 31) // 32 * 32
  net = rng.normal(0, 1, (R_, vf * Wb)).astype(F32)
  sx, sf = rng.normal(0, 1, (R_, 3)).astype(F32), rng.normal(0, 1, (R_, C_)).astype(F32)
  tn, tx, tf = (_dev(a).requires_grad_(True) for a in (net, sx, sf))
  vx, vfeat = PF.VoteFunction.apply(tn, tx, tf, vf)
  dn, dx, df = (torch.from_numpy(a).double().requires_grad_(True) for a in (net, sx, sf))
  wx, wf = _vote_ref(dn, dx, df, vf, C_, Wb)
  assert vx.shape == (R_ * vf, 3) and vfeat.shape == (R_ * vf, C_)
  assert R.rel_err(vx, wx) <= TOL and R.rel_err(vfeat, wf) <= TOL
  gx, gf = rng.normal(0, 1, (R_ * vf, 3)).astype(F32), rng.normal(0, 1, (R_ * vf, C_)).astype(F32)
  got = torch.autograd.grad([vx, vfeat], [tn, tx, tf], [_dev(gx), _dev(gf)])
  vx2, vf2 = PF.VoteFunction.apply(tn, tx, tf, vf)
  again = torch.autograd.grad([vx2, vf2], [tn, tx, tf], [_dev(gx), _dev(gf)])
  want = torch.autograd.grad([wx, wf], [dn, dx, df], [torch.from_numpy(gx).double(), torch.from_numpy(gf).double()])
  for name, a, w in zip(("g_net", "g_seed_xyz", "g_seed_feat"), got, want):
    assert a.shape == w.shape and R.rel_err(a, w) <= TOL, (name, R.rel_err(a, w))
  for a, b in zip(got, again):
    assert torch.equal(a, b)
  g_net = got[0].cpu().numpy().reshape(R_, vf, Wb)
  assert not g_net[:, :, C_ + 3:].any()  # the pad columns of every block
  assert torch.equal(vx, vx2) and torch.equal(vfeat, vf2)


def test_vote_zero_row_gives_the_reference_nan():
  from pointcontrast_amd import functional as PF
  net, sf = torch.zeros((2, 64), device=DEV), torch.zeros((2, 32), device=DEV)
  sf[1] = 1.0
  _, vfeat = PF.VoteFunction.apply(net, torch.zeros((2, 3), device=DEV), sf, 1)
  assert bool(torch.isnan(vfeat[0]).all()) and bool(torch.isfinite(vfeat[1]).all())  # 0 / 0, no epsilon


# ---- adam -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
@pytest.mark.parametrize("n", [1, 1025, 4099])
def test_adam_step_matches_torch(n, weight_decay):
  """Reference: torch.optim.Adam in float64.  Bound: the device's error is at most twice the error of torch.optim.Adam in fp32
  on the CPU against that same float64 run, plus one fp32 ulp of the weights."""
  from pointcontrast_amd import functional as PF
  rng = np.random.RandomState(n)
  w0 = rng.normal(0, 1, n).astype(F32)
  grads = [rng.normal(0, 1, n).astype(F32) * F32(10.0 ** rng.randint(-3, 2)) for _ in range(3)]
  lr, betas, eps = 1e-3, (0.9, 0.999), 1e-8
  p64 = torch.nn.Parameter(torch.from_numpy(w0).double())
  p32 = torch.nn.Parameter(torch.from_numpy(w0).clone())
  o64 = torch.optim.Adam([p64], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
  o32 = torch.optim.Adam([p32], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
  w, m, v = _dev(w0), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
  for step, g in enumerate(grads, 1):
    p64.grad, p32.grad = torch.from_numpy(g).double(), torch.from_numpy(g).clone()
    o64.step()
    o32.step()
    gd = _dev(g)
    PF.adam_step(w, gd, m, v, lr, betas, eps, weight_decay, step)
    assert np.array_equal(gd.cpu().numpy(), g)  # the gradient is not modified
    err_dev = float((w.double().cpu() - p64.data).abs().max())
    err_cpu = float((p32.data.double() - p64.data).abs().max())
    ulp = float(np.spacing(F32(p64.data.abs().max())))
    print("adam n=%d wd=%g step %d: device error %.3e, torch fp32 CPU error %.3e, ulp %.3e" % (n, weight_decay, step, err_dev, err_cpu, ulp))
    assert err_dev <= 2 * err_cpu + ulp
    st = o64.state[p64]
    assert R.rel_err(m, st["exp_avg"]) <= TOL and R.rel_err(v, st["exp_avg_sq"]) <= TOL


def test_flat_adam_matches_the_kernel_and_round_trips():
  from pointcontrast_amd import functional as PF
  from pointcontrast_amd.lib.distributed import FlatParameters
  from pointcontrast_amd.lib.solver import FlatAdam
  torch.manual_seed(0)
  params = [torch.nn.Parameter(torch.randn(s, device=DEV)) for s in ((5, 7), (3,), (129,))]
  flat = FlatParameters(params)
  opt = FlatAdam(flat, lr=1e-3, weight_decay=1e-2)
  w, m, v = flat.w.clone(), torch.zeros_like(flat.w), torch.zeros_like(flat.w)
  for step in (1, 2):
    opt.zero_grad()
    for p in params:  # (the alignment padding between two parameters belongs to none of them and stays zero)
      p.grad.copy_(torch.randn_like(p))
    PF.adam_step(w, flat.g, m, v, 1e-3, (0.9, 0.999), 1e-8, 1e-2, step)
    if step == 2:
      opt.step_range(8, 40)  # a step taken in slices is the step taken in one launch
    opt.step()
    assert torch.equal(flat.w, w) and torch.equal(opt.m, m) and torch.equal(opt.v, v)
    assert torch.equal(params[0].data.reshape(-1), w[:35])  # the parameters are views of the flat buffer
  sd = opt.state_dict()
  assert sd["param_groups"][0]["lr"] == 1e-3 and float(sd["state"][0]["step"]) == 2
  flat2 = FlatParameters([torch.nn.Parameter(p.detach().clone()) for p in params])
  opt2 = FlatAdam(flat2, lr=5e-4)
  opt2.load_state_dict(sd)
  assert opt2.steps == 2 and torch.equal(opt2.m, opt.m) and torch.equal(opt2.v, opt.v) and opt2.param_groups[0]["lr"] == 1e-3
  for p, q in zip(flat.params, flat2.params):
    p.grad.copy_(torch.randn_like(p))
    q.grad.copy_(p.grad)
  opt.step()
  opt2.step()
  assert torch.equal(flat.w, flat2.w)


# ---- pcmi_net_set_bn_momentum -----------------------------------------------------------------------------------------------
def _engine_case(seed=0):
  from helpers import surface_coords
  from pointcontrast_amd import minkowski as ME
  from pointcontrast_amd.engine import NativeEngine
  from pointcontrast_amd.lib.config import get_config
  from pointcontrast_amd.lib.distributed import FlatParameters
  from pointcontrast_amd.model import load_model
  torch.manual_seed(seed)
  cfg = get_config(["net.normalize_feature=False", "opt.bn_momentum=0.02"])
  model = load_model("Res16UNet34C")(3, 32, cfg, D=3).to(DEV)
  flat = FlatParameters(model.parameters())
  engine = NativeEngine(model, flat, in_channels=3, n_passes=1)
  coords = surface_coords(14, seed=3)  # about 200 voxels per scene
  feats = torch.randn(coords.shape[0], 3)
  return model, engine, ME, coords, feats


def test_set_bn_momentum_moves_the_running_mean_by_the_new_momentum():
  model, engine, ME, coords, feats = _engine_case()
  bn0 = model.bn0.bn
  before = bn0.running_mean.clone()
  st = ME.SparseTensor(feats, coords=coords).to(DEV)
  engine.forward(0, st, training=True)
  after_default = bn0.running_mean.clone()
  batch_mean = before + (after_default - before) / 0.02  # running' = (1 - m) running + m batch
  # an engine that never calls set_bn_momentum matches the eager modules, as before
  model2, _, _, _, _ = _engine_case()
  model2.train()
  model2(ME.SparseTensor(feats, coords=coords).to(DEV))
  assert R.rel_err(after_default, model2.bn0.bn.running_mean) <= TOL
  # the same batch again, from the same running estimate, with another momentum
  model3, engine3, _, _, _ = _engine_case()
  engine3.set_bn_momentum(0.5)
  assert all(m.bn.momentum == 0.5 for m in engine3._bn_modules) and model3.bn0.bn.momentum == 0.5
  engine3.forward(0, ME.SparseTensor(feats, coords=coords).to(DEV), training=True)
  want = 0.5 * before + 0.5 * batch_mean
  moved = float((model3.bn0.bn.running_mean - before).abs().max())
  assert moved > 10 * float((after_default - before).abs().max())  # 0.5 against 0.02
  assert float((model3.bn0.bn.running_mean - want).abs().max()) <= 1e-3 * moved  # batch_mean is recovered through a division by 0.02
  with pytest.raises(Exception):
    engine3.set_bn_momentum(1.5)
