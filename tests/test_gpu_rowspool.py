"""The PointNet++ backbone's row kernels (csrc/rowspool.hip) on the MI355X through the C ABI: bn_maxpool (BatchNorm + ReLU +
max over ns rows in one pass; forward in training and eval form, backward) and interp_rows (three_interpolate + concatenation
into rows; forward, backward).  References: tests/pointnet2_backbone_ref.py, pinned on the CPU by
tests/test_pointnet2_backbone_ref.py.

Bounds: float results within 1e-4 of float64 relative to the tensor's largest entry (pointset_ref.rel_err, the bound every
kernel of this library is held to); interp_rows' forward, whose operations are individually rounded fp32, exactly equal to
numpy float32; backward passes bit-identical between two runs.  Every pooling row the device reports must attain its window's
maximum of the float64 y within the forward bound -- no element is excluded."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointnet2_backbone_ref as R  # noqa: E402
import pointset_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-4
F32 = np.float32
EPS, MOMENTUM = 1e-5, 0.1
PCMI_OK, PCMI_ERR_INVALID, PCMI_ERR_RANGE, PCMI_ERR_UNSUPPORTED, PCMI_ERR_WORKSPACE = 0, -1, -5, -6, -7
SENTINEL = -12345.0


def _dev(a, dtype=None):
  t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
  return t if dtype is None else t.to(dtype)


def _strided(a, ld, fill=SENTINEL):
  """a [rows, C] on the device as the first C columns of a [rows, ld] buffer filled with the sentinel."""
  buf = torch.full((a.shape[0], ld), fill, dtype=torch.float32, device=DEV)
  buf[:, :a.shape[1]] = _dev(np.asarray(a, F32))
  return buf


def _lib():
  from pointcontrast_amd._lib import lib
  from pointcontrast_amd.runtime import cur_stream, ptr
  return lib, ptr, cur_stream(DEV)


def _ws(nbytes):
  buf = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=DEV)
  return buf, C.c_void_p(buf.data_ptr())


def bn_maxpool_train(x, ns, gamma, beta, x_ld, out_ld, running=None, ws_short=0):
  """pcmi_bn_maxpool_fwd_train on x [R ns, C] laid out with x_ld: (rc, dict of host arrays and the device buffers)."""
  lib, ptr, st = _lib()
  n, Cc = x.shape
  Rr = n // ns if ns > 0 else n
  xb = _strided(x, x_ld)
  out = torch.full((Rr, out_ld), SENTINEL, dtype=torch.float32, device=DEV)
  arg = torch.full((Rr, Cc), 255, dtype=torch.uint8, device=DEV)
  mean, invstd = torch.zeros(Cc, device=DEV), torch.zeros(Cc, device=DEV)
  g, b = _dev(np.asarray(gamma, F32)), _dev(np.asarray(beta, F32))
  rm = _dev(np.asarray(running[0], F32)) if running is not None else None
  rv = _dev(np.asarray(running[1], F32)) if running is not None else None
  nbytes = lib.pcmi_bn_maxpool_workspace_bytes(Rr, ns, Cc)
  keep, ws = _ws(nbytes)
  rc = lib.pcmi_bn_maxpool_fwd_train(ptr(xb), x_ld, Rr, ns, Cc, ptr(g), ptr(b), ptr(rm), ptr(rv), MOMENTUM, EPS, ptr(out), out_ld, ptr(arg),
                                     ptr(mean), ptr(invstd), ws, max(nbytes - ws_short, 0), st)
  torch.cuda.synchronize()
  return rc, dict(x=xb, out=out, arg=arg, mean=mean, invstd=invstd, rm=rm, rv=rv, gamma=g, beta=b, ws_bytes=nbytes)


def _params(rng, Cc):
  gamma = rng.uniform(0.5, 1.5, Cc).astype(F32)
  gamma[1::3] *= -1  # negative gammas among the columns (none at C == 1)
  return gamma, rng.normal(0, 0.3, Cc).astype(F32)


def _check_rows_attain_the_maximum(arg, ref):
  """Every reported row holds its window's float64 maximum within the forward bound."""
  y = ref["y"]  # [R, ns, C], post-ReLU
  at = np.take_along_axis(y, arg[:, None, :].astype(np.int64), 1)[:, 0]
  scale = max(float(np.abs(y).max()), 1e-30)
  gap = float((y.max(1) - at).max()) / scale
  print("arg gap %.3g" % gap)
  assert gap <= TOL, gap


# ---- bn_maxpool forward ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc", [1, 128, 130])
@pytest.mark.parametrize("ns", [1, 2, 16, 64, 256])
@pytest.mark.parametrize("Rr", [1, 7, 65])
def test_bn_maxpool_forward_train(Rr, ns, Cc):
  rng = np.random.RandomState(Rr * 100000 + ns * 1000 + Cc)
  x = (rng.normal(0, 1, (Rr * ns, Cc)) * rng.uniform(0.5, 2.0, Cc) + rng.normal(0, 1, Cc)).astype(F32)
  gamma, beta = _params(rng, Cc)
  rm0, rv0 = rng.normal(0, 1, Cc).astype(F32), rng.uniform(0.5, 1.5, Cc).astype(F32)
  x_ld, out_ld = Cc + (4 if Cc % 4 == 0 else 3), Cc + (8 if Cc % 4 == 0 else 1)
  rc, d = bn_maxpool_train(x, ns, gamma, beta, x_ld, out_ld, running=(rm0, rv0))
  assert rc == PCMI_OK
  ref = R.bn_maxpool_ref(x, gamma, beta, ns, EPS)
  out = d["out"].cpu().numpy()
  errs = dict(out=P.rel_err(out[:, :Cc], ref["out"]), mean=P.rel_err(d["mean"], ref["mean"]),
              invstd=P.rel_err(d["invstd"], 1.0 / np.sqrt(ref["var"] + EPS)),
              rm=P.rel_err(d["rm"], (1 - MOMENTUM) * rm0.astype(np.float64) + MOMENTUM * ref["mean"]),
              rv=P.rel_err(d["rv"], (1 - MOMENTUM) * rv0.astype(np.float64) + MOMENTUM * ref["unbiased"]))
  print(Rr, ns, Cc, errs)
  assert all(e <= TOL for e in errs.values()), errs
  assert (out[:, Cc:] == SENTINEL).all(), "the columns behind C were written"
  arg = d["arg"].cpu().numpy()
  assert arg.max() < ns
  _check_rows_attain_the_maximum(arg, ref)


def test_bn_maxpool_single_row_moves_the_running_variance_as_bn_fwd_train():
  from pointcontrast_amd import functional as PF
  for Cc in (4, 8):  # pcmi_bn_fwd_train takes multiples of 4
    x = np.linspace(-1, 2, Cc).astype(F32).reshape(1, Cc)
    gamma, beta = np.ones(Cc, F32), np.linspace(-0.5, 0.5, Cc).astype(F32)
    rm0, rv0 = np.full(Cc, 0.25, F32), np.full(Cc, 1.5, F32)
    rc, d = bn_maxpool_train(x, 1, gamma, beta, Cc, Cc, running=(rm0, rv0))
    assert rc == PCMI_OK
    rm, rv = _dev(rm0), _dev(rv0)
    PF.BatchNormFunction.apply(_dev(x), d["gamma"], d["beta"], rm, rv, MOMENTUM, EPS, None, True)
    assert P.rel_err(d["rv"], rv) <= TOL and P.rel_err(d["rm"], rm) <= TOL
    assert P.rel_err(d["rv"], (1 - MOMENTUM) * rv0.astype(np.float64)) <= TOL  # the batch's unbiased variance counts as 0
    assert P.rel_err(d["out"], np.maximum(beta, 0)[None]) <= TOL and not d["arg"].any()


@pytest.mark.parametrize("Cc", [8, 7])  # 16-byte and 4-byte accesses
def test_bn_maxpool_special_cases(Cc):
  rng = np.random.RandomState(Cc)
  ns, Rr = 16, 9
  x = rng.normal(0, 1, (Rr * ns, Cc)).astype(F32)
  gamma, beta = np.ones(Cc, F32), np.zeros(Cc, F32)
  gamma[0], beta[0] = 0.0, 0.5        # zero gamma: y == beta in every row -> a tie of the whole window -> row 0
  gamma[1] = -1.25                    # negative gamma: the smallest x of the window wins
  beta[2] = -100.0                    # a column that is <= 0 in every window -> (0, row 0)
  gamma[3], beta[3] = 0.0, -0.5       # zero gamma below zero -> (0, row 0)
  x[3 * ns:4 * ns] = x[3 * ns + 5]    # window 3: identical rows -> row 0 in every column
  x[5 * ns + 7] = x[5 * ns + 2]       # window 5: rows 2 and 7 identical -> never row 7
  rc, d = bn_maxpool_train(x, ns, gamma, beta, Cc + (4 if Cc % 4 == 0 else 1), Cc)
  assert rc == PCMI_OK
  out, arg = d["out"].cpu().numpy()[:, :Cc], d["arg"].cpu().numpy()
  ref = R.bn_maxpool_ref(x, gamma, beta, ns, EPS)
  assert P.rel_err(out, ref["out"]) <= TOL
  _check_rows_attain_the_maximum(arg, ref)
  assert (out[:, 0] == F32(0.5)).all() and (arg[:, 0] == 0).all()
  live = out[:, 1] > 0
  assert live.any() and np.array_equal(arg[live, 1], x.reshape(Rr, ns, Cc)[:, :, 1].argmin(1)[live])
  assert (out[:, 2] == 0).all() and (arg[:, 2] == 0).all()
  assert (out[:, 3] == 0).all() and (arg[:, 3] == 0).all()
  assert (arg[3] == 0).all()
  assert (arg[5] != 7).all()
  # a NaN in x poisons the batch statistics of its column: every y of the column is NaN, the lowest NaN row is row 0
  x[2 * ns + 3, 4] = np.nan
  rc, d = bn_maxpool_train(x, ns, gamma, beta, Cc, Cc)
  assert rc == PCMI_OK
  out2, arg2 = d["out"].cpu().numpy(), d["arg"].cpu().numpy()
  assert np.isnan(out2[:, 4]).all() and (arg2[:, 4] == 0).all()
  keep = [c for c in range(Cc) if c != 4]
  assert np.array_equal(out2[:, keep], out[:, keep]) and np.array_equal(arg2[:, keep], arg[:, keep])


@pytest.mark.parametrize("Rr,ns,Cc", [(7, 16, 128), (65, 2, 130), (2, 1, 1), (3, 256, 5)])
def test_bn_maxpool_forward_eval(Rr, ns, Cc):
  """The running estimates instead of batch statistics; a NaN stays local: the lowest NaN row of its window; arg may be NULL."""
  lib, ptr, st = _lib()
  rng = np.random.RandomState(Rr + ns + Cc)
  x = rng.normal(0, 1, (Rr * ns, Cc)).astype(F32)
  nan_rows = sorted({min(1, ns - 1), ns - 1})
  for s in nan_rows:
    x[(Rr - 1) * ns + s, Cc - 1] = np.nan
  gamma, beta = _params(rng, Cc)
  rm, rv = rng.normal(0, 0.5, Cc).astype(F32), rng.uniform(0.5, 1.5, Cc).astype(F32)
  x_ld = Cc + (4 if Cc % 4 == 0 else 3)
  xb = _strided(x, x_ld)
  ref = R.bn_maxpool_ref(x, gamma, beta, ns, EPS, mean=rm, var=rv)
  outs = []
  arg = torch.full((Rr, Cc), 255, dtype=torch.uint8, device=DEV)
  g_d, b_d, rm_d, rv_d = _dev(gamma), _dev(beta), _dev(rm), _dev(rv)  # held: a temporary's memory is reused by the next one
  for with_arg in (True, False):
    out = torch.full((Rr, Cc), SENTINEL, dtype=torch.float32, device=DEV)
    rc = lib.pcmi_bn_maxpool_fwd_eval(ptr(xb), x_ld, Rr, ns, Cc, ptr(g_d), ptr(b_d), ptr(rm_d), ptr(rv_d), EPS,
                                      ptr(out), Cc, ptr(arg) if with_arg else None, st)
    torch.cuda.synchronize()
    assert rc == PCMI_OK
    outs.append(out.cpu().numpy())
  out = outs[0]
  assert np.array_equal(outs[0], outs[1], equal_nan=True)
  assert np.isnan(out[Rr - 1, Cc - 1]) and arg.cpu().numpy()[Rr - 1, Cc - 1] == nan_rows[0]
  fin = ~np.isnan(ref["out"])
  assert fin.sum() == Rr * Cc - 1 and not np.isnan(out[fin]).any()
  assert float(np.abs(out[fin] - ref["out"][fin]).max()) <= TOL * max(float(np.abs(ref["out"][fin]).max()), 1e-30)
  a = arg.cpu().numpy()
  y = np.where(np.isnan(ref["y"]), -np.inf, ref["y"])
  at = np.take_along_axis(y, a[:, None, :].astype(np.int64), 1)[:, 0]
  assert float((y.max(1) - at)[fin].max()) <= TOL * float(np.abs(ref["y"][~np.isnan(ref["y"])]).max())


# ---- bn_maxpool backward ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Rr,ns,Cc", [(1, 1, 1), (1, 2, 130), (7, 2, 128), (65, 16, 128), (65, 16, 130), (7, 64, 128), (3, 256, 130),
                                      (65, 1, 4)])
def test_bn_maxpool_backward(Rr, ns, Cc):
  lib, ptr, st = _lib()
  rng = np.random.RandomState(Rr * 7 + ns * 13 + Cc)
  x = (rng.normal(0, 1, (Rr * ns, Cc)) * rng.uniform(0.5, 2.0, Cc)).astype(F32)
  gamma, beta = _params(rng, Cc)
  vec = Cc % 4 == 0
  x_ld, out_ld, g_ld, dx_ld = Cc + (4 if vec else 3), Cc + (8 if vec else 1), Cc + (4 if vec else 2), Cc + (12 if vec else 5)
  rc, d = bn_maxpool_train(x, ns, gamma, beta, x_ld, out_ld)
  assert rc == PCMI_OK
  arg = d["arg"].cpu().numpy()
  gout = rng.normal(0, 1, (Rr, Cc)).astype(F32)
  gb = _strided(gout, g_ld)
  runs = []
  for _ in range(2):
    dx = torch.full((Rr * ns, dx_ld), SENTINEL, dtype=torch.float32, device=DEV)
    dgamma, dbeta = torch.full((Cc,), SENTINEL, device=DEV), torch.full((Cc,), SENTINEL, device=DEV)
    keep, ws = _ws(d["ws_bytes"])
    rc = lib.pcmi_bn_maxpool_bwd(ptr(gb), g_ld, ptr(d["x"]), x_ld, ptr(d["out"]), out_ld, ptr(d["arg"]), Rr, ns, Cc, ptr(d["gamma"]),
                                 ptr(d["mean"]), ptr(d["invstd"]), ptr(dx), dx_ld, ptr(dgamma), ptr(dbeta), ws, d["ws_bytes"], st)
    torch.cuda.synchronize()
    assert rc == PCMI_OK
    runs.append((dx.cpu().numpy(), dgamma.cpu().numpy(), dbeta.cpu().numpy()))
  for a, b in zip(*runs):
    assert np.array_equal(a, b), "two runs differ"
  dx, dgamma, dbeta = runs[0]
  assert (dx[:, Cc:] == SENTINEL).all() and not (dx[:, :Cc] == SENTINEL).any(), "dx is not written whole, or beyond C"
  wdx, wdg, wdb = R.bn_maxpool_grad_ref(x, gamma, beta, ns, arg, gout, EPS)
  errs = (P.rel_err(dx[:, :Cc], wdx), P.rel_err(dgamma, wdg), P.rel_err(dbeta, wdb))
  print(Rr, ns, Cc, "dx %.3g dgamma %.3g dbeta %.3g" % errs)
  if Rr * ns == 1:  # one row: every gradient but dbeta is exactly zero in exact arithmetic
    assert errs[2] <= TOL and np.abs(dx[:, :Cc]).max() <= TOL * max(np.abs(gout).max(), 1e-30)
  else:
    assert max(errs) <= TOL, errs


def test_bn_maxpool_function_matches_the_composition():
  """BatchNormMaxPoolFunction against BatchNormFunction(relu) + RowsMaxPoolFunction on the same tensors: outputs, rows, gradients
  and running estimates within the bound of each other (both are held to float64 above and in tests/test_gpu_votehead.py)."""
  from pointcontrast_amd import functional as PF
  rng = np.random.RandomState(2)
  Rr, ns, Cc = 33, 16, 64
  x = rng.normal(0, 1, (Rr * ns, Cc)).astype(F32)
  gamma, beta = _params(rng, Cc)
  gout = _dev(rng.normal(0, 1, (Rr, Cc)).astype(F32))
  res = []
  for fused in (True, False):
    xt, g, b = _dev(x).requires_grad_(True), _dev(gamma).requires_grad_(True), _dev(beta).requires_grad_(True)
    rm, rv = torch.zeros(Cc, device=DEV), torch.ones(Cc, device=DEV)
    if fused:
      out, arg = PF.BatchNormMaxPoolFunction.apply(xt, g, b, rm, rv, MOMENTUM, EPS, ns)
    else:
      y = PF.BatchNormFunction.apply(xt, g, b, rm, rv, MOMENTUM, EPS, None, True)
      out, arg = PF.RowsMaxPoolFunction.apply(y, ns), PF.rows_maxpool(y.detach(), ns)[1]
    grads = torch.autograd.grad(out, [xt, g, b], gout)
    res.append([out.detach(), rm, rv] + list(grads) + [arg])
  names = ("out", "running_mean", "running_var", "dx", "dgamma", "dbeta")
  for name, a, b in zip(names, res[0], res[1]):
    assert P.rel_err(a, b) <= TOL, (name, P.rel_err(a, b))
  assert (res[0][6] != res[1][6]).float().mean() < 1e-3  # rows may differ only at values within rounding of each other


# ---- bn_maxpool contract --------------------------------------------------------------------------------------------------
def test_bn_maxpool_contract():
  lib, ptr, st = _lib()
  rng = np.random.RandomState(0)
  Rr, ns, Cc = 5, 4, 8
  x = rng.normal(0, 1, (Rr * ns, Cc)).astype(F32)
  gamma, beta = np.ones(Cc, F32), np.zeros(Cc, F32)
  rc, d = bn_maxpool_train(x, ns, gamma, beta, Cc, Cc, ws_short=1)
  assert rc == PCMI_ERR_WORKSPACE
  assert (d["out"] == SENTINEL).all(), "a refused call wrote its output"
  rc, d = bn_maxpool_train(x, ns, gamma, beta, Cc, Cc)  # the exact workspace
  assert rc == PCMI_OK and d["ws_bytes"] == lib.pcmi_bn_maxpool_workspace_bytes(Rr, ns, Cc) > 0
  for bad in (0, 257):
    rc, _ = bn_maxpool_train(np.zeros((Rr, Cc), F32), bad, gamma, beta, Cc, Cc)
    assert rc == PCMI_ERR_UNSUPPORTED, bad
    out = torch.zeros((Rr, Cc), device=DEV)
    assert lib.pcmi_bn_maxpool_fwd_eval(ptr(d["x"]), Cc, Rr, bad, Cc, ptr(d["gamma"]), ptr(d["beta"]), ptr(d["mean"]), ptr(d["invstd"]), EPS,
                                        ptr(out), Cc, None, st) == PCMI_ERR_UNSUPPORTED
    keep, ws = _ws(d["ws_bytes"])
    assert lib.pcmi_bn_maxpool_bwd(ptr(out), Cc, ptr(d["x"]), Cc, ptr(d["out"]), Cc, ptr(d["arg"]), Rr, bad, Cc, ptr(d["gamma"]), ptr(d["mean"]),
                                   ptr(d["invstd"]), ptr(out), Cc, ptr(d["mean"]), ptr(d["invstd"]), ws, d["ws_bytes"], st) == PCMI_ERR_UNSUPPORTED
  gout, dx = torch.ones((Rr, Cc), device=DEV), torch.full((Rr * ns, Cc), SENTINEL, device=DEV)
  dgamma, dbeta = torch.zeros(Cc, device=DEV), torch.zeros(Cc, device=DEV)
  keep, ws = _ws(d["ws_bytes"])
  args = (ptr(gout), Cc, ptr(d["x"]), Cc, ptr(d["out"]), Cc, ptr(d["arg"]), Rr, ns, Cc, ptr(d["gamma"]), ptr(d["mean"]), ptr(d["invstd"]), ptr(dx), Cc,
          ptr(dgamma), ptr(dbeta), ws)
  assert lib.pcmi_bn_maxpool_bwd(*args, d["ws_bytes"] - 1, st) == PCMI_ERR_WORKSPACE
  torch.cuda.synchronize()
  assert (dx == SENTINEL).all()
  assert lib.pcmi_bn_maxpool_bwd(*args, d["ws_bytes"], st) == PCMI_OK
  assert lib.pcmi_bn_maxpool_fwd_train(ptr(d["x"]), Cc - 1, Rr, ns, Cc, ptr(d["gamma"]), ptr(d["beta"]), None, None, MOMENTUM, EPS, ptr(d["out"]), Cc,
                                       ptr(d["arg"]), ptr(d["mean"]), ptr(d["invstd"]), ws, d["ws_bytes"], st) == PCMI_ERR_INVALID
  torch.cuda.synchronize()


# ---- interp_rows ----------------------------------------------------------------------------------------------------------
def _interp_case(rng, B, n, m, C2, C1):
  known = rng.normal(0, 1, (B * m, C2)).astype(F32)
  idx = rng.randint(0, m, (B, n, 3)).astype(np.int32)
  idx[B - 1, n - 1] = idx[B - 1, n - 1, 0]  # all three indices equal
  w = rng.uniform(0.05, 1, (B, n, 3)).astype(F32)
  w = (w / w.sum(-1, keepdims=True)).astype(F32)
  skip = rng.normal(0, 1, (B * n, C1)).astype(F32) if C1 else None
  return known, idx, w, skip


def interp_fwd(known, idx, w, skip, out_ld, known_ld=None, skip_ld=None, validate=0):
  lib, ptr, st = _lib()
  B, n, _ = idx.shape
  m, C2 = known.shape[0] // B, known.shape[1]
  C1 = skip.shape[1] if skip is not None else 0
  kb = _strided(known, known_ld or C2)
  sb = _strided(skip, skip_ld or C1) if C1 else None
  out = torch.full((B * n, out_ld), SENTINEL, dtype=torch.float32, device=DEV)
  idx_d, w_d = _dev(idx), _dev(w)  # held: a temporary's memory is reused by the next one
  rc = lib.pcmi_interp_rows_fwd(ptr(kb), kb.stride(0), ptr(idx_d), ptr(w_d), ptr(sb), sb.stride(0) if C1 else 0, B, m, n, C2, C1,
                                ptr(out), out_ld, validate, st)
  torch.cuda.synchronize()
  return rc, out.cpu().numpy()


@pytest.mark.parametrize("C1", [0, 5, 256])
@pytest.mark.parametrize("C2", [1, 32, 256, 260])
def test_interp_rows_forward_is_exact(C2, C1):
  rng = np.random.RandomState(C2 * 1000 + C1)
  for B in (1, 2):
    for n in (1, 65):
      for m in (3, 64):
        known, idx, w, skip = _interp_case(rng, B, n, m, C2, C1)
        wide = (C2 + C1 + 31) // 32 * 32
        for out_ld, known_ld, skip_ld in ((wide, C2, C1), (wide + 4, C2 + 4, C1 + 4), (C2 + C1 + 3, C2 + 1, C1 + 3)):
          rc, out = interp_fwd(known, idx, w, skip, out_ld, known_ld, skip_ld if C1 else None, validate=1)
          assert rc == PCMI_OK
          want = R.interp_rows_ref(known, idx, w, skip, out_ld)
          assert np.array_equal(out, want), "forward differs (B %d n %d m %d C2 %d C1 %d ld %d)" % (B, n, m, C2, C1, out_ld)
          assert not out[:, C2 + C1:].any()


def _interp_bwd_ref(gout, idx, w, m, C2):
  B, n, _ = idx.shape
  g = np.zeros((B * m, C2))
  for b in range(B):
    for i in range(n):
      for k in range(3):
        t = idx[b, i, k]
        if 0 <= t < m:
          g[b * m + t] += np.float64(w[b, i, k]) * gout[b * n + i, :C2].astype(np.float64)
  return g


@pytest.mark.parametrize("B,n,m,C2,C1", [(1, 1, 64, 32, 0), (2, 65, 3, 1, 5), (2, 65, 64, 256, 256), (2, 65, 64, 260, 5), (1, 65, 3, 32, 256)])
def test_interp_rows_backward(B, n, m, C2, C1):
  lib, ptr, st = _lib()
  rng = np.random.RandomState(B + n + m + C2 + C1)
  known, idx, w, skip = _interp_case(rng, B, n, m, C2, C1)
  g_ld = (C2 + C1 + 31) // 32 * 32
  gout = rng.normal(0, 1, (B * n, g_ld)).astype(F32)
  want = _interp_bwd_ref(gout, idx, w, m, C2)
  gk_ld = C2 + (4 if C2 % 4 == 0 else 1)
  nbytes = lib.pcmi_interp_rows_bwd_workspace_bytes(B, m, n)
  runs = []
  gout_d, idx_d, w_d = _dev(gout), _dev(idx), _dev(w)
  for short in (1, 0, 0):
    gk = torch.full((B * m, gk_ld), SENTINEL, dtype=torch.float32, device=DEV)
    keep, ws = _ws(nbytes)
    rc = lib.pcmi_interp_rows_bwd(ptr(gout_d), g_ld, ptr(idx_d), ptr(w_d), B, m, n, C2, ptr(gk), gk_ld, ws, nbytes - short, st)
    torch.cuda.synchronize()
    if short:
      assert rc == PCMI_ERR_WORKSPACE and (gk == SENTINEL).all()
      continue
    assert rc == PCMI_OK  # the exact workspace
    runs.append(gk.cpu().numpy())
  assert np.array_equal(runs[0], runs[1]), "two runs differ"
  got = runs[0]
  assert (got[:, C2:] == SENTINEL).all() and not (got[:, :C2] == SENTINEL).any()
  unnamed = np.setdiff1d(np.arange(B * m), (idx + np.arange(B)[:, None, None] * m).reshape(-1))
  if m == 64 and n == 1:
    assert len(unnamed) >= 61
  assert not got[unnamed, :C2].any(), "a known point that no row names must get a zero row"
  print(B, n, m, C2, C1, "gknown %.3g" % P.rel_err(got[:, :C2], want))
  assert P.rel_err(got[:, :C2], want) <= TOL
  # through autograd: the same gradient, and the skip's gradient is the view of gout
  from pointcontrast_amd import functional as PF
  kt = _dev(known).requires_grad_(True)
  stt = _dev(skip).requires_grad_(True) if C1 else None
  out = PF.InterpRowsFunction.apply(kt, _dev(idx), _dev(w), stt, g_ld)
  grads = torch.autograd.grad(out, [kt] + ([stt] if C1 else []), _dev(gout))
  assert np.array_equal(grads[0].cpu().numpy(), got[:, :C2])
  if C1:
    assert np.array_equal(grads[1].cpu().numpy(), gout[:, C2:C2 + C1])


def test_interp_rows_index_contract():
  lib, ptr, st = _lib()
  rng = np.random.RandomState(9)
  B, n, m, C2, C1 = 2, 9, 5, 32, 5
  known, idx, w, skip = _interp_case(rng, B, n, m, C2, C1)
  bad = idx.copy()
  bad[0, 0, 1], bad[1, 3, 2], bad[1, 8, 0] = m, -1, 1 << 30
  ld = 64
  rc, out = interp_fwd(known, bad, w, skip, ld, validate=1)
  assert rc == PCMI_ERR_RANGE and (out == SENTINEL).all(), "a refused call wrote its output"
  rc, out = interp_fwd(known, bad, w, skip, ld, validate=0)  # never dereferenced: reads as 0
  assert rc == PCMI_OK and np.array_equal(out, R.interp_rows_ref(known, bad, w, skip, ld))
  gout = rng.normal(0, 1, (B * n, ld)).astype(F32)
  nbytes = lib.pcmi_interp_rows_bwd_workspace_bytes(B, m, n)
  keep, ws = _ws(nbytes)
  gk = torch.full((B * m, C2), SENTINEL, dtype=torch.float32, device=DEV)
  gout_d, bad_d, idx_d, w_d = _dev(gout), _dev(bad), _dev(idx), _dev(w)
  assert lib.pcmi_interp_rows_bwd(ptr(gout_d), ld, ptr(bad_d), ptr(w_d), B, m, n, C2, ptr(gk), C2, ws, nbytes, st) == PCMI_OK
  torch.cuda.synchronize()
  assert P.rel_err(gk, _interp_bwd_ref(gout, bad, w, m, C2)) <= TOL  # the slots out of range are dropped
  # refusals: widths that do not fit
  rc, _ = interp_fwd(known, idx, w, skip, C2 + C1 - 1)
  assert rc == PCMI_ERR_INVALID
  assert lib.pcmi_interp_rows_bwd(ptr(gout_d), C2 - 1, ptr(idx_d), ptr(w_d), B, m, n, C2, ptr(gk), C2, ws, nbytes, st) == PCMI_ERR_INVALID
  # skip may be NULL with C1 == 0
  rc, out = interp_fwd(known, idx, w, None, 32, validate=1)
  assert rc == PCMI_OK and np.array_equal(out, R.interp_rows_ref(known, idx, w, None, 32))
