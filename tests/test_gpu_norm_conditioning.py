"""Every normalisation of the library on ill-conditioned columns, per column, against float64 (pytest -m gpu).

The other BatchNorm tests draw N(0.7, 2): at mean / std 0.35 every variance formula passes.  Here channel j has type j % 7, so
that every float4 lane, every 16-channel group of the one-launch kernels and every 32-channel bit word sees every type:

    0  N(0.7, 2), the control            4  the constant 0.1f
    1  N(256, 1)                         5  N(0, 1) * 1e4
    2  N(-32, 0.125)                     6  N(3, 1), the first 10 % of the rows shifted by +200: the block means differ widely
    3  the constant 0.0, a dead channel     and the cross term of the merge of the blocks carries the variance

drawn in float64 and rounded to fp32; the reference is float64 arithmetic on those rounded values.

Errors are taken PER COLUMN (a constant column has invstd = 1 / sqrt(eps) = 316 and would set the scale for every other one):
y, dx, dres: max_i |got - ref| <= 1e-4 max_i |ref_ij|; dbeta_j, dgamma_j: |got - ref| <= 1e-4 S_j with S_j the float64 sum of the
absolute values of the terms; the statistics element-wise, 1e-4 relative to |ref_j|.  1e-4 is the bound of test_batchnorm_parity.
Every test prints the worst error per column type.

The cases are the smallest shapes that reach each branch of bn_path (csrc/norm.hip): the one-launch kernels compute a centred
second moment; the general path sums, per row block, x and the differences from the block's first row, writes per column the better
conditioned (mean, M2) of the two, and merges the blocks.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import c_contract as cc  # noqa: E402
import pointnet2_backbone_ref as PR  # noqa: E402
import pool_ref as R  # noqa: E402
import test_gpu_bn_segments as seg  # noqa: E402
import test_gpu_instance_norm as inorm  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-4
EPS, MOMENTUM = 1e-5, 0.05
NTYPES = 7
FLIPPED = (1, 2, 6)  # the types whose means change sign in the second segment of a two-segment tensor


def column_mix(rng, n, c, sign=1.0):
  """float32 [n, c] of the column types above; sign = -1 mirrors the columns of types 1, 2 and 6."""
  z = rng.standard_normal((n, c))
  x = np.empty((n, c), np.float64)
  head = max(1, n // 10)
  for j in range(c):
    t = j % NTYPES
    if t == 0:
      x[:, j] = 0.7 + 2.0 * z[:, j]
    elif t == 1:
      x[:, j] = 256.0 + z[:, j]
    elif t == 2:
      x[:, j] = -32.0 + 0.125 * z[:, j]
    elif t == 3:
      x[:, j] = 0.0
    elif t == 4:
      x[:, j] = np.float32(0.1)
    elif t == 5:
      x[:, j] = 1e4 * z[:, j]
    else:
      x[:, j] = 3.0 + z[:, j]
      x[:head, j] += 200.0
    if t in FLIPPED:
      x[:, j] *= sign
  return x.astype(np.float32)


class Held:
  """The per-column bounds of one case: collects what fails, prints the worst error per column type."""

  def __init__(self, what):
    self.what, self.failures = what, []

  def _report(self, name, err, bound, types):
    # err / bound per column (0 / 0 counts as 0, x / 0 as inf), its maximum per type
    with np.errstate(divide="ignore", invalid="ignore"):
      ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)) * TOL
    worst = [float(ratio[types == t].max()) if (types == t).any() else 0.0 for t in range(NTYPES)]
    print("%-34s %-13s %s" % (self.what, name, " ".join("t%d %.2e" % (t, w) for t, w in enumerate(worst))))
    bad = np.nonzero(~(err <= bound))[0]
    if len(bad):
      j = int(bad[np.argmax(ratio[bad])])
      self.failures.append("%s %s: %d columns beyond %.0e, worst column %d (type %d): %.3e" % (
          self.what, name, len(bad), TOL, j, j % NTYPES, ratio[j]))

  def rows(self, name, got, ref):
    """[n, c]: max_i |got - ref| <= TOL max_i |ref_ij| in every column j."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "%s %s: non-finite values" % (self.what, name)
    self._report(name, (got - ref).abs().amax(0).numpy(), TOL * ref.abs().amax(0).numpy(), np.arange(ref.shape[1]) % NTYPES)

  def sums(self, name, got, ref, scale):
    """[c]: |got - ref| <= TOL S_j, S_j the sum of the absolute values of the terms of ref_j."""
    got, ref, scale = (v.detach().double().cpu().reshape(-1) for v in (got, ref, scale))
    assert bool(torch.isfinite(got).all()), "%s %s: non-finite values" % (self.what, name)
    self._report(name, (got - ref).abs().numpy(), TOL * scale.numpy(), np.arange(ref.numel()) % NTYPES)

  def stats(self, name, got, ref):
    """[c]: element-wise, TOL relative to |ref_j|."""
    self.sums(name, got, ref, ref.detach().double().cpu().reshape(-1).abs())

  def scalar(self, name, value):
    print("%-34s %-13s %.2e" % (self.what, name, value))
    if not value <= TOL:
      self.failures.append("%s %s: %.3e > %.0e" % (self.what, name, value, TOL))

  def done(self):
    assert not self.failures, "\n".join(self.failures)


def sum_scales(x, ref, dy, mask, eps):
  """(S of dbeta, S of dgamma): sum_i |g_ij| and sum_i |g_ij xhat_ij| in float64, g the gradient behind the ReLU pattern."""
  xhat = (x.double() - ref["mean"]) / torch.sqrt(ref["var"] + eps)
  g = dy.double() * mask.double() if mask is not None else dy.double()
  return g.abs().sum(0), (g * xhat).abs().sum(0)


# ---- PF.BatchNormFunction: every branch of bn_path with one segment -------------------------------------------------------
# (n, c, environment)
FUNCTION_CASES = [
    (300, 32, {}),    # one launch both ways
    (1000, 32, {}),   # the 512-thread one-launch forward, three-launch backward
    (1536, 96, {}),   # the last row count of the one-launch forward ...
    (1537, 96, {}),   # ... and the first of the general path
    (2000, 16, {}),   # c4 = 4: 64 row lanes, 512-row blocks
    (2049, 64, {}),   # 128-row blocks, the last one of exactly one row
    (2000, 64, {"PCMI_BN_RELU_BITS": "0"}),
    (2000, 64, {"PCMI_BN_LEAN_ROWS": "1"}),  # the lean backward statistics
    (2000, 64, {"PCMI_BN_LEAN_ROWS": "1", "PCMI_BN_RELU_BITS": "0"}),
    (9000, 256, {}),  # 282 blocks: bn_stats_final_kernel / colsum2_final_kernel
    (40000, 32, {}),  # 157 blocks of 256 rows: the lane loop of the merge kernel
]


def function_case_id(case):
  n, c, env = case
  return "%dx%d%s" % (n, c, "".join("-%s=%s" % (k[8:].lower(), v) for k, v in sorted(env.items())))


def function_inputs(n, c, seed):
  rng = np.random.RandomState(seed)
  t = lambda a: torch.from_numpy(np.asarray(a, np.float64).astype(np.float32))
  return dict(x=torch.from_numpy(column_mix(rng, n, c)), gamma=t(rng.uniform(0.5, 1.5, c)), beta=t(rng.uniform(-0.5, 0.5, c)),
              rm=t(rng.standard_normal(c)), rv=t(rng.uniform(0.5, 1.5, c)), dy=t(rng.standard_normal((n, c))),
              res=t(rng.standard_normal((n, c))))


def run_function(inp, fused):
  """One forward and backward of PF.BatchNormFunction, with or without (residual, ReLU); everything on the CPU."""
  from pointcontrast_amd import functional as PF
  x, gamma, beta = (inp[k].to(DEV).requires_grad_(True) for k in ("x", "gamma", "beta"))
  res = inp["res"].to(DEV).requires_grad_(True) if fused else None
  rm, rv = inp["rm"].to(DEV).clone(), inp["rv"].to(DEV).clone()
  y = PF.BatchNormFunction.apply(x, gamma, beta, rm, rv, MOMENTUM, EPS, res, fused)
  _, _, mean, invstd, _ = y.grad_fn.saved_tensors  # what pcmi_bn_fwd_train returned for the backward pass
  y.backward(inp["dy"].to(DEV))
  torch.cuda.synchronize()
  out = dict(y=y.detach(), dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad, dres=res.grad if fused else None, running_mean=rm,
             running_var=rv, save_mean=mean.detach(), save_invstd=invstd.detach())
  return {k: v.cpu().clone() for k, v in out.items() if v is not None}


def hold_function(h, inp, got, fused):
  x, dy = inp["x"], inp["dy"]
  mask = (got["y"] > 0) if fused else None
  ref = cc.bn_ref64(x, inp["gamma"], inp["beta"], EPS, inp["res"] if fused else None, fused, dy, relu_mask=mask)
  h.rows("y", got["y"], ref["y"])
  if fused:  # the device's ReLU pattern differs from float64's only within the forward tolerance of zero
    h.scalar("flipped |y|", ref["flipped_max"] / float(ref["y"].abs().max()))
    h.rows("dres", got["dres"], ref["dres"])
  h.rows("dx", got["dx"], ref["dx"])
  s_beta, s_gamma = sum_scales(x, ref, dy, mask, EPS)
  h.sums("dbeta", got["dbeta"], ref["dbeta"], s_beta)
  h.sums("dgamma", got["dgamma"], ref["dgamma"], s_gamma)
  h.stats("save_mean", got["save_mean"], ref["mean"])
  h.stats("save_invstd", got["save_invstd"], 1.0 / torch.sqrt(ref["var"] + EPS))
  h.stats("running_mean", got["running_mean"], (1 - MOMENTUM) * inp["rm"].double() + MOMENTUM * ref["mean"])
  h.stats("running_var", got["running_var"], (1 - MOMENTUM) * inp["rv"].double() + MOMENTUM * ref["unbiased"])


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "residual-relu"])
@pytest.mark.parametrize("case", FUNCTION_CASES, ids=function_case_id)
def test_batchnorm_function_per_column(case, fused, monkeypatch):
  n, c, env = case
  for k, v in env.items():
    monkeypatch.setenv(k, v)
  inp = function_inputs(n, c, seed=n + c)
  got = run_function(inp, fused)
  again = run_function(inp, fused)
  for k in got:  # every form is deterministic
    assert torch.equal(got[k], again[k]), "two runs differ in %s" % k
  h = Held("%s %s" % (function_case_id(case), "res+relu" if fused else "plain"))
  hold_function(h, inp, got, fused)
  h.done()


def test_the_two_forms_agree_on_the_rows_of_the_one_launch_bound(monkeypatch):
  """The same 1536 rows through the one-launch kernel and, with PCMI_BN_SMALL_ROWS=0, through the general path: the
  statistics agree per column (and with them what is normalised on either side of the bound)."""
  inp = function_inputs(1537, 96, seed=1537 + 96)
  inp = {k: (v[:1536].contiguous() if v.dim() == 2 else v) for k, v in inp.items()}
  one = run_function(inp, False)
  monkeypatch.setenv("PCMI_BN_SMALL_ROWS", "0")
  monkeypatch.setenv("PCMI_BN_SMALL_BWD_ROWS", "0")
  gen = run_function(inp, False)
  h = Held("1536x96 one launch vs general")
  for k in ("save_mean", "save_invstd", "running_mean", "running_var"):
    h.stats(k, gen[k], one[k])
  h.rows("y", gen["y"], one["y"])
  h.done()


# ---- two segments through the executor ------------------------------------------------------------------------------------
def mirrored_mix(rng, n, c, cloud):
  return column_mix(rng, n, c, sign=-1.0 if cloud else 1.0)


def bn0_sums64(x, params, eps, masks, g):
  """bn0's parameter gradients for ONE cloud in float64 with the scales of their sums: (dbeta, dgamma, S_dbeta, S_dgamma)."""
  p = {n: v.double() for n, v in params.items()}
  h0 = x.double() @ p["conv0.kernel"]
  xhat = (h0 - h0.mean(0)) / torch.sqrt(h0.var(0, unbiased=False) + eps[0])
  t0 = (xhat * p["bn0.bn.weight"] + p["bn0.bn.bias"]).requires_grad_(True)
  t1 = seg._bn64(t0 @ p["conv1.kernel"], p["bn1.bn.weight"], p["bn1.bn.bias"], eps[1], None, masks[0].double())
  out = seg._bn64(t1 @ p["conv2.kernel"], p["bn2.bn.weight"], p["bn2.bn.bias"], eps[2], t0, masks[1].double())
  out.backward(g.double())
  g0 = t0.grad
  return g0.sum(0), (g0 * xhat).sum(0), g0.abs().sum(0), (g0 * xhat).abs().sum(0)


@pytest.mark.parametrize("segs", [(300, 200), (2000, 1700), (9000, 5000)], ids=lambda s: "%dx%d" % s)
def test_two_segments_per_column_through_the_executor(segs):
  """The column mix with the means of types 1, 2 and 6 mirrored in the second cloud (a statistic or a pivot that leaks
  across the split shows), conv0 the identity: bn0 normalises the mix itself.  bn0 per column, the rest by check_case."""
  import pointcontrast_amd.minkowski as ME
  c = 64
  res = seg.run_case(ME, segs, c, features=mirrored_mix, identity_conv0=True)
  n0 = segs[0]
  rows = {"joint": [slice(0, n0), slice(n0, None)], "cloud0": [slice(None)], "cloud1": [slice(None)]}
  clouds = {"joint": [0, 1], "cloud0": [0], "cloud1": [1]}
  gamma, beta = res["params"]["bn0.bn.weight"], res["params"]["bn0.bn.bias"]
  names = res["names"]
  grad_of = lambda r, n: r["grad"][res["offsets"][names.index(n)]:res["offsets"][names.index(n)] + c]
  failures = []
  for run in seg.RUNS:
    r = res["runs"][run]
    h = Held("%dx%d %s bn0" % (segs[0], segs[1], run))
    running = res["running0"] if run != "cloud1" else res["runs"]["cloud0"]["running"]
    rm, rv = running[0][0].double(), running[0][1].double()
    want = None
    for s, (cl, sl) in enumerate(zip(clouds[run], rows[run])):
      x, y = r["bn_in"][0][sl], r["bn_out"][0][sl]
      assert torch.equal(x, res["x"][cl]), "conv0 is the identity: bn0 reads the features"
      ref = cc.bn_ref64(x, gamma, beta, res["eps"][0], None, False, torch.zeros_like(x))
      h.rows("segment %d y" % s, y, ref["y"])
      mo = res["momentum"][0]
      rm, rv = (1 - mo) * rm + mo * ref["mean"], (1 - mo) * rv + mo * ref["unbiased"]
      masks = [r["bn_out"][l][sl] > 0 for l in (1, 2)]
      t = bn0_sums64(res["x"][cl], res["params"], res["eps"], masks, res["g"][cl])
      want = t if want is None else tuple(a + b for a, b in zip(want, t))
    h.stats("running_mean", r["running"][0][0], rm)
    h.stats("running_var", r["running"][0][1], rv)
    h.sums("dbeta", grad_of(r, "bn0.bn.bias"), want[0], want[2])
    h.sums("dgamma", grad_of(r, "bn0.bn.weight"), want[1], want[3])
    failures += h.failures
  failures += seg.check_case(res, segs)
  assert not failures, "\n".join(failures)


# ---- the row kernels with statistics of their own -------------------------------------------------------------------------
@pytest.mark.parametrize("Rr,ns,Cc", [(96, 16, 64), (50, 7, 30)], ids=["16-byte", "4-byte"])
def test_bn_maxpool_per_column(Rr, ns, Cc):
  from pointcontrast_amd import functional as PF
  n = Rr * ns
  inp = function_inputs(n, Cc, seed=n + Cc)
  gout = torch.from_numpy(np.random.RandomState(Cc).standard_normal((Rr, Cc)).astype(np.float32))
  x, gamma, beta = (inp[k].to(DEV).requires_grad_(True) for k in ("x", "gamma", "beta"))
  rm, rv = inp["rm"].to(DEV).clone(), inp["rv"].to(DEV).clone()
  out, arg = PF.BatchNormMaxPoolFunction.apply(x, gamma, beta, rm, rv, MOMENTUM, EPS, ns)
  _, _, mean, invstd, _, _ = out.grad_fn.saved_tensors
  dx, dgamma, dbeta = torch.autograd.grad(out, [x, gamma, beta], gout.to(DEV))
  torch.cuda.synchronize()
  xn, gn, bn = inp["x"].numpy(), inp["gamma"].numpy(), inp["beta"].numpy()
  ref = PR.bn_maxpool_ref(xn, gn, bn, ns, EPS)
  h = Held("bn_maxpool %dx%dx%d" % (Rr, ns, Cc))
  h.rows("out", out, torch.from_numpy(ref["out"]))
  # two rows of a window that tie within round-off: the device's row is accepted if its y is the window's maximum to TOL
  a = arg.cpu().numpy()
  at = np.take_along_axis(ref["y"], a[:, None, :].astype(np.int64), 1)[:, 0]
  h.rows("y at arg", torch.from_numpy(at), torch.from_numpy(ref["y"].max(1)))
  print("bn_maxpool: %d of %d argument rows differ from float64's" % (int((a != ref["arg"]).sum()), a.size))
  # ... and the reference's backward pass goes through the device's rows
  wdx, wdg, wdb = PR.bn_maxpool_grad_ref(xn, gn, bn, ns, a, gout.numpy(), EPS)
  h.rows("dx", dx, torch.from_numpy(wdx))
  xhat = (xn.astype(np.float64) - ref["mean"]) / np.sqrt(ref["var"] + EPS)
  g = gout.numpy().astype(np.float64) * (at > 0)  # the gradient that reaches row arg of every window
  xhat_at = np.take_along_axis(xhat.reshape(Rr, ns, Cc), a[:, None, :].astype(np.int64), 1)[:, 0]
  h.sums("dbeta", dbeta, torch.from_numpy(wdb), torch.from_numpy(np.abs(g).sum(0)))
  h.sums("dgamma", dgamma, torch.from_numpy(wdg), torch.from_numpy(np.abs(g * xhat_at).sum(0)))
  h.stats("save_mean", mean, torch.from_numpy(ref["mean"]))
  h.stats("save_invstd", invstd, torch.from_numpy(1.0 / np.sqrt(ref["var"] + EPS)))
  h.stats("running_mean", rm, (1 - MOMENTUM) * inp["rm"].double() + MOMENTUM * torch.from_numpy(ref["mean"]))
  h.stats("running_var", rv, (1 - MOMENTUM) * inp["rv"].double() + MOMENTUM * torch.from_numpy(ref["unbiased"]))
  h.done()


@pytest.mark.parametrize("C", [13, 96])
@pytest.mark.parametrize("residual, relu", [(False, False), (True, True)], ids=["plain", "residual-relu"])
def test_instance_norm_per_column(C, residual, relu):
  """Three instances of 400, 250 and 1 rows; in the one-row instance every column is a constant one."""
  coords = inorm._coords({0: 400, 3: 250, 7: 1}, seed=C)
  x = torch.from_numpy(column_mix(np.random.RandomState(C), len(coords), C)).double()
  got, ref = inorm._run(coords, x, C, residual, relu, seed=C)
  h = Held("instance norm C=%d %s" % (C, "res+relu" if relu else "plain"))
  h.rows("y", got["y"], ref["y"])
  h.rows("dx", got["dx"], ref["dx"])
  if residual:
    h.rows("dres", got["dr"], ref["dr"])
  # the scales of the parameter gradients: the float64 restatement once more, its terms kept
  gen = torch.Generator().manual_seed(C)  # (the draws of _run, in its order)
  torch.rand(1, C, generator=gen), torch.rand(1, C, generator=gen)
  if residual:
    torch.randn(x.shape, dtype=torch.float64, generator=gen)
  dy = torch.randn(x.shape, dtype=torch.float64, generator=gen)
  _, inv = R.instances(coords[:, 0])
  cnt = torch.bincount(inv).double()[:, None]
  mean = torch.zeros((len(cnt), C), dtype=torch.float64).index_add(0, inv, x) / cnt
  var = torch.zeros((len(cnt), C), dtype=torch.float64).index_add(0, inv, (x - mean[inv]) ** 2) / cnt
  xhat = (x - mean[inv]) / torch.sqrt(var[inv] + 1e-5)
  g = dy * (ref["y"] > 0) if relu else dy
  h.sums("dbias", got["db"], ref["db"], g.abs().sum(0))
  h.sums("dweight", got["dw"], ref["dw"], (g * xhat).abs().sum(0))
  h.done()
