"""Layer-sized test of the BatchNorm forms only the network executor reaches (pytest -m gpu): two row segments with
their own statistics in one launch, parameter gradients accumulated across segments, the one-bit ReLU pattern, and a
residual gradient that one consumer writes and the other accumulates.

The model is three 1x1x1 convolutions with a BatchNorm each, all of width c, run through NativeEngine:

    t0  = bn0(conv0(x))                 no ReLU
    t1  = relu(bn1(conv1(t0)))          ReLU, no residual
    out = relu(bn2(conv2(t1)) + t0)     residual: t0's gradient comes from conv1 AND from bn2

A 1x1x1 convolution is a matrix product, so the reference is float64 torch on the CPU, per cloud, with training-mode
statistics per cloud.  Two clouds run three ways: as one two-segment tensor (coords_man.set_split) and each alone.
The reference takes the device's ReLU patterns (both sides differentiate the same piecewise-linear function); where a
pattern differs from float64's, the pre-activation lies within the forward tolerance of zero.

Tolerance: 1e-4 relative to the tensor's maximum, the bound test_batchnorm_parity and test_gpu_c_contract.py hold the
same quantities to.  Joint and single passes are NOT compared bit for bit: the row-block partition of the shorter
segment differs by design.
"""
import numpy as np
import pytest
import torch

import c_contract as cc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-4

# (rows per segment, c, environment): the smallest sizes that reach each branch of the BatchNorm dispatch
# (red_geom, bn_small_rows, bn_lean_eligible in csrc/norm.hip) with the default thresholds unless stated
CASES = [
    # one-launch forward and backward; the segments fall in different rows-per-thread buckets (8 and 4)
    ((300, 200), 32, {}),
    # one-launch forward in its 512-thread form (longest > 768), three-launch backward
    ((1000, 300), 32, {}),
    # c % 32 != 0: no bit pattern, the fp32 output is the mask
    ((300, 200), 16, {}),
    # three launches both ways, the merge of the partials with grid y = 2
    ((2000, 1700), 64, {}),
    # fp32-mask forms of the partial and apply kernels
    ((2000, 1700), 64, {"PCMI_BN_RELU_BITS": "0"}),
    # lean backward statistics <2> on bn1 / bn2, <0> on bn0
    ((2000, 1700), 64, {"PCMI_BN_LEAN_ROWS": "1"}),
    # lean backward statistics <1>
    ((2000, 1700), 64, {"PCMI_BN_LEAN_ROWS": "1", "PCMI_BN_RELU_BITS": "0"}),
    # two segments: the row blocks re-cut to <= 256 (36 rows per block, 250 blocks); the 9000-row cloud alone: 282
    # blocks > 256, so the wide final kernels (bn_stats_final_kernel / colsum2_final_kernel)
    ((9000, 5000), 256, {}),
]
RUNS = ("joint", "cloud0", "cloud1")


def case_id(case):
  segs, c, env = case
  return "%dx%d-c%d%s" % (segs[0], segs[1], c, "".join("-%s=%s" % (k[8:].lower(), v) for k, v in sorted(env.items())))


def _net(ME, c):
  from torch import nn

  class Net(nn.Module):

    def __init__(self):
      super().__init__()
      for i in range(3):
        setattr(self, "conv%d" % i, ME.MinkowskiConvolution(c, c, kernel_size=1, stride=1, dimension=3))
        setattr(self, "bn%d" % i, ME.MinkowskiBatchNorm(c))

    def forward(self, x):
      t0 = self.bn0(self.conv0(x))
      t1 = self.bn1(self.conv1(t0), relu=True)
      return self.bn2(self.conv2(t1), residual=t0, relu=True)

  return Net()


def _cloud(rng, n, c, features=None, cloud=0):
  """n unique integer coordinates (batch index 0) and features with a mean (the batch means are then well off zero).
  features: (rng, n, c, cloud) -> float32 [n, c] instead of them (tests/test_gpu_norm_conditioning.py)."""
  cell = rng.choice(48 ** 3, n, replace=False)
  C = np.stack([np.zeros(n, np.int64), cell // (48 * 48) - 24, cell // 48 % 48 - 24, cell % 48 - 24], 1).astype(np.int32)
  if features is None:
    F = (rng.standard_normal((n, c)) * 2.0 + 0.7).astype(np.float32)
  else:
    F = np.ascontiguousarray(features(rng, n, c, cloud), dtype=np.float32)
    assert F.shape == (n, c)
  return torch.from_numpy(C), torch.from_numpy(F)


def run_case(ME, segs, c, seed=0, features=None, identity_conv0=False):
  """Runs the model on the device three ways and returns everything the checks (and a bit-for-bit comparison of two
  builds) need, on the CPU: {"params", "running0", "x", "g", "eps", "momentum", "runs": {run: {"bn_in", "bn_res",
  "bn_out" (per layer), "running" (after the pass), "grad" (flat.g after its backward)}}}.
  features: the feature generator of _cloud; identity_conv0: conv0.kernel = I, so that bn0 normalises the features themselves."""
  from pointcontrast_amd.engine import NativeEngine, OP_BN
  from pointcontrast_amd.lib.distributed import FlatParameters
  torch.manual_seed(seed)
  rng = np.random.RandomState(seed)
  model = _net(ME, c)
  with torch.no_grad():
    for i in range(3):
      bn = getattr(model, "bn%d" % i).bn
      bn.weight.uniform_(0.5, 1.5)
      bn.bias.uniform_(-0.5, 0.5)
      bn.running_mean.normal_()
      bn.running_var.uniform_(0.5, 1.5)
    if identity_conv0:
      model.conv0.kernel.copy_(torch.eye(c).view_as(model.conv0.kernel))
  model = model.to(DEV).train()
  flat = FlatParameters(model.parameters())
  eng = NativeEngine(model, flat, in_channels=c)
  bns = [getattr(model, "bn%d" % i).bn for i in range(3)]
  bn_ops = [o for o in eng._ops if o["type"] == OP_BN]
  assert len(bn_ops) == 3 and [o["relu"] for o in bn_ops] == [0, 1, 1] and bn_ops[2]["in2"] == bn_ops[0]["out"]
  clouds = [_cloud(rng, n, c, features, k) for k, n in enumerate(segs)]
  g = [torch.randn(n, c) for n in segs]
  running0 = [(b.running_mean.clone(), b.running_var.clone()) for b in bns]

  def snapshot(pass_id, out):
    acts = lambda key: [eng.activation(pass_id, o[key]).cpu() if o[key] >= 0 else None for o in bn_ops]
    r = dict(bn_in=acts("in_"), bn_res=acts("in2"), bn_out=acts("out"),
             running=[(b.running_mean.cpu().clone(), b.running_var.cpu().clone()) for b in bns])
    assert torch.equal(r["bn_out"][2], out.cpu())
    return r

  def backward(pass_id, d_out):
    flat.zero_grad()
    eng.backward(pass_id, d_out.to(DEV))
    return flat.g.cpu().clone()

  runs = {}
  (C0, F0), (C1, F1) = clouds
  C1s = C1.clone()
  C1s[:, 0] += int(C0[:, 0].max()) + 1
  sj = ME.SparseTensor(torch.cat([F0, F1]), coords=torch.cat([C0, C1s])).to(DEV)
  sj.coords_man.set_split(segs[0])
  runs["joint"] = snapshot(0, eng.forward(0, sj))
  runs["joint"]["grad"] = backward(0, torch.cat(g))
  with torch.no_grad():
    for b, (rm, rv) in zip(bns, running0):
      b.running_mean.copy_(rm)
      b.running_var.copy_(rv)
  sts = [ME.SparseTensor(F, coords=C).to(DEV) for C, F in clouds]
  for i in range(2):  # cloud 0 as pass 0, then cloud 1 as pass 1: the running estimates take the two updates in turn
    runs["cloud%d" % i] = snapshot(i, eng.forward(i, sts[i]))
  for i in range(2):
    runs["cloud%d" % i]["grad"] = backward(i, g[i])
  torch.cuda.synchronize()
  names = [n for n, _ in model.named_parameters()]
  return dict(params={n: flat.view(flat.w, i).cpu().clone() for i, n in enumerate(names)}, names=names,
              offsets=list(flat.offsets), running0=[(a.cpu(), b.cpu()) for a, b in running0], x=[F0, F1], g=g,
              eps=[b.eps for b in bns], momentum=[b.momentum for b in bns], runs=runs)


def _bn64(x, gamma, beta, eps, res, mask):
  mean, var = x.mean(0), x.var(0, unbiased=False)
  y = (x - mean) / torch.sqrt(var + eps) * gamma + beta
  if res is not None:
    y = y + res
  return y * mask if mask is not None else y


def model_grads64(x, params, eps, masks, g):
  """Parameter gradients of the whole model for ONE cloud in float64, its two ReLUs taking the patterns `masks`."""
  p = {n: v.double().requires_grad_(True) for n, v in params.items()}
  t0 = _bn64(x.double() @ p["conv0.kernel"], p["bn0.bn.weight"], p["bn0.bn.bias"], eps[0], None, None)
  t1 = _bn64(t0 @ p["conv1.kernel"], p["bn1.bn.weight"], p["bn1.bn.bias"], eps[1], None, masks[0].double())
  out = _bn64(t1 @ p["conv2.kernel"], p["bn2.bn.weight"], p["bn2.bn.bias"], eps[2], t0, masks[1].double())
  out.backward(g.double())
  return {n: v.grad for n, v in p.items()}


def _err(got, ref):
  return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-30))


def check_case(res, segs, report=print):
  n0 = segs[0]
  rows = {"joint": [slice(0, n0), slice(n0, None)], "cloud0": [slice(None)], "cloud1": [slice(None)]}
  clouds = {"joint": [0, 1], "cloud0": [0], "cloud1": [1]}
  failures = []

  def hold(e, what):
    report("%-44s %.3e" % (what, e))
    if not e <= TOL:
      failures.append("%s: %.3e > %.1e" % (what, e, TOL))

  for run in RUNS:
    r = res["runs"][run]
    # ---- every BatchNorm against float64 BatchNorm of ITS OWN device input, per segment; the running estimates ----
    running = res["running0"] if run != "cloud1" else res["runs"]["cloud0"]["running"]
    for l in range(3):
      name, relu = "bn%d.bn" % l, l > 0
      gamma, beta = res["params"][name + ".weight"], res["params"][name + ".bias"]
      rm, rv = running[l][0].double(), running[l][1].double()
      mo = res["momentum"][l]
      for s, sl in enumerate(rows[run]):
        x, y = r["bn_in"][l][sl], r["bn_out"][l][sl]
        rs = r["bn_res"][l][sl] if r["bn_res"][l] is not None else None
        ref = cc.bn_ref64(x, gamma, beta, res["eps"][l], rs, relu, torch.zeros_like(x), relu_mask=(y > 0) if relu else None)
        tag = "%s segment %d %s" % (run, s, name)
        hold(_err(y, ref["y"]), tag + " y")
        # the device's ReLU pattern differs from float64's only within the forward tolerance of zero
        hold(ref["flipped_max"] / float(ref["y"].abs().max()), tag + " |y| where the ReLU patterns differ")
        rm, rv = (1 - mo) * rm + mo * ref["mean"], (1 - mo) * rv + mo * ref["unbiased"]
      hold(_err(r["running"][l][0], rm), "%s %s running_mean" % (run, name))
      hold(_err(r["running"][l][1], rv), "%s %s running_var" % (run, name))
    # ---- every parameter gradient against the float64 model's, summed over the clouds of the run ----
    want = None
    for s, (cl, sl) in enumerate(zip(clouds[run], rows[run])):
      masks = [r["bn_out"][l][sl] > 0 for l in (1, 2)]
      gr = model_grads64(res["x"][cl], res["params"], res["eps"], masks, res["g"][cl])
      want = gr if want is None else {n: want[n] + gr[n] for n in gr}
    for i, n in enumerate(res["names"]):
      got = r["grad"][res["offsets"][i]:res["offsets"][i] + want[n].numel()].view(want[n].shape)
      hold(_err(got, want[n]), "%s grad %s" % (run, n))
  return failures


@pytest.fixture(scope="module")
def ME():
  import pointcontrast_amd.minkowski as me
  return me


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_batchnorm_segments_through_the_executor(ME, case, monkeypatch):
  segs, c, env = case
  for k, v in env.items():
    monkeypatch.setenv(k, v)
  res = run_case(ME, segs, c)
  failures = check_case(res, segs)
  assert not failures, "\n".join(failures)
