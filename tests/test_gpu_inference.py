"""The executor's inference forward (pcmi_net_forward with training = 0) against the float64 oracle in .eval() mode
(pytest -m gpu).  Every validation number of the project goes through this path: SegmentationTrainer.evaluate /
validate / test_original_pointcloud, DetectionTrainer.evaluate with the sparse backbone, feature export.

What the oracle's inference mode is worth is pinned on the CPU by tests/test_reference_source.py (bit-identical to the
reference's model source over the oracle ops; far from the training-mode result on the golden inputs).

Three cases (CASES): Res16UNet14 with 32 normalised outputs, Res16UNet14 with 20 logits, Res16UNet34C with 32 normalised
outputs.  The running estimates are moved by two training forwards of the ORACLE on make_batch(seed=8), every BatchNorm's
gamma is drawn from U(0.5, 1.5) and beta from U(-0.5, 0.5); the inputs are the two clouds of make_batch(seed=3).
On these the fp32 oracle lies 3.3e-7 ... 3.7e-7 (max-norm) from the fp64 oracle, and the fp64 training-mode output of the
same model 1.5 ... 25 times the largest output away from its inference-mode output, so agreement at 1e-4 -- the bound the
training-mode tests hold features and logits to -- cannot be reached with the wrong statistics.
Observed on MI355X: 3.7e-7 ... 6.3e-7 max-norm (worst row 2.4e-7 ... 4.7e-7), alone and as a joint tensor; the eager path
and the executor bit-equal; no row left out by the arg-max rule in the 20-logit case, 5 of 3140 through the trainer.

The references (_oracle) are computed once per case and shared; nothing writes to them."""
import copy
import functools

import numpy as np
import pytest
import torch

from test_gpu_parity import DEV, _make_models, assert_close, assert_rows_close, rel_err, row_err

pytestmark = pytest.mark.gpu

TOL = 1e-4        # features / logits against the oracle: the bound of the training-mode tests
GAP = 2e-4        # arg-max: rows whose float64 top-two gap is below GAP * largest logit are left out ...
LEFT_OUT = 0.01   # ... and at most this share of the rows may be

CASES = {
    "unet14-32": dict(name="Res16UNet14", out=32, batch_size=1, crop=0.6),
    "unet14-20logits": dict(name="Res16UNet14", out=20, batch_size=1, crop=0.6),
    "unet34c-32": dict(name="Res16UNet34C", out=32, batch_size=2, crop=0.8),
}


@pytest.fixture(scope="module")
def ME():
  import pointcontrast_amd.minkowski as me
  return me


def _cfg(case):
  from pointcontrast_amd.lib.config import get_config
  return get_config([] if case["out"] == 32 else ["net.normalize_feature=False"])


def _models(case, seed):
  """(oracle, device model) with equal weights; the 20-logit pair as test_segmentation_head_forward_loss_and_head_gradients
  builds it."""
  from oracle import model_ref as mr
  from pointcontrast_amd.model import load_model
  cfg = _cfg(case)
  if case["out"] == 32:
    return _make_models(case["name"], cfg, seed=seed)
  torch.manual_seed(seed)
  ref = mr.MODELS[case["name"]](3, case["out"], bn_momentum=cfg.opt.bn_momentum, normalize_feature=False)
  dev = load_model(case["name"])(3, case["out"], cfg, D=3)
  dev.load_state_dict(ref.state_dict())
  return ref, dev.to(DEV)


@functools.lru_cache(maxsize=None)
def _make_batch(seed, batch_size, crop):  # (the synthetic frames are ray-cast on the host: seconds per batch)
  from pointcontrast_amd.lib import synthetic
  return synthetic.make_batch(seed=seed, batch_size=batch_size, crop=crop)


def _batch(case, seed):
  return _make_batch(seed, case["batch_size"], case["crop"])


def _ref_forward(model, b, i, dtype):
  from oracle import sparse_ref as sr
  return model(sr.SparseTensorRef(torch.from_numpy(b["sinput%d_F" % i]).to(dtype), coords=b["sinput%d_C" % i])).F


@functools.lru_cache(maxsize=None)
def _oracle(case_id, seed=0):
  """The references of one case, read-only: `state` (the state_dict after the two training forwards, float32), `batch`
  (make_batch(seed=3)), and per cloud of it in float64: `eval` (inference-mode output), `blocks` (the output of every
  BasicBlock of that forward, in call order) and `train` (training-mode output of the same model on the same input)."""
  from oracle import model_ref as mr
  case = CASES[case_id]
  ref, _ = _models(case, seed)
  gen = torch.Generator().manual_seed(100 + seed)
  with torch.no_grad():
    for m in ref.modules():
      if isinstance(m, mr.BatchNormRef):
        m.bn.weight.copy_(torch.rand(m.bn.weight.shape, generator=gen) + 0.5)
        m.bn.bias.copy_(torch.rand(m.bn.bias.shape, generator=gen) - 0.5)
    ref.train()
    moved = _batch(case, 8)
    for i in range(2):
      _ref_forward(ref, moved, i, torch.float32)
    state = {k: v.clone() for k, v in ref.state_dict().items()}
    for k, v in state.items():
      if k.endswith("running_mean"):
        assert bool((v != 0).all()), k + " has not moved"
      if k.endswith("running_var"):
        assert bool((v != 1).all()), k + " has not moved"
    b = _batch(case, 3)
    ref64 = copy.deepcopy(ref).double().eval()
    blocks = []
    hooks = [m.register_forward_hook(lambda mod, inp, out: blocks[-1].append(out.F.clone()))
             for m in ref64.modules() if isinstance(m, mr.BasicBlockRef)]
    ev = []
    for i in range(2):
      blocks.append([])
      ev.append(_ref_forward(ref64, b, i, torch.float64))
    for h in hooks:
      h.remove()
    for k, v in ref64.state_dict().items():
      assert torch.equal(v, state[k].to(v.dtype)), "the oracle's inference forward moved " + k
    tr = [_ref_forward(copy.deepcopy(ref64).train(), b, i, torch.float64) for i in range(2)]
  return dict(state=state, batch=b, eval=ev, blocks=blocks, train=tr)


def _engine(case_id, seed=0):
  """(device model in eval mode holding _oracle(case_id, seed)["state"], its flat parameters, a NativeEngine)."""
  from pointcontrast_amd.engine import NativeEngine
  from pointcontrast_amd.lib.distributed import FlatParameters
  _, dev = _models(CASES[case_id], seed)
  dev.load_state_dict(_oracle(case_id, seed)["state"])
  dev.eval()
  flat = FlatParameters(dev.parameters())
  return dev, flat, NativeEngine(dev, flat)


def _st(ME, b, i):
  return ME.SparseTensor(torch.from_numpy(b["sinput%d_F" % i]), coords=torch.from_numpy(b["sinput%d_C" % i])).to(DEV)


def _assert_output_close(case_id, got, want, what):
  print("%s: max-norm %.3e, worst row %.3e" % (what, rel_err(got, want), row_err(got, want)))
  if CASES[case_id]["out"] == 32:
    assert_rows_close(got, want, TOL, what)
  else:
    assert_close(got, want, TOL, what)


def _assert_argmax(got, want64, what):
  """The arg-max of `got` equals float64's on every row whose float64 top-two gap is at least GAP of the largest logit;
  returns the rows that are held (a bool vector)."""
  top = want64.topk(2, dim=1).values
  keep = (top[:, 0] - top[:, 1]) >= GAP * want64.abs().max()
  left_out = int((~keep).sum())
  print("%s: %d of %d rows left out by the arg-max rule" % (what, left_out, len(keep)))
  assert left_out <= LEFT_OUT * len(keep), "%s: %d of %d rows are closer than the gap" % (what, left_out, len(keep))
  a, b = got.detach().cpu().argmax(1), want64.argmax(1)
  wrong = int((a[keep] != b[keep]).sum())
  assert wrong == 0, "%s: %d rows with another arg-max than float64's" % (what, wrong)
  return keep


# ------------------------------------------------------------------------------------------------
# 1. the inference BatchNorm kernel, layer-sized
# ------------------------------------------------------------------------------------------------
BN_SHAPES = [(n, c) for n in (1, 255, 257) for c in (4, 20, 32, 1024)] + [(70000, 32)]  # 70000 x 8 float4 > 2048 x 256 threads


@pytest.mark.parametrize("n,c", BN_SHAPES)
def test_batch_norm_eval_matches_float64(n, c):
  """PF.batch_norm_eval (pcmi_bn_fwd_eval: bn_apply_kernel reading (mean, var), a grid-stride loop capped at 2048
  workgroups) against float64 with running statistics at their extremes -- var exactly 0, 1e-12 and 1e6 among the
  channels, |mean| up to 1e3, a zero and a negative gamma -- with and without residual and ReLU.  The input is
  distributed as the statistics say (x = mean + sqrt(var + eps) * N(0, 1)), so every channel's output is O(1) and the
  tolerance, 1e-5 of the largest float64 entry, is as tight for the var = 1e6 channel as for the var = 0 one."""
  from pointcontrast_amd import functional as PF
  g = torch.Generator().manual_seed(1000 * n + c)
  eps = 1e-5
  var = torch.rand(c, generator=g) * 1.5 + 0.5
  var[0], var[1], var[2], var[3] = 0.0, 1e-12, 1e6, 0.0
  mean = (torch.rand(c, generator=g) * 2 - 1) * 1e3
  mean[3] = 1e3
  gamma = torch.rand(c, generator=g) + 0.5
  gamma[c - 1], gamma[c - 2] = 0.0, -1.25
  beta = torch.rand(c, generator=g) - 0.5
  x = (mean.double() + torch.sqrt(var.double() + eps) * torch.randn(n, c, generator=g, dtype=torch.float64)).float()
  res = torch.randn(n, c, generator=g)
  pre = (x.double() - mean.double()) / torch.sqrt(var.double() + eps) * gamma.double() + beta.double()
  dev = [t.to(DEV) for t in (x, gamma, beta, mean, var, res)]
  keep = [t.clone() for t in dev]
  for with_res in (False, True):
    for relu in (False, True):
      want_pre = pre + res.double() if with_res else pre
      want = want_pre.clamp_min(0) if relu else want_pre
      got = PF.batch_norm_eval(dev[0], dev[1], dev[2], dev[3], dev[4], eps, dev[5] if with_res else None, relu).cpu()
      what = "bn eval n=%d c=%d residual=%s relu=%s" % (n, c, with_res, relu)
      assert got.shape == (n, c) and bool(torch.isfinite(got).all()), what
      tol = 1e-5 * float(want.abs().max())
      err = float((got.double() - want).abs().max())
      print("%s: %.3e of the largest entry" % (what, err / float(want.abs().max())))
      assert err <= tol, "%s: %.3e > %.3e" % (what, err, tol)
      if relu:  # the patterns may differ only where the float64 pre-activation is within the tolerance of zero
        differ = (got > 0) != (want_pre > 0)
        worst = float(want_pre[differ].abs().max()) if bool(differ.any()) else 0.0
        assert worst <= tol, "%s: ReLU pattern differs at a float64 pre-activation of %.3e" % (what, worst)
  for t, k in zip(dev, keep):
    assert torch.equal(t, k), "an operand of batch_norm_eval was written"


# ------------------------------------------------------------------------------------------------
# 2. the executor's inference forward against the float64 oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", list(CASES))
def test_inference_forward_matches_float64_oracle(ME, case_id):
  """eng.forward(0, st, training=False) on both clouds: output at 1e-4 (worst row too for the normalised outputs), the
  arg-max of the logits, and the output of every BatchNorm op with a residual -- the fused epilogues, some of them
  writing into slices of the U-Net concatenations -- against the oracle's BasicBlock outputs.  The residual BatchNorm
  ops of the program are in the order the blocks run (the tracer moves such an op behind its residual's producer), so
  the k-th of them is the k-th BasicBlock call; every one is matched."""
  from pointcontrast_amd.engine import OP_BN
  o = _oracle(case_id)
  dev, flat, eng = _engine(case_id)
  res_ops = [op for op in eng._ops if op["type"] == OP_BN and op["in2"] >= 0]
  assert res_ops and all(op["relu"] for op in res_ops)
  assert any(eng._tensors[op["out"]]["parent"] >= 0 for op in eng._ops if op["type"] == OP_BN), "no BN writes into a concatenation"
  for i in range(2):
    want = o["eval"][i]
    got = eng.forward(0, _st(ME, o["batch"], i), training=False)
    what = "%s cloud %d inference output" % (case_id, i)
    _assert_output_close(case_id, got, want, what)
    # the same model with batch statistics is nowhere near: the bound above cannot be met with the wrong statistics
    away = rel_err(o["train"][i], want)
    print("%s: the float64 training-mode output is %.3g of the largest output away" % (what, away))
    assert away > 100 * TOL, away
    if CASES[case_id]["out"] != 32:
      _assert_argmax(got, want, what)
    assert len(res_ops) == len(o["blocks"][i])
    for k, (op, blk) in enumerate(zip(res_ops, o["blocks"][i])):
      act = eng.activation(0, op["out"])
      assert act.shape == blk.shape, "residual BatchNorm %d: %s vs block output %s" % (k, tuple(act.shape), tuple(blk.shape))
      assert_close(act, blk, TOL, "%s cloud %d, block %d (tensor %d)" % (case_id, i, k, op["out"]))


# ------------------------------------------------------------------------------------------------
# 3. the eager path and the executor
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", list(CASES))
def test_eager_eval_forward_matches_the_executor(ME, case_id):
  """model.eval(); model(st).F (one PF.batch_norm_eval per layer) against the executor's inference forward: 1e-5, the
  bound test_engine_matches_autograd_path holds the two paths to in training mode."""
  o = _oracle(case_id)
  dev, flat, eng = _engine(case_id)
  for i in range(2):
    st = _st(ME, o["batch"], i)
    with torch.no_grad():
      eager = dev(st).F
    got = eng.forward(0, st, training=False)
    print("%s cloud %d: eager vs executor bit-equal: %s (max-norm %.3e)" % (case_id, i, torch.equal(eager, got), rel_err(got, eager)))
    assert_close(got, eager, 1e-5, "%s cloud %d executor vs eager" % (case_id, i))
    _assert_output_close(case_id, eager, o["eval"][i], "%s cloud %d eager output" % (case_id, i))


# ------------------------------------------------------------------------------------------------
# 4. what an inference forward must not do, and what it must follow
# ------------------------------------------------------------------------------------------------
def test_inference_forward_changes_no_state(ME):
  o = _oracle("unet14-32")
  dev, flat, eng = _engine("unet14-32")
  st = _st(ME, o["batch"], 0)
  flat.g.normal_()
  before = {k: v.clone() for k, v in dev.state_dict().items()}  # (the pre-hook folds the host-side batch counts in)
  w, g = flat.w.clone(), flat.g.clone()
  y1 = eng.forward(0, st, training=False).clone()
  y2 = eng.forward(0, st, training=False)
  torch.cuda.synchronize()
  assert torch.equal(y1, y2), "two inference forwards of the same input differ"
  after = dev.state_dict()
  assert list(after) == list(before)
  for k, v in before.items():
    assert torch.equal(after[k], v), "an inference forward moved " + k
  assert torch.equal(flat.w, w) and torch.equal(flat.g, g)
  assert any(k.endswith("num_batches_tracked") for k in before)


@pytest.mark.parametrize("switch,case_id", [("PCMI_FWD_BRANCH", "unet34c-32"), ("PCMI_X3_PREPACK", "unet14-32")])
def test_inference_forward_switches_are_bit_equal(ME, switch, case_id, monkeypatch):
  """The residual branches on the side stream (Res16UNet34C has them: a 1x1 convolution followed by two BatchNorm ops)
  and the weight packs at the top of the pass reorder launches, never arithmetic."""
  from pointcontrast_amd.engine import OP_BN, OP_CONV
  o = _oracle(case_id)
  dev, flat, eng = _engine(case_id)
  if switch == "PCMI_FWD_BRANCH":
    ops = eng._ops
    forks = [i for i in range(3, len(ops) - 2) if ops[i]["type"] == OP_CONV and ops[i]["kernel_size"] == 1 and
             ops[i + 1]["type"] == OP_BN and ops[i + 1]["in_"] == ops[i]["out"] and not ops[i + 1]["relu"] and
             ops[i + 1]["in2"] < 0 and ops[i + 2]["type"] == OP_BN and ops[i + 2]["in2"] == ops[i + 1]["out"]]
    assert forks, "the program has no residual branch to put on the side stream"
  st = _st(ME, o["batch"], 0)
  monkeypatch.delenv(switch, raising=False)
  y_on = eng.forward(0, st, training=False).clone()
  monkeypatch.setenv(switch, "0")
  y_off = eng.forward(0, st, training=False)
  torch.cuda.synchronize()
  assert torch.equal(y_on, y_off), "%s=0 changes the inference output (max-norm %.3e)" % (switch, rel_err(y_off, y_on))
  _assert_output_close(case_id, y_off, o["eval"][0], "%s=0 inference output" % switch)


def test_inference_forward_follows_load_state_dict(ME):
  """load_state_dict copies in place: the next inference forward of the SAME engine computes with the new weights and
  running estimates (no pack or statistic cached from the previous pass)."""
  o, other = _oracle("unet14-32"), _oracle("unet14-32", seed=1)
  dev, flat, eng = _engine("unet14-32")
  st = _st(ME, o["batch"], 0)
  y0 = eng.forward(0, st, training=False).clone()
  _assert_output_close("unet14-32", y0, o["eval"][0], "first state")
  ptrs = [m.bn.running_mean.data_ptr() for m in eng._bn_modules] + [flat.w.data_ptr()]
  dev.load_state_dict(other["state"])
  assert ptrs == [m.bn.running_mean.data_ptr() for m in eng._bn_modules] + [flat.w.data_ptr()]
  y1 = eng.forward(0, st, training=False)
  assert rel_err(other["eval"][0], o["eval"][0]) > 100 * TOL  # the two states are far apart
  _assert_output_close("unet14-32", y1, other["eval"][0], "after load_state_dict")


def test_inference_forward_and_the_bf16_mode(ME):
  """set_conv_precision("bf16") and back: the fp32 outputs before and after are bit-equal; the bf16 output differs
  from them and lies within 3e-2 norm-wise, the bound test_bf16_network_matches_fp32_engine holds features to."""
  o = _oracle("unet14-32")
  dev, flat, eng = _engine("unet14-32")
  st = _st(ME, o["batch"], 0)
  y1 = eng.forward(0, st, training=False).clone()
  eng.set_conv_precision("bf16")
  y2 = eng.forward(0, st, training=False).clone()
  eng.set_conv_precision("fp32")
  y3 = eng.forward(0, st, training=False)
  torch.cuda.synchronize()
  assert torch.equal(y1, y3), "the fp32 output changed after a round trip through the bf16 mode"
  assert not torch.equal(y1, y2), "the bf16 mode did not reach the inference forward"
  e_norm = float((y2.double() - y1.double()).norm() / y1.double().norm())
  print("bf16 inference output vs fp32: norm-wise %.3e, max-norm %.3e" % (e_norm, rel_err(y2, y1)))
  assert e_norm <= 3e-2, e_norm


# ------------------------------------------------------------------------------------------------
# 5. pass validity, interleaving with training
# ------------------------------------------------------------------------------------------------
def _running(dev):
  return {k: v.clone() for k, v in dev.state_dict().items() if "running" in k or "num_batches" in k}


def _rewind(dev, state):
  dev.load_state_dict({**dev.state_dict(), **state})


def test_backward_after_an_inference_forward_is_refused(ME):
  from pointcontrast_amd._lib import PcmiError
  o = _oracle("unet14-32")
  dev, flat, eng = _engine("unet14-32")
  dev.train()
  st = _st(ME, o["batch"], 0)
  y = eng.forward(0, st)
  eng.forward(0, st, training=False)
  flat.g.normal_()
  g = flat.g.clone()
  with pytest.raises(PcmiError, match=r"net_backward: pass 0 has no training-mode forward"):
    eng.backward(0, torch.ones_like(y))
  torch.cuda.synchronize()
  assert torch.equal(flat.g, g), "the refused backward wrote gradients"


def test_inference_on_the_other_pass_leaves_training_alone(ME):
  """Validation in the middle of a training iteration: forward(0) in training mode, an inference forward of pass 1,
  backward(0) -- gradients and running estimates bit-equal to the iteration without the inference call, and the
  inference output bit-equal to the one taken behind the backward (same weights, same running estimates)."""
  o = _oracle("unet14-32")
  dev, flat, eng = _engine("unet14-32")
  dev.train()
  st, st2 = _st(ME, o["batch"], 0), _st(ME, o["batch"], 1)
  start = _running(dev)
  runs = []
  for validate in (False, True):
    _rewind(dev, start)
    y = eng.forward(0, st)
    if validate:
      z = eng.forward(1, st2, training=False).clone()
    gy = torch.randn(y.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    flat.zero_grad()
    eng.backward(0, gy)
    torch.cuda.synchronize()
    runs.append((y.clone(), flat.g.clone(), _running(dev)))
    if not validate:
      z_behind = eng.forward(1, st2, training=False).clone()
  assert torch.equal(z, z_behind), "the inference forward between forward(0) and backward(0) computed something else"
  assert torch.equal(runs[0][0], runs[1][0])
  assert float(runs[0][1].abs().max()) > 0
  assert torch.equal(runs[0][1], runs[1][1]), "the inference forward of pass 1 changed the gradients of pass 0"
  for k, v in runs[0][2].items():
    assert torch.equal(runs[1][2][k], v), k
  assert any(not torch.equal(v, start[k]) for k, v in runs[0][2].items())  # (the training forward did move them)


def test_forward_is_refused_while_deferred_running_stats_are_pending(ME):
  """forward(1, defer_running_stats=True) leaves the running-estimate updates of pass 1 for apply_running_stats(1).
  A forward of pass 1 in between would start a new table and drop them: it is refused, in either mode, changes nothing,
  and the following apply_running_stats(1) gives exactly the estimates of the undisturbed sequence; the backward of
  the pass is still its own.  A forward that raises leaves nothing pending behind (forward_pair)."""
  from pointcontrast_amd._lib import PcmiError
  o = _oracle("unet14-32")
  dev, flat, eng = _engine("unet14-32")
  dev.train()
  st, st2 = _st(ME, o["batch"], 0), _st(ME, o["batch"], 1)
  start = _running(dev)
  gy = None
  runs = []
  for disturb in (False, True):
    _rewind(dev, start)
    y = eng.forward(1, st, defer_running_stats=True)
    torch.cuda.synchronize()
    pending = _running(dev)  # (the batch counts have taken this forward, the estimates have not)
    for k, v in pending.items():
      if "running" in k:
        assert torch.equal(v, start[k]), "deferred, but %s moved" % k
    if disturb:
      w, y_before = flat.w.clone(), y.clone()
      held = eng._held[1]
      for training in (False, True):
        with pytest.raises(PcmiError, match=r"net_forward: pass 1 still holds \d+ deferred"):
          eng.forward(1, st2, training=training)
      torch.cuda.synchronize()
      assert eng._held[1] is held and torch.equal(flat.w, w) and torch.equal(y, y_before)
      for k, v in _running(dev).items():
        assert torch.equal(v, pending[k]), "the refused forward moved " + k
      eng.forward(0, st2, training=False)  # another pass is not closed
    eng.apply_running_stats(1)
    if gy is None:
      gy = torch.randn(y.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(6))
    flat.zero_grad()
    eng.backward(1, gy)
    torch.cuda.synchronize()
    runs.append((_running(dev), flat.g.clone()))
  assert any("running" in k and not torch.equal(v, start[k]) for k, v in runs[0][0].items())
  for k, v in runs[0][0].items():
    assert torch.equal(runs[1][0][k], v), "%s after the refused forwards and apply_running_stats" % k
  assert torch.equal(runs[0][1], runs[1][1]), "the gradients of the pass after the refused forwards"
  eng.apply_running_stats(1)  # nothing pending: nothing applied
  torch.cuda.synchronize()
  for k, v in runs[1][0].items():
    assert torch.equal(_running(dev)[k], v), k
  # forward_pair: pass 1 deferred on the side stream, then the forward of pass 0 raises (a row too few for its
  # coordinates; refused before anything is enqueued).  Pass 1 must not stay closed, and its updates are applied.
  _rewind(dev, start)
  bad = ME.SparseTensor(st2.F[:-1], coords_key=st2.coords_key, coords_manager=st2.coords_man)
  with pytest.raises(PcmiError, match=r"feature rows"):
    eng.forward_pair(bad, st)
  torch.cuda.synchronize()
  for k, v in runs[0][0].items():
    if "running" in k:
      assert torch.equal(_running(dev)[k], v), "%s after a forward_pair whose pass 0 raised" % k
  eng.forward(1, st, training=False)
  eng._held[0] = eng._held[1] = None


# ------------------------------------------------------------------------------------------------
# 6. a joint two-cloud tensor
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", list(CASES))
def test_joint_two_cloud_tensor_in_inference_mode(ME, case_id):
  """Both clouds in one tensor with coords_man.set_split(n0): in inference mode the split must not matter -- every
  segment's rows match the float64 oracle's inference output of that cloud alone (which is far from the
  per-segment-statistics result: the training-mode distance asserted in test_inference_forward_matches_float64_oracle)."""
  o = _oracle(case_id)
  dev, flat, eng = _engine(case_id)
  b = o["batch"]
  F = [torch.from_numpy(b["sinput%d_F" % i]) for i in range(2)]
  C = [torch.from_numpy(b["sinput%d_C" % i]) for i in range(2)]
  C1 = C[1].clone()
  C1[:, 0] += int(C[0][:, 0].max()) + 1
  n0 = C[0].shape[0]
  sj = ME.SparseTensor(torch.cat(F), coords=torch.cat([C[0], C1])).to(DEV)
  sj.coords_man.set_split(n0)
  got = eng.forward(0, sj, training=False)
  assert got.shape[0] == n0 + C[1].shape[0]
  _assert_output_close(case_id, got[:n0], o["eval"][0], "%s joint tensor, segment 0" % case_id)
  _assert_output_close(case_id, got[n0:], o["eval"][1], "%s joint tensor, segment 1" % case_id)
  assert rel_err(o["train"][0], o["eval"][0]) > 100 * TOL and rel_err(o["train"][1], o["eval"][1]) > 100 * TOL


# ------------------------------------------------------------------------------------------------
# 7. through the trainer
# ------------------------------------------------------------------------------------------------
def test_segmentation_trainer_inference_matches_float64_oracle():
  """SegmentationTrainer after two fine-tuning steps (the running estimates have moved): forward(training=False) and
  evaluate() on another batch against the float64 oracle holding the trainer's state_dict."""
  from oracle import model_ref as mr, sparse_ref as sr
  from pointcontrast_amd.downstream import semseg as ss
  torch.manual_seed(0)
  tr = ss.SegmentationTrainer(20, model="Res16UNet14", lr=0.05, max_iter=50)
  b = _make_batch(8, 2, 0.6)
  C, F = torch.from_numpy(b["sinput0_C"]), torch.from_numpy(b["sinput0_F"])
  target = torch.from_numpy(np.random.RandomState(1).randint(0, 20, len(C)))
  target[::5] = 255
  for _ in range(2):
    tr.train_iter(C, F, target)
  state = {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}
  assert all(bool((v != 0).any()) for k, v in state.items() if k.endswith("running_mean"))
  assert all(int(v) == 2 for k, v in state.items() if k.endswith("num_batches_tracked"))
  ref = mr.MODELS["Res16UNet14"](3, 20, bn_momentum=0.02, normalize_feature=False).double().eval()
  ref.load_state_dict(state)
  v = _make_batch(3, 1, 0.6)
  Cv, Fv = torch.from_numpy(v["sinput0_C"]), torch.from_numpy(v["sinput0_F"])
  with torch.no_grad():
    want = ref(sr.SparseTensorRef(Fv.double(), coords=Cv.numpy())).F
  got = tr.forward(Cv, Fv, training=False)
  print("trainer inference logits: max-norm %.3e" % rel_err(got, want))
  assert_close(got, want, TOL, "trainer inference logits")
  keep = _assert_argmax(got, want, "trainer inference logits")
  labels = torch.from_numpy(np.random.RandomState(2).randint(0, 20, len(Cv)))
  labels[::7] = 255
  labels[~keep] = 255  # the rows the arg-max rule leaves out leave both sides
  miou, ious, hist = tr.evaluate(Cv, Fv, labels.numpy())
  want_hist = ss.fast_hist(want.argmax(1).numpy(), labels.numpy(), 20)
  assert hist.sum() == int((labels != 255).sum()) > 0
  assert np.array_equal(hist, want_hist), "confusion matrix differs from the float64 oracle's in %d cells" % int((hist != want_hist).sum())
  assert abs(miou - float(np.nanmean(ss.per_class_iu(want_hist) * 100.0))) < 1e-9
  for k, s in tr.model.state_dict().items():
    assert torch.equal(s.cpu(), state[k]), "evaluation moved " + k
