"""The VoteNet network and the detection trainer (pointcontrast_amd.downstream.votenet: VotingModule, ProposalModule, VoteNet,
DetectionTrainer) on the MI355X against tests/votenet_model_ref.py, the float64 restatement that tests/test_votenet_model_ref.py
pins to the reference's own modules.  The restatement is given the device's sampled votes and ball-query neighbourhoods as
data; those indices are checked separately, exactly, against tests/pointset_ref.py on the device's own vote_xyz.  Float
results: within 1e-4 of float64 relative to the tensor's largest entry (votenet_model_ref.gradient_error for the gradients
that are exactly zero).

The gradient of the head jumps where a ReLU switches or the pooling's maximum changes rows, and among the 10^5 pre-activations
of a forward some always lie within fp32 rounding of zero or of their neighbour (measured here before this was added: one such
switch moved single gradient entries by 2 % of the tensor's largest).  As in the step-level comparisons of the backbone, the
restatement therefore takes the device's ReLU patterns and arg-max rows as data (Decisions below), and every decision that is
not the restatement's own is held to the forward bound: it may differ only where the float64 pre-activation (or the gap to
the float64 maximum) is within 1e-4 of the tensor's largest entry."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_votenet_model as mk  # noqa: E402
import pointset_ref as P  # noqa: E402
import votenet_fixtures as VF  # noqa: E402
import votenet_model_ref as M  # noqa: E402
import votenet_ref as LR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-4
B, NUM_POINTS, NUM_SEED, NUM_PROPOSAL, C = 2, 320, 64, 16, 256
HEADS = {"sunrgbd": (12, 10, 10), "scannet": (1, 18, 18)}  # (heading bins, size clusters, classes): 79 and 97 outputs
FLOAT_KEYS = M.OBJ_KEYS


def _mean_size(n):
  return np.random.RandomState(n).uniform(0.4, 1.5, (n, 3)).astype(np.float32)


@pytest.fixture(scope="module")
def scans():
  """Two synthetic ScanNet-style scans (vertices, instance labels, semantic labels, boxes) inside a cube of about a metre:
  about 300 voxels of 5 cm per scene, and 64 seeds dense enough for the 0.3 m balls to hold several votes."""
  from pointcontrast_amd.downstream.votenet import SCANNET_NYU40IDS
  rng = np.random.RandomState(11)
  out = []
  for b in range(B):
    n = 400 + 50 * b
    ins = rng.randint(0, 6, n)
    cen = rng.uniform(1.0, 1.6, (6, 3))
    xyz = (cen[ins] + rng.uniform(-0.25, 0.25, (n, 3))).astype(np.float32)
    sem = np.array([0, 3, 4, 5, 1, 7])[ins]
    boxes = np.concatenate([rng.uniform(1.0, 1.6, (4, 3)), rng.uniform(0.2, 0.6, (4, 3)), rng.choice(SCANNET_NYU40IDS, (4, 1))], 1)
    out.append((xyz, ins, sem, boxes))
  return out


@pytest.fixture(scope="module")
def pipeline():
  from pointcontrast_amd.downstream import votenet
  return votenet.DetectionInputPipeline("scannet", NUM_POINTS, 0.05, DEV, mean_size_arr=_mean_size(18))


@pytest.fixture(scope="module")
def batch(scans, pipeline):
  from pointcontrast_amd.downstream import votenet
  out = pipeline(scans, votenet.DetectionDraws.sample([len(s[0]) for s in scans], NUM_POINTS, "scannet", 5))
  M_ = out["voxel_coords"].shape[0]
  assert 2 * 250 <= M_ <= 2 * NUM_POINTS
  return out


def _make_model(dataset, sampling="vote_fps", seed=1):
  from pointcontrast_amd.downstream import votenet
  H, S, Cls = HEADS[dataset]
  torch.manual_seed(0)
  model = votenet.VoteNet(Cls, H, S, _mean_size(S), num_proposal=NUM_PROPOSAL, vote_factor=1, sampling=sampling, num_seed=NUM_SEED).to(DEV)
  # the head's parameters from the restatement's fill: a reference-shaped state dict, loaded by name (the backbone keeps its own)
  missing = model.load_state_dict(M.make_params(C, 1, M.num_outputs(H, S, Cls), seed), strict=False)
  assert all(k.startswith("backbone_net.") for k in missing.missing_keys) and not missing.unexpected_keys
  return model


def _head_state(model):
  return {k: v.detach().cpu().clone() for k, v in model.state_dict().items() if k.startswith(("vgen.", "pnet."))}


def _param_grads(model):
  """The head's parameter gradients under the reference's names and shapes; the padding of every native gradient is zero."""
  from pointcontrast_amd.downstream import votenet
  out = {}
  for name, mod in model.named_modules():
    if isinstance(mod, votenet.RowConv):
      g = mod.weight.grad
      out[name + ".weight"] = votenet.to_reference_weight(g, mod.in_map, mod.out_map, mod.ref_shape)
      live = torch.zeros_like(g, dtype=torch.bool)
      live[mod.in_map.unsqueeze(1), mod.out_map.unsqueeze(0)] = True
      assert not g[~live].any(), "%s: a padded weight received a gradient" % name
      if mod.bias is not None:
        out[name + ".bias"] = mod.bias.grad[0, mod.out_map]
        keep = torch.zeros(mod.cout_pad, dtype=torch.bool, device=g.device)
        keep[mod.out_map] = True
        assert not mod.bias.grad[0, ~keep].any(), "%s: a padded bias received a gradient" % name
    elif isinstance(mod, votenet.RowBatchNorm):
      out[name + ".weight"], out[name + ".bias"] = mod.weight.grad, mod.bias.grad
  return out


class Decisions:
  """Forward hooks on every RowBatchNorm of a head (`root` holds .vgen and .pnet): the ReLU pattern of its fused output and, behind
  the last layer of the vote aggregation, the arg-max rows of the pooling -- of the LAST forward, channel-first as the
  restatement's tensors are."""

  def __init__(self, root, nsample=16):
    from pointcontrast_amd.downstream import votenet
    self.data, self.ns = {}, nsample
    self.hooks = [m.register_forward_hook(self._hook(n)) for n, m in root.named_modules() if isinstance(m, votenet.RowBatchNorm)]

  def _hook(self, name):
    def hook(mod, args, out):
      self.data[name] = out.detach()
    return hook

  def close(self):
    for h in self.hooks:
      h.remove()

  def get(self, Bn, P_):
    """{BatchNorm prefix: bool pattern, "pool": arg-max rows [B, 128, P]} on the host."""
    from pointcontrast_amd import functional as PF
    out = {}
    for name, y in self.data.items():
      Cc = y.shape[1]
      if ".mlp_module." in name:
        out[name] = (y > 0).reshape(Bn, P_, self.ns, Cc).permute(0, 3, 1, 2).cpu()
        if name.endswith("layer2.bn.bn"):
          out["pool"] = PF.rows_maxpool(y, self.ns)[1].reshape(Bn, P_, Cc).permute(0, 2, 1).cpu()
      else:
        out[name] = (y > 0).reshape(Bn, -1, Cc).permute(0, 2, 1).cpu()
    assert len(out) == 8
    return out


def _restate(params, seed_xyz, seed_features, ep, idx, heads, mean_size, training=True, stats=None, vote_factor=1, decisions=None):
  """The restatement on the device's indices (and decisions); every foreign decision is within the forward bound."""
  H, S, Cls = heads
  margins = {}
  out = M.forward(params, seed_xyz, seed_features, ep["aggregated_vote_inds"].cpu(), idx.cpu(), vote_factor, H, S, Cls, mean_size,
                  training=training, stats=stats, decisions=decisions, margins=margins)
  if decisions is not None:
    assert sorted(margins) == sorted(decisions)
    for name, (off, scale) in margins.items():
      assert off <= TOL * scale, "%s: a decision of the device differs from float64 by %.3e of %.3e" % (name, off, scale)
  return out


def _check_indices(ep, idx_dev, num_proposal, sampling="vote_fps"):
  """aggregated_vote_inds / aggregated_vote_idx are pointset_ref's float32 rules on the device's own vote_xyz, bit for bit."""
  vx = ep["vote_xyz"].detach().cpu().numpy()
  src = vx if sampling == "vote_fps" else ep["seed_xyz"].detach().cpu().numpy()
  inds = np.stack([P.fps(src[b], num_proposal) for b in range(vx.shape[0])])
  assert ep["aggregated_vote_inds"].dtype == torch.int32 and np.array_equal(ep["aggregated_vote_inds"].cpu().numpy(), inds)
  new_xyz = np.take_along_axis(vx, inds[..., None].repeat(3, -1).astype(np.int64), 1)
  assert np.array_equal(ep["aggregated_vote_xyz"].detach().cpu().numpy(), new_xyz)
  idx = P.ball_query(vx, new_xyz, 0.3, 16)
  assert idx_dev.dtype == torch.int32 and np.array_equal(idx_dev.cpu().numpy(), idx)
  return idx


@pytest.mark.parametrize("dataset", ["sunrgbd", "scannet"])
def test_votenet_matches_the_restatement(batch, dataset):
  heads = HEADS[dataset]
  H, S, Cls = heads
  nout = M.num_outputs(*heads)
  assert nout == {"sunrgbd": 79, "scannet": 97}[dataset]
  model = _make_model(dataset)
  model.train()
  old = _head_state(model)
  seen = Decisions(model)
  ep = model(batch)
  # the reference's keys, shapes and dtypes
  K = NUM_SEED
  shapes = dict(seed_inds=(B, K), seed_xyz=(B, K, 3), seed_features=(B, C, K), vote_xyz=(B, K, 3), vote_features=(B, C, K),
                aggregated_vote_xyz=(B, NUM_PROPOSAL, 3), aggregated_vote_inds=(B, NUM_PROPOSAL), objectness_scores=(B, NUM_PROPOSAL, 2),
                center=(B, NUM_PROPOSAL, 3), heading_scores=(B, NUM_PROPOSAL, H), heading_residuals_normalized=(B, NUM_PROPOSAL, H),
                heading_residuals=(B, NUM_PROPOSAL, H), size_scores=(B, NUM_PROPOSAL, S), size_residuals_normalized=(B, NUM_PROPOSAL, S, 3),
                size_residuals=(B, NUM_PROPOSAL, S, 3), sem_cls_scores=(B, NUM_PROPOSAL, Cls))
  assert set(ep) == set(shapes)  # exactly the reference's keys
  idx_dev = model.pnet.last_idx  # the ball query's neighbourhoods of that forward
  for k, s in shapes.items():
    assert tuple(ep[k].shape) == s, k
    assert ep[k].dtype == {"seed_inds": torch.int64, "aggregated_vote_inds": torch.int32}.get(k, torch.float32), k
  idx = _check_indices(ep, idx_dev, NUM_PROPOSAL)
  uniq = [len(set(r)) for r in idx.reshape(-1, 16)]
  assert max(uniq) >= 4 and min(uniq) < 16  # several votes in a ball, and balls padded with their first hit
  # the running estimates after ONE training forward, before anything else runs
  stats = {}
  params = M.as_double(old, requires_grad=True)
  sx64 = ep["seed_xyz"].detach().double().cpu().requires_grad_(True)
  sf64 = ep["seed_features"].detach().double().cpu().requires_grad_(True)
  want = _restate(params, sx64, sf64, ep, idx_dev, heads, model.mean_size_arr, stats=stats, decisions=seen.get(B, NUM_PROPOSAL))
  new = _head_state(model)
  for prefix, (mean, unbiased) in stats.items():
    assert P.rel_err(new[prefix + ".running_mean"], 0.9 * params[prefix + ".running_mean"] + 0.1 * mean) <= TOL, prefix
    assert P.rel_err(new[prefix + ".running_var"], 0.9 * params[prefix + ".running_var"] + 0.1 * unbiased) <= TOL, prefix
    assert int(new[prefix + ".num_batches_tracked"]) == 1
  assert len(stats) == 7
  for k in FLOAT_KEYS:
    assert P.rel_err(ep[k], want[k]) <= TOL, (k, P.rel_err(ep[k], want[k]))
  # gradients: the head alone on leaf copies of its inputs, under the fixed objective
  sx = ep["seed_xyz"].detach().clone().requires_grad_(True)
  rows = ep["seed_features"].detach().transpose(1, 2).reshape(B * K, C).contiguous().requires_grad_(True)
  model.zero_grad()
  ep2 = model.forward_head(sx, rows)
  for k in FLOAT_KEYS + ("aggregated_vote_inds",):
    assert torch.equal(ep2[k], ep[k]), k  # the same bits as inside the whole network
  assert torch.equal(model.pnet.last_idx, idx_dev)
  seen.close()
  M.objective(ep2).backward()
  M.objective(want).backward()
  errors = {"seed_xyz": P.rel_err(sx.grad, sx64.grad), "seed_features": P.rel_err(rows.grad.reshape(B, K, C).transpose(1, 2), sf64.grad)}
  got = _param_grads(model)
  names = [n for n, _ in M.head_shapes(C, 1, nout) if n.endswith((".weight", ".bias"))]
  assert sorted(got) == sorted(names)
  for n in names:
    errors[n] = M.gradient_error(n, got[n], params[n].grad, lambda w: params[w].grad)
  for n, e in errors.items():
    print("gradient of %s: %.3e" % (n, e))
  for n, e in errors.items():
    assert e <= TOL, (n, e)
  # the whole network: the objective's gradient reaches the backbone through the seed gather
  model.zero_grad()
  M.objective(model(batch)).backward()
  g0 = model.backbone_net.net.conv0p1s1.kernel.grad
  assert g0 is not None and bool(torch.isfinite(g0).all()) and bool(g0.any())


def test_eval_mode_uses_the_running_estimates(batch):
  heads = HEADS["sunrgbd"]
  model = _make_model("sunrgbd")
  model.eval()
  state = _head_state(model)
  seen = Decisions(model)
  with torch.no_grad():
    ep = model(batch)
  seen.close()
  assert all(torch.equal(v, _head_state(model)[k]) for k, v in state.items())  # nothing is updated
  want = _restate(M.as_double(state), ep["seed_xyz"].double().cpu(), ep["seed_features"].double().cpu(), ep, model.pnet.last_idx, heads,
                  model.mean_size_arr, training=False, decisions=seen.get(B, NUM_PROPOSAL))
  for k in FLOAT_KEYS:
    assert P.rel_err(ep[k], want[k]) <= TOL, (k, P.rel_err(ep[k], want[k]))
  _check_indices(ep, model.pnet.last_idx, NUM_PROPOSAL)


def test_sampling_modes(batch):
  from pointcontrast_amd.downstream import votenet
  with pytest.raises(ValueError, match="sampling"):
    votenet.VoteNet(10, 12, 10, _mean_size(10), sampling="grid")
  model = _make_model("sunrgbd", sampling="seed_fps")
  model.eval()
  with torch.no_grad():
    ep = model(batch)
    _check_indices(ep, model.pnet.last_idx, NUM_PROPOSAL, "seed_fps")
    model.pnet.sampling = "random"
    inds = torch.from_numpy(np.random.RandomState(0).randint(0, NUM_SEED, (B, NUM_PROPOSAL)).astype(np.int32))
    ep = model(dict(batch, sample_inds=inds))  # the draw as data
    assert torch.equal(ep["aggregated_vote_inds"].cpu(), inds)
    assert torch.equal(ep["aggregated_vote_xyz"], torch.gather(ep["vote_xyz"], 1, inds.to(DEV).long().unsqueeze(-1).expand(-1, -1, 3)))
    ep = model(batch)  # drawn here
    got = ep["aggregated_vote_inds"]
    assert got.dtype == torch.int32 and got.shape == (B, NUM_PROPOSAL) and int(got.min()) >= 0 and int(got.max()) < NUM_SEED


def test_golden_fixture_is_reproduced():
  """The reference's own run (tests/golden/golden_votenet_model.npz: 32 seed features, two votes per seed) on the device."""
  from pointcontrast_amd.downstream import votenet
  G = np.load(mk.PATH)
  case = json.loads(str(G["case"]))
  Cg, vf, nout = case["C"], case["vote_factor"], M.num_outputs(case["num_heading_bin"], case["num_size_cluster"], case["num_class"])
  params = M.make_params(Cg, vf, nout, case["param_seed"])
  vgen = votenet.VotingModule(vf, Cg).to(DEV)
  pnet = votenet.ProposalModule(case["num_class"], case["num_heading_bin"], case["num_size_cluster"], G["mean_size_arr"], case["P"],
                                case["sampling"], seed_feat_dim=Cg).to(DEV)
  vgen.load_state_dict({k[5:]: v for k, v in params.items() if k.startswith("vgen.")})
  pnet.load_state_dict({k[5:]: v for k, v in params.items() if k.startswith("pnet.")})
  Bg, S = case["B"], case["S"]
  sx = torch.from_numpy(G["seed_xyz"]).to(DEV).requires_grad_(True)
  rows = torch.from_numpy(G["seed_features"]).to(DEV).transpose(1, 2).reshape(Bg * S, Cg).contiguous().requires_grad_(True)
  vote_xyz, vote_rows = vgen(sx, rows)
  ep = {"seed_xyz": sx, "vote_xyz": vote_xyz.reshape(Bg, S * vf, 3), "vote_features": vote_rows.reshape(Bg, S * vf, Cg).transpose(1, 2)}
  ep = pnet(ep["vote_xyz"], vote_rows, ep)
  assert np.array_equal(ep["aggregated_vote_inds"].cpu().numpy(), G["ep_aggregated_vote_inds"])
  assert np.array_equal(pnet.last_idx.cpu().numpy(), G["idx"])
  for k in FLOAT_KEYS:
    assert P.rel_err(ep[k], G["ep_" + k]) <= TOL, (k, P.rel_err(ep[k], G["ep_" + k]))
  M.objective(ep).backward()
  assert P.rel_err(sx.grad, G["grad_seed_xyz"]) <= TOL
  assert P.rel_err(rows.grad.reshape(Bg, S, Cg).transpose(1, 2), G["grad_seed_features"]) <= TOL
  holder = torch.nn.Module()
  holder.vgen, holder.pnet = vgen, pnet
  got = _param_grads(holder)
  for n, g in got.items():
    e = M.gradient_error(n, g, G["pgrad_" + n], lambda w: G["pgrad_" + w])
    assert e <= TOL, (n, e)
  for k in G.files:
    if k.startswith("buf_"):
      mod = dict(holder.named_modules())[k[4:].rsplit(".", 1)[0]]
      assert P.rel_err(getattr(mod, k.rsplit(".", 1)[1]), G[k]) <= TOL, k


def test_state_dict_round_trip():
  model = _make_model("scannet")
  sd = model.state_dict()
  head = dict(M.head_shapes(C, 1, 97))
  assert {k: tuple(v.shape) for k, v in sd.items() if not k.startswith("backbone_net.")} == head
  backbone = [k for k in sd if k.startswith("backbone_net.net.")]
  assert "backbone_net.net.conv0p1s1.kernel" in backbone and len(backbone) + len(head) == len(sd)
  other = _make_model("scannet", seed=2)
  assert not torch.equal(other.pnet.conv3.weight, model.pnet.conv3.weight)
  other.load_state_dict(copy.deepcopy(sd))
  sd2 = other.state_dict()
  assert list(sd2) == list(sd) and all(torch.equal(sd2[k], sd[k]) for k in sd)
  for a, b in zip(model.parameters(), other.parameters()):
    assert torch.equal(a, b)  # the native (padded) parameters too


# ---- the trainer ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trainer(pipeline):
  from pointcontrast_amd.downstream import votenet
  torch.manual_seed(0)
  dc = VF.DatasetConfig(1, _mean_size(18), 18, zero_heading=True)
  t = votenet.DetectionTrainer(dc, num_proposal=NUM_PROPOSAL, num_seed=NUM_SEED, input_pipeline=pipeline, device=DEV)
  t.model.load_state_dict(M.make_params(C, 1, 97, 4), strict=False)
  return t


def test_trainer_defaults_and_schedules(trainer):
  g = trainer.optimizer.param_groups[0]
  assert (g["lr"], g["betas"], g["eps"], g["weight_decay"]) == (1e-3, (0.9, 0.999), 1e-8, 0.0)
  assert trainer.engine.n_passes == 1 and trainer.model.backbone_net.net.bn0.bn.momentum == 0.5
  lr, mom = trainer.start_epoch(125)
  assert lr == pytest.approx(1e-5) and g["lr"] == lr and mom == 0.5 * 0.5 ** 6
  assert trainer.model.vgen.bn1.momentum == mom and trainer.model.backbone_net.net.bn0.bn.momentum == mom
  assert trainer.start_epoch(0) == (1e-3, 0.5)
  # head parameters are views of the one flat buffer, behind the backbone's
  w = trainer.model.pnet.conv3.weight
  lo, hi = trainer.flat.w.data_ptr(), trainer.flat.w.data_ptr() + 4 * trainer.flat.numel
  assert lo <= w.data_ptr() < hi and w.grad.data_ptr() - trainer.flat.g.data_ptr() == w.data_ptr() - lo


def test_train_iter_is_reproducible_and_steps_like_adam(trainer, batch):
  """Two train_iter calls from the same state give the same loss bits and the same flat.g.  After the step the head's
  parameters match torch.optim.Adam in float64 applied to the RESTATEMENT's gradients (the float64 head and the float64 loss
  of tests/votenet_ref.py on the device's seeds and indices) within the Adam bound of tests/test_gpu_votehead.py: at most twice
  the error of torch.optim.Adam in fp32 on the CPU against that float64 run, plus one fp32 ulp of the weights.  The fp32 CPU run
  steps on the gradients fp32 has -- the device's flat.g, themselves held to 1e-4 of the restatement's here: Adam's first step
  is lr g / (|g| + eps), so wherever |g| is not far above eps = 1e-8 (and exactly there) the step follows the rounding of g,
  in any fp32 implementation."""
  state = copy.deepcopy(trainer.state_dict())
  w0 = trainer.flat.w.clone()
  out1 = trainer.train_iter(batch)
  g1, w1 = trainer.flat.g.clone(), trainer.flat.w.clone()
  assert set(out1) >= {"loss", "vote_loss", "objectness_loss", "box_loss", "sem_cls_loss"} and out1["loss"].is_cuda
  assert bool(torch.isfinite(out1["loss"])) and bool(torch.isfinite(g1).all()) and not torch.equal(w0, w1)
  trainer.load_state_dict(state)
  assert torch.equal(trainer.flat.w, w0) and trainer.optimizer.steps == 0
  out2 = trainer.train_iter(batch)
  assert torch.equal(out1["loss"], out2["loss"]) and torch.equal(trainer.flat.g, g1) and torch.equal(trainer.flat.w, w1)
  # the restatement of this very step: the head from the pre-step parameters on the device's seeds
  trainer.load_state_dict(state)
  trainer.model.train()
  dev_batch = trainer._to_device(batch)
  seen = Decisions(trainer.model)
  ep, _ = trainer.forward(dev_batch, training=True)
  seen.close()
  params = M.as_double({k: v for k, v in state["model_state_dict"].items() if k.startswith(("vgen.", "pnet."))}, requires_grad=True)
  dc = trainer.config
  want = _restate(params, ep["seed_xyz"].detach().double().cpu(), ep["seed_features"].detach().double().cpu(), ep, trainer.model.pnet.last_idx,
                  (1, 18, 18), dc.mean_size_arr, decisions=seen.get(B, NUM_PROPOSAL))
  ep64 = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in dev_batch.items()}
  ep64.update(want)
  ep64["seed_inds"] = ep["seed_inds"].cpu()
  loss64 = LR.get_loss(ep64, dc.num_heading_bin, dc.mean_size_arr)["loss"]
  assert P.rel_err(out1["loss"], loss64) <= TOL
  loss64.backward()
  trainer.load_state_dict(state)
  names = [n for n, _ in M.head_shapes(C, 1, 97) if n.endswith((".weight", ".bias"))]
  mods = dict(trainer.model.named_modules())
  for n in names:
    mod, leaf = mods[n.rsplit(".", 1)[0]], n.rsplit(".", 1)[1]
    p = getattr(mod, leaf)
    off = (p.data_ptr() - trainer.flat.w.data_ptr()) // 4
    def ref_form(flat_buf):
      t = flat_buf[off:off + p.numel()].view(p.shape)
      if hasattr(mod, "ref_shape"):
        from pointcontrast_amd.downstream.votenet import to_reference_weight
        return to_reference_weight(t, mod.in_map, mod.out_map, mod.ref_shape) if leaf == "weight" else t[0, mod.out_map]
      return t
    g_dev, w_before, w_after = ref_form(g1).cpu(), ref_form(w0).cpu(), ref_form(w1).cpu()
    e = M.gradient_error(n, g_dev, params[n].grad, lambda w: params[w].grad)
    assert e <= TOL, ("gradient", n, e)
    p64 = torch.nn.Parameter(w_before.double().clone())
    p32 = torch.nn.Parameter(w_before.clone())
    p64.grad, p32.grad = params[n].grad.reshape(p64.shape).clone(), g_dev.reshape(p32.shape).clone()
    torch.optim.Adam([p64], lr=1e-3).step()
    torch.optim.Adam([p32], lr=1e-3).step()
    err_dev = float((w_after.double() - p64.data).abs().max())
    err_cpu = float((p32.data.double() - p64.data).abs().max())
    ulp = float(np.spacing(np.float32(p64.data.abs().max())))
    print("adam after one step, %s: device error %.3e, torch fp32 CPU error %.3e, ulp %.3e" % (n, err_dev, err_cpu, ulp))
    assert err_dev <= 2 * err_cpu + ulp, (n, err_dev, err_cpu, ulp)


def test_evaluate_returns_the_ap_dict(trainer, batch):
  dc = trainer.config
  config_dict = dict(remove_empty_box=True, use_3d_nms=True, nms_iou=0.25, use_old_type_nms=False, cls_nms=True, per_class_proposal=True,
                     conf_thresh=0.05, dataset_config=dc)
  w = trainer.flat.w.clone()
  out = trainer.evaluate([batch, batch], config_dict, ap_iou_thresh=(0.25, 0.5))
  assert sorted(out) == [0.25, 0.5]
  for t in out:  # (a class with predictions and no ground truth scores NaN, as in the reference, and so do mAP and AR then)
    assert "mAP" in out[t] and "AR" in out[t] and any(k.endswith("Average Precision") for k in out[t])
    rec = [v for k, v in out[t].items() if k.endswith(" Recall") and np.isfinite(v)]
    assert rec and all(0.0 <= v <= 1.0 for v in rec)
  assert sorted(out[0.25]) == sorted(out[0.5])
  assert all(out[0.5][k] <= out[0.25][k] for k in out[0.5] if k.endswith(" Recall") and np.isfinite(out[0.5][k]))
  assert torch.equal(trainer.flat.w, w) and bool(torch.isfinite(trainer.eval_losses["loss"]))
  assert trainer.ap_calculator.scan_cnt == 2 * B


def test_train_iter_scenes(trainer, scans):
  from pointcontrast_amd.downstream import votenet
  draws = votenet.DetectionDraws.sample([len(s[0]) for s in scans], NUM_POINTS, "scannet", 9)
  steps = trainer.optimizer.steps
  out = trainer.train_iter_scenes(scans, draws)
  assert bool(torch.isfinite(out["loss"])) and trainer.optimizer.steps == steps + 1
  sd = trainer.state_dict()
  assert sd["epoch"] == trainer.epoch and "optimizer_state_dict" in sd
  assert tuple(sd["model_state_dict"]["pnet.conv3.weight"].shape) == (97, 128, 1)
