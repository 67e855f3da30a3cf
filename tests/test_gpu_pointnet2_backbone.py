"""VoteNet's PointNet++ backbone on rows (pointcontrast_amd.downstream.votenet: PointnetSAModuleVotes, PointnetFPModule,
Pointnet2Backbone, VoteNet and DetectionTrainer with backbone="pointnet2") on the MI355X against tests/pointnet2_backbone_ref.py,
the float64 restatement that tests/test_pointnet2_backbone_ref.py pins to the reference's own Pointnet2Backbone.forward
(tests/golden/golden_pointnet2_backbone.npz).

The device's furthest-point picks, ball-query neighbourhoods and three nearest neighbours must equal the golden's bit for bit.
Float results: within 1e-4 relative to the tensor's largest entry.  As in tests/test_gpu_votenet_model.py the restatement takes
the device's decisions -- the ReLU patterns and, behind the fused pool, the pooling rows and the sign of the pooled value -- as
data, and every decision that is not its own is held to the forward bound (its margin is within 1e-4 of the tensor's largest
entry)."""
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
import make_golden_pointnet2_backbone as mk  # noqa: E402
import pointnet2_backbone_ref as R  # noqa: E402
import pointset_ref as P  # noqa: E402
import votenet_fixtures as VF  # noqa: E402
import votenet_model_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-4
G = np.load(mk.PATH)
CASE = json.loads(str(G["case"]))
CFG = mk.case_config(CASE)
INDEX_KEYS = ["sa%d_inds" % k for k in (1, 2, 3, 4)] + ["sa%d_idx" % k for k in (1, 2, 3, 4)] + ["fp1_idx", "fp2_idx"]
FLOAT_KEYS = R.OBJ_KEYS + ("fp2_xyz",)


def _mean_size(n):
  return np.random.RandomState(n).uniform(0.4, 1.5, (n, 3)).astype(np.float32)


def _make_backbone(fused_pool=True, seed=None):
  from pointcontrast_amd.downstream import votenet
  torch.manual_seed(0)
  net = votenet.Pointnet2Backbone(input_feature_dim=CASE["F"], npoints=CASE["npoints"], radii=CASE["radii"], nsamples=CASE["nsamples"],
                                  sa_mlps=CASE["sa_mlps"], fp_mlps=CASE["fp_mlps"], fused_pool=fused_pool).to(DEV)
  net.load_state_dict(R.make_params(CFG, CASE["param_seed"] if seed is None else seed))
  return net


def _param_grads(model):
  """Parameter gradients under the reference's names and shapes; the padding of every native gradient is zero."""
  from pointcontrast_amd.downstream import votenet
  out = {}
  for name, mod in model.named_modules():
    if isinstance(mod, votenet.RowConv):
      g = mod.weight.grad
      out[name + ".weight"] = votenet.to_reference_weight(g, mod.in_map, mod.out_map, mod.ref_shape)
      live = torch.zeros_like(g, dtype=torch.bool)
      live[mod.in_map.unsqueeze(1), mod.out_map.unsqueeze(0)] = True
      assert not g[~live].any(), "%s: a padded weight received a gradient" % name
    elif isinstance(mod, votenet.RowBatchNorm):
      out[name + ".weight"], out[name + ".bias"] = mod.weight.grad, mod.bias.grad
  return out


def _padding_is_zero(model):
  from pointcontrast_amd.downstream import votenet
  n = 0
  for name, mod in model.named_modules():
    if isinstance(mod, votenet.RowConv):
      live = torch.zeros_like(mod.weight, dtype=torch.bool)
      live[mod.in_map.unsqueeze(1), mod.out_map.unsqueeze(0)] = True
      assert not mod.weight.detach()[~live].any(), "%s: a padded weight is not zero" % name
      n += int((~live).sum())
      if mod.bias is not None:
        keep = torch.zeros(mod.cout_pad, dtype=torch.bool, device=mod.bias.device)
        keep[mod.out_map] = True
        assert not mod.bias.detach()[0, ~keep].any(), "%s: a padded bias is not zero" % name
  return n


class Decisions:
  """The decisions of a backbone's LAST forward, channel-first as the restatement's tensors are: forward hooks on every
  RowBatchNorm that runs as a module (the ReLU pattern of its fused output), and per set-abstraction level the pooling rows and
  the sign of the pooled value -- from the fused kernel's own argument rows, or (fused_pool=False) from pcmi_rows_maxpool_fwd
  on the hooked output of the last layer."""

  def __init__(self, root, prefix=""):
    from pointcontrast_amd.downstream import votenet
    self.data, self.root, self.prefix = {}, root, prefix
    self.hooks = [m.register_forward_hook(self._hook(n)) for n, m in root.named_modules() if isinstance(m, votenet.RowBatchNorm)]

  def _hook(self, name):
    def hook(mod, args, out):
      self.data[name] = out.detach()
    return hook

  def close(self):
    for h in self.hooks:
      h.remove()

  def get(self, Bn, pooled):
    """pooled: {"sa1": pooled rows [B np, C], ...} of the same forward."""
    from pointcontrast_amd import functional as PF
    out = {}
    for k in (1, 2, 3, 4):
      sa = getattr(self.root, "sa%d" % k)
      last = "sa%d.mlp_module.layer%d.bn.bn" % (k, sa.n_layers - 1)
      arg = sa.last_arg
      if arg is None:
        arg = PF.rows_maxpool(self.data.pop(last), sa.nsample)[1]
      rows = pooled["sa%d" % k]
      Cc = rows.shape[1]
      out["sa%d.pool" % k] = arg.reshape(Bn, sa.npoint, Cc).permute(0, 2, 1).cpu()
      out["sa%d.pool_relu" % k] = (rows.detach() > 0).reshape(Bn, sa.npoint, Cc).permute(0, 2, 1).cpu()
    for name, y in self.data.items():
      Cc = y.shape[1]
      if name.startswith("sa"):
        sa = getattr(self.root, name[:3])
        out[name] = (y > 0).reshape(Bn, sa.npoint, sa.nsample, Cc).permute(0, 3, 1, 2).cpu()
      else:
        out[name] = (y > 0).reshape(Bn, -1, Cc).permute(0, 2, 1).unsqueeze(-1).cpu()
    return out


def _device_indices(net, ep):
  out = {}
  for k in (1, 2, 3, 4):
    sa = getattr(net, "sa%d" % k)
    out["sa%d_inds" % k], out["sa%d_idx" % k] = sa.last_inds.cpu(), sa.last_idx.cpu()
  out["fp1_idx"], out["fp2_idx"] = net.fp1.last_idx.cpu(), net.fp2.last_idx.cpu()
  return out


def _run(net, pc_np, train=True):
  """One forward (and, in training mode, the objective's backward): (end_points, indices, decisions, input gradient)."""
  net.train(train)
  net.zero_grad()
  pc = torch.from_numpy(pc_np).to(DEV).requires_grad_(train)
  seen = Decisions(net)
  with torch.set_grad_enabled(train):
    ep = net(pc)
  seen.close()
  Bn = pc.shape[0]
  pooled = {"sa%d" % k: ep["sa%d_features" % k].transpose(1, 2).reshape(-1, ep["sa%d_features" % k].shape[1]) for k in (1, 2, 3, 4)}
  dec = seen.get(Bn, pooled)
  if train:
    R.objective(ep).backward()
  return ep, _device_indices(net, ep), dec, (pc.grad if train else None)


def _restate(pc_np, indices, decisions, training=True, params=None, stats=None):
  params = M.as_double(params if params is not None else R.make_params(CFG, CASE["param_seed"]), requires_grad=training)
  pc = torch.from_numpy(pc_np).double().requires_grad_(training)
  margins = {}
  ep = R.forward(params, pc, indices, CFG, training=training, stats=stats, decisions=decisions, margins=margins)
  if decisions is not None:
    assert sorted(margins) == sorted(decisions)
    for name, (off, scale) in margins.items():
      print("margin %-34s %.3g of %.3g" % (name, off, scale))
      assert off <= TOL * scale, (name, off, scale)
  if training:
    R.objective(ep).backward()
  return ep, params, pc.grad


@pytest.fixture(scope="module")
def golden_run():
  net = _make_backbone()
  return (net,) + _run(net, G["point_clouds"])


def test_golden_end_points_and_indices(golden_run):
  net, ep, indices, _, _ = golden_run
  for k in INDEX_KEYS:  # bit for bit: the device's sampling, ball query and three-NN are the float32 rules of pointset_ref
    assert indices[k].dtype == torch.int32 and np.array_equal(indices[k].numpy(), G[k]), k
  keys = sorted(k[3:] for k in G.files if k.startswith("ep_"))
  assert sorted(ep) == keys  # the reference's key set
  for k in keys:
    want, got = G["ep_" + k], ep[k]
    assert tuple(got.shape) == want.shape, k
    if want.dtype.kind == "i":
      assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), k
    else:
      assert got.dtype == torch.float32
      e = P.rel_err(got, want)
      print("%-14s %.3g" % (k, e))
      assert e <= TOL, (k, e)
  for k in (1, 2, 3, 4):  # the features are views of the rows
    assert ep["sa%d_features" % k].transpose(1, 2).is_contiguous()
  assert ep["fp2_features"].transpose(1, 2).is_contiguous()


def test_golden_gradients_given_the_device_decisions(golden_run):
  net, ep, indices, dec, gpc = golden_run
  assert len(dec) == 4 * 4 + 4  # per level: two patterns, the rows, the pooled sign; four patterns of the propagations
  want_ep, params, want_gpc = _restate(G["point_clouds"], indices, dec)
  for k in FLOAT_KEYS:
    assert P.rel_err(ep[k], want_ep[k]) <= TOL, (k, P.rel_err(ep[k], want_ep[k]))
  e = P.rel_err(gpc, want_gpc)
  print("input gradient %.3g" % e)
  assert e <= TOL, e
  got = _param_grads(net)
  assert sorted(got) == sorted(n for n, _ in R.backbone_shapes(CFG) if n.endswith((".weight", ".bias")))
  worst = 0.0
  for n, g in got.items():
    e = R.gradient_error(g, params[n].grad)
    worst = max(worst, e)
    assert e <= TOL, (n, e)
  print("largest parameter-gradient error %.3g" % worst)


def test_golden_running_estimates(golden_run):
  net = golden_run[0]
  sd = net.state_dict()
  names = [k[4:] for k in G.files if k.startswith("buf_")]
  assert len(names) == 32
  for n in names:
    assert P.rel_err(sd[n], G["buf_" + n]) <= TOL, (n, P.rel_err(sd[n], G["buf_" + n]))
  assert all(int(v) == 1 for k, v in sd.items() if k.endswith("num_batches_tracked"))


def test_fused_and_composed_pool_agree():
  res = []
  for fused in (True, False):
    net = _make_backbone(fused_pool=fused)
    ep, indices, dec, gpc = _run(net, G["point_clouds"])
    assert (net.sa1.last_arg is not None) == fused
    res.append((ep, _param_grads(net), gpc, net.state_dict(), indices))
  (ep_a, g_a, gpc_a, sd_a, ind_a), (ep_b, g_b, gpc_b, sd_b, ind_b) = res
  for k in INDEX_KEYS:
    assert torch.equal(ind_a[k], ind_b[k]), k
  for k in FLOAT_KEYS:
    assert P.rel_err(ep_a[k], ep_b[k]) <= TOL, (k, P.rel_err(ep_a[k], ep_b[k]))
  assert P.rel_err(gpc_a, gpc_b) <= TOL
  for n in g_a:
    assert R.gradient_error(g_a[n], g_b[n]) <= TOL, (n, R.gradient_error(g_a[n], g_b[n]))
  for n in sd_a:
    if n.endswith(("running_mean", "running_var")):
      assert P.rel_err(sd_a[n], sd_b[n]) <= TOL, n


def test_eval_mode_uses_the_running_estimates():
  net = _make_backbone()
  before = copy.deepcopy(net.state_dict())
  ep, indices, _, _ = _run(net, G["point_clouds"], train=False)
  after = net.state_dict()
  assert all(torch.equal(before[k], after[k]) for k in before), "an eval forward changed the state"
  want, _, _ = _restate(G["point_clouds"], indices, None, training=False)
  for k in FLOAT_KEYS:
    assert P.rel_err(ep[k], want[k]) <= TOL, (k, P.rel_err(ep[k], want[k]))
  train_ep = R.forward(M.as_double(R.make_params(CFG, CASE["param_seed"])), torch.from_numpy(G["point_clouds"]).double(), indices, CFG)
  assert P.rel_err(train_ep["fp2_features"], want["fp2_features"]) > 10 * TOL  # the two modes differ on this fixture


def test_state_dict_is_the_reference_list_and_round_trips():
  net = _make_backbone()
  sd = net.state_dict()
  assert [[k, list(v.shape)] for k, v in sd.items()] == json.loads(str(G["state_shapes"]))
  assert _padding_is_zero(net) > 0
  other = _make_backbone(seed=3)
  assert not torch.equal(other.fp1.mlp.layer0.conv.weight, net.fp1.mlp.layer0.conv.weight)
  other.load_state_dict(copy.deepcopy(sd))
  for a, b in zip(net.parameters(), other.parameters()):
    assert torch.equal(a, b)  # the native (padded) parameters too
  net.eval(), other.eval()
  pc = torch.from_numpy(G["point_clouds"]).to(DEV)
  with torch.no_grad():
    ep_a, ep_b = net(pc), other(pc)
  for k in ep_a:
    assert torch.equal(ep_a[k], ep_b[k]), k
  with pytest.raises(ValueError, match="multiple of 32"):
    from pointcontrast_amd.downstream import votenet
    votenet.PointnetSAModuleVotes(mlp=[0, 16, 32], npoint=4, radius=0.2, nsample=4)


# ---- VoteNet(backbone="pointnet2") at the reference's defaults -----------------------------------------------------------------
B, N = 2, 4096
NUM_PROPOSAL = 64


@pytest.fixture(scope="module")
def scans():
  """Two synthetic ScanNet-style scans of 5000 points in a room of 3 m x 3 m x 1.5 m with a few objects."""
  from pointcontrast_amd.downstream.votenet import SCANNET_NYU40IDS
  rng = np.random.RandomState(21)
  out = []
  for b in range(B):
    n = 5000 + 100 * b
    ins = rng.randint(0, 8, n)
    cen = rng.uniform([0.5, 0.5, 0.3], [2.5, 2.5, 1.2], (8, 3))
    xyz = (cen[ins] + rng.uniform(-0.4, 0.4, (n, 3))).astype(np.float32)
    sem = np.array([0, 3, 4, 5, 1, 7, 8, 9])[ins]
    boxes = np.concatenate([rng.uniform(0.5, 2.5, (5, 3)), rng.uniform(0.3, 0.8, (5, 3)), rng.choice(SCANNET_NYU40IDS, (5, 1))], 1)
    out.append((xyz, ins, sem, boxes))
  return out


@pytest.fixture(scope="module")
def batch(scans):
  from pointcontrast_amd.downstream import votenet
  pipeline = votenet.DetectionInputPipeline("scannet", N, 0.05, DEV, mean_size_arr=_mean_size(18))
  return pipeline(scans, votenet.DetectionDraws.sample([len(s[0]) for s in scans], N, "scannet", 5))


def _config():
  return VF.DatasetConfig(1, _mean_size(18), 18, zero_heading=True)


def test_votenet_with_the_pointnet2_backbone(batch):
  from pointcontrast_amd.downstream import votenet
  dc = _config()
  with pytest.raises(NotImplementedError):
    votenet.VoteNet(18, 1, 18, dc.mean_size_arr, backbone="pointnet")
  torch.manual_seed(0)
  model = votenet.VoteNet(18, 1, 18, dc.mean_size_arr, num_proposal=NUM_PROPOSAL, backbone="pointnet2").to(DEV)
  assert isinstance(model.backbone_net, votenet.Pointnet2Backbone)
  assert tuple(model.state_dict()["backbone_net.sa1.mlp_module.layer0.conv.weight"].shape) == (64, 3, 1, 1)
  assert tuple(model.state_dict()["backbone_net.fp1.mlp.layer0.conv.weight"].shape) == (256, 512, 1, 1)
  model.train()
  inputs = {"point_clouds": batch["point_clouds"]}  # all the forward needs
  runs = []
  for _ in range(2):
    model.zero_grad()
    ep = model(inputs)
    ep.update({k: v for k, v in batch.items() if k not in ep})
    loss, ep = votenet.get_loss(ep, dc)
    loss.backward()
    runs.append((loss.detach().clone(), {k: v.detach().clone() for k, v in ep.items() if torch.is_tensor(v)},
                 [p.grad.clone() for p in model.parameters()]))
  (loss, ep, grads), (loss2, ep2, grads2) = runs
  backbone_keys = {"sa%d_%s" % (k, s) for k in (1, 2, 3, 4) for s in ("xyz", "features")} | {"sa1_inds", "sa2_inds", "fp2_inds", "fp2_xyz",
                                                                                              "fp2_features"}
  head_keys = {"seed_inds", "seed_xyz", "seed_features", "vote_xyz", "vote_features", "aggregated_vote_xyz", "aggregated_vote_inds",
               "objectness_scores", "center", "heading_scores", "heading_residuals_normalized", "heading_residuals", "size_scores",
               "size_residuals_normalized", "size_residuals", "sem_cls_scores"}
  assert backbone_keys | head_keys <= set(ep)
  assert tuple(ep["fp2_features"].shape) == (B, 256, 1024) and tuple(ep["fp2_xyz"].shape) == (B, 1024, 3)
  assert tuple(ep["sa1_features"].shape) == (B, 128, 2048) and tuple(ep["sa4_features"].shape) == (B, 256, 256)
  assert tuple(ep["sa1_xyz"].shape) == (B, 2048, 3) and tuple(ep["sa4_xyz"].shape) == (B, 256, 3)
  assert ep["seed_inds"].dtype == torch.int32 and tuple(ep["seed_inds"].shape) == (B, 1024)
  assert int(ep["seed_inds"].min()) >= 0 and int(ep["seed_inds"].max()) < N
  seeds = torch.gather(batch["point_clouds"][..., 0:3], 1, ep["seed_inds"].long().unsqueeze(-1).expand(-1, -1, 3))
  assert torch.equal(seeds, ep["seed_xyz"]), "seed_inds index the input cloud"
  assert torch.equal(ep["seed_inds"], ep["sa1_inds"][:, :1024])  # the reference's slice, where its comment holds
  assert tuple(ep["center"].shape) == (B, NUM_PROPOSAL, 3) and tuple(ep["sem_cls_scores"].shape) == (B, NUM_PROPOSAL, 18)
  assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(g).all()) for g in grads)
  assert any(bool(g.any()) for g in grads[:3]), "the backbone's first layer received no gradient"
  assert torch.equal(loss, loss2) and all(torch.equal(a, b) for a, b in zip(grads, grads2)), "two runs differ"
  assert all(torch.equal(ep[k], ep2[k]) for k in ep)
  config_dict = dict(remove_empty_box=True, use_3d_nms=True, nms_iou=0.25, use_old_type_nms=False, cls_nms=True, per_class_proposal=True,
                     conf_thresh=0.05, dataset_config=dc)
  decoded = votenet.decode_predictions(runs[1][1] | {"point_clouds": batch["point_clouds"]}, config_dict)
  assert tuple(decoded["obj_prob"].shape) == (B, NUM_PROPOSAL) and bool(torch.isfinite(decoded["corners"]).all())


# ---- DetectionTrainer(backbone="pointnet2") --------------------------------------------------------------------------------------
def test_trainer_with_the_pointnet2_backbone(batch):
  from pointcontrast_amd.downstream import votenet
  dc = _config()
  with pytest.raises(ValueError, match="pretrained"):
    votenet.DetectionTrainer(dc, backbone="pointnet2", pretrained={"state_dict": {}}, device=DEV)
  torch.manual_seed(0)
  t = votenet.DetectionTrainer(dc, num_proposal=NUM_PROPOSAL, backbone="pointnet2", device=DEV)
  assert t.engine is None
  params = dict(t.model.named_parameters())
  lo, hi = t.flat.w.data_ptr(), t.flat.w.data_ptr() + 4 * t.flat.numel
  assert all(lo <= p.data_ptr() < hi for p in params.values()), "every parameter lies in the one flat buffer"
  pads = _padding_is_zero(t.model)
  assert pads > 0
  bns = [m for m in t.model.modules() if isinstance(m, votenet.RowBatchNorm)]
  assert len(bns) == 4 * 3 + 2 * 2 + 2 + 3 + 2 and all(m.momentum == 0.5 for m in bns)
  lr, mom = t.start_epoch(45)
  assert lr == 1e-3 and mom == 0.125 and all(m.momentum == mom for m in bns)
  t.start_epoch(0)
  before = {k: v.detach().clone() for k, v in params.items()}
  small = {k: v for k, v in batch.items() if not k.startswith("voxel_")}  # the batch needs no voxels
  for _ in range(2):
    out = t.train_iter(small)
    assert all(bool(torch.isfinite(out[k])) for k in ("loss", "vote_loss", "objectness_loss", "box_loss", "sem_cls_loss")), out
  assert t.optimizer.steps == 2
  for k, v in params.items():
    assert not torch.equal(v.detach(), before[k]), "%s did not change" % k
  assert _padding_is_zero(t.model) == pads
  state = copy.deepcopy(t.state_dict())
  assert "backbone_net.sa1.mlp_module.layer0.conv.weight" in state["model_state_dict"]
  torch.manual_seed(1)
  fresh = votenet.DetectionTrainer(dc, num_proposal=NUM_PROPOSAL, backbone="pointnet2", device=DEV)
  fresh.load_state_dict(state)
  assert fresh.optimizer.steps == 2
  t.model.eval(), fresh.model.eval()
  with torch.no_grad():
    ep_a, _ = t.forward(t._to_device(small), training=False)
    ep_b, _ = fresh.forward(fresh._to_device(small), training=False)
  for k in ("fp2_features", "vote_xyz", "center", "sem_cls_scores", "seed_inds"):
    assert torch.equal(ep_a[k], ep_b[k]), k
