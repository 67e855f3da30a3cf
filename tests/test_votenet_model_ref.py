"""tests/votenet_model_ref.py (the float64 restatement the GPU tests of the VoteNet head compare against) pinned to
tests/golden/golden_votenet_model.npz, which holds what the reference's own voting and proposal modules computed in float32
on the CPU; plus the host-side pieces of the native head that need no device: the state dict's names and shapes, the
padded parameter layout and the two schedules.

Bound: pointset_ref.rel_err <= 1e-4 (largest deviation over the tensor's largest entry), the project's standing bound.  One
family of gradients is exactly zero in exact arithmetic -- the bias of a convolution that feeds a BatchNorm in training
mode: the normalisation removes any per-channel constant -- so "relative to the tensor's largest entry" has no meaning for
them.  Such a gradient is the plain sum over the rows of the same per-row gradients whose products with the inputs form
the layer's weight gradient, so its rounding error is held to 1e-4 of the weight gradient's largest entry instead
(votenet_model_ref.gradient_error)."""
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
import votenet_model_ref as M  # noqa: E402

TOL = 1e-4
G = np.load(mk.PATH)
CASE = json.loads(str(G["case"]))
NOUT = M.num_outputs(CASE["num_heading_bin"], CASE["num_size_cluster"], CASE["num_class"])
ZERO_GRADIENT = M.ZERO_GRADIENT  # biases in front of a BatchNorm
needs_reference = pytest.mark.skipif(not mk.reference_available(), reason="the reference tree is not present on this host")


def golden_run():
  """The restatement in float64 on the fixture's inputs and indices: (end_points, parameters with .grad, input grads, stats)."""
  params = M.as_double(M.make_params(CASE["C"], CASE["vote_factor"], NOUT, CASE["param_seed"]), requires_grad=True)
  sx = torch.from_numpy(G["seed_xyz"]).double().requires_grad_(True)
  sf = torch.from_numpy(G["seed_features"]).double().requires_grad_(True)
  stats = {}
  ep = M.forward(params, sx, sf, torch.from_numpy(G["ep_aggregated_vote_inds"]), torch.from_numpy(G["idx"]), CASE["vote_factor"],
                 CASE["num_heading_bin"], CASE["num_size_cluster"], CASE["num_class"], G["mean_size_arr"], stats=stats)
  M.objective(ep).backward()
  return ep, params, (sx.grad, sf.grad), stats


RUN = golden_run()


@needs_reference
def test_golden_fixture_is_what_the_reference_modules_produce():
  new = mk.generate()
  assert set(new) == set(G.files)
  for k in G.files:
    assert new[k].dtype == G[k].dtype and new[k].shape == G[k].shape, k
    if new[k].dtype.kind == "f":  # float32 sums whose order the BLAS threading may change
      assert P.rel_err(new[k], G[k]) <= 1e-5 or k[len("pgrad_"):] in ZERO_GRADIENT, k
    else:
      assert np.array_equal(new[k], G[k]), k


def test_fixture_is_small_and_exercises_the_grouping():
  assert os.path.getsize(mk.PATH) < os.path.getsize(os.path.join(HERE, "golden", "golden_small.npz"))
  idx = G["idx"].reshape(-1, G["idx"].shape[-1])
  uniq = [len(set(r)) for r in idx]
  assert max(uniq) > 4 and min(uniq) < idx.shape[1], "the balls hold several votes, and some hold fewer than nsample"
  # the stand-in's indices are the float32 rules of pointset_ref on the fixture's own votes
  vx = G["ep_vote_xyz"]
  inds = np.stack([P.fps(vx[b], CASE["P"]) for b in range(CASE["B"])])
  assert np.array_equal(inds, G["ep_aggregated_vote_inds"])
  new_xyz = np.take_along_axis(vx, inds[..., None].repeat(3, -1).astype(np.int64), 1)
  assert np.array_equal(new_xyz, G["ep_aggregated_vote_xyz"])
  assert np.array_equal(P.ball_query(vx, new_xyz, 0.3, 16), G["idx"])


def test_restatement_matches_the_reference_end_points():
  ep = RUN[0]
  keys = [k for k in G.files if k.startswith("ep_")]
  assert len(keys) == 13
  for k in keys:
    want, got = G[k], ep[k[3:]]
    assert tuple(got.shape) == want.shape, k
    if want.dtype.kind == "i":
      assert np.array_equal(got.numpy(), want)
    else:
      assert P.rel_err(got, want) <= TOL, (k, P.rel_err(got, want))


def test_restatement_matches_the_reference_gradients():
  _, params, (gx, gf), _ = RUN
  assert P.rel_err(gx, G["grad_seed_xyz"]) <= TOL and P.rel_err(gf, G["grad_seed_features"]) <= TOL
  names = [k[len("pgrad_"):] for k in G.files if k.startswith("pgrad_")]
  assert sorted(names) == sorted(n for n, _ in M.head_shapes(CASE["C"], CASE["vote_factor"], NOUT)
                                 if n.endswith(("weight", "bias")))
  for n in names:
    e = M.gradient_error(n, params[n].grad, G["pgrad_" + n], lambda w: G["pgrad_" + w])
    assert e <= TOL, (n, e)
  for n in ZERO_GRADIENT:  # exactly zero but for rounding, in both runs
    assert float(params[n].grad.abs().max()) <= 1e-12 * float(params[n[:-4] + "weight"].grad.abs().max())


def test_restatement_matches_the_reference_running_estimates():
  _, params, _, stats = RUN
  names = [k[len("buf_"):] for k in G.files if k.startswith("buf_")]
  assert len(names) == 14
  for n in names:
    prefix, which = n.rsplit(".", 1)
    batch = stats[prefix][0 if which == "running_mean" else 1]
    want = 0.9 * params[n] + 0.1 * batch  # BatchNorm's default momentum
    assert P.rel_err(want, G["buf_" + n]) <= TOL, n


def test_state_dict_names_and_shapes():
  from pointcontrast_amd.downstream import votenet as V
  ref = [(n, tuple(s)) for n, s in json.loads(str(G["state_shapes"]))]
  assert ref == M.head_shapes(CASE["C"], CASE["vote_factor"], NOUT)
  vgen = V.VotingModule(CASE["vote_factor"], CASE["C"])
  pnet = V.ProposalModule(CASE["num_class"], CASE["num_heading_bin"], CASE["num_size_cluster"], G["mean_size_arr"], CASE["P"],
                          "vote_fps", seed_feat_dim=CASE["C"])
  own = [("vgen." + k, tuple(v.shape)) for k, v in vgen.state_dict().items()] + \
        [("pnet." + k, tuple(v.shape)) for k, v in pnet.state_dict().items()]
  assert own == ref
  # the full-size head of the reference's recipe: the names and shapes the issue quotes
  full = dict(M.head_shapes(256, 1, 79))
  assert full["vgen.conv1.weight"] == (256, 256, 1) and full["pnet.conv3.bias"] == (79,)
  assert full["pnet.vote_aggregation.mlp_module.layer0.conv.weight"] == (128, 259, 1, 1)
  assert full["pnet.vote_aggregation.mlp_module.layer0.bn.bn.running_mean"] == (128,)


@pytest.mark.parametrize("C,vf,heads", [(32, 2, (12, 10, 10)), (256, 1, (1, 18, 18)), (64, 3, (12, 10, 10))])
def test_padded_layout_round_trip_is_exact(C, vf, heads):
  from pointcontrast_amd.downstream import votenet as V
  nout = M.num_outputs(*heads)
  params = M.make_params(C, vf, nout, 3)
  vgen = V.VotingModule(vf, C)
  pnet = V.ProposalModule(heads[2], heads[0], heads[1], np.ones((heads[1], 3), np.float32), 8, "seed_fps", seed_feat_dim=C)
  vgen.load_state_dict({k[5:]: v for k, v in params.items() if k.startswith("vgen.")})
  pnet.load_state_dict({k[5:]: v for k, v in params.items() if k.startswith("pnet.")})
  back = {"vgen." + k: v for k, v in vgen.state_dict().items()}
  back.update({"pnet." + k: v for k, v in pnet.state_dict().items()})
  assert sorted(back) == sorted(params)
  for k, v in params.items():
    assert back[k].dtype == v.dtype and torch.equal(back[k], v), k
  # the native layout itself: [Cin_pad, Cout_pad], features first, xyz behind them, zeros in the padding
  Wb = (C + 3 + 31) // 32 * 32
  w3, ref3 = vgen.conv3.weight.detach(), params["vgen.conv3.weight"][:, :, 0]
  assert tuple(w3.shape) == (C, vf * Wb) and tuple(vgen.conv3.bias.shape) == (1, vf * Wb)
  for v in range(vf):
    blk = w3[:, v * Wb:(v + 1) * Wb]
    assert torch.equal(blk[:, :C], ref3[v * (3 + C) + 3:(v + 1) * (3 + C)].t())  # residual features
    assert torch.equal(blk[:, C:C + 3], ref3[v * (3 + C):v * (3 + C) + 3].t())  # offsets
    assert not blk[:, C + 3:].any() and not vgen.conv3.bias[0, v * Wb + C + 3:(v + 1) * Wb].any()
  w0 = pnet.vote_aggregation.mlp_module.layer0.conv.weight.detach()
  ref0 = params["pnet.vote_aggregation.mlp_module.layer0.conv.weight"][:, :, 0, 0]
  assert tuple(w0.shape) == (Wb, 128)
  assert torch.equal(w0[:C], ref0[:, 3:].t()) and torch.equal(w0[C:C + 3], ref0[:, :3].t()) and not w0[C + 3:].any()
  wl = pnet.conv3.weight.detach()
  assert tuple(wl.shape) == (128, (nout + 31) // 32 * 32) and torch.equal(wl[:, :nout], params["pnet.conv3.weight"][:, :, 0].t())
  assert not wl[:, nout:].any() and not pnet.conv3.bias[0, nout:].any()
  with pytest.raises(RuntimeError, match="size mismatch"):
    vgen.load_state_dict({"conv1.weight": torch.zeros(C, C)}, strict=False)


def test_unknown_sampling_raises():
  from pointcontrast_amd.downstream import votenet as V
  with pytest.raises(ValueError, match="sampling"):
    V.ProposalModule(10, 12, 10, np.ones((10, 3), np.float32), 8, "nearest", seed_feat_dim=32)


def test_schedules():
  from pointcontrast_amd.downstream import votenet as V
  # get_current_lr with learning_rate 1e-3, lr_decay_steps [80, 120, 160], lr_decay_rates [0.1, 0.1, 0.1]
  for epoch, lr in ((0, 1e-3), (79, 1e-3), (80, 1e-4), (119, 1e-4), (120, 1e-5), (159, 1e-5), (160, 1e-6), (179, 1e-6)):
    assert V.detection_lr(epoch) == pytest.approx(lr, rel=1e-12) and M.current_lr(epoch) == pytest.approx(lr, rel=1e-12)
  # bn_lbmd with BN_MOMENTUM_INIT 0.5, bn_decay_rate 0.5, bn_decay_step 20, BN_MOMENTUM_MAX 0.001
  for epoch, mom in ((0, 0.5), (19, 0.5), (20, 0.25), (39, 0.25), (40, 0.125), (100, 0.015625), (160, 0.001953125),
                     (179, 0.001953125), (180, 0.001), (400, 0.001)):
    assert V.detection_bn_momentum(epoch) == mom and M.bn_momentum(epoch) == mom
  # the scheduler sets every BatchNorm of the head, as the reference's does through nn.Module.apply
  vgen = V.VotingModule(1, 32)
  sch = V.BNMomentumScheduler(vgen, V.detection_bn_momentum)
  assert vgen.bn1.momentum == 0.5 and vgen.bn2.momentum == 0.5 and sch.last_epoch == -1
  sch.step(45)
  assert vgen.bn1.momentum == 0.125 and sch.last_epoch == 45
  with pytest.raises(RuntimeError):
    V.BNMomentumScheduler(object(), V.detection_bn_momentum)
