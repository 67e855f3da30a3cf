"""tests/pointnet2_backbone_ref.py (the float64 restatement and the kernel references that the GPU tests of the PointNet++
backbone compare against) pinned to tests/golden/golden_pointnet2_backbone.npz, which holds what the reference's own
Pointnet2Backbone.forward computed in float32 on the CPU; plus bn_maxpool_ref against the float64 composition BatchNorm -> ReLU
-> max, and interp_rows_ref against pointset_ref.interpolate and the concatenation.

Bound: pointset_ref.rel_err <= 1e-4 (largest deviation over the tensor's largest entry), the project's standing bound."""
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
import votenet_model_ref as M  # noqa: E402

TOL = 1e-4
G = np.load(mk.PATH)
CASE = json.loads(str(G["case"]))
CFG = mk.case_config(CASE)
INDEX_KEYS = ["sa%d_inds" % k for k in (1, 2, 3, 4)] + ["sa%d_idx" % k for k in (1, 2, 3, 4)] + ["fp1_idx", "fp2_idx"]
needs_reference = pytest.mark.skipif(not mk.reference_available(), reason="the reference tree is not present on this host")


def golden_indices():
  return {k: torch.from_numpy(G[k]) for k in INDEX_KEYS}


def golden_run():
  """The restatement in float64 on the fixture's input and indices: (end_points, parameters with .grad, input grad, stats)."""
  params = M.as_double(R.make_params(CFG, CASE["param_seed"]), requires_grad=True)
  pc = torch.from_numpy(G["point_clouds"]).double().requires_grad_(True)
  stats = {}
  ep = R.forward(params, pc, golden_indices(), CFG, stats=stats)
  R.objective(ep).backward()
  return ep, params, pc.grad, stats


RUN = golden_run()


@needs_reference
def test_golden_fixture_is_what_the_reference_modules_produce():
  new = mk.generate()
  assert set(new) == set(G.files)
  for k in G.files:
    assert new[k].dtype == G[k].dtype and new[k].shape == G[k].shape, k
    if new[k].dtype.kind == "f":  # float32 sums whose order the BLAS threading may change
      assert P.rel_err(new[k], G[k]) <= 1e-5, k
    else:
      assert np.array_equal(new[k], G[k]), k


def test_fixture_is_small_and_exercises_padding_and_ties():
  assert os.path.getsize(mk.PATH) < (1 << 19)
  pc = G["point_clouds"]
  assert pc.shape == (CASE["B"], CASE["N"], 3 + CASE["F"])
  # the stand-in's indices are the float32 rules of pointset_ref on the fixture's own coordinates, level by level
  xyz = pc[..., 0:3]
  for k in range(4):
    inds = np.stack([P.fps(xyz[b], CASE["npoints"][k]) for b in range(CASE["B"])])
    assert np.array_equal(inds, G["sa%d_inds" % (k + 1)])
    new_xyz = np.take_along_axis(xyz, inds[..., None].repeat(3, -1).astype(np.int64), 1)
    assert np.array_equal(new_xyz, G["ep_sa%d_xyz" % (k + 1)])
    idx = G["sa%d_idx" % (k + 1)]
    assert np.array_equal(P.ball_query(xyz, new_xyz, CASE["radii"][k], CASE["nsamples"][k]), idx)
    xyz = new_xyz
  for k, (u, kn) in enumerate((("sa3", "sa4"), ("sa2", "sa3"))):
    assert np.array_equal(P.three_nn(G["ep_%s_xyz" % u], G["ep_%s_xyz" % kn])[1], G["fp%d_idx" % (k + 1)])
  # many balls of the first level hold only their centre (the whole window repeats one row: ties), others several points
  uniq = np.array([len(set(r)) for r in G["sa1_idx"].reshape(-1, CASE["nsamples"][0])])
  assert (uniq == 1).sum() > 10 and uniq.max() > 2
  # the reference's comment holds on this fixture: the second level's picks are the first ones of the first level's
  assert np.array_equal(G["sa2_inds"], np.arange(CASE["npoints"][1], dtype=np.int32)[None].repeat(CASE["B"], 0))
  assert np.array_equal(G["ep_fp2_inds"], G["sa1_inds"][:, :CASE["npoints"][1]])


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
  _, params, gpc, _ = RUN
  assert P.rel_err(gpc, G["grad_point_clouds"]) <= TOL, P.rel_err(gpc, G["grad_point_clouds"])
  names = [k[len("pgrad_"):] for k in G.files if k.startswith("pgrad_")]
  assert sorted(names) == sorted(n for n, _ in R.backbone_shapes(CFG) if n.endswith(("weight", "bias")))
  for n in names:
    e = R.gradient_error(params[n].grad, G["pgrad_" + n])
    assert e <= TOL, (n, e)


def test_restatement_matches_the_reference_running_estimates():
  _, params, _, stats = RUN
  names = [k[len("buf_"):] for k in G.files if k.startswith("buf_")]
  assert len(names) == 2 * 16
  for n in names:
    prefix, which = n.rsplit(".", 1)
    batch = stats[prefix][0 if which == "running_mean" else 1]
    want = 0.9 * params[n] + 0.1 * batch  # BatchNorm's default momentum
    assert P.rel_err(want, G["buf_" + n]) <= TOL, n


def test_state_dict_names_and_shapes_are_the_reference_list():
  assert json.loads(str(G["state_shapes"])) == [[n, list(s)] for n, s in R.backbone_shapes(CFG)]
  # the reference's defaults: the names the issue quotes
  full = dict(R.backbone_shapes(R.config(F=1)))
  assert full["sa1.mlp_module.layer0.conv.weight"] == (64, 4, 1, 1)
  assert full["sa1.mlp_module.layer0.bn.bn.running_mean"] == (64,)
  assert full["fp1.mlp.layer0.conv.weight"] == (256, 512, 1, 1)
  assert full["sa4.mlp_module.layer2.conv.weight"] == (256, 128, 1, 1)


def test_decisions_given_back_reproduce_the_run_with_zero_margins():
  """The restatement's own decisions handed back as data change nothing, and every margin's first entry is exactly 0."""
  params = M.as_double(R.make_params(CFG, CASE["param_seed"]))
  pc = torch.from_numpy(G["point_clouds"]).double()
  own = {}
  ep0 = R.forward(params, pc, golden_indices(), CFG)
  saved = M._relu  # a second pass that records the sign of every pre-activation the restatement decides on

  def spy(y, name, decisions, margins):
    own[name] = (y.detach() > 0)
    return saved(y, name, None, None)

  M._relu = spy
  try:
    R.forward(params, pc, golden_indices(), CFG, decisions={})
  finally:
    M._relu = saved
  assert len(own) == 4 * 2 + 2 * 2  # every layer but the pooled ones
  margins = {}
  ep1 = R.forward(params, pc, golden_indices(), CFG, decisions=own, margins=margins)
  assert sorted(margins) == sorted(own)
  assert all(m[0] == 0.0 for m in margins.values())
  for k in R.OBJ_KEYS:
    assert torch.equal(ep0[k], ep1[k]), k
  # the pooling's rows as data: the first maximal row of the float64 output
  xyz, feats = pc[..., 0:3], pc[..., 3:].transpose(1, 2)
  idx = golden_indices()
  new_xyz = M._gather_points(xyz, idx["sa1_inds"])
  grouped = torch.cat([(M._gather_points(xyz, idx["sa1_idx"]) - new_xyz.unsqueeze(2)) / CFG["radii"][0],
                       M._gather_points(feats.transpose(1, 2), idx["sa1_idx"])], -1).permute(0, 3, 1, 2)
  x = grouped
  for i in range(2):
    x = torch.relu(R._layer(x, params, "sa1.mlp_module.layer%d" % i, True, None))
  y = torch.relu(R._layer(x, params, "sa1.mlp_module.layer2", True, None))
  rows = y.argmax(dim=3)
  dec = {"sa1.pool": rows, "sa1.pool_relu": torch.gather(y, 3, rows.unsqueeze(-1)).squeeze(-1) > 0}
  margins = {}
  ep2 = R.forward(params, pc, golden_indices(), CFG, decisions=dec, margins=margins)
  assert margins["sa1.pool"][0] == 0.0 and margins["sa1.pool_relu"][0] == 0.0
  for k in R.OBJ_KEYS:
    assert P.rel_err(ep2[k], ep0[k]) <= 1e-12, k


# ---- bn_maxpool_ref ---------------------------------------------------------------------------------------------------------
def _composition(x, gamma, beta, ns, eps=R.BN_EPS):
  """BatchNorm (batch statistics) -> ReLU -> max over every ns rows, in float64 torch."""
  xt = torch.as_tensor(np.asarray(x, np.float64))
  y = (xt - xt.mean(0)) / torch.sqrt(xt.var(0, unbiased=False) + eps) * torch.as_tensor(np.asarray(gamma, np.float64)) + \
      torch.as_tensor(np.asarray(beta, np.float64))
  y = torch.relu(y).reshape(xt.shape[0] // ns, ns, xt.shape[1])
  return y, y.max(dim=1)[0]


@pytest.mark.parametrize("R_,ns,C", [(1, 1, 1), (7, 2, 5), (5, 16, 8), (3, 64, 4)])
def test_bn_maxpool_ref_is_the_composition(R_, ns, C):
  rng = np.random.RandomState(R_ * 1000 + ns * 10 + C)
  x = rng.normal(0, 1, (R_ * ns, C)).astype(np.float32)
  gamma, beta = rng.uniform(0.5, 1.5, C), rng.normal(0, 0.3, C)
  if C > 1:
    gamma[1] = -gamma[1]  # a negative gamma reverses the order: the maximum is over y, not x
  ref = R.bn_maxpool_ref(x, gamma, beta, ns)
  y, want = _composition(x, gamma, beta, ns)
  assert P.rel_err(ref["out"], want) <= 1e-12
  assert P.rel_err(ref["y"], y) <= 1e-12
  got_rows = np.take_along_axis(ref["y"], ref["arg"][:, None, :].astype(np.int64), 1)[:, 0]
  assert np.array_equal(got_rows, ref["out"])
  # the lowest row among equals: no earlier row holds the same value
  for r in range(R_):
    for c in range(C):
      assert not (ref["y"][r, :ref["arg"][r, c], c] == ref["out"][r, c]).any()
  if C > 1 and ns > 1:
    xs = x.reshape(R_, ns, C)
    live = ref["out"][:, 1] > 0
    assert np.array_equal(ref["arg"][live, 1], xs[:, :, 1].argmin(1)[live])  # negative gamma: the smallest x wins


def test_bn_maxpool_ref_special_cases():
  rng = np.random.RandomState(3)
  ns, C = 4, 6
  x = rng.normal(0, 1, (5 * ns, C)).astype(np.float32)
  gamma, beta = np.ones(C), np.zeros(C)
  gamma[0], beta[0] = 0.0, -1.0      # column 0: y == -1 everywhere -> relu 0 everywhere -> (0, row 0)
  beta[1] = -100.0                   # column 1: entirely <= 0 in every window
  x[4:8] = x[4]                      # window 1: identical rows -> the lowest row
  x[9, 3] = np.nan                   # a NaN poisons the batch statistics of column 3: every y of the column is NaN
  ref = R.bn_maxpool_ref(x, gamma, beta, ns)
  assert (ref["out"][:, 0] == 0).all() and (ref["arg"][:, 0] == 0).all()
  assert (ref["out"][:, 1] == 0).all() and (ref["arg"][:, 1] == 0).all()
  assert (ref["arg"][1, [2, 4, 5]] == 0).all()
  assert np.isnan(ref["out"][:, 3]).all() and (ref["arg"][:, 3] == 0).all()
  # with given (running) statistics a NaN stays local: the lowest NaN row of its window, nothing else changes
  x2 = x.copy()
  x2[10, 3] = np.nan
  ev = R.bn_maxpool_ref(x2, gamma, beta, ns, mean=np.zeros(C), var=np.ones(C))
  assert np.isnan(ev["out"][2, 3]) and ev["arg"][2, 3] == 1
  assert not np.isnan(np.delete(ev["out"], 2, 0)[:, 3]).any()
  clean = np.where(np.isnan(x2), 0.0, x2)
  ev0 = R.bn_maxpool_ref(clean, gamma, beta, ns, mean=np.zeros(C), var=np.ones(C))
  keep = np.ones_like(ev["out"], bool)
  keep[2, 3] = False
  assert np.array_equal(ev["out"][keep], ev0["out"][keep]) and np.array_equal(ev["arg"][keep], ev0["arg"][keep])
  # one row in all: the variance is 0 and the unbiased one is the biased one (pcmi_bn_fwd_train's n == 1 guard)
  one = R.bn_maxpool_ref(x[:1], gamma, beta, 1)
  assert (one["var"] == 0).all() and (one["unbiased"] == 0).all()


def test_bn_maxpool_grad_ref_scatters_to_the_argument_rows():
  rng = np.random.RandomState(5)
  R_, ns, C = 6, 4, 3
  x = rng.normal(0, 1, (R_ * ns, C)).astype(np.float32)
  gamma, beta = rng.uniform(0.5, 1.5, C), rng.normal(0, 0.3, C)
  ref = R.bn_maxpool_ref(x, gamma, beta, ns)
  gout = rng.normal(0, 1, (R_, C))
  dx, dgamma, dbeta = R.bn_maxpool_grad_ref(x, gamma, beta, ns, ref["arg"], gout)
  g = np.where(ref["out"] > 0, gout, 0.0)
  assert P.rel_err(dbeta, g.sum(0)) <= 1e-12
  n = R_ * ns
  xh = (x - ref["mean"]) / np.sqrt(ref["var"] + R.BN_EPS)
  xh_at = np.take_along_axis(xh.reshape(R_, ns, C), ref["arg"][:, None, :].astype(np.int64), 1)[:, 0]
  assert P.rel_err(dgamma, (g * xh_at).sum(0)) <= 1e-12
  gi = np.zeros((R_, ns, C))
  np.put_along_axis(gi, ref["arg"][:, None, :].astype(np.int64), g[:, None, :], 1)
  want = gamma / np.sqrt(ref["var"] + R.BN_EPS) * (gi.reshape(n, C) - g.sum(0) / n - xh * (g * xh_at).sum(0) / n)
  assert P.rel_err(dx, want) <= 1e-10


# ---- interp_rows_ref ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,n,m,C2,C1", [(1, 1, 3, 1, 0), (2, 65, 64, 32, 5), (2, 9, 3, 260, 256)])
def test_interp_rows_ref_is_interpolate_plus_concatenation(B, n, m, C2, C1):
  rng = np.random.RandomState(B * 100 + n + C2)
  known = rng.normal(0, 1, (B * m, C2)).astype(np.float32)
  idx = rng.randint(0, m, (B, n, 3)).astype(np.int32)
  idx[0, 0] = idx[0, 0, 0]  # all three indices equal
  w = rng.uniform(0, 1, (B, n, 3)).astype(np.float32)
  w /= w.sum(-1, keepdims=True)
  skip = rng.normal(0, 1, (B * n, C1)).astype(np.float32) if C1 else None
  ld = (C2 + C1 + 31) // 32 * 32
  out = R.interp_rows_ref(known, idx, w, skip, ld)
  assert out.dtype == np.float32 and out.shape == (B * n, ld)
  cf = torch.from_numpy(known).double().reshape(B, m, C2).transpose(1, 2)
  want = P.interpolate(cf, torch.from_numpy(idx), torch.from_numpy(w).double()).transpose(1, 2).reshape(B * n, C2)
  assert P.rel_err(out[:, :C2], want) <= 1e-6
  if C1:
    assert np.array_equal(out[:, C2:C2 + C1], skip)
  assert not out[:, C2 + C1:].any()
  # an index outside [0, m) reads as 0
  bad = idx.copy()
  bad[0, 0, 1], bad[B - 1, n - 1, 2] = m, -1
  w0 = w.copy()
  w0[0, 0, 1] = w0[B - 1, n - 1, 2] = 0
  assert np.array_equal(R.interp_rows_ref(known, bad, w, skip, ld), R.interp_rows_ref(known, np.clip(bad, 0, m - 1), w0, skip, ld))
