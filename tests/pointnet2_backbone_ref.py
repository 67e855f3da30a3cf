"""A torch restatement of VoteNet's PointNet++ backbone (downstream/votenet_det_new of the reference:
models/backbone_module.py Pointnet2Backbone over pointnet2_modules.py PointnetSAModuleVotes / PointnetFPModule, QueryAndGroup
and SharedMLP) in the reference's channel-first form and with the reference's parameter names and shapes, in whatever dtype
its input has (the tests use float64).  Every index is DATA (`indices`): the furthest-point picks sa{k}_inds [B, np], the
ball-query neighbourhoods sa{k}_idx [B, np, ns] and the three nearest neighbours fp{k}_idx [B, n, 3] -- the device's own
(checked separately, bit for bit, against tests/pointset_ref.py) or the reference run's.  The interpolation weights are
computed here, from the coordinates and fp{k}_idx, and carry no gradient (three_nn's outputs do not in the reference).

As in tests/votenet_model_ref.py the DECISIONS can be data too (`decisions`): the ReLU pattern behind a BatchNorm (channel
first) under the BatchNorm's prefix, and for the last layer of a set-abstraction module "sa{k}.pool" -- the arg-max rows
[B, C, np] of the pooling -- with "sa{k}.pool_relu", the sign of the pooled value [B, C, np] (the fused kernel never stores
the layer's full output, so its ReLU pattern exists only at the pooled rows).  `margins` then reports how far each foreign
decision lies from the restatement's own: (the largest |pre-activation| whose sign disagrees, the largest |pre-activation|)
for a pattern, (the largest gap between the own maximum and the value at the given row, the largest maximum) for the rows.

The file also holds the references of the two kernels of csrc/rowspool.hip: bn_maxpool_ref (numpy, the fused pass's decision
rule stated directly) and interp_rows_ref (numpy float32, the kernel's operation order).  tests/test_pointnet2_backbone_ref.py
pins all of it against tests/golden/golden_pointnet2_backbone.npz, which holds what the reference's own modules computed."""
import numpy as np
import torch

import votenet_model_ref as M

BN_EPS = M.BN_EPS
# the reference's numbers (backbone_module.py:33-70)
DEFAULT = dict(F=0, npoints=(2048, 1024, 512, 256), radii=(0.2, 0.4, 0.8, 1.2), nsamples=(64, 32, 16, 16),
               sa_mlps=((0, 64, 64, 128), (128, 128, 128, 256), (256, 128, 128, 256), (256, 128, 128, 256)),
               fp_mlps=((512, 256, 256), (512, 256, 256)))
OBJ_KEYS = ("sa1_xyz", "sa1_features", "sa2_xyz", "sa2_features", "sa3_xyz", "sa3_features", "sa4_xyz", "sa4_features",
            "fp2_features")


def config(F=0, **kw):
  cfg = dict(DEFAULT, **kw)
  cfg["F"] = F
  if "sa_mlps" not in kw:
    cfg["sa_mlps"] = ((F,) + DEFAULT["sa_mlps"][0][1:],) + DEFAULT["sa_mlps"][1:]
  return cfg


def backbone_shapes(cfg):
  """[(name, shape)] of the backbone's state dict, in the reference's module order."""
  out = []
  for k, mlp in enumerate(cfg["sa_mlps"]):
    cin = mlp[0] + 3
    for i, cout in enumerate(mlp[1:]):
      p = "sa%d.mlp_module.layer%d" % (k + 1, i)
      out += [(p + ".conv.weight", (cout, cin, 1, 1))] + M._bn_entries(p + ".bn.bn", cout)
      cin = cout
  for k, mlp in enumerate(cfg["fp_mlps"]):
    cin = mlp[0]
    for i, cout in enumerate(mlp[1:]):
      p = "fp%d.mlp.layer%d" % (k + 1, i)
      out += [(p + ".conv.weight", (cout, cin, 1, 1))] + M._bn_entries(p + ".bn.bn", cout)
      cin = cout
  return out


def make_params(cfg, seed):
  return {name: M.fill(name, shape, seed) for name, shape in backbone_shapes(cfg)}


def objective_weight(key, shape):
  n = int(np.prod(shape))
  return torch.cos(torch.arange(n, dtype=torch.float64) * 0.37 + 1.3 * OBJ_KEYS.index(key)).reshape(shape)


def objective(end_points):
  """sum over OBJ_KEYS of <end_points[key], objective_weight(key)>: touches every float tensor the backbone returns."""
  total = 0
  for key in OBJ_KEYS:
    t = end_points[key]
    total = total + (t * objective_weight(key, tuple(t.shape)).to(device=t.device, dtype=t.dtype)).sum()
  return total


def _layer(x, params, p, training, stats):
  return M._bn(M._conv(x, params[p + ".conv.weight"]), params, p + ".bn.bn", training, stats)


def set_abstraction(params, name, xyz, features, inds, idx, radius, n_layers, training=True, stats=None, decisions=None, margins=None):
  """xyz [B, N, 3], features [B, C, N] or None, inds [B, np], idx [B, np, ns] -> (new_xyz [B, np, 3], new_features [B, C', np])."""
  new_xyz = M._gather_points(xyz, inds)
  grouped = (M._gather_points(xyz, idx) - new_xyz.unsqueeze(2)) / radius  # [B, np, ns, 3]
  if features is not None:
    grouped = torch.cat([grouped, M._gather_points(features.transpose(1, 2), idx)], -1)
  x = grouped.permute(0, 3, 1, 2)  # [B, 3 + C, np, ns]
  for i in range(n_layers - 1):
    p = "%s.mlp_module.layer%d" % (name, i)
    x = M._relu(_layer(x, params, p, training, stats), p + ".bn.bn", decisions, margins)
  y = _layer(x, params, "%s.mlp_module.layer%d" % (name, n_layers - 1), training, stats)
  if decisions is not None and name + ".pool" in decisions:
    own = torch.relu(y.detach()).max(dim=3)[0]
    g = torch.gather(y, 3, decisions[name + ".pool"].to(y.device).long().unsqueeze(-1)).squeeze(-1)
    if margins is not None:
      margins[name + ".pool"] = (float((own - torch.relu(g.detach())).abs().max()), float(own.abs().max()))
    return new_xyz, M._relu(g, name + ".pool_relu", decisions, margins)
  return new_xyz, torch.relu(y).max(dim=3)[0]


def interpolation_weights(unknown, known, idx):
  """The reference's weights 1 / (dist + 1e-8), normalised over the three neighbours; no gradient."""
  d = (unknown.detach().unsqueeze(2) - M._gather_points(known.detach(), idx)).pow(2).sum(-1).sqrt()  # [B, n, 3]
  r = 1.0 / (d + 1e-8)
  return r / r.sum(dim=2, keepdim=True)


def feature_propagation(params, name, unknown, known, unknown_feats, known_feats, idx, n_layers, training=True, stats=None,
                        decisions=None, margins=None):
  """unknown [B, n, 3], known [B, m, 3], unknown_feats [B, C1, n], known_feats [B, C2, m], idx [B, n, 3] -> [B, C', n]."""
  w = interpolation_weights(unknown, known, idx).to(known_feats.dtype)
  g = M._gather_points(known_feats.transpose(1, 2), idx)  # [B, n, 3, C2]
  interp = (g * w.unsqueeze(-1)).sum(2).transpose(1, 2)  # [B, C2, n]
  x = torch.cat([interp, unknown_feats], dim=1).unsqueeze(-1)
  for i in range(n_layers):
    p = "%s.mlp.layer%d" % (name, i)
    x = M._relu(_layer(x, params, p, training, stats), p + ".bn.bn", decisions, margins)
  return x.squeeze(-1)


def forward(params, pointcloud, indices, cfg, training=True, stats=None, decisions=None, margins=None):
  """pointcloud [B, N, 3 + F] -> the reference's end_points."""
  xyz = pointcloud[..., 0:3]
  features = pointcloud[..., 3:].transpose(1, 2) if pointcloud.shape[-1] > 3 else None
  ep = {}
  for k in range(4):
    name = "sa%d" % (k + 1)
    xyz, features = set_abstraction(params, name, xyz, features, indices[name + "_inds"], indices[name + "_idx"], cfg["radii"][k],
                                    len(cfg["sa_mlps"][k]) - 1, training, stats, decisions, margins)
    ep[name + "_xyz"], ep[name + "_features"] = xyz, features
  ep["sa1_inds"], ep["sa2_inds"] = indices["sa1_inds"], indices["sa2_inds"]
  f = feature_propagation(params, "fp1", ep["sa3_xyz"], ep["sa4_xyz"], ep["sa3_features"], ep["sa4_features"], indices["fp1_idx"],
                          len(cfg["fp_mlps"][0]) - 1, training, stats, decisions, margins)
  f = feature_propagation(params, "fp2", ep["sa2_xyz"], ep["sa3_xyz"], ep["sa2_features"], f, indices["fp2_idx"],
                          len(cfg["fp_mlps"][1]) - 1, training, stats, decisions, margins)
  ep["fp2_features"], ep["fp2_xyz"] = f, ep["sa2_xyz"]
  ep["fp2_inds"] = indices["sa1_inds"][:, 0:ep["fp2_xyz"].shape[1]]
  return ep


def gradient_error(got, want):
  got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
  return float((got - want).abs().max() / max(float(want.abs().max()), 1e-30))


# ---- the kernels of csrc/rowspool.hip ---------------------------------------------------------------------------------------
def bn_maxpool_ref(x, gamma, beta, ns, eps=BN_EPS, mean=None, var=None):
  """x [R ns, C] -> dict(out [R, C], arg uint8 [R, C], y [R, ns, C], mean, var (biased), unbiased) in float64.  mean / var
  None: batch statistics over all R ns rows.  The fused pass's decision rule stated directly: rows in ascending order, strict >
  on y = relu(gamma (x - mean) / sqrt(var + eps) + beta), a NaN takes the result and is never replaced."""
  x = np.asarray(x, np.float64)
  n, C = x.shape
  R = n // ns
  assert R * ns == n
  g, b = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
  if mean is None:
    mean, var = x.mean(0), x.var(0)
  mean, var = np.asarray(mean, np.float64), np.asarray(var, np.float64)
  with np.errstate(invalid="ignore"):
    y = (x - mean) / np.sqrt(var + eps) * g + b
    y = np.where(np.isnan(y), y, np.maximum(y, 0.0)).reshape(R, ns, C)
    out, arg = y[:, 0].copy(), np.zeros((R, C), np.uint8)
    for s in range(1, ns):
      v = y[:, s]
      take = ~np.isnan(out) & ((v > out) | np.isnan(v))
      out[take], arg[take] = v[take], s
  return dict(out=out, arg=arg, y=y, mean=mean, var=var, unbiased=var * n / max(n - 1, 1))


def bn_maxpool_grad_ref(x, gamma, beta, ns, arg, gout, eps=BN_EPS):
  """(dx, dgamma, dbeta) in float64 of sum(gout * out) for the composition BatchNorm (batch statistics) -> ReLU -> the value
  at row arg[r, c] of every window: torch autograd over float64."""
  xt = torch.as_tensor(np.asarray(x, np.float64)).requires_grad_(True)
  g = torch.as_tensor(np.asarray(gamma, np.float64)).requires_grad_(True)
  b = torch.as_tensor(np.asarray(beta, np.float64)).requires_grad_(True)
  n, C = xt.shape
  y = torch.relu((xt - xt.mean(0)) / torch.sqrt(xt.var(0, unbiased=False) + eps) * g + b).reshape(n // ns, ns, C)
  out = torch.gather(y, 1, torch.as_tensor(np.asarray(arg)).long().unsqueeze(1)).squeeze(1)
  (out * torch.as_tensor(np.asarray(gout, np.float64))).sum().backward()
  return xt.grad.numpy(), g.grad.numpy(), b.grad.numpy()


def interp_rows_ref(known, idx, weight, skip, out_ld):
  """known [B m, C2], idx / weight [B, n, 3], skip [B n, C1] or None -> float32 [B n, out_ld]: ((w0 f0) + (w1 f1)) + (w2 f2) with
  every operation rounded to float32 on its own, then skip, then zeros.  An index outside [0, m) reads as 0."""
  known, w = np.asarray(known, np.float32), np.asarray(weight, np.float32)
  idx = np.asarray(idx)
  B, n, _ = idx.shape
  m, C2 = known.shape[0] // B, known.shape[1]
  C1 = 0 if skip is None else skip.shape[1]
  out = np.zeros((B * n, out_ld), np.float32)
  f = []
  for k in range(3):
    t = idx[:, :, k]
    ok = (t >= 0) & (t < m)
    rows = (np.arange(B)[:, None] * m + np.where(ok, t, 0)).reshape(-1)
    f.append(np.where(ok.reshape(-1, 1), known[rows], np.float32(0)).astype(np.float32))
  w = w.reshape(B * n, 3)
  out[:, :C2] = ((w[:, 0:1] * f[0]) + (w[:, 1:2] * f[1])) + (w[:, 2:3] * f[2])
  if C1:
    out[:, C2:C2 + C1] = np.asarray(skip, np.float32)
  return out
