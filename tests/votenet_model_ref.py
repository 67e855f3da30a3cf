"""A torch restatement of the VoteNet head (downstream/votenet_det_new of the reference: models/voting_module.py,
models/votenet.py:120-121, models/proposal_module.py with PointnetSAModuleVotes / QueryAndGroup / SharedMLP) in the
reference's channel-first form and with the reference's parameter names and shapes, in whatever dtype its inputs have
(the tests use float64).  The sampled indices `sample_inds` [B, P] and the ball-query indices `idx` [B, P, ns] are DATA: the
device's own (checked separately, bit for bit, against tests/pointset_ref.py) or the reference run's.

The head's gradient is discontinuous where a ReLU switches or the maximum over a neighbourhood changes rows, and some
pre-activation always lies within fp32 rounding of such a switch.  So, like the step-level comparisons of the backbone, the
restatement can be handed the device's DECISIONS as data too (`decisions`: the ReLU pattern behind every BatchNorm, channel
first, and the arg-max rows of the pooling): it then multiplies by the pattern and gathers at the rows instead of deciding
itself, and reports in `margins` how far each foreign decision lies from its own -- the largest |pre-activation| whose sign
it would have taken otherwise, the largest gap between its own maximum and the gathered value -- which the tests hold to the
bound of the forward values.  Without `decisions` it decides itself.

Parameters come from a seeded, name-keyed fill (make_params), so that fixtures need not store them.
tests/test_votenet_model_ref.py pins this file against tests/golden/golden_votenet_model.npz, which holds what the
reference's own modules computed."""
import zlib

import numpy as np
import torch

BN_EPS = 1e-5
SA_MLP = (128, 128, 128)
OBJ_KEYS = ("vote_xyz", "vote_features", "aggregated_vote_xyz", "objectness_scores", "center", "heading_scores",
            "heading_residuals_normalized", "heading_residuals", "size_scores", "size_residuals_normalized", "size_residuals",
            "sem_cls_scores")


def num_outputs(num_heading_bin, num_size_cluster, num_class):
  return 2 + 3 + num_heading_bin * 2 + num_size_cluster * 4 + num_class


def _bn_entries(prefix, c):
  return [(prefix + ".weight", (c,)), (prefix + ".bias", (c,)), (prefix + ".running_mean", (c,)), (prefix + ".running_var", (c,)),
          (prefix + ".num_batches_tracked", ())]


def head_shapes(C, vote_factor, nout):
  """[(name, shape)] of the head's state dict, in the reference's module order."""
  out = []
  for k in (1, 2):
    out += [("vgen.conv%d.weight" % k, (C, C, 1)), ("vgen.conv%d.bias" % k, (C,))]
  out += [("vgen.conv3.weight", ((3 + C) * vote_factor, C, 1)), ("vgen.conv3.bias", ((3 + C) * vote_factor,))]
  out += _bn_entries("vgen.bn1", C) + _bn_entries("vgen.bn2", C)
  cin = C + 3
  for i, cout in enumerate(SA_MLP):
    p = "pnet.vote_aggregation.mlp_module.layer%d" % i
    out += [(p + ".conv.weight", (cout, cin, 1, 1))] + _bn_entries(p + ".bn.bn", cout)
    cin = cout
  for k, cout in ((1, 128), (2, 128), (3, nout)):
    out += [("pnet.conv%d.weight" % k, (cout, 128, 1)), ("pnet.conv%d.bias" % k, (cout,))]
  out += _bn_entries("pnet.bn1", 128) + _bn_entries("pnet.bn2", 128)
  return out


def fill(name, shape, seed):
  """The value of parameter / buffer `name`: a stream keyed by the name and the seed.  BatchNorm weights and running
  variances stay in [0.5, 1.5] (gamma away from 0), convolution weights have unit gain, everything else is small; the
  voting module's last layer is a tenth of that, so that the votes stay near their seeds and the balls of the vote
  aggregation hold several of them."""
  rng = np.random.RandomState((zlib.crc32(name.encode()) ^ (seed * 2654435761)) & 0x7fffffff)
  leaf = name.rsplit(".", 1)[1]
  if leaf == "num_batches_tracked":
    return torch.zeros((), dtype=torch.int64)
  if leaf == "running_var" or (leaf == "weight" and len(shape) == 1):
    v = rng.uniform(0.5, 1.5, shape)
  elif leaf == "weight":
    v = rng.normal(0.0, 1.0 / np.sqrt(shape[1]), shape)
  else:
    v = rng.normal(0.0, 0.1, shape)
  if name.startswith("vgen.conv3."):
    v = v * 0.1
  return torch.from_numpy(np.asarray(v, np.float32))


def make_params(C, vote_factor, nout, seed):
  return {name: fill(name, shape, seed) for name, shape in head_shapes(C, vote_factor, nout)}


def objective_weight(key, shape):
  """The fixed weights of the scalar objective for end_points[key]: a cosine pattern, no random stream."""
  n = int(np.prod(shape))
  k = OBJ_KEYS.index(key)
  return torch.cos(torch.arange(n, dtype=torch.float64) * 0.37 + 1.3 * k).reshape(shape)


def objective(end_points):
  """sum over OBJ_KEYS of <end_points[key], objective_weight(key)>: touches every predicted tensor."""
  total = 0
  for key in OBJ_KEYS:
    t = end_points[key]
    total = total + (t * objective_weight(key, tuple(t.shape)).to(device=t.device, dtype=t.dtype)).sum()
  return total


def _conv(x, w, b=None):
  """1x1 convolution of x [B, Cin, ...] with w [Cout, Cin, 1(, 1)]."""
  w2 = w.reshape(w.shape[0], w.shape[1]).to(x.dtype)
  y = torch.einsum("oc,bc...->bo...", w2, x)
  if b is not None:
    y = y + b.to(x.dtype).reshape([1, -1] + [1] * (x.dim() - 2))
  return y


def _bn(x, params, prefix, training, stats):
  """BatchNorm over every dimension but the channels (dimension 1).  training: batch statistics, and stats[prefix] =
  (batch mean, unbiased batch variance) -- what the running estimates are moved towards."""
  shape = [1, -1] + [1] * (x.dim() - 2)
  if training:
    dims = [0] + list(range(2, x.dim()))
    mean, var = x.mean(dims), x.var(dims, unbiased=False)
    n = x.numel() // x.shape[1]
    if stats is not None:
      stats[prefix] = (mean.detach(), var.detach() * n / max(n - 1, 1))
  else:
    mean, var = params[prefix + ".running_mean"].to(x.dtype), params[prefix + ".running_var"].to(x.dtype)
  g, b = params[prefix + ".weight"].to(x.dtype), params[prefix + ".bias"].to(x.dtype)
  return (x - mean.reshape(shape)) / torch.sqrt(var.reshape(shape) + BN_EPS) * g.reshape(shape) + b.reshape(shape)


def _relu(y, name, decisions, margins):
  """ReLU -- or, with the pattern decisions[name] (bool, y's shape), y times the pattern; margins[name] = (the largest
  |y| whose sign disagrees with the pattern, the largest |y|)."""
  if decisions is None or name not in decisions:
    return torch.relu(y)
  mask = decisions[name].to(y.device)
  assert mask.shape == y.shape, name
  if margins is not None:
    wrong = mask != (y.detach() > 0)
    margins[name] = (float(y.detach().abs()[wrong].max()) if bool(wrong.any()) else 0.0, float(y.detach().abs().max()))
  return y * mask.to(y.dtype)


def voting(params, seed_xyz, seed_features, vote_factor, training=True, stats=None, decisions=None, margins=None):
  """seed_xyz [B, S, 3], seed_features [B, C, S] -> (vote_xyz [B, S vf, 3], normalised vote_features [B, C, S vf])."""
  B, C, S = seed_features.shape
  net = _relu(_bn(_conv(seed_features, params["vgen.conv1.weight"], params["vgen.conv1.bias"]), params, "vgen.bn1", training, stats),
              "vgen.bn1", decisions, margins)
  net = _relu(_bn(_conv(net, params["vgen.conv2.weight"], params["vgen.conv2.bias"]), params, "vgen.bn2", training, stats),
              "vgen.bn2", decisions, margins)
  net = _conv(net, params["vgen.conv3.weight"], params["vgen.conv3.bias"])
  net = net.transpose(2, 1).reshape(B, S, vote_factor, 3 + C)
  vote_xyz = (seed_xyz.unsqueeze(2) + net[..., 0:3]).reshape(B, S * vote_factor, 3)
  feats = (seed_features.transpose(2, 1).unsqueeze(2) + net[..., 3:]).reshape(B, S * vote_factor, C).transpose(2, 1)
  feats = feats / torch.norm(feats, p=2, dim=1, keepdim=True)
  return vote_xyz, feats


def _gather_points(x, inds):
  """x [B, N, D] at inds [B, ...] -> [B, ..., D]."""
  B = x.shape[0]
  flat = inds.reshape(B, -1).long()
  out = torch.gather(x, 1, flat.unsqueeze(-1).expand(B, flat.shape[1], x.shape[2]))
  return out.reshape(tuple(inds.shape) + (x.shape[2],))


def proposal(params, vote_xyz, vote_features, sample_inds, idx, num_heading_bin, num_size_cluster, num_class, mean_size_arr,
             radius=0.3, training=True, stats=None, decisions=None, margins=None):
  """The proposal module on the votes, given the sampled votes sample_inds [B, P] and their neighbourhoods idx [B, P, ns]."""
  B, C, K = vote_features.shape
  end_points = {}
  new_xyz = _gather_points(vote_xyz, sample_inds)  # [B, P, 3]
  grouped_xyz = (_gather_points(vote_xyz, idx) - new_xyz.unsqueeze(2)) / radius  # [B, P, ns, 3]
  grouped_feat = _gather_points(vote_features.transpose(1, 2), idx)  # [B, P, ns, C]
  x = torch.cat([grouped_xyz, grouped_feat], -1).permute(0, 3, 1, 2)  # [B, 3 + C, P, ns]
  for i in range(len(SA_MLP)):
    p = "pnet.vote_aggregation.mlp_module.layer%d" % i
    x = _relu(_bn(_conv(x, params[p + ".conv.weight"]), params, p + ".bn.bn", training, stats), p + ".bn.bn", decisions, margins)
  if decisions is not None and "pool" in decisions:  # arg-max rows [B, 128, P] as data
    own = x.detach().max(dim=3)[0]
    x = torch.gather(x, 3, decisions["pool"].to(x.device).long().unsqueeze(-1)).squeeze(-1)
    if margins is not None:
      margins["pool"] = (float((own - x.detach()).abs().max()), float(own.abs().max()))
  else:
    x = x.max(dim=3)[0]  # [B, 128, P]
  end_points["aggregated_vote_xyz"] = new_xyz
  end_points["aggregated_vote_inds"] = sample_inds
  net = _relu(_bn(_conv(x, params["pnet.conv1.weight"], params["pnet.conv1.bias"]), params, "pnet.bn1", training, stats),
              "pnet.bn1", decisions, margins)
  net = _relu(_bn(_conv(net, params["pnet.conv2.weight"], params["pnet.conv2.bias"]), params, "pnet.bn2", training, stats),
              "pnet.bn2", decisions, margins)
  net = _conv(net, params["pnet.conv3.weight"], params["pnet.conv3.bias"]).transpose(2, 1)  # [B, P, nout]
  H, S = num_heading_bin, num_size_cluster
  P = net.shape[1]
  end_points["objectness_scores"] = net[:, :, 0:2]
  end_points["center"] = new_xyz + net[:, :, 2:5]
  end_points["heading_scores"] = net[:, :, 5:5 + H]
  end_points["heading_residuals_normalized"] = net[:, :, 5 + H:5 + 2 * H]
  end_points["heading_residuals"] = end_points["heading_residuals_normalized"] * (np.pi / H)
  end_points["size_scores"] = net[:, :, 5 + 2 * H:5 + 2 * H + S]
  end_points["size_residuals_normalized"] = net[:, :, 5 + 2 * H + S:5 + 2 * H + 4 * S].reshape(B, P, S, 3)
  msa = torch.as_tensor(np.asarray(mean_size_arr, np.float32)).to(device=net.device, dtype=net.dtype)
  end_points["size_residuals"] = end_points["size_residuals_normalized"] * msa.reshape(1, 1, S, 3)
  end_points["sem_cls_scores"] = net[:, :, 5 + 2 * H + 4 * S:]
  return end_points


def forward(params, seed_xyz, seed_features, sample_inds, idx, vote_factor, num_heading_bin, num_size_cluster, num_class,
            mean_size_arr, radius=0.3, training=True, stats=None, decisions=None, margins=None):
  """The whole head: end_points with seed_xyz, seed_features, vote_xyz, vote_features and the proposal module's keys."""
  vote_xyz, vote_features = voting(params, seed_xyz, seed_features, vote_factor, training, stats, decisions, margins)
  end_points = proposal(params, vote_xyz, vote_features, sample_inds, idx, num_heading_bin, num_size_cluster, num_class,
                        mean_size_arr, radius, training, stats, decisions, margins)
  end_points.update(seed_xyz=seed_xyz, seed_features=seed_features, vote_xyz=vote_xyz, vote_features=vote_features)
  return end_points


# Exactly zero in exact arithmetic: the bias of a convolution that feeds a training-mode BatchNorm (the normalisation removes
# any per-channel constant).  "Relative to the tensor's largest entry" has no meaning for such a gradient; it is the plain sum
# over the rows of the same per-row gradients whose products with the inputs form the layer's weight gradient, so its rounding
# error is measured against the weight gradient's largest entry instead.
ZERO_GRADIENT = ("vgen.conv1.bias", "vgen.conv2.bias", "pnet.conv1.bias", "pnet.conv2.bias")


def gradient_error(name, got, want, want_of):
  """max |got - want| over max |want| -- or, for a ZERO_GRADIENT bias, over max |want_of(<its layer's weight>)|."""
  got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
  if name in ZERO_GRADIENT:
    want = torch.as_tensor(want_of(name[:-len("bias")] + "weight")).detach().double().cpu()
    return float(got.abs().max() / want.abs().max())
  return float((got - want).abs().max() / max(float(want.abs().max()), 1e-30))


def as_double(params, requires_grad=False):
  out = {}
  for k, v in params.items():
    if v.is_floating_point():
      v = v.detach().double().cpu().clone()
      if requires_grad and not k.endswith(("running_mean", "running_var")):
        v.requires_grad_(True)
    out[k] = v
  return out


# ---- the schedules of lib/train.py, restated (tests/test_votenet_model_ref.py types the expected values in) ----------------
def current_lr(epoch, base=1e-3, steps=(80, 120, 160), rates=(0.1, 0.1, 0.1)):
  lr = base
  for s, r in zip(steps, rates):
    if epoch >= s:
      lr *= r
  return lr


def bn_momentum(epoch, init=0.5, rate=0.5, step=20, floor=0.001):
  return max(init * rate ** (epoch // step), floor)
