"""Generates tests/golden/golden_votenet_model.npz by running the REFERENCE'S OWN VoteNet head modules on the CPU.

Run from the repo root where the reference tree is present:
    python tests/golden/make_golden_votenet_model.py

What runs, imported unmodified from downstream/votenet_det_new/models of the reference: voting_module.py (VotingModule) and
proposal_module.py (ProposalModule, decode_scores), and through them backbone/pointnet2/pointnet2_modules.py
(PointnetSAModuleVotes) and pytorch_utils.py (SharedMLP).  Their `pointnet2_utils` (a compiled extension in the reference) is
served by a stand-in built on tests/pointset_ref.py: furthest point sampling and ball query in numpy float32, the gathers
as torch.gather, and QueryAndGroup restated over them.  torch.Tensor.cuda is the identity for the duration of the run.
Between the two modules the two lines of models/votenet.py:120-121 (the L2 normalisation of the vote features) are applied.

The file holds arrays only: the inputs, the indices the stand-in produced, every end_points tensor, and the gradients of
the inputs and of every parameter under the fixed scalar objective of tests/votenet_model_ref.py.  Parameters come from
that file's seeded, name-keyed fill and are not stored; the state dict's names and shapes are, as a list.
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pointset_ref as P  # noqa: E402
import votenet_model_ref as M  # noqa: E402

REF_MODELS = "/root/reference/downstream/votenet_det_new/models"
REF_POINTNET2 = os.path.join(REF_MODELS, "backbone", "pointnet2")
PATH = os.path.join(HERE, "golden_votenet_model.npz")

# B scenes, S seeds, P proposals, C seed features; the SUN RGB-D style head (79 outputs)
CASE = dict(B=2, S=40, P=8, C=32, vote_factor=2, num_heading_bin=12, num_size_cluster=10, num_class=10, sampling="vote_fps",
            param_seed=7, input_seed=20261019)


def reference_available():
  return os.path.isfile(os.path.join(REF_MODELS, "proposal_module.py"))


def make_standin(record):
  """A `pointnet2_utils` module over tests/pointset_ref.py; record["idx"] receives the ball-query result."""
  m = types.ModuleType("pointnet2_utils")

  def furthest_point_sample(xyz, npoint):
    pts = xyz.detach().cpu().numpy()
    return torch.from_numpy(np.stack([P.fps(pts[b], int(npoint)) for b in range(pts.shape[0])]).astype(np.int32))

  def ball_query(radius, nsample, xyz, new_xyz):
    idx = torch.from_numpy(P.ball_query(xyz.detach().cpu().numpy(), new_xyz.detach().cpu().numpy(), radius, nsample))
    record["idx"] = idx.clone()
    return idx

  class QueryAndGroup(torch.nn.Module):
    """Neighbourhoods of new_xyz in xyz as [B, 3 + C, npoint, nsample]: centred (and radius-normalised) coordinates, then
    the gathered features."""

    def __init__(self, radius, nsample, use_xyz=True, ret_grouped_xyz=False, normalize_xyz=False, sample_uniformly=False,
                 ret_unique_cnt=False):
      super().__init__()
      assert use_xyz and not sample_uniformly and not ret_unique_cnt, "the stand-in covers what the proposal module uses"
      self.radius, self.nsample, self.normalize_xyz, self.ret_grouped_xyz = radius, nsample, normalize_xyz, ret_grouped_xyz

    def forward(self, xyz, new_xyz, features=None):
      idx = ball_query(self.radius, self.nsample, xyz, new_xyz)
      rel = P.group(xyz.transpose(1, 2).contiguous(), idx) - new_xyz.transpose(1, 2).unsqueeze(-1)
      if self.normalize_xyz:
        rel = rel / self.radius
      out = torch.cat([rel, P.group(features, idx)], dim=1)
      return (out, rel) if self.ret_grouped_xyz else out

  class GroupAll(torch.nn.Module):

    def __init__(self, *a, **k):
      raise NotImplementedError("GroupAll is not part of the stand-in")

  m.furthest_point_sample, m.ball_query = furthest_point_sample, ball_query
  m.gather_operation, m.grouping_operation = P.gather, P.group
  m.QueryAndGroup, m.GroupAll = QueryAndGroup, GroupAll
  return m


def import_reference(record):
  """(voting_module, proposal_module) of the reference, bound to the stand-in."""
  assert reference_available(), "%s is not present" % REF_MODELS
  names = ("pointnet2_utils", "pointnet2_modules", "pytorch_utils", "voting_module", "proposal_module")
  saved = {k: sys.modules.get(k) for k in names}
  path = list(sys.path)
  for k in names:
    sys.modules.pop(k, None)
  sys.modules["pointnet2_utils"] = make_standin(record)
  sys.path[:0] = [REF_MODELS, REF_POINTNET2]
  try:
    import voting_module as vm
    import proposal_module as pm
    return vm, pm
  finally:
    sys.path[:] = path
    for k, v in saved.items():
      if v is None:
        sys.modules.pop(k, None)
      else:
        sys.modules[k] = v


def make_inputs(case=CASE):
  rng = np.random.RandomState(case["input_seed"])
  B, S, C = case["B"], case["S"], case["C"]
  return dict(seed_xyz=rng.uniform(-0.5, 0.5, (B, S, 3)).astype(np.float32),
              seed_features=rng.normal(0, 1, (B, C, S)).astype(np.float32),
              mean_size_arr=rng.uniform(0.4, 1.5, (case["num_size_cluster"], 3)).astype(np.float32))


def run_reference(inp, case=CASE):
  record = {}
  vm, pm = import_reference(record)
  nout = M.num_outputs(case["num_heading_bin"], case["num_size_cluster"], case["num_class"])
  params = M.make_params(case["C"], case["vote_factor"], nout, case["param_seed"])
  vgen = vm.VotingModule(case["vote_factor"], case["C"])
  pnet = pm.ProposalModule(case["num_class"], case["num_heading_bin"], case["num_size_cluster"], inp["mean_size_arr"], case["P"],
                           case["sampling"], seed_feat_dim=case["C"])
  shapes = [("vgen." + k, list(v.shape)) for k, v in vgen.state_dict().items()] + \
           [("pnet." + k, list(v.shape)) for k, v in pnet.state_dict().items()]
  assert sorted(n for n, _ in shapes) == sorted(params), "the fill does not cover the reference's state dict"
  vgen.load_state_dict({k[5:]: v for k, v in params.items() if k.startswith("vgen.")})
  pnet.load_state_dict({k[5:]: v for k, v in params.items() if k.startswith("pnet.")})
  vgen.train()
  pnet.train()
  seed_xyz = torch.from_numpy(inp["seed_xyz"]).requires_grad_(True)
  seed_features = torch.from_numpy(inp["seed_features"]).requires_grad_(True)
  cuda = torch.Tensor.cuda
  torch.Tensor.cuda = lambda self, *a, **k: self
  try:
    end_points = {"seed_xyz": seed_xyz, "seed_features": seed_features}
    xyz, features = vgen(seed_xyz, seed_features)
    features_norm = torch.norm(features, p=2, dim=1)
    features = features.div(features_norm.unsqueeze(1))
    end_points["vote_xyz"], end_points["vote_features"] = xyz, features
    end_points = pnet(xyz, features, end_points)
  finally:
    torch.Tensor.cuda = cuda
  M.objective(end_points).backward()
  out = {"ep_" + k: v.detach().numpy() for k, v in end_points.items() if k not in ("seed_xyz", "seed_features")}
  out["idx"] = record["idx"].numpy()
  out["grad_seed_xyz"], out["grad_seed_features"] = seed_xyz.grad.numpy(), seed_features.grad.numpy()
  for prefix, mod in (("vgen.", vgen), ("pnet.", pnet)):
    for k, p in mod.named_parameters():
      out["pgrad_" + prefix + k] = p.grad.numpy()
    for k, b in mod.named_buffers():
      if k.endswith(("running_mean", "running_var")):
        out["buf_" + prefix + k] = b.detach().numpy()
  out["state_shapes"] = np.array(json.dumps(shapes))
  out["case"] = np.array(json.dumps(case))
  return out


def generate():
  inp = make_inputs()
  out = run_reference(inp)
  out.update(inp)
  return out


def main():
  out = generate()
  np.savez_compressed(PATH, **out)
  print(PATH, os.path.getsize(PATH), sorted(out))


if __name__ == "__main__":
  main()
