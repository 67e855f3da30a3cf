"""Generates tests/golden/golden_pointnet2_backbone.npz by running the REFERENCE'S OWN PointNet++ backbone on the CPU.

Run from the repo root where the reference tree is present:
    python tests/golden/make_golden_pointnet2_backbone.py

What runs, imported unmodified from downstream/votenet_det_new/models of the reference: backbone_module.py
(Pointnet2Backbone.forward) and through it backbone/pointnet2/pointnet2_modules.py (PointnetSAModuleVotes, PointnetFPModule) and
pytorch_utils.py (SharedMLP).  Their `pointnet2_utils` (a compiled extension in the reference) is served by the stand-in of
make_golden_votenet_model.py, extended here with three_nn / three_interpolate over tests/pointset_ref.py and registered under
both names the reference imports it by; an empty `MinkowskiEngine` module satisfies backbone_module.py's import (only the sparse
backbone uses it).  The backbone's six sub-modules are replaced by reference modules of small size (CASE), so that the run
takes seconds; Pointnet2Backbone.forward is the reference's.  torch.Tensor.cuda is the identity for the duration of the run.

The file holds arrays only: the input, the indices the stand-in produced, every end_points tensor, the gradients of the input
and of every parameter under the fixed cosine objective of tests/pointnet2_backbone_ref.py, the running estimates after the
forward, and the state dict's names and shapes as a list.  Parameters come from the seeded, name-keyed fill and are not stored.
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_golden_votenet_model as head  # noqa: E402
import pointnet2_backbone_ref as R  # noqa: E402
import pointset_ref as P  # noqa: E402

REF_ROOT = "/root/reference/downstream/votenet_det_new"
PATH = os.path.join(HERE, "golden_pointnet2_backbone.npz")

# B scenes of N points in a 1.5 m cube with one extra feature column; many balls of the first levels hold only their centre,
# so ball-query padding (repeated rows) and pooling ties occur
CASE = dict(B=2, N=256, F=1, extent=1.5, npoints=(64, 32, 16, 8), nsamples=(8, 8, 4, 4), radii=(0.2, 0.4, 0.8, 1.2),
            sa_mlps=((1, 32, 32, 64), (64, 32, 32, 64), (64, 32, 32, 64), (64, 32, 32, 64)), fp_mlps=((128, 64, 64), (128, 64, 64)),
            param_seed=11, input_seed=20261019)


def case_config(case=CASE):
  return {k: case[k] for k in ("F", "npoints", "nsamples", "radii", "sa_mlps", "fp_mlps")}


def reference_available():
  return os.path.isfile(os.path.join(REF_ROOT, "models", "backbone_module.py"))


def make_standin(record):
  """make_golden_votenet_model's stand-in plus the feature propagation's two ops; record collects, in call order, "fps",
  "ball" and "nn": the furthest-point picks, the ball-query and the three-nearest-neighbour results."""
  m = head.make_standin({})
  fps, ball = m.furthest_point_sample, m.ball_query

  def furthest_point_sample(xyz, npoint):
    out = fps(xyz, npoint)
    record.setdefault("fps", []).append(out.clone())
    return out

  def ball_query(radius, nsample, xyz, new_xyz):
    out = ball(radius, nsample, xyz, new_xyz)
    record.setdefault("ball", []).append(out.clone())
    return out

  def three_nn(unknown, known):
    d2, idx = P.three_nn(unknown.detach().cpu().numpy(), known.detach().cpu().numpy())
    record.setdefault("nn", []).append(torch.from_numpy(idx).clone())
    return torch.sqrt(torch.from_numpy(d2)), torch.from_numpy(idx)

  class QueryAndGroup(m.QueryAndGroup):
    """The stand-in's grouper over the recording ball query; features may be None (a cloud of coordinates only)."""

    def forward(self, xyz, new_xyz, features=None):
      idx = ball_query(self.radius, self.nsample, xyz, new_xyz)
      rel = P.group(xyz.transpose(1, 2).contiguous(), idx) - new_xyz.transpose(1, 2).unsqueeze(-1)
      if self.normalize_xyz:
        rel = rel / self.radius
      out = rel if features is None else torch.cat([rel, P.group(features, idx)], dim=1)
      return (out, rel) if self.ret_grouped_xyz else out

  m.furthest_point_sample, m.ball_query, m.QueryAndGroup = furthest_point_sample, ball_query, QueryAndGroup
  m.three_nn, m.three_interpolate = three_nn, P.interpolate
  return m


def import_reference(record):
  """backbone_module of the reference, bound to the stand-in."""
  assert reference_available(), "%s is not present" % REF_ROOT
  names = ("pointnet2_utils", "pytorch_utils", "MinkowskiEngine", "models", "models.backbone", "models.backbone.pointnet2",
           "models.backbone.pointnet2.pointnet2_utils", "models.backbone.pointnet2.pointnet2_modules", "models.backbone_module")
  saved = {k: sys.modules.get(k) for k in names}
  path = list(sys.path)
  for k in names:
    sys.modules.pop(k, None)
  standin = make_standin(record)
  sys.modules["pointnet2_utils"] = standin
  sys.modules["models.backbone.pointnet2.pointnet2_utils"] = standin
  sys.modules["MinkowskiEngine"] = types.ModuleType("MinkowskiEngine")
  sys.path.insert(0, REF_ROOT)
  try:
    import models.backbone_module as bm
    import models.backbone.pointnet2.pointnet2_modules as pm
    return bm, pm
  finally:
    sys.path[:] = path
    for k, v in saved.items():
      if v is None:
        sys.modules.pop(k, None)
      else:
        sys.modules[k] = v


def make_inputs(case=CASE):
  rng = np.random.RandomState(case["input_seed"])
  pc = rng.uniform(0.0, case["extent"], (case["B"], case["N"], 3 + case["F"])).astype(np.float32)
  pc[..., 3:] = rng.normal(0, 1, (case["B"], case["N"], case["F"])).astype(np.float32)
  return dict(point_clouds=pc)


def run_reference(inp, case=CASE):
  record = {}
  bm, pm = import_reference(record)
  cfg = case_config(case)
  params = R.make_params(cfg, case["param_seed"])
  net = bm.Pointnet2Backbone(input_feature_dim=case["F"])
  for k in range(4):
    setattr(net, "sa%d" % (k + 1), pm.PointnetSAModuleVotes(npoint=case["npoints"][k], radius=case["radii"][k], nsample=case["nsamples"][k],
                                                           mlp=list(case["sa_mlps"][k]), use_xyz=True, normalize_xyz=True))
  for k in range(2):
    setattr(net, "fp%d" % (k + 1), pm.PointnetFPModule(mlp=list(case["fp_mlps"][k])))
  shapes = [(k, list(v.shape)) for k, v in net.state_dict().items()]
  assert sorted(n for n, _ in shapes) == sorted(params), "the fill does not cover the reference's state dict"
  net.load_state_dict(params)
  net.train()
  pc = torch.from_numpy(inp["point_clouds"]).requires_grad_(True)
  cuda = torch.Tensor.cuda
  torch.Tensor.cuda = lambda self, *a, **k: self
  try:
    end_points = net(pc)
  finally:
    torch.Tensor.cuda = cuda
  R.objective(end_points).backward()
  out = {"ep_" + k: v.detach().numpy() for k, v in end_points.items()}
  assert len(record["fps"]) == 4 and len(record["ball"]) == 4 and len(record["nn"]) == 2
  for k in range(4):
    out["sa%d_inds" % (k + 1)] = record["fps"][k].numpy()
    out["sa%d_idx" % (k + 1)] = record["ball"][k].numpy()
  for k in range(2):
    out["fp%d_idx" % (k + 1)] = record["nn"][k].numpy()
  out["grad_point_clouds"] = pc.grad.numpy()
  for k, p in net.named_parameters():
    out["pgrad_" + k] = p.grad.numpy()
  for k, b in net.named_buffers():
    if k.endswith(("running_mean", "running_var")):
      out["buf_" + k] = b.detach().numpy()
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
