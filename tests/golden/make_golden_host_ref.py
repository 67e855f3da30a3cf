"""Regenerates tests/golden/golden_host_ref.json: what two small torch-only files of the reference produce.

Run from the repo root where the reference checkout is available:
  python tests/golden/make_golden_host_ref.py <reference checkout>

What runs, unmodified:
  * pretrain/pointcontrast/lib/data_sampler.py: InfSampler / DistributedInfSampler index streams, with another
    consumer of the global torch RNG between two indices (tests/test_host_logic.py::sampler_stream);
  * downstream/semseg/lib/solvers.py: PolyLR learning rates of five SGD steps (max_iter 100, power 0.9).
The tests compare this package's restatements with these vectors; they need no reference checkout."""
import importlib.util
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from test_host_logic import SAMPLER_CASES, poly_lrs, sampler_stream  # noqa: E402


def _load(path, name):
  spec = importlib.util.spec_from_file_location(name, path)
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def generate(ref_root):
  sampler = _load(os.path.join(ref_root, "pretrain", "pointcontrast", "lib", "data_sampler.py"), "ref_sampler")
  solvers = _load(os.path.join(ref_root, "downstream", "semseg", "lib", "solvers.py"), "ref_semseg_solvers")
  out = {"sampler": {}, "poly_lr": poly_lrs(solvers.PolyLR, torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))], lr=0.1, momentum=0.9))}
  for key, make in SAMPLER_CASES.items():
    out["sampler"][key] = {"stream": sampler_stream(sampler, make), "len": len(make(sampler))}
  return out


if __name__ == "__main__":
  with open(os.path.join(HERE, "golden_host_ref.json"), "w") as f:
    json.dump(generate(sys.argv[1]), f, indent=0)
    f.write("\n")
  print("wrote", os.path.join(HERE, "golden_host_ref.json"))
