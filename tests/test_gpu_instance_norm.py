"""MinkowskiInstanceNorm on the MI355X against the fp64 reference of tests/pool_ref.py: forward, dx, dresidual, dweight,
dbias, with the fused residual / ReLU epilogue, one-row instances and large-mean features."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pool_ref as R  # noqa: E402
from helpers import random_coords  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-4


def _coords(sizes, seed):
  rng = np.random.RandomState(seed)
  rows = []
  for b, n in sizes.items():
    c = random_coords(n, extent=14, batch=1, seed=int(rng.randint(1 << 30)))
    c[:, 0] = b
    rows.append(c)
  c = np.concatenate(rows)
  return c[rng.permutation(len(c))]


def _run(coords, x, C, residual=False, relu=False, train=True, seed=0):
  import pointcontrast_amd.minkowski as ME
  gen = torch.Generator().manual_seed(seed)
  norm = ME.MinkowskiInstanceNorm(C, D=3)
  with torch.no_grad():
    norm.weight.copy_(torch.rand(1, C, generator=gen) + 0.5)
    norm.bias.copy_(torch.rand(1, C, generator=gen) - 0.5)
  norm = norm.to(DEV).train(train)
  f = x.to(DEV, torch.float32).requires_grad_(True)
  st = ME.SparseTensor(f, coords=torch.from_numpy(coords).to(DEV))
  res64 = torch.randn(x.shape, dtype=torch.float64, generator=gen) if residual else None
  rf = res64.to(DEV, torch.float32).requires_grad_(True) if residual else None
  rs = ME.SparseTensor(rf, coords_key=st.coords_key, coords_manager=st.coords_man) if residual else None
  y = norm(st, residual=rs, relu=relu)
  dy = torch.randn(x.shape, dtype=torch.float64, generator=gen)
  y.F.backward(dy.to(DEV, torch.float32))

  x64 = x.double().clone().requires_grad_(True)
  w64 = norm.weight.detach().double().cpu().requires_grad_(True)
  b64 = norm.bias.detach().double().cpu().requires_grad_(True)
  r64 = res64.clone().requires_grad_(True) if residual else None
  want = R.instance_norm(x64, coords[:, 0], w64, b64, 1e-5, r64, relu)
  want.backward(dy)
  got = dict(y=y.F.detach(), dx=f.grad, dw=norm.weight.grad, db=norm.bias.grad, dr=rf.grad if residual else None)
  ref = dict(y=want.detach(), dx=x64.grad, dw=w64.grad, db=b64.grad, dr=r64.grad if residual else None)
  return got, ref


def _check_all(got, ref, what):
  for k in got:
    if got[k] is None:
      continue
    assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
    e = R.rel_err(got[k], ref[k])
    assert e <= TOL, "%s %s: rel err %.3e" % (what, k, e)


@pytest.mark.parametrize("C", [13, 96])
@pytest.mark.parametrize("residual, relu", [(False, False), (False, True), (True, True)])
def test_instance_norm_matches_reference(C, residual, relu):
  coords = _coords({0: 400, 3: 250, 7: 90}, seed=C)
  x = torch.randn(len(coords), C, dtype=torch.float64, generator=torch.Generator().manual_seed(C)) * 2 + 0.5
  got, ref = _run(coords, x, C, residual, relu, seed=C)
  _check_all(got, ref, "C=%d residual=%s relu=%s" % (C, residual, relu))


def test_one_row_instance_gives_bias_and_finite_gradients():
  coords = _coords({0: 300, 4: 1, 9: 120}, seed=1)
  C = 32
  x = torch.randn(len(coords), C, dtype=torch.float64)
  got, ref = _run(coords, x, C, seed=1)
  _check_all(got, ref, "one-row instance")
  for k in ("dx", "dw", "db"):
    assert torch.isfinite(got[k]).all(), k


def test_one_row_instance_output_is_bias():
  import pointcontrast_amd.minkowski as ME
  coords = _coords({0: 50, 4: 1}, seed=2)
  C = 8
  norm = ME.MinkowskiInstanceNorm(C, D=3).to(DEV)
  with torch.no_grad():
    norm.bias.copy_(torch.linspace(-1, 1, C))
  st = ME.SparseTensor(torch.randn(len(coords), C, device=DEV), coords=torch.from_numpy(coords).to(DEV))
  y = norm(st)
  row = int(np.nonzero(coords[:, 0] == 4)[0][0])
  assert torch.equal(y.F[row].cpu(), torch.linspace(-1, 1, C))


def test_large_mean_features_use_a_centred_variance():
  coords = _coords({0: 500, 3: 300}, seed=3)
  C = 96
  x = torch.randn(len(coords), C, dtype=torch.float64, generator=torch.Generator().manual_seed(3)) + 1e3
  x = x.float().double()  # the values the device sees
  got, ref = _run(coords, x, C, relu=True, seed=3)
  _check_all(got, ref, "mean 1e3")


def test_eval_mode_equals_train_mode():
  coords = _coords({1: 200, 2: 150}, seed=4)
  x = torch.randn(len(coords), 32, dtype=torch.float64)
  got_t, _ = _run(coords, x, 32, residual=True, relu=True, train=True, seed=4)
  got_e, _ = _run(coords, x, 32, residual=True, relu=True, train=False, seed=4)
  for k in got_t:
    assert (got_t[k] is None and got_e[k] is None) or torch.equal(got_t[k], got_e[k]), k


def test_parameter_gradients_sum_over_instances():
  coords = _coords({0: 100, 1: 100, 2: 100, 3: 100, 5: 3}, seed=5)
  C = 16
  x = torch.randn(len(coords), C, dtype=torch.float64)
  got, ref = _run(coords, x, C, seed=5)
  _check_all(got, ref, "five instances")
  assert got["dw"].shape == (1, C) and got["db"].shape == (1, C)
