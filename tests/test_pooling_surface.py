"""CPU checks of the pooling / global pooling / instance-norm surface: the modules build from the reference's factories,
a model that uses them refuses to lower to the native engine, and the fp64 references of tests/pool_ref.py agree with
dense torch."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pool_ref as R  # noqa: E402
from helpers import random_coords, to_dense  # noqa: E402


def test_factories_build_modules(built_lib):
  import pointcontrast_amd.minkowski as ME
  from pointcontrast_amd.model.modules.common import NormType, avg_pool, avg_unpool, get_norm, sum_pool
  assert isinstance(sum_pool(2, 2, D=3), ME.MinkowskiSumPooling)
  assert isinstance(avg_pool(3, 1, D=3), ME.MinkowskiAvgPooling)
  assert isinstance(avg_unpool(2, 2, D=3), ME.MinkowskiAvgUnpooling)
  norm = get_norm(NormType.SPARSE_INSTANCE_NORM, 96, D=3)
  assert isinstance(norm, ME.MinkowskiInstanceNorm)
  sd = norm.state_dict()
  assert sorted(sd) == ["bias", "weight"] and sd["weight"].shape == (1, 96) and sd["bias"].shape == (1, 96)
  assert ME.MinkowskiGlobalPooling(average=False).average is False
  assert isinstance(ME.MinkowskiPoolingTranspose(kernel_size=2, stride=2, dimension=3), ME.MinkowskiPoolingTranspose)
  ME.MinkowskiBroadcastAddition(dimension=3), ME.MinkowskiBroadcastMultiplication(dimension=3)


@pytest.mark.parametrize("make, what", [
    (lambda ME: ME.MinkowskiSumPooling(kernel_size=8, stride=4, dimension=3), "kernel_size=8, stride=4"),
    (lambda ME: ME.MinkowskiAvgPooling(kernel_size=3, stride=2, dimension=3), "kernel_size=3, stride=2"),
    (lambda ME: ME.MinkowskiSumPooling(kernel_size=3, stride=1, dilation=2, dimension=3), "dilation 2"),
    (lambda ME: ME.MinkowskiPoolingTranspose(kernel_size=3, stride=1, dimension=3), "kernel_size=3, stride=1"),
    (lambda ME: ME.MinkowskiMaxPooling(kernel_size=2, stride=2, dimension=3), "MinkowskiMaxPooling"),
])
def test_unsupported_pooling_raises_precisely(built_lib, make, what):
  import pointcontrast_amd.minkowski as ME
  with pytest.raises(NotImplementedError, match=what):
    make(ME)


def test_instance_norm_model_refuses_to_lower(built_lib):
  from pointcontrast_amd.engine import lower_model
  from pointcontrast_amd.lib.config import get_config
  from pointcontrast_amd.lib.distributed import FlatParameters
  from pointcontrast_amd.model.modules.resnet_block import BasicBlockIN
  from pointcontrast_amd.model.res16unet import Res16UNet14

  class Res16UNet14IN(Res16UNet14):
    BLOCK = BasicBlockIN

  model = Res16UNet14IN(3, 32, get_config([]), D=3)
  assert "block1.0.norm1.weight" in dict(model.named_parameters())
  with pytest.raises(NotImplementedError, match="MinkowskiInstanceNorm"):
    lower_model(model, FlatParameters(model.parameters()))


def _grid(coords):
  lo = coords[:, 1:].min(0)
  lo = lo - (lo % 2)  # even origin: the stride-2 cells of the grid are the sparse ones
  shape = tuple(int(v) for v in coords[:, 1:].max(0) - lo + 2)
  return lo, shape


def _dense_at(dense, coords, lo, step=1):
  c = torch.from_numpy(coords.astype(np.int64))
  return dense[c[:, 0], :, (c[:, 1] - lo[0]) // step, (c[:, 2] - lo[1]) // step, (c[:, 3] - lo[2]) // step]


@pytest.mark.parametrize("region", [0, 3])
def test_pool_ref_k3s1_matches_dense(region):
  from oracle.sparse_ref import CoordsManagerRef
  coords = random_coords(300, extent=8, batch=2, seed=1)
  x = torch.randn(len(coords), 5, dtype=torch.float64)
  cm = CoordsManagerRef(coords)
  nbr = cm.kernel_map(0, 0, 3, region).nbr
  lo, shape = _grid(coords)
  dx = to_dense(coords, x, lo, shape)
  dm = to_dense(coords, torch.ones(len(coords), 1, dtype=torch.float64), lo, shape)
  box = lambda d: F.conv3d(d, torch.ones(d.shape[1], 1, 3, 3, 3, dtype=d.dtype), padding=1, groups=d.shape[1])
  want_sum = _dense_at(box(dx), coords, lo)
  want_avg = want_sum / _dense_at(box(dm), coords, lo)
  assert R.rel_err(R.pool(x, nbr, False), want_sum) < 1e-12
  assert R.rel_err(R.pool(x, nbr, True), want_avg) < 1e-12


def test_pool_ref_k2s2_and_unpool_match_dense():
  from oracle.sparse_ref import CoordsManagerRef
  coords = random_coords(300, extent=10, batch=2, seed=2)
  x = torch.randn(len(coords), 4, dtype=torch.float64)
  cm = CoordsManagerRef(coords)
  k1 = cm.stride(0, 2)
  coarse = cm.coords[k1]
  nbr = cm.kernel_map(0, k1, 2).nbr
  lo, shape = _grid(coords)
  dx = to_dense(coords, x, lo, shape)
  dm = to_dense(coords, torch.ones(len(coords), 1, dtype=torch.float64), lo, shape)
  want_sum = _dense_at(F.avg_pool3d(dx, 2, 2) * 8, coarse, lo, 2)
  want_avg = want_sum / _dense_at(F.avg_pool3d(dm, 2, 2) * 8, coarse, lo, 2)
  assert R.rel_err(R.pool(x, nbr, False), want_sum) < 1e-12
  assert R.rel_err(R.pool(x, nbr, True), want_avg) < 1e-12
  # unpooling: a transposed conv with identity 2^3 weights puts every coarse value on its 8 children
  g = torch.randn(len(coarse), 4, dtype=torch.float64)
  cshape = tuple(s // 2 for s in shape)
  dg = torch.zeros((2, 4) + cshape, dtype=torch.float64)
  cc = torch.from_numpy(coarse.astype(np.int64))
  dg[cc[:, 0], :, (cc[:, 1] - lo[0]) // 2, (cc[:, 2] - lo[1]) // 2, (cc[:, 3] - lo[2]) // 2] = g
  up = F.conv_transpose3d(dg, torch.ones(4, 1, 2, 2, 2, dtype=torch.float64), stride=2, groups=4)
  assert R.rel_err(R.unpool(g, nbr, len(coords)), _dense_at(up, coords, lo)) < 1e-12


def test_global_pool_and_instance_norm_refs_match_torch():
  rng = np.random.RandomState(3)
  b = rng.choice([0, 3, 7], size=200)
  x = torch.from_numpy(rng.randn(200, 6) * 2 + 1e3)
  w, bias = torch.randn(1, 6, dtype=torch.float64), torch.randn(1, 6, dtype=torch.float64)
  uniq = [0, 3, 7]
  gp = R.global_pool(x, b, True)
  y = R.instance_norm(x, b, w, bias)
  for i, bi in enumerate(uniq):
    rows = torch.from_numpy(np.nonzero(b == bi)[0])
    xb = x[rows]
    assert torch.allclose(gp[i], xb.mean(0), rtol=1e-13)
    want = F.instance_norm(xb.t()[None], weight=w.reshape(-1), bias=bias.reshape(-1), eps=1e-5)[0].t()
    assert R.rel_err(y[rows], want) < 1e-9
  assert torch.allclose(R.global_pool(x, b, False).sum(0), x.sum(0))


def test_pooling_ops_refuse_cpu_tensors(built_lib):
  from pointcontrast_amd import functional as PF
  from pointcontrast_amd._lib import KMap, PcmiError, Segments
  with pytest.raises(PcmiError, match="no CPU path"):
    PF.PoolFunction.apply(torch.zeros(4, 4), KMap(), False)
  with pytest.raises(PcmiError, match="no CPU path"):
    PF.InstanceNormFunction.apply(torch.zeros(4, 4), torch.ones(1, 4), torch.zeros(1, 4), Segments(), 1e-5, None, False)
