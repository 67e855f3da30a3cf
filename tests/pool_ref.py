"""fp64 CPU references of pooling, unpooling, global pooling, broadcast and instance norm (torch autograd on the
float64 inputs), for tests/test_pooling_surface.py (which pins them against dense torch) and the GPU tests.

Maps are oracle.sparse_ref kernel maps: nbr [K, n_out] = in-row feeding out-row j through offset k, or -1."""
import numpy as np
import torch


def pool(feats, nbr, average):
  """out[j] = sum_k in[nbr[k, j]]; average: divided by the number of present k (ME's nonzero average)."""
  idx = torch.from_numpy(np.asarray(nbr, dtype=np.int64))
  present = (idx >= 0).to(feats.dtype)
  g = feats[idx.clamp(min=0)] * present[..., None]  # [K, n_out, C]
  out = g.sum(0)
  if average:
    out = out / present.sum(0)[:, None]
  return out


def unpool(feats_coarse, nbr_fine_to_coarse, n_fine):
  """out[child] = in[parent]: nbr [8, n_coarse] of the fine -> coarse (k=2, s=2) map."""
  idx = torch.from_numpy(np.asarray(nbr_fine_to_coarse, dtype=np.int64))
  k, j = torch.nonzero(idx >= 0, as_tuple=True)
  fine = idx[k, j]
  return feats_coarse.new_zeros((n_fine, feats_coarse.shape[1])).index_add(0, fine, feats_coarse[j])


def instances(batch_idx):
  """(ascending distinct batch indices, instance of every row)."""
  b = np.asarray(batch_idx)
  uniq, inv = np.unique(b, return_inverse=True)
  return uniq, torch.from_numpy(inv.astype(np.int64))


def global_pool(feats, batch_idx, average):
  uniq, inv = instances(batch_idx)
  out = feats.new_zeros((len(uniq), feats.shape[1])).index_add(0, inv, feats)
  if average:
    cnt = torch.bincount(inv, minlength=len(uniq)).to(feats.dtype)
    out = out / cnt[:, None]
  return out


def broadcast(feats, g, batch_idx, op):
  _, inv = instances(batch_idx)
  return feats + g[inv] if op == "add" else feats * g[inv]


def instance_norm(x, batch_idx, weight, bias, eps=1e-5, residual=None, relu=False):
  """Per instance and channel: mean and biased variance (downstream/semseg/lib/layers.py:54-90); weight / bias [1, C]."""
  uniq, inv = instances(batch_idx)
  n = len(uniq)
  cnt = torch.bincount(inv, minlength=n).to(x.dtype)[:, None]
  mean = x.new_zeros((n, x.shape[1])).index_add(0, inv, x) / cnt
  d = x - mean[inv]
  var = x.new_zeros((n, x.shape[1])).index_add(0, inv, d * d) / cnt
  y = d / torch.sqrt(var[inv] + eps) * weight.reshape(1, -1) + bias.reshape(1, -1)
  if residual is not None:
    y = y + residual
  return torch.relu(y) if relu else y


def align_rows(got_coords, want_coords):
  """Permutation p with got_coords[p] == want_coords (both [n, 4] with unique rows)."""
  g, w = np.asarray(got_coords, dtype=np.int64), np.asarray(want_coords, dtype=np.int64)
  assert g.shape == w.shape, (g.shape, w.shape)
  kg = [tuple(r) for r in g]
  pos = {k: i for i, k in enumerate(kg)}
  p = np.array([pos[tuple(r)] for r in w], dtype=np.int64)
  assert (g[p] == w).all()
  return torch.from_numpy(p)


def rel_err(got, want):
  got, want = got.detach().double().cpu(), want.detach().double().cpu()
  return float((got - want).abs().max() / max(float(want.abs().max()), 1e-30))
