"""torch.autograd.Function wrappers over the libpcmi C ABI.

Every forward/backward below is one or a few calls into libpcmi.so on the
current torch stream; tensors are plain fp32 row-major [rows, channels].  There is
no torch-op fallback: a CPU tensor raises.
"""
import contextlib
import ctypes as C

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ._lib import lib, check, KMap
from .runtime import ptr, cur_stream, ws_args, require_cuda


def _rows(t):
  assert t.dim() == 2 and t.stride(1) == 1, "expected a row-major [rows, channels] tensor"
  return t.shape[0], t.shape[1], t.stride(0)


def _c(t):
  """Contiguous-rows view (ld % 4 == 0, 16-byte aligned base) or a packed copy."""
  if t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0 and t.stride(0) >= t.shape[1]:
    return t
  return t.contiguous()


# Convolution precision modes (include/pcmi.h: pcmi_set_conv_precision).  "bf16": the launches of the split-precision
# kernels round both operands to bf16 and take one bf16 product per 32-channel chunk, fp32 accumulation; every other
# launch and op is unchanged.  The mode is the calling thread's (thread-local in libpcmi).
CONV_PRECISIONS = {"fp32": 0, "bf16": 1}


def conv_precision_code(name):
  if not isinstance(name, str) or name not in CONV_PRECISIONS:
    raise ValueError("conv precision must be one of %s, got %r" % (sorted(CONV_PRECISIONS), name))
  return CONV_PRECISIONS[name]


@contextlib.contextmanager
def _conv_precision_code_as(code):
  """The calling thread's libpcmi conv precision set to `code` for the block (restored afterwards)."""
  prev = lib.pcmi_get_conv_precision()
  if prev == code:
    yield
    return
  check(lib.pcmi_set_conv_precision(code))
  try:
    yield
  finally:
    check(lib.pcmi_set_conv_precision(prev))


def _kmap_ref(kmap):
  return C.byref(kmap) if kmap is not None else None


class SparseConvFunction(Function):
  """MinkowskiConvolution(.Transpose)Function: fwd / bwd-data / bwd-weight
  (replaces MEB.Convolution{Forward,Backward}GPU; pc/model/modules/common.py:130-168)."""

  @staticmethod
  def forward(ctx, feats, kernel, bias, kmap, transpose, n_out, owner=None):
    require_cuda(feats, "sparse conv")
    feats = _c(feats)
    n_in, cin, in_ld = _rows(feats)
    cout = kernel.shape[-1]
    K = kmap.K if kmap is not None else 1
    assert kernel.is_contiguous() and kernel.numel() == K * cin * cout, "kernel shape does not match the map"
    out = torch.empty((n_out, cout), dtype=torch.float32, device=feats.device)
    M = kmap.M if kmap is not None else n_in
    ws, wsb = ws_args(lib.pcmi_spconv_workspace_bytes(n_in, n_out, cin, cout, K, M), feats.device)
    check(lib.pcmi_spconv_fwd(ptr(feats), in_ld, n_in, cin, ptr(kernel), cout, _kmap_ref(kmap), int(transpose),
                              ptr(bias), ptr(out), cout, n_out, ws, wsb, cur_stream(feats.device)))
    ctx.save_for_backward(feats, kernel)
    ctx.kmap, ctx.transpose, ctx.has_bias = kmap, int(transpose), bias is not None
    # autocast's rule: backward-data and weight gradient run in the forward's precision mode, whatever the mode is when
    # (and on whichever thread) .backward() runs
    ctx.precision = lib.pcmi_get_conv_precision()
    ctx.owner = owner  # keeps the coordinate manager (and the arena behind kmap) alive until backward
    return out

  @staticmethod
  @once_differentiable
  def backward(ctx, gout):
    feats, kernel = ctx.saved_tensors
    kmap = ctx.kmap
    gout = _c(gout)
    n_out, cout, g_ld = _rows(gout)
    n_in, cin, in_ld = _rows(feats)
    K = kmap.K if kmap is not None else 1
    M = kmap.M if kmap is not None else n_in
    dev = feats.device
    st = cur_stream(dev)
    ws, wsb = ws_args(lib.pcmi_spconv_workspace_bytes(n_in, n_out, cin, cout, K, M), dev)
    gin = gw = gb = None
    with _conv_precision_code_as(ctx.precision):
      if ctx.needs_input_grad[0]:
        gin = torch.empty((n_in, cin), dtype=torch.float32, device=dev)
        check(lib.pcmi_spconv_bwd_data(ptr(gout), g_ld, n_out, cout, ptr(kernel), cin, _kmap_ref(kmap), ctx.transpose,
                                       ptr(gin), cin, n_in, ws, wsb, st))
      if ctx.needs_input_grad[1]:
        gw = torch.empty_like(kernel)
        if ctx.has_bias and ctx.needs_input_grad[2]:
          gb = torch.empty((1, cout), dtype=torch.float32, device=dev)
        check(lib.pcmi_spconv_bwd_weight(ptr(feats), in_ld, n_in, cin, ptr(gout), g_ld, n_out, cout, _kmap_ref(kmap),
                                         ctx.transpose, ptr(gw), ptr(gb), ws, wsb, st))
    return gin, gw, gb, None, None, None, None


class BatchNormFunction(Function):
  """Training-mode BatchNorm1d over the rows, optionally fused with the residual add and
  ReLU that follow it in the reference blocks (pc/model/modules/resnet_block.py:44-60)."""

  @staticmethod
  def forward(ctx, x, gamma, beta, running_mean, running_var, momentum, eps, residual, relu):
    require_cuda(x, "batch norm")
    x = _c(x)
    n, c, x_ld = _rows(x)
    res = _c(residual) if residual is not None else None
    y = torch.empty((n, c), dtype=torch.float32, device=x.device)
    mean = torch.empty(c, dtype=torch.float32, device=x.device)
    invstd = torch.empty(c, dtype=torch.float32, device=x.device)
    ws, wsb = ws_args(lib.pcmi_bn_workspace_bytes(n, c), x.device)
    check(lib.pcmi_bn_fwd_train(ptr(x), x_ld, n, c, ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var),
                                float(momentum), float(eps), ptr(res), res.stride(0) if res is not None else 0,
                                int(relu), ptr(y), c, ptr(mean), ptr(invstd), ws, wsb, cur_stream(x.device)))
    ctx.save_for_backward(x, gamma, mean, invstd, y if relu else None)
    ctx.has_res, ctx.relu = residual is not None, bool(relu)
    return y

  @staticmethod
  @once_differentiable
  def backward(ctx, dy):
    x, gamma, mean, invstd, y = ctx.saved_tensors
    dy = _c(dy)
    n, c, x_ld = _rows(x)
    dev = x.device
    dx = torch.empty((n, c), dtype=torch.float32, device=dev)
    dres = torch.empty((n, c), dtype=torch.float32, device=dev) if ctx.has_res else None
    dgamma = torch.empty(c, dtype=torch.float32, device=dev)
    dbeta = torch.empty(c, dtype=torch.float32, device=dev)
    ws, wsb = ws_args(lib.pcmi_bn_workspace_bytes(n, c), dev)
    check(lib.pcmi_bn_bwd(ptr(dy), dy.stride(0), ptr(x), x_ld, ptr(y), c if y is not None else 0, n, c, ptr(gamma),
                          ptr(mean), ptr(invstd), ptr(dx), c, ptr(dres), c, ptr(dgamma), ptr(dbeta), ws, wsb,
                          cur_stream(dev)))
    return dx, dgamma, dbeta, None, None, None, None, dres, None


def batch_norm_eval(x, gamma, beta, running_mean, running_var, eps, residual=None, relu=False):
  require_cuda(x, "batch norm (eval)")
  x = _c(x)
  n, c, x_ld = _rows(x)
  res = _c(residual) if residual is not None else None
  y = torch.empty((n, c), dtype=torch.float32, device=x.device)
  check(lib.pcmi_bn_fwd_eval(ptr(x), x_ld, n, c, ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var),
                             float(eps), ptr(res), res.stride(0) if res is not None else 0, int(relu), ptr(y), c,
                             cur_stream(x.device)))
  return y


class ReLUFunction(Function):

  @staticmethod
  def forward(ctx, x):
    require_cuda(x, "relu")
    x = _c(x)
    n, c, ld = _rows(x)
    y = torch.empty((n, c), dtype=torch.float32, device=x.device)
    check(lib.pcmi_relu_fwd(ptr(x), ld, n, c, ptr(y), c, cur_stream(x.device)))
    ctx.save_for_backward(y)
    return y

  @staticmethod
  @once_differentiable
  def backward(ctx, dy):
    (y,) = ctx.saved_tensors
    dy = _c(dy)
    n, c, _ = _rows(y)
    dx = torch.empty_like(y)
    check(lib.pcmi_relu_bwd(ptr(dy), dy.stride(0), ptr(y), c, n, c, ptr(dx), c, cur_stream(y.device)))
    return dx


class AddFunction(Function):

  @staticmethod
  def forward(ctx, a, b):
    require_cuda(a, "add")
    a, b = _c(a), _c(b)
    n, c, _ = _rows(a)
    y = torch.empty((n, c), dtype=torch.float32, device=a.device)
    check(lib.pcmi_add(ptr(a), a.stride(0), ptr(b), b.stride(0), n, c, ptr(y), c, cur_stream(a.device)))
    return y

  @staticmethod
  def backward(ctx, dy):
    return dy, dy


class L2NormalizeFunction(Function):
  """F / ||F||_2 per row, no eps (pc/model/res16unet.py:262-266)."""

  @staticmethod
  def forward(ctx, x):
    require_cuda(x, "l2 normalise")
    x = _c(x)
    n, c, ld = _rows(x)
    y = torch.empty((n, c), dtype=torch.float32, device=x.device)
    norm = torch.empty(n, dtype=torch.float32, device=x.device)
    check(lib.pcmi_l2norm_fwd(ptr(x), ld, n, c, ptr(y), c, ptr(norm), cur_stream(x.device)))
    ctx.save_for_backward(y, norm)
    return y

  @staticmethod
  @once_differentiable
  def backward(ctx, dy):
    y, norm = ctx.saved_tensors
    dy = _c(dy)
    n, c, _ = _rows(y)
    dx = torch.empty_like(y)
    check(lib.pcmi_l2norm_bwd(ptr(dy), dy.stride(0), ptr(y), c, ptr(norm), n, c, ptr(dx), c, cur_stream(y.device)))
    return dx


class GatherRowsFunction(Function):
  """F[idx] with a scatter-add backward (pc/lib/ddp_trainer.py:209-213,409-410)."""

  @staticmethod
  def forward(ctx, src, idx):
    require_cuda(src, "gather rows")
    src = _c(src)
    idx = idx.to(device=src.device, dtype=torch.int64).contiguous()
    n, c = idx.shape[0], src.shape[1]
    out = torch.empty((n, c), dtype=torch.float32, device=src.device)
    check(lib.pcmi_gather_rows(ptr(src), src.stride(0), ptr(idx), n, c, ptr(out), c, cur_stream(src.device)))
    ctx.save_for_backward(idx)
    ctx.n_src = src.shape[0]
    return out

  @staticmethod
  @once_differentiable
  def backward(ctx, dout):
    (idx,) = ctx.saved_tensors
    dout = _c(dout)
    n, c = dout.shape
    dsrc = torch.zeros((ctx.n_src, c), dtype=torch.float32, device=dout.device)
    check(lib.pcmi_scatter_add_rows(ptr(dout), dout.stride(0), ptr(idx), n, c, ptr(dsrc), c, cur_stream(dout.device)))
    return dsrc, None


class GatherManyFunction(Function):
  """(F[idx_0], F[idx_1], ...) of ONE feature matrix -- the two clouds of a pair run as one two-segment tensor
  (lib/ddp_trainer.py: misc.joint_pair), the second cloud's indices already shifted past the first cloud's rows -- with all
  gradients scattered into ONE zero-filled buffer.  Through one GatherRowsFunction per index set on the slices F[:n0] /
  F[n0:] autograd enqueued nine small kernels between the PointInfoNCE loss and the backward pass (two fills + two scatters
  of the halves, two more full-size fills + two slice copies + an add: 92 us on the chain in profiles/r04zy_*; more for
  the four index sets of the hardest-contrastive loss); here: one fill and one scatter per index set (a scatter adds to
  what is there: index sets may share rows)."""

  @staticmethod
  def forward(ctx, src, *idxs):
    require_cuda(src, "gather many")
    src = _c(src)
    idxs = tuple(i.to(device=src.device, dtype=torch.int64).contiguous() for i in idxs)
    c = src.shape[1]
    outs = []
    for idx in idxs:
      out = torch.empty((idx.shape[0], c), dtype=torch.float32, device=src.device)
      check(lib.pcmi_gather_rows(ptr(src), src.stride(0), ptr(idx), idx.shape[0], c, ptr(out), c, cur_stream(src.device)))
      outs.append(out)
    ctx.save_for_backward(*idxs)
    ctx.n_src = src.shape[0]
    return tuple(outs)

  @staticmethod
  @once_differentiable
  def backward(ctx, *douts):
    idxs = ctx.saved_tensors
    c = douts[0].shape[1]
    dsrc = torch.zeros((ctx.n_src, c), dtype=torch.float32, device=douts[0].device)
    for idx, d in zip(idxs, douts):  # in argument order (deterministic; rows shared between index sets accumulate)
      d = _c(d)
      check(lib.pcmi_scatter_add_rows(ptr(d), d.stride(0), ptr(idx), d.shape[0], c, ptr(dsrc), c, cur_stream(d.device)))
    return (dsrc,) + (None,) * len(idxs)


GatherPairFunction = GatherManyFunction  # (the two-index-set case: q / k of the PointInfoNCE loss)


class NCELossFunction(Function):
  """mean_i(logsumexp_j(q_i.k_j/T) - q_i.k_i/T) without materialising the logits
  (torch.mm + CrossEntropyLoss at pc/lib/ddp_trainer.py:419-426)."""

  @staticmethod
  def forward(ctx, q, k, T):
    require_cuda(q, "nce loss")
    q, k = q.contiguous(), k.contiguous()
    n, c = q.shape
    lse = torch.empty(n, dtype=torch.float32, device=q.device)
    loss = torch.empty((), dtype=torch.float32, device=q.device)
    ws, wsb = ws_args(lib.pcmi_nce_workspace_bytes(n, c), q.device)
    check(lib.pcmi_nce_fwd(ptr(q), ptr(k), n, c, 1.0 / float(T), ptr(lse), ptr(loss), ws, wsb, cur_stream(q.device)))
    ctx.save_for_backward(q, k, lse)
    ctx.inv_T = 1.0 / float(T)
    return loss

  @staticmethod
  @once_differentiable
  def backward(ctx, gloss):
    q, k, lse = ctx.saved_tensors
    n, c = q.shape
    dq, dk = torch.empty_like(q), torch.empty_like(k)
    g = gloss.to(torch.float32).contiguous()
    ws, wsb = ws_args(lib.pcmi_nce_workspace_bytes(n, c), q.device)
    check(lib.pcmi_nce_bwd(ptr(q), ptr(k), ptr(lse), n, c, ctx.inv_T, ptr(g), ptr(dq), ptr(dk), ws, wsb,
                           cur_stream(q.device)))
    return dq, dk, None


def _partition_rule(r1_sq, r2_sq, azimuth, elevation, n_scenes):
  r1_sq, r2_sq, A, E, B = int(r1_sq), int(r2_sq), int(azimuth), int(elevation), int(n_scenes)
  return r1_sq, r2_sq, A, E, B, 2 * E * A


class PartitionNCELossFunction(Function):
  """The spatially partitioned PointInfoNCE of include/pcmi.h (csrc/nce_part.hip): one InfoNCE per partition (distance shell
  x elevation half x azimuth sector around the anchor, from the integer voxel coordinates `xyz` of the queries, scenes kept
  apart by `scene`), averaged over live rows, live partitions and live scenes.  One launch over the batch; the n x n logits
  and partitions are never written.  Gradients go to q and k only."""

  @staticmethod
  def forward(ctx, q, k, xyz, scene, T, r1_sq, r2_sq, azimuth, elevation, n_scenes):
    q, k = q.contiguous(), k.contiguous()
    xyz, scene = xyz.to(torch.int32).contiguous(), scene.to(torch.int32).contiguous()
    loss, lse, live = partition_nce_forward(q, k, xyz, scene, T, r1_sq, r2_sq, azimuth, elevation, n_scenes)
    ctx.save_for_backward(q, k, xyz, scene, lse, live)
    ctx.rule = (1.0 / float(T),) + _partition_rule(r1_sq, r2_sq, azimuth, elevation, n_scenes)
    return loss

  @staticmethod
  @once_differentiable
  def backward(ctx, gloss):
    q, k, xyz, scene, lse, live = ctx.saved_tensors
    inv_T, r1_sq, r2_sq, A, E, B, P = ctx.rule
    n, c = q.shape
    dq, dk = torch.empty_like(q), torch.empty_like(k)
    g = gloss.to(torch.float32).contiguous()
    ws, wsb = ws_args(lib.pcmi_pnce_workspace_bytes(n, c, B, P), q.device)
    check(lib.pcmi_pnce_bwd(ptr(q), ptr(k), ptr(xyz), ptr(scene), ptr(lse), ptr(live), n, c, B, inv_T, r1_sq, r2_sq, A, E, ptr(g),
                            ptr(dq), ptr(dk), ws, wsb, cur_stream(q.device)))
    return (dq, dk) + (None,) * 8


def partition_nce_forward(q, k, xyz, scene, T, r1_sq, r2_sq, azimuth, elevation, n_scenes):
  """(loss, lse [n, P], live [n_scenes, P]) of the partitioned loss without autograd: lse of a (row, partition) that is not
  live is l_ii; live[s, p] is the number of live rows of scene s in partition p."""
  require_cuda(q, "partition nce loss")
  q, k = q.detach().contiguous(), k.detach().contiguous()
  xyz, scene = xyz.to(torch.int32).contiguous(), scene.to(torch.int32).contiguous()
  n, c = q.shape
  assert xyz.shape == (n, 3) and scene.shape == (n,), "xyz [n, 3] and scene [n] go with the n rows of q"
  r1_sq, r2_sq, A, E, B, P = _partition_rule(r1_sq, r2_sq, azimuth, elevation, n_scenes)
  lse = torch.empty((n, max(P, 1)), dtype=torch.float32, device=q.device)
  live = torch.empty((max(B, 1), max(P, 1)), dtype=torch.int32, device=q.device)
  loss = torch.empty((), dtype=torch.float32, device=q.device)
  ws, wsb = ws_args(lib.pcmi_pnce_workspace_bytes(n, c, B, P), q.device)
  check(lib.pcmi_pnce_fwd(ptr(q), ptr(k), ptr(xyz), ptr(scene), n, c, B, 1.0 / float(T), r1_sq, r2_sq, A, E, ptr(lse), ptr(live),
                          ptr(loss), ws, wsb, cur_stream(q.device)))
  return loss, lse, live


def partition_matrix(xyz, scene, r1_sq, r2_sq, azimuth, elevation, n_scenes):
  """part(i, j) of every pair as int8 [n, n] (-1: j is no negative of i) from the device function the loss kernels use; a test
  aid, n <= 4096."""
  require_cuda(xyz, "partition matrix")
  xyz, scene = xyz.to(torch.int32).contiguous(), scene.to(torch.int32).contiguous()
  n = xyz.shape[0]
  r1_sq, r2_sq, A, E, B, _ = _partition_rule(r1_sq, r2_sq, azimuth, elevation, n_scenes)
  part = torch.empty((n, n), dtype=torch.int8, device=xyz.device)
  check(lib.pcmi_pnce_partition(ptr(xyz), ptr(scene), n, B, r1_sq, r2_sq, A, E, ptr(part), cur_stream(xyz.device)))
  return part


def pdist_argmin(a, b):
  """(min_s sqrt(|a_p - b_s|^2 + 1e-7), argmin) -- pc/lib/ddp_trainer.py:182-184,218-219."""
  require_cuda(a, "pdist_argmin")
  a, b = a.contiguous(), b.contiguous()
  p, c = a.shape
  dmin = torch.empty(p, dtype=torch.float32, device=a.device)
  amin = torch.empty(p, dtype=torch.int32, device=a.device)
  check(lib.pcmi_pdist_argmin(ptr(a), p, ptr(b), b.shape[0], c, ptr(dmin), ptr(amin), cur_stream(a.device)))
  return dmin, amin


class PairKeySet:
  """Device hash set of the int64 keys i + j*M of the positive pairs
  (_hash + np.isin at pc/lib/ddp_trainer.py:39-51,224-234)."""

  def __init__(self, pairs_i32, M):
    require_cuda(pairs_i32, "pair key set")
    pairs = pairs_i32.to(torch.int32).contiguous()
    self.M = int(M)
    nbytes = lib.pcmi_keyset_bytes(pairs.shape[0])
    self.buf = torch.empty(nbytes, dtype=torch.uint8, device=pairs.device)
    check(lib.pcmi_keyset_build(ptr(pairs), pairs.shape[0], self.M, ptr(self.buf), nbytes, cur_stream(pairs.device)))

  def absent(self, a_i64, b_i64):
    a, b = a_i64.to(torch.int64).contiguous(), b_i64.to(torch.int64).contiguous()
    mask = torch.empty(a.shape[0], dtype=torch.uint8, device=a.device)
    check(lib.pcmi_keyset_mask_absent(ptr(self.buf), self.buf.numel(), ptr(a), ptr(b), a.shape[0], self.M, ptr(mask),
                                      cur_stream(a.device)))
    return mask


class HardestLossFunction(Function):
  """losses = [pos_loss, neg_loss] of pc/lib/ddp_trainer.py:235-238 given the mined minima."""

  @staticmethod
  def forward(ctx, posF0, posF1, subF0, subF1, d01min, d01ind, mask0, d10min, d10ind, mask1, pos_thresh, neg_thresh):
    require_cuda(posF0, "hardest loss")
    posF0, posF1, subF0, subF1 = posF0.contiguous(), posF1.contiguous(), subF0.contiguous(), subF1.contiguous()
    p, c = posF0.shape
    dev = posF0.device
    losses = torch.empty(2, dtype=torch.float32, device=dev)
    stats = torch.empty(8, dtype=torch.float32, device=dev)
    ws, wsb = ws_args(lib.pcmi_hardest_workspace_bytes(p), dev)
    check(lib.pcmi_hardest_loss_fwd(ptr(posF0), ptr(posF1), p, c, ptr(d01min), ptr(mask0), ptr(d10min), ptr(mask1),
                                    float(pos_thresh), float(neg_thresh), ptr(losses), ptr(stats), ws, wsb,
                                    cur_stream(dev)))
    ctx.save_for_backward(posF0, posF1, subF0, subF1, d01min, d01ind, mask0, d10min, d10ind, mask1, stats)
    ctx.thresh = (float(pos_thresh), float(neg_thresh))
    return losses

  @staticmethod
  @once_differentiable
  def backward(ctx, gl):
    posF0, posF1, subF0, subF1, d01min, d01ind, mask0, d10min, d10ind, mask1, stats = ctx.saved_tensors
    p, c = posF0.shape
    gl = gl.to(torch.float32).contiguous()
    g0, g1 = torch.empty_like(posF0), torch.empty_like(posF1)
    gs0, gs1 = torch.zeros_like(subF0), torch.zeros_like(subF1)
    check(lib.pcmi_hardest_loss_bwd(ptr(posF0), ptr(posF1), p, ptr(subF0), ptr(subF1), c, ptr(d01min), ptr(d01ind),
                                    ptr(mask0), ptr(d10min), ptr(d10ind), ptr(mask1), ctx.thresh[0], ctx.thresh[1],
                                    ptr(stats), ptr(gl), ptr(g0), ptr(g1), ptr(gs0), ptr(gs1), cur_stream(posF0.device)))
    return (g0, g1, gs0, gs1) + (None,) * 8


class SoftmaxCrossEntropyFunction(Function):
  """torch.nn.CrossEntropyLoss(ignore_index=ignore_label) on logits [n, c] / int labels [n]
  (downstream/semseg/lib/train.py:64,124), as libpcmi kernels."""

  @staticmethod
  def forward(ctx, logits, labels, ignore_label):
    require_cuda(logits, "softmax cross-entropy")
    x = logits if (logits.stride(1) == 1 and logits.dtype == torch.float32) else logits.float().contiguous()
    lb = labels.to(device=x.device, dtype=torch.int32).contiguous()
    n, c = x.shape
    out2 = torch.empty(2, dtype=torch.float32, device=x.device)
    ws, wsb = ws_args(lib.pcmi_softmax_ce_workspace_bytes(n), x.device)
    check(lib.pcmi_softmax_ce_fwd(ptr(x), x.stride(0), n, c, ptr(lb), int(ignore_label), ptr(out2), ws, wsb, cur_stream(x.device)))
    ctx.save_for_backward(x, lb, out2)
    ctx.ignore = int(ignore_label)
    return out2[0]

  @staticmethod
  @once_differentiable
  def backward(ctx, gloss):
    x, lb, out2 = ctx.saved_tensors
    n, c = x.shape
    dx = torch.empty((n, c), dtype=torch.float32, device=x.device)
    g = gloss.reshape(1).to(dtype=torch.float32, device=x.device).contiguous()
    check(lib.pcmi_softmax_ce_bwd(ptr(x), x.stride(0), n, c, ptr(lb), ctx.ignore, ptr(out2), ptr(g), ptr(dx), c,
                                  cur_stream(x.device)))
    return dx, None, None


def pairs_scan_host(pos_pairs):
  """(number of runs of column 0, sorted?) of HOST correspondences [P, 2] int32 -- one native pass (pcmi_pairs_scan_host)."""
  assert (not pos_pairs.is_cuda) and pos_pairs.dtype == torch.int32 and pos_pairs.dim() == 2 and pos_pairs.shape[1] == 2 \
      and pos_pairs.is_contiguous(), "correspondences must be a contiguous CPU int32 [P, 2] tensor"
  n, srt = C.c_int64(), C.c_int()
  check(lib.pcmi_pairs_scan_host(C.c_void_p(pos_pairs.data_ptr()), pos_pairs.shape[0], C.byref(n), C.byref(srt)))
  return n.value, bool(srt.value)


def pair_select(pairs_dev, n_unique, uniform_dev, sampled_dev=None, workspace=None):
  """Device side of the PointInfoNCE pair selection (pc/lib/ddp_trainer.py:400-417; pcmi_pair_select): row indices
  (q_idx into F0, k_idx into F1), int64 [npos] (or [n_unique] without a sub-sample).  Enqueued on torch's current stream;
  workspace: a caller-owned uint8 tensor (a call on a stream other than the compute stream must not use the shared
  scratch buffer of the compute-stream ops)."""
  require_cuda(pairs_dev, "pair selection")
  assert pairs_dev.dtype == torch.int32 and pairs_dev.is_contiguous() and uniform_dev.dtype == torch.float32
  assert uniform_dev.numel() == n_unique and (sampled_dev is None or sampled_dev.dtype == torch.int64)
  n_sel = sampled_dev.numel() if sampled_dev is not None else n_unique
  q = torch.empty(n_sel, dtype=torch.int64, device=pairs_dev.device)
  k = torch.empty(n_sel, dtype=torch.int64, device=pairs_dev.device)
  P = pairs_dev.shape[0]
  need = lib.pcmi_pair_select_workspace_bytes(P)
  if workspace is not None:
    assert workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.numel() >= need
    ws, wsb = C.c_void_p(workspace.data_ptr()), C.c_size_t(workspace.numel())
  else:
    ws, wsb = ws_args(need, pairs_dev.device)
  check(lib.pcmi_pair_select(ptr(pairs_dev), P, n_unique, ptr(uniform_dev), ptr(sampled_dev), n_sel, ptr(q), ptr(k), ws, wsb,
                             cur_stream(pairs_dev.device)))
  return q, k


def sgd_step(w, g, v, lr, momentum, weight_decay, grad_scale=1.0, dampening=0.0, first_step=True):
  """torch.optim.SGD.step on flat buffers (pc/lib/ddp_trainer.py:107-111,319,435; with dampening:
  downstream/semseg/lib/solvers.py:52-60).  first_step: torch fills a fresh momentum buffer with the gradient itself."""
  require_cuda(w, "sgd step")
  check(lib.pcmi_sgd_step_dampened(ptr(w), ptr(g), ptr(v), w.numel(), float(lr), float(momentum), float(dampening),
                                   float(weight_decay), float(grad_scale), int(bool(first_step)), cur_stream(w.device)))


# ---------------------------------------------------------------------------------------------------------------------
# pooling over kernel maps, per-instance reductions, instance norm (csrc/pool.hip); `owner` keeps the coordinate manager
# -- and the arena behind the map / segment tables -- alive until backward
# ---------------------------------------------------------------------------------------------------------------------
def _packed(t):
  """Row-major fp32 rows with a 16-byte aligned base and a leading dimension that is a multiple of 4 (else a copy)."""
  require_cuda(t, "pooling")
  return _c(t.float() if t.dtype != torch.float32 else t)


class PoolFunction(Function):
  """MinkowskiSumPooling / MinkowskiAvgPooling over a (k=3, s=1) or (k=2, s=2) map (pc/model/modules/common.py:170-214)."""

  @staticmethod
  def forward(ctx, feats, kmap, average, owner=None):
    x = _packed(feats)
    n, c, ld = _rows(x)
    assert n == kmap.n_in, "pooling: %d rows for a map with %d input rows" % (n, kmap.n_in)
    out = torch.empty((kmap.n_out, c), dtype=torch.float32, device=x.device)
    check(lib.pcmi_pool_fwd(ptr(x), ld, c, C.byref(kmap), int(average), ptr(out), c, cur_stream(x.device)))
    ctx.kmap, ctx.average, ctx.owner, ctx.c = kmap, int(average), owner, c
    return out

  @staticmethod
  @once_differentiable
  def backward(ctx, gout):
    g = _packed(gout)
    kmap, dev = ctx.kmap, g.device
    gin = torch.empty((kmap.n_in, ctx.c), dtype=torch.float32, device=dev)
    ws, wsb = ws_args(lib.pcmi_pool_workspace_bytes(kmap.n_out), dev)
    check(lib.pcmi_pool_bwd(ptr(g), g.stride(0), ctx.c, C.byref(kmap), ctx.average, ptr(gin), ctx.c, ws, wsb,
                            cur_stream(dev)))
    return gin, None, None, None


class UnpoolFunction(Function):
  """MinkowskiAvgUnpooling / MinkowskiPoolingTranspose(2, 2): out[child] = in[parent] on the existing finer key
  (pc/model/modules/common.py:189-200).  kmap: the fine -> coarse (k=2, s=2) map, as a transposed conv uses."""

  @staticmethod
  def forward(ctx, feats, kmap, owner=None):
    x = _packed(feats)
    n, c, ld = _rows(x)
    assert n == kmap.n_out, "unpooling: %d rows for a coarse key of %d rows" % (n, kmap.n_out)
    out = torch.empty((kmap.n_in, c), dtype=torch.float32, device=x.device)
    check(lib.pcmi_unpool_fwd(ptr(x), ld, c, C.byref(kmap), ptr(out), c, cur_stream(x.device)))
    ctx.kmap, ctx.owner, ctx.c = kmap, owner, c
    return out

  @staticmethod
  @once_differentiable
  def backward(ctx, gout):
    g = _packed(gout)
    kmap = ctx.kmap
    gin = torch.empty((kmap.n_out, ctx.c), dtype=torch.float32, device=g.device)
    check(lib.pcmi_unpool_bwd(ptr(g), g.stride(0), ctx.c, C.byref(kmap), ptr(gin), ctx.c, cur_stream(g.device)))
    return gin, None, None


class GlobalPoolFunction(Function):
  """MinkowskiGlobalPooling(average): per-instance sum or mean, one output row per batch index (ascending)."""

  @staticmethod
  def forward(ctx, feats, seg, average, owner=None):
    x = _packed(feats)
    n, c, ld = _rows(x)
    assert n == seg.n, "global pooling: %d rows for a key of %d rows" % (n, seg.n)
    out = torch.empty((seg.n_inst, c), dtype=torch.float32, device=x.device)
    ws, wsb = ws_args(lib.pcmi_segments_workspace_bytes(C.byref(seg), c), x.device)
    check(lib.pcmi_global_pool_fwd(ptr(x), ld, c, C.byref(seg), int(average), ptr(out), c, ws, wsb, cur_stream(x.device)))
    ctx.seg, ctx.average, ctx.owner, ctx.c = seg, int(average), owner, c
    return out

  @staticmethod
  @once_differentiable
  def backward(ctx, gout):
    g = _packed(gout)
    seg = ctx.seg
    gin = torch.empty((seg.n, ctx.c), dtype=torch.float32, device=g.device)
    check(lib.pcmi_global_pool_bwd(ptr(g), g.stride(0), ctx.c, C.byref(seg), ctx.average, ptr(gin), ctx.c,
                                   cur_stream(g.device)))
    return gin, None, None, None


class BroadcastFunction(Function):
  """MinkowskiBroadcast{Addition,Multiplication}: out[r] = x[r] op g[instance(r)] (op 0: add, 1: multiply)."""

  @staticmethod
  def forward(ctx, x, g, seg, op, owner=None):
    x, g = _packed(x), _packed(g)
    n, c, ld = _rows(x)
    assert n == seg.n and g.shape == (seg.n_inst, c), "broadcast: shapes do not match the instances"
    out = torch.empty((n, c), dtype=torch.float32, device=x.device)
    check(lib.pcmi_broadcast_fwd(ptr(x), ld, ptr(g), g.stride(0), c, C.byref(seg), int(op), ptr(out), c,
                                 cur_stream(x.device)))
    ctx.save_for_backward(x if op == 1 else None, g if op == 1 else None)
    ctx.seg, ctx.op, ctx.owner, ctx.c = seg, int(op), owner, c
    return out

  @staticmethod
  @once_differentiable
  def backward(ctx, gout):
    x, g = ctx.saved_tensors
    go = _packed(gout)
    seg, c, dev = ctx.seg, ctx.c, go.device
    gx = torch.empty((seg.n, c), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
    gg = torch.empty((seg.n_inst, c), dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
    ws, wsb = ws_args(lib.pcmi_segments_workspace_bytes(C.byref(seg), c), dev)
    check(lib.pcmi_broadcast_bwd(ptr(go), go.stride(0), ptr(x), x.stride(0) if x is not None else 0, ptr(g),
                                 g.stride(0) if g is not None else 0, c, C.byref(seg), ctx.op, ptr(gx), c, ptr(gg), c,
                                 ws, wsb, cur_stream(dev)))
    return gx, gg, None, None, None


class InstanceNormFunction(Function):
  """MinkowskiInstanceNorm (downstream/semseg/lib/layers.py:54-90): per-instance, per-channel mean and biased variance,
  affine weight / bias shared by the instances, optionally fused with the residual add and ReLU of the blocks."""

  @staticmethod
  def forward(ctx, x, weight, bias, seg, eps, residual, relu, owner=None):
    x = _packed(x)
    n, c, ld = _rows(x)
    assert n == seg.n, "instance norm: %d rows for a key of %d rows" % (n, seg.n)
    w, b = weight.reshape(-1).contiguous(), bias.reshape(-1).contiguous()
    assert w.numel() == c and b.numel() == c, "instance norm: weight / bias of %d for %d channels" % (w.numel(), c)
    res = _packed(residual) if residual is not None else None
    assert res is None or res.shape == x.shape, "instance norm: residual %s for features %s" % (res.shape, x.shape)
    y = torch.empty((n, c), dtype=torch.float32, device=x.device)
    mean = torch.empty((seg.n_inst, c), dtype=torch.float32, device=x.device)
    invstd = torch.empty((seg.n_inst, c), dtype=torch.float32, device=x.device)
    ws, wsb = ws_args(lib.pcmi_segments_workspace_bytes(C.byref(seg), c), x.device)
    check(lib.pcmi_instnorm_fwd(ptr(x), ld, c, C.byref(seg), ptr(w), ptr(b), float(eps), ptr(res),
                                res.stride(0) if res is not None else 0, int(relu), ptr(y), c, ptr(mean), ptr(invstd),
                                ws, wsb, cur_stream(x.device)))
    ctx.save_for_backward(x, w, mean, invstd, y if relu else None)
    ctx.seg, ctx.owner, ctx.has_res, ctx.wshape, ctx.bshape = seg, owner, residual is not None, weight.shape, bias.shape
    return y

  @staticmethod
  @once_differentiable
  def backward(ctx, dy):
    x, w, mean, invstd, y = ctx.saved_tensors
    dy = _packed(dy)
    n, c, x_ld = _rows(x)
    dev, seg = x.device, ctx.seg
    dx = torch.empty((n, c), dtype=torch.float32, device=dev)
    dres = torch.empty((n, c), dtype=torch.float32, device=dev) if ctx.has_res else None
    dw = torch.empty(c, dtype=torch.float32, device=dev)
    db = torch.empty(c, dtype=torch.float32, device=dev)
    ws, wsb = ws_args(lib.pcmi_segments_workspace_bytes(C.byref(seg), c), dev)
    check(lib.pcmi_instnorm_bwd(ptr(dy), dy.stride(0), ptr(x), x_ld, ptr(y), c, c, C.byref(seg), ptr(w), ptr(mean),
                                ptr(invstd), ptr(dx), c, ptr(dres), c, ptr(dw), ptr(db), ws, wsb, cur_stream(dev)))
    return dx, dw.reshape(ctx.wshape), db.reshape(ctx.bshape), None, None, dres, None, None


# ---------------------------------------------------------------------------------------------------------------------
# PointNet++ point-set ops (csrc/pointset.hip) -- the reference's pointnet2 extension
# (downstream/votenet_det_new/models/backbone/pointnet2/pointnet2_utils.py).  Channel-first fp32 features [B, C, N],
# int32 indices, as there.  The forward passes validate their indices on the device (an index outside the range raises
# PcmiError instead of faulting); the backward passes reuse the validated indices without a host synchronisation.
# ---------------------------------------------------------------------------------------------------------------------
def _f32c(t, who):
  require_cuda(t, who)
  return (t if t.dtype == torch.float32 else t.float()).contiguous()


def _i32c(t, device):
  return t.to(device=device, dtype=torch.int32).contiguous()


def furthest_point_sample_segments(xyz, offs, rows, n_clouds, max_cloud, npoint):
  """One furthest-point-sampling launch over the segments of xyz [N, 3]: offs / rows are device pointers (ints or
  ctypes void pointers; pcmi_segments_t's tables, rows may be None), max_cloud an upper bound of any cloud's size.
  Returns (positions within the cloud, rows of xyz), both int32 [n_clouds, npoint]; -1 for an empty cloud.  No host sync."""
  xyz = _f32c(xyz, "furthest point sampling")
  assert xyz.dim() == 2 and xyz.shape[1] == 3, "xyz must be [N, 3]"
  N, dev = xyz.shape[0], xyz.device
  out = torch.empty((n_clouds, npoint), dtype=torch.int32, device=dev)
  out_rows = torch.empty((n_clouds, npoint), dtype=torch.int32, device=dev)
  ws, wsb = ws_args(lib.pcmi_fps_workspace_bytes(N, max_cloud, int(rows is not None)), dev)
  check(lib.pcmi_fps(ptr(xyz), N, rows, offs, n_clouds, max_cloud, npoint, ptr(out), ptr(out_rows), ws, wsb, cur_stream(dev)))
  return out, out_rows


class FurthestPointSampleFunction(Function):
  """furthest_point_sample(xyz [B, N, 3], npoint) -> int32 [B, npoint] (pointnet2_utils.py:51-80); not differentiable."""

  @staticmethod
  def forward(ctx, xyz, npoint):
    xyz = _f32c(xyz, "furthest point sampling")
    assert xyz.dim() == 3 and xyz.shape[2] == 3, "xyz must be [B, N, 3]"
    B, N, _ = xyz.shape
    out = torch.empty((B, int(npoint)), dtype=torch.int32, device=xyz.device)
    ws, wsb = ws_args(lib.pcmi_fps_workspace_bytes(B * N, N, 0), xyz.device)
    check(lib.pcmi_fps(ptr(xyz), B * N, None, None, B, N, int(npoint), ptr(out), None, ws, wsb, cur_stream(xyz.device)))
    ctx.mark_non_differentiable(out)
    return out

  @staticmethod
  def backward(ctx, a=None):
    return None, None


class BallQueryFunction(Function):
  """ball_query(radius, nsample, xyz [B, N, 3], new_xyz [B, npoint, 3]) -> int32 [B, npoint, nsample]
  (pointnet2_utils.py:260-291); not differentiable."""

  @staticmethod
  def forward(ctx, radius, nsample, xyz, new_xyz):
    xyz, new_xyz = _f32c(xyz, "ball query"), _f32c(new_xyz, "ball query")
    assert xyz.dim() == 3 and new_xyz.dim() == 3 and xyz.shape[2] == 3 and new_xyz.shape[2] == 3 and \
        xyz.shape[0] == new_xyz.shape[0], "ball query: xyz [B, N, 3], new_xyz [B, npoint, 3]"
    B, N, _ = xyz.shape
    npoint = new_xyz.shape[1]
    idx = torch.empty((B, npoint, int(nsample)), dtype=torch.int32, device=xyz.device)
    check(lib.pcmi_ball_query(ptr(xyz), ptr(new_xyz), B, N, npoint, float(radius), int(nsample), ptr(idx),
                              cur_stream(xyz.device)))
    ctx.mark_non_differentiable(idx)
    return idx

  @staticmethod
  def backward(ctx, a=None):
    return None, None, None, None


def three_nn_squared(unknown, known):
  """(squared distances fp32 [B, n, 3], indices int32 [B, n, 3]) of the three nearest known points (pcmi_three_nn)."""
  unknown, known = _f32c(unknown, "three_nn"), _f32c(known, "three_nn")
  assert unknown.dim() == 3 and known.dim() == 3 and unknown.shape[2] == 3 and known.shape[2] == 3 and \
      unknown.shape[0] == known.shape[0], "three_nn: unknown [B, n, 3], known [B, m, 3]"
  B, n, _ = unknown.shape
  d2 = torch.empty((B, n, 3), dtype=torch.float32, device=unknown.device)
  idx = torch.empty((B, n, 3), dtype=torch.int32, device=unknown.device)
  check(lib.pcmi_three_nn(ptr(unknown), ptr(known), B, n, known.shape[1], ptr(d2), ptr(idx), cur_stream(unknown.device)))
  return d2, idx


class ThreeNNFunction(Function):
  """three_nn(unknown [B, n, 3], known [B, m, 3]) -> (l2 distances [B, n, 3], int32 indices [B, n, 3])
  (pointnet2_utils.py:120-149); not differentiable."""

  @staticmethod
  def forward(ctx, unknown, known):
    d2, idx = three_nn_squared(unknown, known)
    dist = torch.sqrt(d2)
    ctx.mark_non_differentiable(dist, idx)
    return dist, idx

  @staticmethod
  def backward(ctx, a=None, b=None):
    return None, None


class GatherOperationFunction(Function):
  """gather_operation(features [B, C, N], idx [B, npoint]) -> [B, C, npoint] (pointnet2_utils.py:83-117)."""

  @staticmethod
  def forward(ctx, features, idx):
    f = _f32c(features, "gather_operation")
    idx = _i32c(idx, f.device)
    assert f.dim() == 3 and idx.dim() == 2 and idx.shape[0] == f.shape[0], "gather_operation: features [B, C, N], idx [B, npoint]"
    B, Cc, N = f.shape
    m = idx.shape[1]
    out = torch.empty((B, Cc, m), dtype=torch.float32, device=f.device)
    check(lib.pcmi_gather_points_fwd(ptr(f), ptr(idx), B, Cc, N, m, ptr(out), 1, cur_stream(f.device)))
    ctx.save_for_backward(idx)
    ctx.shape = (B, Cc, N, m)
    return out

  @staticmethod
  @once_differentiable
  def backward(ctx, gout):
    (idx,) = ctx.saved_tensors
    B, Cc, N, m = ctx.shape
    g = _f32c(gout, "gather_operation")
    gf = torch.empty((B, Cc, N), dtype=torch.float32, device=g.device)
    ws, wsb = ws_args(lib.pcmi_pointset_scatter_workspace_bytes(B * m, B * N), g.device)
    check(lib.pcmi_gather_points_bwd(ptr(g), ptr(idx), B, Cc, N, m, ptr(gf), 0, ws, wsb, cur_stream(g.device)))
    return gf, None


class GroupingOperationFunction(Function):
  """grouping_operation(features [B, C, N], idx [B, npoint, nsample]) -> [B, C, npoint, nsample]
  (pointnet2_utils.py:209-257)."""

  @staticmethod
  def forward(ctx, features, idx):
    f = _f32c(features, "grouping_operation")
    idx = _i32c(idx, f.device)
    assert f.dim() == 3 and idx.dim() == 3 and idx.shape[0] == f.shape[0], \
        "grouping_operation: features [B, C, N], idx [B, npoint, nsample]"
    B, Cc, N = f.shape
    _, npoint, ns = idx.shape
    out = torch.empty((B, Cc, npoint, ns), dtype=torch.float32, device=f.device)
    check(lib.pcmi_group_points_fwd(ptr(f), ptr(idx), B, Cc, N, npoint, ns, ptr(out), 1, cur_stream(f.device)))
    ctx.save_for_backward(idx)
    ctx.shape = (B, Cc, N, npoint, ns)
    return out

  @staticmethod
  @once_differentiable
  def backward(ctx, gout):
    (idx,) = ctx.saved_tensors
    B, Cc, N, npoint, ns = ctx.shape
    g = _f32c(gout, "grouping_operation")
    gf = torch.empty((B, Cc, N), dtype=torch.float32, device=g.device)
    ws, wsb = ws_args(lib.pcmi_pointset_scatter_workspace_bytes(B * npoint * ns, B * N), g.device)
    check(lib.pcmi_group_points_bwd(ptr(g), ptr(idx), B, Cc, N, npoint, ns, ptr(gf), 0, ws, wsb, cur_stream(g.device)))
    return gf, None


class ThreeInterpolateFunction(Function):
  """three_interpolate(features [B, c, m], idx [B, n, 3], weight [B, n, 3]) -> [B, c, n] (pointnet2_utils.py:152-206);
  differentiable in the features only, as the reference."""

  @staticmethod
  def forward(ctx, features, idx, weight):
    f = _f32c(features, "three_interpolate")
    idx = _i32c(idx, f.device)
    w = _f32c(weight, "three_interpolate")
    assert f.dim() == 3 and idx.dim() == 3 and idx.shape[2] == 3 and w.shape == idx.shape and idx.shape[0] == f.shape[0], \
        "three_interpolate: features [B, c, m], idx / weight [B, n, 3]"
    B, Cc, M = f.shape
    n = idx.shape[1]
    out = torch.empty((B, Cc, n), dtype=torch.float32, device=f.device)
    check(lib.pcmi_three_interpolate_fwd(ptr(f), ptr(idx), ptr(w), B, Cc, M, n, ptr(out), 1, cur_stream(f.device)))
    ctx.save_for_backward(idx, w)
    ctx.shape = (B, Cc, M, n)
    return out

  @staticmethod
  @once_differentiable
  def backward(ctx, gout):
    idx, w = ctx.saved_tensors
    B, Cc, M, n = ctx.shape
    g = _f32c(gout, "three_interpolate")
    gf = torch.empty((B, Cc, M), dtype=torch.float32, device=g.device)
    ws, wsb = ws_args(lib.pcmi_pointset_scatter_workspace_bytes(B * n * 3, B * M), g.device)
    check(lib.pcmi_three_interpolate_bwd(ptr(g), ptr(idx), ptr(w), B, Cc, M, n, ptr(gf), 0, ws, wsb, cur_stream(g.device)))
    return gf, None, None


# ---------------------------------------------------------------------------------------------------------------------
# VoteNet detection head (csrc/detect.hip): the matching of the loss (downstream/votenet_det_new/lib/utils/nn_distance.py)
# and the decoding of the predictions (models/ap_helper.py parse_predictions).
# ---------------------------------------------------------------------------------------------------------------------
NN_DISTANCE_MODES = {"l2": 0, "l1": 1, "huber": 2}


class NNDistanceFunction(Function):
  """nn_distance(pc1 [B, N, 3], pc2 [B, M, 3]) -> (dist1 [B, N], idx1 int64 [B, N], dist2 [B, M], idx2 int64 [B, M])
  (nn_distance.py:34-61): two pcmi_nn_distance_fwd launches; the backward pass routes both distance gradients to their
  argmin pairs in one pcmi_nn_distance_bwd.  The lowest index wins a tie.  The indices are not differentiable."""

  @staticmethod
  def forward(ctx, pc1, pc2, mode, delta):
    a, b = _f32c(pc1, "nn_distance"), _f32c(pc2, "nn_distance")
    B, N, _ = a.shape
    M = b.shape[1]
    dev = a.device
    dist1 = torch.empty((B, N), dtype=torch.float32, device=dev)
    dist2 = torch.empty((B, M), dtype=torch.float32, device=dev)
    idx1 = torch.empty((B, N), dtype=torch.int32, device=dev)
    idx2 = torch.empty((B, M), dtype=torch.int32, device=dev)
    st = cur_stream(dev)
    check(lib.pcmi_nn_distance_fwd(ptr(a), ptr(b), B, N, M, mode, delta, ptr(dist1), ptr(idx1), st))
    check(lib.pcmi_nn_distance_fwd(ptr(b), ptr(a), B, M, N, mode, delta, ptr(dist2), ptr(idx2), st))
    ctx.save_for_backward(a, b, idx1, idx2)
    ctx.args = (B, N, M, mode, delta)
    i1, i2 = idx1.long(), idx2.long()
    ctx.mark_non_differentiable(i1, i2)
    return dist1, i1, dist2, i2

  @staticmethod
  @once_differentiable
  def backward(ctx, g1, _gi1, g2, _gi2):
    a, b, idx1, idx2 = ctx.saved_tensors
    B, N, M, mode, delta = ctx.args
    g1, g2 = _f32c(g1, "nn_distance"), _f32c(g2, "nn_distance")
    ga, gb = torch.empty_like(a), torch.empty_like(b)
    ws, wsb = ws_args(lib.pcmi_nn_distance_bwd_workspace_bytes(B, N, M), a.device)
    check(lib.pcmi_nn_distance_bwd(ptr(a), ptr(b), ptr(idx1), ptr(idx2), ptr(g1), ptr(g2), B, N, M, mode, delta, ptr(ga), ptr(gb),
                                   ws, wsb, cur_stream(a.device)))
    return ga, gb, None, None


def box_decode(center, heading_scores, heading_residuals, size_scores, size_residuals, sem_cls_scores, objectness_scores,
               mean_size_arr, zero_heading, with_counts_of=None, nms=None, min_points=5):
  """pcmi_box_decode, then (with_counts_of = point_clouds [B, N, >= 3]) pcmi_box_point_counts and (nms = (mode, old_type,
  nms_iou)) pcmi_box_nms over the boxes holding at least min_points points (all of them without counts).  Returns a dict of device
  tensors: heading_class / size_class / sem_cls (int32 [B, K]), box_params [B, K, 7], corners [B, K, 8, 3], minmax [B, K, 6],
  obj_prob [B, K], sem_cls_probs [B, K, Cls], counts (int32 [B, K] or None), pred_mask (int32 [B, K] or None), and `packed`:
  the one float32 buffer that corners, obj_prob, sem_cls_probs, sem_cls and pred_mask are views of, in this order (the int32
  ones bit-cast), so that a single copy reads all of them back.  No host synchronisation."""
  who = "box_decode"
  ts = [_f32c(t, who) for t in (center, heading_scores, heading_residuals, size_scores, size_residuals, sem_cls_scores,
                               objectness_scores, mean_size_arr)]
  c, hs, hr, ss, sr, sem, obj, msa = ts
  assert c.dim() == 3 and c.shape[2] == 3, "box_decode: center [B, K, 3]"
  B, K, _ = c.shape
  H, S, Cls = hs.shape[2], ss.shape[2], sem.shape[2]
  assert hs.shape == (B, K, H) and hr.shape == (B, K, H) and ss.shape == (B, K, S) and sr.shape == (B, K, S, 3) and \
      sem.shape == (B, K, Cls) and obj.shape == (B, K, 2) and msa.shape == (S, 3), "box_decode: inconsistent shapes"
  dev = c.device
  n = B * K
  packed = torch.empty(n * (24 + 1 + Cls + 2), dtype=torch.float32, device=dev)
  o = 0
  corners = packed[o:o + n * 24].view(B, K, 8, 3); o += n * 24
  obj_prob = packed[o:o + n].view(B, K); o += n
  sem_probs = packed[o:o + n * Cls].view(B, K, Cls); o += n * Cls
  sem_cls = packed[o:o + n].view(torch.int32).view(B, K); o += n
  pred_mask = packed[o:o + n].view(torch.int32).view(B, K)
  heading_class = torch.empty((B, K), dtype=torch.int32, device=dev)
  size_class = torch.empty((B, K), dtype=torch.int32, device=dev)
  params = torch.empty((B, K, 7), dtype=torch.float32, device=dev)
  minmax = torch.empty((B, K, 6), dtype=torch.float32, device=dev)
  st = cur_stream(dev)
  check(lib.pcmi_box_decode(ptr(c), ptr(hs), ptr(hr), ptr(ss), ptr(sr), ptr(sem), ptr(obj), ptr(msa), B, K, H, S, Cls,
                            int(bool(zero_heading)), ptr(heading_class), ptr(size_class), ptr(sem_cls), ptr(params), ptr(corners),
                            ptr(minmax), ptr(obj_prob), ptr(sem_probs), st))
  counts = None
  if with_counts_of is not None:
    pts = _f32c(with_counts_of, who)
    assert pts.dim() == 3 and pts.shape[0] == B and pts.shape[2] >= 3, "box_decode: point_clouds [B, N, >= 3]"
    counts = torch.empty((B, K), dtype=torch.int32, device=dev)
    check(lib.pcmi_box_point_counts(ptr(pts), pts.shape[2], ptr(params), B, pts.shape[1], K, ptr(counts), st))
  if nms is not None:
    mode, old_type, nms_iou = nms
    check(lib.pcmi_box_nms(ptr(minmax), ptr(obj_prob), ptr(sem_cls), ptr(counts), int(min_points), B, K, int(mode), int(bool(old_type)),
                           float(nms_iou), ptr(pred_mask), st))
  return dict(heading_class=heading_class, size_class=size_class, sem_cls=sem_cls, box_params=params, corners=corners, minmax=minmax,
              obj_prob=obj_prob, sem_cls_probs=sem_probs, counts=counts, pred_mask=pred_mask if nms is not None else None,
              packed=packed)


# ---------------------------------------------------------------------------------------------------------------------
# Detection scoring (csrc/evaldet.hip): box3d_iou of downstream/votenet_det_new/lib/utils/box_util.py and eval_det_cls /
# voc_ap of lib/utils/eval_det.py.
# ---------------------------------------------------------------------------------------------------------------------
DET_MATCH_MAX_K = 1024  # kMatchMaxK / kMatchMaxG of evaldet.hip
DET_MATCH_MAX_G = 256
DET_AP_MAX_THRESHOLDS = 16


def box3d_iou(corners1, corners2, with_2d=True):
  """corners1 [n, 8, 3], corners2 [m, 8, 3] in get_3d_box's corner order -> (iou3d [n, m], iou2d [n, m] or None): the oriented
  overlap of every pair (pcmi_box3d_iou), float32, one launch."""
  a, b = _f32c(corners1, "box3d_iou"), _f32c(corners2, "box3d_iou")
  assert a.dim() == 3 and b.dim() == 3 and a.shape[1:] == (8, 3) and b.shape[1:] == (8, 3), "box3d_iou: corners [n, 8, 3] and [m, 8, 3]"
  n, m = a.shape[0], b.shape[0]
  iou3d = torch.empty((n, m), dtype=torch.float32, device=a.device)
  iou2d = torch.empty((n, m), dtype=torch.float32, device=a.device) if with_2d else None
  check(lib.pcmi_box3d_iou(ptr(a), ptr(b), n, m, ptr(iou3d), ptr(iou2d), cur_stream(a.device)))
  return iou3d, iou2d


def det_match(pred_corners, gt_corners, gt_cls, gt_mask, num_class):
  """pred_corners [B, K, 8, 3], gt_corners [B, G, 8, 3], gt_cls [B, G], gt_mask [B, G] (nonzero: a box) -> (best_gt int32
  [B, K, num_class], best_iou float32 [B, K, num_class]): per predicted box and class the scene's ground-truth box of that
  class it overlaps most (the lowest index of equal overlaps; -1 / -inf without one).  pcmi_det_match, one launch."""
  p, g = _f32c(pred_corners, "det_match"), _f32c(gt_corners, "det_match")
  assert p.dim() == 4 and g.dim() == 4 and p.shape[2:] == (8, 3) and g.shape[2:] == (8, 3) and p.shape[0] == g.shape[0], \
      "det_match: pred_corners [B, K, 8, 3], gt_corners [B, G, 8, 3]"
  B, K, G = p.shape[0], p.shape[1], g.shape[1]
  assert gt_cls.shape == (B, G) and gt_mask.shape == (B, G), "det_match: gt_cls / gt_mask [B, G]"
  cls = _i32c(gt_cls, p.device)
  mask = (gt_mask.to(p.device) != 0).to(torch.int32).contiguous()
  best_gt = torch.empty((B, K, int(num_class)), dtype=torch.int32, device=p.device)
  best_iou = torch.empty((B, K, int(num_class)), dtype=torch.float32, device=p.device)
  check(lib.pcmi_det_match(ptr(p), ptr(g), ptr(cls), ptr(mask), B, K, G, int(num_class), ptr(best_gt), ptr(best_iou),
                           cur_stream(p.device)))
  return best_gt, best_iou


def det_ap(best_iou, gt_id, cls_offs, npos, n_gt, thresholds, use_07_metric=False, curves=False):
  """pcmi_det_ap.  best_iou float32 [nd] / gt_id int32 [nd]: the detections class by class in descending confidence, class c at
  [cls_offs[c], cls_offs[c + 1]) (int32 [Cls + 1]); npos int32 [Cls]; n_gt: ground-truth boxes gt_id indexes; thresholds: a
  sequence of floats (host).  Returns a dict of device tensors: ap, last_rec (float64 [T, Cls]) and, with curves, rec, prec
  (float64 [T, nd]) and tp (int32 [T, nd]).  No host synchronisation."""
  iou = _f32c(best_iou, "det_ap").reshape(-1)
  dev = iou.device
  gid, offs, np_ = _i32c(gt_id, dev).reshape(-1), _i32c(cls_offs, dev), _i32c(npos, dev)
  nd, Cls, T = iou.shape[0], np_.shape[0], len(thresholds)
  assert gid.shape[0] == nd and offs.shape == (Cls + 1,), "det_ap: gt_id [nd], cls_offs [Cls + 1], npos [Cls]"
  thr = (C.c_double * max(T, 1))(*[float(t) for t in thresholds])
  ap = torch.empty((T, Cls), dtype=torch.float64, device=dev)
  last_rec = torch.empty((T, Cls), dtype=torch.float64, device=dev)
  rec = prec = tp = None
  if curves:
    rec = torch.empty((T, nd), dtype=torch.float64, device=dev)
    prec = torch.empty((T, nd), dtype=torch.float64, device=dev)
    tp = torch.empty((T, nd), dtype=torch.int32, device=dev)
  ws, wsb = ws_args(lib.pcmi_det_ap_workspace_bytes(nd, int(n_gt), T), dev)
  check(lib.pcmi_det_ap(ptr(iou), ptr(gid), ptr(offs), ptr(np_), nd, int(n_gt), Cls, thr, T, int(bool(use_07_metric)), ptr(ap),
                        ptr(last_rec), ptr(rec), ptr(prec), ptr(tp), ws, wsb, cur_stream(dev)))
  return dict(ap=ap, last_rec=last_rec, rec=rec, prec=prec, tp=tp)


# ---------------------------------------------------------------------------------------------------------------------
# Segmentation validation (csrc/segeval.hip): the per-batch work of downstream/semseg/lib/test.py:119,137-145.
# ---------------------------------------------------------------------------------------------------------------------
SEG_EVAL_MAX_CLASSES = 64  # kMaxClasses of segeval.hip


def seg_eval_rows(logits, target, ignore_label, hist=None, want_prob=True, totals=None):
  """pcmi_seg_eval_rows.  logits float32 [n, c] (rows may be a column slice), target [n] -> a dict of device tensors: pred
  int32 [n] (arg-max, the lowest class of equal logits), prob_t float32 [c, n] (class-major softmax; None without want_prob),
  hist int64 [c, c] (the confusion matrix ADDED to the one passed in, a fresh one otherwise) and batch float64 [4] = (sum of the
  counted rows' losses, counted rows, correct among them, n).  totals float64 [3] (optional) accumulates the reference's two
  AverageMeters and their count.  No host synchronisation."""
  require_cuda(logits, "seg_eval_rows")
  x = logits if (logits.stride(1) == 1 and logits.dtype == torch.float32) else logits.float().contiguous()
  assert x.dim() == 2 and x.shape[1] >= 1, "seg_eval_rows: logits [n, c]"
  n, c = x.shape
  dev = x.device
  lb = _i32c(target, dev).reshape(-1)
  assert lb.shape[0] == n, "seg_eval_rows: target [n]"
  if hist is None:
    hist = torch.zeros((c, c), dtype=torch.int64, device=dev)
  assert hist.shape == (c, c) and hist.dtype == torch.int64 and hist.is_contiguous() and hist.device == dev, \
      "seg_eval_rows: hist int64 [c, c] on the logits' device"
  assert totals is None or (totals.shape == (3,) and totals.dtype == torch.float64 and totals.device == dev), \
      "seg_eval_rows: totals float64 [3] on the logits' device"
  pred = torch.empty(n, dtype=torch.int32, device=dev)
  prob_t = torch.empty((c, n), dtype=torch.float32, device=dev) if want_prob else None
  batch = torch.zeros(4, dtype=torch.float64, device=dev)
  ws, wsb = ws_args(lib.pcmi_seg_eval_rows_workspace_bytes(n), dev)
  check(lib.pcmi_seg_eval_rows(ptr(x), x.stride(0) if n else c, n, c, ptr(lb), int(ignore_label), ptr(pred), ptr(prob_t), ptr(hist),
                               ptr(batch), ptr(totals), ws, wsb, cur_stream(dev)))
  return dict(pred=pred, prob_t=prob_t, hist=hist, batch=batch)


def seg_average_precision(prob_t, target, ap_sum=None, ap_cnt=None):
  """average_precision(prob, target) of downstream/semseg/lib/test.py:55-59 for class-major scores prob_t float32 [c, n] and
  target [n]: a torch.sort per class on the device, then pcmi_seg_ap.  Returns ap float64 [c] on the device (NaN for a class
  without a positive row); ap_sum float64 [c] / ap_cnt int64 [c] (optional) accumulate the values that are not NaN.  No host
  synchronisation."""
  p = _f32c(prob_t, "seg_average_precision")
  assert p.dim() == 2, "seg_average_precision: prob_t [c, n]"
  c, n = p.shape
  dev = p.device
  lb = _i32c(target, dev).reshape(-1)
  assert lb.shape[0] == n, "seg_average_precision: target [n]"
  assert ap_sum is None or (ap_sum.shape == (c,) and ap_sum.dtype == torch.float64 and ap_sum.device == dev), "ap_sum float64 [c]"
  assert ap_cnt is None or (ap_cnt.shape == (c,) and ap_cnt.dtype == torch.int64 and ap_cnt.device == dev), "ap_cnt int64 [c]"
  sorted_prob, order = torch.sort(p, dim=1, descending=True)
  return seg_ap_sorted(sorted_prob, order, lb, ap_sum, ap_cnt)


def seg_ap_sorted(sorted_prob, order, target, ap_sum=None, ap_cnt=None):
  """pcmi_seg_ap on scores that are sorted already: sorted_prob float32 [c, n] descending along n, order int64 [c, n] the row
  of each sorted element, target int32 [n]."""
  s, o = _f32c(sorted_prob, "seg_ap"), order.to(torch.int64).contiguous()
  c, n = s.shape
  dev = s.device
  lb = _i32c(target, dev).reshape(-1)
  assert o.shape == (c, n) and o.device == dev and lb.shape[0] == n, "seg_ap: sorted_prob / order [c, n], target [n]"
  ap = torch.empty(c, dtype=torch.float64, device=dev)
  ws, wsb = ws_args(lib.pcmi_seg_ap_workspace_bytes(c), dev)
  check(lib.pcmi_seg_ap(ptr(s), ptr(o), ptr(lb), n, c, ptr(ap), ptr(ap_sum), ptr(ap_cnt), ws, wsb, cur_stream(dev)))
  return ap


# ---------------------------------------------------------------------------------------------------------------------
# Evaluation on the original point cloud (csrc/nearest.hip): save_predictions + dataset.test_pointcloud of the reference
# (downstream/semseg/lib/utils.py:304-344, lib/datasets/scannet.py:131-171).  None of these is differentiable.
# ---------------------------------------------------------------------------------------------------------------------
def _f64c(t, device, who):
  t = torch.as_tensor(t)
  assert t.dtype == torch.float64, "%s: float64 (the evaluation geometry is not rounded to float32)" % who
  return t.to(device).contiguous()


def _offsets(offsets, device):
  return torch.as_tensor(offsets).to(device=device, dtype=torch.int64).contiguous()


def voxel_centers(coords, transformation):
  """pcmi_voxel_centers.  coords int32 [n, 4] on the device in (b, x, y, z) order; transformation: the [B, 16] (or [B, 4, 4])
  voxelizer matrices as the loader returns them, on the HOST -- each is inverted here in float64 (np.linalg.inv,
  lib/utils.py:325-327).  Returns centers float64 [n, 3] = inv(T[b]) (x + 0.5, y + 0.5, z + 0.5, 1); a row whose batch index is
  outside [0, B) is NaN.  No synchronisation."""
  import numpy as np
  require_cuda(coords, "voxel_centers")
  assert coords.dim() == 2 and coords.shape[1] == 4, "voxel_centers: coords [n, 4]"
  c = coords.to(torch.int32).contiguous()
  T = np.asarray(transformation.cpu() if torch.is_tensor(transformation) else transformation, dtype=np.float64)
  T = (T[:, :16] if T.ndim == 2 else T.reshape(-1, 16)).reshape(-1, 4, 4)  # (transformation[i, :16], lib/utils.py:325)
  inv = np.ascontiguousarray(np.linalg.inv(T)).reshape(-1)
  B = T.shape[0]
  assert B >= 1, "voxel_centers: at least one transformation"
  out = torch.empty((c.shape[0], 3), dtype=torch.float64, device=c.device)
  check(lib.pcmi_voxel_centers(ptr(c), c.shape[0], inv.ctypes.data_as(C.POINTER(C.c_double)), B, ptr(out), cur_stream(c.device)))
  return out


def default_cell(ref, n_scenes):
  """The cell size nearest_point uses when it is given none, as a device tensor float64 [1] (nothing is read back): twice the
  spacing of m / B points spread over a square of the references' largest extent L -- 2 L / sqrt(m / B).  Voxel centres of
  a scan lie on surfaces, for which this is about two voxels; at least L 2^-15, so that every cell index fits the grid key.
  It is a guess that only costs time: the result does not depend on the cell size."""
  m = ref.shape[0]
  if m == 0:
    return torch.ones(1, dtype=torch.float64, device=ref.device)
  r = torch.nan_to_num(ref, nan=0.0, posinf=0.0, neginf=0.0)
  L = (r.amax(0) - r.amin(0)).amax()
  cell = torch.clamp(2.0 * L / (max(m / max(int(n_scenes), 1), 1.0) ** 0.5), min=L * 2.0 ** -15)
  return torch.where(cell > 0, cell, torch.ones_like(cell)).reshape(1)


def nearest_point(ref, ref_offsets, query, query_offsets, cell=None, return_dist2=False, fallback_count=None):
  """pcmi_nearest_point: the exact nearest reference row of every query row, scene by scene.  ref float64 [m, 3] with
  ref_offsets [B + 1], query float64 [n, 3] with query_offsets [B + 1] (ascending row offsets of the scenes).  Returns idx
  int32 [n], the GLOBAL row of ref minimising (dx dx + dy dy) + dz dz in float64, the lowest row among equal distances; -1 for
  a scene without references and for a non-finite query row; with return_dist2 also dist2 float64 [n] (+inf / NaN there).
  cell: the side of the binning cells -- 2 x voxel_size for voxel centres; None: default_cell(ref, B), computed on the
  device.  It changes the time only, never the result.  fallback_count int64 [1] (optional) += the queries that needed the
  whole-segment scan.  No host synchronisation."""
  require_cuda(query, "nearest_point")
  dev = query.device
  q, r = _f64c(query, dev, "nearest_point"), _f64c(ref, dev, "nearest_point")
  ro, qo = _offsets(ref_offsets, dev), _offsets(query_offsets, dev)
  assert q.dim() == 2 and q.shape[1] == 3 and r.dim() == 2 and r.shape[1] == 3, "nearest_point: ref [m, 3], query [n, 3]"
  assert ro.dim() == 1 and ro.shape == qo.shape and ro.shape[0] >= 2, "nearest_point: offsets [B + 1]"
  m, n, B = r.shape[0], q.shape[0], ro.shape[0] - 1
  cell_dev = None
  if cell is None:
    cell_dev, cell = default_cell(r, B), 0.0
  elif torch.is_tensor(cell):
    cell_dev, cell = cell.to(device=dev, dtype=torch.float64).reshape(1).contiguous(), 0.0
  assert fallback_count is None or (fallback_count.dtype == torch.int64 and fallback_count.numel() == 1 and
                                    fallback_count.device == dev), "nearest_point: fallback_count int64 [1]"
  idx = torch.empty(n, dtype=torch.int32, device=dev)
  dist2 = torch.empty(n, dtype=torch.float64, device=dev) if return_dist2 else None
  ws, wsb = ws_args(lib.pcmi_nearest_point_workspace_bytes(m, n, B), dev)
  check(lib.pcmi_nearest_point(ptr(r), ptr(ro), m, ptr(q), ptr(qo), n, B, float(cell), ptr(cell_dev), ptr(idx), ptr(dist2),
                               ptr(fallback_count), ws, wsb, cur_stream(dev)))
  return (idx, dist2) if return_dist2 else idx


def seg_hist(pred, idx, labels, num_labels, hist=None, missing=None, want_point_pred=True):
  """pcmi_seg_hist: fast_hist(pred[idx], labels) on the device.  pred [m], idx int32 [n] (None: identity), labels [n] -> a dict
  of device tensors: hist int64 [c, c] (ADDED to the one passed in, a fresh one otherwise) counting the rows with 0 <= label
  < c, 0 <= idx < m and 0 <= pred[idx] < c at [label, pred[idx]]; point_pred int32 [n] = pred[idx], -1 where idx is outside
  [0, m) (None without want_point_pred); missing int64 [1] += the number of such rows.  No host synchronisation."""
  require_cuda(pred, "seg_hist")
  dev = pred.device
  p, lb = _i32c(pred, dev).reshape(-1), _i32c(labels, dev).reshape(-1)
  ix = None if idx is None else _i32c(idx, dev).reshape(-1)
  m, n, c = p.shape[0], lb.shape[0], int(num_labels)
  assert ix is None or ix.shape[0] == n, "seg_hist: idx [n], labels [n]"
  if hist is None:
    hist = torch.zeros((c, c), dtype=torch.int64, device=dev)
  assert hist.shape == (c, c) and hist.dtype == torch.int64 and hist.is_contiguous() and hist.device == dev, \
      "seg_hist: hist int64 [c, c] on pred's device"
  if missing is None:
    missing = torch.zeros(1, dtype=torch.int64, device=dev)
  assert missing.dtype == torch.int64 and missing.numel() == 1 and missing.device == dev, "seg_hist: missing int64 [1]"
  point_pred = torch.empty(n, dtype=torch.int32, device=dev) if want_point_pred else None
  check(lib.pcmi_seg_hist(ptr(p), m, ptr(ix), ptr(lb), n, c, ptr(hist), ptr(point_pred), ptr(missing), cur_stream(dev)))
  return dict(hist=hist, point_pred=point_pred, missing=missing)


# ---------------------------------------------------------------------------------------------------------------------
# The input of segmentation fine-tuning (csrc/semseg_input.hip): Voxelizer.voxelize with sparse_quantize and the voxel-space
# augmentations of the reference (downstream/semseg/lib/voxelizer.py, lib/transforms.py) for a batch of scans.  None of these
# is differentiable and none synchronises; errors arrive in `flags` (int32 [B], SEG_FLAG_* bits per scene).
# ---------------------------------------------------------------------------------------------------------------------
SEG_FLAG_RANGE, SEG_FLAG_SPAN, SEG_FLAG_ELASTIC, SEG_FLAG_CROP = 1, 2, 4, 8
SEG_FLAG_NAMES = {SEG_FLAG_RANGE: "a point is not finite or its voxel coordinate is outside +-2^20",
                  SEG_FLAG_SPAN: "a voxel coordinate lies 2^18 or more above the scene's minimum",
                  SEG_FLAG_ELASTIC: "the elastic noise grid does not fit its capacity block",
                  SEG_FLAG_CROP: "no step of the crop ladder brings the scene within max_voxels (it has the last step's window)"}


def seg_flags_message(flags_host):
  """The exception text for a read-back flags array (None if no bit is set): every flagged scene with its causes."""
  bad = ["scene %d: %s" % (b, "; ".join(t for bit, t in SEG_FLAG_NAMES.items() if int(f) & bit) or "flag %d" % int(f))
         for b, f in enumerate(flags_host) if int(f)]
  return "segmentation input: " + " | ".join(bad) if bad else None


def _seg_flags(flags, B, dev):
  if flags is None:
    return torch.zeros(B, dtype=torch.int32, device=dev)
  assert flags.dtype == torch.int32 and flags.shape == (B,) and flags.device == dev and flags.is_contiguous(), "flags: int32 [B]"
  return flags


def _elastic_args(xyz, offsets, noise, what):
  require_cuda(xyz, what)
  dev = xyz.device
  assert xyz.dtype == torch.float64 and xyz.dim() == 2 and xyz.shape[1] == 3 and xyz.is_contiguous(), \
      what + ": xyz float64 [n, 3], contiguous (changed in place)"
  offs = _offsets(offsets, dev)
  B = offs.shape[0] - 1
  assert noise.dtype == torch.float32 and noise.dim() == 5 and noise.shape[0] == B and noise.shape[4] == 3 and \
      noise.is_contiguous() and noise.device == dev, what + ": noise float32 [B, cx, cy, cz, 3] on xyz's device, contiguous"
  return dev, offs, B


def elastic_blur(xyz, offsets, granularity, noise, active=None, flags=None):
  """pcmi_elastic_blur: the noise grids of one elastic stage from the scenes' current extents, smoothed IN PLACE in noise
  float32 [B, cx, cy, cz, 3] (each scene's [dx, dy, dz, 3] volume in the corner of its capacity block).  active int32 [B]
  (None: all).  Returns a dict: grid_dims int32 [B, 4] (dx, dy, dz, on), grid_min float64 [B, 3], flags int32 [B]."""
  dev, offs, B = _elastic_args(xyz, offsets, noise, "elastic_blur")
  act = None if active is None else _i32c(torch.as_tensor(active), dev).reshape(-1)
  assert act is None or act.shape[0] == B, "elastic_blur: active [B]"
  flags = _seg_flags(flags, B, dev)
  cx, cy, cz = (int(v) for v in noise.shape[1:4])
  grid_dims = torch.empty((B, 4), dtype=torch.int32, device=dev)
  grid_min = torch.empty((B, 3), dtype=torch.float64, device=dev)
  ws, wsb = ws_args(lib.pcmi_elastic_blur_workspace_bytes(B, cx, cy, cz), dev)
  check(lib.pcmi_elastic_blur(ptr(xyz), ptr(offs), xyz.shape[0], B, float(granularity), ptr(act), ptr(noise), cx, cy, cz,
                              ptr(grid_dims), ptr(grid_min), ptr(flags), ws, wsb, cur_stream(dev)))
  return dict(grid_dims=grid_dims, grid_min=grid_min, flags=flags)


def elastic_apply(xyz, offsets, granularity, magnitude, noise, grid):
  """pcmi_elastic_apply: xyz += trilinear(noise)(xyz) * magnitude IN PLACE for the scenes that elastic_blur switched on
  (grid: its result)."""
  dev, offs, B = _elastic_args(xyz, offsets, noise, "elastic_apply")
  cx, cy, cz = (int(v) for v in noise.shape[1:4])
  check(lib.pcmi_elastic_apply(ptr(xyz), ptr(offs), xyz.shape[0], B, float(granularity), float(magnitude), ptr(noise), cx, cy, cz,
                               ptr(grid["grid_dims"]), ptr(grid["grid_min"]), cur_stream(dev)))
  return xyz


def seg_transform(xyz, offsets, mats, clip_bound=None, trans_ratio=None, flags=None):
  """pcmi_seg_transform.  xyz float64 [n, 3] and offsets [B + 1] (the scenes' row offsets), mats float64 [B, 16] or [B, 4, 4]
  (host or device).  clip_bound: None, a number, or ((lo, hi),) * 3 as Voxelizer.clip_bound; trans_ratio float64 [B, 3]
  (None: 0).  Returns a dict of device tensors: vox int32 [n, 3], keep uint8 [n], scene_min int32 [B, 3], aligned float64
  [B, 16] and flags int32 [B] (ORed into the one passed in)."""
  require_cuda(xyz, "seg_transform")
  dev = xyz.device
  x, offs = _f64c(xyz, dev, "seg_transform"), _offsets(offsets, dev)
  assert x.dim() == 2 and x.shape[1] == 3 and offs.dim() == 1 and offs.shape[0] >= 2, "seg_transform: xyz [n, 3], offsets [B + 1]"
  n, B = x.shape[0], offs.shape[0] - 1
  M = _f64c(mats, dev, "seg_transform").reshape(-1, 16)
  assert M.shape[0] == B, "seg_transform: one matrix per scene"
  tr = None if trans_ratio is None else _f64c(trans_ratio, dev, "seg_transform").reshape(-1, 3)
  assert tr is None or tr.shape[0] == B, "seg_transform: trans_ratio [B, 3]"
  if clip_bound is None:
    mode, lim = 0, (C.c_double * 6)()
  elif isinstance(clip_bound, (int, float)):
    mode, lim = 1, (C.c_double * 6)(float(clip_bound))
  else:
    mode, lim = 2, (C.c_double * 6)(*[float(v) for pair in clip_bound for v in pair])
  flags = _seg_flags(flags, B, dev)
  vox = torch.empty((n, 3), dtype=torch.int32, device=dev)
  keep = torch.empty(n, dtype=torch.uint8, device=dev)
  scene_min = torch.empty((B, 3), dtype=torch.int32, device=dev)
  aligned = torch.empty((B, 16), dtype=torch.float64, device=dev)
  ws, wsb = ws_args(lib.pcmi_seg_transform_workspace_bytes(B), dev)
  check(lib.pcmi_seg_transform(ptr(x), ptr(offs), n, B, ptr(M), mode, lim, ptr(tr), ptr(vox), ptr(keep), ptr(scene_min),
                               ptr(aligned), ptr(flags), ws, wsb, cur_stream(dev)))
  return dict(vox=vox, keep=keep, scene_min=scene_min, aligned=aligned, flags=flags)


def seg_quantize(vox, offsets, labels=None, keep=None, scene_min=None, ignore_label=255, flags=None):
  """pcmi_seg_quantize: ME.utils.sparse_quantize with labels for a batch.  vox int32 [n, 3], offsets [B + 1], labels [n],
  keep uint8 [n] (None: all), scene_min int32 [B, 3] (None: 0).  Returns a dict of device tensors whose first counts[B] rows
  are valid -- coords int32 [n, 4] (b, x - min, ...), index int64 [n], labels int32 [n] (None without labels) -- and counts
  int64 [B + 1] (voxels per scene, then their sum), flags int32 [B].  Nothing is read back: slice after reading counts."""
  require_cuda(vox, "seg_quantize")
  dev = vox.device
  v, offs = _i32c(vox, dev), _offsets(offsets, dev)
  assert v.dim() == 2 and v.shape[1] == 3 and offs.dim() == 1 and offs.shape[0] >= 2, "seg_quantize: vox [n, 3], offsets [B + 1]"
  n, B = v.shape[0], offs.shape[0] - 1
  lb = None if labels is None else _i32c(labels, dev).reshape(-1)
  kp = None if keep is None else keep.to(device=dev, dtype=torch.uint8).contiguous()
  mn = None if scene_min is None else _i32c(scene_min, dev).reshape(-1, 3)
  assert (lb is None or lb.shape[0] == n) and (kp is None or kp.shape == (n,)) and (mn is None or mn.shape[0] == B), \
      "seg_quantize: labels [n], keep [n], scene_min [B, 3]"
  flags = _seg_flags(flags, B, dev)
  coords = torch.empty((n, 4), dtype=torch.int32, device=dev)
  index = torch.empty(n, dtype=torch.int64, device=dev)
  out_labels = None if lb is None else torch.empty(n, dtype=torch.int32, device=dev)
  counts = torch.empty(B + 1, dtype=torch.int64, device=dev)
  ws, wsb = ws_args(lib.pcmi_seg_quantize_workspace_bytes(n), dev)
  check(lib.pcmi_seg_quantize(ptr(v), ptr(kp), ptr(lb), ptr(offs), ptr(mn), n, B, int(ignore_label), ptr(coords), ptr(index),
                              ptr(out_labels), ptr(counts), ptr(flags), ws, wsb, cur_stream(dev)))
  return dict(coords=coords, index=index, labels=out_labels, counts=counts, flags=flags)


def seg_color_params(B, flip=None, contrast=None, translation=None, jitter_std=None):
  """The [B, 12] float64 parameter block of seg_color_augment on the host (numpy).  Per scene (each a length-B sequence, an
  entry None = that transform is off): flip (fx, fy, fz) booleans; contrast = the blend factor; translation = (tr_r, tr_g,
  tr_b), already scaled to colour units; jitter_std = std (the noise is normal * std * 255)."""
  import numpy as np
  P = np.zeros((B, 12), dtype=np.float64)
  for b in range(B):
    if flip is not None and flip[b] is not None:
      P[b, 0:3] = [1.0 if f else 0.0 for f in flip[b]]
    if contrast is not None and contrast[b] is not None:
      P[b, 3], P[b, 4] = 1.0, float(contrast[b])
    if translation is not None and translation[b] is not None:
      P[b, 5], P[b, 6:9] = 1.0, np.asarray(translation[b], dtype=np.float64).reshape(3)
    if jitter_std is not None and jitter_std[b] is not None:
      P[b, 9], P[b, 10] = 1.0, float(jitter_std[b]) * 255
  return P


def seg_color_augment(feats_src, coords, n_scenes, index=None, labels=None, params=None, normals=None, normalize=False,
                      label_lut=None, ignore_label=255):
  """pcmi_seg_color_augment over the m voxel rows.  feats_src float32 [n_src, 3], read at index int64 [m] (None: the row
  itself); coords int32 [m, 4] and labels int32 [m] are changed IN PLACE (flip; label map) and must be contiguous device
  tensors; params float64 [B, 12] (seg_color_params; None: no augmentation); normals float32 [m, 3]; label_lut int32 [L].
  Returns feats float32 [m, 3]."""
  require_cuda(coords, "seg_color_augment")
  dev = coords.device
  assert coords.dtype == torch.int32 and coords.dim() == 2 and coords.shape[1] == 4 and coords.is_contiguous(), \
      "seg_color_augment: coords int32 [m, 4], contiguous (changed in place)"
  assert labels is None or (labels.dtype == torch.int32 and labels.is_contiguous() and labels.device == dev and
                            labels.shape == (coords.shape[0],)), "seg_color_augment: labels int32 [m] on the device (changed in place)"
  m, B = coords.shape[0], int(n_scenes)
  src = _f32c(torch.as_tensor(feats_src).to(dev), "seg_color_augment")
  assert src.dim() == 2 and src.shape[1] == 3, "seg_color_augment: feats_src [n_src, 3]"
  ix = None if index is None else index.to(device=dev, dtype=torch.int64).contiguous()
  assert ix is None or ix.shape == (m,), "seg_color_augment: index [m]"
  P = None if params is None else _f64c(params, dev, "seg_color_augment").reshape(-1, 12)
  assert P is None or P.shape[0] == B, "seg_color_augment: params [B, 12]"
  nm = None if normals is None else _f32c(normals.to(dev), "seg_color_augment")
  assert nm is None or nm.shape == (m, 3), "seg_color_augment: normals [m, 3]"
  lut = None if label_lut is None else _i32c(torch.as_tensor(label_lut), dev).reshape(-1)
  out = torch.empty((m, 3), dtype=torch.float32, device=dev)
  ws, wsb = ws_args(lib.pcmi_seg_color_augment_workspace_bytes(B), dev)
  check(lib.pcmi_seg_color_augment(ptr(src), src.shape[0], ptr(ix), ptr(coords), ptr(labels), m, B, ptr(P), ptr(nm),
                                   1 if normalize else 0, ptr(lut), 0 if lut is None else lut.shape[0], int(ignore_label),
                                   ptr(out), ws, wsb, cur_stream(dev)))
  return out


# ---------------------------------------------------------------------------------------------------------------------
# The input of contrastive pre-training (csrc/pair_input.hip): ScanNetMatchPairDataset.__getitem__ and default_collate_pair_fn
# of the reference (pretrain/pointcontrast/lib/ddp_data_loaders.py) for a batch of B pairs = 2 B clouds.  None of these is
# differentiable and none synchronises; errors arrive in `flags` (int32 [B], PAIR_FLAG_* bits per pair).
# ---------------------------------------------------------------------------------------------------------------------
PAIR_FLAG_NONFINITE, PAIR_FLAG_RANGE, PAIR_FLAG_MATCHES = 1, 2, 4
PAIR_FLAG_NAMES = {PAIR_FLAG_NONFINITE: "a point is not finite (raw, after its transform or after trans)",
                   PAIR_FLAG_RANGE: "a voxel or search-cell index is outside +-(2^20 - 1)",
                   PAIR_FLAG_MATCHES: "a source point has more than 96 matches (is the search radius far above the voxel size?)"}
PAIR_MAX_PAIRS = 512  # PCMI_PAIR_MAX_PAIRS


def pair_flags_message(flags_host):
  """The exception text for a read-back flags array (None if no bit is set): every flagged pair with its causes."""
  bad = ["pair %d: %s" % (b, "; ".join(t for bit, t in PAIR_FLAG_NAMES.items() if int(f) & bit) or "flag %d" % int(f))
         for b, f in enumerate(flags_host) if int(f)]
  return "pre-training input: " + " | ".join(bad) if bad else None


def _pair_offsets(offsets, dev, who):
  offs = _offsets(offsets, dev)
  assert offs.dim() == 1 and offs.shape[0] >= 3 and offs.shape[0] % 2 == 1, who + ": offsets [2 B + 1]"
  return offs, (offs.shape[0] - 1) // 2


def pair_transform(raw, offsets, scale, rot=None, flags=None):
  """pcmi_pair_transform.  raw float32 or float64 [n, 3] (the clouds of the batch, pair b = clouds 2 b and 2 b + 1), offsets
  [2 B + 1], scale float64 [B], rot float64 [2 B, 3, 3] or [2 B, 9] (None: no rotation and no centring, T = trans = I).  Returns
  a dict of device tensors: points float64 [n, 3], T float64 [2 B, 4, 4], trans float64 [B, 4, 4], flags int32 [B] (ORed into the
  one passed in)."""
  require_cuda(raw, "pair_transform")
  dev = raw.device
  assert raw.dtype in (torch.float32, torch.float64) and raw.dim() == 2 and raw.shape[1] == 3, "pair_transform: raw float32 / float64 [n, 3]"
  x = raw.contiguous()
  offs, B = _pair_offsets(offsets, dev, "pair_transform")
  sc = _f64c(scale, dev, "pair_transform").reshape(-1)
  R = None if rot is None else _f64c(rot, dev, "pair_transform").reshape(-1, 9)
  assert sc.shape[0] == B and (R is None or R.shape[0] == 2 * B), "pair_transform: scale [B], rot [2 B, 3, 3]"
  flags = _seg_flags(flags, B, dev)
  n = x.shape[0]
  points = torch.empty((n, 3), dtype=torch.float64, device=dev)
  T = torch.empty((2 * B, 4, 4), dtype=torch.float64, device=dev)
  trans = torch.empty((B, 4, 4), dtype=torch.float64, device=dev)
  ws, wsb = ws_args(lib.pcmi_pair_transform_workspace_bytes(n, B), dev)
  check(lib.pcmi_pair_transform(ptr(x), 1 if x.dtype == torch.float32 else 0, ptr(offs), n, B, ptr(sc), ptr(R), 0 if R is None else 1,
                                ptr(points), ptr(T), ptr(trans), ptr(flags), ws, wsb, cur_stream(dev)))
  return dict(points=points, T=T, trans=trans, flags=flags)


def pair_voxelize(points, offsets, voxel_size, flags=None):
  """pcmi_pair_voxelize: the first point of every occupied voxel of every cloud, in ascending row order.  points float64 [n, 3],
  offsets [2 B + 1].  Returns a dict of device tensors whose first vox_offsets[2 B] rows are valid -- points float64 [n, 3],
  coords int32 [n, 3], first_index int32 [n] (batch rows) -- and n_vox int64 [2 B], vox_offsets int64 [2 B + 1], side_offsets
  int64 [2, B + 1], flags int32 [B].  Nothing is read back: slice after reading the counts."""
  require_cuda(points, "pair_voxelize")
  dev = points.device
  p = _f64c(points, dev, "pair_voxelize")
  assert p.dim() == 2 and p.shape[1] == 3, "pair_voxelize: points [n, 3]"
  offs, B = _pair_offsets(offsets, dev, "pair_voxelize")
  flags = _seg_flags(flags, B, dev)
  n = p.shape[0]
  out = torch.empty((n, 3), dtype=torch.float64, device=dev)
  coords = torch.empty((n, 3), dtype=torch.int32, device=dev)
  first = torch.empty(n, dtype=torch.int32, device=dev)
  n_vox = torch.empty(2 * B, dtype=torch.int64, device=dev)
  voff = torch.empty(2 * B + 1, dtype=torch.int64, device=dev)
  side = torch.empty((2, B + 1), dtype=torch.int64, device=dev)
  ws, wsb = ws_args(lib.pcmi_pair_voxelize_workspace_bytes(n, B), dev)
  check(lib.pcmi_pair_voxelize(ptr(p), ptr(offs), n, B, float(voxel_size), ptr(out), ptr(coords), ptr(first), ptr(n_vox), ptr(voff),
                               ptr(side), ptr(flags), ws, wsb, cur_stream(dev)))
  return dict(points=out, coords=coords, first_index=first, n_vox=n_vox, vox_offsets=voff, side_offsets=side, flags=flags)


def pair_match(vox, trans, radius, capacity, flags=None, pairs=None, fill_only=False):
  """pcmi_pair_match on pair_voxelize's result `vox`: trans float64 [B, 4, 4], radius float64 [B], room for `capacity` rows
  (in `pairs`, int32 [>= capacity, 2], if given).
  Returns a dict of device tensors: pairs int32 [capacity, 2] (the first totals[0] rows are valid unless totals[2] is set: then
  nothing was written, call again with capacity >= totals[0]), pair_counts int64 [B], totals int64 [4] (rows needed, n_queries,
  overflow, capacity), flags int32 [B].  Nothing is read back.  fill_only: the second call after an overflow -- only the fill
  runs, on what the first call left in the shared workspace (no other op may have used the workspace in between), with the
  flags tensor of that call."""
  pts = vox["points"]
  require_cuda(pts, "pair_match")
  dev = pts.device
  voff, side = vox["vox_offsets"], vox["side_offsets"]
  B = side.shape[1] - 1
  tr = _f64c(trans, dev, "pair_match").reshape(-1, 16)
  rd = _f64c(radius, dev, "pair_match").reshape(-1)
  assert tr.shape[0] == B and rd.shape[0] == B and voff.shape[0] == 2 * B + 1, "pair_match: trans [B, 4, 4], radius [B]"
  flags = _seg_flags(flags, B, dev)
  cap, m_max = int(capacity), pts.shape[0]
  if pairs is None:
    pairs = torch.empty((cap, 2), dtype=torch.int32, device=dev)
  assert pairs.dtype == torch.int32 and pairs.dim() == 2 and pairs.shape[1] == 2 and pairs.shape[0] >= cap and pairs.is_contiguous() and \
      pairs.device == dev, "pair_match: pairs int32 [>= capacity, 2] on the points' device, contiguous"
  counts = torch.empty(B, dtype=torch.int64, device=dev)
  totals = torch.empty(4, dtype=torch.int64, device=dev)
  ws, wsb = ws_args(lib.pcmi_pair_match_workspace_bytes(m_max, B), dev)
  check(lib.pcmi_pair_match(ptr(pts), m_max, ptr(voff), ptr(side), B, ptr(tr), ptr(rd), ptr(pairs) if cap else None, cap, ptr(counts),
                            ptr(totals), ptr(flags), 1 if fill_only else 0, ws, wsb, cur_stream(dev)))
  return dict(pairs=pairs, pair_counts=counts, totals=totals, flags=flags)


def pair_collate(vox, trans, noise=None, jitter_on=None, mu=0.0, sigma=0.01, out_rows=None):
  """pcmi_pair_collate on pair_voxelize's result `vox`: the collated batch with room for out_rows rows per side (None: as many
  as `vox` has).  noise float32 [n_raw, 3] standard normals (None: features are 1), jitter_on int32 [2 B].  Returns a dict of
  device tensors: sinput{0,1}_C int32 [out_rows, 4], pcd{0,1} and sinput{0,1}_F float32 [out_rows, 3] (valid rows:
  side_offsets[s][B]) and T_gt float32 [4 B, 4]."""
  pts = vox["points"]
  require_cuda(pts, "pair_collate")
  dev = pts.device
  voff, side = vox["vox_offsets"], vox["side_offsets"]
  B = side.shape[1] - 1
  tr = _f64c(trans, dev, "pair_collate").reshape(-1, 16)
  assert tr.shape[0] == B, "pair_collate: trans [B, 4, 4]"
  nz = None if noise is None else _f32c(noise.to(dev), "pair_collate")
  assert nz is None or (nz.dim() == 2 and nz.shape[1] == 3), "pair_collate: noise [n_raw, 3]"
  on = None if nz is None else _i32c(torch.as_tensor(jitter_on), dev).reshape(-1)
  assert on is None or on.shape[0] == 2 * B, "pair_collate: jitter_on [2 B]"
  m_max = pts.shape[0]
  rows = m_max if out_rows is None else int(out_rows)
  out = {}
  for s in "01":
    out["sinput%s_C" % s] = torch.empty((rows, 4), dtype=torch.int32, device=dev)
    out["pcd" + s] = torch.empty((rows, 3), dtype=torch.float32, device=dev)
    out["sinput%s_F" % s] = torch.empty((rows, 3), dtype=torch.float32, device=dev)
  out["T_gt"] = torch.empty((4 * B, 4), dtype=torch.float32, device=dev)
  ws, wsb = ws_args(lib.pcmi_pair_collate_workspace_bytes(m_max, B), dev)
  check(lib.pcmi_pair_collate(ptr(pts), ptr(vox["coords"]), ptr(vox["first_index"]), m_max, ptr(voff), ptr(side), B, ptr(tr), ptr(nz),
                              0 if nz is None else nz.shape[0], ptr(on), float(mu), float(sigma), rows, ptr(out["sinput0_C"]),
                              ptr(out["sinput1_C"]), ptr(out["pcd0"]), ptr(out["pcd1"]), ptr(out["sinput0_F"]), ptr(out["sinput1_F"]),
                              ptr(out["T_gt"]), ws, wsb, cur_stream(dev)))
  return out


def pair_color_features(color, vox, collated, noise=None, jitter_on=None, mu=0.0, sigma=0.01):
  """pcmi_pair_color_features: writes the colour features into sinput0_F / sinput1_F of pair_collate's result `collated`, in
  place and after it in stream order.  color uint8 [n_raw, 3] (the RGB of the raw rows pair_voxelize's first_index points into),
  noise / jitter_on / mu / sigma as in pair_collate.  F = fp32((c / 255 - 0.5) + (mu + sigma z)), or fp32(c / 255 - 0.5) without
  jitter.  Returns `collated`."""
  require_cuda(color, "pair_color_features")
  dev = color.device
  assert color.dtype == torch.uint8 and color.dim() == 2 and color.shape[1] == 3, "pair_color_features: color uint8 [n_raw, 3]"
  col = color.contiguous()
  voff, side, first = vox["vox_offsets"], vox["side_offsets"], vox["first_index"]
  B = side.shape[1] - 1
  nz = None if noise is None else _f32c(noise.to(dev), "pair_color_features")
  assert nz is None or tuple(nz.shape) == (col.shape[0], 3), "pair_color_features: noise [n_raw, 3]"
  on = None if nz is None else _i32c(torch.as_tensor(jitter_on), dev).reshape(-1)
  assert on is None or on.shape[0] == 2 * B, "pair_color_features: jitter_on [2 B]"
  F0, F1 = collated["sinput0_F"], collated["sinput1_F"]
  for F in (F0, F1):
    assert F.dtype == torch.float32 and F.dim() == 2 and F.shape[1] == 3 and F.is_contiguous() and F.device == dev and \
        F.shape[0] == F0.shape[0], "pair_color_features: sinput{0,1}_F float32 [out_rows, 3] on the colours' device, contiguous"
  m_max = first.shape[0]
  ws, wsb = ws_args(lib.pcmi_pair_color_features_workspace_bytes(m_max, B), dev)
  check(lib.pcmi_pair_color_features(ptr(col), ptr(first), m_max, ptr(voff), ptr(side), B, ptr(nz), col.shape[0], ptr(on), float(mu),
                                     float(sigma), F0.shape[0], ptr(F0), ptr(F1), ws, wsb, cur_stream(dev)))
  return collated


# ---------------------------------------------------------------------------------------------------------------------
# The input of detection fine-tuning (csrc/detect_input.hip): what ScannetDetectionDataset / SunrgbdDetectionVotesDataset
# __getitem__ and VoxelizationDataset + collate_fn of the reference (downstream/votenet_det_new) do per scan on the host, for a
# batch.  None of these is differentiable and none synchronises; errors arrive in `flags` (int32 [B], DET_FLAG_* bits per scene).
# ---------------------------------------------------------------------------------------------------------------------
DET_FLAG_RANGE, DET_FLAG_SPAN, DET_FLAG_CHOICE, DET_FLAG_INSTANCE, DET_FLAG_LABEL, DET_FLAG_BOXES = 1, 2, 4, 8, 16, 32
DET_FLAG_FEATURE = 64
DET_FLAG_NAMES = {DET_FLAG_RANGE: "a chosen point or a box is not finite, or a voxel coordinate is outside +-2^20",
                  DET_FLAG_SPAN: "a voxel coordinate lies 2^18 or more above the scene's minimum",
                  DET_FLAG_CHOICE: "a choice is outside the scene's rows",
                  DET_FLAG_INSTANCE: "an instance id is outside [0, 1024)",
                  DET_FLAG_LABEL: "a box's label has no class",
                  DET_FLAG_BOXES: "the number of boxes is outside [0, 64]",
                  DET_FLAG_FEATURE: "the scan is empty or holds a non-finite z (no floor height), or a chosen colour or z is not finite"}
DET_MAX_INSTANCES = 1024  # PCMI_DET_MAX_INSTANCES
DET_MAX_NUM_OBJ = 64      # PCMI_DET_MAX_NUM_OBJ, the reference's MAX_NUM_OBJ
DET_MODES = {"scannet": 0, "sunrgbd": 1}


def det_flags_message(flags_host):
  """The exception text for a read-back flags array (None if no bit is set): every flagged scene with its causes."""
  bad = ["scene %d: %s" % (b, "; ".join(t for bit, t in DET_FLAG_NAMES.items() if int(f) & bit) or "flag %d" % int(f))
         for b, f in enumerate(flags_host) if int(f)]
  return "detection input: " + " | ".join(bad) if bad else None


def _det_draws(dev, B, augment, flip, rot, scale, who):
  if not augment:
    return None, None, None
  fl = _i32c(torch.as_tensor(flip), dev).reshape(-1, 2)
  R = _f64c(rot, dev, who).reshape(-1, 9)
  sc = _f64c(scale, dev, who).reshape(-1)
  assert fl.shape[0] == B and R.shape[0] == B and sc.shape[0] == B, who + ": flip [B, 2], rot [B, 9], scale [B]"
  return fl, R, sc


def _det_sample_args(xyz, offsets, choices, who):
  require_cuda(xyz, who)
  dev = xyz.device
  x, offs = _f32c(xyz, who), _offsets(offsets, dev)
  ch = _i32c(torch.as_tensor(choices), dev)
  assert x.dim() == 2 and x.shape[1] == 3 and offs.dim() == 1 and offs.shape[0] >= 2, who + ": xyz [n, 3], offsets [B + 1]"
  B = offs.shape[0] - 1
  assert ch.dim() == 2 and ch.shape[0] == B and ch.shape[1] >= 1, who + ": choices [B, num_points]"
  return dev, x, offs, ch, B, ch.shape[1]


def det_sample_transform(xyz, offsets, choices, augment=True, flip=None, rot=None, scale=None, instance=None, semantic=None,
                         flags=None):
  """pcmi_det_sample_transform.  xyz float32 [n, 3], offsets [B + 1], choices int32 [B, P] (rows within the scene); with
  augment: flip [B, 2], rot float64 [B, 9], scale float64 [B].  instance, semantic int32 [n] (optional payloads).  Returns a
  dict of device tensors: point_clouds float32 [B, P, 3], out_instance / out_semantic int32 [B, P] (None without the
  payload), flags int32 [B]."""
  dev, x, offs, ch, B, P = _det_sample_args(xyz, offsets, choices, "det_sample_transform")
  fl, R, sc = _det_draws(dev, B, augment, flip, rot, scale, "det_sample_transform")
  ins = None if instance is None else _i32c(torch.as_tensor(instance), dev).reshape(-1)
  sem = None if semantic is None else _i32c(torch.as_tensor(semantic), dev).reshape(-1)
  assert (ins is None or ins.shape[0] == x.shape[0]) and (sem is None or sem.shape[0] == x.shape[0]), \
      "det_sample_transform: instance [n], semantic [n]"
  flags = _seg_flags(flags, B, dev)
  pc = torch.empty((B, P, 3), dtype=torch.float32, device=dev)
  oi = None if ins is None else torch.empty((B, P), dtype=torch.int32, device=dev)
  os_ = None if sem is None else torch.empty((B, P), dtype=torch.int32, device=dev)
  check(lib.pcmi_det_sample_transform(ptr(x), ptr(offs), x.shape[0], B, P, ptr(ch), 1 if augment else 0, ptr(fl), ptr(R), ptr(sc),
                                      ptr(ins), ptr(sem), ptr(pc), ptr(oi), ptr(os_), ptr(flags), cur_stream(dev)))
  return dict(point_clouds=pc, out_instance=oi, out_semantic=os_, flags=flags)


def det_votes_transform(xyz, votes, offsets, choices, augment=True, flip=None, rot=None, scale=None, flags=None):
  """pcmi_det_votes_transform: det_sample_transform with the stored votes float64 [n, 10] of SUN RGB-D carried along.  Returns
  point_clouds float32 [B, P, 3], vote_label float32 [B, P, 9], vote_label_mask int64 [B, P], flags."""
  dev, x, offs, ch, B, P = _det_sample_args(xyz, offsets, choices, "det_votes_transform")
  v = _f64c(votes, dev, "det_votes_transform")
  assert v.shape == (x.shape[0], 10), "det_votes_transform: votes float64 [n, 10]"
  fl, R, sc = _det_draws(dev, B, augment, flip, rot, scale, "det_votes_transform")
  flags = _seg_flags(flags, B, dev)
  pc = torch.empty((B, P, 3), dtype=torch.float32, device=dev)
  vl = torch.empty((B, P, 9), dtype=torch.float32, device=dev)
  vm = torch.empty((B, P), dtype=torch.int64, device=dev)
  check(lib.pcmi_det_votes_transform(ptr(x), ptr(v), ptr(offs), x.shape[0], B, P, ptr(ch), 1 if augment else 0, ptr(fl), ptr(R),
                                     ptr(sc), ptr(pc), ptr(vl), ptr(vm), ptr(flags), cur_stream(dev)))
  return dict(point_clouds=pc, vote_label=vl, vote_label_mask=vm, flags=flags)


def det_votes_from_instances(point_clouds, instance, semantic, valid_sem, flags=None):
  """pcmi_det_votes_from_instances.  point_clouds float32 [B, P, 3], instance and semantic int32 [B, P], valid_sem int32
  [n_valid].  Returns vote_label float32 [B, P, 9], vote_label_mask int64 [B, P], flags int32 [B]."""
  require_cuda(point_clouds, "det_votes_from_instances")
  dev = point_clouds.device
  pc = _f32c(point_clouds, "det_votes_from_instances")
  assert pc.dim() == 3 and pc.shape[2] == 3 and pc.shape[1] >= 1, "det_votes_from_instances: point_clouds [B, P, 3]"
  B, P = pc.shape[0], pc.shape[1]
  ins, sem = _i32c(torch.as_tensor(instance), dev).reshape(-1), _i32c(torch.as_tensor(semantic), dev).reshape(-1)
  assert ins.shape[0] == B * P and sem.shape[0] == B * P, "det_votes_from_instances: instance [B, P], semantic [B, P]"
  vs = _i32c(torch.as_tensor(valid_sem), dev).reshape(-1)
  flags = _seg_flags(flags, B, dev)
  vl = torch.empty((B, P, 9), dtype=torch.float32, device=dev)
  vm = torch.empty((B, P), dtype=torch.int64, device=dev)
  ws, wsb = ws_args(lib.pcmi_det_votes_from_instances_workspace_bytes(B), dev)
  check(lib.pcmi_det_votes_from_instances(ptr(pc), ptr(ins), ptr(sem), B, P, ptr(vs), vs.shape[0], ptr(vl), ptr(vm), ptr(flags), ws,
                                          wsb, cur_stream(dev)))
  return dict(vote_label=vl, vote_label_mask=vm, flags=flags)


def det_box_labels(boxes, n_boxes, dataset, mean_size, augment=True, flip=None, rot=None, rot_angle=None, scale=None,
                   heading_cs=None, label_to_class=None, num_heading_bin=1, flags=None):
  """pcmi_det_box_labels.  boxes float64 [B, 64, 8] on the device, n_boxes int32 [B], dataset "scannet" or "sunrgbd", mean_size
  float64 [n_class, 3]; with augment: flip [B, 2], rot [B, 9], and for SUN RGB-D rot_angle [B], scale [B]; heading_cs float64
  [B, 64, 2] (SUN RGB-D: cos and sin of -1 * the final heading); label_to_class int32 [n_lut] (ScanNet).  Returns the
  reference's label keys as device tensors [B, 64(, 3)], and flags."""
  require_cuda(boxes, "det_box_labels")
  dev = boxes.device
  bx = _f64c(boxes, dev, "det_box_labels")
  assert bx.dim() == 3 and bx.shape[1:] == (DET_MAX_NUM_OBJ, 8), "det_box_labels: boxes [B, 64, 8]"
  B, mode = bx.shape[0], DET_MODES[dataset]
  nb = _i32c(torch.as_tensor(n_boxes), dev).reshape(-1)
  ms = _f64c(mean_size, dev, "det_box_labels").reshape(-1, 3)
  assert nb.shape[0] == B and ms.shape[0] >= 1, "det_box_labels: n_boxes [B], mean_size [n_class, 3]"
  fl = R = ra = sc = None
  if augment:
    fl, R = _i32c(torch.as_tensor(flip), dev).reshape(-1, 2), _f64c(rot, dev, "det_box_labels").reshape(-1, 9)
    assert fl.shape[0] == B and R.shape[0] == B, "det_box_labels: flip [B, 2], rot [B, 9]"
    if mode == 1:
      ra, sc = _f64c(rot_angle, dev, "det_box_labels").reshape(-1), _f64c(scale, dev, "det_box_labels").reshape(-1)
      assert ra.shape[0] == B and sc.shape[0] == B, "det_box_labels: rot_angle [B], scale [B]"
  cs = None if heading_cs is None else _f64c(heading_cs, dev, "det_box_labels")
  assert cs is None or cs.shape == (B, DET_MAX_NUM_OBJ, 2), "det_box_labels: heading_cs [B, 64, 2]"
  lut = None if label_to_class is None else _i32c(torch.as_tensor(label_to_class), dev).reshape(-1)
  flags = _seg_flags(flags, B, dev)
  K = DET_MAX_NUM_OBJ
  out = dict(center_label=torch.empty((B, K, 3), dtype=torch.float32, device=dev),
             heading_class_label=torch.empty((B, K), dtype=torch.int64, device=dev),
             heading_residual_label=torch.empty((B, K), dtype=torch.float32, device=dev),
             size_class_label=torch.empty((B, K), dtype=torch.int64, device=dev),
             size_residual_label=torch.empty((B, K, 3), dtype=torch.float32, device=dev),
             sem_cls_label=torch.empty((B, K), dtype=torch.int64, device=dev),
             box_label_mask=torch.empty((B, K), dtype=torch.float32, device=dev), flags=flags)
  check(lib.pcmi_det_box_labels(ptr(bx), ptr(nb), B, mode, 1 if augment else 0, ptr(fl), ptr(R), ptr(ra), ptr(sc), ptr(cs), ptr(lut),
                                0 if lut is None else lut.shape[0], ptr(ms), ms.shape[0], int(num_heading_bin), ptr(out["center_label"]),
                                ptr(out["heading_class_label"]), ptr(out["heading_residual_label"]), ptr(out["size_class_label"]),
                                ptr(out["size_residual_label"]), ptr(out["sem_cls_label"]), ptr(out["box_label_mask"]), ptr(flags),
                                cur_stream(dev)))
  return out


def det_voxelize(point_clouds, voxel_size, flags=None):
  """pcmi_det_voxelize.  point_clouds float32 [B, P, 3].  Returns a dict of device tensors whose first counts[B] rows are valid
  -- voxel_coords int32 [B P, 4] (b, x, y, z), voxel_inds int32 [B P] (the voxel's first row within its scene), voxel_feats
  float32 [B P, 3] (ones) -- and counts int64 [B + 1] (voxels per scene, then their sum), flags int32 [B].  Nothing is read
  back: slice after reading counts."""
  require_cuda(point_clouds, "det_voxelize")
  dev = point_clouds.device
  pc = _f32c(point_clouds, "det_voxelize")
  assert pc.dim() == 3 and pc.shape[2] == 3 and pc.shape[1] >= 1, "det_voxelize: point_clouds [B, P, 3]"
  B, P = pc.shape[0], pc.shape[1]
  flags = _seg_flags(flags, B, dev)
  coords = torch.empty((B * P, 4), dtype=torch.int32, device=dev)
  inds = torch.empty(B * P, dtype=torch.int32, device=dev)
  feats = torch.empty((B * P, 3), dtype=torch.float32, device=dev)
  counts = torch.empty(B + 1, dtype=torch.int64, device=dev)
  ws, wsb = ws_args(lib.pcmi_det_voxelize_workspace_bytes(B, P), dev)
  check(lib.pcmi_det_voxelize(ptr(pc), B, P, float(voxel_size), ptr(coords), ptr(inds), ptr(feats), ptr(counts), ptr(flags), ws, wsb,
                              cur_stream(dev)))
  return dict(voxel_coords=coords, voxel_inds=inds, voxel_feats=feats, counts=counts, flags=flags)


def segment_quantile(values, offsets, q, column=None, flags=None, return_stats=False):
  """pcmi_segment_quantile: numpy's percentile (method "linear") of every scene of a batch, exact order statistics, no
  synchronisation.  values float32 [n] -- or [n, w] with column = the column to read in place (xyz [n, 3], column 2: the z
  of every vertex); offsets [B + 1]; q in [0, 100].  Returns a dict of device tensors: quantile float64 [B], stats float32
  [B, 2] (the two order statistics lo, hi; None unless return_stats), flags int32 [B] (DET_FLAG_FEATURE for an empty scene or
  one with a non-finite value, whose quantile is 0)."""
  require_cuda(values, "segment_quantile")
  dev = values.device
  v, offs = _f32c(values, "segment_quantile"), _offsets(offsets, dev)
  assert offs.dim() == 1 and offs.shape[0] >= 2, "segment_quantile: offsets [B + 1]"
  if column is None:
    assert v.dim() == 1, "segment_quantile: values [n], or [n, w] with column"
    stride, first = 1, 0
  else:
    assert v.dim() == 2 and 0 <= int(column) < v.shape[1], "segment_quantile: values [n, w] and 0 <= column < w"
    stride, first = v.shape[1], int(column)
  n, B = v.shape[0], offs.shape[0] - 1
  flags = _seg_flags(flags, B, dev)
  out = torch.empty(B, dtype=torch.float64, device=dev)
  stats = torch.empty((B, 2), dtype=torch.float32, device=dev) if return_stats else None
  ws, wsb = ws_args(lib.pcmi_segment_quantile_workspace_bytes(B), dev)
  base = C.c_void_p(v.data_ptr() + 4 * first) if n else None
  check(lib.pcmi_segment_quantile(base, stride, ptr(offs), n, B, float(q), ptr(out), ptr(stats), ptr(flags), ws, wsb, cur_stream(dev)))
  return dict(quantile=out, stats=stats, flags=flags)


def det_point_features(point_clouds, xyz, offsets, choices, dataset, rgb=None, floor_height=None, augment=False, scale=None,
                       color_gain=None, color_shift=None, color_jitter=None, color_keep=None, flags=None):
  """pcmi_det_point_features: the final point_clouds float32 [B, P, 3 + C] -- xyz, then rgb, then height.  point_clouds float32
  [B, P, 3] (det_sample_transform / det_votes_transform); xyz float32 [n, 3], the raw scans; offsets [B + 1]; choices int32
  [B, P]; dataset "scannet" or "sunrgbd"; rgb float32 [n, 3] (raw colours; None: no colour columns); floor_height float64 [B]
  on the device (segment_quantile's; None: no height column).  With augment and "sunrgbd": scale float64 [B] (the height),
  color_gain, color_shift float64 [B, 3], color_jitter float64 [B, P], color_keep bool / uint8 [B, P] (each None = identity).
  Returns (point_clouds [B, P, 3 + C], flags int32 [B])."""
  require_cuda(point_clouds, "det_point_features")
  dev = point_clouds.device
  pc, x, offs = _f32c(point_clouds, "det_point_features"), _f32c(xyz, "det_point_features"), _offsets(offsets, dev)
  ch = _i32c(torch.as_tensor(choices), dev)
  assert pc.dim() == 3 and pc.shape[2] == 3 and x.dim() == 2 and x.shape[1] == 3, "det_point_features: point_clouds [B, P, 3], xyz [n, 3]"
  B, P, n = pc.shape[0], pc.shape[1], x.shape[0]
  assert offs.shape == (B + 1,) and ch.shape == (B, P), "det_point_features: offsets [B + 1], choices [B, P]"
  assert rgb is not None or floor_height is not None, "det_point_features: rgb, floor_height or both"
  col = None if rgb is None else _f32c(rgb, "det_point_features")
  assert col is None or col.shape == (n, 3), "det_point_features: rgb [n, 3]"
  fh = None if floor_height is None else _f64c(floor_height, dev, "det_point_features").reshape(-1)
  assert fh is None or fh.shape[0] == B, "det_point_features: floor_height [B]"
  mode = DET_MODES[dataset]
  sc = gain = shift = jit = keep = None
  if augment and mode == 1:
    if fh is not None:
      sc = _f64c(scale, dev, "det_point_features").reshape(-1)
      assert sc.shape[0] == B, "det_point_features: scale [B]"
    if col is not None:
      gain = None if color_gain is None else _f64c(color_gain, dev, "det_point_features").reshape(-1, 3)
      shift = None if color_shift is None else _f64c(color_shift, dev, "det_point_features").reshape(-1, 3)
      jit = None if color_jitter is None else _f64c(color_jitter, dev, "det_point_features")
      keep = None if color_keep is None else torch.as_tensor(color_keep).to(device=dev, dtype=torch.uint8).contiguous()
      assert (gain is None or gain.shape[0] == B) and (shift is None or shift.shape[0] == B) and (jit is None or jit.shape == (B, P)) and \
          (keep is None or keep.shape == (B, P)), "det_point_features: color_gain, color_shift [B, 3], color_jitter, color_keep [B, P]"
  flags = _seg_flags(flags, B, dev)
  Cf = (0 if col is None else 3) + (0 if fh is None else 1)
  out = torch.empty((B, P, 3 + Cf), dtype=torch.float32, device=dev)
  check(lib.pcmi_det_point_features(ptr(pc), ptr(x), ptr(col), ptr(offs), n, B, P, ptr(ch), ptr(fh), mode, 1 if augment else 0, ptr(sc),
                                    ptr(gain), ptr(shift), ptr(jit), ptr(keep), ptr(out), ptr(flags), cur_stream(dev)))
  return out, flags


# ---------------------------------------------------------------------------------------------------------------------
# VoteNet head on row-major activations (csrc/votehead.hip): fp32 rows [rows, ld], feature columns first, geometric columns
# behind them, zero columns up to ld.  As with the point-set ops, the forward pass validates the indices on the device and
# the backward pass reuses them without a host synchronisation.
# ---------------------------------------------------------------------------------------------------------------------
def pad_width(c, multiple=32):
  """c rounded up to the next multiple (the dense GEMM's channel granularity)."""
  return (int(c) + multiple - 1) // multiple * multiple


class GroupRowsFunction(Function):
  """QueryAndGroup(use_xyz=True, normalize_xyz) as rows: (xyz [B, n, 3], centre [B, np, 3], feat [B n, C] or None,
  idx int32 [B, np, ns], radius_div, out_ld) -> [B np ns, out_ld] = features, (xyz - centre) / radius_div, zeros."""

  @staticmethod
  def forward(ctx, xyz, centre, feat, idx, radius_div, out_ld, validate=True):
    xyz, centre = _f32c(xyz, "group_rows"), _f32c(centre, "group_rows")
    dev = xyz.device
    idx = _i32c(idx, dev)
    assert xyz.dim() == 3 and centre.dim() == 3 and idx.dim() == 3 and xyz.shape[2] == 3 and centre.shape[2] == 3 and \
        idx.shape[:2] == centre.shape[:2] and xyz.shape[0] == centre.shape[0], \
        "group_rows: xyz [B, n, 3], centre [B, np, 3], idx [B, np, ns]"
    B, n, _ = xyz.shape
    _, npoint, ns = idx.shape
    if feat is not None:
      feat = _c(feat if feat.dtype == torch.float32 else feat.float())
      assert feat.dim() == 2 and feat.shape[0] == B * n, "group_rows: feat [B n, C]"
    Cc = feat.shape[1] if feat is not None else 0
    out = torch.empty((B * npoint * ns, int(out_ld)), dtype=torch.float32, device=dev)
    check(lib.pcmi_group_rows_fwd(ptr(xyz), ptr(centre), ptr(feat) if Cc else None, feat.stride(0) if Cc else 0, ptr(idx), B, n,
                                  npoint, ns, Cc, float(radius_div), ptr(out), int(out_ld), int(bool(validate)), cur_stream(dev)))
    ctx.save_for_backward(idx)
    ctx.shape, ctx.radius_div, ctx.has_feat = (B, n, npoint, ns, Cc), float(radius_div), feat is not None
    return out

  @staticmethod
  @once_differentiable
  def backward(ctx, gout):
    (idx,) = ctx.saved_tensors
    B, n, npoint, ns, Cc = ctx.shape
    g = _c(gout)
    dev = g.device
    gfeat = torch.empty((B * n, Cc), dtype=torch.float32, device=dev) if ctx.has_feat else None
    gxyz = torch.empty((B, n, 3), dtype=torch.float32, device=dev)
    gcentre = torch.empty((B, npoint, 3), dtype=torch.float32, device=dev)
    ws, wsb = ws_args(lib.pcmi_group_rows_bwd_workspace_bytes(B, n, npoint, ns), dev)
    check(lib.pcmi_group_rows_bwd(ptr(g), g.stride(0), ptr(idx), B, n, npoint, ns, Cc, ctx.radius_div,
                                  ptr(gfeat) if Cc else None, Cc, ptr(gxyz), ptr(gcentre), ws, wsb, cur_stream(dev)))
    return gxyz, gcentre, gfeat, None, None, None, None


def rows_maxpool(x, ns):
  """(out [R, C], arg uint8 [R, C]) of x [R ns, C]: the maximum over every ns consecutive rows and the row within the window
  that holds it -- the lowest among equals, the lowest NaN if there is one (pcmi_rows_maxpool_fwd)."""
  require_cuda(x, "rows_maxpool")
  x = _c(x)
  rows, c, ld = _rows(x)
  assert ns >= 1 and rows % ns == 0, "rows_maxpool: %d rows are not windows of %d" % (rows, ns)
  R = rows // ns
  out = torch.empty((R, c), dtype=torch.float32, device=x.device)
  arg = torch.empty((R, c), dtype=torch.uint8, device=x.device)
  check(lib.pcmi_rows_maxpool_fwd(ptr(x), ld, R, int(ns), c, ptr(out), c, ptr(arg), cur_stream(x.device)))
  return out, arg


class RowsMaxPoolFunction(Function):
  """max_pool2d over nsample (pointnet2_modules.py:255-257) on rows: x [R ns, C] -> [R, C]."""

  @staticmethod
  def forward(ctx, x, ns):
    out, arg = rows_maxpool(x, ns)
    ctx.save_for_backward(arg)
    ctx.ns = int(ns)
    return out

  @staticmethod
  @once_differentiable
  def backward(ctx, gout):
    (arg,) = ctx.saved_tensors
    g = _c(gout)
    R, c = arg.shape
    gx = torch.empty((R * ctx.ns, c), dtype=torch.float32, device=g.device)
    check(lib.pcmi_rows_maxpool_bwd(ptr(g), g.stride(0), ptr(arg), R, ctx.ns, c, ptr(gx), c, cur_stream(g.device)))
    return gx, None


# ---------------------------------------------------------------------------------------------------------------------
# The PointNet++ backbone on rows (csrc/rowspool.hip): BatchNorm + ReLU + max over nsample in one pass, and the feature
# propagation's interpolation + concatenation written into rows.
# ---------------------------------------------------------------------------------------------------------------------
def _maxpool_rows(x, ns, who):
  require_cuda(x, who)
  x = _c(x)
  rows, c, ld = _rows(x)
  assert ns >= 1 and rows % ns == 0, "%s: %d rows are not windows of %d" % (who, rows, ns)
  return x, rows // int(ns), c, ld


class BatchNormMaxPoolFunction(Function):
  """rows_maxpool(bn_relu(x), ns) without the intermediate: (x [R ns, C], gamma, beta, running_mean, running_var, momentum,
  eps, ns) -> (out [R, C], arg uint8 [R, C]) with training-mode statistics over all R ns rows (pcmi_bn_maxpool_fwd_train /
  _bwd).  Keeps x, the pooled output and the argument rows for the backward pass."""

  @staticmethod
  def forward(ctx, x, gamma, beta, running_mean, running_var, momentum, eps, ns):
    x, R, c, x_ld = _maxpool_rows(x, ns, "bn_maxpool")
    dev = x.device
    out = torch.empty((R, c), dtype=torch.float32, device=dev)
    arg = torch.empty((R, c), dtype=torch.uint8, device=dev)
    mean = torch.empty(c, dtype=torch.float32, device=dev)
    invstd = torch.empty(c, dtype=torch.float32, device=dev)
    ws, wsb = ws_args(lib.pcmi_bn_maxpool_workspace_bytes(R, int(ns), c), dev)
    check(lib.pcmi_bn_maxpool_fwd_train(ptr(x), x_ld, R, int(ns), c, ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var),
                                        float(momentum), float(eps), ptr(out), c, ptr(arg), ptr(mean), ptr(invstd), ws, wsb,
                                        cur_stream(dev)))
    ctx.save_for_backward(x, gamma, mean, invstd, out, arg)
    ctx.mark_non_differentiable(arg)
    ctx.ns = int(ns)
    return out, arg

  @staticmethod
  @once_differentiable
  def backward(ctx, gout, garg=None):
    x, gamma, mean, invstd, out, arg = ctx.saved_tensors
    g = _c(gout)
    n, c, x_ld = _rows(x)
    R, dev = out.shape[0], x.device
    dx = torch.empty((n, c), dtype=torch.float32, device=dev)
    dgamma = torch.empty(c, dtype=torch.float32, device=dev)
    dbeta = torch.empty(c, dtype=torch.float32, device=dev)
    ws, wsb = ws_args(lib.pcmi_bn_maxpool_workspace_bytes(R, ctx.ns, c), dev)
    check(lib.pcmi_bn_maxpool_bwd(ptr(g), g.stride(0), ptr(x), x_ld, ptr(out), c, ptr(arg), R, ctx.ns, c, ptr(gamma), ptr(mean),
                                  ptr(invstd), ptr(dx), c, ptr(dgamma), ptr(dbeta), ws, wsb, cur_stream(dev)))
    return dx, dgamma, dbeta, None, None, None, None, None


def batch_norm_maxpool_eval(x, gamma, beta, running_mean, running_var, eps, ns, want_arg=False):
  """The eval form of BatchNormMaxPoolFunction: the same pass on the running estimates (pcmi_bn_maxpool_fwd_eval); no
  gradient.  want_arg: also return the uint8 argument rows."""
  x, R, c, x_ld = _maxpool_rows(x, ns, "bn_maxpool (eval)")
  out = torch.empty((R, c), dtype=torch.float32, device=x.device)
  arg = torch.empty((R, c), dtype=torch.uint8, device=x.device) if want_arg else None
  check(lib.pcmi_bn_maxpool_fwd_eval(ptr(x), x_ld, R, int(ns), c, ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var),
                                     float(eps), ptr(out), c, ptr(arg), cur_stream(x.device)))
  return (out, arg) if want_arg else out


class InterpRowsFunction(Function):
  """three_interpolate + the concatenation of PointnetFPModule.forward as rows: (known [B m, C2], idx int32 [B, n, 3],
  weight [B, n, 3], skip [B n, C1] or None, out_ld) -> [B n, out_ld] = interpolated features, skip features, zeros.
  Differentiable in known and skip (the weights carry no gradient, as in the reference)."""

  @staticmethod
  def forward(ctx, known, idx, weight, skip, out_ld, validate=True):
    require_cuda(known, "interp_rows")
    known = _c(known if known.dtype == torch.float32 else known.float())
    dev = known.device
    idx, w = _i32c(idx, dev), _f32c(weight, "interp_rows")
    assert known.dim() == 2 and idx.dim() == 3 and idx.shape[2] == 3 and w.shape == idx.shape and known.shape[0] % idx.shape[0] == 0, \
        "interp_rows: known [B m, C2], idx / weight [B, n, 3]"
    B, n, _ = idx.shape
    m, C2 = known.shape[0] // B, known.shape[1]
    C1 = 0
    if skip is not None:
      skip = _c(skip if skip.dtype == torch.float32 else skip.float())
      assert skip.dim() == 2 and skip.shape[0] == B * n, "interp_rows: skip [B n, C1]"
      C1 = skip.shape[1]
    out = torch.empty((B * n, int(out_ld)), dtype=torch.float32, device=dev)
    check(lib.pcmi_interp_rows_fwd(ptr(known), known.stride(0), ptr(idx), ptr(w), ptr(skip) if C1 else None, skip.stride(0) if C1 else 0,
                                   B, m, n, C2, C1, ptr(out), int(out_ld), int(bool(validate)), cur_stream(dev)))
    ctx.save_for_backward(idx, w)
    ctx.shape, ctx.has_skip = (B, m, n, C2, C1), skip is not None
    return out

  @staticmethod
  @once_differentiable
  def backward(ctx, gout):
    idx, w = ctx.saved_tensors
    B, m, n, C2, C1 = ctx.shape
    g = _c(gout)
    dev = g.device
    gknown = torch.empty((B * m, C2), dtype=torch.float32, device=dev)
    ws, wsb = ws_args(lib.pcmi_interp_rows_bwd_workspace_bytes(B, m, n), dev)
    check(lib.pcmi_interp_rows_bwd(ptr(g), g.stride(0), ptr(idx), ptr(w), B, m, n, C2, ptr(gknown), C2, ws, wsb, cur_stream(dev)))
    return gknown, None, None, (g[:, C2:C2 + C1] if ctx.has_skip else None), None, None


class VoteFunction(Function):
  """The tail of VotingModule.forward and the feature normalisation of votenet.py:120-121: (net [R, vf Wb], seed_xyz [R, 3],
  seed_feat [R, C], vote_factor) -> (vote_xyz [R vf, 3], vote_feat [R vf, C]); block v of a row of net holds C residual
  features, then 3 offsets, then zeros."""

  @staticmethod
  def forward(ctx, net, seed_xyz, seed_feat, vote_factor):
    require_cuda(net, "vote")
    net, seed_feat = _c(net), _c(seed_feat)
    seed_xyz = _f32c(seed_xyz, "vote").reshape(-1, 3)
    R, width, net_ld = _rows(net)
    vf, Cc = int(vote_factor), seed_feat.shape[1]
    assert width % vf == 0 and seed_feat.shape[0] == R and seed_xyz.shape[0] == R, "vote: net [R, vf Wb], seed_xyz [R, 3], seed_feat [R, C]"
    Wb, dev = width // vf, net.device
    vote_xyz = torch.empty((R * vf, 3), dtype=torch.float32, device=dev)
    vote_feat = torch.empty((R * vf, Cc), dtype=torch.float32, device=dev)
    norm = torch.empty(R * vf, dtype=torch.float32, device=dev)
    check(lib.pcmi_vote_fwd(ptr(net), net_ld, ptr(seed_xyz), ptr(seed_feat), seed_feat.stride(0), R, vf, Cc, Wb, ptr(vote_xyz),
                            ptr(vote_feat), Cc, ptr(norm), cur_stream(dev)))
    ctx.save_for_backward(vote_feat, norm)
    ctx.shape = (R, vf, Cc, Wb)
    return vote_xyz, vote_feat

  @staticmethod
  @once_differentiable
  def backward(ctx, g_xyz, g_feat):
    vote_feat, norm = ctx.saved_tensors
    R, vf, Cc, Wb = ctx.shape
    dev = vote_feat.device
    g_xyz, g_feat = _f32c(g_xyz, "vote"), _c(g_feat)
    g_net = torch.empty((R, vf * Wb), dtype=torch.float32, device=dev)
    g_sf = torch.empty((R, Cc), dtype=torch.float32, device=dev)
    g_sx = torch.empty((R, 3), dtype=torch.float32, device=dev)
    check(lib.pcmi_vote_bwd(ptr(g_feat), g_feat.stride(0), ptr(g_xyz), ptr(vote_feat), Cc, ptr(norm), R, vf, Cc, Wb, ptr(g_net),
                            vf * Wb, ptr(g_sf), Cc, ptr(g_sx), cur_stream(dev)))
    return g_net, g_sx, g_sf, None


def adam_step(w, g, m, v, lr, betas, eps, weight_decay, step):
  """torch.optim.Adam's step number `step` (>= 1) on flat buffers (pcmi_adam_step): amsgrad off, L2 weight decay."""
  require_cuda(w, "adam step")
  check(lib.pcmi_adam_step(ptr(w), ptr(g), ptr(m), ptr(v), w.numel(), float(lr), float(betas[0]), float(betas[1]), float(eps),
                           float(weight_decay), int(step), cur_stream(w.device)))


# ---------------------------------------------------------------------------------------------------------------------
# Validation of the pre-training by feature matching (csrc/featmatch.hip; include/pcmi.h states every rule).  None of
# these is differentiable and none synchronises.  Offsets are the [B + 1] ascending row offsets of the pairs.
# ---------------------------------------------------------------------------------------------------------------------
MATCH_STAT_COLS, MATCH_MAX_TAU = 12, 4
MATCH_N_QUERY, MATCH_N_VALID, MATCH_N_MUTUAL, MATCH_N_GT, MATCH_HITS, MATCH_HITS_GT = 0, 1, 2, 3, 4, 8


def _host_rows_in_segments(rows, row_offsets, seg_offsets, who):
  """query_rows handed over from the HOST are checked there: every row inside its own pair's segment."""
  import numpy as np
  from ._lib import PcmiError
  r, ro, so = np.asarray(rows).reshape(-1), np.asarray(row_offsets).reshape(-1), np.asarray(seg_offsets).reshape(-1)
  seg = np.searchsorted(ro, np.arange(r.shape[0]), side="right") - 1
  ok = (seg >= 0) & (seg < so.shape[0] - 1)
  segc = np.clip(seg, 0, so.shape[0] - 2)
  ok &= (r >= so[segc]) & (r < so[segc + 1])
  if not ok.all():
    i = int(np.flatnonzero(~ok)[0])
    raise PcmiError("%s: query_rows[%d] = %d lies outside its pair's segment of the query features" % (who, i, int(r[i])))


def _on_host(t):
  return not (torch.is_tensor(t) and t.is_cuda)


def feature_nn(qf, q_offsets, rf, r_offsets, query_rows=None, query_offsets=None):
  """pcmi_feat_nn: for every query the row of rf, inside the query's own pair, that minimises |a - b|^2 in fp32 -- all pairs
  in one call.  qf [Nq, C] with q_offsets [B + 1], rf [Nr, C] with r_offsets [B + 1]; C a multiple of 16 in 16 ... 128; rows may
  be strided.  query_rows int32 [Q] with query_offsets [B + 1]: the rows of qf that are queries (repeats, any order), each in
  its pair's segment; None: every row.  Returns (nn int32 [Q], the GLOBAL row of rf, the lowest among equal distances; d2
  float32 [Q]).  nn = -1 and d2 = NaN where the pair has no reference row, the query has a non-finite feature or its row
  lies outside its segment; a reference row with a non-finite feature is never chosen.  query_rows given from the host are
  checked against their segments here (PcmiError); on the device the rule above holds.  Bit-identical from run to run."""
  require_cuda(qf, "feature_nn")
  require_cuda(rf, "feature_nn")
  assert qf.dim() == 2 and rf.dim() == 2 and qf.dtype == torch.float32 and rf.dtype == torch.float32, \
      "feature_nn: float32 [rows, C] features"
  assert qf.shape[1] == rf.shape[1], "feature_nn: query width %d, reference width %d" % (qf.shape[1], rf.shape[1])
  assert (query_rows is None) == (query_offsets is None), "feature_nn: query_rows and query_offsets go together"
  dev = qf.device
  if query_rows is not None and _on_host(query_rows) and _on_host(query_offsets) and _on_host(q_offsets):
    _host_rows_in_segments(query_rows, query_offsets, q_offsets, "feature_nn")
  qf, rf = _c(qf), _c(rf)
  qo, ro = _offsets(q_offsets, dev), _offsets(r_offsets, dev)
  assert qo.dim() == 1 and qo.shape == ro.shape and qo.shape[0] >= 2, "feature_nn: offsets [B + 1]"
  B, c = qo.shape[0] - 1, qf.shape[1]
  rows = offs = None
  Q = qf.shape[0]
  if query_rows is not None:
    rows, offs = _i32c(torch.as_tensor(query_rows), dev).reshape(-1), _offsets(query_offsets, dev)
    assert offs.shape == qo.shape, "feature_nn: query_offsets [B + 1]"
    Q = rows.shape[0]
  nn = torch.empty(Q, dtype=torch.int32, device=dev)
  d2 = torch.empty(Q, dtype=torch.float32, device=dev)
  ws, wsb = ws_args(lib.pcmi_feat_nn_workspace_bytes(Q), dev)
  check(lib.pcmi_feat_nn(ptr(qf), qf.stride(0), qf.shape[0], ptr(qo), ptr(rf), rf.stride(0), rf.shape[0], ptr(ro), B, c,
                         ptr(rows), ptr(offs), Q, ptr(nn), ptr(d2), ws, wsb, cur_stream(dev)))
  return nn, d2


def match_stats(xyz0, xyz1, T_gt, query_offsets, nn01, taus, query_rows=None, nn10=None, has_gt=None, counts=None):
  """pcmi_match_stats: the matches nn01 of the queries checked against the known pose.  xyz0 [N0, 3], xyz1 [N1, 3] float64;
  T_gt float64 [B, 4, 4]; query_rows int32 [Q] (None: every row of cloud 0, query_offsets then cloud 0's offsets); nn01 int32
  [Q]; nn10 int32 [Q] (optional: the nearest row of cloud 0 of each matched row, for the mutual check); has_gt uint8 [N0]
  (optional); taus: 1 ... 4 thresholds.  Returns (counts int64 [B, 12] -- ADDED to the tensor passed in, a fresh one otherwise;
  columns MATCH_N_QUERY, MATCH_N_VALID, MATCH_N_MUTUAL, MATCH_N_GT, MATCH_HITS + t, MATCH_HITS_GT + t -- and residual2
  float64 [Q], NaN where the query has no match)."""
  require_cuda(xyz0, "match_stats")
  dev = xyz0.device
  x0, x1 = _f64c(xyz0, dev, "match_stats"), _f64c(xyz1, dev, "match_stats")
  T = _f64c(T_gt, dev, "match_stats").reshape(-1, 16)
  qo = _offsets(query_offsets, dev)
  assert x0.dim() == 2 and x0.shape[1] == 3 and x1.dim() == 2 and x1.shape[1] == 3, "match_stats: xyz0 [N0, 3], xyz1 [N1, 3]"
  B = qo.shape[0] - 1
  assert B >= 1 and T.shape[0] == B, "match_stats: T_gt [B, 4, 4] for query_offsets [B + 1]"
  taus = [float(t) for t in taus]
  assert 1 <= len(taus) <= MATCH_MAX_TAU, "match_stats: 1 ... %d thresholds" % MATCH_MAX_TAU
  nn01 = _i32c(nn01, dev).reshape(-1)
  Q = nn01.shape[0]
  rows = None if query_rows is None else _i32c(query_rows, dev).reshape(-1)
  assert (rows is None and Q == x0.shape[0]) or (rows is not None and rows.shape[0] == Q), "match_stats: one nn01 per query"
  nn10 = None if nn10 is None else _i32c(nn10, dev).reshape(-1)
  assert nn10 is None or nn10.shape[0] == Q, "match_stats: nn10 [Q]"
  if has_gt is not None:
    has_gt = has_gt.to(device=dev, dtype=torch.uint8).contiguous().reshape(-1)
    assert has_gt.shape[0] == x0.shape[0], "match_stats: has_gt [N0]"
  if counts is None:
    counts = torch.zeros((B, MATCH_STAT_COLS), dtype=torch.int64, device=dev)
  assert counts.shape == (B, MATCH_STAT_COLS) and counts.dtype == torch.int64 and counts.is_contiguous() and counts.device == dev, \
      "match_stats: counts int64 [B, %d] on the clouds' device" % MATCH_STAT_COLS
  residual2 = torch.empty(Q, dtype=torch.float64, device=dev)
  tau_arr = (C.c_double * len(taus))(*taus)
  check(lib.pcmi_match_stats(ptr(x0), x0.shape[0], ptr(x1), x1.shape[0], ptr(T), B, ptr(rows), ptr(qo), Q, ptr(nn01), ptr(nn10),
                             ptr(has_gt), tau_arr, len(taus), ptr(counts), ptr(residual2), cur_stream(dev)))
  return counts, residual2


def ransac_score(src, dst, offsets, triples, tau):
  """pcmi_ransac_score: src, dst float64 [M, 3] (matched points of cloud 0 / cloud 1) with offsets [B + 1]; triples int32
  [B, H, 3], indices local to each pair's matches, H <= 65536.  Returns (counts int32 [B, H]: the inliers within tau of each
  hypothesis' transform, -1 for an invalid one; best int32 [B]: the highest count, lowest hypothesis among equals, -1 if none;
  Rt float64 [B, 12]: the winner's R row-major, then t)."""
  require_cuda(src, "ransac_score")
  dev = src.device
  s, d = _f64c(src, dev, "ransac_score"), _f64c(dst, dev, "ransac_score")
  assert s.dim() == 2 and s.shape[1] == 3 and s.shape == d.shape, "ransac_score: src, dst [M, 3]"
  of = _offsets(offsets, dev)
  B = of.shape[0] - 1
  tr = _i32c(triples, dev)
  assert tr.dim() == 3 and tr.shape[0] == B and tr.shape[2] == 3 and B >= 1, "ransac_score: triples [B, H, 3] for offsets [B + 1]"
  H = tr.shape[1]
  counts = torch.empty((B, H), dtype=torch.int32, device=dev)
  best = torch.empty(B, dtype=torch.int32, device=dev)
  Rt = torch.empty((B, 12), dtype=torch.float64, device=dev)
  check(lib.pcmi_ransac_score(ptr(s), ptr(d), s.shape[0], ptr(of), B, ptr(tr), H, float(tau), ptr(counts), ptr(best), ptr(Rt),
                              cur_stream(dev)))
  return counts, best, Rt


def rigid_sums(src, dst, offsets, best, Rt, tau):
  """pcmi_rigid_sums: over the inliers of each pair's best hypothesis (ransac_score's best and Rt, the same tau) -> float64
  [B, 16]: n, sum p (3), sum q (3) and the 3 x 3 sum of (p - mean p)(q - mean q)^T, row-major; zeros where best is -1."""
  require_cuda(src, "rigid_sums")
  dev = src.device
  s, d = _f64c(src, dev, "rigid_sums"), _f64c(dst, dev, "rigid_sums")
  assert s.dim() == 2 and s.shape[1] == 3 and s.shape == d.shape, "rigid_sums: src, dst [M, 3]"
  of = _offsets(offsets, dev)
  B = of.shape[0] - 1
  best, Rt = _i32c(best, dev).reshape(-1), _f64c(Rt, dev, "rigid_sums").reshape(-1, 12)
  assert B >= 1 and best.shape[0] == B and Rt.shape[0] == B, "rigid_sums: best [B], Rt [B, 12] for offsets [B + 1]"
  out = torch.empty((B, 16), dtype=torch.float64, device=dev)
  check(lib.pcmi_rigid_sums(ptr(s), ptr(d), s.shape[0], ptr(of), B, ptr(best), ptr(Rt), float(tau), ptr(out), cur_stream(dev)))
  return out


# ---------------------------------------------------------------------------------------------------------------------
# Virtual views of a whole scan (csrc/views.hip; no counterpart in the reference): which points F pinhole cameras see.
# The rule -- projection, splat window, float32 depth comparison -- is include/pcmi.h's; nothing here is differentiable.
# ---------------------------------------------------------------------------------------------------------------------
def _view_args(points, w2c, who):
  require_cuda(points, who)
  assert points.dim() == 2 and points.shape[1] == 3 and points.dtype == torch.float64, "%s: points float64 [n, 3]" % who
  dev = points.device
  assert torch.is_tensor(w2c) and w2c.device == dev and w2c.dtype == torch.float64 and w2c.dim() == 3 and w2c.shape[1:] == (4, 4), \
      "%s: w2c float64 [F, 4, 4] on the points' device" % who
  return _c(points), w2c.contiguous(), dev


def view_zbuffer(points, w2c, fx, fy, cx, cy, height, width, z_near=0.1, z_far=10.0, splat=3):
  """pcmi_views_zbuffer: points float64 [n, 3] (world frame; rows may be strided), w2c float64 [F, 4, 4] world-to-camera ->
  zbuf float32 [F, height, width], the smallest float32 depth among the projectable points whose splat x splat window (odd,
  1 ... 7, clipped at the borders) covers the pixel, +inf where there is none.  Bit-identical from run to run; no
  synchronisation."""
  p, m, dev = _view_args(points, w2c, "view_zbuffer")
  F, H, W = m.shape[0], int(height), int(width)
  zbuf = torch.empty((F, max(H, 0), max(W, 0)), dtype=torch.float32, device=dev)
  check(lib.pcmi_views_zbuffer(ptr(p), p.stride(0), p.shape[0], ptr(m), F, float(fx), float(fy), float(cx), float(cy), H, W,
                               float(z_near), float(z_far), int(splat), ptr(zbuf), cur_stream(dev)))
  return zbuf


def view_visible(points, w2c, fx, fy, cx, cy, zbuf, z_near=0.1, z_far=10.0, rel_tol=0.05):
  """pcmi_views_visible + pcmi_views_rows against zbuf float32 [F, H, W] (view_zbuffer's, same points and cameras): a point is
  visible in view f iff it is projectable, its pixel lies inside the image and (double)zf <= (double)zbuf[f, py, px] (1 +
  rel_tol).  Returns (rows int32 [total], the visible rows of every view, ascending inside a view; offsets int64 [F + 1] on
  the device; offsets_host, the same as a numpy array; pixels int64 [F], the occupied pixels of every view; mask int64 [F,
  ceil(n / 64)], bit l of word w = point 64 w + l).  One synchronisation (the offsets)."""
  import numpy as np
  p, m, dev = _view_args(points, w2c, "view_visible")
  n, F = p.shape[0], m.shape[0]
  assert torch.is_tensor(zbuf) and zbuf.device == dev and zbuf.dtype == torch.float32 and zbuf.dim() == 3 and zbuf.shape[0] == F \
      and zbuf.is_contiguous(), "view_visible: zbuf contiguous float32 [F, H, W] on the points' device"
  H, W = zbuf.shape[1], zbuf.shape[2]
  nw = (n + 63) // 64
  mask = torch.empty((F, nw), dtype=torch.int64, device=dev)
  start = torch.empty((F, nw), dtype=torch.int64, device=dev)
  offsets = torch.empty(F + 1, dtype=torch.int64, device=dev)
  pixels = torch.empty(F, dtype=torch.int64, device=dev)
  offs_h = (C.c_int64 * (F + 1))()
  ws, wsb = ws_args(lib.pcmi_views_visible_workspace_bytes(n, F), dev)
  check(lib.pcmi_views_visible(ptr(p), p.stride(0), n, ptr(m), F, float(fx), float(fy), float(cx), float(cy), H, W, float(z_near),
                               float(z_far), float(rel_tol), ptr(zbuf), ptr(mask), ptr(start), ptr(offsets), offs_h, ptr(pixels), ws, wsb,
                               cur_stream(dev)))  # syncs
  offs_np = np.frombuffer(offs_h, dtype=np.int64).copy()
  rows = torch.empty(int(offs_np[-1]), dtype=torch.int32, device=dev)
  if rows.shape[0]:
    check(lib.pcmi_views_rows(ptr(mask), ptr(start), n, F, ptr(rows), cur_stream(dev)))
  return rows, offsets, offs_np, pixels, mask


# ---------------------------------------------------------------------------------------------------------------------
# Instance segmentation (csrc/cluster.hip; the rules are include/pcmi.h's): radius components of the shifted voxels, their
# compaction into instances, per-instance scores, overlap / matching for pcmi_det_ap, integer centroids, the offset losses.
# Only OffsetLossFunction is differentiable; nothing synchronises.
# ---------------------------------------------------------------------------------------------------------------------
def _xyz_rows(xyz, who):
  require_cuda(xyz, who)
  assert xyz.dim() == 2 and xyz.shape[1] == 3, "%s: [n, 3]" % who
  x = xyz if xyz.dtype == torch.float32 else xyz.float()
  return x if (x.stride(1) == 1 and x.stride(0) >= 3) or x.shape[0] == 0 else x.contiguous()


def radius_components(xyz, offsets, group, radius, dropped=None):
  """pcmi_radius_components: xyz float32 [n, 3] (rows may be a column slice), offsets [B + 1] (ascending row offsets of the
  scenes), group [n] -> label int32 [n]: the LOWEST row of the connected component of the row in the graph whose edges join
  rows of one scene and one group with (dx dx + dy dy) + dz dz <= radius radius in float64; -1 for a row outside every scene,
  with group < 0, a non-finite coordinate or |floor(x / radius)| >= 2^20.  dropped int64 [1] (optional) += the rows lost to
  the last condition."""
  x = _xyz_rows(xyz, "radius_components")
  dev = x.device
  offs, g = _offsets(offsets, dev), _i32c(group, dev).reshape(-1)
  n, B = x.shape[0], offs.shape[0] - 1
  assert offs.dim() == 1 and B >= 1 and g.shape[0] == n, "radius_components: offsets [B + 1], group [n]"
  assert dropped is None or (dropped.dtype == torch.int64 and dropped.numel() == 1 and dropped.device == dev), \
      "radius_components: dropped int64 [1]"
  label = torch.empty(n, dtype=torch.int32, device=dev)
  ws, wsb = ws_args(lib.pcmi_radius_components_workspace_bytes(n, B), dev)
  check(lib.pcmi_radius_components(ptr(x), x.stride(0) if n else 3, n, ptr(offs), B, ptr(g), float(radius), ptr(label), ptr(dropped),
                                   ws, wsb, cur_stream(dev)))
  return label


def components_compact(label, offsets, group, min_points, max_instances):
  """pcmi_components_compact: the components of label int32 [n] (radius_components') with at least min_points rows, numbered
  in ascending order of their lowest row -> a dict of device tensors: instance int32 [n] (-1: in none), count int32 [1] (the
  true number, even beyond max_instances: components numbered >= max_instances are written nowhere), and root, size, scene,
  group int32 [max_instances] (-1 / size 0 from the count on)."""
  require_cuda(label, "components_compact")
  dev = label.device
  lb, offs = _i32c(label, dev).reshape(-1), _offsets(offsets, dev)
  g = None if group is None else _i32c(group, dev).reshape(-1)
  n, B, M = lb.shape[0], offs.shape[0] - 1, int(max_instances)
  assert B >= 1 and (g is None or g.shape[0] == n), "components_compact: offsets [B + 1], group [n]"
  inst = torch.empty(n, dtype=torch.int32, device=dev)
  count = torch.empty(1, dtype=torch.int32, device=dev)
  root, size, scene, grp = (torch.empty(M, dtype=torch.int32, device=dev) for _ in range(4))
  ws, wsb = ws_args(lib.pcmi_components_compact_workspace_bytes(n), dev)
  check(lib.pcmi_components_compact(ptr(lb), ptr(offs), B, n, ptr(g), int(min_points), M, ptr(inst), ptr(count), ptr(root), ptr(size),
                                    ptr(scene), ptr(grp), ws, wsb, cur_stream(dev)))
  return dict(instance=inst, count=count, root=root, size=size, scene=scene, group=grp)


def instance_scores(score, instance, inst_size):
  """pcmi_instance_scores: the mean of score float32 [n] (clamped to [0, 1], non-finite -> 0) over the rows of each instance,
  exact in 2^-30 fixed point -> float64 [P], P = len(inst_size); 0 for an instance without rows."""
  s = _f32c(score, "instance_scores").reshape(-1)
  dev = s.device
  inst, size = _i32c(instance, dev).reshape(-1), _i32c(inst_size, dev).reshape(-1)
  n, P = s.shape[0], size.shape[0]
  assert inst.shape[0] == n, "instance_scores: score [n], instance [n]"
  out = torch.empty(P, dtype=torch.float64, device=dev)
  ws, wsb = ws_args(lib.pcmi_instance_scores_workspace_bytes(P), dev)
  check(lib.pcmi_instance_scores(ptr(s), ptr(inst), n, P, ptr(size), ptr(out), ws, wsb, cur_stream(dev)))
  return out


def instance_overlap(pred_instance, gt_instance, n_pred, n_gt):
  """pcmi_instance_overlap: pred_instance / gt_instance [n] -> (inter int32 [P, G], pred_size int32 [P], gt_size int32 [G]);
  ids outside [0, P) / [0, G) count nowhere."""
  require_cuda(pred_instance, "instance_overlap")
  dev = pred_instance.device
  p, g = _i32c(pred_instance, dev).reshape(-1), _i32c(gt_instance, dev).reshape(-1)
  P, G = int(n_pred), int(n_gt)
  assert p.shape == g.shape, "instance_overlap: pred_instance [n], gt_instance [n]"
  inter = torch.empty((P, G), dtype=torch.int32, device=dev)
  ps, gs = torch.empty(P, dtype=torch.int32, device=dev), torch.empty(G, dtype=torch.int32, device=dev)
  check(lib.pcmi_instance_overlap(ptr(p), ptr(g), p.shape[0], P, G, ptr(inter), ptr(ps), ptr(gs), cur_stream(dev)))
  return inter, ps, gs


def instance_match(inter, pred_size, gt_size, pred_scene, pred_class, gt_scene, gt_class):
  """pcmi_instance_match: per predicted instance the ground-truth instance of its scene and class with the largest
  inter / (pred_size + gt_size - inter) (float64, the lowest index of equal ones) -> (best_gt int32 [P], best_iou float32 [P]);
  -1 / -inf without one: what det_ap consumes."""
  require_cuda(inter, "instance_match")
  dev = inter.device
  it = _i32c(inter, dev)
  assert it.dim() == 2, "instance_match: inter [P, G]"
  P, G = it.shape
  ps, psc, pcl = (_i32c(t, dev).reshape(-1) for t in (pred_size, pred_scene, pred_class))
  gs, gsc, gcl = (_i32c(t, dev).reshape(-1) for t in (gt_size, gt_scene, gt_class))
  assert ps.shape[0] == psc.shape[0] == pcl.shape[0] == P and gs.shape[0] == gsc.shape[0] == gcl.shape[0] == G, \
      "instance_match: pred_* [P], gt_* [G]"
  best_gt = torch.empty(P, dtype=torch.int32, device=dev)
  best_iou = torch.empty(P, dtype=torch.float32, device=dev)
  check(lib.pcmi_instance_match(ptr(it), ptr(ps), ptr(gs), ptr(psc), ptr(pcl), ptr(gsc), ptr(gcl), P, G, ptr(best_gt), ptr(best_iou),
                                cur_stream(dev)))
  return best_gt, best_iou


def instance_centroids(coords, instance, n_instances):
  """pcmi_instance_centroids: coords int32 [n, 4] (b, x, y, z), instance [n] -> (sum int64 [G, 3], cnt int64 [G]): the exact
  sums of the voxel coordinates of each instance and their number."""
  require_cuda(coords, "instance_centroids")
  dev = coords.device
  assert coords.dim() == 2 and coords.shape[1] == 4, "instance_centroids: coords [n, 4]"
  c, inst = _i32c(coords, dev), _i32c(instance, dev).reshape(-1)
  n, G = c.shape[0], int(n_instances)
  assert inst.shape[0] == n, "instance_centroids: instance [n]"
  s, cnt = torch.empty((G, 3), dtype=torch.int64, device=dev), torch.empty(G, dtype=torch.int64, device=dev)
  check(lib.pcmi_instance_centroids(ptr(c), ptr(inst), n, G, ptr(s), ptr(cnt), cur_stream(dev)))
  return s, cnt


# ---------------------------------------------------------------------------------------------------------------------
# The input of instance-segmentation fine-tuning (csrc/insseg_input.hip; the rules are include/pcmi.h's): batch-unique
# instance indices from per-scene raw ids, the per-instance table, the per-scene crop.  Integer arithmetic, bit-exact against
# tests/insseg_input_ref.py.  offsets stays on the device and nothing synchronises: the arrays hold n rows of capacity and a
# row outside every scene is neither read nor written, so the calls chain behind seg_quantize before its counts are read.
# ---------------------------------------------------------------------------------------------------------------------
ROW_SCAN_BLOCK = 2048              # kScanBlock of csrc/rowscan.h: the rows one workgroup of the numbering scan covers
ROW_SCAN_LEVEL = 256 * 2048        # kThreads kScanBlock: the rows from which its second level takes another round
CROP_MAX_STEPS = 32                # kMaxSteps of insseg_input.hip


def instance_relabel(raw, offsets, keep=None):
  """pcmi_instance_relabel: raw int32 [n] (per-scene instance ids, any non-negative integers; the same id in two scenes is two
  instances), offsets [B + 1], keep uint8 / bool [n] (None: all).  A row with raw < 0 or keep == 0 is in no instance; instances
  are numbered in ascending order of their lowest row (components_compact's convention).  Returns a dict of device tensors:
  instance int32 [n] (-1: in none), first_row int32 [n] (the lowest row of instance g at g, valid up to the count), counts
  int64 [B + 1] (the instances that begin in each scene, then their sum)."""
  require_cuda(raw, "instance_relabel")
  dev = raw.device
  r, offs = _i32c(raw, dev).reshape(-1), _offsets(offsets, dev)
  n, B = r.shape[0], offs.shape[0] - 1
  kp = None if keep is None else keep.to(device=dev, dtype=torch.uint8).contiguous()
  assert offs.dim() == 1 and B >= 1 and (kp is None or kp.shape == (n,)), "instance_relabel: offsets [B + 1], keep [n]"
  inst = torch.empty(n, dtype=torch.int32, device=dev)
  first = torch.empty(n, dtype=torch.int32, device=dev)
  counts = torch.empty(B + 1, dtype=torch.int64, device=dev)
  ws, wsb = ws_args(lib.pcmi_instance_relabel_workspace_bytes(n), dev)
  check(lib.pcmi_instance_relabel(ptr(r), ptr(kp), ptr(offs), n, B, ptr(inst), ptr(first), ptr(counts), ws, wsb, cur_stream(dev)))
  return dict(instance=inst, first_row=first, counts=counts)


def instance_table(instance, klass, coords, offsets, n_instances):
  """pcmi_instance_table: instance [n], klass [n] or None, coords int32 [n, 4] or None, offsets [B + 1], G = n_instances (a
  host integer) -> a dict of device tensors per instance: size, scene int32 [G] (the largest scene among its rows, -1 without
  rows), cls int32 [G] (max(-1, max klass); None without klass), sum int64 [G, 3], box_min, box_max int32 [G, 3] (None without
  coords).  sum / size are instance_centroids' outputs; cls / scene what both instance evaluators derive (their table=)."""
  require_cuda(instance, "instance_table")
  dev = instance.device
  inst, offs = _i32c(instance, dev).reshape(-1), _offsets(offsets, dev)
  n, B, G = inst.shape[0], offs.shape[0] - 1, int(n_instances)
  kl = None if klass is None else _i32c(klass, dev).reshape(-1)
  c = None if coords is None else _i32c(coords, dev)
  assert offs.dim() == 1 and B >= 1 and G >= 0 and (kl is None or kl.shape[0] == n) and (c is None or c.shape == (n, 4)), \
      "instance_table: offsets [B + 1], klass [n], coords [n, 4]"
  size, scene = torch.empty(G, dtype=torch.int32, device=dev), torch.empty(G, dtype=torch.int32, device=dev)
  cls = None if kl is None else torch.empty(G, dtype=torch.int32, device=dev)
  s = None if c is None else torch.empty((G, 3), dtype=torch.int64, device=dev)
  lo, hi = (None, None) if c is None else (torch.empty((G, 3), dtype=torch.int32, device=dev) for _ in range(2))
  check(lib.pcmi_instance_table(ptr(inst), ptr(kl), ptr(c), ptr(offs), n, B, G, ptr(size), ptr(scene), ptr(cls), ptr(s), ptr(lo), ptr(hi),
                                cur_stream(dev)))
  return dict(size=size, scene=scene, cls=cls, sum=s, box_min=lo, box_max=hi)


def seg_crop_ladder(coords, offsets, axes, sides, draws, max_voxels, flags=None):
  """pcmi_seg_crop_ladder -- this project's own rule, in the spirit of PointGroup's crop, not a restatement, untuned.  coords
  int32 [n, 4] (seg_quantize's), offsets [B + 1] over its rows, axes: the two horizontal columns (1 ... 3), sides: [S, 2] host
  integers (window sides in voxels, each column non-increasing), draws uint32-valued [B, S, 2] (an int64 or int32 tensor of
  values in [0, 2^32)), max_voxels.  A scene above max_voxels rows takes the lowest step whose window holds at most max_voxels
  of its rows, else the last one and SEG_FLAG_CROP.  Returns a dict of device tensors: rows int64 [n] (the kept rows, ascending;
  0 beyond the count), counts int64 [B + 1], step int32 [B] (-1: not cropped), flags int32 [B] (ORed into the one passed in)."""
  import numpy as np
  require_cuda(coords, "seg_crop_ladder")
  dev = coords.device
  c, offs = _i32c(coords, dev), _offsets(offsets, dev)
  assert c.dim() == 2 and c.shape[1] == 4 and offs.dim() == 1 and offs.shape[0] >= 2, "seg_crop_ladder: coords [n, 4], offsets [B + 1]"
  n, B = c.shape[0], offs.shape[0] - 1
  sd = np.ascontiguousarray(np.asarray(sides, dtype=np.int64).reshape(-1, 2))
  assert np.all(np.abs(sd) < 2**31), "seg_crop_ladder: sides fit int32"
  sd, S = sd.astype(np.int32), sd.shape[0]
  d = torch.as_tensor(draws)
  if d.dtype != torch.int32:  # values in [0, 2^32) -> their 32 bits
    d = d.to(torch.int64).bitwise_and(0xFFFFFFFF)
    d = torch.where(d >= 2**31, d - 2**32, d).to(torch.int32)
  d = d.to(dev).contiguous()
  assert d.numel() == B * S * 2, "seg_crop_ladder: draws [B, S, 2]"
  flags = _seg_flags(flags, B, dev)
  rows = torch.zeros(n, dtype=torch.int64, device=dev)
  counts = torch.empty(B + 1, dtype=torch.int64, device=dev)
  step = torch.full((B,), -1, dtype=torch.int32, device=dev)
  ws, wsb = ws_args(lib.pcmi_seg_crop_ladder_workspace_bytes(n, B), dev)
  check(lib.pcmi_seg_crop_ladder(ptr(c), ptr(offs), n, B, int(axes[0]), int(axes[1]), sd.ctypes.data_as(C.POINTER(C.c_int32)), S, ptr(d),
                                 int(max_voxels), ptr(rows), ptr(counts), ptr(step), ptr(flags), ws, wsb, cur_stream(dev)))
  return dict(rows=rows, counts=counts, step=step, flags=flags)


# ---- instance masks by the benchmark protocol (csrc/insbench.hip): restated from the rules of ScanNet's script, never run
# against the script; include/pcmi.h states them ---------------------------------------------------------------------------------
def instance_void_overlap(pred_instance, gt_instance, gt_valid, n_pred):
  """pcmi_instance_void_overlap: pred_instance / gt_instance [n], gt_valid [G] (non-zero: a scored ground-truth instance) ->
  void_inter int32 [P]: the rows of each prediction whose ground-truth id is outside [0, G) or not valid; a prediction id
  outside [0, P) counts nowhere.  The overlap matrix beside it is instance_overlap's."""
  require_cuda(pred_instance, "instance_void_overlap")
  dev = pred_instance.device
  p, g, v = _i32c(pred_instance, dev).reshape(-1), _i32c(gt_instance, dev).reshape(-1), _i32c(gt_valid, dev).reshape(-1)
  assert p.shape == g.shape, "instance_void_overlap: pred_instance [n], gt_instance [n]"
  P = int(n_pred)
  out = torch.empty(P, dtype=torch.int32, device=dev)
  check(lib.pcmi_instance_void_overlap(ptr(p), ptr(g), ptr(v), p.shape[0], P, v.shape[0], ptr(out), cur_stream(dev)))
  return out


def instance_bench_match(inter, pred_size, gt_size, void_inter, pred_scene, pred_class, pred_score, gt_scene, gt_class, n_scenes,
                         num_classes, thresholds, min_region=100, npos=None):
  """pcmi_instance_bench_match: the benchmark protocol's matching of one batch.  inter int32 [P, G], pred_size [P], gt_size [G]
  (instance_overlap's), void_inter [P] (instance_void_overlap's), pred_scene / pred_class [P], pred_score float64 [P] (not
  NaN), gt_scene / gt_class [G] (class -1: not scored); thresholds: a sequence of at most 16 floats in [0.25, 1) (host).
  Returns (entry_flag int8 [T, P, 3]: -1 none, 0 false positive, 1 true positive, slot s = the prediction's s-th claim;
  gt_state int32 [T, G]: 1 matched, 0 counted and unmatched, -1 not counted; npos int32 [num_classes]: the counted ground
  truths ADDED to the tensor passed in, a fresh one otherwise).  No host synchronisation."""
  require_cuda(inter, "instance_bench_match")
  dev = inter.device
  it = _i32c(inter, dev)
  assert it.dim() == 2, "instance_bench_match: inter [P, G]"
  P, G = it.shape
  ps, vi, psc, pcl = (_i32c(t, dev).reshape(-1) for t in (pred_size, void_inter, pred_scene, pred_class))
  gs, gsc, gcl = (_i32c(t, dev).reshape(-1) for t in (gt_size, gt_scene, gt_class))
  score = _f64c(pred_score, dev, "instance_bench_match").reshape(-1)
  assert ps.shape[0] == vi.shape[0] == psc.shape[0] == pcl.shape[0] == score.shape[0] == P and \
      gs.shape[0] == gsc.shape[0] == gcl.shape[0] == G, "instance_bench_match: pred_* [P], gt_* [G]"
  T, Cls = len(thresholds), int(num_classes)
  thr = (C.c_double * max(T, 1))(*[float(t) for t in thresholds])
  if npos is None:
    npos = torch.zeros(Cls, dtype=torch.int32, device=dev)
  assert npos.dtype == torch.int32 and npos.shape == (Cls,) and npos.is_contiguous() and npos.device == dev, \
      "instance_bench_match: npos int32 [num_classes] on inter's device"
  flag = torch.empty((T, P, 3), dtype=torch.int8, device=dev)
  state = torch.empty((T, G), dtype=torch.int32, device=dev)
  check(lib.pcmi_instance_bench_match(ptr(it), ptr(ps), ptr(gs), ptr(vi), ptr(psc), ptr(pcl), ptr(score), ptr(gsc), ptr(gcl), P, G,
                                      int(n_scenes), Cls, int(min_region), thr, T, ptr(flag), ptr(state), ptr(npos), cur_stream(dev)))
  return flag, state, npos


def instance_bench_ap(entry_flag, score, cls_offs, npos, curves=False):
  """pcmi_instance_bench_ap.  entry_flag int8 [T, E] / score float64 [E]: the entries class by class in descending score, class
  c at [cls_offs[c], cls_offs[c + 1]) (int32 [Cls + 1]); flags of -1 are skipped; npos int32 [Cls].  Returns a dict of device
  tensors: ap float64 [T, Cls] (NaN where npos is 0) in the benchmark script's convolution form, equal scores forming one
  group, and with curves prec, rec float64 [T, E]: the curve at the last entry of each group, NaN elsewhere.  No host
  synchronisation."""
  require_cuda(entry_flag, "instance_bench_ap")
  dev = entry_flag.device
  fl = entry_flag.to(torch.int8).contiguous()
  assert fl.dim() == 2, "instance_bench_ap: entry_flag [T, E]"
  T, E = fl.shape
  sc, offs, np_ = _f64c(score, dev, "instance_bench_ap").reshape(-1), _i32c(cls_offs, dev), _i32c(npos, dev)
  Cls = np_.shape[0]
  assert sc.shape[0] == E and offs.shape == (Cls + 1,), "instance_bench_ap: score [E], cls_offs [Cls + 1], npos [Cls]"
  ap = torch.empty((T, Cls), dtype=torch.float64, device=dev)
  prec = torch.empty((T, E), dtype=torch.float64, device=dev) if curves else None
  rec = torch.empty((T, E), dtype=torch.float64, device=dev) if curves else None
  ws, wsb = ws_args(lib.pcmi_instance_bench_ap_workspace_bytes(E, Cls, T), dev)
  check(lib.pcmi_instance_bench_ap(ptr(fl), ptr(sc), ptr(offs), ptr(np_), E, Cls, T, ptr(ap), ptr(prec), ptr(rec), ws, wsb, cur_stream(dev)))
  return dict(ap=ap, prec=prec, rec=rec)


# ---- dual-set instance proposals (csrc/proposals.hip; the rules are include/pcmi.h's): overlapping proposals as a membership
# matrix, their pairwise intersections per scene, non-maximum suppression on mask IoU.  Nothing synchronises. ---------------------
PROPOSAL_MAX_SETS = 4         # kMaxSets of proposals.hip
PROPOSAL_MAX_PER_SCENE = 1024  # kMaxK


def _member_rows(member, who):
  require_cuda(member, who)
  assert member.dim() == 2 and 1 <= member.shape[1] <= PROPOSAL_MAX_SETS, "%s: member [n, S], 1 <= S <= %d" % (who, PROPOSAL_MAX_SETS)
  m = member if member.dtype == torch.int32 else member.to(torch.int32)
  return m if (m.stride(1) == 1 and m.stride(0) >= m.shape[1]) or m.shape[0] == 0 else m.contiguous()


def proposal_overlap(member, prop_scene, n_scenes, max_per_scene=PROPOSAL_MAX_PER_SCENE, dropped=None):
  """pcmi_proposal_overlap: member int32 [n, S] (column s: one partition of the rows into proposals, -1 none; may be a column
  slice of a wider tensor), prop_scene [P] (outside [0, n_scenes): an unused slot), max_per_scene: a host bound <= 1024 on the
  proposals of one scene -> a dict of device tensors: size int32 [P] (the entries of member naming p), local int32 [P] (the
  proposal's index within its scene in ascending slot order; -1 unused, or beyond max_per_scene), scene_count int32 [B] (the
  used slots of each scene, the true number), inter int32 [B, Kmax, Kmax] (the rows naming both proposals in two different
  columns, by local index: symmetric, zero diagonal).  dropped int64 [1] (optional) += the proposals beyond max_per_scene."""
  m = _member_rows(member, "proposal_overlap")
  dev = m.device
  sc = _i32c(prop_scene, dev).reshape(-1)
  n, S, P, B, K = m.shape[0], m.shape[1], sc.shape[0], int(n_scenes), int(max_per_scene)
  assert dropped is None or (dropped.dtype == torch.int64 and dropped.numel() == 1 and dropped.device == dev), \
      "proposal_overlap: dropped int64 [1]"
  size, local = torch.empty(P, dtype=torch.int32, device=dev), torch.empty(P, dtype=torch.int32, device=dev)
  count = torch.empty(max(B, 0), dtype=torch.int32, device=dev)
  ok = B >= 1 and 1 <= K <= PROPOSAL_MAX_PER_SCENE and B * K * K < 2**31  # (the call refuses anything else before it touches inter)
  inter = torch.empty((B, K, K) if ok else (0, 0, 0), dtype=torch.int32, device=dev)
  ws, wsb = ws_args(lib.pcmi_proposal_overlap_workspace_bytes(P), dev)
  check(lib.pcmi_proposal_overlap(ptr(m), m.stride(0) if n else S, n, S, ptr(sc), P, B, K, ptr(size), ptr(local), ptr(count), ptr(inter),
                                  ptr(dropped), ws, wsb, cur_stream(dev)))
  return dict(size=size, local=local, scene_count=count, inter=inter)


def proposal_nms(overlap, prop_scene, prop_class, score, nms_iou, min_score=0.0):
  """pcmi_proposal_nms: overlap = proposal_overlap's dict for the same prop_scene; prop_class int32 [P], score float64 [P] ->
  keep int32 [P]: per scene, the candidates (local >= 0, size >= 1, class >= 0, a finite score >= min_score) in descending score
  (equal scores: ascending slot); one still alive is kept and clears every later one with inter / (size_i + size_j - inter) >
  nms_iou in float64 (strict; classes are not looked at).  0 for every slot that is not kept."""
  inter = overlap["inter"]
  require_cuda(inter, "proposal_nms")
  dev = inter.device
  assert inter.dim() == 3 and inter.shape[1] == inter.shape[2] and inter.dtype == torch.int32 and inter.is_contiguous(), \
      "proposal_nms: inter int32 [B, Kmax, Kmax]"
  B, K = inter.shape[0], inter.shape[1]
  size, local, count = (_i32c(overlap[k], dev).reshape(-1) for k in ("size", "local", "scene_count"))
  sc, cl = _i32c(prop_scene, dev).reshape(-1), _i32c(prop_class, dev).reshape(-1)
  s = _f64c(score, dev, "proposal_nms").reshape(-1)
  P = sc.shape[0]
  assert size.shape[0] == local.shape[0] == cl.shape[0] == s.shape[0] == P and count.shape[0] == B, \
      "proposal_nms: size, local, prop_scene, prop_class, score [P], scene_count [B]"
  keep = torch.empty(P, dtype=torch.int32, device=dev)
  check(lib.pcmi_proposal_nms(ptr(inter), ptr(size), ptr(local), ptr(count), ptr(sc), ptr(cl), ptr(s), P, B, K, float(nms_iou),
                              float(min_score), ptr(keep), cur_stream(dev)))
  return keep


class OffsetLossFunction(Function):
  """PointGroup's two offset losses (pcmi_offset_loss_fwd / _bwd): pred float32 [n, 3] (may be a column slice of the logits),
  target float32 [n, 3], instance [n] (a row counts iff instance >= 0) -> (norm_loss, dir_loss), float64 scalars."""

  @staticmethod
  def forward(ctx, pred, target, instance):
    require_cuda(pred, "offset loss")
    assert pred.dim() == 2 and pred.shape[1] == 3 and target.shape == pred.shape, "offset loss: pred [n, 3], target [n, 3]"
    p = pred if (pred.stride(1) == 1 and pred.dtype == torch.float32 and pred.stride(0) >= 3) else pred.float().contiguous()
    dev = p.device
    g, inst = _f32c(target.to(dev), "offset loss"), _i32c(instance, dev).reshape(-1)
    n = p.shape[0]
    assert inst.shape[0] == n, "offset loss: instance [n]"
    out3 = torch.empty(3, dtype=torch.float64, device=dev)
    ws, wsb = ws_args(lib.pcmi_offset_loss_workspace_bytes(n), dev)
    check(lib.pcmi_offset_loss_fwd(ptr(p), p.stride(0) if n else 3, ptr(g), ptr(inst), n, ptr(out3), ws, wsb, cur_stream(dev)))
    ctx.save_for_backward(p, g, inst, out3)
    return out3[0], out3[1]

  @staticmethod
  @once_differentiable
  def backward(ctx, gnorm, gdir):
    p, g, inst, out3 = ctx.saved_tensors
    n, dev = p.shape[0], p.device
    gl = torch.stack([gnorm.reshape(()), gdir.reshape(())]).to(device=dev, dtype=torch.float64).contiguous()
    dp = torch.empty((n, 3), dtype=torch.float32, device=dev)
    check(lib.pcmi_offset_loss_bwd(ptr(p), p.stride(0) if n else 3, ptr(g), ptr(inst), n, ptr(out3), ptr(gl), ptr(dp), 3, cur_stream(dev)))
    return dp, None, None


# ---- active labelling: batched k-means on features (csrc/kmeans.hip) ----------------------------------------------------------
KMEANS_MAX_K, KMEANS_MAX_SCENE_ROWS = 1024, 1 << 20


class KMeansDraws:
  """The uint64 draws [B, K] of the k-means++ seeding (column k: the draw of step k), kept as the int64 tensor with the same
  bits.  Every random quantity of kmeans_select is in here: the same draws give the same rows."""

  def __init__(self, bits):
    import numpy as np
    if not torch.is_tensor(bits):
      a = np.asarray(bits)
      bits = torch.from_numpy(np.ascontiguousarray(a.astype(np.uint64) if a.dtype != np.int64 else a).view(np.int64))
    assert bits.dim() == 2 and bits.dtype == torch.int64, "KMeansDraws: uint64 [B, K] (or an int64 tensor holding those bits)"
    self.bits = bits

  @staticmethod
  def sample(B, K, generator=None):
    """Uniform draws from torch.randint over the int64 range, whose upper bound is exclusive: the bit pattern 2^63 - 1 is
    never drawn (one of the 2^64 values; a target moves by at most total / 2^64 < 1 weight unit)."""
    return KMeansDraws(torch.randint(-(1 << 63), (1 << 63) - 1, (int(B), int(K)), dtype=torch.int64, generator=generator))

  def to(self, device):
    return self.bits.to(device).contiguous()


def _km_feat(feat, who):
  """float32 [n, C] rows the kernels take as they are (a column slice with a stride of a multiple of 4 floats too); a width
  that is not a multiple of 16 is zero-padded (zeros add nothing to a distance)."""
  require_cuda(feat, who)
  assert feat.dim() == 2 and feat.dtype == torch.float32, "%s: float32 [n, C] features" % who
  c = feat.shape[1]
  cp = pad_width(c, 16)
  if cp != c:
    padded = torch.zeros((feat.shape[0], cp), dtype=torch.float32, device=feat.device)
    padded[:, :c] = feat
    return padded
  return _c(feat) if feat.shape[0] else feat.contiguous()


def _km_scene_rows(offsets, n, max_scene_rows):
  """The bound on the rows of a scene that the C calls take: the largest segment where the offsets are on the host; for
  offsets on the device min(n, 2^20) without looking at them (a longer scene is cut to its first 2^20 rows; the rows cut off
  get assign = -1 and are counted in `skipped`, so the cut shows in what the caller reads back)."""
  if max_scene_rows is not None:
    return int(max_scene_rows)
  if _on_host(offsets):
    import numpy as np
    o = np.asarray(offsets, dtype=np.int64).reshape(-1)
    return int(max(0, np.diff(o).max())) if o.shape[0] >= 2 else 0
  return min(int(n), KMEANS_MAX_SCENE_ROWS)


def _km_common(feat, offsets, max_scene_rows, who):
  f = _km_feat(feat, who)
  offs = _offsets(offsets, f.device)
  assert offs.dim() == 1 and offs.shape[0] >= 2, "%s: offsets [B + 1]" % who
  n = f.shape[0]
  return f, offs, n, offs.shape[0] - 1, f.shape[1], f.stride(0) if n else f.shape[1], _km_scene_rows(offsets, n, max_scene_rows)


def kmeans_init(feat, offsets, init_rows, max_scene_rows=None):
  """pcmi_kmeans_init: the centroids of all scenes from the feature rows init_rows int32 [B, K] (global rows; -1: a dead
  cluster).  Returns (centroid float32 [B, K, C], live int32 [B, K]: init_rows with every row outside its scene or inactive
  replaced by -1, flags int64 [B]: how many were replaced).  No synchronisation."""
  f, offs, n, B, c, ld, msr = _km_common(feat, offsets, max_scene_rows, "kmeans_init")
  rows = _i32c(torch.as_tensor(init_rows), f.device)
  assert rows.dim() == 2 and rows.shape[0] == B, "kmeans_init: init_rows [B, K]"
  K = rows.shape[1]
  cen = torch.empty((B, K, c), dtype=torch.float32, device=f.device)
  live = torch.empty((B, K), dtype=torch.int32, device=f.device)
  flags = torch.empty(B, dtype=torch.int64, device=f.device)
  check(lib.pcmi_kmeans_init(ptr(f), ld, n, ptr(offs), B, K, c, msr, ptr(rows), ptr(cen), ptr(live), ptr(flags), cur_stream(f.device)))
  return cen, live, flags


def kmeans_step(feat, offsets, centroid, live, assign_prev=None, max_scene_rows=None):
  """pcmi_kmeans_step: one Lloyd iteration of all scenes -- assignment against centroid [B, K, C] and the fixed-point sums in
  one pass over feat.  Returns a dict: assign int32 [n] (-1: inactive), sum int64 [B, K, C] (2^-32 fixed point), cnt int32
  [B, K], centroid float32 [B, K, C] (the new ones), changed int64 [B] (against assign_prev; None: all -1), skipped int64 [B].
  No synchronisation; bit-identical from run to run."""
  f, offs, n, B, c, ld, msr = _km_common(feat, offsets, max_scene_rows, "kmeans_step")
  dev = f.device
  cen, lv = _f32c(centroid, "kmeans_step"), _i32c(live, dev)
  assert cen.dim() == 3 and cen.shape[0] == B and cen.shape[2] == c and lv.shape == cen.shape[:2], \
      "kmeans_step: centroid [B, K, C] of the (padded) feature width, live [B, K]"
  K = cen.shape[1]
  prev = None if assign_prev is None else _i32c(assign_prev, dev).reshape(-1)
  assert prev is None or prev.shape[0] == n, "kmeans_step: assign_prev [n]"
  assign = torch.empty(n, dtype=torch.int32, device=dev)
  s = torch.empty((B, K, c), dtype=torch.int64, device=dev)
  cnt = torch.empty((B, K), dtype=torch.int32, device=dev)
  out = torch.empty((B, K, c), dtype=torch.float32, device=dev)
  changed, skipped = torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.int64, device=dev)
  check(lib.pcmi_kmeans_step(ptr(f), ld, n, ptr(offs), B, K, c, msr, ptr(cen), ptr(lv), ptr(prev), ptr(assign), ptr(s), ptr(cnt),
                             ptr(out), ptr(changed), ptr(skipped), cur_stream(dev)))
  return dict(assign=assign, sum=s, cnt=cnt, centroid=out, changed=changed, skipped=skipped)


def kmeans_assign(feat, offsets, centroid, live, max_scene_rows=None):
  """pcmi_kmeans_assign: the final pass.  Returns a dict: assign int32 [n], d2 float32 [n] (NaN: inactive), nearest int32
  [B, K] (the global row of the member nearest to its centre, the lowest among equals; -1: no member), inertia float64 [B],
  cnt int32 [B, K], skipped int64 [B].  assign / d2 equal feature_nn(feat, offsets, centroids of the live clusters) bit for
  bit.  No synchronisation."""
  f, offs, n, B, c, ld, msr = _km_common(feat, offsets, max_scene_rows, "kmeans_assign")
  dev = f.device
  cen, lv = _f32c(centroid, "kmeans_assign"), _i32c(live, dev)
  assert cen.dim() == 3 and cen.shape[0] == B and cen.shape[2] == c and lv.shape == cen.shape[:2], \
      "kmeans_assign: centroid [B, K, C] of the (padded) feature width, live [B, K]"
  K = cen.shape[1]
  assign, d2 = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
  nearest, cnt = torch.empty((B, K), dtype=torch.int32, device=dev), torch.empty((B, K), dtype=torch.int32, device=dev)
  inertia, skipped = torch.empty(B, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.int64, device=dev)
  ws, wsb = ws_args(lib.pcmi_kmeans_assign_workspace_bytes(B, K), dev)
  check(lib.pcmi_kmeans_assign(ptr(f), ld, n, ptr(offs), B, K, c, msr, ptr(cen), ptr(lv), ptr(assign), ptr(d2), ptr(nearest),
                               ptr(inertia), ptr(cnt), ptr(skipped), ws, wsb, cur_stream(dev)))
  return dict(assign=assign, d2=d2, nearest=nearest, inertia=inertia, cnt=cnt, skipped=skipped)


def kmeans_pp_step(feat, offsets, mind2, last, draw, max_scene_rows=None):
  """pcmi_kmeans_pp_step: one step of k-means++ seeding for all scenes.  mind2 float32 [n] is lowered IN PLACE to the distance
  to the centres `last` int32 [B] (None / -1: nothing to lower -- the first step, with mind2 = +inf, picks uniformly among the
  active rows); draw: uint64 [B] as int64 bits.  Returns next int32 [B] (global rows; -1: no active row).  No synchronisation."""
  f, offs, n, B, c, ld, msr = _km_common(feat, offsets, max_scene_rows, "kmeans_pp_step")
  dev = f.device
  assert torch.is_tensor(mind2) and mind2.is_cuda and mind2.dtype == torch.float32 and mind2.is_contiguous() and mind2.shape == (n,), \
      "kmeans_pp_step: mind2 float32 [n] on the device (updated in place)"
  lst = None if last is None else _i32c(last, dev).reshape(-1)
  dr = torch.as_tensor(draw).to(device=dev, dtype=torch.int64).contiguous().reshape(-1)
  assert dr.shape[0] == B and (lst is None or lst.shape[0] == B), "kmeans_pp_step: last [B], draw [B]"
  nxt = torch.empty(B, dtype=torch.int32, device=dev)
  ws, wsb = ws_args(lib.pcmi_kmeans_pp_step_workspace_bytes(B), dev)
  check(lib.pcmi_kmeans_pp_step(ptr(f), ld, n, ptr(offs), B, c, msr, ptr(lst), ptr(dr), ptr(mind2), ptr(nxt), ws, wsb, cur_stream(dev)))
  return nxt


def kmeans_pp_init(feat, offsets, K, draws, max_scene_rows=None):
  """k-means++ seeding of all scenes: K kmeans_pp_step calls, no read-back.  draws: KMeansDraws (or its int64 bits) [B, K].
  Returns init_rows int32 [B, K]; a row picked a second time (only when no weight is left: fewer distinct active rows than
  K) is -1, a dead cluster."""
  f = _km_feat(feat, "kmeans_pp_init")
  dev = f.device
  bits = (draws if isinstance(draws, KMeansDraws) else KMeansDraws(draws)).to(dev)
  K = int(K)
  assert bits.shape[1] >= K, "kmeans_pp_init: draws [B, >= K]"
  msr = _km_scene_rows(offsets, f.shape[0], max_scene_rows)
  offs = _offsets(offsets, dev)
  mind2 = torch.full((f.shape[0],), float("inf"), dtype=torch.float32, device=dev)
  picks, last = [], None
  for k in range(K):
    last = kmeans_pp_step(f, offs, mind2, last, bits[:, k], msr)
    picks.append(last)
  rows = torch.stack(picks, 1)
  again = (rows[:, :, None] == rows[:, None, :]) & torch.ones((K, K), dtype=torch.bool, device=dev).tril(-1)
  return torch.where(again.any(2), torch.full_like(rows, -1), rows)


def kmeans_select(feat, offsets, K, draws=None, iters=10, init_rows=None, max_scene_rows=None):
  """Active labelling of a batch of scenes: k-means++ seeding (or init_rows int32 [B, K]), `iters` Lloyd iterations and the
  final pass, all on the device with one read-back at the end (`rows`).  Returns a dict: rows int32 [B, K] ON THE HOST (the
  row to annotate per cluster: the member nearest to its centre; -1 for a cluster that is dead or stayed empty), and on the
  device assign int32 [n], centroid float32 [B, K, C], cnt int32 [B, K], inertia float64 [B], changed int64 [iters, B],
  skipped int64 [B], live int32 [B, K].  draws None: sampled from torch's default generator."""
  f = _km_feat(feat, "kmeans_select")
  dev = f.device
  offs = _offsets(offsets, dev)
  B, K = offs.shape[0] - 1, int(K)
  msr = _km_scene_rows(offsets, f.shape[0], max_scene_rows)
  if init_rows is None:
    init_rows = kmeans_pp_init(f, offs, K, KMeansDraws.sample(B, K) if draws is None else draws, msr)
  cen, live, _ = kmeans_init(f, offs, init_rows, msr)
  prev, changed = None, []
  for _ in range(int(iters)):
    st = kmeans_step(f, offs, cen, live, prev, msr)
    cen, prev = st["centroid"], st["assign"]
    changed.append(st["changed"])
  fin = kmeans_assign(f, offs, cen, live, msr)
  return dict(rows=fin["nearest"].cpu(), assign=fin["assign"], centroid=cen, cnt=fin["cnt"], inertia=fin["inertia"],
              changed=torch.stack(changed) if changed else torch.zeros((0, B), dtype=torch.int64, device=dev),
              skipped=fin["skipped"], live=live)
