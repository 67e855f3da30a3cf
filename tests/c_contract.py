"""Helpers of tests/test_gpu_c_contract.py: libpcmi's C entry points driven directly through ctypes, the way a C caller
and the native executor (csrc/engine.hip) drive them -- workspaces of exactly the queried size, rows with a leading
dimension larger than their width at a column offset of a wider buffer -- with guard bands and sentinels that turn an
overrun into a failed assertion (every band lies inside the allocation it guards: an overrun is detected, never a fault).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import surface_coords

DEV = "cuda:0"
GUARD = 64 << 10          # bytes of each guard band
GUARD_BYTE = 0xA5
SENTINEL_BITS = 0x7FC0BEEF  # a quiet NaN with a payload no kernel produces; compared as int32 bits

PCMI_OK, PCMI_ERR_INVALID, PCMI_ERR_WORKSPACE = 0, -1, -7


def align256(n):
  return (int(n) + 255) // 256 * 256


class Guarded:
  """`nbytes` of device memory between two guard bands of one allocation: G + align256(nbytes) + G bytes."""

  def __init__(self, nbytes, device=DEV):
    self.nbytes = int(nbytes)
    inner = align256(self.nbytes)
    # (the allocator's own alignment is not assumed: up to 255 bytes of slack bring the inner pointer to 256)
    self.buf = torch.empty(GUARD + inner + GUARD + 256, dtype=torch.uint8, device=device)
    self.lead = GUARD + (-(self.buf.data_ptr() + GUARD)) % 256
    self.inner = inner
    self.buf.fill_(GUARD_BYTE)
    self.ptr = self.buf.data_ptr() + self.lead
    assert self.ptr % 256 == 0

  @property
  def vp(self):
    return C.c_void_p(self.ptr)

  @property
  def size(self):
    return C.c_size_t(self.nbytes)

  def view(self, dtype, numel):
    """The first numel elements of the inner region as a tensor (for outputs kept in a guarded buffer)."""
    nb = numel * torch.empty(0, dtype=dtype).element_size()
    assert nb <= self.inner
    return self.buf[self.lead:self.lead + nb].view(dtype)

  def check(self, what=""):
    """Both bands -- and the alignment slack behind the last queried byte -- still hold the pattern."""
    lo = self.buf[:self.lead]
    hi = self.buf[self.lead + self.nbytes:]
    bad_lo = int((lo != GUARD_BYTE).sum())
    bad_hi = int((hi != GUARD_BYTE).sum())
    first = int((hi != GUARD_BYTE).nonzero()[0]) if bad_hi else -1
    assert bad_lo == 0 and bad_hi == 0, "%s: %d bytes written below and %d bytes beyond %d bytes (first at +%d)" % (
        what, bad_lo, bad_hi, self.nbytes, first)


def guarded(nbytes, device=DEV):
  g = Guarded(nbytes, device)
  return g.ptr, g.nbytes, g


class Strided:
  """A [rows, ld] fp32 buffer filled with the sentinel whose columns [col_off, col_off + c) are the tensor a call reads
  or writes: `view` is that [rows, c] slice (stride ld).  The buffer itself sits between guard bands."""

  def __init__(self, rows, c, ld, col_off, fill=None, device=DEV):
    assert ld % 4 == 0 and col_off % 4 == 0 and col_off + c <= ld, "documented requirement: ld % 4 == 0, 16-byte aligned rows"
    self.rows, self.c, self.ld, self.col_off = int(rows), int(c), int(ld), int(col_off)
    self.g = Guarded(max(self.rows * self.ld, 1) * 4, device)
    self.full = self.g.view(torch.int32, self.rows * self.ld).view(self.rows, self.ld)
    self.full.fill_(SENTINEL_BITS)
    self.view = self.full.view(torch.float32)[:, self.col_off:self.col_off + self.c]
    if fill is not None:
      self.view.copy_(torch.as_tensor(fill, dtype=torch.float32).to(device))

  @property
  def vp(self):
    return C.c_void_p(self.view.data_ptr())

  def cpu(self):
    return self.view.detach().cpu().clone()

  def check(self, what=""):
    outside = torch.ones(self.ld, dtype=torch.bool, device=self.full.device)
    outside[self.col_off:self.col_off + self.c] = False
    bad = int((self.full[:, outside] != SENTINEL_BITS).sum())
    assert bad == 0, "%s: %d elements outside columns [%d, %d) of ld %d were written" % (
        what, bad, self.col_off, self.col_off + self.c, self.ld)
    self.g.check(what)

  def untouched(self):
    """True if the view itself still holds the sentinel everywhere (a refused call wrote nothing)."""
    return bool((self.full == SENTINEL_BITS).all())


def strided(rows, c, ld, col_off, fill=None, device=DEV):
  return Strided(rows, c, ld, col_off, fill, device)


def lds(c, form):
  """The two column-slice forms of the module: (ld, col_off) = (c + 32, 4) and (2 c, c), c rounded up to a multiple of 4
  (rows must start 16-byte aligned)."""
  c4 = (c + 3) // 4 * 4
  return (c4 + 32, 4) if form == 0 else (2 * c4, c4)


_BASES = {}


def coords_with_rows(n, base="mid"):
  """The first n rows of a fixed surface_coords set (any subset of unique voxels is a valid input): a stride-1 map has
  exactly n output rows."""
  if base not in _BASES:
    _BASES[base] = surface_coords(72, 2, seed=3) if base == "mid" else surface_coords(110, 2, seed=4)
  b = _BASES[base]
  assert n <= len(b)
  return np.ascontiguousarray(b[:n])


def conv_ref64(x, W, pair_in, pair_out, offs, n_out, transpose=False, gout=None, bias=None):
  """Forward, backward-data and backward-weight of one sparse convolution in float64 on the CPU from the exported pair
  lists of the map (grouped by offset, `offs` their K + 1 prefix): index_add_ per offset.
  transpose: the pairs are used the other way round (in = the map's output rows), same weight slice.
  Returns out, and with gout: (out, gin, gW, gbias)."""
  x, W = x.double(), W.double()
  pi, po = pair_in.long(), pair_out.long()
  if transpose:
    pi, po = po, pi
  K = W.shape[0]
  out = torch.zeros(n_out, W.shape[2], dtype=torch.float64)
  for k in range(K):
    a, b = int(offs[k]), int(offs[k + 1])
    if b > a:
      out.index_add_(0, po[a:b], x[pi[a:b]] @ W[k])
  if bias is not None:
    out += bias.double()
  if gout is None:
    return out
  g = gout.double()
  gin = torch.zeros_like(x)
  gW = torch.zeros_like(W)
  for k in range(K):
    a, b = int(offs[k]), int(offs[k + 1])
    if b > a:
      gk = g[po[a:b]]
      gin.index_add_(0, pi[a:b], gk @ W[k].t())
      gW[k] = x[pi[a:b]].t() @ gk
  return out, gin, gW, g.sum(0)


def bn_ref64(x, gamma, beta, eps, res, relu, dy, relu_mask=None):
  """Training-mode BatchNorm (+ residual, + ReLU) and its gradients in float64 (torch autograd on the CPU).
  relu_mask: the device's ReLU pattern (its forward output > 0).  pcmi.h defines the backward pass through it
  ("relu_mask_y ... whose sign gives the ReLU mask"), and among millions of activations a few lie within round-off of
  zero, where fp32 and float64 may fall on different sides of the kink: both sides must differentiate the same
  piecewise-linear function.  `flipped_max` = the largest |pre-activation| at which the patterns differ."""
  x64 = x.double().requires_grad_(True)
  g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
  r64 = res.double().requires_grad_(True) if res is not None else None
  mean, var = x64.mean(0), x64.var(0, unbiased=False)
  pre = (x64 - mean) / torch.sqrt(var + eps) * g64 + b64
  if r64 is not None:
    pre = pre + r64
  y_free = torch.relu(pre.detach()) if relu else pre.detach()
  flipped_max = 0.0
  if relu and relu_mask is not None:
    differ = relu_mask != (pre.detach() > 0)
    flipped_max = float(pre.detach().abs()[differ].max()) if bool(differ.any()) else 0.0
    y = pre * relu_mask.double()
  else:
    y = torch.relu(pre) if relu else pre
  y.backward(dy.double())
  n = x.shape[0]
  return dict(y=y_free, mean=mean.detach(), var=var.detach(), unbiased=(var * n / max(n - 1, 1)).detach(), dx=x64.grad,
              dgamma=g64.grad, dbeta=b64.grad, dres=r64.grad if r64 is not None else None, flipped_max=flipped_max)


# ---- a workspace of exactly the queried size, and one byte less, under the Python wrappers ---------------------------------------
class _ExactWorkspace:
  """Stands in for runtime.ws_args: every call gets a guarded buffer of exactly the queried size, the `short_at`-th one a byte
  less.  `untouched()`: no byte of any buffer, guard bands included, was written."""

  def __init__(self, short_at=None):
    self.short_at, self.bufs = short_at, []

  def __call__(self, nbytes, device):
    g = Guarded(nbytes, device)
    short = 1 if self.short_at == len(self.bufs) else 0
    self.bufs.append(g)
    return g.vp, C.c_size_t(g.nbytes - short)

  def check(self):
    torch.cuda.synchronize()
    assert self.bufs and all(g.nbytes > 0 for g in self.bufs)
    for g in self.bufs:
      g.check("workspace of %d bytes" % g.nbytes)

  def untouched(self):
    torch.cuda.synchronize()
    return all(bool((g.buf == GUARD_BYTE).all()) for g in self.bufs)


@pytest.fixture
def exact_ws(monkeypatch):
  """installs an _ExactWorkspace wherever the wrappers look ws_args up; restore=True puts the shared workspace back"""
  from pointcontrast_amd import functional, runtime
  from pointcontrast_amd.lib import device_loader

  def install(short_at=None, restore=False):
    monkeypatch.undo()
    if restore:
      return None
    ws = _ExactWorkspace(short_at)
    for mod in (functional, runtime, device_loader):
      monkeypatch.setattr(mod, "ws_args", ws)
    return ws
  return install


def _pcmi_error():
  from pointcontrast_amd._lib import PcmiError
  return PcmiError


def _exact_and_short(exact_ws, run, same, calls=1, short_at=(0,)):
  """run() with the wrappers' shared (generous) workspace, with exactly the queried bytes, and with one byte less at call k"""
  want = run()
  ws = exact_ws()
  got = run()
  ws.check()
  assert len(ws.bufs) == calls
  same(got, want)
  for k in short_at:
    ws = exact_ws(short_at=k)
    with pytest.raises(_pcmi_error(), match="error -7"):
      run()
    assert len(ws.bufs) == k + 1 and bool((ws.bufs[k].buf == GUARD_BYTE).all()), "the refused call wrote nothing"
  exact_ws(restore=True)


def _same_arrays(got, want):
  assert len(got) == len(want)
  for g, w in zip(got, want):
    assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()
