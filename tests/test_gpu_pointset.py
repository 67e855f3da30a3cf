"""The PointNet++ point-set ops (csrc/pointset.hip, pointcontrast_amd.pointnet2_utils, downstream.votenet.sample_seeds) on the
MI355X against tests/pointset_ref.py: index outputs exactly, float outputs within 1e-4 of float64 relative to the tensor's
largest entry (the bound every kernel of this library is held to), backward passes bit-identical between two runs."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointset_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-4


def _cloud(rng, n, scale=2.0):
  return ((rng.rand(n, 3).astype(np.float32) - 0.5) * scale + 1.5).astype(np.float32)  # outside the origin's 1e-3 ball


def _dev(a, dtype=None):
  t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
  return t if dtype is None else t.to(dtype)


# ---- furthest point sampling ------------------------------------------------------------------------------------------------
def test_fps_dense_sizes():
  from pointcontrast_amd import pointnet2_utils as P
  rng = np.random.RandomState(0)
  n_cases = 0
  for n in (1, 63, 64, 65, 1000, 4097, 40000):
    xyz = np.stack([_cloud(rng, n), _cloud(rng, n)])
    for m in (1, 16, 1024):
      got = P.furthest_point_sample(_dev(xyz), m)
      assert got.dtype == torch.int32 and got.shape == (2, m) and not got.requires_grad
      want = np.stack([R.fps(xyz[b], m, tie_free=m <= n) for b in range(2)])
      assert (got.cpu().numpy() == want).all(), "fps n=%d m=%d: %d picks differ" % (n, m, int((got.cpu().numpy() != want).sum()))
      n_cases += 1
  assert n_cases == 21


def test_fps_ties_padding_and_more_picks_than_points():
  from pointcontrast_amd import pointnet2_utils as P
  rng = np.random.RandomState(1)
  dup = np.tile(_cloud(rng, 37), (9, 1))  # every point nine times: each pick is a tie, the lowest index wins
  pad = _cloud(rng, 500)
  pad[rng.choice(500, 200, replace=False)] = (rng.rand(200, 3).astype(np.float32) - 0.5) * 0.02  # inside the 1e-3 ball
  pad0 = pad.copy()
  pad0[0] = 0.0  # pick 0 itself is padding
  allpad = np.zeros((70, 3), np.float32)  # no point qualifies: index 0 throughout
  few = _cloud(rng, 5)
  for name, pts, m in (("dup", dup, 64), ("pad", pad, 128), ("pad0", pad0, 128), ("allpad", allpad, 8), ("few", few, 16),
                       ("dup-large", np.tile(_cloud(rng, 300), (30, 1)), 400)):
    got = P.furthest_point_sample(_dev(pts[None]), m).cpu().numpy()[0]
    want = R.fps(pts, m)
    assert (got == want).all(), "fps %s: %d picks differ" % (name, int((got != want).sum()))
  assert R.qualifies(pad)[R.fps(pad, 128)[1:]].all()  # padding is never chosen


def test_fps_segments_mixed_sizes():
  from pointcontrast_amd import functional as PF
  rng = np.random.RandomState(2)
  sizes = [1000, 0, 65, 4097, 9000, 1, 64]
  offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
  N = int(offs[-1])
  xyz = _cloud(rng, N)
  offs_d = _dev(offs)
  for with_rows in (False, True):
    rows = rng.permutation(N).astype(np.int32) if with_rows else None
    rows_d = _dev(rows) if with_rows else None
    for m in (1, 16, 1024):
      pos, row = PF.furthest_point_sample_segments(_dev(xyz), C.c_void_p(offs_d.data_ptr()),
                                                   C.c_void_p(rows_d.data_ptr()) if with_rows else None, len(sizes), N, m)
      wpos, wrow = R.fps_segments(xyz, offs, rows, m)
      assert (pos.cpu().numpy() == wpos).all() and (row.cpu().numpy() == wrow).all(), (with_rows, m)
      assert (pos.cpu().numpy()[1] == -1).all()
      # a tight bound launches fewer tiers and gives the same picks
      pos2, _ = PF.furthest_point_sample_segments(_dev(xyz), C.c_void_p(offs_d.data_ptr()),
                                                  C.c_void_p(rows_d.data_ptr()) if with_rows else None, len(sizes), max(sizes), m)
      assert torch.equal(pos, pos2)


# ---- ball query / three_nn ----------------------------------------------------------------------------------------------------
def test_ball_query_fill_levels():
  from pointcontrast_amd import pointnet2_utils as P
  rng = np.random.RandomState(3)
  xyz = rng.rand(2, 3000, 3).astype(np.float32)
  new_xyz = np.concatenate([xyz[:, :50], rng.rand(2, 27, 3).astype(np.float32), np.full((2, 3, 3), 9.0, np.float32)], axis=1)
  seen = set()
  for nsample in (1, 16, 64):
    for radius in (1e-4, 0.08, 0.2, 0.5):
      got = P.ball_query(radius, nsample, _dev(xyz), _dev(new_xyz))
      assert got.dtype == torch.int32 and got.shape == (2, 80, nsample) and not got.requires_grad
      want = R.ball_query(xyz, new_xyz, radius, nsample)
      assert (got.cpu().numpy() == want).all(), (nsample, radius)
      cnt = (R.sq_dist(xyz[0], new_xyz[0, 60])[None] < np.float32(radius) * np.float32(radius)).sum()
      seen.add("none" if cnt == 0 else "partial" if cnt < nsample else "overflow")
      assert (want[:, -3:] == 0).all()  # the far centres have no hit
  assert seen == {"none", "partial", "overflow"}


def test_three_nn_sizes_and_ties():
  from pointcontrast_amd import functional as PF, pointnet2_utils as P
  from pointcontrast_amd._lib import PcmiError
  rng = np.random.RandomState(4)
  unknown = rng.rand(2, 700, 3).astype(np.float32)
  for m in (3, 4, 1000):
    known = rng.rand(2, m, 3).astype(np.float32)
    if m == 1000:
      known[:, 400] = known[:, 17]  # a duplicated known point: tied distances for every unknown
      known[:, 999] = known[:, 17]
    d2, idx = PF.three_nn_squared(_dev(unknown), _dev(known))
    wd2, widx = R.three_nn(unknown, known)
    assert (idx.cpu().numpy() == widx).all(), m
    assert (d2.cpu().numpy().view(np.uint32) == wd2.view(np.uint32)).all(), m
    dist, idx2 = P.three_nn(_dev(unknown), _dev(known))
    assert torch.equal(idx2, idx) and torch.equal(dist, torch.sqrt(d2)) and idx2.dtype == torch.int32
  with pytest.raises(PcmiError, match="at least 3"):
    P.three_nn(_dev(unknown), _dev(rng.rand(2, 2, 3).astype(np.float32)))


# ---- gathers --------------------------------------------------------------------------------------------------------------------
def _index_sets(rng, B, N):
  """Duplicate-heavy index tensors: every index the same, a ball query's padded output, and a random one."""
  from pointcontrast_amd import pointnet2_utils as P
  xyz = rng.rand(B, N, 3).astype(np.float32)
  bq = P.ball_query(0.15, 16, _dev(xyz), _dev(xyz[:, :40])).cpu().numpy()  # [B, 40, 16], padded with the first hit
  return {"same": np.full((B, 40, 16), 5, np.int32), "ball": bq, "random": rng.randint(0, N, (B, 40, 16)).astype(np.int32)}


def test_forward_gathers_bit_equal_to_torch_indexing():
  from pointcontrast_amd import pointnet2_utils as P
  rng = np.random.RandomState(5)
  B, Cc, N = 3, 13, 257
  feat = _dev(rng.randn(B, Cc, N).astype(np.float32))
  for name, idx in _index_sets(rng, B, N).items():
    it = _dev(idx)
    assert torch.equal(P.grouping_operation(feat, it), R.group(feat, it)), name
    flat = it.reshape(B, -1)
    assert torch.equal(P.gather_operation(feat, flat), R.gather(feat, flat)), name


def _twice(fn):
  a, b = fn(), fn()
  assert torch.equal(a, b), "two runs differ"
  return a


def test_interpolate_forward_and_all_backwards():
  from pointcontrast_amd import pointnet2_utils as P
  rng = np.random.RandomState(6)
  B, Cc, N = 3, 13, 257
  feat = _dev(rng.randn(B, Cc, N).astype(np.float32))
  for name, idx in _index_sets(rng, B, N).items():
    it = _dev(idx)
    # grouping
    gout = _dev(rng.randn(B, Cc, 40, 16).astype(np.float32))
    f = feat.clone().requires_grad_(True)
    got = _twice(lambda: torch.autograd.grad(P.grouping_operation(f, it), f, gout)[0])
    e = R.rel_err(got, R.grad_of(lambda x: R.group(x, it.cpu()), feat, gout))
    print("group bwd %s: rel err %.3e" % (name, e))
    assert e <= TOL, ("group bwd", name, e)
    # gather
    flat = it.reshape(B, -1)
    gflat = gout.reshape(B, Cc, -1)
    got = _twice(lambda: torch.autograd.grad(P.gather_operation(f, flat), f, gflat)[0])
    e = R.rel_err(got, R.grad_of(lambda x: R.gather(x, flat.cpu()), feat, gflat))
    print("gather bwd %s: rel err %.3e" % (name, e))
    assert e <= TOL, ("gather bwd", name, e)
    # interpolation: idx [B, n, 3] from the same sets
    i3 = it.reshape(B, -1)[:, :213].reshape(B, 71, 3).contiguous()
    w = _dev(rng.rand(B, 71, 3).astype(np.float32))
    out = _twice(lambda: P.three_interpolate(feat, i3, w))
    e = R.rel_err(out, R.interpolate(feat.double().cpu(), i3.cpu(), w.double().cpu()))
    print("interpolate fwd %s: rel err %.3e" % (name, e))
    assert e <= TOL, ("interpolate fwd", name, e)
    g3 = _dev(rng.randn(B, Cc, 71).astype(np.float32))
    got = _twice(lambda: torch.autograd.grad(P.three_interpolate(f, i3, w), f, g3)[0])
    e = R.rel_err(got, R.grad_of(lambda x: R.interpolate(x, i3.cpu(), w.double().cpu()), feat, g3))
    print("interpolate bwd %s: rel err %.3e" % (name, e))
    assert e <= TOL, ("interpolate bwd", name, e)


def test_query_and_group_module():
  from pointcontrast_amd import pointnet2_utils as P
  rng = np.random.RandomState(7)
  xyz, feats = _dev(rng.rand(2, 500, 3).astype(np.float32)), _dev(rng.randn(2, 6, 500).astype(np.float32)).requires_grad_(True)
  new_xyz = xyz[:, :32].contiguous()
  new_f, gxyz = P.QueryAndGroup(0.2, 16, use_xyz=True, ret_grouped_xyz=True, normalize_xyz=True)(xyz, new_xyz, feats)
  idx = _dev(R.ball_query(xyz.cpu().numpy(), new_xyz.cpu().numpy(), 0.2, 16))
  want_xyz = (R.group(xyz.transpose(1, 2).contiguous(), idx) - new_xyz.transpose(1, 2).unsqueeze(-1)) / 0.2
  assert new_f.shape == (2, 9, 32, 16) and torch.equal(gxyz, want_xyz) and torch.equal(new_f[:, :3], want_xyz)
  assert torch.equal(new_f[:, 3:], R.group(feats, idx))
  new_f.sum().backward()
  assert feats.grad is not None and float(feats.grad.sum()) == 2 * 6 * 32 * 16
  assert P.QueryAndGroup(0.2, 16, use_xyz=False)(xyz, new_xyz, feats).shape == (2, 6, 32, 16)


# ---- error paths: an error code, nothing launched, no fault ----------------------------------------------------------------
def test_error_paths():
  from pointcontrast_amd import pointnet2_utils as P
  from pointcontrast_amd._lib import lib, PcmiError
  from pointcontrast_amd.runtime import ptr, cur_stream, ws_args
  feat = torch.randn(2, 4, 50, device=DEV)
  bad = torch.randint(0, 50, (2, 8, 4), device=DEV, dtype=torch.int32)
  bad[1, 3, 2] = 50
  neg = bad.clone()
  neg[1, 3, 2] = -1
  w = torch.rand(2, 8, 3, device=DEV)
  for idx in (bad, neg):
    with pytest.raises(PcmiError, match="outside"):
      P.grouping_operation(feat, idx)
    with pytest.raises(PcmiError, match="outside"):
      P.gather_operation(feat, idx.reshape(2, -1))
    with pytest.raises(PcmiError, match="outside"):
      P.three_interpolate(feat, idx[:, :, :3].contiguous(), w)
  st = cur_stream(DEV)
  out = torch.full((2, 4, 32), 7.0, device=DEV)
  ws, wsb = ws_args(lib.pcmi_pointset_scatter_workspace_bytes(64, 100), DEV)
  flat = bad.reshape(2, 32).contiguous()
  gf = torch.full((2, 4, 50), 7.0, device=DEV)
  assert lib.pcmi_gather_points_bwd(ptr(out), ptr(flat), 2, 4, 50, 32, ptr(gf), 1, ws, wsb, st) == -5  # PCMI_ERR_RANGE
  assert lib.pcmi_gather_points_fwd(ptr(feat), ptr(flat), 2, 4, 50, 32, ptr(out), 1, st) == -5
  assert lib.pcmi_gather_points_fwd(None, ptr(flat), 2, 4, 50, 32, ptr(out), 1, st) == -1  # null pointer
  assert lib.pcmi_gather_points_fwd(ptr(feat), ptr(flat), 2, 4, -50, 32, ptr(out), 1, st) == -1  # negative size
  assert lib.pcmi_group_points_fwd(ptr(feat), ptr(flat), 2, 4, 50, -8, 4, ptr(out), 1, st) == -1
  assert lib.pcmi_gather_points_bwd(ptr(out), ptr(flat), 2, 4, 50, 32, ptr(gf), 1, ws, C.c_size_t(16), st) == -7  # workspace
  assert lib.pcmi_three_interpolate_fwd(ptr(feat), ptr(flat), None, 2, 4, 50, 8, ptr(out), 1, st) == -1
  xyz = torch.rand(2, 30, 3, device=DEV)
  i32 = torch.full((2, 4), 7, device=DEV, dtype=torch.int32)
  assert lib.pcmi_fps(None, 60, None, None, 2, 30, 4, ptr(i32), None, None, 0, st) == -1
  assert lib.pcmi_fps(ptr(xyz), 60, None, None, 2, 30, 0, ptr(i32), None, None, 0, st) == -1  # no picks asked for
  assert lib.pcmi_fps(ptr(xyz), 60, None, None, 2, 31, 4, ptr(i32), None, None, 0, st) == -1  # shape mismatch
  assert lib.pcmi_fps(ptr(xyz), -60, None, None, 2, 30, 4, ptr(i32), None, None, 0, st) == -1
  big = torch.rand(1, 9000, 3, device=DEV)
  assert lib.pcmi_fps(ptr(big), 9000, None, None, 1, 9000, 4, ptr(i32), None, None, 0, st) == -7  # needs the minima workspace
  assert lib.pcmi_ball_query(ptr(xyz), None, 2, 30, 4, 0.1, 1, ptr(i32), st) == -1
  assert lib.pcmi_ball_query(ptr(xyz), ptr(xyz), 2, 30, 4, 0.1, 0, ptr(i32), st) == -1
  assert lib.pcmi_ball_query(ptr(xyz), ptr(xyz), 2, -30, 4, 0.1, 1, ptr(i32), st) == -1
  assert lib.pcmi_three_nn(ptr(xyz), ptr(xyz), 2, 30, 2, ptr(xyz), ptr(i32), st) == -1
  assert b"three_nn" in lib.pcmi_last_error()
  torch.cuda.synchronize()
  assert float(out.min()) == 7.0 and float(gf.min()) == 7.0 and int(i32.min()) == 7, "a refused call wrote to its output"


# ---- the detection backbone's seed sampling -------------------------------------------------------------------------------------
def test_sample_seeds_two_scenes():
  import pointcontrast_amd.minkowski as ME
  from pointcontrast_amd.downstream.votenet import sample_seeds
  from pointcontrast_amd.lib.config import get_config
  from pointcontrast_amd.model import load_model
  rng = np.random.RandomState(8)
  B, num_points, num_seed, voxel = 2, 3000, 256, 0.05
  points = (rng.rand(B, num_points, 3) * np.array([2.0, 2.0, 1.0]) + 0.5).astype(np.float32)
  coords, inds = [], []
  for b in range(B):  # quantise: the first point of every occupied voxel, rows shuffled
    q = np.floor(points[b] / voxel).astype(np.int32)
    _, first = np.unique(q, axis=0, return_index=True)
    first = rng.permutation(first)
    coords.append(np.concatenate([np.full((len(first), 1), b, np.int32), q[first]], axis=1))
    inds.append(first)
  coords, inds = np.concatenate(coords), np.concatenate(inds)
  perm = rng.permutation(len(coords))  # the scenes' rows interleaved
  coords, inds = coords[perm], inds[perm]
  torch.manual_seed(0)
  cfg = get_config(["net.normalize_feature=False"])
  model = load_model("Res16UNet14")(3, 32, cfg, D=3).to(DEV)
  feats = torch.from_numpy(rng.rand(len(coords), 3).astype(np.float32))
  out = model(ME.SparseTensor(feats, coords=torch.from_numpy(coords)).to(DEV))
  pts_d, inds_d = _dev(points), _dev(inds, torch.int64)
  xyz, f, si = sample_seeds(out, pts_d, inds_d, num_seed)
  assert xyz.shape == (B, num_seed, 3) and f.shape == (B, 32, num_seed) and si.shape == (B, num_seed) and si.dtype == torch.int64
  # the reference's loop (backbone_module.py:159-177) in torch indexing on the same device outputs, sampling by the reference fps
  F_ = out.F.detach()
  batch_ids = _dev(coords[:, 0], torch.int64)
  flat = pts_d.reshape(-1, 3)
  voxel_ids = inds_d + batch_ids * num_points
  rows_all = []
  for b in range(B):
    mask = batch_ids == b
    pb = flat[voxel_ids[mask]]
    sid = _dev(R.fps(pb.cpu().numpy(), num_seed, tie_free=True), torch.int64)
    assert torch.equal(si[b], inds_d[mask][sid]) and torch.equal(xyz[b], pb[sid]), b
    assert torch.equal(f[b], F_[mask][sid].transpose(0, 1)), b
    rows_all.append(torch.nonzero(mask).reshape(-1)[sid])
  gout = torch.randn(B, 32, num_seed, device=DEV)

  def grad():
    return torch.autograd.grad(f, out.F, gout, retain_graph=True)[0]
  got = _twice(grad)
  want = torch.zeros(F_.shape, dtype=torch.float64)
  want.index_add_(0, torch.cat(rows_all).cpu(), gout.double().cpu().transpose(1, 2).reshape(B * num_seed, 32))
  e = R.rel_err(got, want)
  print("sample_seeds grad: rel err %.3e" % e)
  assert e <= TOL
