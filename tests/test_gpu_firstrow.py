"""The five device quantisers held to EACH OTHER (csrc/firstrow.h, csrc/cubscan.h): the loader's pcmi_voxelize, the segmentation
input's pcmi_seg_quantize, the pair input's pcmi_pair_voxelize and the instance input's pcmi_instance_relabel all keep the lowest
row of every key and number those rows by an exclusive scan, so on the same keys they must report the same rows -- those of
np.unique(return_index=True).  Integer-valued points in a cube of side 6: at most 216 keys, many repeats.  Sizes: one row, the
workgroup (256) +- 1, rowscan.h's block (2048) +- 1, the first size with more than two scan blocks.  Then the per-segment
bookkeeping (an empty scene, offsets that stop short of n) and, for every *_workspace_bytes whose formula goes through
cub_scan_bytes and that no other test file holds to it, a workspace of exactly the queried size and one byte less."""
import numpy as np
import pytest
import torch

from c_contract import DEV, _exact_and_short, _same_arrays, exact_ws  # noqa: F401  (exact_ws is a fixture)

pytestmark = pytest.mark.gpu

SIDE = 6
SIZES = [1, 2, 255, 256, 257, 2047, 2048, 2049, 4097]


@pytest.fixture(scope="module")
def PF():
  from pointcontrast_amd import functional as pf
  return pf


def _dev(a, dtype=None):
  t = torch.from_numpy(np.ascontiguousarray(a))
  return (t if dtype is None else t.to(dtype)).to(DEV)


def _cells(n, seed):
  """n integer points of the cube and their packed voxel ids x + 6 (y + 6 z)"""
  c = np.random.RandomState(seed).randint(0, SIDE, size=(n, 3)).astype(np.int64)
  return c, c[:, 0] + SIDE * (c[:, 1] + SIDE * c[:, 2])


def _first_rows(ids):
  return np.sort(np.unique(ids, return_index=True)[1]).astype(np.int64)


def _four_families(PF, cells, ids):
  """(first rows, count) of each family on the same keys; the pair input gives two, one per cloud"""
  from pointcontrast_amd.lib import device_loader
  n = len(ids)
  out = {}
  sel = device_loader.sparse_quantize_index(cells.astype(np.float64), 1.0, device=DEV)
  out["voxelize"] = (sel, len(sel))
  q = PF.seg_quantize(_dev(cells, torch.int32), [0, n])
  cnt = q["counts"].cpu().numpy()
  assert cnt[0] == cnt[1] and int(q["flags"].cpu()[0]) == 0
  out["seg_quantize"] = (q["index"][:cnt[1]].cpu().numpy(), int(cnt[1]))
  both = np.concatenate([cells, cells]).astype(np.float64)
  v = PF.pair_voxelize(_dev(both), [0, n, 2 * n], 1.0)
  nv, voff = v["n_vox"].cpu().numpy(), v["vox_offsets"].cpu().numpy()
  assert int(v["flags"].cpu()[0]) == 0 and voff.tolist() == [0, nv[0], nv[0] + nv[1]]
  first = v["first_index"].cpu().numpy().astype(np.int64)
  out["pair_voxelize cloud 0"] = (first[voff[0]:voff[1]], int(nv[0]))
  out["pair_voxelize cloud 1"] = (first[voff[1]:voff[2]] - n, int(nv[1]))
  r = PF.instance_relabel(_dev(ids, torch.int32), [0, n])
  cnt = r["counts"].cpu().numpy()
  assert cnt[0] == cnt[1]
  out["instance_relabel"] = (r["first_row"][:cnt[1]].cpu().numpy().astype(np.int64), int(cnt[1]))
  return out


@pytest.mark.parametrize("n", SIZES)
def test_families_agree_on_the_first_rows(PF, n):
  cells, ids = _cells(n, seed=n)
  want = _first_rows(ids)
  assert len(want) <= SIDE ** 3 and (n < 256 or len(want) < n), "the keys repeat"
  for name, (rows, count) in _four_families(PF, cells, ids).items():
    print("n %d %s: %d first rows (numpy %d)" % (n, name, count, len(want)))
    assert count == len(rows) == len(want), name
    assert np.array_equal(rows, want), name


def test_no_rows(PF, exact_ws):
  """n = 0 where the entry accepts it: zero counts, and nothing enqueued that touches the workspace"""
  from pointcontrast_amd.lib import device_loader
  ws = exact_ws()
  assert len(device_loader.sparse_quantize_index(np.zeros((0, 3)), 1.0, device=DEV)) == 0
  q = PF.seg_quantize(torch.zeros((0, 3), dtype=torch.int32, device=DEV), [0, 0, 0])
  assert q["counts"].cpu().tolist() == [0, 0, 0] and q["flags"].cpu().tolist() == [0, 0]
  v = PF.pair_voxelize(torch.zeros((0, 3), dtype=torch.float64, device=DEV), [0, 0, 0], 1.0)
  assert v["n_vox"].cpu().tolist() == [0, 0] and v["vox_offsets"].cpu().tolist() == [0, 0, 0] and v["flags"].cpu().tolist() == [0]
  assert v["side_offsets"].cpu().tolist() == [[0, 0], [0, 0]]
  r = PF.instance_relabel(torch.zeros(0, dtype=torch.int32, device=DEV), [0, 0, 0])
  assert r["counts"].cpu().tolist() == [0, 0, 0]
  assert len(ws.bufs) == 4 and ws.untouched()


# ---- the per-segment bookkeeping ----------------------------------------------------------------------------------------------
def _per_scene(ids, offsets):
  """np.unique per scene: the first rows in output order, the counts [B + 1], the instance of every row (-1 outside every scene)"""
  rows, counts, inst = [], [], np.full(len(ids), -1, np.int64)
  for lo, hi in zip(offsets[:-1], offsets[1:]):
    uniq, first, inverse = np.unique(ids[lo:hi], return_index=True, return_inverse=True)
    order = np.argsort(first)  # rank of a key = the rank of its first row
    rank = np.empty(len(uniq), np.int64)
    rank[order] = np.arange(len(uniq))
    inst[lo:hi] = len(rows) + rank[inverse.reshape(-1)]
    rows += (lo + first[order]).tolist()
    counts.append(len(uniq))
  return np.asarray(rows, np.int64), np.asarray(counts + [len(rows)], np.int64), inst


@pytest.mark.parametrize("short", [0, 5])
def test_empty_scene_and_rows_of_no_scene(PF, short):
  n, k = 2049, 700
  cells, ids = _cells(n, seed=11 + short)
  offsets = [0, k, k, n - short]
  rows, counts, inst = _per_scene(ids, offsets)
  assert counts[1] == 0 and counts[:3].sum() == counts[3] and (rows < n - short).all()
  q = PF.seg_quantize(_dev(cells, torch.int32), offsets)
  r = PF.instance_relabel(_dev(ids, torch.int32), offsets)
  for name, got_counts, got_rows in (("seg_quantize", q["counts"], q["index"]), ("instance_relabel", r["counts"], r["first_row"])):
    c = got_counts.cpu().numpy()
    print("%s offsets %s: counts %s (numpy %s)" % (name, offsets, c.tolist(), counts.tolist()))
    assert np.array_equal(c, counts) and c[:3].sum() == c[3], name
    assert np.array_equal(got_rows[:c[3]].cpu().numpy().astype(np.int64), rows), name
  assert q["flags"].cpu().tolist() == [0, 0, 0]
  scene = np.repeat(np.arange(3), np.diff(offsets))
  assert np.array_equal(q["coords"][:counts[3]].cpu().numpy(), np.column_stack([scene[rows], cells[rows]]).astype(np.int32))
  assert np.array_equal(r["instance"][:n - short].cpu().numpy().astype(np.int64), inst[:n - short])


# ---- a workspace of exactly the queried size, and one byte less -------------------------------------------------------------------
N = 257


def _points(seed, n=N):
  return np.random.RandomState(seed).rand(n, 3) * SIDE


def test_voxelize_and_match_radius_workspace(exact_ws):
  from pointcontrast_amd.lib import device_loader
  a, b = _points(1), _points(2)
  _exact_and_short(exact_ws, lambda: device_loader.sparse_quantize_index(a, 0.5, device=DEV, return_coords=True), _same_arrays)
  _exact_and_short(exact_ws, lambda: [device_loader.get_matching_indices(a, b, np.eye(4), 0.75, device=DEV)], _same_arrays)


def test_corpus_workspace(exact_ws):
  """pcmi_corpus_backproject and pcmi_corpus_voxel_centroids (calls 0 and 1 of process_scene; the third has no scan)"""
  from pointcontrast_amd.lib import pair_corpus
  rng = np.random.RandomState(3)
  depths = rng.randint(500, 3000, size=(1, 1, N)).astype(np.uint16)  # 257 pixels, all valid: 257 points
  K = np.eye(4)
  K[0, 0] = K[1, 1] = 100.0
  K[0, 2] = N / 2

  def run():
    out = pair_corpus.process_scene(depths, np.eye(4)[None], K, voxel_size=0.05, device=DEV)
    assert len(out["points"]) == 1 and len(out["points"][0]) == N
    return [out["points"][0], out["centroids"][0], out["C"]]
  _exact_and_short(exact_ws, run, _same_arrays, calls=3, short_at=(0, 1))


def test_pair_voxelize_and_match_workspace(PF, exact_ws):
  pts = _dev(np.concatenate([_points(4, 128), _points(5, N - 128)]))
  offsets, trans, radius = [0, 128, N], _dev(np.eye(4)[None]), _dev(np.array([0.75]))

  def voxelize():
    v = PF.pair_voxelize(pts, offsets, 0.5)
    m = int(v["vox_offsets"].cpu()[2])
    return v, [v[k].cpu().numpy() for k in ("n_vox", "vox_offsets", "side_offsets", "flags")] + [v[k][:m].cpu().numpy() for k in ("points", "coords", "first_index")]
  _exact_and_short(exact_ws, lambda: voxelize()[1], _same_arrays)
  # pcmi_pair_match with m_max = 257: the capacity of pair_voxelize's outputs
  vox = voxelize()[0]

  def match():
    m = PF.pair_match(vox, trans, radius, 16 * N)
    tot = m["totals"].cpu().numpy()
    assert tot[0] > 0 and tot[2] == 0
    return [tot, m["pair_counts"].cpu().numpy(), m["flags"].cpu().numpy(), m["pairs"][:tot[0]].cpu().numpy()]
  _exact_and_short(exact_ws, match, _same_arrays)


def test_pointset_scatter_workspace(PF, exact_ws):
  """pcmi_gather_points_bwd: the pointset.hip entry that builds inverse lists (pcmi_pointset_scatter_workspace_bytes)"""
  rng = np.random.RandomState(6)
  feats = _dev(rng.randn(1, 3, N).astype(np.float32))
  idx = _dev(rng.randint(0, N, size=(1, 64)).astype(np.int32))
  gout = _dev(rng.randn(1, 3, 64).astype(np.float32))

  def run():
    f = feats.clone().requires_grad_(True)
    PF.GatherOperationFunction.apply(f, idx).backward(gout)
    return [f.grad.cpu().numpy()]
  _exact_and_short(exact_ws, run, _same_arrays)
