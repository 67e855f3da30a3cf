"""Active labelling on the device (csrc/kmeans.hip, functional.py's kmeans_* wrappers, downstream/semseg.py's
AnnotationSelector) against tests/kmeans_ref.py, which tests/test_kmeans_ref.py holds to independent ground.  Every output is
an integer, a single rounding or a fixed-order fp64 sum: everything is compared BIT for bit (floats through their integer
images).  Shapes: at most 4096 rows per scene, 4 scenes and 64 clusters, except the cases that sit on a dispatch boundary of
DESIGN.md 3.27 and say so."""
import ctypes as C

import numpy as np
import pytest
import torch

import kmeans_ref as kr
from c_contract import DEV, Guarded, PCMI_ERR_INVALID, PCMI_ERR_WORKSPACE, PCMI_OK

pytestmark = pytest.mark.gpu
PCMI_ERR_UNSUPPORTED = -6


@pytest.fixture(scope="module")
def PF():
  from pointcontrast_amd import functional as pf
  return pf


def _dev(a, dtype=None):
  t = torch.from_numpy(np.ascontiguousarray(a))
  return (t if dtype is None else t.to(dtype)).to(DEV)


def _stream():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _vp(t):
  return C.c_void_p(t.data_ptr())


def _bits(a):
  a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
  return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(got, want, keys, what):
  for k in keys:
    g, w = _bits(got[k]), _bits(want[k])
    assert g.shape == w.shape, "%s: %s has shape %s, want %s" % (what, k, g.shape, w.shape)
    bad = np.flatnonzero(g.ravel() != w.ravel())
    assert len(bad) == 0, "%s: %s differs at %d of %d entries, first %d: got %r want %r" % (
        what, k, len(bad), g.size, bad[0], np.asarray(got[k].cpu() if torch.is_tensor(got[k]) else got[k]).ravel()[bad[0]],
        np.asarray(want[k]).ravel()[bad[0]])


STEP_KEYS = ("assign", "sum", "cnt", "centroid", "changed", "skipped")
FINAL_KEYS = ("assign", "d2", "nearest", "inertia", "cnt", "skipped")
SELECT_KEYS = ("rows", "assign", "centroid", "cnt", "inertia", "changed", "skipped", "live")


def features(n, c, seed, scale=1.0):
  return (np.random.default_rng(seed).normal(size=(n, c)) * scale).astype(np.float32)


def grid_features(n, c, seed):
  """Multiples of 2^-10: exact at the 2^-32 quantum of the sums, so the mean of equal rows is the row itself."""
  return (np.round(features(n, c, seed) * 1024) / 1024).astype(np.float32)


def init_rows_for(offs, K, seed):
  """K rows per scene in ascending scene order: distinct where the scene has them, -1 for the surplus."""
  rng = np.random.default_rng(seed)
  rows = np.full((len(offs) - 1, K), -1, dtype=np.int32)
  for b in range(len(offs) - 1):
    m = int(offs[b + 1] - offs[b])
    pick = rng.permutation(m)[:K]
    rows[b, :len(pick)] = offs[b] + pick
  return rows


def run_lloyd(PF, feat_d, feat, offs, init, steps, what, max_rows=None):
  """init, `steps` iterations and the final pass on the device and in the restatement, everything compared; returns both."""
  offs_d = _dev(np.asarray(offs, np.int64))
  cen, live, flags = PF.kmeans_init(feat_d, offs_d, _dev(init), max_rows)
  wcen, wlive, wflags = kr.kmeans_init(feat, offs, init, max_rows)
  same(dict(c=cen, l=live, f=flags), dict(c=wcen, l=wlive, f=wflags), ("c", "l", "f"), what + ": init")
  prev, wprev = None, None
  for it in range(steps):
    st = PF.kmeans_step(feat_d, offs_d, cen, live, prev, max_rows)
    wst = kr.kmeans_step(feat, offs, wcen, wlive, wprev, max_rows)
    same(st, wst, STEP_KEYS, "%s: step %d" % (what, it))
    cen, prev, wcen, wprev = st["centroid"], st["assign"], wst["centroid"], wst["assign"]
  fin = PF.kmeans_assign(feat_d, offs_d, cen, live, max_rows)
  wfin = kr.kmeans_assign(feat, offs, wcen, wlive, max_rows)
  same(fin, wfin, FINAL_KEYS, what + ": final pass")
  return fin, wfin, cen, live


# ---- bit parity with the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [16, 32, 48, 96, 128])
def test_lloyd_matches_restatement(PF, c):
  offs = kr.offsets_of([257, 0, 1000, 63])
  feat = features(offs[-1], c, seed=c)
  init = init_rows_for(offs, 7, seed=1)
  init[2, 3] = -1  # a dead cluster among live ones
  run_lloyd(PF, _dev(feat), feat, offs, init, 2, "C = %d" % c)


@pytest.mark.parametrize("c", [16, 32])
def test_column_slice_of_a_wider_buffer(PF, c):
  offs = kr.offsets_of([300, 129])
  feat = features(offs[-1], c, seed=3)
  wide = torch.full((offs[-1], c + 32), float("nan"), device=DEV)
  wide[:, 4:4 + c] = _dev(feat)
  view = wide[:, 4:4 + c]
  assert view.stride(0) == c + 32 and PF._km_feat(view, "test").data_ptr() == view.data_ptr(), "the slice itself is what the kernels read"
  run_lloyd(PF, view, feat, offs, init_rows_for(offs, 5, seed=2), 2, "ld = C + 32")
  draws = np.random.default_rng(4).integers(0, 2 ** 64, size=(2, 5), dtype=np.uint64)
  got = PF.kmeans_pp_init(view, _dev(offs), 5, PF.KMeansDraws(draws))
  assert np.array_equal(got.cpu().numpy(), kr.kmeans_pp_init(feat, offs, 5, draws))


def test_seeding_and_select_match_restatement(PF):
  offs = kr.offsets_of([4096, 130, 1, 0])
  feat = features(offs[-1], 32, seed=11)
  feat[7, 5] = np.inf
  K = 16
  draws = np.random.default_rng(12).integers(0, 2 ** 64, size=(4, K), dtype=np.uint64)
  offs_d, feat_d = _dev(offs), _dev(feat)
  # step by step, mind2 included
  mind2, wmind2 = torch.full((offs[-1],), float("inf"), device=DEV), np.full(offs[-1], np.inf, np.float32)
  last, wlast = None, None
  for k in range(3):
    last = PF.kmeans_pp_step(feat_d, offs_d, mind2, last, _dev(draws[:, k].view(np.int64)))
    wlast, wmind2 = kr.kmeans_pp_step(feat, offs, wmind2, wlast, draws[:, k])
    same(dict(next=last, mind2=mind2), dict(next=wlast, mind2=wmind2), ("next", "mind2"), "seeding step %d" % k)
  want_rows = kr.kmeans_pp_init(feat, offs, K, draws)
  assert np.array_equal(PF.kmeans_pp_init(feat_d, offs_d, K, PF.KMeansDraws(draws)).cpu().numpy(), want_rows)
  assert want_rows[2].tolist() == [4226] + [-1] * (K - 1) and want_rows[3].tolist() == [-1] * K  # K > n: the surplus is dead
  got = PF.kmeans_select(feat_d, offs, K, PF.KMeansDraws(draws), iters=3)
  want = kr.kmeans_select(feat, offs, K, draws, iters=3)
  assert not got["rows"].is_cuda and got["changed"].shape == (3, 4)
  same(got, want, SELECT_KEYS, "kmeans_select")
  assert 7 not in got["rows"].tolist()[0] and int(got["skipped"][0]) == 1 and int(got["assign"][7]) == -1


def test_assign_equals_feature_nn(PF):
  offs = kr.offsets_of([700, 64, 333])
  feat = features(offs[-1], 32, seed=21)
  K = 9
  cen = features(3 * K, 32, seed=22).reshape(3, K, 32)
  cen[1, 4] = cen[1, 2]  # equal distances: the lowest index wins in both
  live = np.zeros((3, K), np.int32)
  fin = PF.kmeans_assign(_dev(feat), _dev(offs), _dev(cen), _dev(live))
  k_offs = np.arange(4, dtype=np.int64) * K
  nn, d2 = PF.feature_nn(_dev(feat), _dev(offs), _dev(cen.reshape(-1, 32)), _dev(k_offs))
  scene = np.repeat(np.arange(3), np.diff(offs))
  assert np.array_equal(fin["assign"].cpu().numpy(), nn.cpu().numpy() - scene * K)
  assert np.array_equal(_bits(fin["d2"]), _bits(d2))
  assert 4 not in fin["assign"][700:764].tolist()


# ---- edges -----------------------------------------------------------------------------------------------------------------------
EDGE_LENS = [0, 1, 63, 64, 65, 255, 256, 257]


def test_scene_sizes_around_the_tiles_and_no_leakage(PF):
  offs = kr.offsets_of(EDGE_LENS)
  feat = features(offs[-1], 16, seed=31)
  init = init_rows_for(offs, 3, seed=32)  # (K > n for the scenes of 0 and 1 rows: their surplus clusters are dead)
  fin, _, cen, live = run_lloyd(PF, _dev(feat), feat, offs, init, 2, "eight scenes")
  assert fin["nearest"][0].tolist() == [-1, -1, -1] and fin["nearest"][1].tolist() == [0, -1, -1]
  for b in range(len(EDGE_LENS)):  # a call with this scene alone gives the same bits
    lo, hi = int(offs[b]), int(offs[b + 1])
    if hi == lo:
      continue
    one = init[b:b + 1].copy()
    one[one >= 0] -= lo
    alone, _, _, _ = run_lloyd(PF, _dev(feat[lo:hi]), feat[lo:hi], np.array([0, hi - lo]), one, 2, "scene %d alone" % b)
    assert np.array_equal(alone["assign"].cpu().numpy(), fin["assign"][lo:hi].cpu().numpy())
    assert np.array_equal(_bits(alone["d2"]), _bits(fin["d2"][lo:hi])) and _bits(alone["inertia"])[0] == _bits(fin["inertia"])[b]
    near = alone["nearest"][0].cpu().numpy()
    assert np.array_equal(np.where(near >= 0, near + lo, -1), fin["nearest"][b].cpu().numpy())


def test_very_different_scene_sizes_in_one_call(PF):
  offs = kr.offsets_of([4096, 3, 900])
  feat = features(offs[-1], 32, seed=33)
  run_lloyd(PF, _dev(feat), feat, offs, init_rows_for(offs, 8, seed=34), 1, "4096 + 3 + 900 rows")


def test_one_cluster_and_every_row_its_own(PF):
  feat = grid_features(40, 16, seed=35)
  offs = np.array([0, 40])
  fin, _, _, _ = run_lloyd(PF, _dev(feat), feat, offs, np.array([[17]], np.int32), 2, "K = 1")
  assert (fin["assign"] == 0).all()
  fin, _, _, _ = run_lloyd(PF, _dev(feat), feat, offs, np.arange(40, dtype=np.int32)[None], 2, "K = n")
  assert fin["assign"].tolist() == list(range(40)) and float(fin["inertia"][0]) == 0.0 and fin["nearest"][0].tolist() == list(range(40))


def test_identical_rows_and_duplicated_centroids(PF):
  feat = np.tile(grid_features(1, 16, seed=36), (100, 1))
  offs = np.array([0, 100])
  draws = np.random.default_rng(37).integers(0, 2 ** 64, size=(1, 4), dtype=np.uint64)
  rows = PF.kmeans_pp_init(_dev(feat), _dev(offs), 4, PF.KMeansDraws(draws)).cpu().numpy()
  want = kr.kmeans_pp_init(feat, offs, 4, draws)
  assert np.array_equal(rows, want)
  first = (100 * int(draws[0, 0])) >> 64
  assert want[0].tolist() == ([first, 0, -1, -1] if first != 0 else [0, -1, -1, -1])  # total == 0: the lowest active row
  got = PF.kmeans_select(_dev(feat), offs, 4, PF.KMeansDraws(draws), iters=2)
  same(got, kr.kmeans_select(feat, offs, 4, draws, iters=2), SELECT_KEYS, "identical rows")
  assert (got["assign"] == 0).all() and got["rows"][0].tolist() == [0, -1, -1, -1]  # every tie goes to k = 0, to the lowest row
  # two distinct rows with the same features as centres: the second cluster stays empty and keeps its centroid
  feat2 = features(200, 16, seed=38)
  feat2[150] = feat2[20]
  offs2, init2 = np.array([0, 200]), np.array([[20, 150, 3]], np.int32)
  run_lloyd(PF, _dev(feat2), feat2, offs2, init2, 2, "duplicated centroids")
  cen, live, _ = PF.kmeans_init(_dev(feat2), offs2, _dev(init2))
  st = PF.kmeans_step(_dev(feat2), offs2, cen, live)  # (in the NEXT iteration the first has moved and the second may win rows)
  assert int(st["cnt"][0, 1]) == 0 and 1 not in st["assign"].tolist() and np.array_equal(st["centroid"][0, 1].cpu().numpy(), feat2[20])
  fin = PF.kmeans_assign(_dev(feat2), offs2, cen, live)
  assert int(fin["cnt"][0, 1]) == 0 and int(fin["nearest"][0, 1]) == -1 and int(fin["nearest"][0, 0]) == 20


def test_inactive_rows(PF):
  offs = kr.offsets_of([130, 70])
  feat = features(offs[-1], 16, seed=39)
  feat[3, 0], feat[64, 15], feat[129, 7], feat[131, 1] = np.nan, np.inf, 1024.25, -np.inf
  feat[5, 2] = -1024.0  # the clamp itself is active
  init = np.array([[3, 10, 140], [131, 150, 160]], np.int32)  # inactive, fine, outside its scene | inactive, fine, fine
  fin, _, _, live = run_lloyd(PF, _dev(feat), feat, offs, init, 2, "NaN, inf and |x| > 1024")
  assert live.tolist() == [[-1, 10, -1], [-1, 150, 160]] and fin["skipped"].tolist() == [3, 1]
  assert (fin["assign"][[3, 64, 129, 131]] == -1).all() and int(fin["assign"][5]) == 1
  assert torch.isnan(fin["d2"][[3, 64, 129, 131]]).all() and not set(fin["nearest"].flatten().tolist()) & {3, 64, 129, 131}
  # seeding never draws them either, and a scene without an active row gives -1
  bad = np.full((4, 16), np.nan, np.float32)
  draws = np.random.default_rng(40).integers(0, 2 ** 64, size=(1, 2), dtype=np.uint64)
  assert PF.kmeans_pp_init(_dev(bad), _dev(np.array([0, 4])), 2, PF.KMeansDraws(draws)).tolist() == [[-1, -1]]


# ---- one case on each side of every dispatch boundary of DESIGN.md 3.27 ----------------------------------------------------------
@pytest.mark.parametrize("c,K", [(128, 36), (128, 37), (32, 245), (32, 246)])
def test_lds_and_global_accumulators(PF, c, K):
  # sums in LDS while 8 K C + 4 K bytes fit beside the tiles in 80 KiB: K <= 36 at C = 128, K <= 245 at C = 32
  offs = kr.offsets_of([1100, 300])
  feat = features(offs[-1], c, seed=K)
  run_lloyd(PF, _dev(feat), feat, offs, init_rows_for(offs, K, seed=41), 1, "C = %d, K = %d" % (c, K))


@pytest.mark.parametrize("K", [64, 65])
def test_cluster_tiles(PF, K):
  offs = kr.offsets_of([500])
  feat = features(500, 16, seed=42)
  run_lloyd(PF, _dev(feat), feat, offs, init_rows_for(offs, K, seed=43), 1, "K = %d" % K)


def row_chunks(n, B):
  """The launch rule of the step and the final pass restated: (chunks per scene, which term binds)."""
  cus = torch.cuda.get_device_properties(0).multi_processor_count
  by_rows, by_chip = -(-max(n, 1) // 1024), max(1, 2 * cus // B)
  return min(by_rows, by_chip, 65535), "chip" if by_chip < by_rows else "rows"


def test_row_chunks_bound_by_the_chip_many_tiles_per_workgroup(PF):
  # every other case here is cut by rows (ceil(n / 1024) chunks); a ScanNet batch is cut by the chip term, 2 CUs / B chunks per
  # scene, and a workgroup then walks many tiles.  B = 4 and more than 1024 * 2 CUs / 4 rows: at 256 CUs 128 chunks, scene 0 in
  # chunks of 832 rows = 13 tiles with an uneven last chunk of 160 rows (2.5 tiles), scene 1 in chunks of 320 with 53 left over
  cus = torch.cuda.get_device_properties(0).multi_processor_count
  lens = [100000 * cus // 256, 33333 * cus // 256, 7, 5000 * cus // 256 + 11]
  offs = kr.offsets_of(lens)
  nch, bound = row_chunks(int(offs[-1]), 4)
  assert bound == "chip" and nch == 2 * cus // 4, (nch, bound)
  cs = -(-(-(-lens[0] // nch)) // 64) * 64
  assert cs >= 8 * 64 and lens[0] % cs != 0 and (lens[0] % cs) % 64 != 0, "many tiles per workgroup, an uneven last chunk and tile"
  feat = features(offs[-1], 16, seed=46)
  feat[lens[0] - 1, 3] = np.nan  # in the uneven tail
  run_lloyd(PF, _dev(feat), feat, offs, init_rows_for(offs, 5, seed=47), 2, "B = 4, chunks bound by the chip")


def test_row_chunks_one_per_scene_with_many_scenes(PF):
  # B above 2 CUs: one chunk per scene although ceil(n / 1024) >= 2, so ONE workgroup walks the whole 1100-row scene (18 tiles,
  # the last of 12 rows) with its LDS accumulators, between scenes of 3 rows
  cus = torch.cuda.get_device_properties(0).multi_processor_count
  B = 2 * cus + 44
  lens = [3] * B
  lens[B // 2] = 1100
  offs = kr.offsets_of(lens)
  assert row_chunks(int(offs[-1]), B) == (1, "chip")
  feat = features(offs[-1], 32, seed=48)
  run_lloyd(PF, _dev(feat), feat, offs, init_rows_for(offs, 4, seed=49), 2, "B = %d, one chunk per scene" % B)


def test_long_scene_crosses_the_chunk_and_partial_boundaries(PF):
  # 66000 rows in one scene: more than one seeding chunk (4096 rows), more than 64 inertia partials per workgroup walk
  # (16384 rows) and more than 256 partials in the final merge (65536 rows)
  offs = kr.offsets_of([66000, 5000])
  feat = features(offs[-1], 16, seed=44)
  draws = np.random.default_rng(45).integers(0, 2 ** 64, size=(2, 3), dtype=np.uint64)
  rows = PF.kmeans_pp_init(_dev(feat), _dev(offs), 3, PF.KMeansDraws(draws)).cpu().numpy()
  assert np.array_equal(rows, kr.kmeans_pp_init(feat, offs, 3, draws))
  run_lloyd(PF, _dev(feat), feat, offs, rows, 1, "66000 rows")
  # the scene cut to its first rows by max_scene_rows: the rest lies in no scene
  fin, _, _, _ = run_lloyd(PF, _dev(feat), feat, offs, rows % 4000 + np.array([[0], [66000]], np.int32), 1, "cut to 4500 rows", max_rows=4500)
  assert (fin["assign"][4500:66000] == -1).all() and (fin["assign"][70500:] == -1).all() and (fin["assign"][:4500] >= 0).all()


# ---- determinism -------------------------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_equal_under_contention(PF):
  feat = features(4096, 32, seed=51, scale=30.0)  # K = 2: every lane of every tile adds to one of two rows of accumulators
  draws = PF.KMeansDraws(np.random.default_rng(52).integers(0, 2 ** 64, size=(1, 2), dtype=np.uint64))
  a = PF.kmeans_select(_dev(feat), [0, 4096], 2, draws, iters=4)
  b = PF.kmeans_select(_dev(feat), [0, 4096], 2, draws, iters=4)
  same(a, b, SELECT_KEYS, "run to run")
  same(a, kr.kmeans_select(feat, np.array([0, 4096]), 2, draws.bits.numpy(), iters=4), SELECT_KEYS, "against the restatement")


# ---- the C contract ----------------------------------------------------------------------------------------------------------------
def test_c_contract_exact_workspaces_and_refusals():
  from pointcontrast_amd._lib import lib
  B, K, c, n = 2, 5, 16, 700
  offs = kr.offsets_of([400, 300])
  feat = features(n, c, seed=61)
  init = init_rows_for(offs, K, seed=62)
  wcen, wlive, _ = kr.kmeans_init(feat, offs, init)
  feat_d, offs_d, cen_d, live_d = _dev(feat), _dev(offs), _dev(wcen), _dev(wlive)
  need = lib.pcmi_kmeans_assign_workspace_bytes(B, K)
  assert need > 0 and need % 8 == 0 and lib.pcmi_kmeans_assign_workspace_bytes(0, K) == 0
  assign, d2, near, inert, cnt, skip = Guarded(4 * n), Guarded(4 * n), Guarded(4 * B * K), Guarded(8 * B), Guarded(4 * B * K), Guarded(8 * B)
  ws = Guarded(need)

  def call(feat_p=_vp(feat_d), ld=c, K_=K, c_=c, msr=400, ws_p=None, ws_n=need):
    return lib.pcmi_kmeans_assign(feat_p, ld, n, _vp(offs_d), B, K_, c_, msr, _vp(cen_d), _vp(live_d), assign.vp, d2.vp, near.vp,
                                  inert.vp, cnt.vp, skip.vp, ws.vp if ws_p is None else ws_p, C.c_size_t(ws_n), _stream())

  assert call(c_=24) == PCMI_ERR_UNSUPPORTED and call(c_=144) == PCMI_ERR_UNSUPPORTED
  assert call(K_=1025) == PCMI_ERR_UNSUPPORTED and call(K_=0) == PCMI_ERR_INVALID
  assert call(msr=(1 << 20) + 1) == PCMI_ERR_UNSUPPORTED  # a scene above 2^20 rows, by the bound alone
  assert call(ld=c - 4) == PCMI_ERR_INVALID and call(feat_p=C.c_void_p(feat_d.data_ptr() + 4)) == PCMI_ERR_INVALID
  assert call(ws_n=need - 1) == PCMI_ERR_WORKSPACE and call(ws_p=C.c_void_p(ws.ptr + 4)) == PCMI_ERR_INVALID
  torch.cuda.synchronize()
  for g in (assign, d2, near, inert, cnt, skip, ws):
    assert bool((g.buf == 0xA5).all()), "a refused call enqueues nothing"
  assert call() == PCMI_OK
  torch.cuda.synchronize()
  for g, what in ((assign, "assign"), (d2, "d2"), (near, "nearest"), (inert, "inertia"), (cnt, "cnt"), (skip, "skipped"), (ws, "workspace")):
    g.check(what)
  want = kr.kmeans_assign(feat, offs, wcen, wlive, 400)
  got = dict(assign=assign.view(torch.int32, n), d2=d2.view(torch.float32, n), nearest=near.view(torch.int32, B * K).view(B, K),
             inertia=inert.view(torch.float64, B), cnt=cnt.view(torch.int32, B * K).view(B, K), skipped=skip.view(torch.int64, B))
  same(got, want, FINAL_KEYS, "pcmi_kmeans_assign through ctypes")

  # the seeding step: exactly its workspace; the step and init take none
  need = lib.pcmi_kmeans_pp_step_workspace_bytes(B)
  ws2, nxt, mind2 = Guarded(need), Guarded(4 * B), Guarded(4 * n)
  mind2.view(torch.float32, n).fill_(float("inf"))
  draw = _dev(np.array([1 << 62, 3 << 62], np.uint64).view(np.int64))

  def pp(c_=c, msr=400, ws_p=None, ws_n=need):
    return lib.pcmi_kmeans_pp_step(_vp(feat_d), c, n, _vp(offs_d), B, c_, msr, None, _vp(draw), mind2.vp, nxt.vp,
                                   ws2.vp if ws_p is None else ws_p, C.c_size_t(ws_n), _stream())

  assert pp(c_=8) == PCMI_ERR_UNSUPPORTED and pp(msr=(1 << 20) + 1) == PCMI_ERR_UNSUPPORTED
  assert pp(ws_n=need - 1) == PCMI_ERR_WORKSPACE and pp(ws_p=C.c_void_p(ws2.ptr + 4)) == PCMI_ERR_INVALID
  assert pp() == PCMI_OK
  torch.cuda.synchronize()
  for g, what in ((ws2, "seeding workspace"), (nxt, "next"), (mind2, "mind2")):
    g.check(what)
  assert nxt.view(torch.int32, B).tolist() == [100, 400 + 225]  # uniform: floor(400 / 4), 400 + floor(300 * 3 / 4)

  cen, live, flags = Guarded(4 * B * K * c), Guarded(4 * B * K), Guarded(8 * B)
  init_d = _dev(init)
  args = (_vp(feat_d), c, n, _vp(offs_d), B)
  assert lib.pcmi_kmeans_init(*args, 1025, c, 400, _vp(init_d), cen.vp, live.vp, flags.vp, _stream()) == PCMI_ERR_UNSUPPORTED
  assert lib.pcmi_kmeans_init(*args, K, 20, 400, _vp(init_d), cen.vp, live.vp, flags.vp, _stream()) == PCMI_ERR_UNSUPPORTED
  assert lib.pcmi_kmeans_init(*args, K, c, 400, _vp(init_d), cen.vp, live.vp, flags.vp, _stream()) == PCMI_OK
  asg, s, cn, out, ch, sk = Guarded(4 * n), Guarded(8 * B * K * c), Guarded(4 * B * K), Guarded(4 * B * K * c), Guarded(8 * B), Guarded(8 * B)
  step = lambda K_, msr: lib.pcmi_kmeans_step(*args, K_, c, msr, cen.vp, live.vp, None, asg.vp, s.vp, cn.vp, out.vp, ch.vp, sk.vp, _stream())
  assert step(1025, 400) == PCMI_ERR_UNSUPPORTED and step(K, (1 << 20) + 1) == PCMI_ERR_UNSUPPORTED
  assert step(K, 400) == PCMI_OK
  torch.cuda.synchronize()
  for g, what in ((cen, "centroid"), (live, "live"), (flags, "flags"), (asg, "assign"), (s, "sum"), (cn, "cnt"), (out, "centroid_out"),
                  (ch, "changed"), (sk, "skipped")):
    g.check(what)
  wst = kr.kmeans_step(feat, offs, wcen, wlive, None, 400)
  got = dict(assign=asg.view(torch.int32, n), sum=s.view(torch.int64, B * K * c).view(B, K, c), cnt=cn.view(torch.int32, B * K).view(B, K),
             centroid=out.view(torch.float32, B * K * c).view(B, K, c), changed=ch.view(torch.int64, B), skipped=sk.view(torch.int64, B))
  same(got, wst, STEP_KEYS, "pcmi_kmeans_step through ctypes")


# ---- planted blobs -------------------------------------------------------------------------------------------------------------------
def test_planted_blobs_as_the_cpu_test_pinned_them(PF):
  K, per = 8, 48
  feat, label = kr.blobs(K, per, 16, seed=7)  # tests/test_kmeans_ref.py::test_planted_blobs_are_recovered
  draws = np.random.default_rng(7).integers(0, 2 ** 64, size=(1, K), dtype=np.uint64)
  got = PF.kmeans_select(_dev(feat), [0, len(feat)], K, PF.KMeansDraws(draws), iters=4)
  same(got, kr.kmeans_select(feat, np.array([0, len(feat)]), K, draws, iters=4), SELECT_KEYS, "planted blobs")
  pairs = set(zip(got["assign"].tolist(), label.tolist()))
  assert len(pairs) == K and len({a for a, _ in pairs}) == K
  assert sorted(label[got["rows"][0].numpy()].tolist()) == list(range(K)), "one annotated row per blob"


# ---- downstream ------------------------------------------------------------------------------------------------------------------------
def _batch(seed=8, batch_size=2):
  from pointcontrast_amd.lib import synthetic
  b = synthetic.make_batch(seed=seed, batch_size=batch_size, crop=0.6)
  return torch.from_numpy(b["sinput0_C"]), torch.from_numpy(b["sinput0_F"])


def test_selectors_give_distinct_rows_of_their_scene():
  from pointcontrast_amd import functional as pf
  from pointcontrast_amd.downstream import semseg as ss
  coords, feats = _batch()
  offs = ss.scene_offsets(coords).numpy()
  assert len(offs) == 3 and offs[-1] == len(coords)
  budget = 20
  draws = pf.KMeansDraws(np.random.default_rng(71).integers(0, 2 ** 64, size=(2, budget), dtype=np.uint64))
  for kind in ("xyzrgb", "random"):
    rows = ss.AnnotationSelector(budget, features=kind, iters=3)(coords, feats, draws)
    assert rows.shape == (2, budget) and rows.dtype == torch.int32 and not rows.is_cuda
    for b in range(2):
      r = rows[b][rows[b] >= 0].tolist()
      assert len(set(r)) == len(r) and all(offs[b] <= x < offs[b + 1] for x in r), kind
      assert len(r) == budget if kind == "random" else len(r) >= budget // 2, kind
    again = ss.AnnotationSelector(budget, features=kind, iters=3)(coords, feats, draws)
    assert torch.equal(rows, again), "the draws are the only randomness"
  # xyzrgb is kmeans_select on the six columns, padded to 16
  sel = ss.AnnotationSelector(budget, features="xyzrgb", iters=3)
  rows = sel(coords, feats, draws)
  x = np.concatenate([coords[:, 1:4].numpy().astype(np.float32) * np.float32(0.05), feats.numpy().astype(np.float32)], 1)
  want = kr.kmeans_select(np.pad(x, ((0, 0), (0, 10))), offs, budget, draws.bits.numpy(), iters=3)
  assert np.array_equal(rows.numpy(), want["rows"])
  # fewer voxels than the budget: -1 for the surplus
  few = ss.AnnotationSelector(budget, features="random")(coords[:7], feats[:7], pf.KMeansDraws(draws.bits[:1]))
  assert sorted(few[0, :7].tolist()) == list(range(7)) and few[0, 7:].tolist() == [-1] * (budget - 7)
  target = torch.arange(len(coords)) % 20
  lim = ss.limited_annotation_target(target, rows)
  keep = rows[rows >= 0].long()
  assert torch.equal(lim[keep], target[keep]) and int((lim != 255).sum()) == len(keep) and int((lim == 255).sum()) == len(target) - len(keep)


def test_train_iter_with_annotated_rows_is_train_iter_on_the_masked_target():
  from pointcontrast_amd.downstream import semseg as ss
  coords, feats = _batch()
  target = torch.from_numpy(np.random.RandomState(3).randint(0, 20, len(coords)))
  rows = ss.AnnotationSelector(20, features="random")(coords, feats, np.random.default_rng(72).integers(0, 2 ** 64, size=(2, 20), dtype=np.uint64))
  losses = []
  for masked in (False, True):
    torch.manual_seed(5)
    tr = ss.SegmentationTrainer(20, model="Res16UNet14", lr=0.05, max_iter=50)
    if masked:
      out = tr.train_iter(coords, feats, ss.limited_annotation_target(target, rows))
    else:
      out = tr.train_iter(coords, feats, target, annotated=rows)
    losses.append(out["loss"].cpu())
  assert torch.isfinite(losses[0]) and _bits(losses[0].reshape(1))[0] == _bits(losses[1].reshape(1))[0]
  # the host target's range check still sees the labels that count: a bad label raises at an annotated row only
  keep = rows[rows >= 0].long()
  free = int(np.setdiff1d(np.arange(len(target)), keep.numpy())[0])
  bad = target.clone()
  bad[free] = 77
  assert torch.isfinite(tr.train_iter(coords, feats, bad, annotated=rows)["loss"])
  bad[int(keep[0])] = 77
  with pytest.raises(IndexError):
    tr.train_iter(coords, feats, bad, annotated=rows)
  dev_target = target.to(DEV)  # a device target is masked on the device
  assert torch.isfinite(tr.train_iter(coords, feats, dev_target, annotated=rows.to(DEV))["loss"])


def test_net_selector_is_kmeans_select_of_its_inference_features():
  from pointcontrast_amd import functional as pf
  from pointcontrast_amd.downstream import semseg as ss
  coords, feats = _batch(seed=3, batch_size=2)
  torch.manual_seed(5)
  sel = ss.AnnotationSelector(12, features="net", model="Res16UNet14", iters=3)
  draws = pf.KMeansDraws(np.random.default_rng(73).integers(0, 2 ** 64, size=(2, 12), dtype=np.uint64))
  rows = sel(coords, feats, draws)
  f = sel.point_features(coords, feats)
  assert f.shape == (len(coords), 32) and torch.allclose(f.norm(dim=1), torch.ones(len(coords), device=f.device), atol=1e-4)
  want = pf.kmeans_select(f, ss.scene_offsets(coords), 12, draws, iters=3)
  assert torch.equal(rows, want["rows"]) and torch.equal(sel.last["assign"], want["assign"])
  ref = kr.kmeans_select(f.cpu().numpy(), ss.scene_offsets(coords).numpy(), 12, draws.bits.numpy(), iters=3)
  assert np.array_equal(rows.numpy(), ref["rows"])
