"""Validation by feature matching on the device (csrc/featmatch.hip: pcmi_feat_nn, pcmi_match_stats, pcmi_ransac_score,
pcmi_rigid_sums; lib/feature_match.py; ContrastiveLossTrainer.validate; pointcontrast_amd.eval_features) against
tests/featmatch_ref.py, which tests/test_featmatch_ref.py holds to independent ground.

Tolerances.  The fp64 entry points have a fixed operation order (include/pcmi.h): counts, residuals, transforms and sums are
compared BIT for bit.  feat_nn is fp32: it is held to float64 distances D with tol_i = 4 (C + 4) 2^-24 (|a_i|^2 + max_j |b_j|^2)
-- the bound of a C-term fp32 dot product and the two squared norms, doubled because two candidates are compared: where the
two smallest D[i, .] are further apart than tol_i the float64 argmin is required exactly, elsewhere D[i, nn_i] - min D[i, .] <=
tol_i; d2 within tol_i + 1e-5 D (the project's figure for dmin).  Exact ties are required bit-exactly."""
import ctypes as C
import io
import json
import os
import contextlib

import numpy as np
import pytest
import torch

import featmatch_ref as fr
from c_contract import DEV, Guarded, PCMI_ERR_WORKSPACE, PCMI_OK

pytestmark = pytest.mark.gpu

TILE, MIN_CHUNK, MAX_CHUNKS = 64, 256, 64  # csrc/featmatch.hip: kTQ = kTS, kMinChunk, kMaxChunks


@pytest.fixture(scope="module")
def PF():
  from pointcontrast_amd import functional as pf
  return pf


def _dev(a, dtype=None):
  t = torch.from_numpy(np.ascontiguousarray(a))
  return (t if dtype is None else t.to(dtype)).to(DEV)


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _bits32(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _strided(a, pad):
  """The rows of `a` as a column slice of a wider device buffer (ld = C + pad, offset 4), NaN around it."""
  if not pad:
    return _dev(a)
  full = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=torch.float32, device=DEV)
  view = full[:, 4:4 + a.shape[1]]
  view.copy_(_dev(a))
  return view


def chunk_rows(Q, B, nr, longest):
  """The launch rule of pcmi_feat_nn (include/pcmi.h) restated: rows per chunk of a reference segment of `longest` rows."""
  n_cu = torch.cuda.get_device_properties(0).multi_processor_count
  tiles = -(-Q // TILE) + B
  nch = max(1, min(-(-4 * n_cu // tiles), -(-nr // MIN_CHUNK), MAX_CHUNKS))
  return -(-(-(-longest // nch)) // TILE) * TILE


def _rows_for(rng, q_lens):
  """query_rows for every segment: about as many as it has rows, with repeats, in DESCENDING order."""
  qo = fr.offsets_of(q_lens)
  parts = [np.sort(rng.randint(qo[b], qo[b + 1], n))[::-1] if n else np.zeros(0, np.int64) for b, n in enumerate(q_lens)]
  return np.concatenate(parts).astype(np.int32), fr.offsets_of([len(p) for p in parts])


def check_nn(qf, qo, rf, ro, rows, offs, nn, d2, what, min_clear=0.99):
  """Every query by one of the two rules of the module docstring; returns the share decided by the first."""
  C_ = qf.shape[1]
  r = np.arange(len(qf)) if rows is None else rows.astype(np.int64)
  offs = qo if rows is None else offs
  assert len(nn) == len(r) == len(d2)
  clear = total = 0
  for b in range(len(qo) - 1):
    lo, hi = int(offs[b]), int(offs[b + 1])
    ref = rf[ro[b]:ro[b + 1]]
    if hi == lo:
      continue
    if len(ref) == 0:
      assert (nn[lo:hi] == -1).all() and np.isnan(d2[lo:hi]).all(), "%s: pair %d has no reference rows" % (what, b)
      continue
    a = qf[r[lo:hi]]
    D = fr.dist2_f64(a, ref)
    tol = 4.0 * (C_ + 4) * 2.0 ** -24 * ((a.astype(np.float64) ** 2).sum(1) + (ref.astype(np.float64) ** 2).sum(1).max())
    order = np.sort(D, 1)
    gap = order[:, 1] - order[:, 0] if D.shape[1] > 1 else np.full(len(a), np.inf)
    got = nn[lo:hi].astype(np.int64) - ro[b]
    assert ((got >= 0) & (got < len(ref))).all(), "%s: pair %d: a row outside the pair's segment" % (what, b)
    is_clear = gap > tol
    want = D.argmin(1)
    bad = np.flatnonzero(is_clear & (got != want))
    assert len(bad) == 0, "%s: pair %d query %d: got row %d, float64 argmin %d (gap %.3e, tol %.3e)" % (
        what, b, bad[0], got[bad[0]], want[bad[0]], gap[bad[0]], tol[bad[0]])
    Dg = D[np.arange(len(a)), got]
    excess = Dg - order[:, 0]
    assert (excess[~is_clear] <= tol[~is_clear]).all(), "%s: pair %d: a near-tie chose a row %.3e above the minimum" % (
        what, b, excess[~is_clear].max())
    err = np.abs(d2[lo:hi].astype(np.float64) - Dg)
    assert (err <= tol + 1e-5 * Dg).all(), "%s: pair %d: d2 off by %.3e" % (what, b, err.max())
    clear += int(is_clear.sum())
    total += len(a)
  share = clear / max(total, 1)
  assert share >= min_clear, "%s: only %.1f %% of the queries have a clear nearest neighbour" % (what, 100 * share)
  return share


# (query segment lengths, reference segment lengths): 1, tile - 1, tile, tile + 1, 2 tile + 1 on both sides, an empty query
# segment, an empty reference segment, and reference segments longer than one chunk (asserted through chunk_rows)
NN_CASES = {
    "b3_edges": ([1, TILE - 1, TILE], [TILE + 1, 2 * TILE + 1, 1]),
    "b3_empty_query": ([TILE + 1, 2 * TILE + 1, 0], [TILE, TILE - 1, 50]),
    "b3_empty_ref_and_chunks": ([10, 20, 5], [0, 700, TILE]),
    "b1_chunks": ([2 * TILE + 1], [1000]),
}
NN_MERGES = {"b3_empty_ref_and_chunks", "b1_chunks"}


@pytest.mark.parametrize("case", sorted(NN_CASES))
@pytest.mark.parametrize("c", [16, 32, 64, 128])
def test_feature_nn_at_tile_and_chunk_edges(PF, c, case):
  q_lens, r_lens = NN_CASES[case]
  rng = np.random.RandomState(c + len(case))
  qo, ro = fr.offsets_of(q_lens), fr.offsets_of(r_lens)
  qf, rf = rng.normal(size=(qo[-1], c)).astype(np.float32), rng.normal(size=(ro[-1], c)).astype(np.float32)
  rows, offs = _rows_for(rng, q_lens)
  for use_rows in (False, True):
    Q = len(rows) if use_rows else len(qf)
    if case in NN_MERGES:
      assert chunk_rows(Q, len(q_lens), len(rf), max(r_lens)) < max(r_lens), "the case does not force a chunk merge"
    for pad in (0, 36):
      qd, rd = _strided(qf, pad), _strided(rf, pad)
      kw = dict(query_rows=_dev(rows), query_offsets=_dev(offs)) if use_rows else {}
      nn, d2 = PF.feature_nn(qd, _dev(qo), rd, _dev(ro), **kw)
      nn2, d22 = PF.feature_nn(qd, _dev(qo), rd, _dev(ro), **kw)
      nn, d2, nn2, d22 = nn.cpu().numpy(), d2.cpu().numpy(), nn2.cpu().numpy(), d22.cpu().numpy()
      what = "%s c=%d rows=%s pad=%d" % (case, c, use_rows, pad)
      assert np.array_equal(nn, nn2) and np.array_equal(_bits32(d2), _bits32(d22)), what + ": two runs differ"
      check_nn(qf, qo, rf, ro, rows if use_rows else None, offs, nn, d2, what)
      # the restatement's own fp32 chain agrees wherever the float64 rule is decisive (checked above), and always in count
      want_nn, _ = fr.feat_nn(qf, qo, rf, ro, rows if use_rows else None, offs if use_rows else None)
      assert np.array_equal(nn == -1, want_nn == -1), what


@pytest.mark.parametrize("c", [48, 80, 96, 112])
def test_feature_nn_other_supported_widths(PF, c):
  rng = np.random.RandomState(c)
  qo, ro = fr.offsets_of([70]), fr.offsets_of([300])
  qf, rf = rng.normal(size=(70, c)).astype(np.float32), rng.normal(size=(300, c)).astype(np.float32)
  nn, d2 = PF.feature_nn(_dev(qf), _dev(qo), _dev(rf), _dev(ro))
  check_nn(qf, qo, rf, ro, None, None, nn.cpu().numpy(), d2.cpu().numpy(), "c=%d" % c)


@pytest.mark.parametrize("c", [16, 128])
def test_feature_nn_exact_ties_go_to_the_lowest_row(PF, c):
  """Every reference row occurs twice, 300 rows apart -- in different chunks of 256 rows for most -- and rows 10 / 11 are equal
  inside one tile: equal fp32 distances, so the lower row must win, bit-exactly."""
  rng = np.random.RandomState(7 + c)
  base = rng.normal(size=(300, c)).astype(np.float32)
  base[11] = base[10]
  rf = np.concatenate([base, base])
  qf = (base[rng.randint(0, 300, 150)] + rng.normal(0, 0.05, (150, c))).astype(np.float32)  # each near one base row
  qf[0] = base[10] + 0.01
  qo, ro = fr.offsets_of([150]), fr.offsets_of([600])
  assert chunk_rows(150, 1, 600, 600) == 256
  nn, d2 = PF.feature_nn(_dev(qf), _dev(qo), _dev(rf), _dev(ro))
  nn, d2 = nn.cpu().numpy(), d2.cpu().numpy()
  assert (nn < 300).all(), "a duplicate in a later chunk won the tie: rows %s" % nn[nn >= 300][:5]
  assert nn[0] == 10
  check_nn(qf, qo, base, fr.offsets_of([300]), None, None, nn, d2, "ties c=%d" % c, min_clear=0.9)


def test_feature_nn_non_finite_rows(PF):
  rng = np.random.RandomState(9)
  qo, ro = fr.offsets_of([40, 30]), fr.offsets_of([300, 20])
  qf, rf = rng.normal(size=(70, 32)).astype(np.float32), rng.normal(size=(320, 32)).astype(np.float32)
  clean, _ = PF.feature_nn(_dev(qf), _dev(qo), _dev(rf), _dev(ro))
  clean = clean.cpu().numpy()
  qf2, rf2 = qf.copy(), rf.copy()
  qf2[3, 5], qf2[41, 0], qf2[42, 31] = np.nan, np.inf, -np.inf
  rf2[clean[0], 7], rf2[clean[1], 0], rf2[clean[45], 3] = np.nan, np.inf, -np.inf  # the winners of three queries
  rf2[300:305] = np.nan
  nn, d2 = PF.feature_nn(_dev(qf2), _dev(qo), _dev(rf2), _dev(ro))
  nn, d2 = nn.cpu().numpy(), d2.cpu().numpy()
  bad_q = np.array([3, 41, 42])
  assert (nn[bad_q] == -1).all() and np.isnan(d2[bad_q]).all(), "a non-finite query matches nothing"
  bad_r = ~np.isfinite(rf2).all(1)
  ok_q = np.setdiff1d(np.arange(70), bad_q)
  assert not bad_r[nn[ok_q]].any(), "a non-finite reference row was chosen"
  # the finite rows alone give the same answer
  keep = np.flatnonzero(~bad_r)
  ro_k = np.array([0, (keep < 300).sum(), len(keep)])
  nn_k, d2_k = PF.feature_nn(_dev(qf2), _dev(qo), _dev(rf2[keep]), _dev(ro_k))
  assert np.array_equal(keep[nn_k.cpu().numpy()[ok_q]], nn[ok_q]) and np.array_equal(_bits32(d2_k.cpu().numpy()[ok_q]), _bits32(d2[ok_q]))
  # a pair whose reference rows are all non-finite, and -1 / foreign rows among query_rows
  nn3, d23 = PF.feature_nn(_dev(qf), _dev(qo), _dev(np.full((320, 32), np.nan, np.float32)), _dev(ro))
  assert (nn3.cpu().numpy() == -1).all() and np.isnan(d23.cpu().numpy()).all()
  rows = np.array([5, -1, 45, 39, 40, 69, 70], dtype=np.int32)  # 45 is pair 1's row, 40 pair 1's first, 70 outside
  nn4, d24 = PF.feature_nn(_dev(qf), _dev(qo), _dev(rf), _dev(ro), query_rows=_dev(rows), query_offsets=_dev(np.array([0, 4, 7])))
  nn4 = nn4.cpu().numpy()
  assert nn4.tolist() == [clean[5], -1, -1, clean[39], clean[40], clean[69], -1] and np.isnan(d24.cpu().numpy()[[1, 2, 6]]).all()


def test_feature_nn_refusals(PF):
  from pointcontrast_amd._lib import PcmiError
  o = _dev(np.array([0, 8]))
  for c in (8, 24, 144):
    x = torch.zeros((8, c), device=DEV)
    with pytest.raises(PcmiError, match="feature width"):
      PF.feature_nn(x, o, x, o)
  x = torch.zeros((8, 32), device=DEV)
  with pytest.raises(PcmiError, match="no CPU path"):
    PF.feature_nn(x.cpu(), o, x, o)
  with pytest.raises(PcmiError, match="no CPU path"):
    PF.feature_nn(x, o, x.cpu(), o)
  with pytest.raises(PcmiError, match="no CPU path"):
    PF.match_stats(torch.zeros((8, 3), dtype=torch.float64), torch.zeros((8, 3), dtype=torch.float64, device=DEV),
                   torch.eye(4, dtype=torch.float64)[None], o, torch.zeros(8, dtype=torch.int32), [0.1])
  with pytest.raises(PcmiError, match="no CPU path"):
    PF.ransac_score(torch.zeros((8, 3), dtype=torch.float64), torch.zeros((8, 3), dtype=torch.float64), o, torch.zeros((1, 4, 3)), 0.1)
  # query_rows handed over from the host are checked there: row 5 is pair 1's
  with pytest.raises(PcmiError, match="outside its pair's segment"):
    PF.feature_nn(x, np.array([0, 4, 8]), x, np.array([0, 4, 8]), query_rows=np.array([1, 5], dtype=np.int32),
                  query_offsets=np.array([0, 2, 2]))
  with pytest.raises(PcmiError, match="hypotheses"):
    PF.ransac_score(torch.zeros((8, 3), dtype=torch.float64, device=DEV), torch.zeros((8, 3), dtype=torch.float64, device=DEV), o,
                    torch.zeros((1, 65537, 3), dtype=torch.int32, device=DEV), 0.1)


def test_feature_nn_workspace_contract():
  """The C contract: exactly the queried workspace is enough and nothing beyond it is touched; one byte less is refused."""
  from pointcontrast_amd._lib import lib
  rng = np.random.RandomState(3)
  Q, R, c = 130, 600, 32
  assert lib.pcmi_feat_nn_workspace_bytes(Q) == 8 * Q and lib.pcmi_feat_nn_workspace_bytes(0) == 0
  qf, rf = _dev(rng.normal(size=(Q, c)).astype(np.float32)), _dev(rng.normal(size=(R, c)).astype(np.float32))
  qo, ro = _dev(np.array([0, Q])), _dev(np.array([0, R]))
  ws = Guarded(8 * Q)
  out_nn, out_d2 = Guarded(4 * Q), Guarded(4 * Q)
  st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
  args = lambda nbytes: (C.c_void_p(qf.data_ptr()), c, Q, C.c_void_p(qo.data_ptr()), C.c_void_p(rf.data_ptr()), c, R,
                         C.c_void_p(ro.data_ptr()), 1, c, None, None, 0, out_nn.vp, out_d2.vp, ws.vp, C.c_size_t(nbytes), st)
  assert lib.pcmi_feat_nn(*args(8 * Q - 1)) == PCMI_ERR_WORKSPACE
  torch.cuda.synchronize()
  assert bool((out_nn.view(torch.uint8, 4 * Q) == 0xA5).all()), "a refused call wrote its output"
  assert lib.pcmi_feat_nn(*args(8 * Q)) == PCMI_OK
  torch.cuda.synchronize()
  for g, name in ((ws, "workspace"), (out_nn, "nn"), (out_d2, "d2")):
    g.check(name)
  nn = out_nn.view(torch.int32, Q).cpu().numpy()
  check_nn(qf.cpu().numpy(), np.array([0, Q]), rf.cpu().numpy(), np.array([0, R]), None, None, nn,
           out_d2.view(torch.float32, Q).cpu().numpy(), "exact workspace")


# ---- match_stats ------------------------------------------------------------------------------------------------------------
def _stats_case(seed):
  rng = np.random.RandomState(seed)
  n0, n1 = [300, 1, 280], [310, 5, 0]
  o0, o1 = fr.offsets_of(n0), fr.offsets_of(n1)
  T = np.stack([np.eye(4), fr.random_pose(rng), fr.random_pose(rng)])
  xyz0 = rng.randint(-20, 20, (o0[-1], 3)).astype(np.float64)
  xyz0[o0[1]:] *= 0.05
  xyz1 = np.empty((o1[-1], 3))
  for b in range(3):
    src = fr.apply_rigid(T[b], xyz0[o0[b]:o0[b + 1]])
    idx = np.arange(n1[b]) % n0[b] if b == 0 else rng.randint(0, max(n0[b], 1), n1[b])
    xyz1[o1[b]:o1[b + 1]] = src[idx] + (rng.normal(0, 0.03, (n1[b], 3)) if b else 0.0)
  # pair 0: integer coordinates under the identity, row j of cloud 1 is row j of cloud 0; some displaced by (3, 4, 0), whose
  # residual is exactly 25
  shift = rng.rand(n1[0]) < 0.3
  xyz1[:n1[0]][shift] += np.array([3.0, 4.0, 0.0])
  rows = np.concatenate([rng.randint(o0[b], o0[b + 1], k) for b, k in enumerate([500, 3, 40])]).astype(np.int32)
  qoffs = fr.offsets_of([500, 3, 40])
  nn01 = np.concatenate([rng.randint(o1[b], o1[b + 1], k) if n1[b] else np.full(k, -1) for b, k in enumerate([500, 3, 40])]).astype(np.int32)
  partner = rng.rand(500) < 0.8  # pair 0: mostly the true partner, so that the residuals 0 and 25 occur
  nn01[:500][partner] = rows[:500][partner]
  nn01[rng.rand(len(nn01)) < 0.1] = -1
  nn10 = np.where(rng.rand(len(rows)) < 0.5, rows, rows + 1).astype(np.int32)
  has_gt = (rng.rand(o0[-1]) < 0.6).astype(np.uint8)
  return dict(xyz0=xyz0, xyz1=xyz1, T=T, rows=rows, qoffs=qoffs, nn01=nn01, nn10=nn10, has_gt=has_gt, o0=o0)


@pytest.mark.parametrize("taus", [(5.0,), (5.0, float(np.nextafter(5.0, 0.0)), 0.1, 0.04)])
@pytest.mark.parametrize("with_gt", [False, True])
def test_match_stats_is_bit_equal_and_accumulates(PF, taus, with_gt):
  k = _stats_case(21)
  gt = k["has_gt"] if with_gt else None
  want, want_r2 = fr.match_stats(k["xyz0"], k["xyz1"], k["T"], k["qoffs"], k["nn01"], taus, k["rows"], k["nn10"], gt)
  assert (want_r2 == 25.0).sum() > 0 and (want_r2 == 0.0).sum() > 0 and np.isnan(want_r2).sum() > 40, "the case lost its edges"
  assert want[0, fr.HITS] > (want_r2[:500] < 25.0).sum(), "no residual lies exactly on the threshold"
  if len(taus) > 1:
    assert want[0, fr.HITS + 1] < want[0, fr.HITS]
  args = (_dev(k["xyz0"]), _dev(k["xyz1"]), _dev(k["T"]), _dev(k["qoffs"]), _dev(k["nn01"]), taus)
  kw = dict(query_rows=_dev(k["rows"]), nn10=_dev(k["nn10"]), has_gt=None if gt is None else _dev(gt))
  counts, r2 = PF.match_stats(*args, **kw)
  assert np.array_equal(counts.cpu().numpy(), want), (counts.cpu().numpy(), want)
  assert np.array_equal(_bits(r2.cpu().numpy()), _bits(want_r2))
  if not with_gt:
    assert (want[:, fr.N_GT] == 0).all() and (want[:, fr.HITS_GT:] == 0).all()
  counts2, _ = PF.match_stats(*args, counts=counts, **kw)  # a second call adds up
  assert counts2.data_ptr() == counts.data_ptr() and np.array_equal(counts2.cpu().numpy(), 2 * want)
  # every row of cloud 0 as a query, no mutual check
  nn_all = np.where(np.arange(k["o0"][-1]) % 7 == 0, -1, np.minimum(np.arange(k["o0"][-1]), len(k["xyz1"]) - 1)).astype(np.int32)
  want3, r23 = fr.match_stats(k["xyz0"], k["xyz1"], k["T"], k["o0"], nn_all, taus, None, None, gt)
  c3, r3 = PF.match_stats(_dev(k["xyz0"]), _dev(k["xyz1"]), _dev(k["T"]), _dev(k["o0"]), _dev(nn_all), taus,
                          has_gt=None if gt is None else _dev(gt))
  assert np.array_equal(c3.cpu().numpy(), want3) and np.array_equal(_bits(r3.cpu().numpy()), _bits(r23))
  assert (want3[:, fr.N_MUTUAL] == 0).all()


# ---- RANSAC and the refit ---------------------------------------------------------------------------------------------------
def _ransac_case(seed, H, lens=(2, 1300, 40)):
  """Matches of three pairs: 2 (below 3), 1300 (several LDS steps of 512) and 40; 60 % inliers of a planted pose with voxel
  noise, NaN rows (queries without a match), three collinear points at the head of each long segment."""
  rng = np.random.RandomState(seed)
  offs = fr.offsets_of(lens)
  src = rng.uniform(-2, 2, (offs[-1], 3))
  dst = np.empty_like(src)
  for b in range(len(lens)):
    T = fr.random_pose(rng)
    s = slice(offs[b], offs[b + 1])
    dst[s] = fr.apply_rigid(T, src[s]) + rng.uniform(-0.01, 0.01, (lens[b], 3))
    out = rng.rand(lens[b]) < 0.4
    dst[s][out] = rng.uniform(-4, 4, (int(out.sum()), 3))
    if lens[b] >= 10:
      src[offs[b] + 1] = src[offs[b]] + (src[offs[b] + 2] - src[offs[b]]) * 0.5  # 0, 1, 2 collinear in cloud 0
      dst[offs[b] + 7] = np.nan
      src[offs[b] + 9] = src[offs[b] + 8]  # 8, 9: the same point
  tri = np.stack([np.stack([rng.choice(max(n, 3), 3, replace=False) for _ in range(H)]) for n in lens]).astype(np.int32)
  if H >= 16:
    tri[:, 1] = [0, 1, 2]      # collinear
    tri[:, 2] = [3, 3, 4]      # a repeated index
    tri[:, 3] = [3, 4, 1300]   # outside every segment
    tri[:, 4] = [-1, 4, 5]
    tri[:, 5] = [7, 4, 5]      # a NaN match
    tri[:, 6] = [8, 9, 5]      # a zero-length edge
    tri[:, H - 1] = tri[:, 10]  # two equal hypotheses: a tie
    tri[:, 12] = tri[:, 10]
  return src, dst, offs, tri


@pytest.mark.parametrize("H", [1, 300])
def test_ransac_score_and_rigid_sums_are_bit_equal(PF, H):
  from pointcontrast_amd.lib.feature_match import kabsch
  src, dst, offs, tri = _ransac_case(31 + H, H)
  tau = 0.05
  want_c, want_b, want_Rt = fr.ransac_score(src, dst, offs, tri, tau)
  if H > 1:
    assert (want_c[0] == -1).all() and want_b[0] == -1, "a segment of 2 matches has no valid hypothesis"
    assert (want_c[1:, 1:7] == -1).all() and (want_c[1:, 7:] >= 3).any()
    assert (want_c[:, 10] == want_c[:, 12]).all() and (want_c[:, 10] == want_c[:, H - 1]).all()
    assert want_c[1].max() > 600, "no hypothesis found the planted pose"
  counts, best, Rt = PF.ransac_score(_dev(src), _dev(dst), _dev(offs), _dev(tri), tau)
  assert np.array_equal(counts.cpu().numpy(), want_c)
  assert np.array_equal(best.cpu().numpy(), want_b), (best.cpu().numpy(), want_b)
  assert np.array_equal(_bits(Rt.cpu().numpy()), _bits(want_Rt))
  want_s = fr.rigid_sums(src, dst, offs, want_b, want_Rt, tau)
  sums = PF.rigid_sums(_dev(src), _dev(dst), _dev(offs), best, Rt, tau).cpu().numpy()
  assert np.array_equal(_bits(sums), _bits(want_s))
  for b in range(3):
    fit = kabsch(sums[b])
    if want_b[b] < 0:
      assert fit is None and (sums[b] == 0).all()
      continue
    inl = fr.inliers(src, dst, offs, want_b, want_Rt, tau, b)
    assert sums[b, 0] == inl.sum() == want_c[b, want_b[b]]
    if inl.sum() < 4:
      continue
    R, t = fr.kabsch_points(src[offs[b]:offs[b + 1]][inl], dst[offs[b]:offs[b + 1]][inl])
    assert np.abs(fit[0] - R).max() <= 1e-9 and np.abs(fit[1] - t).max() <= 1e-9


def test_ransac_tie_between_hypotheses_goes_to_the_lowest(PF):
  """Noise-free matches: every valid hypothesis counts all of them, so best is the first valid one -- also when that one sits
  behind 255 invalid ones, in the second workgroup's share."""
  rng = np.random.RandomState(5)
  src = rng.uniform(-1, 1, (50, 3))
  T = fr.random_pose(rng)
  dst = fr.apply_rigid(T, src)
  tri = np.zeros((1, 600, 3), dtype=np.int32)  # all invalid (repeated index) ...
  tri[0, 257:] = np.stack([rng.choice(50, 3, replace=False) for _ in range(343)])  # ... up to hypothesis 257
  want_c, want_b, want_Rt = fr.ransac_score(src, dst, [0, 50], tri, 0.01)
  assert want_b[0] == 257 and (want_c[0, 257:] == 50).all()
  counts, best, Rt = PF.ransac_score(_dev(src), _dev(dst), _dev(np.array([0, 50])), _dev(tri), 0.01)
  assert np.array_equal(counts.cpu().numpy(), want_c) and best.cpu().numpy().tolist() == [257]
  assert np.array_equal(_bits(Rt.cpu().numpy()), _bits(want_Rt))


# ---- the evaluator ----------------------------------------------------------------------------------------------------------
PLANT = dict(n=400, c=32, voxel_size=0.05)


def _planted(seeds):
  return fr.collate_planted([fr.planted_pair(np.random.RandomState(s), **PLANT) for s in seeds])


def _step_args(batch, draws, on_device=False):
  """The arguments of FeatureMatchEvaluator.step: the features on the device, the rest as the loader hands it over (host) or,
  with on_device, as a device batch."""
  conv = (lambda a: _dev(np.asarray(a))) if on_device else (lambda a: a)
  from pointcontrast_amd.lib.feature_match import MatchDraws
  d = draws
  if on_device:
    d = MatchDraws(None if draws.query_rows is None else _dev(draws.query_rows),
                   None if draws.query_offsets is None else _dev(draws.query_offsets), _dev(draws.triples))
  return ((_dev(batch["F0"]), _dev(batch["F1"]), conv(batch["C0"]), conv(batch["C1"]), conv(batch["T"]), batch["len_batch"]),
          dict(correspondences=conv(batch["corr"]), draws=d))


def _step_both(ev, ref, batch, draws):
  args, kw = _step_args(batch, draws)
  ev.step(*args, **kw)


def _compare_last(ev, ref, batch, draws):
  last = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in ev.last.items()}
  # the device's matches against the restatement's own search: equal on all but near-ties
  o0, o1 = fr.offsets_of([l[0] for l in batch["len_batch"]]), fr.offsets_of([l[1] for l in batch["len_batch"]])
  want_nn, _ = fr.feat_nn(batch["F0"], o0, batch["F1"], o1, draws.query_rows, draws.query_offsets)
  assert (want_nn == last["nn01"]).mean() >= 0.99
  want = ref.step(batch["F0"], batch["F1"], batch["C0"], batch["C1"], batch["T"], batch["len_batch"], batch["corr"],
                  draws.query_rows, draws.query_offsets, draws.triples, nn=(last["nn01"], last["nn10"]))
  assert np.array_equal(last["counts"], want["counts"]), (last["counts"], want["counts"])
  assert np.array_equal(_bits(last["residual2"]), _bits(want["residual2"]))
  assert np.array_equal(last["hyp_counts"], want["hyp_counts"]) and np.array_equal(last["best"], want["best"])
  assert np.array_equal(_bits(last["Rt"]), _bits(want["Rt"])) and np.array_equal(_bits(last["sums"]), _bits(want["sums"]))


def test_evaluator_recovers_the_planted_pairs_and_accumulates():
  from pointcontrast_amd.lib.feature_match import FeatureMatchEvaluator, MatchDraws
  ev = FeatureMatchEvaluator(PLANT["voxel_size"], hit_thresholds=(0.1, 0.05), ransac_hypotheses=256)
  ref = fr.EvaluatorRef(PLANT["voxel_size"], hit_thresholds=(0.1, 0.05))
  b1, b2 = _planted((10, 11)), _planted((12,))
  d1 = MatchDraws.sample(b1["len_batch"], None, 256, np.random.RandomState(5))
  d2 = MatchDraws.sample(b2["len_batch"], 150, 256, np.random.RandomState(6))
  assert d1.query_rows is None and d2.query_rows is not None
  _step_both(ev, ref, b1, d1)
  _compare_last(ev, ref, b1, d1)
  args, kw = _step_args(b2, d2, on_device=True)
  torch.cuda.synchronize()
  torch.cuda.set_sync_debug_mode("error")  # everything is on the device: a step must not wait for it
  try:
    ev.step(*args, **kw)
  finally:
    torch.cuda.set_sync_debug_mode("default")
  _compare_last(ev, ref, b2, d2)
  m, want = ev.compute_metrics(), ref.compute_metrics()
  assert m["n_pairs"] == want["n_pairs"] == 3
  for k in want:
    if k == "pairs":
      continue
    assert m[k] == pytest.approx(want[k], abs=1e-9), k
  assert np.array_equal(m["pairs"]["counts"], want["pairs"]["counts"])
  assert np.abs(m["pairs"]["pose"] - want["pairs"]["pose"]).max() <= 1e-9
  assert m["hit_ratio_overlap@0.1"] >= 0.9 and m["registration_recall"] == 1.0
  assert (m["pairs"]["rte"] <= PLANT["voxel_size"]).all() and (m["pairs"]["rre_deg"] <= 1.0).all()
  ev.reset()
  assert ev.compute_metrics()["n_pairs"] == 0
  _step_both(ev, ref, b2, d2)
  m2 = ev.compute_metrics()
  assert m2["n_pairs"] == 1 and m2["pairs"]["counts"].tolist() == m["pairs"]["counts"][2:].tolist()


def test_evaluator_mutual_only_and_too_few_matches():
  from pointcontrast_amd.lib.feature_match import FeatureMatchEvaluator, MatchDraws
  b = _planted((13,))
  d = MatchDraws.sample(b["len_batch"], None, 64, np.random.RandomState(1))
  ev = FeatureMatchEvaluator(PLANT["voxel_size"], mutual_only=True, ransac_hypotheses=64)
  ref = fr.EvaluatorRef(PLANT["voxel_size"], mutual_only=True)
  _step_both(ev, ref, b, d)
  _compare_last(ev, ref, b, d)
  assert np.isnan(ev.last["dst"].cpu().numpy()).any()
  tiny = fr.collate_planted([fr.planted_pair(np.random.RandomState(4), n=2, c=16, voxel_size=0.05, clutter=0.0)])
  ev2 = FeatureMatchEvaluator(0.05, ransac_hypotheses=8)
  ev2.step(_dev(tiny["F0"]), _dev(tiny["F1"]), tiny["C0"], tiny["C1"], tiny["T"], tiny["len_batch"])
  m = ev2.compute_metrics()
  assert m["registration_recall"] == 0.0 and m["n_pairs"] == 1 and not m["pairs"]["registered"][0]


# ---- the trainers -----------------------------------------------------------------------------------------------------------
OVERRIDES = ["net.model=Res16UNet14", "misc.nceT=0.4", "misc.npos=256", "opt.lr=0.1", "opt.max_iter=4", "trainer.stat_freq=2",
             "trainer.num_pos_per_batch=64", "trainer.num_hn_samples_per_batch=64", "val.ransac_hypotheses=128", "val.num_queries=300"]
METRIC_KEYS = ["hit_ratio@0.1", "hit_ratio_overlap@0.1", "feature_match_recall@0.1", "mutual_ratio", "registration_recall", "rte",
               "rre_deg", "n_pairs"]


@pytest.fixture(scope="module")
def synth_batches():
  """(training batches, validation batches) of two pairs each from three items of SyntheticScanNetPairDataset, generated once
  (ray casting a pair is the slow part; that the two sets share an item does not matter here)."""
  from pointcontrast_amd.lib.config import get_config
  from pointcontrast_amd.lib.ddp_data_loaders import SyntheticScanNetPairDataset, default_collate_pair_fn
  ds = SyntheticScanNetPairDataset(config=get_config(["data.crop=0.45"]), num_pairs=3)
  items = [ds[i] for i in range(3)]
  # the validation pairs twice: as a list of batches, and as a torch DataLoader WITHOUT a generator of its own -- every
  # iter() of it takes a seed from torch's global generator, which the trainer has to put back
  plain_loader = torch.utils.data.DataLoader(items[1:3], batch_size=2, shuffle=False, collate_fn=default_collate_pair_fn)
  return [default_collate_pair_fn(items[0:2])], [default_collate_pair_fn(items[1:3])], plain_loader


def _make_trainer(name, val_freq, val_batches, train_batches):
  from pointcontrast_amd.lib import ddp_trainer
  from pointcontrast_amd.lib.config import get_config
  from pointcontrast_amd.lib.ddp_data_loaders import FixedBatchLoader
  cfg = get_config(OVERRIDES + ["trainer.trainer=%s" % name, "trainer.val_freq=%d" % val_freq])
  torch.manual_seed(3)
  np.random.seed(3)
  return getattr(ddp_trainer, name)(cfg, FixedBatchLoader(train_batches, batch_size=2), val_data_loader=val_batches)


def _state(trainer):
  torch.cuda.synchronize()
  out = {"w": trainer.flat.w.clone(), "v": trainer.flat.v.clone()}
  out.update({"sd." + k: v.clone() for k, v in trainer.model.state_dict().items()})
  return out


@pytest.mark.parametrize("name", ["PointNCELossTrainer", "HardestContrastiveLossTrainer"])
def test_validation_leaves_the_training_state_bit_identical(name, synth_batches, tmp_path, monkeypatch):
  train_batches, val_batches, plain_loader = synth_batches
  assert all(300 < n < 4000 for pair in val_batches[0]["len_batch"] for n in pair), val_batches[0]["len_batch"]
  if name == "PointNCELossTrainer":  # the trainer whose draws come from torch's global generator
    val_batches = plain_loader
  states, metrics = [], None
  for val_freq in (0, 2):
    run_dir = tmp_path / ("val%d" % val_freq)
    run_dir.mkdir()
    monkeypatch.chdir(run_dir)  # the loop saves a checkpoint into the working directory
    trainer = _make_trainer(name, val_freq, val_batches, train_batches)
    trainer.train()
    assert trainer.curr_iter == 4
    assert (trainer.val_metrics is not None) == (val_freq > 0)
    states.append(_state(trainer))
    if val_freq:
      metrics = trainer.val_metrics
      # validate: every key, finite, and the same dict when it runs again
      again = trainer.validate(val_batches)
      assert trainer.match_evaluator is not None
      for k in METRIC_KEYS:
        assert np.isfinite(metrics[k]), (k, metrics[k])
        assert metrics[k] == again[k], (k, metrics[k], again[k])
      assert metrics["n_pairs"] == 2 and np.array_equal(metrics["pairs"]["counts"], again["pairs"]["counts"])
      assert (metrics["pairs"]["counts"][:, fr.N_QUERY] == 300).all()
      states.append(_state(trainer))  # validating once more changes nothing either
  assert states[0].keys() == states[1].keys()
  for k in states[0]:
    assert torch.equal(states[0][k], states[1][k]), "validation changed %s" % k
    assert torch.equal(states[1][k], states[2][k]), "validate() changed %s" % k
  assert any(k.endswith("running_mean") for k in states[0]), "no BatchNorm running estimate was compared"


def test_eval_features_entry_point_scores_a_checkpoint(synth_batches, tmp_path, monkeypatch, capsys):
  from pointcontrast_amd import eval_features
  monkeypatch.chdir(tmp_path)
  trainer = _make_trainer("PointNCELossTrainer", 0, None, synth_batches[0])
  assert trainer.val_data_loader is None and trainer.val_freq == 0
  trainer._save_checkpoint(1, "ckpt")
  ckpt = os.path.join(str(tmp_path), "weights", "ckpt.pth")
  assert os.path.isfile(ckpt)
  empty = tmp_path / "eval"
  empty.mkdir()
  monkeypatch.chdir(empty)
  m = eval_features.main(OVERRIDES + ["misc.weight=" + ckpt, "data.val_num_pairs=2", "data.crop=0.45", "trainer.batch_size=1"])
  line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1]
  printed = json.loads(line)
  assert printed["n_pairs"] == 2 and "pairs" not in printed
  for k in METRIC_KEYS:
    assert printed[k] == m[k] and np.isfinite(printed[k])
  with pytest.raises(ValueError, match="misc.weight"):
    eval_features.main(OVERRIDES)
