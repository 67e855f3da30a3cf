"""The dual-set proposal kernels (csrc/proposals.hip: pcmi_proposal_overlap, pcmi_proposal_nms, functional.py's wrappers) against
tests/proposals_ref.py, which tests/test_proposals_ref.py holds to a brute force over sets, to PointGroup's dense spelling and to
planted answers.  Counts are integers and every tested pair is one float64 division: everything is compared EXACTLY.  Shapes
are the smallest that reach each path: rows around a wave, every number of sets, proposals per scene around a word of the
suppression bits (64), around the boundary between the two kernel instantiations (Kmax 256 | 257) and around the limit (1024)."""
import ctypes as C

import numpy as np
import pytest
import torch

import proposals_ref as pr
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
  return C.c_void_p(t.data_ptr()) if t.numel() else None


def device_run(PF, case, member=None):
  """The two calls on the device -> (overlap dict of host arrays with `dropped`, keep)."""
  dropped = torch.zeros(1, dtype=torch.int64, device=DEV)
  ov = PF.proposal_overlap(_dev(case["member"]) if member is None else member, _dev(case["prop_scene"]), case["B"], case["Kmax"], dropped)
  keep = PF.proposal_nms(ov, _dev(case["prop_scene"]), _dev(case["prop_class"]), _dev(case["score"]), case["nms_iou"], case["min_score"])
  assert all(ov[k].dtype == torch.int32 for k in ov) and keep.dtype == torch.int32
  assert tuple(ov["inter"].shape) == (case["B"], case["Kmax"], case["Kmax"]) and tuple(ov["scene_count"].shape) == (case["B"],)
  out = {k: v.cpu().numpy() for k, v in ov.items()}
  out["dropped"] = int(dropped.cpu())
  return out, keep.cpu().numpy()


def check(PF, case, what, member=None):
  """Both calls equal the restatement; returns the restatement's (overlap, keep)."""
  want, want_keep = pr.run_case(case)
  got, keep = device_run(PF, case, member)
  for k in ("size", "local", "scene_count", "dropped"):
    assert np.array_equal(got[k], want[k]), "%s: %s differs" % (what, k)
  bad = np.argwhere(got["inter"] != want["inter"])
  assert len(bad) == 0, "%s: %d intersections differ, first at (b, i, j) %s: got %d want %d" % (
      what, len(bad), bad[0].tolist(), got["inter"][tuple(bad[0])], want["inter"][tuple(bad[0])])
  bad = np.flatnonzero(keep != want_keep)
  assert len(bad) == 0, "%s: keep differs at %d slots, first %d: got %d want %d" % (what, len(bad), bad[0], keep[bad[0]], want_keep[bad[0]])
  return want, want_keep


# ---- rows around a wave, every number of sets ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 3, 4])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_rows_around_a_wave_and_every_number_of_sets(PF, n, S):
  want, _ = check(PF, pr.random_case(100 * S + n, n, S, 2, 5, Kmax=8, run=3), "n %d S %d" % (n, S))
  assert want["size"].sum() >= n // 2 and (S > 1 or not want["inter"].any()), "one set: no pairs"


def test_member_as_a_column_slice_of_a_wider_tensor(PF):
  case = pr.random_case(5, 777, 2, 3, 7, Kmax=16, run=9)
  wide = torch.full((777, 5), 3, dtype=torch.int32, device=DEV)  # the columns beside the slice name a valid proposal
  wide[:, 1:3] = _dev(case["member"])
  member = wide[:, 1:3]
  assert not member.is_contiguous()
  want, _ = check(PF, case, "column slice", member)
  assert want["inter"].any()


# ---- the wave aggregation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", [1, 64, 50], ids=["pairs change inside every wave", "wave-uniform pairs", "runs of 50 broken here and there"])
def test_100000_rows_with_ids_outside_on_both_sides_against_unique_counts(PF, run):
  n, S, M, B = 100000, 2, 24, 3
  case = pr.random_case(7 + run, n, S, B, M, Kmax=64, run=run, outside=0.15)
  member, P = case["member"], S * M
  if run == 50:
    member[::97, 0] = (member[::97, 0] + 1) % M  # runs broken up here and there
    member[::89, 1] = M + (member[::89, 1] + 1) % M
  want, _ = check(PF, case, "run %d" % run)
  # the same counts from np.unique, without the restatement
  valid = (member >= 0) & (member < P)
  assert (~valid[:, 0]).sum() > 5000 and (~valid[:, 1]).sum() > 5000 and (member < 0).any() and (member >= P).any()
  ids, counts = np.unique(member[valid], return_counts=True)
  size = np.zeros(P, np.int64)
  size[ids] = counts
  assert np.array_equal(want["size"], size)
  both = valid.all(1)
  a, c = member[both, 0].astype(np.int64), member[both, 1].astype(np.int64)
  scene, local = case["prop_scene"], want["local"]
  ok = (scene[a] >= 0) & (scene[a] == scene[c]) & (local[a] >= 0) & (local[c] >= 0)
  keys, counts = np.unique(a[ok] * P + c[ok], return_counts=True)
  assert len(keys) > 50 and counts.sum() > 10000
  for key, cnt in zip(keys.tolist(), counts.tolist()):
    pa, pc = key // P, key % P
    assert want["inter"][scene[pa], local[pa], local[pc]] == cnt and want["inter"][scene[pa], local[pc], local[pa]] == cnt
  assert want["inter"].sum() == 2 * counts.sum()


def test_100000_rows_that_all_name_one_pair(PF):
  n = 100000
  member = np.tile(np.array([[2, 9]], np.int32), (n, 1))
  case = dict(member=member, prop_scene=np.array([-1, -1, 1, -1, -1, -1, -1, 1, -1, 1, -1, -1], np.int32),
              prop_class=np.full(12, 2, np.int32), score=np.linspace(0.1, 0.9, 12), B=2, Kmax=4, nms_iou=0.3, min_score=0.0)
  want, keep = check(PF, case, "one pair")
  assert want["size"][[2, 9]].tolist() == [n, n] and want["local"][[2, 7, 9]].tolist() == [0, 1, 2]
  assert want["inter"][1].tolist() == [[0, 0, n, 0], [0, 0, 0, 0], [n, 0, 0, 0], [0, 0, 0, 0]] and not want["inter"][0].any()
  assert keep.tolist() == [0] * 9 + [1, 0, 0], "slot 9 (0.75) covers slot 2; slot 7 has no rows"


# ---- proposals per scene: the words of the suppression bits, the two instantiations, the limit ------------------------------------
@pytest.mark.parametrize("K,Kmax", [(63, 64), (64, 64), (65, 64), (63, 256), (64, 256), (65, 256), (255, 256), (256, 256), (257, 256),
                                    (255, 257), (256, 257), (257, 257), (1023, 1024), (1024, 1024), (1025, 1024)])
def test_proposals_per_scene(PF, K, Kmax):
  """crowded_case: every proposal overlaps its two neighbours above the threshold, so the sweep walks chains through every
  word.  Kmax <= 256 takes the 256-thread instantiation, Kmax = 257 and 1024 the 1024-thread one."""
  case = pr.crowded_case(K, Kmax, seed=K)
  want, keep = check(PF, case, "K %d Kmax %d" % (K, Kmax))
  assert want["scene_count"].tolist() == [K] and want["dropped"] == max(K - Kmax, 0)
  used = min(K, Kmax)
  assert (want["local"] >= 0).sum() == used and used // 3 <= keep.sum() < used, "chains: a part is suppressed, a part survives"


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S", [2, 3])
def test_scenes_without_proposals_between_scenes_that_have_some(PF, B, S):
  case = pr.crowded_case(70, 80, B=B, S=S, seed=B)
  want, keep = check(PF, case, "B %d S %d" % (B, S))
  assert want["scene_count"].tolist() == ([70] if B == 1 else [70, 0, 23]) and keep.sum() > 20
  none = dict(case, prop_scene=np.full_like(case["prop_scene"], -1))  # no proposal anywhere
  want, keep = check(PF, none, "no proposals")
  assert not keep.any() and not want["inter"].any() and want["size"].sum() > 0


def test_more_than_the_limit_is_refused(PF):
  from pointcontrast_amd._lib import PcmiError, lib
  case = pr.crowded_case(10, 1025)
  with pytest.raises(PcmiError, match="-6.*at most 1024"):
    PF.proposal_overlap(_dev(case["member"]), _dev(case["prop_scene"]), 1, 1025)
  P = len(case["prop_scene"])
  z = torch.zeros(P, dtype=torch.int32, device=DEV)
  score = torch.zeros(P, dtype=torch.float64, device=DEV)
  keep = torch.full((P,), 7, dtype=torch.int32, device=DEV)
  rc = lib.pcmi_proposal_nms(_vp(z), _vp(z), _vp(z), _vp(z), _vp(z), _vp(z), _vp(score), P, 1, 1025, 0.3, 0.0, _vp(keep), _stream())
  assert rc == PCMI_ERR_UNSUPPORTED
  torch.cuda.synchronize()
  assert bool((keep == 7).all()), "a refused call enqueues nothing"


# ---- the planted answers of the CPU tests -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pr.planted_cases()))
def test_planted_cases(PF, name):
  case = pr.planted_cases()[name]
  got, keep = device_run(PF, case)
  assert keep.tolist() == case["keep"].tolist() and got["dropped"] == case["dropped"]
  check(PF, case, name)


def test_scores_with_ties_infinities_and_negative_zero(PF):
  case = pr.crowded_case(130, 256, seed=4)
  used = np.flatnonzero(case["prop_scene"] == 0)
  case["score"][used[::7]] = np.inf    # not finite: no candidate
  case["score"][used[1::7]] = -0.0     # >= 0.0: a candidate, equal to 0.0
  case["score"][used[2::7]] = 0.0
  case["score"][used[3::7]] = np.nan
  case["score"][used[4::7]] = -1e-300  # below min_score
  want, keep = check(PF, case, "special scores")
  assert not keep[used[::7]].any() and not keep[used[3::7]].any() and not keep[used[4::7]].any() and keep[used[1::7]].any()


# ---- the C entry points in exactly the queried workspace, between guard bands, twice ----------------------------------------------
def test_entry_points_guarded_exact_workspace_and_determinism():
  from pointcontrast_amd._lib import lib
  case = pr.random_case(21, 5000, 3, 2, 20, Kmax=32, run=13)
  want, want_keep = pr.run_case(case)
  n, S, P, B, K = 5000, 3, 60, 2, 32
  wide = torch.full((n, 4), -1, dtype=torch.int32, device=DEV)  # ld 4 > S
  wide[:, :3] = _dev(case["member"])
  scene, cls, score = _dev(case["prop_scene"]), _dev(case["prop_class"]), _dev(case["score"])
  need = lib.pcmi_proposal_overlap_workspace_bytes(P)
  assert need >= P * 4 and lib.pcmi_proposal_overlap_workspace_bytes(-1) == 0
  runs = []
  for _ in range(2):
    size, local, count, inter, ws, keep = Guarded(P * 4), Guarded(P * 4), Guarded(B * 4), Guarded(B * K * K * 4), Guarded(need), Guarded(P * 4)
    dropped = torch.zeros(1, dtype=torch.int64, device=DEV)
    rc = lib.pcmi_proposal_overlap(_vp(wide), 4, n, S, _vp(scene), P, B, K, size.vp, local.vp, count.vp, inter.vp, _vp(dropped), ws.vp, ws.size,
                                   _stream())
    assert rc == PCMI_OK, lib.pcmi_last_error()
    rc = lib.pcmi_proposal_nms(inter.vp, size.vp, local.vp, count.vp, _vp(scene), _vp(cls), _vp(score), P, B, K, 0.3, 0.0, keep.vp, _stream())
    assert rc == PCMI_OK, lib.pcmi_last_error()
    torch.cuda.synchronize()
    for g, what in ((size, "size"), (local, "local"), (count, "scene_count"), (inter, "inter"), (ws, "workspace"), (keep, "keep")):
      g.check(what)
    runs.append([g.view(torch.int32, m).cpu().numpy().copy() for g, m in ((size, P), (local, P), (count, B), (inter, B * K * K), (keep, P))] +
                [dropped.cpu().numpy()])
  h_size, h_local, h_count, h_inter, h_keep, h_dropped = runs[0]
  assert np.array_equal(h_size, want["size"]) and np.array_equal(h_local, want["local"]) and np.array_equal(h_count, want["scene_count"])
  assert np.array_equal(h_inter, want["inter"].reshape(-1)) and np.array_equal(h_keep, want_keep) and int(h_dropped[0]) == want["dropped"]
  assert h_inter.any() and 0 < h_keep.sum() < (h_local >= 0).sum()
  for a, b in zip(runs[0], runs[1]):
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "the same bits from run to run"
  # refusals enqueue nothing
  out, small = Guarded(B * K * K * 4), Guarded(need - 1)
  st = _stream()
  call = lambda S_=S, ld=4, B_=B, K_=K, ws=ws, nbytes=None: lib.pcmi_proposal_overlap(  # noqa: E731
      _vp(wide), ld, n, S_, _vp(scene), P, B_, K_, size.vp, local.vp, count.vp, out.vp, None, ws.vp, ws.size if nbytes is None else nbytes, st)
  assert call(ws=small) == PCMI_ERR_WORKSPACE
  assert call(S_=0) == PCMI_ERR_INVALID and call(S_=5) == PCMI_ERR_INVALID and call(ld=2) == PCMI_ERR_INVALID
  assert call(B_=0) == PCMI_ERR_INVALID and call(K_=0) == PCMI_ERR_INVALID and call(K_=1025) == PCMI_ERR_UNSUPPORTED
  torch.cuda.synchronize()
  assert bool((out.buf == 0xA5).all()), "a refused call must enqueue nothing"
  # no rows and no proposals
  assert lib.pcmi_proposal_overlap(None, 2, 0, 2, None, 0, B, K, None, None, count.vp, inter.vp, None, ws.vp, ws.size, st) == PCMI_OK
  assert lib.pcmi_proposal_nms(None, None, None, None, None, None, None, 0, B, K, 0.3, 0.0, None, st) == PCMI_OK
  torch.cuda.synchronize()
  assert not count.view(torch.int32, B).any() and not inter.view(torch.int32, B * K * K).any()
  inter.check("inter, P = 0")
