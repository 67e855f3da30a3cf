"""tests/proposals_ref.py -- the numpy restatement the GPU tests of csrc/proposals.hip compare with -- held to (a) a brute force
over Python sets, one set of rows per proposal, (b) PointGroup's dense spelling written fresh here (an integer indicator matrix
[proposals, rows] times its transpose, then the textbook greedy loop over an argsort) and (c) planted answers.  No GPU."""
import numpy as np
import pytest

import proposals_ref as pr


def _used(case):
  """Per scene the slots that take part: the first Kmax used slots in slot order."""
  scene = case["prop_scene"]
  return [np.flatnonzero(scene == b)[:case["Kmax"]] for b in range(case["B"])]


# ---- (a) brute force over sets ------------------------------------------------------------------------------------------------------
def brute_force(case):
  member, scene, P = case["member"], case["prop_scene"], len(case["prop_scene"])
  rows_of, size = [set() for _ in range(P)], np.zeros(P, np.int32)
  for i, row in enumerate(member.tolist()):
    for m in row:
      if 0 <= m < P:
        rows_of[m].add(i)
        size[m] += 1
  local, inter = np.full(P, -1, np.int32), np.zeros((case["B"], case["Kmax"], case["Kmax"]), np.int32)
  keep = np.zeros(P, np.int32)
  for b, slots in enumerate(_used(case)):
    for k, p in enumerate(slots):
      local[p] = k
    for i, a in enumerate(slots):
      for j, c in enumerate(slots):
        if a != c:
          inter[b, i, j] = len(rows_of[a] & rows_of[c])
    cand = [p for p in slots if size[p] >= 1 and case["prop_class"][p] >= 0 and np.isfinite(case["score"][p]) and
            case["score"][p] >= case["min_score"]]
    kept = []
    for p in sorted(cand, key=lambda p: (-case["score"][p], p)):  # p stays unless a KEPT proposal before it covers it
      if not any(pr.mask_iou(len(rows_of[q] & rows_of[p]), size[q], size[p]) > case["nms_iou"] for q in kept):
        kept.append(p)
    keep[kept] = 1
  dropped = sum(max(int((scene == b).sum()) - case["Kmax"], 0) for b in range(case["B"]))
  return dict(size=size, local=local, inter=inter, dropped=dropped), keep


CASES = {
    "random S 1": lambda: pr.random_case(1, 300, 1, 2, 12, Kmax=16),
    "random S 2": lambda: pr.random_case(2, 400, 2, 3, 10, Kmax=16, run=7),
    "random S 3, a scene beyond Kmax": lambda: pr.random_case(3, 500, 3, 2, 9, Kmax=8, run=5),
    "random S 4": lambda: pr.random_case(4, 500, 4, 3, 8, Kmax=16, run=11),
    "crowded 65": lambda: pr.crowded_case(65, 80),
    "crowded 70 of 64, two scenes": lambda: pr.crowded_case(70, 64, B=3, S=3),
}


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_the_brute_force_over_sets(name):
  case = CASES[name]()
  ov, keep = pr.run_case(case)
  want, want_keep = brute_force(case)
  for k in ("size", "local", "inter"):
    assert ov[k].dtype == np.int32 and np.array_equal(ov[k], want[k]), k
  assert ov["dropped"] == want["dropped"]
  assert np.array_equal(ov["scene_count"], [int((case["prop_scene"] == b).sum()) for b in range(case["B"])])
  assert np.array_equal(ov["inter"], ov["inter"].transpose(0, 2, 1)) and not ov["inter"][:, np.arange(case["Kmax"]), np.arange(case["Kmax"])].any()
  assert keep.dtype == np.int32 and np.array_equal(keep, want_keep)
  if name.startswith("crowded"):
    assert 0 < keep.sum() < (ov["local"] >= 0).sum(), "some are suppressed, some survive"
  if "beyond" in name or "70 of 64" in name:
    assert ov["dropped"] > 0 and not keep[(case["prop_scene"] >= 0) & (ov["local"] < 0)].any()


# ---- (b) the dense spelling ---------------------------------------------------------------------------------------------------------
def dense_spelling(case):
  """PointGroup's: proposals_idx -> a [proposals, rows] indicator, intersection = A A^T, iou = inter / (size_i + size_j - inter),
  then the greedy loop over the scores' argsort.  Per scene, as the union is taken per scene."""
  member, P = case["member"], len(case["prop_scene"])
  A = np.zeros((P, len(member)), np.int64)
  for s in range(member.shape[1]):
    ok = (member[:, s] >= 0) & (member[:, s] < P)
    A[member[ok, s], np.flatnonzero(ok)] = 1
  size = A.sum(1)
  keep = np.zeros(P, np.int32)
  for slots in _used(case):
    score = case["score"][slots]
    ok = (size[slots] >= 1) & (case["prop_class"][slots] >= 0) & np.isfinite(score) & (score >= case["min_score"])
    idx = slots[ok]
    a = A[idx]
    inter = a @ a.T
    with np.errstate(all="ignore"):
      iou = inter / (size[idx][:, None] + size[idx][None, :] - inter).astype(np.float64)
    np.fill_diagonal(iou, 0.0)
    gone = np.zeros(len(idx), bool)
    for i in np.argsort(-case["score"][idx], kind="stable"):
      if gone[i]:
        continue
      keep[idx[i]] = 1
      gone |= iou[i] > case["nms_iou"]
  return size.astype(np.int32), keep


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_the_dense_spelling(name):
  case = CASES[name]()
  ov, keep = pr.run_case(case)
  size, want_keep = dense_spelling(case)
  assert np.array_equal(ov["size"], size) and np.array_equal(keep, want_keep)


# ---- (c) planted answers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pr.planted_cases()))
def test_planted_answers(name):
  case = pr.planted_cases()[name]
  ov, keep = pr.run_case(case)
  assert keep.tolist() == case["keep"].tolist() and ov["dropped"] == case["dropped"]
  assert np.array_equal(keep, brute_force(case)[1]) and np.array_equal(keep, dense_spelling(case)[1])


def test_planted_numbers_are_what_the_comments_say():
  cases = pr.planted_cases()
  ov, _ = pr.run_case(cases["chain"])
  a, c, b = ov["local"][[0, 1, 4]]
  assert ov["size"][[0, 1, 4]].tolist() == [10, 10, 14] and ov["inter"][0, a, b] == 6 and ov["inter"][0, b, c] == 6 and ov["inter"][0, a, c] == 0
  any_higher = [p for p in (0, 1, 4) if not any(cases["chain"]["score"][q] > cases["chain"]["score"][p] and
                                                 ov["inter"][0, ov["local"][q], ov["local"][p]] > 0 for q in (0, 1, 4))]
  assert any_higher == [0], "suppressing on ANY higher-scored overlap would lose C"
  ov, _ = pr.run_case(cases["iou at the threshold"])
  assert ov["size"][[0, 4]].tolist() == [5, 8] and ov["inter"][0, 0, 1] == 3 and pr.mask_iou(3, 5, 8) == 0.3
  ov, _ = pr.run_case(cases["pair across scenes"])
  assert not ov["inter"].any() and ov["scene_count"].tolist() == [1, 1] and ov["local"][[0, 4]].tolist() == [0, 0]
  ov, _ = pr.run_case(cases["Kmax + 1 in a scene"])
  assert ov["scene_count"].tolist() == [5] and ov["local"].tolist() == [0, 1, 2, 3, -1, -1, -1, -1] and not ov["inter"].any()


def test_the_quotient_is_one_division_whatever_it_gives():
  """The division is not guarded: a NaN compares false (suppresses nothing), an infinity and a negative threshold suppress."""
  assert np.isnan(pr.mask_iou(0, 0, 0)) and not pr.mask_iou(0, 0, 0) > 0.3 and pr.mask_iou(2, 1, 1) == np.inf
  ov = dict(inter=np.zeros((1, 2, 2), np.int32), size=np.array([1, 1], np.int32), local=np.array([0, 1], np.int32))
  assert pr.proposal_nms(ov, [0, 0], [2, 2], [0.9, 0.8], 0.3).tolist() == [1, 1]
  assert pr.proposal_nms(ov, [0, 0], [2, 2], [0.9, 0.8], -1.0).tolist() == [1, 0], "0 > -1"
  ov["inter"][0] = [[0, 1], [1, 0]]
  assert pr.proposal_nms(ov, [0, 0], [2, 2], [0.8, 0.9], 0.3).tolist() == [0, 1], "1 / 1"
  ov["inter"][0] = [[0, 2], [2, 0]]  # sizes that contradict the intersection, which no overlap call produces: 2 / 0
  assert pr.proposal_nms(ov, [0, 0], [2, 2], [0.9, 0.8], 0.3).tolist() == [1, 0]


def test_the_limits_are_the_kernels_own():
  import os
  import re
  root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "pointcontrast_amd")
  src, fn = open(os.path.join(root, "csrc", "proposals.hip")).read(), open(os.path.join(root, "functional.py")).read()
  sets, per_scene = (int(re.search(r"constexpr int %s = (\d+);" % k, src).group(1)) for k in ("kMaxSets", "kMaxK"))
  assert (sets, per_scene) == (pr.MAX_SETS, pr.MAX_PER_SCENE) and per_scene == 1 << int(re.search(r"constexpr int kLocalBits = (\d+);", src).group(1))
  assert int(re.search(r"^PROPOSAL_MAX_SETS = (\d+)", fn, re.M).group(1)) == sets
  assert int(re.search(r"^PROPOSAL_MAX_PER_SCENE = (\d+)", fn, re.M).group(1)) == per_scene
  assert "proposals.hip" in open(os.path.join(root, "build.py")).read()


# ---- the evaluators' entry-wise overlap ---------------------------------------------------------------------------------------------
def test_member_overlap_counts_entries_for_predictions_and_rows_for_ground_truth():
  member = np.array([[0, 2], [0, 2], [0, -1], [-1, 3], [1, 3], [1, 5]], np.int32)  # 5: outside [0, 4)
  gt = np.array([0, 0, 1, 1, 1, -1])
  inter, ps, gs = pr.member_overlap(member, gt, 4, 2)
  assert inter.tolist() == [[2, 1], [0, 1], [2, 0], [0, 2]] and ps.tolist() == [3, 2, 2, 2] and gs.tolist() == [2, 3]
  one, ps1, gs1 = pr.member_overlap(member[:, :1], gt, 4, 2)
  want = pr.ir.instance_overlap(member[:, 0], gt, 4, 2)
  assert all(np.array_equal(a, b) for a, b in zip((one, ps1, gs1), want)), "one column: instance_overlap itself"


def test_combine_sets_numbers_slots_per_set_and_picks_the_best_column():
  """Two sets of M = 3 slots on 12 rows: set 0 holds {rows 0 - 5} (0.6) and {6 - 11} (0.9); set 1 holds {0 - 2} (0.8),
  {3 - 5} (0.7) and {6 - 11} (0.9).  Rank: slot 1 (0.9), slot 5 (0.9; equal to slot 1: iou 1, suppressed), slot 3 (0.8),
  slot 4 (0.7), slot 0 (0.6; 3 / 6 with both halves, both kept before it: suppressed)."""
  r = np.arange(12)
  parts = [dict(instance=np.where(r < 6, 0, 1).astype(np.int32), count=np.array([2], np.int32), inst_class=np.array([2, 2, -1], np.int32),
                inst_size=np.array([6, 6, 0], np.int32), inst_scene=np.array([0, 0, -1], np.int32), inst_score=np.array([0.6, 0.9, 0.0])),
           dict(instance=np.where(r < 3, 0, np.where(r < 6, 1, 2)).astype(np.int32), count=np.array([3], np.int32),
                inst_class=np.array([2, 2, 2], np.int32), inst_size=np.array([3, 3, 6], np.int32), inst_scene=np.array([0, 0, 0], np.int32),
                inst_score=np.array([0.8, 0.7, 0.9]))]
  out = pr.combine_sets(parts, 1)
  assert out["keep"].tolist() == [0, 1, 0, 1, 1, 0] and out["inst_class"].tolist() == [-1, 2, -1, 2, 2, -1]
  assert out["count"].tolist() == [2, 3] and out["inst_size"].tolist() == [6, 6, 0, 3, 3, 6] and out["dropped"].tolist() == [0]
  assert out["member"].tolist() == [[-1, 3]] * 3 + [[-1, 4]] * 3 + [[1, -1]] * 6
  assert out["instance"].tolist() == [3] * 3 + [4] * 3 + [1] * 6
  both = pr.combine_sets(parts, 1, nms_iou=1.0)  # nothing above 1: everything stays, rows take the higher score, then the lower slot
  assert both["keep"].tolist() == [1, 1, 0, 1, 1, 1] and both["instance"].tolist() == [3] * 3 + [4] * 3 + [1] * 6
