"""numpy restatement of the dual-set proposal entry points of csrc/proposals.hip (pcmi_proposal_overlap, pcmi_proposal_nms)
under exactly the rules of include/pcmi.h, of downstream/insseg.py's cluster_proposals from the per-set clusterings on, and of
the evaluators' entry-wise overlap for overlapping masks.  tests/test_proposals_ref.py holds it to a brute force over Python
sets, to PointGroup's dense spelling and to planted answers; tests/test_gpu_proposals*.py hold the kernels to it.  Everything is
an integer but the one float64 division per tested pair, which numpy rounds once as the kernel does."""
import numpy as np

import insbench_ref as br
import insseg_ref as ir

MAX_SETS, MAX_PER_SCENE = 4, 1024


# ---- pcmi_proposal_overlap ------------------------------------------------------------------------------------------------------
def proposal_overlap(member, prop_scene, B, Kmax):
  """-> dict(size int32 [P], local int32 [P], scene_count int32 [B], inter int32 [B, Kmax, Kmax], dropped int)."""
  member = np.asarray(member, np.int64)
  assert member.ndim == 2, "member [n, S]"
  scene = np.asarray(prop_scene, np.int64).reshape(-1)
  P, S = len(scene), member.shape[1]
  assert 1 <= S <= MAX_SETS and 1 <= Kmax <= MAX_PER_SCENE and B >= 1
  valid = (member >= 0) & (member < P)
  size = np.bincount(member[valid], minlength=P)[:P].astype(np.int32)
  local, count, dropped = np.full(P, -1, np.int32), np.zeros(B, np.int32), 0
  for b in range(B):
    slots = np.flatnonzero(scene == b)  # ascending slot order
    count[b] = len(slots)
    local[slots[:Kmax]] = np.arange(min(len(slots), Kmax))
    dropped += max(len(slots) - Kmax, 0)
  inter = np.zeros((B, Kmax, Kmax), np.int32)
  for s in range(S):
    for t in range(s + 1, S):
      a, c = member[:, s], member[:, t]
      ok = valid[:, s] & valid[:, t]
      a, c = a[ok], c[ok]
      ok = (a != c) & (local[a] >= 0) & (local[c] >= 0) & (scene[a] == scene[c])
      a, c = a[ok], c[ok]
      np.add.at(inter, (scene[a], local[a], local[c]), 1)
      np.add.at(inter, (scene[a], local[c], local[a]), 1)
  return dict(size=size, local=local, scene_count=count, inter=inter, dropped=dropped)


# ---- pcmi_proposal_nms ----------------------------------------------------------------------------------------------------------
def mask_iou(inter, size_i, size_j):
  """(double) inter / (double) (size_i + size_j - inter): one division, whatever it gives."""
  with np.errstate(all="ignore"):
    return np.float64(int(inter)) / np.float64(int(size_i) + int(size_j) - int(inter))


def proposal_nms(overlap, prop_scene, prop_class, score, nms_iou, min_score=0.0):
  """-> keep int32 [P].  overlap: proposal_overlap's dict."""
  inter, size, local = overlap["inter"], overlap["size"], overlap["local"]
  scene, cls, score = np.asarray(prop_scene), np.asarray(prop_class), np.asarray(score, np.float64)
  P, B = len(scene), inter.shape[0]
  keep = np.zeros(P, np.int32)
  thr, floor = np.float64(nms_iou), np.float64(min_score)
  for b in range(B):
    cand = [p for p in range(P) if scene[p] == b and local[p] >= 0 and size[p] >= 1 and cls[p] >= 0 and np.isfinite(score[p]) and
            score[p] >= floor]
    cand.sort(key=lambda p: (-score[p], p))  # descending score, ascending slot among equal scores
    cand = np.asarray(cand, np.int64)
    loc, sz = np.asarray(local)[cand], np.asarray(size)[cand].astype(np.int64)
    alive = np.ones(len(cand), bool)
    for i, p in enumerate(cand):
      if not alive[i]:
        continue
      keep[p] = 1
      it = inter[b, loc[i], loc[i + 1:]].astype(np.int64)
      with np.errstate(all="ignore"):  # mask_iou on every later candidate: one division each
        iou = it.astype(np.float64) / (sz[i] + sz[i + 1:] - it).astype(np.float64)
      alive[i + 1:] &= ~(iou > thr)  # strict; a NaN suppresses nothing
  return keep


# ---- cluster_proposals, from the per-set clusterings on -------------------------------------------------------------------------
def combine_sets(parts, n_scenes, nms_iou=0.3, min_score=0.0, max_per_scene=1024):
  """parts: per set a dict of host arrays instance [n], count [1], inst_class, inst_size, inst_scene, inst_score [M]
  (cluster_instances' for that coordinate set).  -> cluster_proposals' dict without scene_offsets."""
  M, S = len(parts[0]["inst_class"]), len(parts)
  member = np.stack([np.where(p["instance"] >= 0, p["instance"].astype(np.int64) + s * M, -1) for s, p in enumerate(parts)], 1).astype(np.int32)
  cat = lambda k: np.concatenate([np.asarray(p[k]).reshape(-1) for p in parts])  # noqa: E731
  cls, scene, score = cat("inst_class"), cat("inst_scene"), cat("inst_score")
  ov = proposal_overlap(member, scene, n_scenes, max_per_scene)
  keep = proposal_nms(ov, scene, cls, score, nms_iou, min_score)
  member = np.where((member >= 0) & (keep[np.maximum(member, 0)] > 0), member, -1).astype(np.int32)
  instance = np.full(len(member), -1, np.int32)
  for i, row in enumerate(member):  # the kept proposal of the highest rank: score, then the lowest slot
    named = sorted((-score[m], m) for m in row if m >= 0)
    if named:
      instance[i] = named[0][1]
  return dict(instance=instance, count=cat("count").astype(np.int32), inst_class=np.where(keep > 0, cls, -1).astype(np.int32),
              inst_size=cat("inst_size").astype(np.int32), inst_scene=scene.astype(np.int32), inst_score=score, member=member, keep=keep,
              dropped=np.array([ov["dropped"]], np.int64))


# ---- the evaluators on overlapping masks ----------------------------------------------------------------------------------------
def member_overlap(member, gt, P, G):
  """-> inter int32 [P, G], pred_size [P] over the n S ENTRIES of member; gt_size [G] over the n ROWS."""
  member = np.asarray(member)
  S = member.shape[1]
  inter, ps, _ = ir.instance_overlap(member.reshape(-1), np.repeat(np.asarray(gt), S), P, G)
  _, _, gs = ir.instance_overlap(np.full(len(member), -1), gt, 0, G)
  return inter, ps, gs


class BenchEvaluator(br.Evaluator):
  """insbench_ref.Evaluator taking a pred with `member` [n, S]: the predictions' overlaps, sizes and void overlaps over the
  entries, the ground truth's sizes over the rows."""

  def step(self, pred, gt_instance, gt_class, n_instances=None):
    if "member" not in pred:
      return super().step(pred, gt_instance, gt_class, n_instances)
    gi, gc = np.asarray(gt_instance).astype(np.int64), np.asarray(gt_class).astype(np.int64)
    G = max(int(n_instances) if n_instances is not None else (int(gi.max()) + 1 if len(gi) else 0), 0)
    offs = np.asarray(pred["scene_offsets"])
    B = len(offs) - 1
    row_scene = np.searchsorted(offs, np.arange(len(gi)), side="right") - 1
    cls, scene = np.full(G, -1, np.int64), np.full(G, -1, np.int64)
    for g in range(G):
      rows = gi == g
      if rows.any():
        cls[g], scene[g] = max(gc[rows].max(), -1), max(row_scene[rows].max(), -1)
    scored = (cls >= 0) & (cls < self.C) & ~np.isin(cls, self.stuff)
    cls = np.where(scored, cls, -1)
    P, member = len(pred["inst_class"]), np.asarray(pred["member"])
    S = member.shape[1]
    inter, ps, gs = member_overlap(member, gi, P, G)
    void = br.void_overlap(member.reshape(-1), np.repeat(gi, S), scored, P)
    score = np.asarray(pred["inst_score"], dtype=np.float64)
    score = np.where(np.isfinite(score), score, 0.0)
    flag, self.last_state, npos = br.bench_match(inter, ps, gs, void, pred["inst_scene"], pred["inst_class"], score, scene, cls, B, self.C,
                                                 self.thr, self.min_region)
    self.npos += npos
    self.flag.append(flag)
    self.cls.append(np.asarray(pred["inst_class"]).astype(np.int64))
    self.score.append(score)

  def step_points(self, coords, pred, transformation, points, point_instance, point_class, point_offsets):
    inst = br.carry_instances(coords, pred["instance"], transformation, points, point_offsets)
    carried = dict(pred, instance=inst, scene_offsets=np.asarray(point_offsets))
    if "member" in pred:
      member = np.asarray(pred["member"])
      carried["member"] = np.stack([br.carry_instances(coords, member[:, s], transformation, points, point_offsets)
                                    for s in range(member.shape[1])], 1)
    self.step(carried, point_instance, point_class)
    return inst


# ---- the planted cases the CPU and the GPU tests share --------------------------------------------------------------------------
def _case(columns, n, scene, cls, score, B=1, Kmax=8, nms_iou=0.3, min_score=0.0, keep=None, dropped=0):
  """columns: per column a dict {proposal: (first row, one past the last row)}."""
  member = np.full((n, len(columns)), -1, np.int32)
  for s, col in enumerate(columns):
    for p, (a, b) in col.items():
      member[a:b, s] = p
  return dict(member=member, prop_scene=np.asarray(scene, np.int32), prop_class=np.asarray(cls, np.int32),
              score=np.asarray(score, np.float64), B=B, Kmax=Kmax, nms_iou=nms_iou, min_score=min_score,
              keep=None if keep is None else np.asarray(keep, np.int32), dropped=dropped)


def planted_cases():
  """name -> the arguments of the two calls and the planted keep / dropped.  Column 0 owns slots 0 - 3, column 1 slots 4 - 7."""
  U = -1  # an unused slot
  cases = {}
  # A (slot 0, rows 0 - 9) > B (slot 4, rows 4 - 17) > C (slot 1, rows 12 - 21): A n B = B n C = 6 rows, IoU 6 / 18 and 6 / 18;
  # A n C is empty.  A suppresses B; ONLY B overlaps C, and B is dead: C is kept.
  cases["chain"] = _case([{0: (0, 10), 1: (12, 22)}, {4: (4, 18)}], 24, [0, 0, U, U, 0, U, U, U], [2, 2, U, U, 2, U, U, U],
                         [0.9, 0.7, 0, 0, 0.8, 0, 0, 0], keep=[1, 1, 0, 0, 0, 0, 0, 0])
  # 3 rows shared by proposals of 5 and 8 rows: 3 / 10 against 0.3 -- equal, not above: both kept
  cases["iou at the threshold"] = _case([{0: (0, 5)}, {4: (2, 10)}], 12, [0, U, U, U, 0, U, U, U], [3, U, U, U, 3, U, U, U],
                                        [0.9, 0, 0, 0, 0.8, 0, 0, 0], keep=[1, 0, 0, 0, 1, 0, 0, 0])
  # one row more in common: 4 / 9 > 0.3
  cases["iou above the threshold"] = _case([{0: (0, 5)}, {4: (1, 9)}], 12, [0, U, U, U, 0, U, U, U], [3, U, U, U, 3, U, U, U],
                                           [0.9, 0, 0, 0, 0.8, 0, 0, 0], keep=[1, 0, 0, 0, 0, 0, 0, 0])
  # equal scores: the lower slot ranks first, although it is the smaller mask and stands in the later rows
  cases["equal scores"] = _case([{1: (4, 10)}, {4: (0, 10)}], 10, [U, 0, U, U, 0, U, U, U], [U, 2, U, U, 2, U, U, U],
                                [0, 0.5, 0, 0, 0.5, 0, 0, 0], keep=[0, 1, 0, 0, 0, 0, 0, 0])
  # slot 0 (NaN) and slot 1 (below min_score) are no candidates: they are not kept and suppress nothing, so slots 4 and 5, which
  # they cover entirely, stay; slot 2 sits exactly at min_score and is a candidate
  cases["NaN and low scores"] = _case([{0: (0, 10), 1: (10, 20), 2: (20, 30)}, {4: (0, 10), 5: (10, 20)}], 30,
                                      [0, 0, 0, U, 0, 0, U, U], [2, 2, 2, U, 2, 2, U, U], [np.nan, 0.2, 0.25, 0, 0.5, 0.6, 0, 0],
                                      min_score=0.25, keep=[0, 0, 1, 0, 1, 1, 0, 0])
  # the same rows in two scenes' proposals (which no clustering produces): a pair across scenes counts nowhere
  cases["pair across scenes"] = _case([{0: (0, 10)}, {4: (0, 10)}], 10, [0, U, U, U, 1, U, U, U], [2, U, U, U, 2, U, U, U],
                                      [0.9, 0, 0, 0, 0.8, 0, 0, 0], B=2, keep=[1, 0, 0, 0, 1, 0, 0, 0])
  # Kmax + 1 proposals in one scene: the last in slot order is dropped -- never kept, though it has the highest score, and it
  # suppresses nothing: slot 0, which it covers, is kept
  cases["Kmax + 1 in a scene"] = _case([{0: (0, 10), 1: (10, 20), 2: (20, 30), 3: (30, 40)}, {4: (0, 10)}], 40,
                                       [0, 0, 0, 0, 0, U, U, U], [2, 2, 2, 2, 2, U, U, U], [0.5, 0.5, 0.5, 0.5, 0.9, 0, 0, 0], Kmax=4,
                                       keep=[1, 1, 1, 1, 0, 0, 0, 0], dropped=1)
  # an empty mask (size 0), a proposal of class -1: no candidates
  cases["empty mask and no class"] = _case([{0: (0, 10)}, {5: (0, 10)}], 10, [0, U, U, U, 0, 0, U, U], [2, U, U, U, 2, U, U, U],
                                           [0.5, 0, 0, 0, 0.9, 0.8, 0, 0], keep=[1, 0, 0, 0, 0, 0, 0, 0])
  return cases


def run_case(case, overlap_fn=proposal_overlap, nms_fn=proposal_nms):
  ov = overlap_fn(case["member"], case["prop_scene"], case["B"], case["Kmax"])
  return ov, nms_fn(ov, case["prop_scene"], case["prop_class"], case["score"], case["nms_iou"], case["min_score"])


def random_case(seed, n, S, B, M, Kmax=64, run=1, outside=0.1):
  """Random proposals: per column a random partition of the rows into runs of `run` equal values, ids in the column's slots
  [s M, (s + 1) M) (a share `outside` of ids outside [0, S M)); every slot gets a random scene in [-1, B), a class in [-1, 3)
  and a score in multiples of 1 / 8 (ties)."""
  rng = np.random.default_rng(seed)
  P = S * M
  m = -(-n // run) if n else 0
  member = np.full((n, S), -1, np.int32)
  for s in range(S):
    ids = rng.integers(s * M, (s + 1) * M, m)
    out = rng.random(m) < outside
    ids = np.where(out, rng.choice([-1, -7, P, P + 5], m), ids)
    member[:, s] = np.repeat(ids, run)[:n]
  return dict(member=member, prop_scene=rng.integers(-1, B, P).astype(np.int32), prop_class=rng.integers(-1, 3, P).astype(np.int32),
              score=rng.integers(0, 9, P) / 8.0, B=B, Kmax=Kmax, nms_iou=0.3, min_score=0.0, keep=None, dropped=None)


def crowded_case(K, Kmax, B=1, seed=0, S=2, rows=6):
  """K proposals in scene 0 (B > 1: and K // 3 in the last scene; the scenes between have none).  Proposal k stands in column
  k % S, slot (k % S) M + k // S, on the rows [k h, k h + 2 h), h = rows // 2, where its column is still free: with S >= 2 it
  shares h rows with proposal k + 1 (IoU 1 / 3 > 0.3) -- suppression chains through every word of the bit matrix, which five
  different scores with many ties break up -- and a scene's index order (by slot) differs from k."""
  rng = np.random.default_rng(seed)
  T = K + (K // 3 if B > 1 else 0)
  M, h = -(-T // S) + 1, rows // 2
  P = S * M
  scene, cls, score = np.full(P, -1, np.int32), np.full(P, -1, np.int32), np.zeros(P)
  member = np.full((h * (T + 1), S), -1, np.int32)
  for k in range(T):
    col = k % S
    p = col * M + k // S
    scene[p], cls[p], score[p] = (0 if k < K else B - 1), 2, rng.integers(1, 6) / 8.0
    seg = member[k * h:(k + 2) * h, col]
    seg[seg < 0] = p
  return dict(member=member, prop_scene=scene, prop_class=cls, score=score, B=B, Kmax=Kmax, nms_iou=0.3, min_score=0.0, keep=None,
              dropped=None)
