"""Validation of the pre-training on held-out pairs: feature matching between the two clouds of a pair, on the device.

The reference has no validation (pc/lib/ddp_trainer.py logs the contrastive loss and nothing else).  Its trainers descend
from FCGF's contrastive trainer, which validates by matching every feature of cloud 0 to its nearest feature of cloud 1 and
checking the match against the known relative pose; this module restores that step and adds the registration metrics of
3DMatch: a RANSAC pose from the matches, refitted by least squares on its inliers.

Per batch (FeatureMatchEvaluator.step) everything stays on the device -- PF.feature_nn both ways, PF.match_stats,
PF.ransac_score, PF.rigid_sums (csrc/featmatch.hip, rules in include/pcmi.h) -- and compute_metrics() reads back once and
does the 3 x 3 SVDs on the host.  Every random quantity (the sampled query rows, the RANSAC triples) is data: MatchDraws.
"""
import numpy as np
import torch

from .. import functional as PF


def offsets_of(lengths):
  """[B] lengths -> int64 [B + 1] ascending offsets (host)."""
  out = np.zeros(len(lengths) + 1, dtype=np.int64)
  np.cumsum(np.asarray(lengths, dtype=np.int64), out=out[1:])
  return out


def _up(a, device):
  """A host array -> the device through pinned memory, without waiting for the stream; a device tensor as it is."""
  t = torch.as_tensor(a)
  if t.is_cuda:
    return t
  return t.contiguous().pin_memory().to(device, non_blocking=True)


class MatchDraws:
  """The random quantities of one step.  query_rows: int32 [Q] GLOBAL rows of cloud 0 with query_offsets int64 [B + 1] (None:
  every row is a query); triples: int32 [B, H, 3], indices into each pair's own queries (its matches)."""

  def __init__(self, query_rows, query_offsets, triples):
    self.query_rows, self.query_offsets, self.triples = query_rows, query_offsets, triples

  @staticmethod
  def sample(len_batch, num_queries, hypotheses, rng):
    """len_batch: [[n0, n1]] per pair; rng: a np.random.RandomState of the caller's (never the global generator, which the
    training loop's draws own).  A pair with more than num_queries rows in cloud 0 gets num_queries distinct rows, ascending;
    num_queries None, or no pair that large: every row is a query.  Three distinct indices per hypothesis, uniform."""
    n0 = [int(l[0]) for l in len_batch]
    offs0 = offsets_of(n0)
    rows = offs = None
    nq = list(n0)
    if num_queries is not None and any(n > num_queries for n in n0):
      parts = []
      for b, n in enumerate(n0):
        sel = np.sort(rng.choice(n, num_queries, replace=False)) if n > num_queries else np.arange(n)
        parts.append(sel.astype(np.int64) + offs0[b])
      nq = [len(p) for p in parts]
      rows, offs = np.concatenate(parts).astype(np.int32), offsets_of(nq)
    tri = np.zeros((len(n0), int(hypotheses), 3), dtype=np.int32)
    for b, m in enumerate(nq):
      if m < 3:
        continue  # (all zeros: every hypothesis repeats an index and is invalid)
      i0 = rng.randint(0, m, hypotheses)
      i1 = (i0 + 1 + rng.randint(0, m - 1, hypotheses)) % m
      lo, hi = np.minimum(i0, i1), np.maximum(i0, i1)
      i2 = rng.randint(0, m - 2, hypotheses)
      i2 = i2 + (i2 >= lo)
      i2 = i2 + (i2 >= hi)
      tri[b] = np.stack([i0, i1, i2], 1)
    return MatchDraws(rows, offs, tri)


def kabsch(sums):
  """The least-squares rigid transform of PF.rigid_sums' row [16] (float64, host): R = V diag(1, 1, det(V U^T)) U^T for S = U
  diag V^T, t = mean q - R mean p.  None if fewer than 3 inliers or a non-finite sum."""
  s = np.asarray(sums, dtype=np.float64)
  n = s[0]
  if not np.isfinite(s).all() or n < 3:
    return None
  pm, qm, S = s[1:4] / n, s[4:7] / n, s[7:16].reshape(3, 3)
  U, _, Vt = np.linalg.svd(S)
  d = np.sign(np.linalg.det(Vt.T @ U.T))
  R = Vt.T @ np.diag([1.0, 1.0, d if d != 0 else 1.0]) @ U.T
  return R, qm - R @ pm


def pose_errors(R, t, T_gt):
  """(translation error, rotation error in degrees) of (R, t) against the 4 x 4 T_gt."""
  T = np.asarray(T_gt, dtype=np.float64).reshape(4, 4)
  rte = float(np.linalg.norm(t - T[:3, 3]))
  c = (np.trace(R.T @ T[:3, :3]) - 1.0) / 2.0
  return rte, float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def metrics_from_records(counts, sums, T_gt, hit_thresholds, inlier_ratio_thresh, rte_thresh, rre_thresh_deg):
  """The metrics dict from the per-pair records on the host (shared with the numpy restatement of the tests): counts [P, 12]
  (PF.MATCH_* columns), sums [P, 16], T_gt [P, 4, 4]."""
  counts, sums = np.asarray(counts, dtype=np.int64), np.asarray(sums, dtype=np.float64)
  P = counts.shape[0]
  nq = np.maximum(counts[:, PF.MATCH_N_QUERY], 1).astype(np.float64)
  ngt = counts[:, PF.MATCH_N_GT]
  out, pairs = {"n_pairs": P}, {}
  for k, tau in enumerate(hit_thresholds):
    hr = counts[:, PF.MATCH_HITS + k] / nq
    with_gt = ngt > 0
    hro = counts[with_gt, PF.MATCH_HITS_GT + k] / ngt[with_gt].astype(np.float64)
    out["hit_ratio@%g" % tau] = float(hr.mean()) if P else 0.0
    out["hit_ratio_overlap@%g" % tau] = float(hro.mean()) if hro.size else 0.0
    out["feature_match_recall@%g" % tau] = float((hr >= inlier_ratio_thresh).mean()) if P else 0.0
    pairs["hit_ratio@%g" % tau] = hr
  mutual = counts[:, PF.MATCH_N_MUTUAL] / nq
  out["mutual_ratio"] = float(mutual.mean()) if P else 0.0
  rte, rre, ok = np.full(P, np.nan), np.full(P, np.nan), np.zeros(P, dtype=bool)
  poses = np.full((P, 12), np.nan)
  for p in range(P):
    fit = kabsch(sums[p])
    if fit is None:
      continue  # fewer than 3 valid matches, or no valid hypothesis: a registration failure
    poses[p, :9], poses[p, 9:] = fit[0].reshape(-1), fit[1]
    rte[p], rre[p] = pose_errors(fit[0], fit[1], T_gt[p])
    ok[p] = rte[p] < rte_thresh and rre[p] < rre_thresh_deg
  out["registration_recall"] = float(ok.mean()) if P else 0.0
  # means over the successful pairs, as 3DMatch reports them; 0 when there is none (registration_recall says so)
  out["rte"] = float(rte[ok].mean()) if ok.any() else 0.0
  out["rre_deg"] = float(rre[ok].mean()) if ok.any() else 0.0
  pairs.update(mutual_ratio=mutual, rte=rte, rre_deg=rre, registered=ok, pose=poses, n_inliers=sums[:, 0], counts=counts)
  out["pairs"] = pairs
  return out


class FeatureMatchEvaluator:
  """hit_thresholds (metres, at most 4), inlier_ratio_thresh, num_queries, rte / rre thresholds: FCGF's and 3DMatch's
  conventions -- parameters, not tuned values.  ransac_thresh None: 2 x voxel_size."""

  def __init__(self, voxel_size, hit_thresholds=(0.1,), inlier_ratio_thresh=0.05, num_queries=5000, mutual_only=False,
               ransac_hypotheses=4096, ransac_thresh=None, rte_thresh=0.3, rre_thresh_deg=15.0, device=None, seed=0):
    assert 1 <= len(hit_thresholds) <= PF.MATCH_MAX_TAU, "1 ... %d hit thresholds" % PF.MATCH_MAX_TAU
    assert 1 <= ransac_hypotheses <= 65536, "1 ... 65536 RANSAC hypotheses"
    self.voxel_size = float(voxel_size)
    self.hit_thresholds = tuple(float(t) for t in hit_thresholds)
    self.inlier_ratio_thresh, self.num_queries, self.mutual_only = float(inlier_ratio_thresh), num_queries, bool(mutual_only)
    self.ransac_hypotheses = int(ransac_hypotheses)
    self.ransac_thresh = 2.0 * self.voxel_size if ransac_thresh is None else float(ransac_thresh)
    self.rte_thresh, self.rre_thresh_deg = float(rte_thresh), float(rre_thresh_deg)
    self.device, self.seed = device, int(seed)
    self.reset()

  def reset(self):
    """Forgets every step, and starts the evaluator's own generator (the draws of steps that are given none) again from
    `seed`: two passes over the same pairs draw the same queries and triples."""
    self._rng = np.random.RandomState(self.seed)
    self._records = []  # one packed float64 device tensor [B, 12 + 16 + 16] per step
    self.last = None    # the device tensors of the last step (tests, inspection)

  def step(self, F0, F1, C0, C1, T_gt, len_batch, correspondences=None, draws=None):
    """F0 [N0, C], F1 [N1, C]: the features of the two clouds (device); C0, C1: their int32 [N, 4] coordinates, batch index
    first; T_gt [B, 4, 4] or the collate's [4 B, 4]; len_batch: [[n0, n1]] per pair (host); correspondences [P, 2] (optional:
    hit_ratio_overlap counts the queries that occur in column 0).  draws: MatchDraws (sampled from the evaluator's own
    generator otherwise).  Nothing is read back."""
    PF.require_cuda(F0, "FeatureMatchEvaluator.step")
    dev = F0.device
    B = len(len_batch)
    if draws is None:
      draws = MatchDraws.sample(len_batch, self.num_queries, self.ransac_hypotheses, self._rng)
    o0, o1 = offsets_of([l[0] for l in len_batch]), offsets_of([l[1] for l in len_batch])
    assert int(o0[-1]) == F0.shape[0] == C0.shape[0] and int(o1[-1]) == F1.shape[0] == C1.shape[0], \
        "len_batch does not add up to the rows of the clouds"
    offs0, offs1 = _up(o0, dev), _up(o1, dev)
    xyz0 = _up(C0, dev)[:, 1:4].to(torch.float64) * self.voxel_size
    xyz1 = _up(C1, dev)[:, 1:4].to(torch.float64) * self.voxel_size
    T = _up(T_gt, dev).to(torch.float64).reshape(B, 4, 4).contiguous()
    rows = qoffs = None
    if draws.query_rows is not None:
      rows, qoffs = _up(draws.query_rows, dev).to(torch.int32), _up(draws.query_offsets, dev).to(torch.int64)
    nn01, d2 = PF.feature_nn(F0, offs0, F1, offs1, query_rows=rows, query_offsets=qoffs)
    moffs = offs0 if rows is None else qoffs  # the pairs' segments of the matches
    # the reverse search of the MATCHED rows (-1 where there is no match: such a query row matches nothing, by the rule)
    nn10, _ = PF.feature_nn(F1, offs1, F0, offs0, query_rows=nn01, query_offsets=moffs)
    has_gt = None
    if correspondences is not None:
      corr = _up(correspondences, dev)
      has_gt = torch.zeros(F0.shape[0], dtype=torch.uint8, device=dev)
      has_gt.index_fill_(0, corr[:, 0].long(), 1)
    counts, residual2 = PF.match_stats(xyz0, xyz1, T, moffs, nn01, self.hit_thresholds, query_rows=rows, nn10=nn10, has_gt=has_gt)
    # the matched points; a query without a match (or, with mutual_only, without a mutual one) becomes NaN, which is no
    # inlier of any hypothesis and makes a hypothesis that draws it invalid
    qrow = torch.arange(F0.shape[0], device=dev) if rows is None else rows.long()
    keep = nn01 >= 0
    if self.mutual_only:
      keep = keep & (nn10.long() == qrow)
    src = xyz0[qrow]
    dst = torch.where(keep[:, None], xyz1[nn01.clamp(min=0).long()], torch.full_like(src, float("nan")))
    triples = _up(draws.triples, dev).to(torch.int32)
    hcounts, best, Rt = PF.ransac_score(src, dst, moffs, triples, self.ransac_thresh)
    sums = PF.rigid_sums(src, dst, moffs, best, Rt, self.ransac_thresh)
    self._records.append(torch.cat([counts.to(torch.float64), sums, T.reshape(B, 16)], 1))
    self.last = dict(nn01=nn01, d2=d2, nn10=nn10, counts=counts, residual2=residual2, src=src, dst=dst, hyp_counts=hcounts,
                     best=best, Rt=Rt, sums=sums, draws=draws)

  def compute_metrics(self):
    """One read-back, the SVDs, the dict: hit_ratio@t (mean over pairs of hits / queries), hit_ratio_overlap@t (over the queries
    that have a ground-truth correspondence), feature_match_recall@t (share of pairs with hit_ratio >= inlier_ratio_thresh),
    mutual_ratio, registration_recall, rte and rre_deg (means over the registered pairs), n_pairs, and `pairs`: the per-pair
    arrays."""
    if not self._records:
      rec = np.zeros((0, 44))
    else:
      rec = torch.cat(self._records).cpu().numpy()
    counts = np.rint(rec[:, :12]).astype(np.int64)  # (exact: the counts are far below 2^53)
    return metrics_from_records(counts, rec[:, 12:28], rec[:, 28:44].reshape(-1, 4, 4), self.hit_thresholds,
                                self.inlier_ratio_thresh, self.rte_thresh, self.rre_thresh_deg)
