"""Host restatement of the VoteNet detection head (csrc/detect.hip, pointcontrast_amd.downstream.votenet) in float64
numpy / torch-CPU, written from the semantics in include/pcmi.h: the oracle of tests/test_gpu_votenet_head.py, itself pinned
to the reference's functions by tests/test_votenet_ref.py.

Index outputs follow the device's float32 rule (every operation rounded on its own, in the order of include/pcmi.h, the
lowest index of a tie); values are float64.  The functions that decide something by a threshold also report how close the
closest decision was, so that a test can assert its inputs leave float32 no room to decide differently."""
import math

import numpy as np
import torch

FAR_THRESHOLD, NEAR_THRESHOLD, GT_VOTE_FACTOR = 0.6, 0.3, 3
OBJECTNESS_CLS_WEIGHTS = (0.2, 0.8)
MODES = ("l2", "l1", "huber")


# ---- nn_distance -------------------------------------------------------------------------------------------------------------
def _comp32(x, mode, delta):
  """One component of a distance in float32, each numpy operation rounding on its own."""
  if mode == "l2":
    return x * x
  ax = np.abs(x)
  if mode == "l1":
    return ax
  d = np.float32(delta)
  q = np.minimum(ax, d)
  return np.float32(0.5) * (q * q) + d * (ax - q)


def nn_indices(pc1, pc2, mode="l2", delta=1.0, chunk=1 << 22):
  """(idx1 [B, N], idx2 [B, M]) int64 by the float32 rule: ((cx) + (cy)) + (cz), argmin with the lowest index of a tie."""
  a, b = np.asarray(pc1, np.float32), np.asarray(pc2, np.float32)
  B, N, _ = a.shape
  M = b.shape[1]
  idx1, idx2 = np.empty((B, N), np.int64), np.empty((B, M), np.int64)
  step = max(1, chunk // max(N * M, 1))
  for s in range(0, B, step):
    aa, bb = a[s:s + step, :, None, :], b[s:s + step, None, :, :]
    d = (_comp32(aa[..., 0] - bb[..., 0], mode, delta) + _comp32(aa[..., 1] - bb[..., 1], mode, delta)) + \
        _comp32(aa[..., 2] - bb[..., 2], mode, delta)
    assert d.dtype == np.float32
    idx1[s:s + step] = np.argmin(d, axis=2)
    idx2[s:s + step] = np.argmin(d, axis=1)
  return idx1, idx2


def huber(error, delta=1.0):
  a = error.abs()
  q = torch.clamp(a, max=delta)
  return 0.5 * q * q + delta * (a - q)


def pair_distance(p, q, mode="l2", delta=1.0):
  """Distance of matching points p, q [..., 3] (torch, any float dtype), summed over the last axis; differentiable."""
  diff = p - q
  if mode == "l2":
    return (diff * diff).sum(-1)
  if mode == "l1":
    return diff.abs().sum(-1)
  return huber(diff, delta).sum(-1)


def nn_distance_at(pc1, pc2, idx1, idx2, mode="l2", delta=1.0):
  """(dist1 [B, N], dist2 [B, M]) in the dtype of pc1 / pc2 (torch) for GIVEN argmins: what torch.min of the [B, N, M]
  tensor returns and differentiates, without forming it."""
  i1 = torch.as_tensor(idx1, dtype=torch.int64)
  i2 = torch.as_tensor(idx2, dtype=torch.int64)
  near2 = torch.gather(pc2, 1, i1.unsqueeze(-1).expand(-1, -1, 3))
  near1 = torch.gather(pc1, 1, i2.unsqueeze(-1).expand(-1, -1, 3))
  return pair_distance(pc1, near2, mode, delta), pair_distance(near1, pc2, mode, delta)


def nn_distance(pc1, pc2, l1smooth=False, delta=1.0, l1=False):
  """The reference's signature on float64 torch tensors -> (dist1, idx1, dist2, idx2); indices by the float32 rule."""
  mode = "huber" if l1smooth else ("l1" if l1 else "l2")
  p1, p2 = pc1.double(), pc2.double()
  idx1, idx2 = nn_indices(pc1.detach().numpy(), pc2.detach().numpy(), mode, delta)
  d1, d2 = nn_distance_at(p1, p2, idx1, idx2, mode, delta)
  return d1, torch.from_numpy(idx1), d2, torch.from_numpy(idx2)


def _dcomp32(x, mode, delta):
  """The derivative of _comp32 in float32: 2 x / sign(x) / clamp(x, -delta, delta)."""
  if mode == "l2":
    return np.float32(2) * x
  if mode == "l1":
    return np.sign(x).astype(np.float32)
  d = np.float32(delta)
  return np.minimum(np.maximum(x, -d), d)


def nn_backward_f32(pc1, pc2, idx1, idx2, g1, g2, mode="l2", delta=1.0):
  """(gpc1 [B, N, 3], gpc2 [B, M, 3]) in float32 in the ORDER include/pcmi.h promises for pcmi_nn_distance_bwd: a point's own
  term first, then the term of every point of the other cloud whose nearest neighbour it is, in ascending index of the other
  cloud, every operation rounded on its own (g * d'(a - o), then the add).  An index outside its cloud drops its term.  What a
  kernel that sums in another order misses by a few last bits, and a float64 comparison at 1e-4 cannot see."""
  p1, p2 = np.asarray(pc1, np.float32), np.asarray(pc2, np.float32)

  def one_cloud(a, o, idx_a, idx_o, g_a, g_o):
    B, N, _ = a.shape
    M = o.shape[1]
    af, of = a.reshape(B * N, 3), o.reshape(B * M, 3)
    ia, io = np.asarray(idx_a, np.int64).reshape(B * N), np.asarray(idx_o, np.int64).reshape(B * M)
    ga_, go_ = np.asarray(g_a, np.float32).reshape(B * N), np.asarray(g_o, np.float32).reshape(B * M)
    out = np.zeros((B * N, 3), np.float32)
    rows = np.nonzero((ia >= 0) & (ia < M))[0]
    out[rows] = out[rows] + ga_[rows, None] * _dcomp32(af[rows] - of[(rows // N) * M + ia[rows]], mode, delta)
    src = np.nonzero((io >= 0) & (io < N))[0]  # flat positions b M + j, ascending
    tgt = (src // M) * N + io[src]
    order = np.argsort(tgt, kind="stable")     # grouped by target, ascending j within a target
    src, tgt = src[order], tgt[order]
    first = np.searchsorted(tgt, tgt, side="left")
    rank = np.arange(len(tgt)) - first
    for k in range(int(rank.max()) + 1 if len(rank) else 0):  # the k-th source of every target: one add each
      s, t = src[rank == k], tgt[rank == k]
      out[t] = out[t] + go_[s, None] * _dcomp32(af[t] - of[s], mode, delta)
    assert out.dtype == np.float32
    return out.reshape(B, N, 3)

  return one_cloud(p1, p2, idx1, idx2, g1, g2), one_cloud(p2, p1, idx2, idx1, g2, g1)


# ---- get_loss -----------------------------------------------------------------------------------------------------------------
def _masked_mean(v, w):
  return (v * w).sum() / (w.sum() + 1e-6)


def _ce(scores, labels, weight=None):
  logp = torch.log_softmax(scores, dim=-1)
  picked = -torch.gather(logp, -1, labels.unsqueeze(-1)).squeeze(-1)
  return picked if weight is None else picked * weight[labels]


def get_loss(ep, num_heading_bin, mean_size_arr):
  """The VoteNet loss on float64 CPU tensors (dict ep with the reference's keys; float tensors float64) -> dict of the nine
  loss terms, `loss`, the labels, ratios, obj_acc and `euclidean_dist1` (the quantity the two thresholds cut)."""
  out = {}
  seed_xyz = ep["seed_xyz"]
  B, num_seed = seed_xyz.shape[:2]
  inds = ep["seed_inds"].long()
  vmask = torch.gather(ep["vote_label_mask"], 1, inds).double()
  gt_votes = torch.gather(ep["vote_label"], 1, inds.unsqueeze(-1).expand(-1, -1, 3 * GT_VOTE_FACTOR)) + seed_xyz.repeat(1, 1, GT_VOTE_FACTOR)
  votes = ep["vote_xyz"].reshape(B * num_seed, -1, 3)
  _, _, d2, _ = nn_distance(votes, gt_votes.reshape(B * num_seed, GT_VOTE_FACTOR, 3), l1=True)
  out["vote_loss"] = _masked_mean(d2.min(dim=1)[0].view(B, num_seed), vmask)

  gt_center = ep["center_label"][:, :, 0:3]
  d1, ind1, _, _ = nn_distance(ep["aggregated_vote_xyz"], gt_center)
  eu = torch.sqrt(d1.detach() + 1e-6)
  label = (eu < NEAR_THRESHOLD).long()
  mask = ((eu < NEAR_THRESHOLD) | (eu > FAR_THRESHOLD)).double()
  w = torch.tensor(OBJECTNESS_CLS_WEIGHTS, dtype=torch.float64)
  out["objectness_loss"] = _masked_mean(_ce(ep["objectness_scores"], label, w), mask)
  out.update(objectness_label=label, objectness_mask=mask, object_assignment=ind1, euclidean_dist1=eu)
  total = float(label.numel())
  out["pos_ratio"] = label.double().sum() / total
  out["neg_ratio"] = mask.sum() / total - out["pos_ratio"]

  d1, _, d2, _ = nn_distance(ep["center"], gt_center)
  obj = label.double()
  out["center_loss"] = _masked_mean(d1, obj) + _masked_mean(d2, ep["box_label_mask"].double())
  pick = lambda key: torch.gather(ep[key], 1, ind1)  # noqa: E731
  hcl = pick("heading_class_label")
  out["heading_cls_loss"] = _masked_mean(_ce(ep["heading_scores"], hcl), obj)
  hres = pick("heading_residual_label") / (math.pi / num_heading_bin)
  onehot = torch.zeros(ep["heading_scores"].shape, dtype=torch.float64).scatter_(2, hcl.unsqueeze(-1), 1.0)
  out["heading_reg_loss"] = _masked_mean(huber((ep["heading_residuals_normalized"] * onehot).sum(-1) - hres), obj)
  scl = pick("size_class_label")
  out["size_cls_loss"] = _masked_mean(_ce(ep["size_scores"], scl), obj)
  sres = torch.gather(ep["size_residual_label"], 1, ind1.unsqueeze(-1).expand(-1, -1, 3))
  onehot = torch.zeros(ep["size_scores"].shape, dtype=torch.float64).scatter_(2, scl.unsqueeze(-1), 1.0).unsqueeze(-1)
  pred = (ep["size_residuals_normalized"] * onehot).sum(2)
  mean_size = (onehot * torch.as_tensor(np.asarray(mean_size_arr, np.float32)).double()[None, None]).sum(2)
  out["size_reg_loss"] = _masked_mean(huber(pred - sres / mean_size).mean(-1), obj)
  out["sem_cls_loss"] = _masked_mean(_ce(ep["sem_cls_scores"], pick("sem_cls_label")), obj)
  out["box_loss"] = out["center_loss"] + 0.1 * out["heading_cls_loss"] + out["heading_reg_loss"] + 0.1 * out["size_cls_loss"] + \
      out["size_reg_loss"]
  out["loss"] = (out["vote_loss"] + 0.5 * out["objectness_loss"] + out["box_loss"] + 0.1 * out["sem_cls_loss"]) * 10
  pred_obj = torch.argmax(ep["objectness_scores"], 2)
  out["obj_acc"] = _masked_mean((pred_obj == label).double(), mask)
  return out


# ---- decode -------------------------------------------------------------------------------------------------------------------
def _softmax(x):
  e = np.exp(x - x.max(axis=-1, keepdims=True))
  return e / e.sum(axis=-1, keepdims=True)


def corners_of(size, angle, center):
  """[..., 8, 3] corners of boxes of size [..., 3] = (l, w, h), heading angle [...] about the y axis and centre [..., 3]."""
  sx = np.array([1, 1, -1, -1, 1, 1, -1, -1], np.float64)
  sy = np.array([1, 1, 1, 1, -1, -1, -1, -1], np.float64)
  sz = np.array([1, -1, -1, 1, 1, -1, -1, 1], np.float64)
  x = size[..., 0:1] / 2 * sx
  y = size[..., 2:3] / 2 * sy
  z = size[..., 1:2] / 2 * sz
  c, s = np.cos(angle)[..., None], np.sin(angle)[..., None]
  return np.stack([c * x + s * z + center[..., 0:1], y + center[..., 1:2], -s * x + c * z + center[..., 2:3]], axis=-1)


def box_decode(center, heading_scores, heading_residuals, size_scores, size_residuals, sem_cls_scores, objectness_scores,
               mean_size_arr, zero_heading):
  """float64 decode of float32 inputs -> dict(heading_class, size_class, sem_cls, box_params [B, K, 7], corners, minmax,
  obj_prob, sem_cls_probs).  argmax: the first maximum (np.argmax), as torch.argmax."""
  f = lambda a: np.asarray(a, np.float32).astype(np.float64)  # noqa: E731
  center, hr, sr, msa = f(center), f(heading_residuals), f(size_residuals), f(mean_size_arr)
  hc = np.argmax(np.asarray(heading_scores, np.float32), -1)
  sc = np.argmax(np.asarray(size_scores, np.float32), -1)
  cc = np.argmax(np.asarray(sem_cls_scores, np.float32), -1)
  H = hr.shape[-1]
  if zero_heading:
    angle = np.zeros(hc.shape)
  else:
    angle = hc * (2 * np.pi / H) + np.take_along_axis(hr, hc[..., None], -1)[..., 0]
    angle = np.where(angle > np.pi, angle - 2 * np.pi, angle)
  size = msa[sc] + np.take_along_axis(sr, sc[..., None, None].repeat(3, -1), 2)[:, :, 0, :]
  cam = np.stack([center[..., 0], -center[..., 2], center[..., 1]], -1)
  corners = corners_of(size, angle, cam)
  minmax = np.concatenate([corners.min(axis=2), corners.max(axis=2)], -1)
  return dict(heading_class=hc, size_class=sc, sem_cls=cc, box_params=np.concatenate([cam, size, angle[..., None]], -1),
              corners=corners, minmax=minmax, obj_prob=_softmax(f(objectness_scores))[..., 1], sem_cls_probs=_softmax(f(sem_cls_scores)))


# ---- points in boxes ----------------------------------------------------------------------------------------------------------
def box_point_counts(points, box_params):
  """points [N, >= 3] (upright-depth), box_params [K, 7] (camera centre, (l, w, h), angle) -> (counts [K] int64, the smallest
  distance of any point to any face plane of each box [K]: how far the closest in/out decision is from flipping)."""
  p = np.asarray(points, np.float64)[:, :3]
  cam = np.stack([p[:, 0], -p[:, 2], p[:, 1]], -1)
  bp = np.asarray(box_params, np.float64)
  counts, face = np.zeros(bp.shape[0], np.int64), np.full(bp.shape[0], np.inf)
  for k0 in range(0, bp.shape[0], 32):
    q = bp[k0:k0 + 32]
    d = cam[None] - q[:, None, 0:3]                     # [k, N, 3]
    c, s = np.cos(q[:, 6])[:, None], np.sin(q[:, 6])[:, None]
    local = np.stack([c * d[..., 0] - s * d[..., 2], d[..., 1], s * d[..., 0] + c * d[..., 2]], -1)
    half = np.abs(q[:, [3, 5, 4]])[:, None, :] / 2      # box x = l, y = h, z = w
    margin = half - np.abs(local)                       # >= 0 on every axis: inside
    counts[k0:k0 + 32] = (margin >= 0).all(-1).sum(1)
    if p.shape[0]:
      face[k0:k0 + 32] = np.abs(margin).min(axis=(1, 2))
  return counts, face


def points_near_faces(points, box_params, tol):
  """bool [N]: points closer than tol to a face plane of any box."""
  p = np.asarray(points, np.float64)[:, :3]
  cam = np.stack([p[:, 0], -p[:, 2], p[:, 1]], -1)
  bp = np.asarray(box_params, np.float64)
  near = np.zeros(p.shape[0], bool)
  for k0 in range(0, bp.shape[0], 32):
    q = bp[k0:k0 + 32]
    d = cam[None] - q[:, None, 0:3]
    c, s = np.cos(q[:, 6])[:, None], np.sin(q[:, 6])[:, None]
    local = np.stack([c * d[..., 0] - s * d[..., 2], d[..., 1], s * d[..., 0] + c * d[..., 2]], -1)
    near |= (np.abs(np.abs(q[:, [3, 5, 4]])[:, None, :] / 2 - np.abs(local)) < tol).any(axis=(0, 2))
  return near


# ---- NMS ----------------------------------------------------------------------------------------------------------------------
def nms(minmax, score, sem_cls, nonempty, mode, old_type, thr):
  """Greedy NMS of one scene.  minmax [K, 6], score [K], sem_cls [K], nonempty [K] bool; mode 0: 2D on x / z, 1: 3D, 2: 3D
  within a class.  Returns (pred_mask [K] int64, the smallest |o - thr| over the overlaps that were compared).  Boxes are
  visited by descending score, equal scores by ascending index."""
  mm = np.asarray(minmax, np.float64)
  K = mm.shape[0]
  axes = (0, 2) if mode == 0 else (0, 1, 2)
  lo, hi = mm[:, list(axes)], mm[:, [a + 3 for a in axes]]
  area = np.prod(hi - lo, axis=1)
  order = [i for i in sorted(range(K), key=lambda i: (-float(score[i]), i)) if nonempty[i]]
  mask = np.zeros(K, np.int64)
  closest = np.inf
  alive = np.asarray(order, np.int64)
  cls = np.asarray(sem_cls)
  while alive.size:
    i, rest = alive[0], alive[1:]
    mask[i] = 1
    inter = np.prod(np.maximum(0.0, np.minimum(hi[i], hi[rest]) - np.maximum(lo[i], lo[rest])), axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
      o = inter / area[rest] if old_type else inter / (area[i] + area[rest] - inter)
    compared = np.ones(rest.shape, bool) if mode != 2 else cls[rest] == cls[i]
    seen = compared & ~np.isnan(o)
    if seen.any():
      closest = min(closest, float(np.abs(o[seen] - thr).min()))
    alive = rest[~(compared & (o > thr))]
  return mask, closest


# ---- parse_predictions ----------------------------------------------------------------------------------------------------------
def parse_predictions(arrays, mean_size_arr, num_class, zero_heading, remove_empty_box, mode, old_type, nms_iou, conf_thresh,
                      per_class_proposal):
  """arrays: dict of numpy float32 inputs (center, heading_scores, heading_residuals, size_scores, size_residuals,
  sem_cls_scores, objectness_scores, point_clouds).  Returns (batch_pred_map_cls with the kept index added as a 4th entry,
  pred_mask [B, K], dict(min_face, min_iou_gap))."""
  dec = box_decode(arrays["center"], arrays["heading_scores"], arrays["heading_residuals"], arrays["size_scores"],
                   arrays["size_residuals"], arrays["sem_cls_scores"], arrays["objectness_scores"], mean_size_arr, zero_heading)
  B, K = dec["obj_prob"].shape
  pred_mask = np.zeros((B, K), np.int64)
  stats = dict(min_face=np.inf, min_iou_gap=np.inf)
  out = []
  for i in range(B):
    nonempty = np.ones(K, bool)
    if remove_empty_box:
      cnt, face = box_point_counts(arrays["point_clouds"][i], dec["box_params"][i])
      nonempty = cnt >= 5
      stats["min_face"] = min(stats["min_face"], float(face.min()))
    pred_mask[i], gap = nms(dec["minmax"][i], dec["obj_prob"][i], dec["sem_cls"][i], nonempty, mode, old_type, nms_iou)
    stats["min_iou_gap"] = min(stats["min_iou_gap"], gap)
    kept = [j for j in range(K) if pred_mask[i, j] == 1 and dec["obj_prob"][i, j] > conf_thresh]
    if per_class_proposal:
      out.append([(c, dec["corners"][i, j], dec["sem_cls_probs"][i, j, c] * dec["obj_prob"][i, j], j) for c in range(num_class) for j in kept])
    else:
      out.append([(int(dec["sem_cls"][i, j]), dec["corners"][i, j], dec["obj_prob"][i, j], j) for j in kept])
  return out, pred_mask, stats
