"""numpy restatement of the detection input entry points (pcmi_det_* of csrc/detect_input.hip) under exactly the rules that
include/pcmi.h writes down: the same operation order, the same precision of every product and sum, the same flags.  The
GPU tests compare the kernels with this bit for bit; tests/test_detect_input_ref.py holds it to what the reference's own
dataset classes returned (tests/golden/golden_detinput.npz)."""
import numpy as np

FLAG_RANGE, FLAG_SPAN, FLAG_CHOICE, FLAG_INSTANCE, FLAG_LABEL, FLAG_BOXES = 1, 2, 4, 8, 16, 32
MAX_INSTANCES = 1024
MAX_NUM_OBJ = 64
SCANNET, SUNRGBD = 0, 1
VOXEL_LIMIT = 1 << 20
SPAN = 1 << 18


def rotz(t):
  """pc_util.rotz / sunrgbd_utils.rotz of the reference: numpy's cos and sin of the angle."""
  c, s = np.cos(t), np.sin(t)
  return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float64)


def _rot_rows(x, y, z, R):
  """((x R[i][0] + y R[i][1]) + z R[i][2]) for i = 0, 1, 2 on float64 arrays: every product and sum rounded on its own."""
  return [(x * R[i, 0] + y * R[i, 1]) + z * R[i, 2] for i in range(3)]


def sample_transform(xyz, offsets, choices, augment=True, flip=None, rot=None, scale=None, instance=None, semantic=None, votes=None):
  """pcmi_det_sample_transform (votes None) and pcmi_det_votes_transform (votes [n, 10] float64).  Returns a dict:
  point_clouds [B, P, 3] float32, flags int32 [B], out_instance / out_semantic [B, P] int32 for the payloads given, and with
  votes vote_label [B, P, 9] float32 and vote_label_mask [B, P] int64."""
  xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
  offsets = np.asarray(offsets, dtype=np.int64)
  choices = np.asarray(choices, dtype=np.int32)
  B, P = choices.shape
  n = len(xyz)
  pc = np.zeros((B, P, 3), np.float32)
  flags = np.zeros(B, np.int32)
  out = dict(point_clouds=pc, flags=flags)
  oi = None if instance is None else np.full((B, P), -1, np.int32)
  os_ = None if semantic is None else np.full((B, P), -1, np.int32)
  vl = None if votes is None else np.zeros((B, P, 9), np.float32)
  vm = None if votes is None else np.zeros((B, P), np.int64)
  for b in range(B):
    lo, hi = int(offsets[b]), int(offsets[b + 1])
    c = choices[b].astype(np.int64)
    ok = (c >= 0) & (c < hi - lo) if (0 <= lo <= hi <= n) else np.zeros(P, bool)
    if not ok.all():
      flags[b] |= FLAG_CHOICE
    g = np.where(ok, lo + c, 0)
    p = xyz[g] if n else np.zeros((P, 3), np.float32)
    fin = np.isfinite(p).all(1)
    if (ok & ~fin).any():
      flags[b] |= FLAG_RANGE
    ok = ok & fin
    p = np.where(ok[:, None], p, np.float32(0)).astype(np.float32)
    v = None
    if votes is not None:
      src = np.asarray(votes, dtype=np.float64)[g] if n else np.zeros((P, 10))
      src = np.where(ok[:, None], src, 0.0)
      m0 = src[:, 0]
      vm[b] = np.where(np.abs(m0) < 9.0e18, np.where(np.isfinite(m0), m0, 0.0), 0.0).astype(np.int64)
      v = src[:, 1:].copy()
    if augment:
      fx, fy = bool(flip[b][0]), bool(flip[b][1])
      R = np.asarray(rot[b], dtype=np.float64).reshape(3, 3)
      sc = np.float64(scale[b])
      if fx:
        p[:, 0] = -p[:, 0]
      if fy:
        p[:, 1] = -p[:, 1]
      x, y, z = (p[:, a].astype(np.float64) for a in range(3))
      r32 = np.stack(_rot_rows(x, y, z, R), 1).astype(np.float32)
      if v is not None:
        for k in range(3):
          if fx:
            v[:, 3 * k] = -v[:, 3 * k]
          if fy:
            v[:, 3 * k + 1] = -v[:, 3 * k + 1]
          ex, ey, ez = x + v[:, 3 * k], y + v[:, 3 * k + 1], z + v[:, 3 * k + 2]
          end = _rot_rows(ex, ey, ez, R)
          for i in range(3):
            v[:, 3 * k + i] = (end[i] - r32[:, i].astype(np.float64)) * sc
      o = (r32.astype(np.float64) * sc).astype(np.float32)
    else:
      o = p
    pc[b] = np.where(ok[:, None], o, np.float32(0))
    if oi is not None:
      oi[b] = np.where(ok, np.asarray(instance, dtype=np.int32)[g] if n else -1, -1)
    if os_ is not None:
      os_[b] = np.where(ok, np.asarray(semantic, dtype=np.int32)[g] if n else -1, -1)
    if vl is not None:
      vl[b] = np.where(ok[:, None], v, 0.0).astype(np.float32)
  if oi is not None:
    out["out_instance"] = oi
  if os_ is not None:
    out["out_semantic"] = os_
  if vl is not None:
    out["vote_label"], out["vote_label_mask"] = vl, vm
  return out


def _ord32(f):
  """The order-preserving integer image of float32 values: a < b <=> image(a) < image(b); -0.0 sorts below +0.0."""
  u = np.asarray(f, dtype=np.float32).view(np.uint32)
  return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _unord32(u):
  u = np.asarray(u, dtype=np.uint32)
  return np.where(u >> 31 != 0, u & np.uint32(0x7fffffff), ~u).astype(np.uint32).view(np.float32)


def votes_from_instances(point_clouds, instance, semantic, valid_sem):
  """pcmi_det_votes_from_instances.  Returns (vote_label [B, P, 9] float32, vote_label_mask [B, P] int64, flags [B])."""
  pc = np.asarray(point_clouds, dtype=np.float32)
  B, P = pc.shape[:2]
  inst = np.asarray(instance, dtype=np.int32).reshape(B, P)
  sem = np.asarray(semantic, dtype=np.int32).reshape(B, P)
  valid = set(int(v) for v in np.asarray(valid_sem).reshape(-1))
  vote = np.zeros((B, P, 3), np.float32)
  mask = np.zeros((B, P), np.int64)
  flags = np.zeros(B, np.int32)
  for b in range(B):
    dropped = inst[b] == -1
    bad_id = ~dropped & ((inst[b] < 0) | (inst[b] >= MAX_INSTANCES))
    if bad_id.any():
      flags[b] |= FLAG_INSTANCE
    nonfin = ~dropped & ~bad_id & ~np.isfinite(pc[b]).all(1)
    if nonfin.any():
      flags[b] |= FLAG_RANGE
    live = ~dropped & ~bad_id & ~nonfin
    for i in np.unique(inst[b][live]):
      ind = np.where(live & (inst[b] == i))[0]
      if int(sem[b, ind[0]]) not in valid:
        continue
      x = pc[b, ind]
      img = _ord32(x)
      mn, mx = _unord32(img.min(0)), _unord32(img.max(0))
      center = (np.float32(0.5) * (mn + mx).astype(np.float32)).astype(np.float32)
      vote[b, ind] = center - x
      mask[b, ind] = 1
  return np.tile(vote, (1, 1, 3)), mask, flags


def py_mod(a, m):
  """Python's float a % m for m > 0: fmod moved into [0, m); a zero result is +0."""
  r = np.fmod(np.float64(a), np.float64(m))
  if r != 0.0:
    if r < 0.0:
      r = r + np.float64(m)
  else:
    r = np.float64(0.0)
  return r


def final_heading(boxes, n_boxes, augment, flip, rot_angle):
  """The heading of every slot after the augmentation [B, 64] (float64) -- what the caller takes cos and sin of."""
  h = np.array(np.asarray(boxes, dtype=np.float64)[:, :, 6])
  B = h.shape[0]
  for b in range(B):
    k = int(n_boxes[b])
    k = k if 0 <= k <= MAX_NUM_OBJ else 0
    h[b, k:] = 0.0
    if augment:
      if flip[b][0]:
        h[b, :k] = np.pi - h[b, :k]
      h[b, :k] = h[b, :k] - np.float64(rot_angle[b])
  return np.where(np.isfinite(h), h, 0.0)


def heading_cs(boxes, n_boxes, augment, flip, rot_angle):
  """heading_cs [B, 64, 2] of pcmi_det_box_labels: numpy's cos and sin of -1 * the final heading."""
  h = final_heading(boxes, n_boxes, augment, flip, rot_angle)
  return np.stack([np.cos(-1 * h), np.sin(-1 * h)], -1)


def box_labels(boxes, n_boxes, mode, augment=True, flip=None, rot=None, rot_angle=None, scale=None, label_to_class=None,
               mean_size=None, num_heading_bin=12, cs=None):
  """pcmi_det_box_labels.  boxes [B, 64, 8] float64.  Returns a dict under the reference's keys plus flags."""
  boxes = np.asarray(boxes, dtype=np.float64)
  B = boxes.shape[0]
  mean_size = np.asarray(mean_size, dtype=np.float64).reshape(-1, 3)
  n_class = len(mean_size)
  K = MAX_NUM_OBJ
  out = dict(center_label=np.zeros((B, K, 3), np.float32), heading_class_label=np.zeros((B, K), np.int64),
             heading_residual_label=np.zeros((B, K), np.float32), size_class_label=np.zeros((B, K), np.int64),
             size_residual_label=np.zeros((B, K, 3), np.float32), sem_cls_label=np.zeros((B, K), np.int64),
             box_label_mask=np.zeros((B, K), np.float32), flags=np.zeros(B, np.int32))
  if mode == SUNRGBD and cs is None:
    cs = heading_cs(boxes, n_boxes, augment, flip, rot_angle)
  two_pi = np.float64(2.0) * np.float64(np.pi)
  for b in range(B):
    k = int(n_boxes[b])
    if k < 0 or k > K:
      k = 0
      out["flags"][b] |= FLAG_BOXES
    R = np.asarray(rot[b], dtype=np.float64).reshape(3, 3) if augment else np.eye(3)
    fx = bool(augment and flip[b][0])
    fy = bool(augment and flip[b][1])
    for i in range(K):
      live = i < k
      c, l, h, lab = np.zeros(3), np.zeros(3), np.float64(0), np.float64(0)
      fin = True  # a live box that is not finite counts as a slot of zeros: class 0, no residual
      if live:
        s = boxes[b, i]
        if np.isfinite(s).all():
          c, l, h, lab = s[0:3].copy(), s[3:6].copy(), np.float64(s[6]), np.float64(s[7])
        else:
          out["flags"][b] |= FLAG_RANGE
          fin = False
      center, res, hcls, hres, cls = np.zeros(3), np.zeros(3), 0, np.float64(0), 0
      if mode == SCANNET:
        if fx:
          c[0] = -1.0 * c[0]
        if fy:
          c[1] = -1.0 * c[1]
        if augment:
          nc = [(c[0] * R[r, 0] + c[1] * R[r, 1]) + c[2] * R[r, 2] for r in range(3)]
          dx, dy = l[0] / 2.0, l[1] / 2.0
          xs, ys = [], []
          for sx, sy in ((-1.0, -1.0), (1.0, -1.0), (1.0, 1.0), (-1.0, 1.0)):
            u, v = sx * dx, sy * dy
            xs.append((u * R[0, 0] + v * R[0, 1]) + 0.0 * R[0, 2])
            ys.append((u * R[1, 0] + v * R[1, 1]) + 0.0 * R[1, 2])
          c = np.array(nc)
          l = np.array([2.0 * max(xs), 2.0 * max(ys), l[2]])
        center = c
        if live and fin:
          idx = int(lab) if abs(lab) < 2.0e9 else -1
          cls = int(label_to_class[idx]) if (0 <= idx < len(label_to_class) and float(idx) == lab) else -1
          if cls < 0 or cls >= n_class:
            out["flags"][b] |= FLAG_LABEL
            cls = 0
          else:
            res = l - mean_size[cls]
      elif live and fin:
        if augment:
          sc = np.float64(scale[b])
          if fx:
            c[0] = -1.0 * c[0]
            h = np.float64(np.pi) - h
          nc = [(c[0] * R[r, 0] + c[1] * R[r, 1]) + c[2] * R[r, 2] for r in range(3)]
          h = h - np.float64(rot_angle[b])
          c = np.array(nc) * sc
          l = l * sc
        ang = py_mod(h, two_pi)
        per = two_pi / np.float64(num_heading_bin)
        shifted = py_mod(ang + per / 2.0, two_pi)
        hcls = int(shifted / per)
        hres = shifted - (np.float64(hcls) * per + per / 2.0)
        idx = int(lab) if abs(lab) < 2.0e9 else -1
        cls = idx
        if idx < 0 or idx >= n_class:
          out["flags"][b] |= FLAG_LABEL
          cls, hcls, hres = 0, 0, np.float64(0)
        else:
          res = l * 2.0 - mean_size[cls]
          co, si = np.float64(cs[b, i, 0]), np.float64(cs[b, i, 1])
          xo = np.array([-l[0], l[0], l[0], -l[0], -l[0], l[0], l[0], -l[0]])
          yo = np.array([l[1], l[1], -l[1], -l[1], l[1], l[1], -l[1], -l[1]])
          zo = np.array([l[2], l[2], l[2], l[2], -l[2], -l[2], -l[2], -l[2]])
          X = ((co * xo + (-si) * yo) + 0.0 * zo) + c[0]
          Y = ((si * xo + co * yo) + 0.0 * zo) + c[1]
          Z = ((0.0 * xo + 0.0 * yo) + 1.0 * zo) + c[2]
          center = np.array([(X.min() + X.max()) / 2.0, (Y.min() + Y.max()) / 2.0, (Z.min() + Z.max()) / 2.0])
      out["center_label"][b, i] = center.astype(np.float32)
      out["size_residual_label"][b, i] = np.asarray(res).astype(np.float32)
      out["heading_class_label"][b, i] = hcls
      out["heading_residual_label"][b, i] = np.float32(hres)
      out["size_class_label"][b, i] = cls if live else 0
      out["sem_cls_label"][b, i] = cls if live else 0
      out["box_label_mask"][b, i] = 1.0 if live else 0.0
  return out


def voxelize(point_clouds, voxel_size):
  """pcmi_det_voxelize.  Returns (voxel_coords [M, 4] int32, voxel_inds [M] int32, voxel_feats [M, 3] float32, counts [B + 1]
  int64, flags [B]): per scene the voxels in the order of their first row."""
  pc = np.asarray(point_clouds, dtype=np.float32)
  B, P = pc.shape[:2]
  vs = np.float32(voxel_size)
  flags = np.zeros(B, np.int32)
  coords, inds, counts = [], [], []
  for b in range(B):
    with np.errstate(invalid="ignore", over="ignore"):
      f = np.floor(pc[b] / vs)
    ok = (np.abs(f) < np.float32(VOXEL_LIMIT)).all(1)
    if not ok.all():
      flags[b] |= FLAG_RANGE
    v = np.where(ok[:, None], f, 0).astype(np.int32)
    mn = v[ok].min(0) if ok.any() else np.zeros(3, np.int32)
    span = ((v - mn >= 0) & (v - mn < SPAN)).all(1)
    if (ok & ~span).any():
      flags[b] |= FLAG_SPAN
    ok = ok & span
    seen, rows = set(), []
    for i in np.nonzero(ok)[0]:
      key = (int(v[i, 0]), int(v[i, 1]), int(v[i, 2]))
      if key not in seen:
        seen.add(key)
        rows.append(i)
    rows = np.asarray(rows, dtype=np.int64)
    coords.append(np.concatenate([np.full((len(rows), 1), b, np.int32), v[rows].reshape(-1, 3)], 1).astype(np.int32))
    inds.append(rows.astype(np.int32))
    counts.append(len(rows))
  M = sum(counts)
  return (np.concatenate(coords, 0).reshape(M, 4), np.concatenate(inds, 0), np.ones((M, 3), np.float32),
          np.asarray(counts + [M], dtype=np.int64), flags)


def pad_boxes(box_list, dataset):
  """The [B, 64, 8] box block and n_boxes [B] from the per-scene arrays: ScanNet [k, 7] (the label id moves to column 7),
  SUN RGB-D [k, 8]."""
  B = len(box_list)
  out = np.zeros((B, MAX_NUM_OBJ, 8), np.float64)
  n = np.zeros(B, np.int32)
  for b, bx in enumerate(box_list):
    bx = np.asarray(bx, dtype=np.float64)
    k = bx.shape[0]
    n[b] = k
    if k == 0:
      continue
    if dataset == "scannet":
      out[b, :k, 0:6] = bx[:, 0:6]
      out[b, :k, 7] = bx[:, -1]
    else:
      out[b, :k] = bx
  return out, n


def batch(dataset, scenes, choices, augment, flip, rot_angle, scale, voxel_size, valid_sem=None, label_to_class=None, mean_size=None,
          num_heading_bin=12, point_clouds=None):
  """The whole pipeline, as DetectionInputPipeline chains the entry points.  scenes as the pipeline takes them; flip [B, 2],
  rot_angle [B], scale [B].  point_clouds: if given, the votes from instances and the voxels are computed from these instead of
  from the restatement's own (the golden comparison feeds the reference's).  Returns the batch dict (numpy) plus flags."""
  B = len(scenes)
  sizes = [len(s[0]) for s in scenes]
  offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
  xyz = np.concatenate([np.asarray(s[0], dtype=np.float32).reshape(-1, 3) for s in scenes])
  rot = np.stack([rotz(t) for t in np.asarray(rot_angle, dtype=np.float64)])
  kw = dict(augment=augment, flip=flip, rot=rot, scale=scale)
  if dataset == "scannet":
    s = sample_transform(xyz, offsets, choices, instance=np.concatenate([np.asarray(x[1]).reshape(-1) for x in scenes]),
                         semantic=np.concatenate([np.asarray(x[2]).reshape(-1) for x in scenes]), **kw)
    pc = s["point_clouds"] if point_clouds is None else np.asarray(point_clouds, dtype=np.float32)
    vl, vm, f2 = votes_from_instances(pc, s["out_instance"], s["out_semantic"], valid_sem)
    boxes, n_boxes = pad_boxes([x[3] for x in scenes], "scannet")
    out = box_labels(boxes, n_boxes, SCANNET, label_to_class=label_to_class, mean_size=mean_size, num_heading_bin=1, **kw)
  else:
    s = sample_transform(xyz, offsets, choices, votes=np.concatenate([np.asarray(x[2], dtype=np.float64).reshape(-1, 10) for x in scenes]), **kw)
    pc = s["point_clouds"] if point_clouds is None else np.asarray(point_clouds, dtype=np.float32)
    vl, vm, f2 = s["vote_label"], s["vote_label_mask"], 0
    boxes, n_boxes = pad_boxes([x[1] for x in scenes], "sunrgbd")
    out = box_labels(boxes, n_boxes, SUNRGBD, rot_angle=rot_angle, mean_size=mean_size, num_heading_bin=num_heading_bin, **kw)
  vc, vi, vf, counts, f3 = voxelize(pc, voxel_size)
  out["flags"] = out["flags"] | s["flags"] | f2 | f3
  out.update(point_clouds=s["point_clouds"], vote_label=vl, vote_label_mask=vm, voxel_coords=vc, voxel_inds=vi, voxel_feats=vf, counts=counts)
  return out


def nyu40id_table(ids):
  """label_to_class of pcmi_det_box_labels from the reference's nyu40ids: the id's position, -1 elsewhere."""
  ids = np.asarray(ids).reshape(-1)
  t = np.full(int(ids.max()) + 1, -1, np.int32)
  t[ids] = np.arange(len(ids))
  return t
