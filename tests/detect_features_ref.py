"""numpy restatement of the feature-column entry points (pcmi_segment_quantile and pcmi_det_point_features of
csrc/detect_features.hip) under exactly the rules that include/pcmi.h writes down: the same operation order, the same
precision of every product and sum, the same flags.  The GPU tests compare the kernels with this bit for bit;
tests/test_detect_features_ref.py holds it to np.sort, np.percentile and to what the reference's own dataset classes returned
(tests/golden/golden_detfeatures.npz)."""
import numpy as np

import detect_input_ref as R

FLAG_FEATURE = 64
SCANNET_MEAN = np.array([109.8, 97.2, 83.8], dtype=np.float64)


def rank_of(m, q):
  """(k, g) of a scene of m values: v = (m - 1) (q / 100), k = floor(v), g = v - k, in float64."""
  f = np.float64(q) / np.float64(100.0)
  v = np.float64(m - 1) * f
  k = np.floor(v)
  k = min(max(k, np.float64(0.0)), np.float64(m - 1))
  return int(k), np.float64(v - k)


def _plus_zero(x):
  return x if x != 0 else type(x)(0)


def segment_quantile(values, offsets, q):
  """pcmi_segment_quantile.  values float32 [n] (the column already taken).  Returns (out float64 [B], stats float32 [B, 2],
  flags int32 [B])."""
  values = np.asarray(values, dtype=np.float32).reshape(-1)
  offsets = np.asarray(offsets, dtype=np.int64)
  B, n = len(offsets) - 1, len(values)
  out, stats, flags = np.zeros(B, np.float64), np.zeros((B, 2), np.float32), np.zeros(B, np.int32)
  for b in range(B):
    lo, hi = int(offsets[b]), int(offsets[b + 1])
    m = hi - lo if 0 <= lo <= hi <= n else 0
    z = values[lo:lo + m]
    if m == 0 or not np.isfinite(z).all():
      flags[b] |= FLAG_FEATURE
      continue
    k, g = rank_of(m, q)
    img = np.sort(R._ord32(z))  # the order of the integer images: the floats' own, -0.0 below +0.0
    a, c = R._unord32(img[k:k + 1])[0], R._unord32(img[min(k + 1, m - 1):min(k + 1, m - 1) + 1])[0]
    a, c = _plus_zero(a), _plus_zero(c)
    d = np.float64(c) - np.float64(a)
    w = d * g
    r = np.float64(a) + w
    out[b] = _plus_zero(r)
    stats[b] = a, c
  return out, stats, flags


def point_features(point_clouds, xyz, offsets, choices, dataset, rgb=None, floor_height=None, augment=False, scale=None, color_gain=None,
                   color_shift=None, color_jitter=None, color_keep=None):
  """pcmi_det_point_features.  Returns (point_clouds float32 [B, P, 3 + C], flags int32 [B])."""
  pc = np.asarray(point_clouds, dtype=np.float32)
  B, P = pc.shape[:2]
  xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
  n = len(xyz)
  offsets = np.asarray(offsets, dtype=np.int64)
  choices = np.asarray(choices, dtype=np.int32)
  C = (0 if rgb is None else 3) + (0 if floor_height is None else 1)
  assert C > 0
  out = np.zeros((B, P, 3 + C), np.float32)
  out[:, :, 0:3] = pc
  flags = np.zeros(B, np.int32)
  sun = dataset == "sunrgbd"
  for b in range(B):
    lo, hi = int(offsets[b]), int(offsets[b + 1])
    c = choices[b].astype(np.int64)
    ok = (c >= 0) & (c < hi - lo) if (0 <= lo <= hi <= n) else np.zeros(P, bool)
    if not ok.all():
      flags[b] |= R.FLAG_CHOICE
    g = np.where(ok, lo + c, 0)
    at = 3
    if rgb is not None:
      s = np.asarray(rgb, dtype=np.float32).reshape(-1, 3)[g] if n else np.zeros((P, 3), np.float32)
      fin = np.isfinite(s).all(1)
      if (ok & ~fin).any():
        flags[b] |= FLAG_FEATURE
      live = ok & fin
      s64 = np.where(live[:, None], s, 0).astype(np.float64)
      if not sun:
        col = ((s64 - SCANNET_MEAN) / 256.0).astype(np.float32)
      else:
        col = (s64 - 0.5).astype(np.float32)
        if augment:
          x = col.astype(np.float64) + 0.5
          x = x * (np.ones(3) if color_gain is None else np.asarray(color_gain, dtype=np.float64).reshape(B, 3)[b])
          x = x + (np.zeros(3) if color_shift is None else np.asarray(color_shift, dtype=np.float64).reshape(B, 3)[b])
          x = x + (np.zeros(P) if color_jitter is None else np.asarray(color_jitter, dtype=np.float64)[b])[:, None]
          x = np.minimum(np.maximum(x, 0.0), 1.0)
          x = x * (np.ones(P) if color_keep is None else (np.asarray(color_keep)[b] != 0).astype(np.float64))[:, None]
          col = (x - 0.5).astype(np.float32)
      out[b, :, at:at + 3] = np.where(live[:, None], col, np.float32(0))
      at += 3
    if floor_height is not None:
      z = xyz[g, 2] if n else np.zeros(P, np.float32)
      fin = np.isfinite(z)
      if (ok & ~fin).any():
        flags[b] |= FLAG_FEATURE
      live = ok & fin
      z64 = np.where(live, z, 0).astype(np.float64)
      h = (z64 - np.float64(np.asarray(floor_height, dtype=np.float64)[b])).astype(np.float32)
      if sun and augment:
        h = (h.astype(np.float64) * np.float64(scale[b])).astype(np.float32)
      out[b, :, at] = np.where(live, h, np.float32(0))
  return out, flags


def split_points(scenes):
  """(scenes with points [n, 3], the raw colours [sum n, 3] or None) from scenes whose points are [n, 3] or [n, 6]."""
  pts = [np.asarray(s[0], dtype=np.float32) for s in scenes]
  rgb = np.concatenate([p[:, 3:6] for p in pts]) if pts[0].shape[1] == 6 else None
  return [(p[:, 0:3],) + tuple(s[1:]) for p, s in zip(pts, scenes)], rgb


def batch(dataset, scenes, choices, augment, flip, rot_angle, scale, voxel_size, use_height=False, use_color=False, color_gain=None,
          color_shift=None, color_jitter=None, color_keep=None, **kw):
  """The whole pipeline with the feature columns, as DetectionInputPipeline(use_height, use_color) chains the entry points:
  detect_input_ref.batch on xyz, then the quantile of every scan's z and the feature columns."""
  scenes3, rgb = split_points(scenes)
  out = R.batch(dataset, scenes3, choices, augment, flip, rot_angle, scale, voxel_size, **kw)
  if not (use_height or use_color):
    return out
  assert not use_color or rgb is not None, "use_color: points [n, 6]"
  sizes = [len(s[0]) for s in scenes3]
  offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
  xyz = np.concatenate([s[0] for s in scenes3])
  floor = None
  if use_height:
    floor, _, f = segment_quantile(xyz[:, 2], offsets, 0.99)
    out["flags"] = out["flags"] | f
  pc, f = point_features(out["point_clouds"], xyz, offsets, choices, dataset, rgb=rgb if use_color else None, floor_height=floor,
                         augment=augment, scale=scale, color_gain=color_gain, color_shift=color_shift, color_jitter=color_jitter,
                         color_keep=color_keep)
  out["flags"] = out["flags"] | f
  out["point_clouds"] = pc
  return out
