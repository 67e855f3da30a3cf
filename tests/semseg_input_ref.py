"""A numpy restatement of csrc/semseg_input.hip (include/pcmi.h: pcmi_elastic_blur, pcmi_elastic_apply, pcmi_seg_transform,
pcmi_seg_quantize, pcmi_seg_color_augment) and of the pipeline's dropout in the SAME operation order: float64 arrays, one numpy operation per rounded operation, so the
kernels can be compared with it bit for bit.  tests/test_semseg_input_ref.py holds it to recorded outputs of the reference's
own Voxelizer and transforms (tests/golden/golden_seginput.npz)."""
import numpy as np

FLAG_RANGE, FLAG_SPAN, FLAG_ELASTIC = 1, 2, 4
VOXEL_LIMIT, SPAN = 1 << 20, 1 << 18


def _scenes(offsets, n):
  offs = np.clip(np.asarray(offsets, dtype=np.int64), 0, n)
  return [(b, int(offs[b]), int(max(offs[b + 1], offs[b]))) for b in range(len(offs) - 1)]


def elastic_blur_volume(vol):
  """Two rounds of the 3-tap box filter along x, y, z over one volume float32 [dx, dy, dz, 3], zero padding: per pass
  float32(((v[i-1] w + v[i] w) + v[i+1] w)) in float64 with w = float32(1/3) widened."""
  w = np.float64(np.float32(1.0) / np.float32(3.0))
  v = np.asarray(vol, dtype=np.float32)
  for _ in range(2):
    for axis in range(3):
      x = np.moveaxis(v.astype(np.float64), axis, 0)
      pad = np.zeros((1,) + x.shape[1:])
      lo, hi = np.concatenate([pad, x[:-1]]), np.concatenate([x[1:], pad])
      v = np.moveaxis(((lo * w + x * w) + hi * w).astype(np.float32), 0, axis)
  return v


def elastic_apply_scene(p, vol, mn, d, g, mag):
  """p float64 [m, 3] + trilinear(vol)(p) * mag on the grid np.linspace(mn - g, mn + g (d - 2), d) per axis; a point outside the
  grid (or NaN) is returned as it is.  The interval of a point on a node starts at that node, the last node belongs to the
  last interval (scipy's rule)."""
  p, mn, d = np.array(p, dtype=np.float64).reshape(-1, 3), np.asarray(mn, np.float64), np.asarray(d, np.int64)
  g, mag = np.float64(g), np.float64(mag)
  start, stop = mn - g, mn + g * (d - 2).astype(np.float64)
  step = (stop - start) / (d - 1).astype(np.float64)
  with np.errstate(invalid="ignore"):
    inside = ((p >= start) & (p <= stop)).all(1)
  rows = np.flatnonzero(inside)
  pi = p[rows]
  idx, wt = np.zeros((len(rows), 3), np.int64), np.zeros((len(rows), 3))
  for a in range(3):
    nodes = np.arange(d[a]).astype(np.float64) * step[a] + start[a]
    nodes[-1] = stop[a]
    k = np.clip(np.searchsorted(nodes, pi[:, a], side="right") - 1, 0, d[a] - 2)
    idx[:, a] = k
    wt[:, a] = (pi[:, a] - nodes[k]) / (nodes[k + 1] - nodes[k])
  val = np.zeros((len(rows), 3))
  for c in range(8):
    o = ((c >> 2) & 1, (c >> 1) & 1, c & 1)
    ws = [wt[:, a] if o[a] else 1.0 - wt[:, a] for a in range(3)]
    w = (ws[0] * ws[1]) * ws[2]
    val = val + vol[idx[:, 0] + o[0], idx[:, 1] + o[1], idx[:, 2] + o[2]].astype(np.float64) * w[:, None]
  p[rows] = pi + val * mag
  return p


def elastic_stage(xyz, offsets, granularity, magnitude, noise, active=None):
  """One (granularity, magnitude) stage for the batch.  noise float32 [B, cx, cy, cz, 3] capacity blocks.
  -> xyz float64 [n, 3] (new), noise (the blocks after the blur), grid_dims int32 [B, 4], flags int32 [B]."""
  xyz = np.array(xyz, dtype=np.float64).reshape(-1, 3)
  noise = np.array(noise, dtype=np.float32)
  B, cap = noise.shape[0], np.array(noise.shape[1:4])
  g, mag = np.float64(granularity), np.float64(magnitude)
  dims, flags = np.zeros((B, 4), np.int32), np.zeros(B, np.int32)
  for b, lo, hi in _scenes(offsets, len(xyz)):
    p = xyz[lo:hi]
    finite = np.isfinite(p).all(1)
    if not finite.any():
      continue
    mn, mx = p[finite].min(0), p[finite].max(0)
    q = ((mx - mn) // g) + 3.0
    on = active is None or bool(active[b])
    if not (q <= cap).all():
      if on:
        flags[b] |= FLAG_ELASTIC
      continue
    d = q.astype(np.int64)
    dims[b, :3], dims[b, 3] = d, int(on)
    if not on:
      continue
    vol = elastic_blur_volume(noise[b, :d[0], :d[1], :d[2]])
    noise[b, :d[0], :d[1], :d[2]] = vol
    xyz[lo:hi] = elastic_apply_scene(p, vol, mn, d, g, mag)
  return xyz, noise, dims, flags


def dropout_rows(keys, ratio=0.2):
  """The rows that RandomDropout keeps: the int(m (1 - ratio)) rows with the smallest keys (ties: the lower row), ascending."""
  keys = np.asarray(keys)
  return np.sort(np.argsort(keys, kind="stable")[:int(len(keys) * (1 - ratio))])


def seg_transform(xyz, offsets, mats, clip_bound=None, trans_ratio=None):
  """-> vox int32 [n, 3], keep uint8 [n], scene_min int32 [B, 3], aligned float64 [B, 16], flags int32 [B]."""
  xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
  n = len(xyz)
  mats = np.asarray(mats, dtype=np.float64).reshape(-1, 4, 4)
  B = len(mats)
  vox, keep = np.zeros((n, 3), np.int32), np.zeros(n, np.uint8)
  scene_min, aligned, flags = np.zeros((B, 3), np.int32), np.zeros((B, 4, 4)), np.zeros(B, np.int32)
  for b, lo, hi in _scenes(offsets, n):
    p, m = xyz[lo:hi], mats[b]
    finite = np.isfinite(p).all(1)
    ok = finite.copy()
    bad = ~finite
    if clip_bound is not None and finite.any():
      mn, mx = p[finite].min(0), p[finite].max(0)
      size = mx - mn
      center = mn + size * 0.5
      center = center + (np.zeros(3) if trans_ratio is None else np.asarray(trans_ratio, np.float64).reshape(-1, 3)[b]) * size
      if isinstance(clip_bound, (int, float)):
        L = float(clip_bound)
        if not size.max() < L:
          ok &= ((p >= -L + center) & (p < L + center)).all(1)
      else:
        lim = np.asarray(clip_bound, dtype=np.float64).reshape(3, 2)
        ok &= ((p >= lim[:, 0] + center) & (p < lim[:, 1] + center)).all(1)
    with np.errstate(invalid="ignore", over="ignore"):
      f = np.stack([np.floor(((p[:, 0] * m[r, 0] + p[:, 1] * m[r, 1]) + p[:, 2] * m[r, 2]) + m[r, 3]) for r in range(3)], 1)
      inside = (np.abs(f) < VOXEL_LIMIT).all(1)  # NaN: False
    bad |= ok & ~inside
    ok &= inside
    if bad.any():
      flags[b] |= FLAG_RANGE
    vox[lo:hi][ok] = f[ok].astype(np.int32)
    keep[lo:hi] = ok
    if ok.any():
      scene_min[b] = vox[lo:hi][ok].min(0)
    aligned[b] = m
    for r in range(3):
      aligned[b, r] = m[r] + (-float(scene_min[b, r])) * m[3]
  return vox, keep, scene_min, aligned.reshape(B, 16), flags


def seg_quantize(vox, offsets, labels=None, keep=None, scene_min=None, ignore_label=255):
  """-> coords int32 [M, 4], index int64 [M], labels int32 [M] (None without labels), counts int64 [B + 1], flags int32 [B]."""
  vox = np.asarray(vox, dtype=np.int64).reshape(-1, 3)
  n, B = len(vox), len(offsets) - 1
  mins = np.zeros((B, 3), np.int64) if scene_min is None else np.asarray(scene_min, np.int64).reshape(B, 3)
  coords, index, out_labels, counts, flags = [], [], [], np.zeros(B + 1, np.int64), np.zeros(B, np.int32)
  for b, lo, hi in _scenes(offsets, n):
    seen = {}
    for i in range(lo, hi):
      if keep is not None and not keep[i]:
        continue
      d = vox[i] - mins[b]
      if (d < 0).any() or (d >= SPAN).any():
        flags[b] |= FLAG_SPAN
        continue
      key = tuple(int(v) for v in d)
      if key not in seen:
        seen[key] = len(coords)
        coords.append((b,) + key)
        index.append(i)
        out_labels.append(int(labels[i]) if labels is not None else 0)
        counts[b] += 1
      elif labels is not None and int(labels[i]) != int(labels[index[seen[key]]]):
        out_labels[seen[key]] = int(ignore_label)
  counts[B] = len(coords)
  return (np.asarray(coords, np.int32).reshape(-1, 4), np.asarray(index, np.int64),
          np.asarray(out_labels, np.int32) if labels is not None else None, counts, flags)


def seg_color_augment(feats_src, coords, n_scenes, index=None, labels=None, params=None, normals=None, normalize=False,
                      label_lut=None, ignore_label=255):
  """-> (coords int32 [m, 4], feats float64 [m, 3] BEFORE the final rounding to float32, labels int32 [m] or None)."""
  coords = np.array(coords, dtype=np.int32).reshape(-1, 4)
  m, B = len(coords), int(n_scenes)
  src = np.asarray(feats_src, dtype=np.float32).reshape(-1, 3)
  idx = np.arange(m) if index is None else np.asarray(index, np.int64)
  inside = (idx >= 0) & (idx < len(src))
  raw = np.zeros((m, 3), np.float32)
  raw[inside] = src[idx[inside]]
  f = raw.astype(np.float64)
  out_coords = coords.copy()
  if params is not None:
    P = np.asarray(params, np.float64).reshape(B, 12)
    for b in range(B):
      rows = np.flatnonzero(coords[:, 0] == b)
      if len(rows) == 0:
        continue
      q = P[b]
      for a in range(3):
        if q[a] != 0:
          out_coords[rows, 1 + a] = coords[rows, 1 + a].max() - coords[rows, 1 + a]
        g = f[rows, a]
        if q[3] != 0:
          ch = raw[rows, a][inside[rows]]
          ch = ch[~np.isnan(ch)]
          if len(ch) and ch.max() > ch.min():
            lo, hi = float(ch.min()), float(ch.max())
            scale = 255.0 / (hi - lo)
            g = (1.0 - q[4]) * g + q[4] * ((g - lo) * scale)
        if q[5] != 0:
          g = np.minimum(np.maximum(q[6 + a] + g, 0.0), 255.0)
        if q[9] != 0 and normals is not None:
          g = np.minimum(np.maximum(np.asarray(normals, np.float32)[rows, a].astype(np.float64) * q[10] + g, 0.0), 255.0)
        f[rows, a] = g
  if normalize:
    f = f / 255.0 - 0.5
  out_labels = None
  if labels is not None:
    out_labels = np.asarray(labels, np.int32).copy()
    if label_lut is not None:
      lut = np.asarray(label_lut, np.int32)
      ok = (out_labels >= 0) & (out_labels < len(lut))
      out_labels = np.where(ok, lut[np.clip(out_labels, 0, len(lut) - 1)], np.int32(ignore_label)).astype(np.int32)
  return out_coords, f, out_labels


def pipeline(scenes, mats, clip_bound=None, trans_ratio=None, params=None, normals=None, normalize=False, label_lut=None,
             ignore_label=255, limit_numpoints=0, elastic=None, dropout_keys=None):
  """SegmentationInputPipeline with injected draws: scenes = [(xyz, feats, labels)], -> coords, feats (float32), target,
  transformation [B', 16], with the batch truncated as cfl_collate_fn does (lib/transforms.py:251-283).  elastic: a list of
  (granularity, magnitude, noise, active) stages applied to the raw points; dropout_keys: float32 [rows] read by voxel row and
  dropout_on [B] as the pair (keys, on)."""
  sizes = [len(s[0]) for s in scenes]
  offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
  xyz = np.concatenate([np.asarray(s[0], np.float64).reshape(-1, 3) for s in scenes])
  feats = np.concatenate([np.asarray(s[1], np.float32).reshape(-1, 3) for s in scenes])
  labels = np.concatenate([np.asarray(s[2], np.int32).reshape(-1) for s in scenes])
  B = len(scenes)
  f0 = np.zeros(B, np.int32)
  for g, mag, noise, active in elastic or []:
    xyz, _, _, fe = elastic_stage(xyz, offs, g, mag, noise, active)
    f0 |= fe
  vox, keep, mn, aligned, f1 = seg_transform(xyz, offs, mats, clip_bound, trans_ratio)
  coords, index, lab, counts, f2 = seg_quantize(vox, offs, labels, keep, mn, ignore_label)
  flags = f0 | f1 | f2
  if dropout_keys is not None:
    keys, on = dropout_keys
    starts = np.concatenate([[0], np.cumsum(counts[:B])])
    rows = np.concatenate([starts[b] + (dropout_rows(keys[starts[b]:starts[b + 1]]) if on[b] else np.arange(counts[b])) for b in range(B)])
    rows = rows.astype(np.int64)
    counts = np.concatenate([np.bincount(coords[rows, 0], minlength=B), [len(rows)]]).astype(np.int64)
    coords, index, lab = coords[rows], index[rows], lab[rows]
  nb, total = truncate(counts[:B], limit_numpoints)
  c2, f, lab = seg_color_augment(feats, coords, B, index, lab, params, normals, normalize, label_lut, ignore_label)
  return c2[:total], f[:total].astype(np.float32), lab[:total], aligned[:nb], flags


def truncate(counts, limit_numpoints):
  """cfl_collate_fn's rule: scenes are added in order until the running number of rows would exceed limit_numpoints."""
  nb, total = 0, 0
  for c in counts:
    if limit_numpoints and total + int(c) > limit_numpoints:
      break
    total += int(c)
    nb += 1
  return nb, total
