"""A numpy restatement of csrc/insseg_input.hip (include/pcmi.h: pcmi_instance_relabel, pcmi_instance_table,
pcmi_seg_crop_ladder) and of downstream.insseg.InstanceInputPipeline, built on tests/semseg_input_ref.py.  Everything is integer
arithmetic, so the kernels are compared with it bit for bit.  tests/test_insseg_input_ref.py holds it to independent
spellings (np.unique, np.bincount / np.maximum.at, a loop over Python integers)."""
import numpy as np

import semseg_input_ref as sr

FLAG_CROP = 8
INT32_MAX, INT32_MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min


def _scenes(offsets, n):
  """(b, lo, hi) of every scene, clipped to the n rows; a row outside [offsets[0], offsets[B]) is in none."""
  return sr._scenes(offsets, n)


def instance_relabel(raw, offsets, keep=None):
  """-> instance int32 [n] (-1 for a row in no instance; rows outside every scene: -1 too, the kernel leaves them alone),
  first_row int32 [G], counts int64 [B + 1].  One pass in row order: an instance is numbered when its first row arrives."""
  raw = np.asarray(raw, dtype=np.int64).reshape(-1)
  n, B = len(raw), len(offsets) - 1
  inst, first, counts = np.full(n, -1, np.int32), [], np.zeros(B + 1, np.int64)
  for b, lo, hi in _scenes(offsets, n):
    seen = {}
    for i in range(lo, hi):
      if raw[i] < 0 or (keep is not None and not keep[i]):
        continue
      r = int(raw[i])
      if r not in seen:
        seen[r] = len(first)
        first.append(i)
        counts[b] += 1
      inst[i] = seen[r]
  counts[B] = len(first)
  return inst, np.asarray(first, np.int32), counts


def instance_table(instance, klass, coords, offsets, G):
  """-> dict(size, scene, cls int32 [G]; sum int64 [G, 3]; box_min, box_max int32 [G, 3]); cls / sum / boxes None without their
  input.  One pass over the rows in Python integers."""
  instance = np.asarray(instance, dtype=np.int64).reshape(-1)
  n = len(instance)
  size, scene = np.zeros(G, np.int32), np.full(G, -1, np.int32)
  cls = None if klass is None else np.full(G, -1, np.int32)
  s = None if coords is None else np.zeros((G, 3), np.int64)
  lo3 = None if coords is None else np.full((G, 3), INT32_MAX, np.int32)
  hi3 = None if coords is None else np.full((G, 3), INT32_MIN, np.int32)
  for b, lo, hi in _scenes(offsets, n):
    for i in range(lo, hi):
      g = int(instance[i])
      if g < 0 or g >= G:
        continue
      size[g] += 1
      scene[g] = max(scene[g], b)
      if klass is not None:
        cls[g] = max(int(cls[g]), int(klass[i]))
      if coords is not None:
        c = np.asarray(coords[i][1:4], np.int64)
        s[g] += c
        lo3[g], hi3[g] = np.minimum(lo3[g], c), np.maximum(hi3[g], c)
  return dict(size=size, scene=scene, cls=cls, sum=s, box_min=lo3, box_max=hi3)


def crop_origin(draw, ext, side):
  """(uint64(draw) (slack + 1)) >> 32 with slack = max(ext + 1 - side, 0), vectorised in uint64 (draw < 2^32, slack < 2^31)."""
  slack = np.maximum(np.asarray(ext, np.int64) + 1 - np.asarray(side, np.int64), 0)
  return ((np.asarray(draw, np.uint64) * (slack + 1).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)


def seg_crop_ladder(coords, offsets, axes, sides, draws, max_voxels):
  """-> rows int64 [M] (ascending), counts int64 [B + 1], step int32 [B], flags int32 [B]."""
  coords = np.asarray(coords, dtype=np.int64).reshape(-1, 4)
  n, B = len(coords), len(offsets) - 1
  sides = np.asarray(sides, dtype=np.int64).reshape(-1, 2)
  S = len(sides)
  draws = np.asarray(draws, dtype=np.uint64).reshape(B, S, 2)
  rows, counts, step, flags = [], np.zeros(B + 1, np.int64), np.full(B, -1, np.int32), np.zeros(B, np.int32)
  for b, lo, hi in _scenes(offsets, n):
    c = coords[lo:hi][:, list(axes)]
    inside = np.ones(hi - lo, bool)
    if hi - lo > max_voxels:
      ext = c.max(0)
      for s in range(S):
        origin = crop_origin(draws[b, s], ext, sides[s])
        inside = ((c >= origin) & (c < origin + sides[s])).all(1)
        step[b] = s
        if inside.sum() <= max_voxels:
          break
      else:
        flags[b] |= FLAG_CROP
    rows.append(lo + np.flatnonzero(inside))
    counts[b] = inside.sum()
  counts[B] = counts[:B].sum()
  return np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, np.int64), counts, step, flags


def pipeline(scenes, mats, clip_bound=None, trans_ratio=None, params=None, normals=None, normalize=False, label_lut=None,
             ignore_label=255, limit_numpoints=0, elastic=None, dropout_keys=None, stuff_classes=(0, 1), crop=None, crop_draws=None,
             horizontal_axes=(0, 1)):
  """InstanceInputPipeline with injected draws: scenes = [(xyz, feats, labels, instance_ids)] -> coords, feats (float32),
  target, instance, n_instances, transformation [B', 16], flags, step.  The stages of semseg_input_ref.pipeline in its order,
  with the voxel's raw id (a second seg_quantize with -1 as the ignore label), the crop = (sides, max_voxels) and the
  relabelling between the quantizer and the dropout; dropout_keys and normals are read by voxel row AFTER the crop."""
  B = len(scenes)
  offs = np.concatenate([[0], np.cumsum([len(s[0]) for s in scenes])]).astype(np.int64)
  xyz = np.concatenate([np.asarray(s[0], np.float64).reshape(-1, 3) for s in scenes])
  feats = np.concatenate([np.asarray(s[1], np.float32).reshape(-1, 3) for s in scenes])
  labels = np.concatenate([np.asarray(s[2], np.int32).reshape(-1) for s in scenes])
  ids = np.concatenate([np.asarray(s[3], np.int32).reshape(-1) for s in scenes])
  flags = np.zeros(B, np.int32)
  for g, mag, noise, active in elastic or []:
    xyz, _, _, fe = sr.elastic_stage(xyz, offs, g, mag, noise, active)
    flags |= fe
  vox, keep, mn, aligned, f1 = sr.seg_transform(xyz, offs, mats, clip_bound, trans_ratio)
  coords, index, lab, counts, f2 = sr.seg_quantize(vox, offs, labels, keep, mn, ignore_label)
  coords2, _, raw, counts2, _ = sr.seg_quantize(vox, offs, ids, keep, mn, -1)
  assert np.array_equal(coords, coords2) and np.array_equal(counts, counts2), "the two quantizer calls give the same voxels"
  flags |= f1 | f2
  step = np.full(B, -1, np.int32)
  voffs = np.concatenate([[0], np.cumsum(counts[:B])]).astype(np.int64)
  if crop is not None:
    rows, counts, step, f3 = seg_crop_ladder(coords, voffs, [1 + a for a in horizontal_axes], crop[0], crop_draws, crop[1])
    flags |= f3
    coords, index, lab, raw = coords[rows], index[rows], lab[rows], raw[rows]
    voffs = np.concatenate([[0], np.cumsum(counts[:B])]).astype(np.int64)
  mapped = lab
  if label_lut is not None:
    lut = np.asarray(label_lut, np.int32)
    ok = (lab >= 0) & (lab < len(lut))
    mapped = np.where(ok, lut[np.clip(lab, 0, len(lut) - 1)], np.int32(ignore_label))
  keep_inst = (mapped != ignore_label) & ~np.isin(mapped, list(stuff_classes))
  inst, _, inst_counts = instance_relabel(raw, voffs, keep_inst)
  if dropout_keys is not None:
    keys, on = dropout_keys
    rows = np.concatenate([voffs[b] + (sr.dropout_rows(keys[voffs[b]:voffs[b + 1]]) if on[b] else np.arange(counts[b])) for b in range(B)])
    rows = rows.astype(np.int64)
    counts = np.concatenate([np.bincount(coords[rows, 0], minlength=B), [len(rows)]]).astype(np.int64)
    coords, index, lab, inst = coords[rows], index[rows], lab[rows], inst[rows]
  nb, total = sr.truncate(counts[:B], limit_numpoints)
  coords, index, lab, inst = coords[:total], index[:total], lab[:total], inst[:total]
  c2, f, lab = sr.seg_color_augment(feats, coords, max(nb, 1), index, lab, None if params is None else np.asarray(params)[:max(nb, 1)],
                                    None if normals is None else np.asarray(normals)[:total], normalize, label_lut, ignore_label)
  return c2, f.astype(np.float32), lab, inst, int(inst_counts[:nb].sum()), aligned[:nb], flags, step
