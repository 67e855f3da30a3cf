"""Times the on-device segmentation input (csrc/semseg_input.hip, pointcontrast_amd.downstream.semseg.SegmentationInputPipeline)
on one synthetic ScanNet-like batch: B rooms (floor, ceiling and four walls of a 6 x 5 x 2.6 m box, uniformly sampled, random
colours, 20 raw labels in patches) of N points each at 2 cm voxels, with the SCANNET_2CM augmentation and sampled draws.
  * the stages on tensors that already sit on the device -- the two elastic stages (pcmi_elastic_blur + pcmi_elastic_apply
    each, with the copies of the points and the noise they change in place), pcmi_seg_transform, pcmi_seg_quantize,
    pcmi_seg_color_augment -- with device events, median after warm-up;
  * the upload of the batch (xyz float64, colours, labels) and the whole SegmentationInputPipeline.__call__ from host arrays,
    read-back included: wall clock with a synchronise, median;
  * the host path it replaces, one scan after another as a DataLoader worker would, wall clock, median: the elastic distortion
    with scipy as the reference calls it (ndimage.convolve, RegularGridInterpolator) on its own, then the rest restated in
    vectorised numpy (homogeneous transform and floor, np.unique over the voxel rows with the label rule, dropout, flip,
    auto-contrast, translation, jitter, normalisation, label map).  Every scene is distorted and dropped from on both sides.
One JSON line per measurement.

  python scripts/semseg_input_bench.py [--scenes 8] [--points 150000] [--warmup 3] [--repeats 15] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def device_ms(fn, warmup, repeats):
  """Median / min / max stream time of fn() in ms (HIP events), after `warmup` untimed calls."""
  for _ in range(warmup):
    fn()
  torch.cuda.synchronize()
  ms = []
  for _ in range(repeats):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    ms.append(a.elapsed_time(b))
  return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))


def wall_ms(fn, warmup, repeats, sync=True):
  out = []
  for i in range(warmup + repeats):
    if sync:
      torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    if sync:
      torch.cuda.synchronize()
    if i >= warmup:
      out.append((time.perf_counter() - t0) * 1e3)
  return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out))


def make_room(rng, n):
  """n points on the six faces of a 6 x 5 x 2.6 m box (faces drawn by area), colours in 0..255, raw labels 0..40 in patches."""
  size = np.array([6.0, 5.0, 2.6])
  area = np.array([size[1] * size[2], size[0] * size[2], size[0] * size[1]])
  face = rng.choice(6, size=n, p=np.repeat(area / (2 * area.sum()), 2))
  xyz = rng.rand(n, 3) * size
  axis, side = face // 2, face % 2
  xyz[np.arange(n), axis] = side * size[axis] + rng.normal(0, 0.004, n)
  feats = rng.randint(0, 256, size=(n, 3)).astype(np.float32)
  labels = ((np.floor(xyz[:, 0] / 0.75) * 7 + np.floor(xyz[:, 1] / 0.75) * 3 + face) % 41).astype(np.int32)
  return xyz, feats, labels


def host_elastic(xyz, params, noises):
  """ElasticDistortion as transforms.py:187-217 runs it, with the given noise volumes (capacity blocks: the corner is used)."""
  import scipy.interpolate
  import scipy.ndimage
  xyz = xyz.copy()
  for (g, mag), block in zip(params, noises):
    mn = xyz.min(0)
    d = ((xyz - mn).max(0) // g).astype(int) + 3
    v = np.ascontiguousarray(block[:d[0], :d[1], :d[2]])
    for _ in range(2):
      for shape in ((3, 1, 1, 1), (1, 3, 1, 1), (1, 1, 3, 1)):
        v = scipy.ndimage.convolve(v, np.ones(shape).astype("float32") / 3, mode="constant", cval=0)
    ax = [np.linspace(a, b, k) for a, b, k in zip(mn - g, mn + g * (d - 2), d)]
    xyz += scipy.interpolate.RegularGridInterpolator(ax, v, bounds_error=0, fill_value=0)(xyz) * mag
  return xyz


def host_scan(aug, xyz, feats, labels, M, flip, blend, tr, std, normals, keys):
  """One scan through the rest of the host path in vectorised numpy: voxelize, quantize with the label rule, dropout, flip and
  colour."""
  homo = np.hstack([xyz, np.ones((len(xyz), 1))])
  vox = np.floor(homo @ M.T[:, :3]).astype(np.int64)
  vox -= vox.min(0)
  key = (vox[:, 0] << 40) | (vox[:, 1] << 20) | vox[:, 2]
  _, index, inverse = np.unique(key, return_index=True, return_inverse=True)
  lo, hi = np.full(len(index), 1 << 30), np.full(len(index), -1)
  np.minimum.at(lo, inverse, labels)
  np.maximum.at(hi, inverse, labels)
  target = np.where(lo == hi, lo, aug.ignore_label)
  rows = np.sort(np.argsort(keys[:len(index)], kind="stable")[:int(len(index) * (1 - aug.dropout_ratio))])
  index, target = index[rows], target[rows]
  coords, f = vox[index], feats[index].astype(np.float64)
  for a in range(3):
    if flip is not None and flip[a]:
      coords[:, a] = coords[:, a].max() - coords[:, a]
  if blend is not None:
    cl, ch = f.min(0, keepdims=True), f.max(0, keepdims=True)
    f = (1 - blend) * f + blend * ((f - cl) * (255 / np.where(ch > cl, ch - cl, 1)))
  if tr is not None:
    f = np.clip(tr + f, 0, 255)
  if std is not None:
    f = np.clip(normals[:len(f)] * (std * 255) + f, 0, 255)
  if aug.normalize_color:
    f = f / 255 - 0.5
  if aug.label_map is not None:
    inside = (target >= 0) & (target < len(aug.label_map))
    target = np.where(inside, aug.label_map[np.clip(target, 0, len(aug.label_map) - 1)], aug.ignore_label)
  return coords, f.astype(np.float32), target


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--scenes", type=int, default=8)
  ap.add_argument("--points", type=int, default=150000)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--repeats", type=int, default=15)
  ap.add_argument("--host-repeats", type=int, default=3)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  from pointcontrast_amd import functional as PF
  from pointcontrast_amd.downstream import semseg as ss
  dev = torch.device("cuda:0")
  B, n = args.scenes, args.points
  rng = np.random.RandomState(0)
  scenes = [make_room(rng, n) for _ in range(B)]
  aug = ss.SCANNET_2CM
  draws = ss.AugmentationDraws.sample(aug, scenes, np.random.RandomState(1), torch.Generator(device=dev).manual_seed(2), dev)
  draws.elastic_on, draws.dropout_on = [True] * B, [True] * B  # the costly case on both sides
  pipeline = ss.SegmentationInputPipeline(aug, dev)
  results = []

  def emit(name, **kw):
    results.append(dict(name=name, scenes=B, points=n, voxel_size=aug.voxel_size, **kw))
    print(json.dumps(results[-1]), flush=True)

  held = {}

  def upload():
    held["xyz"] = torch.cat([torch.from_numpy(s[0]) for s in scenes]).to(dev)
    held["feats"] = torch.cat([torch.from_numpy(s[1]) for s in scenes]).to(dev)
    held["labels"] = torch.cat([torch.from_numpy(s[2]) for s in scenes]).to(dev)

  emit("upload", **wall_ms(upload, args.warmup, args.repeats), megabytes=B * n * (24 + 12 + 4) / 1e6)
  offs = torch.arange(B + 1, dtype=torch.int64) * n
  mats = torch.from_numpy(draws.mats.reshape(B, 16)).to(dev)
  offs_dev = offs.to(dev)

  def elastic():
    xyz = held["xyz"].clone()
    for (g, mag), noise in zip(aug.elastic_params, draws.elastic_noise):
      noise = noise.clone()
      PF.elastic_apply(xyz, offs_dev, g, mag, noise, PF.elastic_blur(xyz, offs_dev, g, noise))
    return xyz

  emit("stage_elastic_two_stages", **device_ms(elastic, args.warmup, args.repeats),
       noise_blocks=[list(v.shape[1:4]) for v in draws.elastic_noise])
  held["xyz"] = elastic()

  def transform():
    return PF.seg_transform(held["xyz"], offs_dev, mats, aug.clip_bound, None)

  emit("stage_transform", **device_ms(transform, args.warmup, args.repeats))
  t = transform()

  def quantize():
    return PF.seg_quantize(t["vox"], offs_dev, held["labels"], t["keep"], t["scene_min"], aug.ignore_label)

  emit("stage_quantize", **device_ms(quantize, args.warmup, args.repeats))
  q = quantize()
  counts = q["counts"].cpu().numpy()
  M = int(counts[B])
  params = torch.from_numpy(PF.seg_color_params(B, draws.flip, draws.contrast, draws.translation, draws.jitter_std)).to(dev)
  lut = torch.from_numpy(aug.label_map).to(dev)
  index = q["index"][:M]

  def colour():  # in place on coords and labels, so each call works on a fresh copy of the M rows (the copies are timed too)
    return PF.seg_color_augment(held["feats"], q["coords"][:M].clone(), B, index, q["labels"][:M].clone(), params,
                                draws.normals[:M], aug.normalize_color, lut, aug.ignore_label)

  emit("stage_color_augment", **device_ms(colour, args.warmup, args.repeats), voxels=M)
  kept = {}
  emit("pipeline_call", **wall_ms(lambda: kept.update(rows=len(pipeline(scenes, draws)[0])), args.warmup, args.repeats), voxels=M,
       rows_after_dropout=kept["rows"])
  normals = draws.normals.cpu().numpy().astype(np.float64)
  keys = draws.dropout_keys.cpu().numpy()
  noises = [v.cpu().numpy() for v in draws.elastic_noise]
  distorted = []

  def host_el():
    distorted[:] = [host_elastic(s[0], aug.elastic_params, [v[b] for v in noises]) for b, s in enumerate(scenes)]

  emit("host_scipy_elastic_batch", **wall_ms(host_el, 1, args.host_repeats, sync=False))

  def host():
    for b, (_, feats, labels) in enumerate(scenes):
      host_scan(aug, distorted[b], feats, labels, draws.mats[b], draws.flip[b], draws.contrast[b], draws.translation[b],
                draws.jitter_std[b], normals[b * n:(b + 1) * n], keys[b * n:(b + 1) * n])

  emit("host_numpy_batch", **wall_ms(host, 1, args.host_repeats, sync=False))
  if args.out:
    with open(args.out, "w") as f:
      for r in results:
        f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
  main()
