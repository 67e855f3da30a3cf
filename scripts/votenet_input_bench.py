"""Times the on-device detection input (csrc/detect_input.hip, pointcontrast_amd.downstream.votenet.DetectionInputPipeline) at
the shape of the reference's ScanNet recipe (scripts/train_scannet.sh): B synthetic rooms of 50 000 to 150 000 vertices (floor,
ceiling, walls and about 30 box-shaped objects with an instance id each), 40 000 points chosen per room, 64 box slots, 2.5 cm
voxels, sampled draws.
  * each entry point on tensors that already sit on the device -- pcmi_det_sample_transform, pcmi_det_votes_from_instances,
    pcmi_det_box_labels, pcmi_det_voxelize -- with device events, median after warm-up;
  * the whole DetectionInputPipeline.__call__ from host arrays, upload and read-back included: wall clock with a synchronise;
  * the host path it replaces, one scan after another as a DataLoader worker would: the numpy restatement
    tests/detect_input_ref.py (which loops over instances, box slots and voxel rows in Python as the reference's __getitem__
    does), wall clock (--host-repeats 0 leaves it out).
--height and --color add the feature columns (csrc/detect_features.hip; DetectionInputPipeline(use_height, use_color)): the
device time of pcmi_segment_quantile over every room's z (all of its launches), of pcmi_det_point_features, and the same work
in numpy on the host -- np.percentile per scan, then the gathers and the colour arithmetic; the whole call then includes them.
One JSON line per measurement.

  python scripts/votenet_input_bench.py [--scenes 32] [--points 40000] [--vertices 50000 150000] [--height] [--color] [--warmup 3] [--repeats 15] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

NYU = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39])


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


def make_room(rng, n, n_obj=30):
  """n vertices: 60 % on the faces of a 6 x 5 x 2.6 m room (instance 0, wall / floor labels), the rest on n_obj boxes standing on
  the floor (instance 1.., a detection class each).  Returns (vertices float32, instance, semantic, boxes [n_obj, 7])."""
  size = np.array([6.0, 5.0, 2.6])
  n_room = int(n * 0.6)
  face = rng.randint(0, 6, n_room)
  xyz = rng.rand(n_room, 3) * size
  axis, side = face // 2, face % 2
  xyz[np.arange(n_room), axis] = side * size[axis] + rng.normal(0, 0.004, n_room)
  ins, sem = [np.zeros(n_room, np.int32)], [np.where(axis == 2, 2, 1).astype(np.int32)]
  pts = [xyz]
  boxes = np.zeros((n_obj, 7))
  per = (n - n_room) // n_obj
  for k in range(n_obj):
    m = per if k < n_obj - 1 else n - n_room - per * (n_obj - 1)
    dim = rng.uniform(0.3, 1.2, 3)
    cen = np.array([rng.uniform(0.7, 5.3), rng.uniform(0.7, 4.3), dim[2] / 2])
    p = cen + (rng.rand(m, 3) - 0.5) * dim
    f = rng.randint(0, 3, m)
    p[np.arange(m), f] = cen[f] + np.where(rng.rand(m) < 0.5, -0.5, 0.5) * dim[f]
    cls = int(rng.choice(NYU))
    pts.append(p), ins.append(np.full(m, k + 1, np.int32)), sem.append(np.full(m, cls, np.int32))
    boxes[k] = np.concatenate([cen, dim, [cls]])
  return np.concatenate(pts).astype(np.float32), np.concatenate(ins), np.concatenate(sem), boxes


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--scenes", type=int, default=32)
  ap.add_argument("--points", type=int, default=40000)
  ap.add_argument("--voxel-size", type=float, default=0.025)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--repeats", type=int, default=15)
  ap.add_argument("--host-repeats", type=int, default=2)
  ap.add_argument("--vertices", type=int, nargs=2, default=[50000, 150000], metavar=("LO", "HI"),
                  help="vertices per room, drawn from [LO, HI]; rooms of up to 16384 take pcmi_segment_quantile's one-workgroup launch")
  ap.add_argument("--height", action="store_true", help="the height column: DetectionInputPipeline(use_height=True)")
  ap.add_argument("--color", action="store_true", help="the colour columns: DetectionInputPipeline(use_color=True), vertices [n, 6]")
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  import detect_input_ref as dr
  from pointcontrast_amd import functional as PF
  from pointcontrast_amd.downstream import votenet
  dev = torch.device("cuda:0")
  B, P, vs = args.scenes, args.points, args.voxel_size
  rng = np.random.RandomState(0)
  scenes = [make_room(rng, int(rng.randint(args.vertices[0], args.vertices[1] + 1))) for _ in range(B)]
  sizes = [len(s[0]) for s in scenes]
  scenes_xyz = scenes
  if args.color:  # vertices [n, 6]: xyz, then rgb in 0..255 as the ScanNet arrays hold it
    crng = np.random.RandomState(1)
    scenes = [(np.concatenate([s[0], crng.randint(0, 256, (len(s[0]), 3)).astype(np.float32)], 1),) + s[1:] for s in scenes]
  mean = rng.uniform(0.3, 1.5, (18, 3))
  draws = votenet.DetectionDraws.sample(sizes, P, "scannet", 1)
  pipe = votenet.DetectionInputPipeline("scannet", P, vs, dev, mean_size_arr=mean, use_height=args.height, use_color=args.color)
  results = []

  def emit(name, **kw):
    results.append(dict(name=name, scenes=B, num_points=P, vertices=int(sum(sizes)), voxel_size=vs, **kw))
    print(json.dumps(results[-1]), flush=True)

  host = pipe.host_inputs(scenes, draws)
  d = votenet._upload(dict(host), dev)
  aug = dict(augment=True, flip=d["flip"], rot=d["rot"], scale=d["scale"])
  emit("upload", **wall_ms(lambda: votenet._upload(dict(host), dev), args.warmup, args.repeats),
       megabytes=sum(np.asarray(v).nbytes for v in host.values()) / 1e6)

  def sample():
    return PF.det_sample_transform(d["xyz"], d["offsets"], d["choices"], instance=d["instance"], semantic=d["semantic"], **aug)

  emit("stage_sample_transform", **device_ms(sample, args.warmup, args.repeats))
  s = sample()
  emit("stage_votes_from_instances",
       **device_ms(lambda: PF.det_votes_from_instances(s["point_clouds"], s["out_instance"], s["out_semantic"], pipe._valid),
                   args.warmup, args.repeats))
  emit("stage_box_labels",
       **device_ms(lambda: PF.det_box_labels(d["boxes"], d["n_boxes"], "scannet", pipe._mean, label_to_class=pipe._lut, **aug),
                   args.warmup, args.repeats))
  emit("stage_voxelize", **device_ms(lambda: PF.det_voxelize(s["point_clouds"], vs), args.warmup, args.repeats),
       voxels=int(PF.det_voxelize(s["point_clouds"], vs)["counts"][B]))
  if args.height or args.color:
    def quantile():
      return PF.segment_quantile(d["xyz"], d["offsets"], 0.99, column=2)["quantile"]

    if args.height:
      emit("stage_segment_quantile", **device_ms(quantile, args.warmup, args.repeats))
    floor = quantile() if args.height else None
    emit("stage_point_features", columns=pipe.feature_dim,
         **device_ms(lambda: PF.det_point_features(s["point_clouds"], d["xyz"], d["offsets"], d["choices"], "scannet", rgb=d.get("rgb"),
                                                   floor_height=floor, augment=True), args.warmup, args.repeats))

    def host_features():  # the reference's lines per scan: the percentile over every vertex, then the columns of the chosen rows
      for b, sc in enumerate(scenes):
        v, cols = sc[0], []
        c = draws.choices[b]
        if args.color:
          cols.append(((v[c, 3:6] - np.array([109.8, 97.2, 83.8])) / 256.0).astype(np.float32))
        if args.height:
          cols.append((v[c, 2] - np.percentile(v[:, 2], 0.99))[:, None])
        np.concatenate(cols, 1)

    emit("host_numpy_feature_columns", columns=pipe.feature_dim, **wall_ms(host_features, 1, max(args.host_repeats, 3), sync=False))
  emit("pipeline_call", feature_columns=pipe.feature_dim, **wall_ms(lambda: pipe(scenes, draws), args.warmup, args.repeats))
  lut = dr.nyu40id_table(NYU)

  def host_batch():
    for b, sc in enumerate(scenes_xyz):
      dr.batch("scannet", [sc], draws.choices[b:b + 1], True, draws.flip()[b:b + 1], draws.rot_angle[b:b + 1], draws.scale[b:b + 1], vs,
               valid_sem=NYU, label_to_class=lut, mean_size=mean)

  if args.host_repeats > 0:
    emit("host_numpy_restatement_batch", **wall_ms(host_batch, 0, args.host_repeats, sync=False))
  if args.out:
    with open(args.out, "w") as f:
      for r in results:
        f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
  main()
