"""Times the on-device instance input (csrc/insseg_input.hip, pointcontrast_amd.downstream.insseg.InstanceInputPipeline) at the
shape of scripts/semseg_input_bench.py plus instances, and the two instance evaluators' step with and without table=.

  input       B synthetic rooms (semseg_input_bench.make_room) of N points at 2 cm with the SCANNET_2CM augmentation and sampled
              draws, about 30 instances per room (1 m x 1 m patches of the floor plan, the same raw ids in every room), a crop to
              --max-voxels with an 8-step ladder: pcmi_instance_relabel, pcmi_instance_table, pcmi_seg_crop_ladder and the second
              pcmi_seg_quantize call (the ids as labels) on tensors that sit on the device; the whole
              InstanceInputPipeline.__call__ from host arrays beside SegmentationInputPipeline.__call__ on the same scans; the
              numpy restatement (tests/insseg_input_ref.py) of the three entry points on this machine's CPU, once.
  evaluators  scripts/insbench_bench.py's batch and degraded prediction: InstanceEvaluator.step and
              InstanceBenchmarkEvaluator.step as they are, and with PF.instance_table computed inside the timed call and passed
              as table=; with --parent FILE (downstream/insseg.py of the parent commit) the parent's two steps in the same loop.

Device times are HIP events around each call on warm kernels, the median of --runs with the variants ALTERNATING inside one loop
of one process (a call that reads back is timed with its wait).  The data are synthetic: nothing here says anything about
accuracy.  Prints one JSON line.

  python scripts/insseg_input_bench.py [--scenes 8] [--points 150000] [--max-voxels 120000] [--runs 25] [--no-host] [--parent FILE]
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from insbench_bench import MAX_INSTANCES, degrade  # noqa: E402
from insseg_bench import CLASSES, batch  # noqa: E402
from semseg_input_bench import make_room  # noqa: E402

LADDER = [[320, 320], [288, 288], [256, 256], [224, 224], [192, 192], [176, 176], [160, 160], [128, 128]]


def timed(variants, runs):
  """{name: dict(median, min, max, runs)} in ms from HIP events, the variants alternating inside one loop after two warm calls."""
  for fn in variants.values():
    for _ in range(2):
      fn()
  torch.cuda.synchronize()
  ms = {k: [] for k in variants}
  for _ in range(runs):
    for k, fn in variants.items():
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      fn()
      e1.record()
      e1.synchronize()
      ms[k].append(e0.elapsed_time(e1))
  return {k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), runs=runs) for k, v in ms.items()}


def load_parent(path):
  """downstream/insseg.py of another commit as a module of this package (its relative imports resolve to this tree)."""
  spec = importlib.util.spec_from_file_location("pointcontrast_amd.downstream._parent_insseg", path)
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--scenes", type=int, default=8)
  ap.add_argument("--points", type=int, default=150000)
  ap.add_argument("--max-voxels", type=int, default=120000)
  ap.add_argument("--boxes", type=int, default=30)
  ap.add_argument("--runs", type=int, default=25)
  ap.add_argument("--no-host", action="store_true")
  ap.add_argument("--parent", default=None)
  a = ap.parse_args()
  assert torch.cuda.is_available(), "insseg_input_bench measures the device path: it needs the GPU"
  from pointcontrast_amd import functional as PF
  from pointcontrast_amd.downstream import insseg as iseg, semseg as ss
  import insseg_input_ref as ir
  dev = torch.device("cuda", 0)
  B, n = a.scenes, a.points
  res = dict(scenes=B, points=n, max_voxels=a.max_voxels, ladder=LADDER, synthetic=True)

  # ---- the input ------------------------------------------------------------------------------------------------------------------
  rng = np.random.RandomState(0)
  scenes = []
  for _ in range(B):
    xyz, feats, labels = make_room(rng, n)
    scenes.append((xyz, feats, labels, (np.floor(xyz[:, 0]).clip(0, 5) * 5 + np.floor(xyz[:, 1]).clip(0, 4)).astype(np.int32)))
  aug = ss.SCANNET_2CM
  draws = ss.AugmentationDraws.sample(aug, scenes, np.random.RandomState(1), torch.Generator(device=dev).manual_seed(2), dev)
  draws.elastic_on, draws.dropout_on = [True] * B, [True] * B
  crop = (LADDER, a.max_voxels)
  crop_draws = iseg.InstanceInputPipeline.sample_crop_draws(crop, B, np.random.RandomState(3))
  sem, ins = ss.SegmentationInputPipeline(aug, dev), iseg.InstanceInputPipeline(aug, dev, crop=crop)
  sem_scenes = [s[:3] for s in scenes]
  st = ins.stage_upload(scenes, draws, crop_draws=crop_draws)
  ins.stage_voxelize(st)
  t, q = st["t"], st["q"]
  zero = torch.zeros(1, dtype=torch.int64, device=dev)
  voffs = torch.cat([zero, q["counts"][:B].cumsum(0)])
  axes = [1 + x for x in aug.horizontal_axes]
  quantize2 = lambda: PF.seg_quantize(t["vox"], st["offs_dev"], st["extra"][3], t["keep"], t["scene_min"], -1)  # noqa: E731
  raw = quantize2()["labels"]
  lut = torch.from_numpy(aug.label_map).to(dev)
  mapped = lut[q["labels"].clamp(0, len(lut) - 1).long()]
  keep = (mapped != aug.ignore_label) & (mapped != 0) & (mapped != 1)
  rl = PF.instance_relabel(raw, voffs, keep)
  counts = torch.cat([q["counts"], rl["counts"]]).cpu().numpy()
  M, G = int(counts[B]), int(counts[-1])
  cd = torch.as_tensor(crop_draws)  # the 32 bits of each draw, on the device once
  cd = torch.where(cd >= 2**31, cd - 2**32, cd).to(torch.int32).to(dev)
  cr = PF.seg_crop_ladder(q["coords"], voffs, axes, LADDER, cd, a.max_voxels)
  res.update(voxels=M, voxels_per_scene=counts[:B].tolist(), instances=G, crop_step=cr["step"].tolist(), crop_kept=int(cr["counts"][-1]))
  kept = {}
  variants = dict(
      instance_relabel=lambda: PF.instance_relabel(raw, voffs, keep),
      instance_table=lambda: PF.instance_table(rl["instance"], q["labels"], q["coords"], voffs, G),
      seg_crop_ladder=lambda: PF.seg_crop_ladder(q["coords"], voffs, axes, LADDER, cd, a.max_voxels),
      seg_quantize_second_call=quantize2,
      instance_pipeline_call=lambda: kept.update(ins=ins(scenes, draws, 0, crop_draws)),
      semantic_pipeline_call=lambda: kept.update(sem=sem(sem_scenes, draws)))
  res["input_device_ms"] = timed(variants, a.runs)
  res.update(pipeline_rows=len(kept["ins"][0]), pipeline_instances=kept["ins"][4], semantic_pipeline_rows=len(kept["sem"][0]),
             pipeline_crop_step=[int(s) for s in ins.last_crop_step])
  if not a.no_host:
    h = dict(raw=raw.cpu().numpy(), keep=keep.cpu().numpy(), voffs=voffs.cpu().numpy(), coords=q["coords"].cpu().numpy(),
             labels=q["labels"].cpu().numpy(), draws=np.asarray(crop_draws))
    t0 = time.perf_counter()
    w_inst, w_first, w_counts = ir.instance_relabel(h["raw"], h["voffs"], h["keep"])
    t1 = time.perf_counter()
    w_table = ir.instance_table(w_inst, h["labels"], h["coords"], h["voffs"], G)
    t2 = time.perf_counter()
    w_crop = ir.seg_crop_ladder(h["coords"], h["voffs"], axes, LADDER, h["draws"], a.max_voxels)
    t3 = time.perf_counter()
    res["host_numpy_ms"] = dict(instance_relabel=(t1 - t0) * 1e3, instance_table=(t2 - t1) * 1e3, seg_crop_ladder=(t3 - t2) * 1e3)
    tb = PF.instance_table(rl["instance"], q["labels"], q["coords"], voffs, G)
    res["host_agrees"] = bool(
        np.array_equal(rl["instance"][:M].cpu().numpy(), w_inst[:M]) and np.array_equal(rl["counts"].cpu().numpy(), w_counts) and
        all(np.array_equal(tb[k].cpu().numpy(), w_table[k]) for k in w_table) and
        np.array_equal(cr["rows"][:int(cr["counts"][-1])].cpu().numpy(), w_crop[0]) and np.array_equal(cr["step"].cpu().numpy(), w_crop[2]))
  del st, t, q, raw, rl, cr, kept
  torch.cuda.empty_cache()

  # ---- the evaluators' step ---------------------------------------------------------------------------------------------------------
  coords, cls, inst, offs, brng = batch(B, a.points, a.boxes)
  Ge = B * a.boxes
  pinst, pcls = degrade(inst, cls, a.boxes, brng)
  P = len(pcls)
  pscene = np.array([coords[np.flatnonzero(pinst == k)[0], 0] for k in range(P)], np.int32)
  pad = lambda v, fill, dt: np.concatenate([v, np.full(MAX_INSTANCES - P, fill)]).astype(dt)  # noqa: E731
  pred = dict(instance=pinst, inst_class=pad(pcls, -1, np.int32), inst_scene=pad(pscene, -1, np.int32),
              inst_score=pad(brng.random(P), 0.0, np.float64), inst_size=pad(np.bincount(pinst[pinst >= 0], minlength=P), 0, np.int32),
              scene_offsets=offs)
  pred = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in pred.items()}
  gi, gc = torch.from_numpy(inst).to(dev), torch.from_numpy(cls).to(dev)
  gi32, gc32 = gi.to(torch.int32), gc.to(torch.int32)

  def step(module, name, table):
    def run():
      e = getattr(module, name)(CLASSES)
      e.step(pred, gi, gc, Ge, **(dict(table=PF.instance_table(gi32, gc32, None, pred["scene_offsets"], Ge)) if table else {}))
      return e
    return run

  variants = dict(voc_step=step(iseg, "InstanceEvaluator", False), voc_step_table=step(iseg, "InstanceEvaluator", True),
                  bench_step=step(iseg, "InstanceBenchmarkEvaluator", False), bench_step_table=step(iseg, "InstanceBenchmarkEvaluator", True),
                  instance_table_cls_scene=lambda: PF.instance_table(gi32, gc32, None, pred["scene_offsets"], Ge))
  if a.parent:
    parent = load_parent(a.parent)
    variants.update(parent_voc_step=step(parent, "InstanceEvaluator", False), parent_bench_step=step(parent, "InstanceBenchmarkEvaluator", False))
  res["evaluator"] = dict(rows=len(coords), instances=Ge, predictions=P, slots=MAX_INSTANCES, device_ms=timed(variants, a.runs))
  same = []
  for name in ("InstanceEvaluator", "InstanceBenchmarkEvaluator"):
    m0, m1 = step(iseg, name, False)().compute_metrics(), step(iseg, name, True)().compute_metrics()
    same.append(all(np.array_equal(np.atleast_1d(m0[k]).view(np.uint8), np.atleast_1d(m1[k]).view(np.uint8)) for k in m0))
  res["evaluator"]["table_metrics_identical"] = bool(all(same))
  print(json.dumps(res))


if __name__ == "__main__":
  main()
