"""Generates tests/golden/golden_ap.npz by running the REFERENCE'S OWN detection scoring on small seeded inputs.

Run from the repo root where the reference tree is present:
    python tests/golden/make_golden_ap.py

What runs, imported unmodified from downstream/votenet_det_new/lib/utils of the reference: box_util.py (box3d_iou, get_3d_box)
and eval_det.py (eval_det_cls, eval_det, with its get_iou_obb).  eval_det.py imports lib.utils.metric_util, which imports
trimesh; an empty stand-in module serves that import, because none of the functions used here reaches it.  The file holds
arrays only -- the inputs, what those functions returned, and the true-positive flags of tests/ap_ref.py cross-checked
through the reference's rec / prec -- so that tests/test_ap_ref.py and tests/test_gpu_ap.py also run where the reference is
absent.  The seeded input builders below are shared with those tests.
"""
import contextlib
import io
import os
import sys
import types

import numpy as np

REF_ROOT = "/root/reference/downstream/votenet_det_new"
HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden_ap.npz")
sys.path.insert(0, os.path.dirname(HERE))
import ap_ref as A  # noqa: E402

THRESHOLDS = (0.25, 0.5)
N_HEADINGS = 7  # headings are k pi / 7 - 3 pi / 7: two boxes are parallel exactly or at least pi / 7 apart, never near pi / 2
CLASS_IDS = (3, 7, 11, 20)


def reference_available():
  return os.path.isfile(os.path.join(REF_ROOT, "lib", "utils", "eval_det.py"))


def import_reference():
  """(box_util module, eval_det module) of the reference."""
  assert reference_available(), "%s is not present" % REF_ROOT
  names = ("trimesh", "lib", "lib.utils", "lib.utils.metric_util", "lib.utils.box_util", "lib.utils.eval_det")
  saved = {k: sys.modules.get(k) for k in names}
  for k in names:
    sys.modules.pop(k, None)
  if saved["trimesh"] is None:
    sys.modules["trimesh"] = types.ModuleType("trimesh")
  else:
    sys.modules["trimesh"] = saved["trimesh"]
  sys.path.insert(0, REF_ROOT)
  try:
    import lib.utils.box_util as bu
    import lib.utils.eval_det as ed
    return bu, ed
  finally:
    sys.path.remove(REF_ROOT)
    for k, v in saved.items():
      if v is None:
        sys.modules.pop(k, None)
      else:
        sys.modules[k] = v


def heading_of(index):
  return np.asarray(index, np.float64) * (np.pi / N_HEADINGS) - 3 * np.pi / N_HEADINGS


def corners32(size, angle, center):
  return A.box_corners(size, angle, center).astype(np.float32)


def random_boxes(rng, n, spread=1.2, lo=0.4, hi=1.4):
  """(corners float32 [n, 8, 3], heading [n]) of n boxes crowded into a small volume, so that most pairs overlap."""
  h = heading_of(rng.randint(0, N_HEADINGS, n))
  c = np.stack([corners32(rng.uniform(lo, hi, 3), h[i], rng.uniform(-spread, spread, 3) * (1, 0.3, 1)) for i in range(n)]) if n else \
      np.zeros((0, 8, 3), np.float32)
  return c, h


def clear_boxes(rng, n, others, spread=3.0, margin=1e-3):
  """n boxes as random_boxes draws them, each redrawn until its overlaps with the boxes `others` [m, 8, 3] are either 0 or at
  least `margin` away from 0 and from one another: whatever classes the others get, no best overlap has a close runner-up.
  Returns (corners float32 [n, 8, 3], heading [n], iou3d [n, m], iou2d [n, m])."""
  boxes, heads, rows3, rows2 = [], [], [], []
  while len(boxes) < n:
    c, h = random_boxes(rng, 1, spread)
    o3, o2 = A.iou_matrix(c, others)
    v = np.sort(o3[0][o3[0] > 0])
    if v.size and (v[0] < margin or (np.diff(v) < margin).any()):
      continue
    boxes.append(c[0]); heads.append(h[0]); rows3.append(o3[0]); rows2.append(o2[0])
  return np.stack(boxes), np.array(heads), np.stack(rows3), np.stack(rows2)


def special_pairs():
  """[(name, corners1, corners2)]: the hand-made overlap cases; sizes and centres are exact in float32."""
  unit = (1.0, 1.0, 1.0)
  cases = [
      ("identical", (unit, 0.0, (0.5, 0.25, -1.0)), (unit, 0.0, (0.5, 0.25, -1.0))),
      ("disjoint", (unit, 0.0, (0, 0, 0)), (unit, 0.0, (3, 0, 0))),
      ("shared_face_x", (unit, 0.0, (0, 0, 0)), (unit, 0.0, (1, 0, 0))),
      ("shared_face_z", (unit, 0.0, (0, 0, 0)), ((1.0, 2.0, 1.0), 0.0, (0, 0, 1.5))),
      ("inside", ((2.0, 3.0, 2.0), 0.0, (0, 0, 0)), ((0.5, 1.0, 0.5), 0.0, (0.25, 0.25, -0.5))),
      ("inside_rotated", ((2.0, 3.0, 2.0), 0.3, (0, 0, 0)), ((0.5, 0.75, 0.5), 1.1, (0.125, 0.25, -0.25))),
      ("octagon", ((2.0, 2.0, 1.0), 0.0, (0, 0, 0)), ((2.0, 2.0, 1.0), np.pi / 4, (0, 0, 0))),
      ("heading_pi", ((2.0, 1.0, 1.0), np.pi, (0.25, 0, 0.125)), ((1.5, 1.25, 1.0), 0.0, (0, 0, 0))),
      ("heading_minus_pi", ((2.0, 1.0, 1.0), -np.pi, (0.25, 0, 0.125)), ((1.5, 1.25, 1.0), 0.0, (0, 0, 0))),
      ("heading_half_pi", ((2.0, 1.0, 1.0), np.pi / 2, (0.25, 0, 0.125)), ((1.5, 1.25, 1.0), 0.0, (0, 0, 0))),
      ("bev_only", (unit, 0.3, (0, 0, 0)), (unit, 0.9, (0.25, 2.0, 0.125))),
      ("small_in_large", ((0.05, 0.05, 0.05), 0.4, (1.0, 0.5, -2.0)), ((5.0, 5.0, 5.0), 1.0, (0.5, 0, -1.0))),
      ("small_small_far", ((0.05, 0.05, 0.05), 0.4, (3.0, 0.5, -3.0)), ((0.05, 0.05, 0.05), 1.0, (3.015625, 0.5, -2.984375))),
      ("large_large", ((5.0, 4.0, 5.0), -0.7, (0, 0, 0)), ((5.0, 5.0, 3.0), 0.6, (1.0, 0.5, -1.0))),
  ]
  return [(n, corners32(*a), corners32(*b)) for n, a, b in cases]


def dataset(seed, n_scenes, class_ids=CLASS_IDS, max_gt=5, n_pred=12, tie_scores=False, gt_only_class=None, pred_only_class=None):
  """A seeded evaluation as flat arrays: pred_scene / pred_cls / pred_corners (float32) / pred_score / pred_heading and
  gt_scene / gt_cls / gt_corners (float32) / gt_heading.  Detections are jittered copies of ground-truth boxes (several per box,
  some of another class) and stray boxes; the first scene has no ground truth and the last no detection.  gt_only_class: a
  class that gets ground truth and no detection; pred_only_class: the reverse."""
  rng = np.random.RandomState(seed)
  P = dict(pred_scene=[], pred_cls=[], pred_corners=[], pred_score=[], pred_heading=[], gt_scene=[], gt_cls=[], gt_corners=[],
           gt_heading=[])
  for s in range(n_scenes):
    n_gt = 0 if s == 0 else rng.randint(1, max_gt + 1)
    gts = []
    for _ in range(n_gt):
      hi = rng.randint(0, N_HEADINGS)
      size, cen = rng.uniform(0.4, 1.4, 3), rng.uniform(-1.5, 1.5, 3) * (1, 0.3, 1)
      cls = class_ids[rng.randint(0, len(class_ids))]
      gts.append((cls, size, hi, cen))
      P["gt_scene"].append(s); P["gt_cls"].append(cls); P["gt_corners"].append(corners32(size, heading_of(hi), cen))
      P["gt_heading"].append(heading_of(hi))
    if gt_only_class is not None and s == 1:
      P["gt_scene"].append(s); P["gt_cls"].append(gt_only_class); P["gt_corners"].append(corners32((1, 1, 1), heading_of(2), (0.2, 0, 0.1)))
      P["gt_heading"].append(heading_of(2))
    if s == n_scenes - 1 and n_scenes > 1:
      continue
    for k in range(n_pred):
      if gts and rng.rand() < 0.75:
        cls, size, hi, cen = gts[rng.randint(0, len(gts))]
        size = size * rng.uniform(0.75, 1.25, 3)
        cen = cen + rng.normal(0, 0.12, 3)
        if rng.rand() < 0.3:
          hi = rng.randint(0, N_HEADINGS)
        if rng.rand() < 0.15:
          cls = class_ids[rng.randint(0, len(class_ids))]
      else:
        cls, size, hi, cen = class_ids[rng.randint(0, len(class_ids))], rng.uniform(0.4, 1.4, 3), rng.randint(0, N_HEADINGS), \
            rng.uniform(-1.5, 1.5, 3) * (1, 0.3, 1)
      if pred_only_class is not None and k == 0:
        cls = pred_only_class
      score = np.round(rng.rand(), 1) if tie_scores else rng.rand()
      P["pred_scene"].append(s); P["pred_cls"].append(cls); P["pred_corners"].append(corners32(size, heading_of(hi), cen))
      P["pred_score"].append(score); P["pred_heading"].append(heading_of(hi))
  out = {}
  for k, v in P.items():
    dt = np.float32 if k.endswith("corners") else (np.int64 if k.endswith(("scene", "cls")) else np.float64)
    out[k] = np.asarray(v, dt).reshape((-1, 8, 3) if k.endswith("corners") else (-1,))
  out["n_scenes"] = np.int64(n_scenes)
  return out


def to_maps(d):
  """The flat arrays as the dicts eval_det takes: ({scene: [(class, corners, score)]}, {scene: [(class, corners)]}), every
  scene present in both, corners float64."""
  n = int(d["n_scenes"])
  pred = {s: [] for s in range(n)}
  gt = {s: [] for s in range(n)}
  for s, c, box, sc in zip(d["pred_scene"], d["pred_cls"], d["pred_corners"], d["pred_score"]):
    pred[int(s)].append((int(c), box.astype(np.float64), float(sc)))
  for s, c, box in zip(d["gt_scene"], d["gt_cls"], d["gt_corners"]):
    gt[int(s)].append((int(c), box.astype(np.float64)))
  return pred, gt


def to_lists(d):
  """(batch_pred_map_cls, batch_gt_map_cls) as parse_predictions / parse_groundtruths return them."""
  pred, gt = to_maps(d)
  n = int(d["n_scenes"])
  return [pred[s] for s in range(n)], [gt[s] for s in range(n)]


GOLDEN_DATASET = dict(seed=2, n_scenes=7, pred_only_class=42)


def make_inputs():
  out = {}
  sp = special_pairs()
  out["sp_names"] = np.array([n for n, _, _ in sp])
  out["sp_c1"] = np.stack([a for _, a, _ in sp])
  out["sp_c2"] = np.stack([b for _, _, b in sp])
  rng = np.random.RandomState(20261017)
  out["iou_a"], out["iou_a_heading"] = random_boxes(rng, 13)
  out["iou_b"], out["iou_b_heading"] = random_boxes(rng, 11)
  for k, v in dataset(**GOLDEN_DATASET).items():
    out["ds_" + k] = v
  return out


def run_reference(inp):
  bu, ed = import_reference()
  out = {}
  sp = [bu.box3d_iou(a.astype(np.float64), b.astype(np.float64)) for a, b in zip(inp["sp_c1"], inp["sp_c2"])]
  out["sp_iou3d"], out["sp_iou2d"] = np.array([v[0] for v in sp]), np.array([v[1] for v in sp])
  a, b = inp["iou_a"].astype(np.float64), inp["iou_b"].astype(np.float64)
  both = np.array([[bu.box3d_iou(a[i], b[j]) for j in range(len(b))] for i in range(len(a))])
  out["iou3d"], out["iou2d"] = both[..., 0], both[..., 1]
  # get_3d_box against the corner builder the inputs were made with
  out["corners_check"] = bu.get_3d_box(np.array([1.2, 0.7, 0.9]), 0.37, np.array([0.3, -0.2, 1.1]))
  d = {k[3:]: v for k, v in inp.items() if k.startswith("ds_")}
  pred_all, gt_all = to_maps(d)
  for ti, t in enumerate(THRESHOLDS):
    for m in (0, 1):
      with contextlib.redirect_stdout(io.StringIO()), np.errstate(invalid="ignore", divide="ignore"):
        rec, prec, ap = ed.eval_det(pred_all, gt_all, ovthresh=t, use_07_metric=bool(m), get_iou_func=ed.get_iou_obb)
      classes = sorted(ap)
      mine = A.eval_det(pred_all, gt_all, t, bool(m))
      out["classes"] = np.asarray(classes, np.int64)
      out["ap_t%d_m%d" % (ti, m)] = np.array([ap[c] for c in classes], np.float64)
      if m == 0:
        out["rec_t%d" % ti] = np.concatenate([rec[c] for c in classes])
        out["prec_t%d" % ti] = np.concatenate([prec[c] for c in classes])
        out["curve_offs"] = np.cumsum([0] + [len(rec[c]) for c in classes])
        flags = []
        for c in classes:
          tp = mine[c]["tp"]
          if mine[c]["npos"] > 0:  # the flags through the reference's own curves: tp = cumulative recall x npos, tp + fp = rank
            assert np.array_equal(np.rint(rec[c] * mine[c]["npos"]).astype(np.int64), np.cumsum(tp)), c
          assert np.allclose(prec[c], np.cumsum(tp) / np.arange(1, len(tp) + 1), rtol=0, atol=1e-12), c
          flags.append(tp)
        out["tp_t%d" % ti] = np.concatenate(flags)
        # the metrics dict as APCalculator.compute_metrics builds it from these values (ap_helper.py:256-271)
        keys = ["%d Average Precision" % c for c in classes] + ["mAP"] + ["%d Recall" % c for c in classes] + ["AR"]
        last = [rec[c][-1] if len(rec[c]) else 0 for c in classes]
        vals = [ap[c] for c in classes] + [np.mean(list(ap.values()))] + last + [np.mean(last)]
        out["metric_keys"] = np.array(keys)
        out["metric_vals_t%d" % ti] = np.asarray(vals, np.float64)
  # one class on its own through eval_det_cls
  pred, gt = A.split_classes(pred_all, gt_all)
  c = CLASS_IDS[0]
  with np.errstate(invalid="ignore", divide="ignore"):
    r, p, a1 = ed.eval_det_cls(pred[c], gt[c], ovthresh=0.25, use_07_metric=False, get_iou_func=ed.get_iou_obb)
  out["cls_rec"], out["cls_prec"], out["cls_ap"] = r, p, np.float64(a1)
  return out


def generate():
  inp = make_inputs()
  out = run_reference(inp)
  out.update(inp)
  return out


def main():
  out = generate()
  np.savez_compressed(PATH, **out)
  print(PATH, os.path.getsize(PATH), sorted(out))


if __name__ == "__main__":
  main()
