"""Generates tests/golden/golden_votenet.npz by running the REFERENCE'S OWN detection-head functions on small seeded inputs.

Run from the repo root where the reference tree is present:
    python tests/golden/make_golden_votenet.py

What runs, imported unmodified from downstream/votenet_det_new/lib/utils of the reference: nn_distance.py (nn_distance,
huber_loss), box_util.py (get_3d_box) and nms.py (nms_2d_faster, nms_3d_faster, nms_3d_faster_samecls; its `pc_util` import
is served by an empty stand-in, because the real module exits at import without plyfile and the three functions never call
the name taken from it).  The file holds arrays only -- inputs and what those functions returned -- so that
tests/test_votenet_ref.py and tests/test_gpu_votenet_head.py also run where the reference is absent.
"""
import os
import sys
import types

import numpy as np
import torch

REF_UTILS = "/root/reference/downstream/votenet_det_new/lib/utils"
HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden_votenet.npz")
NMS_IOU = 0.25
NUM_HEADING_BIN = 12


def reference_available():
  return os.path.isfile(os.path.join(REF_UTILS, "nn_distance.py"))


def import_reference():
  """(nn_distance module, box_util module, nms module) of the reference."""
  assert reference_available(), "%s is not present" % REF_UTILS
  saved = {k: sys.modules.get(k) for k in ("pc_util", "nn_distance", "box_util", "nms")}
  stub = types.ModuleType("pc_util")
  stub.bbox_corner_dist_measure = None  # imported by name, called by none of the functions used here
  sys.modules["pc_util"] = stub
  sys.path.insert(0, REF_UTILS)
  try:
    for k in ("nn_distance", "box_util", "nms"):
      sys.modules.pop(k, None)
    import nn_distance as nd
    import box_util as bu
    import nms as nm
    return nd, bu, nm
  finally:
    sys.path.remove(REF_UTILS)
    for k, v in saved.items():
      if v is None:
        sys.modules.pop(k, None)
      else:
        sys.modules[k] = v


def clustered_boxes(rng, K, n_clusters):
  """[K, 6] (min xyz, max xyz) boxes jittered around n_clusters centres, so that many overlap."""
  cen = rng.uniform(-3, 3, (n_clusters, 3))
  c = cen[rng.randint(0, n_clusters, K)] + rng.normal(0, 0.15, (K, 3))
  half = rng.uniform(0.3, 0.6, (K, 3))
  return np.concatenate([c - half, c + half], 1)


def make_inputs():
  rng = np.random.RandomState(20261017)
  out = {}
  out["nn_pc1"] = rng.uniform(-1, 1, (2, 7, 3)).astype(np.float32) * 2
  out["nn_pc2"] = rng.uniform(-1, 1, (2, 5, 3)).astype(np.float32) * 2
  out["huber_in"] = np.linspace(-3, 3, 25).astype(np.float32)
  out["box_size"] = rng.uniform(0.2, 2.0, (6, 3))
  out["box_angle"] = np.array([0.0, 0.3, -1.2, 3.0, -3.1, 1.5707963])
  out["box_center"] = rng.uniform(-2, 2, (6, 3))
  K = 24
  out["nms_boxes"] = clustered_boxes(rng, K, 5)
  out["nms_score"] = rng.permutation(K).astype(np.float64) / K + 0.01
  out["nms_cls"] = rng.randint(0, 3, K).astype(np.float64)
  # one parse_predictions case: B = 1, K = 16, SUN RGB-D style heading bins
  Kp, H, S, Cls = 16, NUM_HEADING_BIN, 4, 4
  cen = rng.uniform(-1, 1, (3, 3))
  out["pp_center"] = (cen[rng.randint(0, 3, Kp)] + rng.normal(0, 0.1, (Kp, 3)))[None].astype(np.float32)
  out["pp_heading_scores"] = rng.normal(0, 1, (1, Kp, H)).astype(np.float32)
  out["pp_heading_residuals"] = rng.uniform(-0.2, 0.2, (1, Kp, H)).astype(np.float32)
  out["pp_size_scores"] = rng.normal(0, 1, (1, Kp, S)).astype(np.float32)
  out["pp_size_residuals"] = rng.uniform(-0.1, 0.1, (1, Kp, S, 3)).astype(np.float32)
  out["pp_sem_cls_scores"] = rng.normal(0, 1, (1, Kp, Cls)).astype(np.float32)
  out["pp_objectness_scores"] = rng.normal(0, 2, (1, Kp, 2)).astype(np.float32)
  out["pp_mean_size_arr"] = rng.uniform(0.5, 1.2, (S, 3)).astype(np.float32)
  return out


def run_reference(inp):
  nd, bu, nm = import_reference()
  out = {}
  p1, p2 = torch.from_numpy(inp["nn_pc1"]), torch.from_numpy(inp["nn_pc2"])
  for name, kw in (("l2", {}), ("l1", dict(l1=True)), ("huber", dict(l1smooth=True, delta=0.75))):
    d1, i1, d2, i2 = nd.nn_distance(p1, p2, **kw)
    out["nn_%s_dist1" % name], out["nn_%s_idx1" % name] = d1.numpy(), i1.numpy()
    out["nn_%s_dist2" % name], out["nn_%s_idx2" % name] = d2.numpy(), i2.numpy()
  out["huber_out"] = nd.huber_loss(torch.from_numpy(inp["huber_in"]), delta=0.75).numpy()
  out["box_corners"] = np.stack([bu.get_3d_box(inp["box_size"][k], inp["box_angle"][k], inp["box_center"][k]) for k in range(6)])
  b, s, c = inp["nms_boxes"], inp["nms_score"], inp["nms_cls"]
  K = b.shape[0]
  for old in (0, 1):
    for name, pick in (("2d", nm.nms_2d_faster(np.stack([b[:, 0], b[:, 2], b[:, 3], b[:, 5], s], 1), NMS_IOU, bool(old))),
                       ("3d", nm.nms_3d_faster(np.concatenate([b, s[:, None]], 1), NMS_IOU, bool(old))),
                       ("3dcls", nm.nms_3d_faster_samecls(np.concatenate([b, s[:, None], c[:, None]], 1), NMS_IOU, bool(old)))):
      mask = np.zeros(K, np.int64)
      mask[np.asarray(pick, np.int64)] = 1
      out["nms_%s_old%d" % (name, old)] = mask
  # the parse case, as ap_helper.parse_predictions strings the reference's functions together (3D NMS, nothing removed)
  hs, ss = inp["pp_heading_scores"][0], inp["pp_size_scores"][0]
  Kp = hs.shape[0]
  corners = np.zeros((Kp, 8, 3))
  for j in range(Kp):
    hc, sc = int(np.argmax(hs[j])), int(np.argmax(ss[j]))
    angle = hc * (2 * np.pi / NUM_HEADING_BIN) + float(inp["pp_heading_residuals"][0, j, hc])  # model_util_sunrgbd.class2angle
    if angle > np.pi:
      angle = angle - 2 * np.pi
    size = inp["pp_mean_size_arr"][sc].astype(np.float64) + inp["pp_size_residuals"][0, j, sc]
    cen = inp["pp_center"][0, j]
    corners[j] = bu.get_3d_box(size, angle, np.array([cen[0], -cen[2], cen[1]], np.float64))
  o = inp["pp_objectness_scores"][0].astype(np.float32)
  e = np.exp(o - o.max(-1, keepdims=True))
  prob = (e / e.sum(-1, keepdims=True))[:, 1]
  boxes = np.concatenate([corners.min(1), corners.max(1), prob[:, None]], 1)
  mask = np.zeros(Kp, np.int64)
  mask[np.asarray(nm.nms_3d_faster(boxes, NMS_IOU, False), np.int64)] = 1
  out["pp_corners"], out["pp_obj_prob"], out["pp_pred_mask"] = corners[None], prob[None], mask[None]
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
