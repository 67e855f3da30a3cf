"""tests/ap_ref.py -- the float64 restatement the detection-scoring kernels are held to -- against what the reference's own
box3d_iou, eval_det_cls and eval_det returned (tests/golden/golden_ap.npz, written by tests/golden/make_golden_ap.py): overlaps
and AP to 1e-12, true-positive flags exactly.  Where the reference tree is present the golden arrays are regenerated live and
compared with the committed file."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import ap_ref as A  # noqa: E402
import make_golden_ap as mk  # noqa: E402

G = np.load(mk.PATH)
TOL = 1e-12


def _dataset():
  return {k[3:]: G[k] for k in G.files if k.startswith("ds_")}


def test_inputs_are_the_seeded_ones():
  inp = mk.make_inputs()
  for k, v in inp.items():
    assert np.array_equal(G[k], v), k


def test_corner_builder_matches_get_3d_box():
  got = A.box_corners(np.array([1.2, 0.7, 0.9]), 0.37, np.array([0.3, -0.2, 1.1]))
  assert np.abs(got - G["corners_check"]).max() <= 1e-15


def test_special_overlaps():
  names = list(G["sp_names"])
  for i, n in enumerate(names):
    o3, o2 = A.box3d_iou(G["sp_c1"][i], G["sp_c2"][i])
    assert abs(o3 - G["sp_iou3d"][i]) <= TOL and abs(o2 - G["sp_iou2d"][i]) <= TOL, n
  ref = dict(zip(names, G["sp_iou3d"]))
  assert abs(ref["identical"] - 1) <= 1e-12
  assert ref["disjoint"] == 0 and ref["shared_face_x"] == 0 and ref["shared_face_z"] == 0 and ref["bev_only"] == 0
  assert G["sp_iou2d"][names.index("bev_only")] > 0.1
  assert abs(ref["inside"] - (0.5 * 0.5 * 1.0) / (2 * 2 * 3)) <= 1e-12
  # a 2 x 2 square against itself turned by 45 degrees: the regular octagon of area 8 (sqrt(2) - 1)
  oct_area = 8 * (np.sqrt(2) - 1)
  assert abs(G["sp_iou2d"][names.index("octagon")] - oct_area / (8 - oct_area)) <= 1e-12
  for i, n in enumerate(names):
    got = A.box3d_iou(G["sp_c1"][i], G["sp_c2"][i])[0]
    if G["sp_iou3d"][i] == 0:
      assert got == 0, n


def test_overlap_matrix():
  o3, o2 = A.iou_matrix(G["iou_a"], G["iou_b"])
  assert np.abs(o3 - G["iou3d"]).max() <= TOL and np.abs(o2 - G["iou2d"]).max() <= TOL
  assert (G["iou3d"] > 0.05).mean() > 0.2, "the seeded boxes should mostly overlap"
  A.assert_headings_clear(G["iou_a_heading"], G["iou_b_heading"], "golden matrix")


@pytest.mark.parametrize("ti", range(len(mk.THRESHOLDS)))
def test_eval_det(ti):
  pred_all, gt_all = mk.to_maps(_dataset())
  classes = [int(c) for c in G["classes"]]
  offs = G["curve_offs"]
  for m in (0, 1):
    res = A.eval_det(pred_all, gt_all, mk.THRESHOLDS[ti], bool(m))
    assert sorted(res) == classes
    want = G["ap_t%d_m%d" % (ti, m)]
    for k, c in enumerate(classes):
      assert (np.isnan(want[k]) and np.isnan(res[c]["ap"])) or abs(res[c]["ap"] - want[k]) <= TOL, (c, m)
      sl = slice(offs[k], offs[k + 1])
      assert np.array_equal(res[c]["tp"], G["tp_t%d" % ti][sl]), c
      assert np.allclose(res[c]["rec"], G["rec_t%d" % ti][sl], rtol=0, atol=TOL, equal_nan=True), c
      assert np.allclose(res[c]["prec"], G["prec_t%d" % ti][sl], rtol=0, atol=TOL, equal_nan=True), c
  res = A.eval_det(pred_all, gt_all, mk.THRESHOLDS[ti])
  got = A.metrics(res)
  assert list(got) == list(G["metric_keys"])
  assert np.allclose(np.array(list(got.values()), np.float64), G["metric_vals_t%d" % ti], rtol=0, atol=TOL, equal_nan=True)
  assert np.isnan(got["42 Average Precision"]) and np.isnan(got["mAP"])  # detections of a class without ground truth


def test_single_class():
  pred_all, gt_all = mk.to_maps(_dataset())
  pred, gt = A.split_classes(pred_all, gt_all)
  c = mk.CLASS_IDS[0]
  r = A.eval_class(pred[c], gt[c], 0.25)
  assert np.allclose(r["rec"], G["cls_rec"], rtol=0, atol=TOL) and np.allclose(r["prec"], G["cls_prec"], rtol=0, atol=TOL)
  assert abs(r["ap"] - float(G["cls_ap"])) <= TOL


def test_golden_dataset_is_clear_of_the_thresholds():
  d = _dataset()
  A.assert_headings_clear(d["pred_heading"], d["gt_heading"], "golden dataset")
  A.assert_results_clear(A.eval_det(*mk.to_maps(d), 0.25), mk.THRESHOLDS, "golden dataset")
  assert len(np.unique(d["pred_score"])) == len(d["pred_score"]), "numpy's argsort leaves equal confidences unspecified"


def test_class_without_detections_scores_zero():
  d = mk.dataset(seed=3, n_scenes=3, gt_only_class=99)
  res = A.eval_det(*mk.to_maps(d), 0.25)
  assert res[99]["ap"] == 0 and len(res[99]["rec"]) == 0 and res[99]["npos"] == 1
  m = A.metrics(res)
  assert m["99 Average Precision"] == 0 and m["99 Recall"] == 0


def test_voc_ap_forms():
  rec, prec = np.array([0.0, 0.5, 0.5, 1.0]), np.array([0.0, 0.5, 1 / 3, 0.5])
  assert abs(A.voc_ap(rec, prec) - 0.5) <= 1e-15
  assert abs(A.voc_ap(rec, prec, True) - 0.5) <= 1e-15
  assert A.voc_ap(np.zeros(0), np.zeros(0)) == 0 and A.voc_ap(np.zeros(0), np.zeros(0), True) == 0


@pytest.mark.skipif(not mk.reference_available(), reason="the reference tree is not present")
def test_golden_file_is_current():
  with np.errstate(all="ignore"):
    live = mk.generate()
  assert sorted(live) == sorted(G.files)
  for k, v in live.items():
    v = np.asarray(v)
    if v.dtype.kind in "fc":
      assert np.allclose(G[k], v, rtol=0, atol=1e-12, equal_nan=True), k
    else:
      assert np.array_equal(G[k], v), k
