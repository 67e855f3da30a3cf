"""The detection scoring (csrc/evaldet.hip, pointcontrast_amd.downstream.votenet.APCalculator) on the MI355X against the
reference's recorded outputs (tests/golden/golden_ap.npz) and tests/ap_ref.py.

Tolerances: overlaps within 1e-4 absolute (the project's bound; the largest entry is 1); AP and recall within 1e-10 of float64
(they are float64 sums of at most nd + 2 terms <= 1 on integer counts: nd 2^-53 is far below that for the sizes here); best_gt
and the true-positive flags exactly.  Where a float32 overlap could decide differently from float64 the tests first assert on
the host that the inputs stay clear: headings parallel exactly or >= 0.05 (in |sin| and |cos|) apart, every best overlap
1e-3 away from the thresholds and from its runner-up, best_gt compared only where the best overlap exceeds 1e-3."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import ap_ref as A  # noqa: E402
import make_golden_ap as mk  # noqa: E402
import votenet_fixtures as VF  # noqa: E402
import votenet_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL, TOL_AP = 1e-4, 1e-10
G = np.load(mk.PATH)
PCMI_ERR_INVALID, PCMI_ERR_UNSUPPORTED, PCMI_ERR_WORKSPACE = -1, -6, -7
THRESHOLDS = list(mk.THRESHOLDS)
AP_BLOCK = 1024  # kApChunk of evaldet.hip: the detections one pass of the scan's workgroup covers


def _dev(a, dtype=None):
  t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
  return t if dtype is None else t.to(dtype)


def _p(t):
  return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
  return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


_POOL = {}


def pool():
  """65 x 65 boxes with their float64 overlaps, computed once: a [65] against b [65]; every row's overlaps are 0 or 1e-3 clear
  of 0 and of one another."""
  if not _POOL:
    rng = np.random.RandomState(5)
    b, hb = mk.random_boxes(rng, 65, spread=3.0)
    a, ha, o3, o2 = mk.clear_boxes(rng, 65, b)
    A.assert_headings_clear(ha, hb, "pool")
    assert (o3 > 0.25).sum() >= 10 and (o3 == 0).mean() > 0.5
    _POOL.update(a=a, b=b, o3=o3, o2=o2)
  return _POOL


# ---- 1. overlaps ----------------------------------------------------------------------------------------------------------------
def test_special_overlaps():
  from pointcontrast_amd import functional as PF
  names = list(G["sp_names"])
  for i, n in enumerate(names):
    o3, o2 = PF.box3d_iou(_dev(G["sp_c1"][i:i + 1]), _dev(G["sp_c2"][i:i + 1]))
    o3, o2 = float(o3[0, 0]), float(o2[0, 0])
    print("%s: %.9g (reference %.9g), 2D %.9g (%.9g)" % (n, o3, G["sp_iou3d"][i], o2, G["sp_iou2d"][i]))
    assert abs(o3 - G["sp_iou3d"][i]) <= TOL and abs(o2 - G["sp_iou2d"][i]) <= TOL, n
    if G["sp_iou3d"][i] == 0:
      assert o3 == 0.0, n
    if G["sp_iou2d"][i] == 0:
      assert o2 == 0.0, n
  # all of them in one launch, and the pairs the other way round
  o3, _ = PF.box3d_iou(_dev(G["sp_c1"]), _dev(G["sp_c2"]))
  assert np.abs(np.diag(o3.cpu().numpy()) - G["sp_iou3d"]).max() <= TOL
  o3t, _ = PF.box3d_iou(_dev(G["sp_c2"]), _dev(G["sp_c1"]))
  assert np.abs(np.diag(o3t.cpu().numpy()) - G["sp_iou3d"]).max() <= TOL


def test_overlap_matrix_against_the_reference():
  from pointcontrast_amd import functional as PF
  A.assert_headings_clear(G["iou_a_heading"], G["iou_b_heading"], "golden matrix")
  o3, o2 = PF.box3d_iou(_dev(G["iou_a"]), _dev(G["iou_b"]))
  e3, e2 = np.abs(o3.cpu().numpy() - G["iou3d"]).max(), np.abs(o2.cpu().numpy() - G["iou2d"]).max()
  print("max error %.3g (3D), %.3g (2D)" % (e3, e2))
  assert e3 <= TOL and e2 <= TOL
  assert np.array_equal(o3.cpu().numpy() == 0, G["iou3d"] == 0)
  only3, none = PF.box3d_iou(_dev(G["iou_a"]), _dev(G["iou_b"]), with_2d=False)
  assert none is None and torch.equal(only3, o3)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_overlap_matrix_shapes(n):
  from pointcontrast_amd import functional as PF
  P = pool()
  # the kernel takes the flat [n m] list in workgroups of 256 pairs: 1 x 255 / 256 / 257 sit on that edge
  for m in (1, 63, 64, 65, 257) + ((255, 256) if n == 1 else ()):
    ia, ib = (np.arange(n) * 7) % 65, (np.arange(m) * 3 + 1) % 65
    o3, o2 = PF.box3d_iou(_dev(P["a"][ia]), _dev(P["b"][ib]))
    assert o3.shape == (n, m) and o2.shape == (n, m)
    assert np.abs(o3.cpu().numpy() - P["o3"][np.ix_(ia, ib)]).max() <= TOL, (n, m)
    assert np.abs(o2.cpu().numpy() - P["o2"][np.ix_(ia, ib)]).max() <= TOL, (n, m)
  e = torch.zeros((0, 8, 3), device=DEV)
  assert PF.box3d_iou(e, _dev(P["b"]))[0].shape == (0, 65) and PF.box3d_iou(_dev(P["a"]), e)[0].shape == (65, 0)


# ---- 2. matching ----------------------------------------------------------------------------------------------------------------
def _match_case(K, G_, Cls, seed, B=3):
  """Scenes of K boxes of pool a against G_ distinct boxes of pool b; scene 1 has every box masked out, and with 18 classes
  some class has no box in a scene."""
  rng = np.random.RandomState(seed)
  P = pool()
  ik = rng.randint(0, 65, (B, K))
  ig = np.stack([rng.permutation(65)[:G_] for _ in range(B)]) if G_ else np.zeros((B, 0), np.int64)
  cls = rng.randint(0, Cls, (B, G_))
  mask = rng.rand(B, G_) > 0.2
  if B > 1:
    mask[1] = False
  return ik, ig, cls, mask, P


@pytest.mark.parametrize("Cls", [1, 18])
@pytest.mark.parametrize("K,G_", [(1, 0), (1, 1), (1, 64), (256, 0), (256, 1), (256, 64), (1024, 64), (33, 7)])
def test_det_match(K, G_, Cls):
  from pointcontrast_amd import functional as PF
  ik, ig, cls, mask, P = _match_case(K, G_, Cls, 100 * K + G_ + Cls)
  B = ik.shape[0]
  best_gt, best_iou = PF.det_match(_dev(P["a"][ik]), _dev(P["b"][ig].reshape(B, G_, 8, 3)), _dev(cls), _dev(mask), Cls)
  assert best_gt.shape == (B, K, Cls) and best_gt.dtype == torch.int32 and best_iou.dtype == torch.float32
  bg, bo = best_gt.cpu().numpy(), best_iou.cpu().numpy()
  compared = 0
  for b in range(B):
    iou = P["o3"][np.ix_(ik[b], ig[b])] if G_ else np.zeros((K, 0))
    wg, wo, sec = A.match(iou, cls[b], mask[b], Cls)
    fin = np.isfinite(wo) & np.isfinite(sec) & ~((wo == 0) & (sec == 0))
    assert (wo[fin] - sec[fin] >= 1e-3).all(), "a runner-up within 1e-3 of the best overlap"
    none = wg < 0
    assert np.array_equal(bg[b] < 0, none) and (bg[b][none] == -1).all() and np.isneginf(bo[b][none]).all()
    assert np.abs(bo[b][~none] - wo[~none]).max(initial=0) <= TOL
    sure = wo > 1e-3
    assert np.array_equal(bg[b][sure], wg[sure])
    compared += int(sure.sum())
    if Cls == 18 and G_ == 7 and b != 1:
      assert none.all(axis=0).any(), "7 boxes cannot cover 18 classes: some class has no box in the scene"
  if B > 1:
    assert (bg[1] == -1).all(), "every box of scene 1 is masked out"
  if G_ == 64 and K >= 256:
    assert compared > 0
  again = PF.det_match(_dev(P["a"][ik]), _dev(P["b"][ig].reshape(B, G_, 8, 3)), _dev(cls), _dev(mask), Cls)
  assert torch.equal(again[0], best_gt) and torch.equal(again[1], best_iou)


def test_det_match_lowest_index_of_identical_boxes_and_limits():
  from pointcontrast_amd import functional as PF
  from pointcontrast_amd._lib import PcmiError
  P = pool()
  k = int(np.argmax(P["o3"].max(1)))
  g = int(np.argmax(P["o3"][k]))
  other = int(np.argmin(P["o3"][k]))
  gt = np.stack([P["b"][other], P["b"][g], P["b"][g], P["b"][g]])[None]  # boxes 1, 2, 3 are bit-identical
  best_gt, best_iou = PF.det_match(_dev(P["a"][k][None, None]), _dev(gt), _dev(np.array([[0, 0, 0, 1]])), _dev(np.ones((1, 4), bool)), 2)
  assert best_gt.cpu().tolist() == [[[1, 3]]]
  assert abs(float(best_iou[0, 0, 0]) - P["o3"][k, g]) <= TOL and float(best_iou[0, 0, 0]) == float(best_iou[0, 0, 1])
  # a scene without any box of class 1, and a class id outside [0, Cls) counts as no box
  best_gt, _ = PF.det_match(_dev(P["a"][k][None, None]), _dev(gt), _dev(np.array([[0, 0, 0, 5]])), _dev(np.ones((1, 4), bool)), 2)
  assert best_gt.cpu().tolist() == [[[1, -1]]]
  z = lambda *s: torch.zeros(s, device=DEV)  # noqa: E731
  with pytest.raises(PcmiError, match="at most"):
    PF.det_match(z(1, 1025, 8, 3), z(1, 4, 8, 3), z(1, 4), z(1, 4), 2)
  with pytest.raises(PcmiError, match="at most"):
    PF.det_match(z(1, 4, 8, 3), z(1, 257, 8, 3), z(1, 257), z(1, 257), 2)
  PF.det_match(z(1, 1024, 8, 3), z(1, 256, 8, 3), z(1, 256), z(1, 256), 2)  # the limits themselves


# ---- 3. true positives, curves, AP ------------------------------------------------------------------------------------------------
def _ap_case(counts, npos, seed, kind="random"):
  """Per class `counts` detections with a best overlap and a box among the class's npos boxes (flat, class by class)."""
  rng = np.random.RandomState(seed)
  iou, gid, offs, base = [], [], [0], 0
  for n, g in zip(counts, npos):
    if kind == "all_tp":
      o, i = np.full(n, 0.9), (np.arange(n) if g >= n else rng.randint(0, max(g, 1), n))
    elif kind == "all_fp":
      o, i = np.full(n, 0.1), rng.randint(0, max(g, 1), n)
    elif kind == "duplicates":
      o, i = rng.uniform(0.6, 0.9, n), np.zeros(n, np.int64)
    else:
      o = rng.choice([0.0, 0.1, 0.2, 0.3, 0.4, 0.6, 0.8], n) + rng.uniform(0.01, 0.04, n)  # clear of 0.25 and 0.5
      i = rng.randint(0, max(g, 1), n)
    i = np.where((g > 0) & (rng.rand(n) > 0.1 if kind == "random" else True), base + i, -1)
    o = np.where(i >= 0, o, -np.inf)
    iou.append(o); gid.append(i); offs.append(offs[-1] + n); base += g
  return np.concatenate(iou).astype(np.float32), np.concatenate(gid).astype(np.int64), np.array(offs), np.array(npos), base


def _check_ap(case, thresholds, use_07, what):
  from pointcontrast_amd import functional as PF
  iou, gid, offs, npos, n_gt = case
  out = PF.det_ap(_dev(iou), _dev(gid), _dev(offs), _dev(npos), n_gt, thresholds, use_07, curves=True)
  got = {k: v.cpu().numpy() for k, v in out.items()}
  for t, thr in enumerate(thresholds):
    for c in range(len(npos)):
      sl = slice(offs[c], offs[c + 1])
      tp = A.flags_from_matches(iou[sl].astype(np.float64), gid[sl], thr)
      rec, prec = A.curves(tp, npos[c])
      with np.errstate(invalid="ignore"):
        ap = A.voc_ap(rec, prec, use_07)
      assert np.array_equal(got["tp"][t, sl], tp), (what, thr, c)
      assert np.allclose(got["rec"][t, sl], rec, rtol=0, atol=TOL_AP, equal_nan=True), (what, thr, c)
      assert np.allclose(got["prec"][t, sl], prec, rtol=0, atol=TOL_AP), (what, thr, c)
      last = rec[-1] if len(rec) else 0.0
      assert np.isclose(got["last_rec"][t, c], last, rtol=0, atol=TOL_AP, equal_nan=True), (what, thr, c)
      print("%s thr %g class %d: nd %d, ap %.12g (float64 %.12g)" % (what, thr, c, len(tp), got["ap"][t, c], ap))
      assert np.isclose(got["ap"][t, c], ap, rtol=0, atol=TOL_AP, equal_nan=True), (what, thr, c)
  return out


COUNTS = [0, 1, AP_BLOCK - 1, AP_BLOCK, AP_BLOCK + 1, 3 * AP_BLOCK + 77]


@pytest.mark.parametrize("use_07", [False, True])
@pytest.mark.parametrize("kind", ["random", "all_tp", "all_fp", "duplicates"])
def test_det_ap(kind, use_07):
  #          nd:   0  1  1023  1024  1025  3149   5 (no ground truth)
  npos = [4, 1, 300, 2000, 17, 900, 0]
  out = _check_ap(_ap_case(COUNTS + [5], npos, 7, kind), THRESHOLDS, use_07, kind)
  ap = out["ap"].cpu().numpy()
  assert ap[0, 0] == 0 and out["last_rec"][0, 0] == 0, "ground truth and no detection: 0"
  assert np.isnan(out["last_rec"].cpu().numpy()[:, 6]).all(), "detections and no ground truth: recall 0 / 0"
  assert (ap[:, 6] == 0).all() if use_07 else np.isnan(ap[:, 6]).all()
  if kind == "duplicates":
    assert int(out["tp"][0].sum()) == 5 and all(int(out["tp"][0, o]) == 1 for o in np.cumsum([0] + COUNTS)[1:6])
  if kind == "all_tp":
    assert abs(ap[0, 3] - AP_BLOCK / 2000.0) <= TOL_AP or use_07
  if kind == "all_fp":
    assert (ap[:, :6] == 0).all() and int(out["tp"].sum()) == 0


def test_det_ap_thresholds_from_one_match_equal_single_runs():
  from pointcontrast_amd import functional as PF
  iou, gid, offs, npos, n_gt = _ap_case(COUNTS, [4, 1, 300, 2000, 17, 900], 11)
  args = (_dev(iou), _dev(gid), _dev(offs), _dev(npos), n_gt)
  both = PF.det_ap(*args, THRESHOLDS, curves=True)
  for t, thr in enumerate(THRESHOLDS):
    one = PF.det_ap(*args, [thr], curves=True)
    for k in ("ap", "last_rec", "rec", "prec", "tp"):
      assert torch.equal(one[k][0], both[k][t]), (k, thr)
  again = PF.det_ap(*args, THRESHOLDS, curves=True)
  assert all(torch.equal(again[k].view(torch.int64) if again[k].dtype == torch.float64 else again[k],
                         both[k].view(torch.int64) if both[k].dtype == torch.float64 else both[k]) for k in ("ap", "rec", "prec", "tp"))
  assert not torch.equal(both["tp"][0], both["tp"][1])


# ---- 4. APCalculator --------------------------------------------------------------------------------------------------------------
def _golden_dataset():
  return {k[3:]: G[k] for k in G.files if k.startswith("ds_")}


def _flags_by_class(calc, thresholds):
  res = calc.evaluate(thresholds, curves=True)
  offs, tp = res["cls_offs"].cpu().numpy(), res["tp"].cpu().numpy()
  return {cid: tp[:, offs[d]:offs[d + 1]] for d, cid in enumerate(res["class_ids"])}


def test_calculator_reproduces_the_reference_metrics():
  from pointcontrast_amd.downstream import votenet
  d = _golden_dataset()
  A.assert_headings_clear(d["pred_heading"], d["gt_heading"], "golden dataset")
  A.assert_results_clear(A.eval_det(*mk.to_maps(d), 0.25), THRESHOLDS, "golden dataset")
  pred, gt = mk.to_lists(d)
  calc = votenet.APCalculator(THRESHOLDS)
  calc.step(pred[:3], gt[:3])
  calc.step(pred[3:], gt[3:])
  both = calc.compute_metrics()
  assert list(both) == THRESHOLDS
  for t, thr in enumerate(THRESHOLDS):
    single = votenet.APCalculator(thr)
    single.step(pred, gt)
    for got in (both[thr], single.compute_metrics()):
      assert list(got) == list(G["metric_keys"])
      vals = np.array(list(got.values()), np.float64)
      print(thr, dict(zip(got, vals)))
      assert np.allclose(vals, G["metric_vals_t%d" % t], rtol=0, atol=TOL_AP, equal_nan=True)
  flags = _flags_by_class(calc, THRESHOLDS)
  offs = G["curve_offs"]
  for k, c in enumerate(int(c) for c in G["classes"]):
    for t in range(2):
      assert np.array_equal(flags[c][t], G["tp_t%d" % t][offs[k]:offs[k + 1]]), (c, t)
  named = votenet.APCalculator(0.25, {c: "thing%d" % c for c in (3, 7, 11, 20, 42)})
  named.step(pred, gt)
  assert "thing7 Average Precision" in named.compute_metrics()
  calc.reset()
  assert calc.scan_cnt == 0 and np.isnan(calc.compute_metrics()[0.25]["mAP"])
  calc.step(pred, gt)
  assert np.allclose(list(calc.compute_metrics()[0.5].values()), G["metric_vals_t1"], rtol=0, atol=TOL_AP, equal_nan=True)


def test_calculator_tied_confidences_and_missing_classes():
  from pointcontrast_amd.downstream import votenet
  d = mk.dataset(seed=2, n_scenes=5, tie_scores=True, gt_only_class=99, pred_only_class=42)
  assert len(np.unique(d["pred_score"])) < len(d["pred_score"]) // 2
  A.assert_headings_clear(d["pred_heading"], d["gt_heading"], "tied dataset")
  want = {thr: A.eval_det(*mk.to_maps(d), thr) for thr in THRESHOLDS}
  A.assert_results_clear(want[0.25], THRESHOLDS, "tied dataset")
  calc = votenet.APCalculator(THRESHOLDS)
  calc.step(*mk.to_lists(d))
  got = calc.compute_metrics()
  flags = _flags_by_class(calc, THRESHOLDS)
  for t, thr in enumerate(THRESHOLDS):
    m = A.metrics(want[thr])
    assert list(got[thr]) == list(m)
    assert np.allclose(np.array(list(got[thr].values()), np.float64), np.array(list(m.values()), np.float64), rtol=0, atol=TOL_AP,
                       equal_nan=True)
    for c, r in want[thr].items():
      assert np.array_equal(flags[c][t], r["tp"]), (c, thr)
    assert got[thr]["99 Average Precision"] == 0 and got[thr]["99 Recall"] == 0
    assert np.isnan(got[thr]["42 Average Precision"]) and np.isnan(got[thr]["42 Recall"])


def _decoded_case(style, seed=0):
  """Predictions as tests/test_gpu_votenet_head.py's parse case, and labels placed on some of the decoded boxes."""
  rng = np.random.RandomState(seed + (17 if style == "bins" else 0))
  B, K, N, H, S, Cls, K2 = 2, 64, 2048, (12 if style == "bins" else 1), 6, 6, 12
  a = VF.prediction_inputs(rng, B, K, N, H, S, Cls)
  msa = rng.uniform(0.5, 1.4, (S, 3)).astype(np.float32)
  dec = R.box_decode(a["center"], a["heading_scores"], a["heading_residuals"], a["size_scores"], a["size_residuals"],
                     a["sem_cls_scores"], a["objectness_scores"], msa, style == "zero")
  pick = np.stack([rng.choice(K, K2, replace=False) for _ in range(B)])
  par = np.take_along_axis(np.asarray(dec["box_params"], np.float64), pick[..., None].repeat(7, -1), 1)
  cam = par[..., 0:3] + rng.normal(0, 0.05, (B, K2, 3))
  size_class = rng.randint(0, S, (B, K2))
  lab = dict(center_label=np.stack([cam[..., 0], cam[..., 2], -cam[..., 1]], -1).astype(np.float32),
             heading_class_label=rng.randint(0, H, (B, K2)), heading_residual_label=rng.uniform(-0.2, 0.2, (B, K2)).astype(np.float32),
             size_class_label=size_class, size_residual_label=(par[..., 3:6] * rng.uniform(0.9, 1.1, (B, K2, 3)) - msa[size_class]).astype(np.float32),
             sem_cls_label=rng.randint(0, Cls, (B, K2)), box_label_mask=(rng.rand(B, K2) > 0.25).astype(np.float32))
  cfg = dict(dataset_config=VF.DatasetConfig(H, msa, Cls, style == "zero"), remove_empty_box=True, use_3d_nms=True, cls_nms=True,
             nms_iou=0.25, use_old_type_nms=False, conf_thresh=0.05, per_class_proposal=False)
  a.update(lab)
  return a, cfg


@pytest.mark.parametrize("per_class", [False, True])
@pytest.mark.parametrize("style", ["zero", "bins"])
def test_step_decoded_equals_step_on_the_parsed_lists(style, per_class):
  from pointcontrast_amd.downstream import votenet
  a, cfg = _decoded_case(style)
  cfg["per_class_proposal"] = per_class
  ep = {k: _dev(v) for k, v in a.items()}
  gc, gk, gm = votenet.ground_truth_boxes(ep, cfg)
  lists = votenet.parse_groundtruths(ep, cfg)
  for b in range(2):
    kept = np.where(a["box_label_mask"][b] == 1)[0]
    assert [c for c, _ in lists[b]] == gk[b].cpu().numpy()[kept].tolist() and gm[b].cpu().numpy().sum() == len(kept)
    want = np.stack([box for _, box in lists[b]])
    assert np.abs(gc[b].cpu().numpy()[kept] - want).max() <= TOL * np.abs(want).max()
  host = votenet.APCalculator(THRESHOLDS)
  dev = votenet.APCalculator(THRESHOLDS)
  for _ in range(2):  # two batches: the ground-truth slots of the second come behind the first's
    host.step(votenet.parse_predictions(ep, cfg), lists)
    dev.step_decoded(votenet.decode_predictions(ep, cfg), ep, cfg)
  hm, dm = host.compute_metrics(), dev.compute_metrics()
  hf, df = _flags_by_class(host, THRESHOLDS), _flags_by_class(dev, THRESHOLDS)
  n_tp = 0
  for thr in THRESHOLDS:
    assert list(hm[thr]) == list(dm[thr]), (sorted(hm[thr]), sorted(dm[thr]))
    assert np.allclose(np.array(list(hm[thr].values()), np.float64), np.array(list(dm[thr].values()), np.float64), rtol=0,
                       atol=TOL_AP, equal_nan=True)
  for c in hf:
    assert np.array_equal(hf[c], df[c]), c
    n_tp += int(hf[c][0].sum())
  assert n_tp > 0, "the labels sit on decoded boxes: some detection must be a true positive"
  again = votenet.APCalculator(THRESHOLDS)
  for _ in range(2):
    again.step_decoded(votenet.decode_predictions(ep, cfg), ep, cfg)
  am = again.compute_metrics()
  assert all(np.array_equal(np.array(list(am[t].values())).view(np.int64), np.array(list(dm[t].values())).view(np.int64)) for t in THRESHOLDS)


def test_step_decoded_does_not_synchronise():
  from pointcontrast_amd.downstream import votenet
  a, cfg = _decoded_case("bins")
  cfg["per_class_proposal"] = True
  ep = {k: _dev(v) for k, v in a.items()}
  calc = votenet.APCalculator(THRESHOLDS)
  decoded = votenet.decode_predictions(ep, cfg)
  calc.step_decoded(decoded, ep, cfg)  # the constants are uploaded by the first call
  torch.cuda.synchronize()
  torch.cuda.set_sync_debug_mode("error")
  try:
    calc.step_decoded(decoded, ep, cfg)
  finally:
    torch.cuda.set_sync_debug_mode("default")
  assert calc.evaluate()["ap"].is_cuda and calc.scan_cnt == 4


# ---- 5. the C contract ------------------------------------------------------------------------------------------------------------
def test_c_contract():
  from pointcontrast_amd._lib import lib, check
  st = _stream()
  nd, n_gt, Cls, T = 1500, 40, 3, 2
  iou, gid, offs, npos, _ = _ap_case([700, 0, 800], [20, 5, 15], 3)
  iou, gid, offs, npos = _dev(iou), _dev(gid, torch.int32), _dev(offs, torch.int32), _dev(npos, torch.int32)
  ap = torch.full((T, Cls), -7.0, dtype=torch.float64, device=DEV)
  last = torch.full((T, Cls), -7.0, dtype=torch.float64, device=DEV)
  thr = (C.c_double * 2)(0.25, 0.5)
  need = lib.pcmi_det_ap_workspace_bytes(nd, n_gt, T)
  assert need >= T * (nd + n_gt) * 4 and lib.pcmi_det_ap_workspace_bytes(nd, n_gt, 17) == 0
  ws = torch.empty(need, dtype=torch.uint8, device=DEV)
  run = lambda w, nbytes, n=nd, t=T, cls=Cls, i=_p(iou): lib.pcmi_det_ap(i, _p(gid), _p(offs), _p(npos), n, n_gt, cls, thr, t, 0, _p(ap),  # noqa: E731
                                                                       _p(last), None, None, None, w, nbytes, st)
  assert run(_p(ws), need - 1) == PCMI_ERR_WORKSPACE and run(None, 0) == PCMI_ERR_WORKSPACE and lib.pcmi_last_error()
  assert run(_p(ws), need, n=-1) == PCMI_ERR_INVALID and run(_p(ws), need, t=0) == PCMI_ERR_INVALID
  assert run(_p(ws), need, t=17) == PCMI_ERR_INVALID and run(_p(ws), need, cls=0) == PCMI_ERR_INVALID
  assert run(_p(ws), need, i=None) == PCMI_ERR_INVALID
  z = torch.zeros((1, 4, 8, 3), device=DEV)
  zi = torch.zeros((1, 4), dtype=torch.int32, device=DEV)
  bg = torch.full((1, 4, 2), -7, dtype=torch.int32, device=DEV)
  bo = torch.full((1, 4, 2), -7.0, device=DEV)
  assert lib.pcmi_det_match(None, _p(z), _p(zi), _p(zi), 1, 4, 4, 2, _p(bg), _p(bo), st) == PCMI_ERR_INVALID
  assert lib.pcmi_det_match(_p(z), None, _p(zi), _p(zi), 1, 4, 4, 2, _p(bg), _p(bo), st) == PCMI_ERR_INVALID
  assert lib.pcmi_det_match(_p(z), _p(z), _p(zi), _p(zi), 1, 4, 4, 0, _p(bg), _p(bo), st) == PCMI_ERR_INVALID
  assert lib.pcmi_det_match(_p(z), _p(z), _p(zi), _p(zi), 1, -1, 4, 2, _p(bg), _p(bo), st) == PCMI_ERR_INVALID
  assert lib.pcmi_det_match(_p(z), _p(z), _p(zi), _p(zi), 1, 1025, 4, 2, _p(bg), _p(bo), st) == PCMI_ERR_UNSUPPORTED
  assert lib.pcmi_det_match(_p(z), _p(z), _p(zi), _p(zi), 1, 4, 257, 2, _p(bg), _p(bo), st) == PCMI_ERR_UNSUPPORTED
  assert lib.pcmi_box3d_iou(None, _p(z), 4, 4, _p(bo), None, st) == PCMI_ERR_INVALID
  assert lib.pcmi_box3d_iou(_p(z), _p(z), -1, 4, _p(bo), None, st) == PCMI_ERR_INVALID
  assert lib.pcmi_box3d_iou(_p(z), _p(z), 4, 4, None, None, st) == PCMI_ERR_INVALID
  torch.cuda.synchronize()
  assert bool((ap == -7).all()) and bool((last == -7).all()) and bool((bg == -7).all()) and bool((bo == -7).all()), \
      "a refused call wrote into an output"
  check(run(_p(ws), need))  # exactly the queried size
  check(lib.pcmi_det_ap(None, None, _p(offs.zero_()), _p(npos), 0, 0, Cls, thr, T, 0, _p(ap), _p(last), None, None, None, None, 0, st))
  torch.cuda.synchronize()
  assert bool((ap == 0).all()) and bool((last == 0).all()), "no detections: ap 0 and recall 0 for every class"
