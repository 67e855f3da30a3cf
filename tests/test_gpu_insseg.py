"""Instance segmentation on the device (csrc/cluster.hip, functional.py's wrappers, downstream/insseg.py) against
tests/insseg_ref.py, which tests/test_insseg_ref.py holds to planted answers.  Labels, compaction, scores, overlap, matching
and centroids are integer or single-rounding results and are compared EXACTLY; the offset losses within the bounds stated at
their test."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import ap_ref
import insseg_ref as ir
from c_contract import DEV, Guarded, PCMI_OK

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def PF():
  from pointcontrast_amd import functional as pf
  return pf


def _dev(a, dtype=None):
  t = torch.from_numpy(np.ascontiguousarray(a))
  return (t if dtype is None else t.to(dtype)).to(DEV)


def _stream():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _vp(t):
  return C.c_void_p(t.data_ptr())


def check_labels(PF, xyz, offs, group, r, what):
  """The device's labels and dropped count equal the restatement's; returns the labels."""
  xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
  want, want_dropped = ir.radius_components(xyz, offs, group, r)
  dropped = torch.zeros(1, dtype=torch.int64, device=DEV)
  got = PF.radius_components(_dev(xyz), _dev(np.asarray(offs, np.int64)), _dev(np.asarray(group, np.int32)), r, dropped=dropped).cpu().numpy()
  bad = np.flatnonzero(got != want)
  assert len(bad) == 0, "%s: %d of %d labels differ, first row %d: got %d want %d" % (what, len(bad), len(want), bad[0] if len(bad) else -1,
                                                                                   got[bad[0]] if len(bad) else 0, want[bad[0]] if len(bad) else 0)
  assert int(dropped.cpu()) == want_dropped, "%s: dropped %d, want %d" % (what, int(dropped.cpu()), want_dropped)
  return got


# ---- labels: degenerate inputs --------------------------------------------------------------------------------------------------
def test_labels_empty_single_and_empty_scenes(PF):
  assert check_labels(PF, np.zeros((0, 3)), [0, 0], np.zeros(0), 0.05, "n = 0").shape == (0,)
  assert check_labels(PF, [[0.1, 0.2, 0.3]], [0, 1], [3], 0.05, "n = 1").tolist() == [0]
  rng = np.random.default_rng(2)
  p = rng.uniform(0, 0.3, (90, 3))
  got = check_labels(PF, p, [0, 0, 40, 40, 90, 90], rng.integers(0, 2, 90), 0.05, "empty scenes first, in the middle and last")
  assert (got >= 0).all() and len(np.unique(got)) < 90


def test_no_rows_enqueues_nothing(PF):
  from pointcontrast_amd._lib import lib
  offs = _dev(np.array([0, 0], np.int64))
  label, ws = Guarded(64), Guarded(lib.pcmi_radius_components_workspace_bytes(0, 1))
  assert lib.pcmi_radius_components(None, 3, 0, _vp(offs), 1, None, 0.05, label.vp, None, ws.vp, ws.size, _stream()) == PCMI_OK
  torch.cuda.synchronize()
  for g in (label, ws):
    assert bool((g.buf == 0xA5).all()), "n == 0 must enqueue nothing"


# ---- labels: the three CPU cases ------------------------------------------------------------------------------------------------
def test_labels_generic_cloud(PF):
  p = ir.blob_case()
  got = check_labels(PF, p, [0, len(p)], np.zeros(len(p)), 0.06, "blobs")
  assert (np.bincount(got) >= 50).sum() == 3


def test_labels_tie_lattice(PF):
  p, _ = ir.lattice_case()
  got = check_labels(PF, p, [0, 56], np.zeros(56), 0.25, "lattice, r = pitch")
  assert len(np.unique(got)) == 3, "69 pairs at exactly r^2 are edges"
  got = check_labels(PF, p, [0, 56], np.zeros(56), float(np.nextafter(0.25, 0)), "lattice, r one ulp below the pitch")
  assert np.array_equal(got, np.arange(56))


def test_labels_scenes_groups_and_inactive_rows(PF):
  base = np.array([[0.0, 0, 0], [0.01, 0, 0], [0.02, 0, 0]], np.float32)
  p = np.concatenate([base, base, [[np.nan, 0, 0]], [[3e7, 0, 0]], [[0.0, 0, 0]], [[0.0, 0, 0]]]).astype(np.float32)
  got = check_labels(PF, p, [1, 3, 9], [0, 0, 0, 0, 1, 1, 0, 0, -1, 0], 0.015, "separation")
  assert got.tolist() == [-1, 1, 1, 3, 4, 4, -1, -1, -1, -1]


# ---- labels: the union-find under load ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing,components", [(0.9, 1), (1.1, 2048)])
def test_labels_shuffled_chain(PF, spacing, components):
  """2048 points on a line in random row order: deep trees and many retried hooks (0.9 r), or no edge at all (1.1 r)."""
  r = 0.03
  rng = np.random.default_rng(7)
  p = np.zeros((2048, 3), np.float32)
  p[:, 0] = (rng.permutation(2048) * (spacing * r)).astype(np.float32)
  got = check_labels(PF, p, [0, 2048], np.zeros(2048), r, "chain spaced %.1f r" % spacing)
  assert len(np.unique(got)) == components


def test_labels_identical_points_one_cell(PF):
  """4096 identical points: one cell, every pair an edge -- the trained-state worst case at the smallest size that shows it."""
  p = np.tile(np.array([[0.4, -1.3, 2.2]], np.float32), (4096, 1))
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  got = check_labels(PF, p, [0, 4096], np.full(4096, 5), 0.03, "identical points")
  assert (got == 0).all()
  # (the bound covers the restatement's 16.8 M pairs on the host too; the device's share is printed by scripts/insseg_bench.py)
  assert time.perf_counter() - t0 < 5.0, "the pair scan of a crowded cell must stay inside a test's few seconds"


def test_labels_uniform_singletons(PF):
  """20 000 uniform points in a 10 m cube, r = 0.03: almost all singletons: nearly one occupied table slot per row, the table at its sizing edge."""
  rng = np.random.default_rng(11)
  p = rng.uniform(0.0, 10.0, (20000, 3)).astype(np.float32)
  got = check_labels(PF, p, [0, 20000], np.zeros(20000), 0.03, "uniform")
  assert len(np.unique(got)) > 19900


def test_labels_negative_coordinates_and_the_boundary_at_zero(PF):
  rng = np.random.default_rng(13)
  chain = np.zeros((9, 3), np.float32)
  chain[:, 1] = (np.arange(9) - 4) * 0.02  # y from -0.08 to 0.08: crosses the cell boundary at 0 (r = 0.03)
  cloud = rng.uniform(-0.4, 0.0, (300, 3)).astype(np.float32)
  p = np.concatenate([chain - np.float32(0.001), cloud + np.float32([5.0, 0, 0])])
  got = check_labels(PF, p, [0, len(p)], np.zeros(len(p)), 0.03, "negative coordinates")
  assert (got[:9] == 0).all(), "one component across the boundary at 0"


def test_labels_column_slice(PF):
  p = ir.blob_case()
  wide = torch.full((len(p), 8), float("nan"), device=DEV)
  wide[:, 4:7] = _dev(p)
  want, _ = ir.radius_components(p, [0, len(p)], np.zeros(len(p)), 0.06)
  got = PF.radius_components(wide[:, 4:7], _dev(np.array([0, len(p)], np.int64)), _dev(np.zeros(len(p), np.int32)), 0.06)
  assert np.array_equal(got.cpu().numpy(), want)


# ---- every entry point in exactly its workspace, twice ----------------------------------------------------------------------------
def _instances_case():
  """Two scenes of the blob cloud with three groups: labels from the restatement, and everything downstream of them."""
  p = ir.blob_case()
  p = np.concatenate([p, p + np.float32(0.003)])
  n = len(p)
  rng = np.random.default_rng(17)
  group = np.where(rng.random(n) < 0.1, -1, 2).astype(np.int32)
  group[150:180] = 3
  offs = np.array([0, 220, 440], np.int64)
  label, _ = ir.radius_components(p, offs, group, 0.06)
  return p, offs, group, label


def test_radius_components_exact_workspace_and_determinism():
  from pointcontrast_amd._lib import lib
  p, offs, group, want = _instances_case()
  n = len(p)
  need = lib.pcmi_radius_components_workspace_bytes(n, 2)
  assert need > 0
  xyz, o, g = _dev(p), _dev(offs), _dev(group)
  runs = []
  for _ in range(2):
    ws, label = Guarded(need), Guarded(n * 4)
    rc = lib.pcmi_radius_components(_vp(xyz), 3, n, _vp(o), 2, _vp(g), 0.06, label.vp, None, ws.vp, ws.size, _stream())
    assert rc == PCMI_OK, lib.pcmi_last_error()
    torch.cuda.synchronize()
    ws.check("radius_components workspace")
    label.check("radius_components label")
    runs.append(label.view(torch.int32, n).cpu().numpy().copy())
  assert np.array_equal(runs[0], want) and np.array_equal(runs[0], runs[1])
  small = Guarded(need - 1)
  assert lib.pcmi_radius_components(_vp(xyz), 3, n, _vp(o), 2, _vp(g), 0.06, Guarded(n * 4).vp, None, small.vp, small.size, _stream()) == -7
  assert lib.pcmi_radius_components(_vp(xyz), 3, n, _vp(o), 2, _vp(g), 0.0, Guarded(n * 4).vp, None, small.vp, small.size, _stream()) == -1


@pytest.mark.parametrize("min_points,max_inst", [(40, 16), (1, 5)])
def test_compaction_exact_workspace_and_determinism(min_points, max_inst):
  """(1, 5): every component counts and max_inst overflows."""
  from pointcontrast_amd._lib import lib
  _, offs, group, label = _instances_case()
  n = len(label)
  want = ir.components_compact(label, offs, group, min_points, max_inst)
  if max_inst == 5:
    assert want["count"] > 5
  need = lib.pcmi_components_compact_workspace_bytes(n)
  lb, o, g = _dev(label), _dev(offs), _dev(group)
  runs = []
  for _ in range(2):
    ws = Guarded(need)
    outs = [Guarded(n * 4), Guarded(4)] + [Guarded(max_inst * 4) for _ in range(4)]
    rc = lib.pcmi_components_compact(_vp(lb), _vp(o), 2, n, _vp(g), min_points, max_inst, *[x.vp for x in outs], ws.vp, ws.size, _stream())
    assert rc == PCMI_OK, lib.pcmi_last_error()
    torch.cuda.synchronize()
    for x in [ws] + outs:
      x.check("components_compact")
    runs.append([x.view(torch.int32, m).cpu().numpy().copy() for x, m in zip(outs, [n, 1] + [max_inst] * 4)])
  inst, count, root, size, scene, grp = runs[0]
  assert int(count[0]) == want["count"]
  for got, name in ((inst, "instance"), (root, "root"), (size, "size"), (scene, "scene"), (grp, "group")):
    assert np.array_equal(got, want[name]), name
  for a, b in zip(runs[0], runs[1]):
    assert np.array_equal(a, b)


def test_compaction_keeps_min_points_and_drops_one_less(PF):
  label = np.concatenate([np.zeros(50), np.full(49, 50), np.full(51, 99)]).astype(np.int32)
  offs, group = np.array([0, 150], np.int64), np.arange(150).astype(np.int32)
  want = ir.components_compact(label, offs, group, 50, 8)
  got = PF.components_compact(_dev(label), _dev(offs), _dev(group), 50, 8)
  assert int(got["count"].cpu()) == want["count"] == 2
  for name in ("instance", "root", "size", "scene", "group"):
    assert np.array_equal(got[name].cpu().numpy(), want[name]), name
  assert got["root"].cpu().tolist()[:2] == [0, 99] and got["size"].cpu().tolist()[:2] == [50, 51]
  empty = PF.components_compact(_dev(np.zeros(0, np.int32)), _dev(np.array([0, 0], np.int64)), None, 1, 3)
  assert int(empty["count"].cpu()) == 0 and empty["size"].cpu().tolist() == [0, 0, 0] and empty["root"].cpu().tolist() == [-1] * 3


def test_scores_overlap_match_centroids_exact_and_deterministic(PF):
  from pointcontrast_amd._lib import lib
  rng = np.random.default_rng(23)
  n, P, G = 5000, 7, 9
  pred = np.repeat(rng.integers(-1, P + 1, n // 50), 50).astype(np.int32)  # runs of one id (the wave-uniform path) ...
  pred[::97] = rng.integers(-1, P + 1, len(pred[::97]))                      # ... broken up here and there
  gt = np.repeat(rng.integers(-2, G + 2, n // 25), 25).astype(np.int32)
  score = rng.random(n).astype(np.float32)
  score[:6] = [np.nan, np.inf, -0.5, 1.5, 0.0, 1.0]
  coords = np.concatenate([rng.integers(0, 2, (n, 1)), rng.integers(-70000, 70000, (n, 3))], 1).astype(np.int32)
  inter_w, ps_w, gs_w = ir.instance_overlap(pred, gt, P, G)
  psc, pcl = rng.integers(0, 2, P), rng.integers(0, 3, P)
  gsc, gcl = rng.integers(0, 2, G), rng.integers(0, 3, G)
  gs_w2 = gs_w.copy()
  best_gt_w, best_iou_w = ir.instance_match(inter_w, ps_w, gs_w2, psc, pcl, gsc, gcl)
  runs = []
  for _ in range(2):
    inter, ps, gs = PF.instance_overlap(_dev(pred), _dev(gt), P, G)
    best_gt, best_iou = PF.instance_match(inter, ps, gs, _dev(psc), _dev(pcl), _dev(gsc), _dev(gcl))
    s, cnt = PF.instance_centroids(_dev(coords), _dev(gt), G)
    # the scores in exactly the queried workspace
    need = lib.pcmi_instance_scores_workspace_bytes(P)
    ws, out = Guarded(need), Guarded(P * 8)
    score_d, pred_d = _dev(score), _dev(pred)
    rc = lib.pcmi_instance_scores(_vp(score_d), _vp(pred_d), n, P, _vp(ps), out.vp, ws.vp, ws.size, _stream())
    assert rc == PCMI_OK, lib.pcmi_last_error()
    torch.cuda.synchronize()
    ws.check("instance_scores workspace")
    out.check("instance_scores out")
    runs.append([t.cpu().numpy().copy() for t in (inter, ps, gs, best_gt, best_iou, s, cnt, out.view(torch.float64, P))])
  inter, ps, gs, best_gt, best_iou, s, cnt, sc = runs[0]
  assert np.array_equal(inter, inter_w) and np.array_equal(ps, ps_w) and np.array_equal(gs, gs_w)
  assert np.array_equal(best_gt, best_gt_w) and np.array_equal(best_iou.view(np.int32), best_iou_w.view(np.int32))
  assert (best_gt_w >= 0).any() and (best_gt_w < 0).any()
  s_w, c_w = ir.instance_centroids(coords, gt, G)
  assert np.array_equal(s, s_w) and np.array_equal(cnt, c_w)
  assert np.array_equal(sc.view(np.int64), ir.instance_scores(score, pred, ps_w).view(np.int64))
  for a, b in zip(runs[0], runs[1]):
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
  # ties go to the lowest index; another class is no candidate
  tie = _dev(np.array([[2, 2]], np.int32))
  one = lambda *v: _dev(np.array(v, np.int32))  # noqa: E731
  assert PF.instance_match(tie, one(4), one(3, 3), one(0), one(1), one(0, 0), one(1, 1))[0].cpu().tolist() == [0]
  assert PF.instance_match(tie, one(4), one(3, 3), one(0), one(1), one(0, 0), one(2, 1))[0].cpu().tolist() == [1]


# ---- offset losses --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 10000])
def test_offset_loss_against_the_restatement(PF, n):
  """Each loss within 2 n u S + 16 u S of the float64 restatement, S = the sum of |t| over the valid rows' terms t of that loss
  and u = 2^-53: two float64 sums of n terms taken in different orders, and the per-row arithmetic.  Every gradient element
  within 2^-23 |ref| + 1e-30: one float32 rounding of a value that is accurate in float64."""
  p, g, inst = ir.kink_rows(n, 100 + n)
  C_ = 4
  logits = torch.full((n, C_ + 3 + 1), float("nan"), device=DEV)  # the offsets are a column slice: ld = 8
  logits[:, C_:C_ + 3] = _dev(p)
  logits.requires_grad_(True)
  runs = []
  for _ in range(2):
    logits.grad = None
    norm, direction = PF.OffsetLossFunction.apply(logits[:, C_:C_ + 3], _dev(g), _dev(inst))
    (0.7 * norm - 1.3 * direction).backward()
    runs.append((float(norm.detach()), float(direction.detach()), logits.grad[:, C_:C_ + 3].cpu().numpy().copy()))
  want = ir.offset_loss(p, g, inst)
  terms = ir.offset_terms(p, g, inst)
  u, V = 2.0 ** -53, want[2]
  for k, name in ((0, "norm"), (1, "dir")):
    S = float(np.abs(terms[k]).sum())
    bound = (2 * V * u * S + 16 * u * S) / (V + 1e-6)
    print("offset %s loss, n = %d: got %.17g want %.17g, |diff| %.3g, bound %.3g" % (name, n, runs[0][k], want[k], abs(runs[0][k] - want[k]), bound))
    assert abs(runs[0][k] - want[k]) <= bound
  ref = ir.offset_grad(p, g, inst, 0.7, -1.3)
  err = np.abs(runs[0][2].astype(np.float64) - ref)
  tol = 2.0 ** -23 * np.abs(ref) + 1e-30
  print("offset gradient, n = %d: worst error / tolerance %.3g" % (n, float((err / tol).max())))
  assert (err <= tol).all()
  assert (runs[0][2][inst < 0] == 0).all()
  assert runs[0][:2] == runs[1][:2] and np.array_equal(runs[0][2].view(np.int32), runs[1][2].view(np.int32))
  assert bool(torch.isnan(logits.grad[:, C_ + 3:]).logical_not().all()) and bool((logits.grad[:, :C_] == 0).all())


def test_offset_loss_without_a_valid_row_and_exact_workspace(PF):
  from pointcontrast_amd._lib import lib
  p, g, _ = ir.kink_rows(300, 3)
  inst = np.full(300, -1, np.int32)
  pd = _dev(p).requires_grad_(True)
  norm, direction = PF.OffsetLossFunction.apply(pd, _dev(g), _dev(inst))
  (norm + direction).backward()
  assert float(norm.detach()) == 0.0 and float(direction.detach()) == 0.0 and bool((pd.grad == 0).all())
  p, g, inst = ir.kink_rows(1000, 4)
  need = lib.pcmi_offset_loss_workspace_bytes(1000)
  ws, out = Guarded(need), Guarded(24)
  p_d, g_d, inst_d = _dev(p), _dev(g), _dev(inst)
  rc = lib.pcmi_offset_loss_fwd(_vp(p_d), 3, _vp(g_d), _vp(inst_d), 1000, out.vp, ws.vp, ws.size, _stream())
  assert rc == PCMI_OK, lib.pcmi_last_error()
  torch.cuda.synchronize()
  ws.check("offset_loss workspace")
  out.check("offset_loss out")
  assert out.view(torch.float64, 3).cpu()[2] == float((inst >= 0).sum())


# ---- trainer --------------------------------------------------------------------------------------------------------------------
def _box_scenes():
  """Two scenes of two hollow boxes each (14 x 14 x 10 voxels, about 900 surface voxels per box): coords int32 [n, 4] scene-major,
  feats, target (classes 2 and 3; a floor strip of class 0), instance (0 .. 3 across the batch, -1 on the floor)."""
  rng = np.random.default_rng(29)
  g = np.stack(np.meshgrid(np.arange(14), np.arange(14), np.arange(10), indexing="ij"), -1).reshape(-1, 3)
  shell = g[((g == 0) | (g == np.array([13, 13, 9]))).any(1)]
  coords, target, instance = [], [], []
  for b in range(2):
    for k, origin in enumerate(([2, 3, 1], [30, 8, 1])):
      v = shell + np.array(origin) + b
      coords.append(np.concatenate([np.full((len(v), 1), b), v], 1))
      target.append(np.full(len(v), 2 + k))
      instance.append(np.full(len(v), 2 * b + k))
    f = np.stack(np.meshgrid(np.arange(0, 48), np.arange(0, 24), [0], indexing="ij"), -1).reshape(-1, 3)
    coords.append(np.concatenate([np.full((len(f), 1), b), f], 1))
    target.append(np.zeros(len(f)))
    instance.append(np.full(len(f), -1))
  coords = np.concatenate(coords).astype(np.int32)
  feats = rng.normal(0, 0.3, (len(coords), 3)).astype(np.float32)
  return (torch.from_numpy(coords), torch.from_numpy(feats), torch.from_numpy(np.concatenate(target).astype(np.int64)),
          torch.from_numpy(np.concatenate(instance).astype(np.int64)))


def _trainer(seed):
  from pointcontrast_amd.downstream.insseg import InstanceSegmentationTrainer
  torch.manual_seed(seed)
  return InstanceSegmentationTrainer(4, model="Res16UNet14", lr=0.05, max_iter=50, voxel_size=0.02, min_points=20)


def test_trainer_losses_gradient_determinism_and_predict(PF):
  coords, feats, target, instance = _box_scenes()
  assert 3000 < len(coords) < 7000
  a, b = _trainer(3), _trainer(3)
  assert a.model.final.kernel.shape[-1] == 7 and a.num_labels == 4
  seen = {}
  fwd, bwd = a.forward, a.engine.backward

  def forward(*args, **kw):
    seen["logits"] = fwd(*args, **kw)
    return seen["logits"]

  def backward(which, grad):
    seen["grad"] = grad.detach().clone()
    return bwd(which, grad)

  a.forward, a.engine.backward = forward, backward
  out = a.train_iter(coords, feats, target, instance)
  a.forward, a.engine.backward = fwd, bwd
  for k in ("loss", "loss_sem", "loss_norm", "loss_dir"):
    assert np.isfinite(float(out[k])), k
  assert float(out["loss"]) == float(out["loss_sem"].double() + out["loss_norm"] + out["loss_dir"])
  # the gradient that reached the backbone: [CE gradient | offset gradient] of the separate functions
  logits = seen["logits"].detach()
  sem = logits[:, :4].clone().requires_grad_(True)
  PF.SoftmaxCrossEntropyFunction.apply(sem, target.to(DEV), 255).backward()
  off = logits[:, 4:7].clone().requires_grad_(True)
  goal = a.offset_targets(coords, instance, 4)
  norm, direction = PF.OffsetLossFunction.apply(off, goal, instance.to(DEV))
  (norm + direction).backward()
  assert seen["grad"].shape == (len(coords), 7)
  assert torch.equal(seen["grad"][:, :4], sem.grad) and torch.equal(seen["grad"][:, 4:], off.grad)
  # the offset targets: centroid - voxel in metres, from exact integer sums
  c = coords.numpy().astype(np.int64)
  inst = instance.numpy()
  for k in range(4):
    rows = inst == k
    want = ((c[rows, 1:].sum(0) / rows.sum())[None] - c[rows, 1:]) * 0.02
    assert np.array_equal(goal.cpu().numpy()[rows], want.astype(np.float32))
  # two identically seeded trainers stay bit-identical
  b.train_iter(coords, feats, target, instance)
  for _ in range(2):
    ra, rb = a.train_iter(coords, feats, target, instance), b.train_iter(coords, feats, target, instance)
    assert float(ra["loss"]) == float(rb["loss"])
  for (name, pa), (_, pb) in zip(a.model.named_parameters(), b.model.named_parameters()):
    assert torch.equal(pa, pb), name
  pred = a.predict(coords, feats)
  n, M = len(coords), a.max_instances
  want = dict(instance=(torch.int32, (n,)), count=(torch.int32, (1,)), inst_class=(torch.int32, (M,)), inst_size=(torch.int32, (M,)),
              inst_scene=(torch.int32, (M,)), inst_score=(torch.float64, (M,)), scene_offsets=(torch.int64, (3,)))
  assert set(pred) == set(want)
  for k, (dt, shape) in want.items():
    assert pred[k].dtype == dt and tuple(pred[k].shape) == shape and pred[k].is_cuda, k
  miou, _, hist = a.evaluate(coords, feats, target.numpy())  # the parent's evaluation scores the class columns
  assert hist.shape == (4, 4) and 0.0 <= miou <= 100.0


# ---- evaluator ------------------------------------------------------------------------------------------------------------------
def _perfect_prediction(coords, target, instance, C_=4):
  """Ground-truth offsets and one-hot logits."""
  from pointcontrast_amd.downstream.insseg import cluster_instances, scene_offsets_of
  c = coords.numpy().astype(np.int64)
  inst = instance.numpy()
  offsets = np.zeros((len(c), 3), np.float32)
  for k in range(inst.max() + 1):
    rows = inst == k
    offsets[rows] = (((c[rows, 1:].sum(0) / rows.sum())[None] - c[rows, 1:]) * 0.02).astype(np.float32)
  logits = np.full((len(c), C_), -10.0, np.float32)
  logits[np.arange(len(c)), target.numpy()] = 10.0
  run = lambda lg, of: cluster_instances(coords.to(DEV), _dev(of), _dev(lg), scene_offsets_of(coords), 0.02, min_points=20)  # noqa: E731
  return logits, offsets, run


def test_evaluator_perfect_prediction_scores_one():
  from pointcontrast_amd.downstream.insseg import InstanceEvaluator
  coords, _, target, instance = _box_scenes()
  logits, offsets, run = _perfect_prediction(coords, target, instance)
  pred = run(logits, offsets)
  assert int(pred["count"].cpu()) == 4
  ev = InstanceEvaluator(4)
  ev.step(pred, instance, target)
  m = ev.compute_metrics()
  assert m["AP"] == 1.0 and m["AP50"] == 1.0 and m["AP25"] == 1.0
  assert (m["ap"][:, 2:] == 1.0).all() and np.isnan(m["ap"][:, :2]).all(), "every threshold; stuff classes are not scored"
  assert m["n_gt"].tolist() == [0, 0, 2, 2]


def test_evaluator_planted_degradation_equals_ap_ref():
  """Six ground-truth instances in two scenes; the prediction merges one into another, drops a third and halves a fourth."""
  from pointcontrast_amd.downstream.insseg import AP_THRESHOLDS, InstanceEvaluator
  sizes = [400, 300, 500, 350, 450, 250]
  gt = np.repeat(np.arange(6), sizes)
  n = len(gt)
  gt_cls = np.repeat([2, 2, 3, 2, 3, 3], sizes)
  scene_offsets = np.array([0, 1200, n], np.int64)  # instances 0 - 2 | 3 - 5
  pred = gt.copy()
  pred[gt == 1] = 0                                   # merged into instance 0 (same class, same scene)
  pred[gt == 2] = -1                                  # dropped
  pred[np.flatnonzero(gt == 3)[200:]] = -1            # (roughly) halved: 200 of 350 rows, IoU 0.571
  pred[np.flatnonzero(gt == 5)[:30]] = -1             # frayed: IoU 0.88
  ids = {0: 0, 3: 1, 4: 2, 5: 3}
  pinst = np.array([ids.get(v, -1) for v in pred], np.int32)
  P, M = 4, 8
  p_class = np.array([2, 2, 3, 3] + [-1] * (M - P), np.int32)
  p_scene = np.array([0, 1, 1, 1] + [-1] * (M - P), np.int32)
  p_score = np.array([0.9, 0.8, 0.95, 0.7] + [0.0] * (M - P))
  p_size = np.concatenate([np.bincount(pinst[pinst >= 0], minlength=P), np.zeros(M - P)]).astype(np.int32)
  dev_pred = dict(instance=_dev(pinst), count=_dev(np.array([P], np.int32)), inst_class=_dev(p_class), inst_size=_dev(p_size),
                  inst_scene=_dev(p_scene), inst_score=_dev(p_score), scene_offsets=_dev(scene_offsets))
  ev = InstanceEvaluator(4)
  ev.step(dev_pred, torch.from_numpy(gt), torch.from_numpy(gt_cls))
  m = ev.compute_metrics(keep_curves=True)
  # the restatement: overlap -> float32 quotients -> ap_ref.eval_class per class and threshold
  inter, ps, gs = ir.instance_overlap(pinst, gt, M, 6)
  iou32 = ir.iou_table(inter, ps, gs).astype(np.float32)
  g_scene = np.array([0, 0, 0, 1, 1, 1])
  g_class = np.array([2, 2, 3, 2, 3, 3])
  res = ir.evaluate_ap(iou32, p_scene[:P], p_class[:P], p_score[:P], g_scene, g_class, AP_THRESHOLDS, 4)
  ap_ref.assert_results_clear({(t, c): r for t in res for c, r in res[t].items()}, AP_THRESHOLDS, "planted degradation", margin=1e-3)
  # which predictions are true positives, exactly: the evaluator's own lists against eval_class
  out = ev.last_ap
  order = out["order"].cpu().numpy()
  tp = out["tp"].cpu().numpy()
  for ti, t in enumerate(AP_THRESHOLDS):
    for c in (2, 3):
      r = res[t][c]
      ranked = [r["pred_ids"][d] for d in r["order"]]
      mine = [int(q) for q in order if q < P and p_class[q] == c]
      assert mine == ranked, (t, c, mine, ranked)
      flags = [int(tp[ti, pos]) for pos, q in enumerate(order) if q < P and p_class[q] == c]
      assert flags == r["tp"].tolist(), (t, c, flags, r["tp"].tolist())
      assert abs(m["ap"][ti, c] - r["ap"]) <= 1e-12, (t, c, m["ap"][ti, c], r["ap"])
  want_ap = np.mean([[res[t][c]["ap"] for c in (2, 3)] for t in AP_THRESHOLDS[1:]])
  assert abs(m["AP"] - want_ap) <= 1e-12 and 0.0 < m["AP"] < 1.0
  assert abs(m["AP25"] - np.mean([res[0.25][c]["ap"] for c in (2, 3)])) <= 1e-12
  assert abs(m["AP50"] - np.mean([res[0.5][c]["ap"] for c in (2, 3)])) <= 1e-12
