"""Dual-set proposals through the Python surface (downstream/insseg.py: cluster_proposals, both evaluators and step_points on
overlapping masks, InstanceSegmentationTrainer(dual_set=True)) against tests/proposals_ref.py, on three small synthetic scenes
with planted offsets: two objects that touch where they are and separate where their offsets send them, one object with zero
offsets and one whose offsets scatter it.  Everything is compared EXACTLY."""
import numpy as np
import pytest
import torch

import insbench_ref as br
import insseg_ref as ir
import proposals_ref as pr
from c_contract import DEV

pytestmark = pytest.mark.gpu
V, M, MIN_POINTS = 0.02, 16, 20
KEYS = ("instance", "count", "inst_class", "inst_size", "inst_scene", "inst_score", "scene_offsets")


def _dev(a, dtype=None):
  t = torch.from_numpy(np.ascontiguousarray(a))
  return (t if dtype is None else t.to(dtype)).to(DEV)


def _host(d):
  return {k: v.cpu().numpy() for k, v in d.items()}


def _scenes():
  """coords int32 [n, 4] scene-major, logits [n, 4], offsets [n, 3], gt instance [n], gt class [n], scene offsets [4].
    scene 0  A and B: boxes of 6 x 6 x 4 voxels of class 2 that TOUCH (one component where they are), offsets to their own
             centroids (two components where the offsets send them); A's rows are the more confident ones
    scene 1  C: class 3, ZERO offsets (both sets find the same mask);  D: 5 x 6 x 4, class 2, offsets to its centroid
    scene 2  E: class 3, offsets that scatter it over a metre (only the unshifted set finds it);  F: class 2, to its centroid
  and a floor strip of class 0 (stuff) under each."""
  rng = np.random.default_rng(17)
  box = lambda o, s: np.stack(np.meshgrid(*[np.arange(a, a + b) for a, b in zip(o, s)], indexing="ij"), -1).reshape(-1, 3)  # noqa: E731
  plan = [[("A", [2, 2, 1], (6, 6, 4), 2, 6.0, "centre"), ("B", [8, 2, 1], (6, 6, 4), 2, 3.0, "centre")],
          [("C", [2, 2, 1], (6, 6, 4), 3, 5.0, "zero"), ("D", [20, 2, 1], (5, 6, 4), 2, 4.0, "centre")],
          [("E", [2, 2, 1], (6, 6, 4), 3, 5.5, "scatter"), ("F", [20, 2, 1], (6, 6, 4), 2, 4.5, "centre")]]
  coords, logits, offsets, inst, cls, sizes, g = [], [], [], [], [], [], 0
  for b, objects in enumerate(plan):
    rows = 0
    for _, origin, shape, c, confidence, kind in objects:
      v = box(origin, shape)
      lg = np.full((len(v), 4), -2.0, np.float32)
      lg[:, c] = confidence + rng.integers(0, 4, len(v)) / 8.0
      off = {"centre": (v.mean(0)[None] - v) * V, "zero": np.zeros((len(v), 3)), "scatter": rng.uniform(-0.5, 0.5, (len(v), 3))}[kind]
      coords.append(np.concatenate([np.full((len(v), 1), b), v], 1))
      logits.append(lg)
      offsets.append(off.astype(np.float32))
      inst.append(np.full(len(v), g))
      cls.append(np.full(len(v), c))
      g, rows = g + 1, rows + len(v)
    f = box([0, 0, 0], (30, 10, 1))
    lg = np.full((len(f), 4), -2.0, np.float32)
    lg[:, 0] = 5.0
    coords.append(np.concatenate([np.full((len(f), 1), b), f], 1))
    logits.append(lg)
    offsets.append(np.zeros((len(f), 3), np.float32))
    inst.append(np.full(len(f), -1))
    cls.append(np.zeros(len(f), np.int64))
    sizes.append(rows + len(f))
  return (np.concatenate(coords).astype(np.int32), np.concatenate(logits), np.concatenate(offsets), np.concatenate(inst).astype(np.int64),
          np.concatenate(cls).astype(np.int64), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))


@pytest.fixture(scope="module")
def world():
  """The scenes on the device, the two per-set clusterings (cluster_instances, which tests/test_gpu_insseg.py holds to ITS
  restatement) on the host, and cluster_proposals at PointGroup's threshold and at 1 (nothing is suppressed)."""
  from pointcontrast_amd.downstream import insseg as iseg
  coords, logits, offsets, gt, gt_cls, offs = _scenes()
  args = (_dev(coords), _dev(offsets), _dev(logits), _dev(offs), V)
  kw = dict(min_points=MIN_POINTS, max_instances=M)
  parts = [_host(iseg.cluster_instances(*args, shifted=s, **kw)) for s in (False, True)]
  return dict(iseg=iseg, coords=coords, gt=gt, gt_cls=gt_cls, offs=offs, args=args, kw=kw, parts=parts,
              nms=iseg.cluster_proposals(*args, **kw), all=iseg.cluster_proposals(*args, nms_iou=1.0, **kw))


def _same_dict(got, want, what):
  for k, w in want.items():
    g = got[k].cpu().numpy()
    assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g.view(np.uint8), w.view(np.uint8)), "%s: %s differs" % (what, k)


def test_cluster_proposals_equals_the_restatement_and_the_planted_answer(world):
  n = len(world["coords"])
  for key, thr in (("nms", 0.3), ("all", 1.0)):
    got = world[key]
    assert set(got) == set(KEYS) | {"member", "keep", "dropped"} and all(v.is_cuda for v in got.values())
    assert tuple(got["member"].shape) == (n, 2) and tuple(got["keep"].shape) == (2 * M,) and got["inst_score"].dtype == torch.float64
    _same_dict(got, pr.combine_sets(world["parts"], 3, nms_iou=thr), key)
    assert np.array_equal(got["scene_offsets"].cpu().numpy(), world["offs"])
  # where they are: AB, C, D, E, F;  shifted: A, B, C, D, F (E is scattered)
  p, q = world["parts"]
  assert p["count"].tolist() == [5] and q["count"].tolist() == [5] and p["inst_size"][:5].tolist() == [288, 144, 120, 144, 144]
  assert q["inst_size"][:5].tolist() == [144, 144, 144, 120, 144]
  got = _host(world["nms"])
  assert got["count"].tolist() == [5, 5] and got["dropped"].tolist() == [0]
  # A (shifted, the most confident) suppresses AB; only AB overlaps B, and AB is dead: B stays.  C, D, F: equal masks with equal
  # scores, the lower slot -- the unshifted set's -- stays
  assert np.flatnonzero(got["keep"]).tolist() == [1, 2, 3, 4, M, M + 1]
  gt, inst = world["gt"], got["instance"]
  assert [sorted(set(inst[gt == g].tolist())) for g in range(6)] == [[M], [M + 1], [1], [2], [3], [4]] and (inst[gt < 0] == -1).all()
  assert (got["inst_class"][got["keep"] == 0] == -1).all() and got["inst_size"][0] == 288, "the size before suppression stays"
  assert ((got["member"] >= 0).sum(1) <= 1).all(), "after suppression these masks are disjoint"
  both = _host(world["all"])
  assert both["keep"].sum() == 10 and ((both["member"] >= 0).sum(1) == 2).sum() == 288 + 144 + 120 + 144
  assert [sorted(set(both["instance"][gt == g].tolist())) for g in range(6)] == [[M], [0], [1], [2], [3], [4]], "rows of B: AB outranks B"


def test_one_shifted_set_is_cluster_instances(world):
  iseg = world["iseg"]
  got = iseg.cluster_proposals(*world["args"], sets=("shifted",), **world["kw"])
  want = iseg.cluster_instances(*world["args"], **world["kw"])
  for k in KEYS:
    assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
  assert torch.equal(got["member"][:, 0], want["instance"]) and got["keep"].sum() == 5
  with pytest.raises(AssertionError):
    iseg.cluster_proposals(*world["args"], sets=("shifted", "moved"), **world["kw"])


def test_cluster_proposals_reads_nothing_back_and_repeats_its_bits(world):
  iseg = world["iseg"]
  torch.cuda.synchronize()
  mode = torch.cuda.get_sync_debug_mode()
  try:
    torch.cuda.set_sync_debug_mode("error")
    again = iseg.cluster_proposals(*world["args"], **world["kw"])
  finally:
    torch.cuda.set_sync_debug_mode(mode)
  bits = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t  # noqa: E731
  for k, v in world["nms"].items():
    assert torch.equal(bits(v), bits(again[k])), k


# ---- evaluators -----------------------------------------------------------------------------------------------------------------
def _evaluators(iseg):
  return ((iseg.InstanceEvaluator, {}), (iseg.InstanceBenchmarkEvaluator, dict(min_region=100)))


def test_a_member_of_one_column_scores_as_the_same_masks_as_instance(world):
  iseg = world["iseg"]
  pred = iseg.cluster_instances(*world["args"], shifted=False, **world["kw"])  # AB merged: not a perfect score
  as_member = dict(pred, member=pred["instance"].reshape(-1, 1), instance=torch.full_like(pred["instance"], -1))
  gt, gt_cls = torch.from_numpy(world["gt"]), torch.from_numpy(world["gt_cls"])
  for cls, kw in _evaluators(iseg):
    a, b = cls(4, **kw), cls(4, **kw)
    a.step(pred, gt, gt_cls)
    b.step(as_member, gt, gt_cls)
    ma, mb = a.compute_metrics(), b.compute_metrics()
    assert br.same_metrics(ma, mb), cls.__name__
    assert 0.0 < ma["AP"] < 1.0 and ma["n_gt"].tolist() == [0, 0, 4, 2]


def test_two_overlapping_columns_equal_the_restatement(world):
  iseg = world["iseg"]
  pred, host = world["all"], _host(world["all"])
  gt, gt_cls = world["gt"], world["gt_cls"]
  # the benchmark protocol: the whole metrics dict
  ev, ref = iseg.InstanceBenchmarkEvaluator(4), pr.BenchEvaluator(4)
  ev.step(pred, torch.from_numpy(gt), torch.from_numpy(gt_cls))
  ref.step(host, gt, gt_cls)
  m, want = ev.compute_metrics(), ref.compute_metrics()
  print({k: m[k] for k in ("AP", "AP50", "AP25", "n_gt")})
  assert br.same_metrics(m, want)
  assert 0.0 < m["AP"] < 1.0 and m["n_gt"].tolist() == [0, 0, 4, 2]
  exact = iseg.InstanceBenchmarkEvaluator(4)
  exact.step(world["nms"], torch.from_numpy(gt), torch.from_numpy(gt_cls))
  assert exact.compute_metrics()["AP"] == 1.0, "after suppression every mask is a ground-truth instance"
  # the VOC-style evaluator: what it hands to det_ap -- per prediction its best ground truth and the quotient
  voc = iseg.InstanceEvaluator(4)
  voc.step(pred, torch.from_numpy(gt), torch.from_numpy(gt_cls))
  inter, ps, gs = pr.member_overlap(host["member"], gt, 2 * M, 6)
  assert gs.tolist() == [144, 144, 144, 120, 144, 144] and ps[0] == 288 and inter[0, :2].tolist() == [144, 144]
  best_gt, best_iou = ir.instance_match(inter, ps, gs, host["inst_scene"], host["inst_class"], [0, 0, 1, 1, 2, 2], [2, 2, 3, 2, 3, 2])
  assert np.array_equal(voc._gid[0].cpu().numpy(), best_gt) and np.array_equal(voc._iou[0].cpu().numpy().view(np.int32), best_iou.view(np.int32))
  assert best_iou[0] == np.float32(0.5) and best_iou[M] == 1.0
  mv = voc.compute_metrics()
  assert 0.0 < mv["AP"] < 1.0 and mv["AP25"] < 1.0, "AB, and a duplicate of every object found twice, are false positives"


def test_step_points_on_jittered_vertices_equals_the_restatement(world):
  iseg = world["iseg"]
  rng = np.random.default_rng(23)
  coords, gt, gt_cls = world["coords"], world["gt"], world["gt_cls"]
  k = rng.integers(1, 3, len(coords))  # one or two vertices per voxel, less than half a voxel off its centre
  rows = np.repeat(np.arange(len(coords)), k)
  points = (coords[rows, 1:].astype(np.float64) + 0.5 + rng.uniform(-0.45, 0.45, (len(rows), 3))) * V
  T = np.tile(np.diag([1 / V, 1 / V, 1 / V, 1.0]).reshape(1, 16), (3, 1))
  offs = np.searchsorted(coords[rows, 0], np.arange(4)).astype(np.int64)
  pred, host = world["all"], _host(world["all"])
  ev, ref = iseg.InstanceBenchmarkEvaluator(4), pr.BenchEvaluator(4)
  got = ev.step_points(_dev(coords), pred, T, torch.from_numpy(points), torch.from_numpy(gt[rows]), torch.from_numpy(gt_cls[rows]),
                       torch.from_numpy(offs))
  want = ref.step_points(coords, host, T, points, gt[rows], gt_cls[rows], offs)
  assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want) and np.array_equal(want, host["instance"][rows])
  m, m_want = ev.compute_metrics(), ref.compute_metrics()
  assert br.same_metrics(m, m_want) and 0.0 < m["AP"] < 1.0
  # a vertex carries both columns of its voxel: the same masks as an evaluator stepped on the voxels, counted per vertex
  per_voxel = pr.BenchEvaluator(4)
  per_voxel.step(dict(host, member=host["member"][rows], instance=host["instance"][rows], scene_offsets=offs), gt[rows], gt_cls[rows])
  assert br.same_metrics(per_voxel.compute_metrics(), m_want)


# ---- trainer --------------------------------------------------------------------------------------------------------------------
def _trainer(seed, **kw):
  from pointcontrast_amd.downstream.insseg import InstanceSegmentationTrainer
  torch.manual_seed(seed)
  return InstanceSegmentationTrainer(4, model="Res16UNet14", lr=0.05, max_iter=50, voxel_size=0.02, min_points=20, **kw)


def _outputs(tr, coords, feats):
  tr.model.eval()
  tr._full_width = True
  try:
    with torch.no_grad():
      return tr.forward(coords, feats, training=False)
  finally:
    tr._full_width = False


def test_trainer_predict_with_and_without_the_dual_set():
  from test_gpu_insseg import _box_scenes
  from pointcontrast_amd.downstream import insseg as iseg
  coords, feats, _, _ = _box_scenes()
  for dual in (False, True):
    tr = _trainer(3, dual_set=True, nms_iou=0.25) if dual else _trainer(3)
    assert tr.dual_set == dual and tr.nms_iou == (0.25 if dual else 0.3)
    out = _outputs(tr, coords, feats)
    common = (coords, out[:, 4:7], out[:, :4], iseg.scene_offsets_of(coords), tr.voxel_size, tr.radius, tr.min_points, tr.stuff_classes,
              tr.max_instances)
    want = iseg.cluster_proposals(*common, nms_iou=0.25) if dual else iseg.cluster_instances(*common)
    got = tr.predict(coords, feats)
    assert set(got) == (set(KEYS) | {"member", "keep", "dropped"} if dual else set(KEYS))
    for k in want:
      assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and torch.equal(got[k], want[k]), (dual, k)


def test_trainer_validate_scenes_on_overlapping_masks_equals_the_restatement():
  from test_gpu_insseg_input import _aug, _rooms
  from pointcontrast_amd.downstream import insseg as iseg, semseg as ss
  from pointcontrast_amd.downstream.insseg import InstanceSegmentationTrainer
  scenes = _rooms()
  torch.manual_seed(3)
  tr = InstanceSegmentationTrainer(5, model="Res16UNet14", lr=0.05, max_iter=50, voxel_size=0.05, radius=0.08, min_points=20, max_instances=64,
                                   dual_set=True, input_pipeline=iseg.InstanceInputPipeline(_aug(ss), DEV))
  batches = [scenes[:2], scenes[2:]]
  got = tr.validate_scenes(batches, benchmark=True)
  assert isinstance(tr.instance_evaluator, iseg.InstanceBenchmarkEvaluator)
  pipe = iseg.InstanceInputPipeline(_aug(ss, augment=False), DEV)
  ref, kept = pr.BenchEvaluator(5, tr.stuff_classes), 0
  for batch in batches:
    coords, feats, target, instance, G, _ = pipe(batch)
    pred = _host(tr.predict(coords, feats))
    assert pred["member"].shape == (len(coords), 2) and pred["keep"].shape == (128,)
    kept += int(pred["keep"].sum())
    ref.step(pred, instance.cpu().numpy(), target.cpu().numpy(), G)
  want = ref.compute_metrics()
  print("kept proposals", kept, {k: got[k] for k in ("AP", "AP50", "AP25", "n_gt")})
  assert br.same_metrics(got, want)
  voc = tr.validate_scenes(batches, benchmark=False)
  assert set(voc) == set(want) and voc["n_gt"].tolist() == [0, 0, 6, 6, 3]
