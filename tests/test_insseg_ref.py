"""tests/insseg_ref.py -- the float64 restatement the kernels of csrc/cluster.hip are held to -- against planted answers and
independent spellings: scipy's KD-tree and connected components, exact rational arithmetic, torch.autograd in float64."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import insseg_ref as ir


def _one_scene(p):
  return [0, len(p)], np.zeros(len(p), np.int32)


def _scipy_labels(p, r):
  """The lowest row of every component by scipy: query_pairs + connected_components."""
  from scipy.sparse import coo_matrix
  from scipy.sparse.csgraph import connected_components
  from scipy.spatial import cKDTree
  n = len(p)
  pairs = cKDTree(np.asarray(p, np.float64)).query_pairs(r, output_type="ndarray")
  graph = coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
  comp = connected_components(graph, directed=False)[1]
  lowest = np.full(comp.max() + 1, n)
  np.minimum.at(lowest, comp, np.arange(n))
  return lowest[comp]


# ---- case 1: a generic cloud --------------------------------------------------------------------------------------------------
def test_generic_cloud_equals_scipy():
  p, r = ir.blob_case(), 0.06
  assert p.shape == (220, 3)
  d = p.astype(np.float64)[:, None] - p.astype(np.float64)[None]
  dist = np.sqrt((d ** 2).sum(-1))[np.triu_indices(len(p), 1)]
  assert np.abs(dist - r).min() > 1e-9, "precondition: no pair within 1e-9 of r (scipy's and the rule's rounding may then differ)"
  offs, group = _one_scene(p)
  label, dropped = ir.radius_components(p, offs, group, r)
  assert dropped == 0 and np.array_equal(label, _scipy_labels(p, r))
  sizes = np.bincount(label)
  assert (sizes >= 50).sum() == 3, "three blobs of 60 rows each stay three components of at least 50"


# ---- case 2: ties at exactly r^2 ----------------------------------------------------------------------------------------------
def test_tie_lattice():
  p, _ = ir.lattice_case()
  assert len(p) == 56
  offs, group = _one_scene(p)
  ei, ej = ir.radius_edges(p, offs, group, 0.25)
  d = p[ei].astype(np.float64) - p[ej].astype(np.float64)
  assert len(ei) == 69 and ((d ** 2).sum(1) == 0.0625).all(), "every edge is a lattice face at exactly r^2: <= keeps it"
  label, _ = ir.radius_components(p, offs, group, 0.25)
  # the planted answer: face-connected components of the occupied lattice sites, by flood fill on integer sites
  sites = {tuple(int(v) for v in np.rint(q / 0.25)): i for i, q in enumerate(p)}
  want = np.arange(len(p))
  changed = True
  while changed:
    changed = False
    for s, i in sites.items():
      for a in range(3):
        for step in (-1, 1):
          t = list(s)
          t[a] += step
          j = sites.get(tuple(t))
          if j is not None and want[j] < want[i]:
            want[i], changed = want[j], True
  assert np.array_equal(label, want) and len(np.unique(label)) == 3
  below, _ = ir.radius_components(p, offs, group, np.nextafter(0.25, 0))
  assert np.array_equal(below, np.arange(56)), "one ulp below the lattice pitch: 56 singletons"


# ---- case 3: separation -------------------------------------------------------------------------------------------------------
def test_scenes_groups_and_inactive_rows():
  base = np.array([[0.0, 0, 0], [0.01, 0, 0], [0.02, 0, 0]], np.float32)
  p = np.concatenate([base, base, [[np.nan, 0, 0]], [[3e7, 0, 0]], [[0.0, 0, 0]], [[0.0, 0, 0]]]).astype(np.float32)
  offs = [1, 3, 9]  # row 0 and row 9 lie in no scene; the two scenes overlap in space
  group = np.array([0, 0, 0, 0, 1, 1, 0, 0, -1, 0], np.int32)
  label, dropped = ir.radius_components(p, offs, group, 0.015)
  # scene 0 = rows 1, 2 (joined); scene 1: row 3 (group 0, alone), rows 4, 5 (group 1, joined), NaN, out of range, group -1
  assert label.tolist() == [-1, 1, 1, 3, 4, 4, -1, -1, -1, -1]
  assert dropped == 1, "3e7 / 0.015 = 2e9 cells: the one finite in-scene row that does not fit"


# ---- compaction ---------------------------------------------------------------------------------------------------------------
def test_compaction_threshold_numbering_and_overflow():
  #        rows: 0  1  2  3  4  5  6  7  8  9
  label = np.array([0, 1, 0, 1, 1, -1, 6, 0, 8, 99], np.int32)
  group = np.arange(10, 20)
  out = ir.components_compact(label, [0, 5, 10], group, 3, 4)  # sizes: root 0 -> 3, root 1 -> 3, root 6 -> 1, root 8 -> 1
  assert out["count"] == 2 and out["instance"].tolist() == [0, 1, 0, 1, 1, -1, -1, 0, -1, -1]
  assert out["root"].tolist() == [0, 1, -1, -1] and out["size"].tolist() == [3, 3, 0, 0]
  assert out["scene"].tolist() == [0, 0, -1, -1] and out["group"].tolist() == [10, 11, -1, -1]
  assert ir.components_compact(label, [0, 5, 10], group, 4, 4)["count"] == 0, "size == min_points - 1 is dropped"
  over = ir.components_compact(label, [0, 5, 10], group, 1, 2)  # four components, room for two
  assert over["count"] == 4 and over["instance"].tolist() == [0, 1, 0, 1, 1, -1, -1, 0, -1, -1] and over["root"].tolist() == [0, 1]


# ---- fixed-point scores -------------------------------------------------------------------------------------------------------
def test_scores_against_rational_arithmetic():
  rng = np.random.default_rng(5)
  score = rng.random(300).astype(np.float32)
  score[:6] = [np.nan, np.inf, -0.5, 1.5, 0.0, 1.0]
  inst = rng.integers(-1, 4, 300)
  inst[:6] = 0
  size = np.bincount(inst[inst >= 0], minlength=5)  # instance 4 has no row
  got = ir.instance_scores(score, inst, size)
  for k in range(5):
    total = Fraction(0)
    for s in score[inst == k]:
      c = Fraction(0) if not np.isfinite(s) else min(max(Fraction(float(s)), Fraction(0)), Fraction(1))
      total += Fraction(int(round(c * 2 ** 30)))  # (a float32 times 2^30 is never half-way between integers: 24 bits)
    want = float(total / (int(size[k]) * 2 ** 30)) if size[k] else 0.0
    assert got[k] == want, (k, got[k], want)


# ---- overlap, match, centroids ------------------------------------------------------------------------------------------------
def test_overlap_match_ties_and_centroids():
  pred = np.array([0, 0, 0, 0, 1, 1, -1, 5, 2, 2])
  gt = np.array([0, 0, 1, 1, 2, 2, 2, 0, -1, 9])
  inter, ps, gs = ir.instance_overlap(pred, gt, 3, 4)
  assert ps.tolist() == [4, 2, 2] and gs.tolist() == [3, 2, 3, 0]
  assert inter.tolist() == [[2, 2, 0, 0], [0, 0, 2, 0], [0, 0, 0, 0]]
  # prediction 0 overlaps gt 0 (2 / 5) and gt 1 (2 / 4); prediction 2 stands in a scene without ground truth
  best_gt, best_iou = ir.instance_match(inter, ps, gs, [0, 0, 1], [7, 7, 7], [0, 0, 0, 0], [7, 7, 7, 7])
  assert best_gt.tolist() == [1, 2, -1] and best_iou[0] == np.float32(0.5) and np.isneginf(best_iou[2])
  tie = np.array([[2, 2]], np.int32)
  assert ir.instance_match(tie, [4], [3, 3], [0], [1], [0, 0], [1, 1])[0].tolist() == [0], "equal overlaps: the lowest index"
  assert ir.instance_match(tie, [4], [3, 3], [0], [1], [0, 0], [2, 1])[0].tolist() == [1], "another class is no candidate"
  coords = np.array([[0, 1, 2, 3], [0, -5, 0, 7], [1, 2, 2, 2], [0, 9, 9, 9]], np.int32)
  s, c = ir.instance_centroids(coords, [0, 0, 1, -1], 2)
  assert s.tolist() == [[-4, 2, 10], [2, 2, 2]] and c.tolist() == [2, 1]


# ---- offset losses against torch.autograd -------------------------------------------------------------------------------------
def _torch_losses(p, g, valid):
  v = valid.double()
  V = v.sum()
  norm = ((p - g).abs().sum(1) * v).sum() / (V + 1e-6)
  gh = g / (g.norm(dim=1, keepdim=True) + 1e-8)
  ph = p / (p.norm(dim=1, keepdim=True) + 1e-8)
  direction = (-(gh * ph).sum(1) * v).sum() / (V + 1e-6)
  return norm, direction


@pytest.mark.parametrize("n", [1, 9, 300])
def test_offset_losses_and_gradients_against_autograd(n):
  p, g, inst = ir.kink_rows(n, n)
  pt = torch.from_numpy(p).double().requires_grad_(True)
  norm, direction = _torch_losses(pt, torch.from_numpy(g).double(), torch.from_numpy(inst >= 0))
  got = ir.offset_loss(p, g, inst)
  # both sides sum at most n terms of float64 with |t| <= 3 |p - g|_max: n u relative to the sum of |t| covers either order
  a, d = ir.offset_terms(p, g, inst)
  u = 2.0 ** -53
  assert abs(got[0] - float(norm.detach())) <= 2 * (n + 8) * u * np.abs(a).sum() / (got[2] + 1e-6)
  assert abs(got[1] - float(direction.detach())) <= 2 * (n + 8) * u * max(np.abs(d).sum(), 1.0) / (got[2] + 1e-6)
  assert got[2] == float((inst >= 0).sum())
  for gn, gd in ((1.0, 0.0), (0.0, 1.0), (0.7, -1.3)):
    (grad,) = torch.autograd.grad(gn * norm + gd * direction, pt, retain_graph=True)
    want, have = grad.numpy(), ir.offset_grad(p, g, inst, gn, gd)
    # the direction gradient is a difference of two terms of size |gd| / (V |p|) that cancel where p is parallel to g: both
    # sides carry a few u of THAT size, whatever is left of the difference
    pn = np.sqrt((p.astype(np.float64) ** 2).sum(1))
    scale = (abs(gn) + abs(gd) / np.maximum(pn, 1e-8)[:, None]) / (got[2] + 1e-6)
    assert (np.abs(have - want) <= 16 * u * scale).all(), np.abs(have - want).max()
    assert (have[inst < 0] == 0).all()
  assert (ir.offset_grad(p, g, inst)[1] != 0).any() if n >= 8 else True, "p = 0: the direction term still pulls (d|p|/dp = 0)"


def test_offset_losses_without_a_valid_row():
  p, g, _ = ir.kink_rows(9, 2)
  inst = np.full(9, -1)
  assert ir.offset_loss(p, g, inst) == (0.0, 0.0, 0.0)
  assert (ir.offset_grad(p, g, inst) == 0).all()
  pt = torch.from_numpy(p).double().requires_grad_(True)
  norm, direction = _torch_losses(pt, torch.from_numpy(g).double(), torch.zeros(9, dtype=torch.bool))
  assert float(norm.detach()) == 0.0 and float(direction.detach()) == 0.0
