"""CPU tests of the float64 restatement of the spatially partitioned PointInfoNCE (tests/partition_nce_ref.py) -- the sector
rule against atan2, the degenerate configuration against the oracle's PointInfoNCE, loss and gradients against an independent
dense spelling through torch's cross-entropy and autograd, the rules for dead partitions / scenes -- and of the trainer's
registration and configuration keys."""
import math

import numpy as np
import pytest
import torch

import partition_nce_ref as pr


@pytest.mark.parametrize("A", [2, 4, 8])
def test_sector_rule_is_the_atan2_floor(A):
  g = np.arange(-8, 9)
  dx, dy = [a.ravel() for a in np.meshgrid(g, g, indexing="ij")]
  got = pr.sector(dx, dy, A)
  for x, y, s in zip(dx, dy, got):
    if x == 0 and y == 0:
      assert s == A - 1
      continue
    # half-open sectors [lo, hi): a direction ON a boundary (a multiple of 45 degrees) belongs to the sector it opens.  atan2
    # rounds such an angle to within an ulp of the boundary; 1e-9 rad puts it inside, and no other lattice direction of
    # [-8, 8]^2 lies within 3 degrees of a boundary.
    ang = (math.atan2(y, x) % (2 * math.pi) + 1e-9) % (2 * math.pi)
    assert s == int(ang // (2 * math.pi / A)), (x, y, A, s)


def _case(n, c, B, seed, lo=-6, hi=6, scale=1.0):
  rng = np.random.default_rng(seed)
  q = rng.standard_normal((n, c))
  q /= np.linalg.norm(q, axis=1, keepdims=True)
  k = q + 0.3 * rng.standard_normal((n, c))
  k /= np.linalg.norm(k, axis=1, keepdims=True)
  xyz = rng.integers(lo, hi + 1, (n, 3))
  scene = rng.permutation(np.arange(n) % B)
  return (q * scale).astype(np.float32), (k * scale).astype(np.float32), xyz.astype(np.int32), scene.astype(np.int32)


def test_degenerate_configuration_is_point_info_nce():
  from oracle import loss_ref as lr
  n, T = 97, 0.4
  q, k, _, _ = _case(n, 32, 1, 5)
  xyz = np.stack([np.arange(n), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)], 1)  # distinct coordinates
  big = 10 ** 12
  r = pr.loss_and_grads(q, k, xyz, np.zeros(n, dtype=np.int64), 1, T, big, big, 1, 1, gscale=1.7)
  q64, k64 = torch.from_numpy(q).double().requires_grad_(True), torch.from_numpy(k).double().requires_grad_(True)
  idx = torch.arange(n)
  ref = lr.nce_loss(q64, k64, idx, idx, T)
  (ref * 1.7).backward()
  # P = 2: every negative lies in shell 0; shell 1 is dead everywhere and counts nowhere
  assert (r["live"] == np.array([[n, 0]])).all()
  assert abs(r["loss"] - float(ref)) <= 1e-12 * abs(float(ref))
  assert np.abs(r["dq"] - q64.grad.numpy()).max() <= 1e-12 and np.abs(r["dk"] - k64.grad.numpy()).max() <= 1e-12


def dense_torch(q, k, part, scene, B, P, T, gscale):
  """The independent spelling: P logit matrices masked with -inf (the diagonal kept), torch's float64 cross-entropy, autograd."""
  q64, k64 = torch.from_numpy(q).double().requires_grad_(True), torch.from_numpy(k).double().requires_grad_(True)
  n = len(q)
  logits = (q64 @ k64.t()) / T
  part_t, eye, labels = torch.from_numpy(part.astype(np.int64)), torch.eye(n, dtype=torch.bool), torch.arange(n)
  scene_t = torch.from_numpy(np.asarray(scene, dtype=np.int64))
  total, S = 0.0, 0
  for s in range(B):
    vals = []
    for p in range(P):
      mask = part_t == p
      rows = (scene_t == s) & mask.any(1)
      if not bool(rows.any()):
        continue
      lp = torch.where(mask | eye, logits, torch.full_like(logits, -float("inf")))
      vals.append(torch.nn.functional.cross_entropy(lp[rows], labels[rows]))
    if vals:
      total = total + sum(vals) / len(vals)
      S += 1
  if S == 0:
    return 0.0, np.zeros_like(q, dtype=np.float64), np.zeros_like(k, dtype=np.float64)
  loss = total / S
  (loss * gscale).backward()
  return float(loss), q64.grad.numpy(), k64.grad.numpy()


@pytest.mark.parametrize("n,B,A,E,T", [(130, 2, 8, 2, 0.4), (65, 1, 4, 2, 0.07), (90, 3, 2, 1, 0.4), (64, 2, 1, 1, 0.07)])
def test_loss_and_gradients_equal_the_dense_spelling(n, B, A, E, T):
  q, k, xyz, scene = _case(n, 16, B, n)
  r = pr.loss_and_grads(q, k, xyz, scene, B, T, 16, 100, A, E, gscale=1.7)
  loss, dq, dk = dense_torch(q, k, r["part"], scene, B, 2 * E * A, T, 1.7)
  assert abs(r["loss"] - loss) <= 1e-12 * max(abs(loss), 1.0)
  assert np.abs(r["dq"] - dq).max() <= 1e-12 and np.abs(r["dk"] - dk).max() <= 1e-12


def test_dead_partitions_scenes_duplicates_and_bad_scene_ids():
  T = 0.4
  q, k, _, _ = _case(8, 16, 1, 3)
  # scene 0: rows 0..3, rows 0 and 1 share a voxel (d2 == 0: no negatives of each other), row 2 at distance 1 (shell 0 with
  # r1_sq = 1), row 3 at distance 3 (shell 1); scene 1: row 4 alone (dead scene); scene 5 and -1 (rows 5, 6): out of range;
  # scene 2: row 7 alone.  A = E = 1: P = 2.
  xyz = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [3, 0, 0], [0, 0, 0], [1, 0, 0], [1, 0, 0], [2, 0, 0]])
  scene = np.array([0, 0, 0, 0, 1, 5, -1, 2])
  r = pr.loss_and_grads(q, k, xyz, scene, 3, T, 1, 9, 1, 1)
  part = r["part"]
  assert part[0, 1] == -1 and part[1, 0] == -1            # duplicates
  assert part[0, 2] == 0 and part[0, 3] == 1 and part[2, 3] == 1 and part[3, 2] == 1
  assert (part[4:] == -1).all() and (part[:, 4:] == -1).all()  # single rows, out-of-range scene ids
  assert (r["live"] == np.array([[3, 4], [0, 0], [0, 0]])).all()  # shell 0: rows 0, 1, 2; shell 1: all four
  assert not r["rowlive"][3, 0] and r["lse"][3, 0] == r["logits"][3, 3]  # a dead (row, partition): lse = l_ii
  loss, dq, dk = dense_torch(q, k, part, scene, 3, 2, T, 1.0)
  assert abs(r["loss"] - loss) <= 1e-12 and np.abs(r["dq"] - dq).max() <= 1e-12 and np.abs(r["dk"] - dk).max() <= 1e-12
  assert (r["dq"][4:] == 0).all() and (r["dk"][4:] == 0).all()
  # S == 0: everything beyond r2_sq
  far = pr.loss_and_grads(q, k, xyz * 100, np.zeros(8, dtype=np.int64), 1, T, 1, 9, 2, 2)
  assert far["loss"] == 0.0 and (far["dq"] == 0).all() and (far["dk"] == 0).all() and (far["live"] == 0).all()
  assert np.isfinite(far["lse"]).all()


def test_partition_is_not_symmetric_and_uses_64_bit_distances():
  m = 2 ** 17 - 1
  xyz = np.array([[-m, -m, -m], [m, m, m], [0, 0, 1]])
  part = pr.partition_matrix(xyz, np.zeros(3, dtype=np.int64), 1, 0, 12 * m * m, 8, 2)
  assert part[0, 1] == (1 * 2 + 0) * 8 + 1 and part[1, 0] == (1 * 2 + 1) * 8 + 5  # 45 degrees: sector 1; 225 degrees: sector 5
  assert pr.partition_matrix(xyz, np.zeros(3, dtype=np.int64), 1, 0, 12 * m * m - 1, 8, 2)[0, 1] == -1  # d2 = 12 m^2 > 2^32


def test_trainer_is_registered_and_configured():
  from pointcontrast_amd import ddp_train
  from pointcontrast_amd.lib import ddp_trainer
  from pointcontrast_amd.lib.config import get_config
  cls = ddp_train.get_trainer("PartitionPointNCELossTrainer")
  assert cls is ddp_trainer.PartitionPointNCELossTrainer and issubclass(cls, ddp_trainer.PointNCELossTrainer)
  c = get_config(["trainer.partition_azimuth=4"])
  assert c.trainer.partition_r1 == 20.0 and c.trainer.partition_r2 == 80.0
  assert c.trainer.partition_azimuth == 4 and c.trainer.partition_elevation == 2
  assert cls.partition_rule(get_config([])) == (400, 6400, 2, 2)
  assert cls.partition_rule(get_config(["trainer.partition_r1=2.5"]))[0] == 6  # floor(2.5^2)
  assert get_config([]).trainer.trainer == "HardestContrastiveLossTrainer"     # the default trainer is unchanged
