"""GPU tests of the spatially partitioned PointInfoNCE (csrc/nce_part.hip; PF.PartitionNCELossFunction, PF.partition_matrix,
PartitionPointNCELossTrainer) against the float64 restatement tests/partition_nce_ref.py.

Tolerances are the project's own (tests/test_gpu_parity.py): the loss within 1e-4 max(|ref|, 0.1); dq, dk and lse (on live
entries) max|err| <= 1e-4 max|ref|; an upstream gradient of 1.7.  The partition matrix and the live counts are exact.  Inputs:
T in {0.4, 0.07}, c in {16, 32}, k = normalised q + 0.3 noise as in test_nce_parity."""
import ctypes as C

import numpy as np
import pytest
import torch

import partition_nce_ref as pr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G_UP = 1.7
PCMI_OK, PCMI_ERR_INVALID, PCMI_ERR_UNSUPPORTED, PCMI_ERR_WORKSPACE = 0, -1, -6, -7


@pytest.fixture(scope="module")
def PF(built_lib):
  from pointcontrast_amd import functional
  return functional


def make_case(n, c, B, seed=None, lo=-6, hi=6, scale=1.0):
  """Coordinates uniform in [lo, hi]^3, shuffled scene ids, normalised q and k = normalised (q + 0.3 noise), all from
  numpy.random.default_rng(seed or n)."""
  rng = np.random.default_rng(n if seed is None else seed)
  xyz = rng.integers(lo, hi + 1, (n, 3)).astype(np.int32)
  scene = rng.permutation(np.arange(n) % B).astype(np.int32)
  q = rng.standard_normal((n, c))
  q /= np.linalg.norm(q, axis=1, keepdims=True)
  k = q + 0.3 * rng.standard_normal((n, c))
  k /= np.linalg.norm(k, axis=1, keepdims=True)
  return (q * scale).astype(np.float32), (k * scale).astype(np.float32), xyz, scene


_REFS = {}


def reference(key, q, k, xyz, scene, B, T, r1, r2, A, E):
  """The restatement of a case, computed once (inv_T as the device takes it: the fp32 nearest to 1 / T)."""
  if key not in _REFS:
    _REFS[key] = pr.loss_and_grads(q, k, xyz, scene, B, T, r1, r2, A, E, gscale=G_UP, inv_T=float(np.float32(1.0 / T)))
  return _REFS[key]


def run_device(PF, q, k, xyz, scene, B, T, r1, r2, A, E):
  qd, kd = torch.from_numpy(q).to(DEV).requires_grad_(True), torch.from_numpy(k).to(DEV).requires_grad_(True)
  xd, sd = torch.from_numpy(xyz).to(DEV), torch.from_numpy(scene).to(DEV)
  loss = PF.PartitionNCELossFunction.apply(qd, kd, xd, sd, T, r1, r2, A, E, B)
  (loss * G_UP).backward()
  loss2, lse, live = PF.partition_nce_forward(qd, kd, xd, sd, T, r1, r2, A, E, B)
  torch.cuda.synchronize()
  assert torch.equal(loss.detach().view(torch.int32), loss2.view(torch.int32))
  return dict(loss=float(loss.detach()), lse=lse.cpu().numpy(), live=live.cpu().numpy(), dq=qd.grad.cpu().numpy(), dk=kd.grad.cpu().numpy(),
              bits=[t.detach().clone() for t in (loss, lse, qd.grad, kd.grad)])


def compare(got, ref, what):
  assert (got["live"] == ref["live"]).all(), (what, got["live"], ref["live"])
  figures = dict(loss=(got["loss"], ref["loss"]))
  for name in ("dq", "dk"):
    figures[name] = (float(np.abs(got[name] - ref[name]).max()), float(np.abs(ref[name]).max()))
  lv = ref["rowlive"]
  figures["lse"] = (float(np.abs(got["lse"] - ref["lse"])[lv].max()) if lv.any() else 0.0, float(np.abs(ref["lse"][lv]).max()) if lv.any() else 0.0)
  print(what, {k_: ("%.6g" % a, "%.6g" % b) for k_, (a, b) in figures.items()})
  assert np.isfinite(got["lse"]).all() and np.isfinite(got["dq"]).all() and np.isfinite(got["dk"]).all(), what
  assert abs(got["loss"] - ref["loss"]) <= 1e-4 * max(abs(ref["loss"]), 0.1), (what, figures["loss"])
  for name in ("dq", "dk", "lse"):
    err, mx = figures[name]
    assert err <= 1e-4 * mx, (what, name, err, mx)


MAIN = [(130, 2, 8, 2), (65, 1, 8, 2), (300, 4, 2, 2), (64, 2, 1, 1)]


@pytest.mark.parametrize("T,c", [(0.4, 32), (0.07, 32), (0.4, 16), (0.07, 16)])
@pytest.mark.parametrize("n,B,A,E", MAIN)
def test_main_parity(PF, n, B, A, E, T, c):
  """Coordinates uniform in [-6, 6]^3, r1_sq = 16, r2_sq = 100, shuffled scene ids.  Every (scene, partition) must be live in the
  reference -- asserted before comparing, so a kernel that drops a partition cannot hide."""
  q, k, xyz, scene = make_case(n, c, B)
  ref = reference(("main", n, c, T), q, k, xyz, scene, B, T, 16, 100, A, E)
  assert (ref["live"] > 0).all(), ref["live"]
  compare(run_device(PF, q, k, xyz, scene, B, T, 16, 100, A, E), ref, "main n=%d B=%d A=%d E=%d T=%g c=%d" % (n, B, A, E, T, c))


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129, 130, 300])
def test_sizes_around_the_tiles(PF, n):
  """64-row tiles and 64-row chunks: one tile with one split (n <= 64: the backward stores its gradients directly), several tiles
  and splits beyond; a last tile and a last chunk that are partly or wholly padding."""
  B, T, c = (2 if n > 2 else 1), (0.4 if n % 2 else 0.07), (32 if n % 3 else 16)
  q, k, xyz, scene = make_case(n, c, B, seed=1000 + n, lo=-4, hi=4)
  ref = reference(("tiles", n), q, k, xyz, scene, B, T, 9, 49, 4, 1)
  compare(run_device(PF, q, k, xyz, scene, B, T, 9, 49, 4, 1), ref, "tiles n=%d" % n)


def test_n_4097(PF):
  """65 row tiles, 8 splits of 9 chunks, the last chunk one row: P = 2 keeps the dense reference to a few seconds."""
  n, B, T = 4097, 3, 0.07
  q, k, xyz, scene = make_case(n, 32, B, lo=-20, hi=20)
  ref = reference(("4097",), q, k, xyz, scene, B, T, 64, 400, 1, 1)
  assert (ref["live"] > 0).all()
  compare(run_device(PF, q, k, xyz, scene, B, T, 64, 400, 1, 1), ref, "n=4097")


# ---- bit-exact: the partition rule --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,E", [(1, 1), (2, 1), (4, 2), (8, 2), (8, 1)])
def test_partition_matrix_is_exact(PF, A, E):
  """Every offset of [-3, 3]^3 from the centre and between one another (every sector boundary, dx == dy == 0, points exactly
  on r1_sq = 4 and r2_sq = 9), duplicate coordinates, scene ids outside [0, B)."""
  g = np.arange(-3, 4)
  xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
  xyz = np.concatenate([xyz, xyz[:40]]).astype(np.int32)  # duplicates
  rng = np.random.default_rng(7)
  scene = rng.integers(-1, 4, len(xyz)).astype(np.int32)  # B = 3: -1 and 3 lie outside
  got = PF.partition_matrix(torch.from_numpy(xyz).to(DEV), torch.from_numpy(scene).to(DEV), 4, 9, A, E, 3).cpu().numpy()
  ref = pr.partition_matrix(xyz, scene, 3, 4, 9, A, E)
  assert got.dtype == np.int8 and (got == ref).all(), np.argwhere(got != ref)[:5]
  assert set(np.unique(ref)) == set(range(-1, 2 * E * A))  # every partition occurs


def test_partition_matrix_needs_64_bit_distances(PF):
  m = 2 ** 17 - 1
  xyz = np.array([[-m, -m, -m], [m, m, m], [m, -m, m], [-m, m, -m], [0, 0, 0], [m, 0, 0], [0, -m, 0]], dtype=np.int32)
  scene = np.zeros(len(xyz), dtype=np.int32)
  for r2 in (12 * m * m, 12 * m * m - 1, 8 * m * m, 3 * m * m, m * m):
    for r1 in (0, m * m, r2):
      got = PF.partition_matrix(torch.from_numpy(xyz).to(DEV), torch.from_numpy(scene).to(DEV), r1, r2, 8, 2, 1).cpu().numpy()
      assert (got == pr.partition_matrix(xyz, scene, 1, r1, r2, 8, 2)).all(), (r1, r2)
  assert pr.partition_matrix(xyz, scene, 1, 0, 12 * m * m, 8, 2)[0, 1] >= 0 > pr.partition_matrix(xyz, scene, 1, 0, 12 * m * m - 1, 8, 2)[0, 1]


# ---- edges ------------------------------------------------------------------------------------------------------------------------
def test_single_row_scene_and_partition_dead_in_one_scene(PF):
  """Scene 0: a cloud with every partition live; scene 1: two points one step apart along x (only shell 0, elevation 0, sectors 0
  and 4 of 8: every other partition is dead THERE and live in scene 0); scene 2: a single row (a dead scene)."""
  T, c, A, E = 0.4, 32, 8, 2
  q, k, xyz, scene = make_case(123, c, 1, seed=5)
  xyz[120], xyz[121], xyz[122] = (0, 0, 0), (1, 0, 0), (2, 2, 2)
  scene[120:122], scene[122] = 1, 2
  ref = reference(("dead",), q, k, xyz, scene, 3, T, 16, 100, A, E)
  assert (ref["live"][0] > 0).all() and (ref["live"][1] > 0).sum() == 2 and (ref["live"][2] == 0).all()
  got = run_device(PF, q, k, xyz, scene, 3, T, 16, 100, A, E)
  compare(got, ref, "dead partitions")
  assert (got["dq"][122] == 0).all() and (got["dk"][122] == 0).all()


@pytest.mark.parametrize("c", [16, 32])
def test_all_rows_beyond_r2(PF, c):
  q, k, xyz, scene = make_case(130, c, 2)
  got = run_device(PF, q, k, xyz * 100, scene, 2, 0.07, 16, 100, 2, 2)
  assert got["loss"] == 0.0 and (got["live"] == 0).all()
  assert (got["dq"] == 0).all() and (got["dk"] == 0).all() and np.isfinite(got["lse"]).all()


@pytest.mark.parametrize("T,c", [(0.4, 32), (0.07, 16)])
def test_unnormalised_features_scaled_by_30(PF, T, c):
  """Logits up to 900 / T: a maximum per (row, partition), no overflow, and the 1e-4 of the normalised cases."""
  n, B, A, E = 130, 2, 8, 2
  q, k, xyz, scene = make_case(n, c, B, scale=30.0)
  ref = reference(("x30", T, c), q, k, xyz, scene, B, T, 16, 100, A, E)
  assert (ref["live"] > 0).all()
  compare(run_device(PF, q, k, xyz, scene, B, T, 16, 100, A, E), ref, "features x 30, T=%g c=%d" % (T, c))


@pytest.mark.parametrize("T", [0.4, 0.07])
def test_degenerate_configuration_is_the_plain_loss(PF, T):
  """One scene, distinct coordinates, A = E = 1, r1_sq = r2_sq beyond every distance: PF.NCELossFunction on the same data."""
  n, c = 300, 32
  q, k, _, _ = make_case(n, c, 1)
  xyz = np.stack([np.arange(n), np.zeros(n), np.zeros(n)], 1).astype(np.int32)
  got = run_device(PF, q, k, xyz, np.zeros(n, dtype=np.int32), 1, T, 10 ** 12, 10 ** 12, 1, 1)
  qd, kd = torch.from_numpy(q).to(DEV).requires_grad_(True), torch.from_numpy(k).to(DEV).requires_grad_(True)
  plain = PF.NCELossFunction.apply(qd, kd, T)
  (plain * G_UP).backward()
  assert (got["live"] == np.array([[n, 0]])).all()
  plain_loss = float(plain.detach())
  assert abs(got["loss"] - plain_loss) <= 1e-4 * max(abs(plain_loss), 0.1), (got["loss"], plain_loss)
  for name, ref in (("dq", qd.grad.cpu().numpy()), ("dk", kd.grad.cpu().numpy())):
    assert np.abs(got[name] - ref).max() <= 1e-4 * np.abs(ref).max(), name


def test_two_runs_give_identical_bits(PF):
  n, B, A, E, T = 300, 4, 8, 2, 0.07
  q, k, xyz, scene = make_case(n, 32, B)
  a = run_device(PF, q, k, xyz, scene, B, T, 16, 100, A, E)["bits"]
  b = run_device(PF, q, k, xyz, scene, B, T, 16, 100, A, E)["bits"]
  for x, y in zip(a, b):
    assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ---- the C contract (tests/c_contract.py) ---------------------------------------------------------------------------------------
def _vp(t):
  return None if t is None else C.c_void_p(t.data_ptr())


def _c_case(n=300, c=32, B=4):
  q, k, xyz, scene = make_case(n, c, B)
  dev = [torch.from_numpy(a).to(DEV) for a in (q, k, xyz, scene)]
  return dev + [torch.tensor([G_UP], device=DEV), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)]


def _c_run(lib, case, n, c, B, A, E, ws, r1=16, r2=100, outs=None):
  from c_contract import Guarded
  qd, kd, xd, sd, gs, st = case
  P = 2 * E * A
  o = outs or [Guarded(n * P * 4), Guarded(B * P * 4), Guarded(4), Guarded(n * c * 4), Guarded(n * c * 4)]
  rc = lib.pcmi_pnce_fwd(_vp(qd), _vp(kd), _vp(xd), _vp(sd), n, c, B, 2.5, r1, r2, A, E, o[0].vp, o[1].vp, o[2].vp, ws.vp, ws.size, st)
  rc2 = lib.pcmi_pnce_bwd(_vp(qd), _vp(kd), _vp(xd), _vp(sd), o[0].vp, o[1].vp, n, c, B, 2.5, r1, r2, A, E, _vp(gs), o[3].vp, o[4].vp,
                          ws.vp, ws.size, st)
  torch.cuda.synchronize()
  return rc, rc2, o


@pytest.mark.parametrize("n,c,A,E", [(300, 32, 8, 2), (64, 16, 1, 1), (4097, 32, 2, 2)])
def test_exact_workspace(built_lib, n, c, A, E):
  """The queried size between guard bands gives the bits of a 64 MiB workspace, and nothing outside an output is written."""
  from c_contract import Guarded
  from pointcontrast_amd._lib import lib
  B, P = 4, 2 * E * A
  case = _c_case(n, c, B)
  need = lib.pcmi_pnce_workspace_bytes(n, c, B, P)
  assert 0 < need <= 64 << 20
  runs = []
  for size in (need, 64 << 20):
    ws = Guarded(size)
    rc, rc2, o = _c_run(lib, case, n, c, B, A, E, ws)
    assert rc == PCMI_OK and rc2 == PCMI_OK, lib.pcmi_last_error().decode()
    ws.check("workspace of %d bytes" % size)
    for g in o:
      g.check("output")
    runs.append([g.view(torch.uint8, g.nbytes).clone() for g in o])
  for a, b in zip(*runs):
    assert torch.equal(a, b)


def test_refused_calls_enqueue_nothing(built_lib):
  from c_contract import GUARD_BYTE, Guarded
  from pointcontrast_amd._lib import lib
  n, c, B = 300, 32, 4
  case = _c_case(n, c, B)
  xd, sd, st = case[2], case[3], case[5]

  def untouched(gs):
    torch.cuda.synchronize()
    for g in gs:
      g.check("refused call")
      assert bool((g.view(torch.uint8, g.nbytes) == GUARD_BYTE).all()), "a refused call wrote an output"

  need = lib.pcmi_pnce_workspace_bytes(n, c, B, 32)
  for what, kw, code in (("A = 3", dict(A=3, E=2), PCMI_ERR_INVALID), ("A = 16", dict(A=16, E=1), PCMI_ERR_INVALID),
                         ("E = 3", dict(A=2, E=3), PCMI_ERR_INVALID), ("E = 0", dict(A=2, E=0), PCMI_ERR_INVALID),
                         ("r1_sq > r2_sq", dict(A=2, E=2, r1=101, r2=100), PCMI_ERR_INVALID)):
    ws = Guarded(need)
    rc, rc2, o = _c_run(lib, case, n, c, B, ws=ws, **kw)
    assert rc == code and rc2 == code, (what, rc, rc2)
    assert lib.pcmi_last_error().decode() != ""
    untouched(o + [ws])
  need = lib.pcmi_pnce_workspace_bytes(n, c, B, 8)
  ws = Guarded(need)
  ws.nbytes = need - 1  # the same allocation, declared one byte short
  rc, rc2, o = _c_run(lib, case, n, c, B, 2, 2, ws)
  ws.nbytes = need
  assert rc == PCMI_ERR_WORKSPACE and rc2 == PCMI_ERR_WORKSPACE, (rc, rc2)
  untouched(o + [ws])
  # the test aid beyond 4096 rows (the inputs are not read: the call is refused first)
  part = Guarded(4097)
  rc = lib.pcmi_pnce_partition(_vp(xd), _vp(sd), 4097, B, 16, 100, 2, 2, part.vp, st)
  assert rc == PCMI_ERR_UNSUPPORTED, rc
  untouched([part])
  rc = lib.pcmi_pnce_partition(_vp(xd), _vp(sd), n, B, 16, 100, 5, 2, part.vp, st)
  assert rc == PCMI_ERR_INVALID, rc
  untouched([part])


# ---- the trainer ------------------------------------------------------------------------------------------------------------------
OVERRIDES = ["net.model=Res16UNet14", "misc.nceT=0.4", "misc.npos=256", "opt.lr=0.1", "opt.max_iter=3", "trainer.stat_freq=2",
             "trainer.trainer=PartitionPointNCELossTrainer", "val.ransac_hypotheses=128", "val.num_queries=300"]


@pytest.fixture(scope="module")
def synth_batch():
  from pointcontrast_amd.lib.config import get_config
  from pointcontrast_amd.lib.ddp_data_loaders import SyntheticScanNetPairDataset, default_collate_pair_fn
  ds = SyntheticScanNetPairDataset(config=get_config(["data.crop=0.45"]), num_pairs=2)
  return default_collate_pair_fn([ds[0], ds[1]])


def _device_form(batch):
  """The batch as the device loader hands it over: tensors on the device, the number of distinct queries beside them."""
  out = {k_: (v.to(DEV) if torch.is_tensor(v) and k_ in ("sinput0_C", "sinput1_C", "sinput0_F", "sinput1_F", "correspondences") else v)
         for k_, v in batch.items()}
  out["correspondences"] = out["correspondences"].to(torch.int32).contiguous()
  out["n_queries"] = int(torch.unique(batch["correspondences"][:, 0]).numel())
  return out


@pytest.mark.parametrize("device_batch", [False, True])
def test_trainer_loss_equals_the_restatement(built_lib, synth_batch, device_batch, tmp_path, monkeypatch):
  """Res16UNet14 on the synthetic dataset, 3 iterations with fixed draws: each loss equals the restatement on that iteration's
  read-back features, coordinates and scene ids; the parameters change; validate still runs.  data.device_batch itself needs a
  frame corpus on disk, which the synthetic dataset has not: the second run feeds the SAME batch in the device loader's form
  (tensors on the device, n_queries beside them), which takes the trainer's device-batch path -- device pair selection from
  device correspondences, the queries' coordinates gathered from the batch's own device tensor."""
  from pointcontrast_amd.lib import ddp_trainer
  from pointcontrast_amd.lib.config import get_config
  from pointcontrast_amd.lib.ddp_data_loaders import FixedBatchLoader
  from pointcontrast_amd.lib.timer import AverageMeter, Timer
  monkeypatch.chdir(tmp_path)
  cfg = get_config(OVERRIDES + ["trainer.partition_r1=6", "trainer.partition_r2=30"])
  batch = _device_form(synth_batch) if device_batch else synth_batch
  torch.manual_seed(3)
  np.random.seed(3)
  tr = ddp_trainer.PartitionPointNCELossTrainer(cfg, FixedBatchLoader([batch], batch_size=2), val_data_loader=[synth_batch])
  assert (tr.r1_sq, tr.r2_sq, tr.azimuth, tr.elevation) == (36, 900, 2, 2)
  nq = int(torch.unique(synth_batch["correspondences"][:, 0]).numel())
  assert nq > 256
  w0 = tr.flat.w.clone()
  rng = np.random.RandomState(11)
  for it in range(3):
    draws = dict(uniform=torch.from_numpy(rng.rand(nq).astype(np.float32)), sampled_inds=rng.choice(nq, 256, replace=False))
    res = tr._train_iter(iter(tr.data_loader), [AverageMeter(), Timer(), Timer()], draws=draws)
    torch.cuda.synchronize()
    seen = {k_: v.cpu().numpy() for k_, v in tr._last_pairs.items()}
    assert seen["q"].shape == (256, 32) and seen["xyz"].shape == (256, 3)
    C0 = synth_batch["sinput0_C"].numpy()
    q_idx = tr_q_idx(synth_batch, draws)
    assert (seen["xyz"] == C0[q_idx, 1:4]).all() and (seen["scene"] == C0[q_idx, 0]).all()
    ref = pr.loss_and_grads(seen["q"], seen["k"], seen["xyz"], seen["scene"], 2, 0.4, 36, 900, 2, 2, inv_T=float(np.float32(1 / 0.4)))
    assert (ref["live"] > 0).any(), "no live partition: the comparison would be of zeros"
    print("iteration %d: loss %.6f, restatement %.6f, live %s" % (it, float(res["loss"]), ref["loss"], ref["live"].tolist()))
    assert abs(float(res["loss"]) - ref["loss"]) <= 1e-4 * max(abs(ref["loss"]), 0.1)
  assert not torch.equal(w0, tr.flat.w), "three steps left the parameters as they were"
  m = tr.validate([synth_batch])
  assert m["n_pairs"] == 2 and np.isfinite(m["hit_ratio@0.1"])


def tr_q_idx(batch, draws):
  from pointcontrast_amd.lib.ddp_trainer import PointNCELossTrainer
  return PointNCELossTrainer.select_pairs(batch["correspondences"], 256, draws)[0].numpy()
