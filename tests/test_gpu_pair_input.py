"""The pre-training input kernels (csrc/pair_input.hip: pcmi_pair_transform, pcmi_pair_voxelize, pcmi_pair_match,
pcmi_pair_collate), lib/pair_input.py (PairInputPipeline, DevicePairLoader) and the trainers' device-batch paths against
tests/pair_input_ref.py, which tests/test_pair_input_ref.py holds to the host loader.  The arithmetic is fixed -- integers, fp64
in stated orders, float32 outputs from one rounding -- so every comparison is BIT-exact.  Cloud sizes: 0, 1, 63 / 64 / 65 around
the wave, 1023 / 1024 / 1025 / 2049 around the centroid chunk, and about 5000 for several workgroups."""
import numpy as np
import pytest
import torch

import pair_input_ref as pr
from c_contract import DEV
from test_pair_input_ref import MULT, config, make_frames, write_corpus

pytestmark = pytest.mark.gpu

V = 0.05
SIZES = {1: [4999, 1025], 2: [0, 64, 1024, 1023], 3: [1, 63, 65, 5003, 2049, 0]}


@pytest.fixture(scope="module")
def PF():
  from pointcontrast_amd import functional as pf
  return pf


def _dev(a, dtype=None):
  t = torch.from_numpy(np.ascontiguousarray(a))
  return (t if dtype is None else t.to(dtype)).to(DEV)


def _host(t):
  return t.cpu().numpy()


def _offs(sizes):
  return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _same(got, want, what):
  got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
  assert got.dtype == want.dtype and got.shape == want.shape, "%s: %s %s, want %s %s" % (what, got.dtype, got.shape, want.dtype, want.shape)
  assert got.tobytes() == want.tobytes(), "%s differs" % what


def _rotations(rng, k):
  from pointcontrast_amd.lib import synthetic
  return np.stack([synthetic._rotation(rng.rand(3) - 0.5, 2 * np.pi * (rng.rand() - 0.5)) for _ in range(k)])


def _clouds(rng, sizes, dtype):
  """Pairs of overlapping surface patches, negative coordinates included: cloud 2 b + 1 is a moved, noisy copy of the pool that
  cloud 2 b is cut from."""
  out = []
  for b in range(len(sizes) // 2):
    n0, n1 = sizes[2 * b], sizes[2 * b + 1]
    k = max(n0, n1, 1)
    pool = np.stack([rng.uniform(-0.9, 0.5, k), rng.uniform(-0.6, 0.6, k), rng.normal(0, 0.004, k) - 0.3], 1)
    out += [pool[:n0].astype(dtype), (pool[rng.permutation(k)[:n1]] + rng.normal(0, 0.003, (n1, 3)) + [0.01, -0.02, 0.005]).astype(dtype)]
  return out


# ---- transform ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("B", [1, 2, 3])
def test_transform_equals_restatement(PF, B, dtype):
  rng = np.random.RandomState(10 * B)
  clouds = _clouds(rng, SIZES[B], dtype)
  raw, offs = np.concatenate(clouds), _offs(SIZES[B])
  scale, rot = rng.uniform(0.8, 1.2, B), _rotations(rng, 2 * B)
  for R in (rot, None):
    want = pr.pair_transform(raw, offs, scale, R)
    got = PF.pair_transform(_dev(raw), _dev(offs), _dev(scale), None if R is None else _dev(R))
    for k in ("points", "T", "trans", "flags"):
      _same(_host(got[k]), want[k], "B %d rotate %s: %s" % (B, R is not None, k))
    assert not want["flags"].any()
  if B > 1:  # a non-finite point flags its pair (before and after the transform) and leaves the neighbours' rows alone
    clean = pr.pair_transform(raw, offs, scale, rot)
    bad = raw.copy()
    bad[offs[2] + 5, 2] = np.inf
    want2 = pr.pair_transform(bad, offs, scale, rot)
    got2 = PF.pair_transform(_dev(bad), _dev(offs), _dev(scale), _dev(rot))
    assert want2["flags"].tolist() == [0, pr.FLAG_NONFINITE] + [0] * (B - 2)
    _same(_host(got2["flags"]), want2["flags"], "flags with an infinity")
    keep = np.r_[0:offs[2], offs[4]:offs[-1]]
    _same(_host(got2["points"])[keep], clean["points"][keep], "the neighbours of a flagged pair")


def test_cpu_tensors_are_refused(PF):
  from pointcontrast_amd._lib import PcmiError
  raw, offs = torch.zeros((4, 3), dtype=torch.float64), torch.tensor([0, 2, 4])
  with pytest.raises(PcmiError, match="no CPU path"):
    PF.pair_transform(raw, offs, torch.ones(1, dtype=torch.float64))
  with pytest.raises(PcmiError, match="no CPU path"):
    PF.pair_voxelize(raw, offs, V)
  vox = dict(points=raw, vox_offsets=offs, side_offsets=torch.zeros((2, 2), dtype=torch.int64))
  with pytest.raises(PcmiError, match="no CPU path"):
    PF.pair_match(vox, torch.eye(4, dtype=torch.float64)[None], torch.ones(1, dtype=torch.float64), 8)
  with pytest.raises(PcmiError, match="no CPU path"):
    PF.pair_collate(vox, torch.eye(4, dtype=torch.float64)[None])


# ---- voxelise -------------------------------------------------------------------------------------------------------------------
def check_voxelize(PF, points, sizes, voxel, flags=None, what=""):
  offs = _offs(sizes)
  want = pr.pair_voxelize(points, offs, voxel, None if flags is None else flags.copy())
  got = PF.pair_voxelize(_dev(points), _dev(offs), voxel, None if flags is None else _dev(flags))
  for k in ("n_vox", "vox_offsets", "side_offsets", "flags"):
    _same(_host(got[k]), want[k], "%s: %s" % (what, k))
  M = int(want["vox_offsets"][-1])
  for k in ("points", "coords", "first_index"):
    _same(_host(got[k])[:M], want[k], "%s: %s" % (what, k))
  return got, want


@pytest.mark.parametrize("B", [1, 2, 3])
def test_voxelize_equals_restatement(PF, B):
  rng = np.random.RandomState(20 + B)
  clouds = _clouds(rng, SIZES[B], np.float64)
  if B == 3:
    clouds[2] = np.array([-0.31, 0.27, -0.12]) + rng.uniform(0, 0.01, (65, 3))                       # all points in one voxel
    clouds[1] = (np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3)[:63] * 2 - 3.5) * V  # each its own voxel
  got, want = check_voxelize(PF, np.concatenate(clouds), SIZES[B], V, what="B %d" % B)
  assert not want["flags"].any()
  if B == 3:
    assert want["n_vox"][2] == 1 and want["n_vox"][1] == 63 and want["n_vox"][0] == 1 and want["n_vox"][5] == 0
  else:
    assert (want["n_vox"] <= np.array(SIZES[B])).all() and want["n_vox"].sum() < sum(SIZES[B])


def test_voxelize_range_edges_and_flagged_pairs(PF):
  """Voxel indices +-(2^20 - 1) are accepted, one beyond is flagged; a flagged pair yields no rows, its neighbours all of theirs."""
  v, L = 0.0625, (1 << 20) - 1  # a power of two: the products below are exact
  rng = np.random.RandomState(3)
  inner = _clouds(rng, [70, 66, 300, 290, 64, 65], np.float64)
  edge = np.array([[(L + 0.5) * v, 0.1, -0.2], [0.3, (-L + 0.5) * v, 0.0], [0.0, 0.0, (L + 0.25) * v], [(L + 0.5) * v, 0.1, -0.2]])
  clouds = [np.concatenate([inner[0], edge])] + inner[1:]
  sizes = [len(c) for c in clouds]
  got, want = check_voxelize(PF, np.concatenate(clouds), sizes, v, what="at the range")
  assert not want["flags"].any() and np.abs(want["coords"]).max() == L and want["coords"].min() == -L
  clean = want
  for beyond, flag in (([(L + 1.5) * v, 0, 0], pr.FLAG_RANGE), ([0, (-L - 0.5) * v, 0], pr.FLAG_RANGE), ([0, np.nan, 0], pr.FLAG_NONFINITE)):
    c2 = list(clouds)
    c2[3] = np.concatenate([clouds[3][:100], [beyond], clouds[3][100:]])
    sizes2 = [len(c) for c in c2]
    got, want = check_voxelize(PF, np.concatenate(c2), sizes2, v, what="beyond %s" % (beyond,))
    assert want["flags"].tolist() == [0, flag, 0]
    assert want["n_vox"].tolist() == clean["n_vox"][:2].tolist() + [0, 0] + clean["n_vox"][4:].tolist()
  # a flag the caller hands in (an earlier stage's) drops the pair as well
  pre = np.array([0, 0, pr.FLAG_NONFINITE], np.int32)
  got, want = check_voxelize(PF, np.concatenate(clouds), sizes, v, flags=pre, what="flag handed in")
  assert want["n_vox"][4:].tolist() == [0, 0] and want["n_vox"][:4].tolist() == clean["n_vox"][:4].tolist()


# ---- match ----------------------------------------------------------------------------------------------------------------------
def _star(k):
  """A source point and k targets in k different voxels, all well inside 3.5 voxels of it."""
  s = np.array([[0.5 * V] * 3]) + [0.4, -0.8, 0.2]
  g = np.stack(np.meshgrid(*[np.arange(-4, 5)] * 3, indexing="ij"), -1).reshape(-1, 3)
  centres = (g + 0.5) * V + [0.4, -0.8, 0.2]
  d = np.linalg.norm(centres - s, axis=1)
  order = np.argsort(d, kind="stable")
  assert d[order[k - 1]] < 3.3 * V
  return s, centres[order[:k]]


def check_match(PF, clouds, trans, radius, what="", capacity=None):
  sizes = [len(c) for c in clouds]
  pts, offs = np.concatenate(clouds), _offs(sizes)
  gv, wv = check_voxelize(PF, pts, sizes, V, what=what)
  want = pr.pair_match(wv, trans, radius, wv["flags"].copy())
  need = int(want["totals"][0])
  cap = need + 7 if capacity is None else capacity
  got = PF.pair_match(gv, _dev(trans), _dev(radius), cap, flags=gv["flags"].clone())
  tot = _host(got["totals"])
  assert tot.tolist() == [need, int(want["totals"][1]), 0, cap], "%s: totals %s, want %s" % (what, tot, want["totals"])
  _same(_host(got["pair_counts"]), want["pair_counts"], what + ": pair_counts")
  _same(_host(got["flags"]), want["flags"], what + ": flags")
  _same(_host(got["pairs"])[:need], want["pairs"], what + ": pairs")
  return gv, wv, got, want


def _moves(rng, B):
  T = np.tile(np.eye(4), (B, 1, 1))
  T[:, :3, :3] = _rotations(rng, B)
  T[:, :3, 3] = rng.uniform(-0.5, 0.5, (B, 3))
  return T


def _moved_pairs(rng, sizes, T):
  clouds = _clouds(rng, sizes, np.float64)
  for b in range(len(T)):  # cloud 2 b + 1 = T (cloud 2 b's pool): the search maps the sources onto it
    clouds[2 * b + 1] = clouds[2 * b + 1] @ T[b, :3, :3].T + T[b, :3, 3]
  return clouds


@pytest.mark.parametrize("B", [1, 2, 3])
def test_match_equals_restatement(PF, B):
  rng = np.random.RandomState(30 + B)
  T = _moves(rng, B)
  radius = V * MULT * rng.uniform(0.8, 1.2, B)
  gv, wv, got, want = check_match(PF, _moved_pairs(rng, SIZES[B], T), T, radius, what="B %d" % B)
  c = want["pairs"]
  assert (np.diff(c[:, 0]) >= 0).all() and not want["flags"].any()
  if B == 1:
    assert want["pair_counts"][0] > 1000
  if B == 2:  # an empty source cloud: the placeholder row at the pair's offsets
    assert want["pair_counts"].tolist()[0] == 1 and c[0].tolist() == [0, 0] and want["pair_counts"][1] > 500
  if B == 3:  # an empty target cloud
    assert want["pair_counts"][2] == 1 and c[-1].tolist() == [wv["side_offsets"][0, 2], wv["side_offsets"][1, 2]]
    assert want["totals"][1] == len(np.unique(c[:, 0]))


@pytest.mark.parametrize("k", [96, 97])
def test_match_96_matches_pass_and_97_flag(PF, k):
  rng = np.random.RandomState(41)
  T = _moves(rng, 3)
  T[1] = np.eye(4)
  T[2, :3, 3] += 40.0  # pair 2: the targets are where trans does NOT send the sources -- no match
  clouds = _moved_pairs(rng, [700, 690, 1, 1, 300, 310], T)
  clouds[5] = clouds[5] - 80.0
  clouds[2], clouds[3] = _star(k)
  radius = np.array([V * MULT, 3.5 * V, V * MULT])
  gv, wv, got, want = check_match(PF, clouds, T, radius, what="%d matches" % k)
  assert wv["n_vox"][2:4].tolist() == [1, k]
  assert want["flags"].tolist() == [0, 0 if k == 96 else pr.FLAG_MATCHES, 0]
  assert want["pair_counts"][1] == (96 if k == 96 else 0) and want["pair_counts"][2] == 1 and want["pair_counts"][0] > 300
  n0 = int(want["pair_counts"][0])
  assert want["pairs"][n0 + int(want["pair_counts"][1])].tolist() == [wv["side_offsets"][0, 2], wv["side_offsets"][1, 2]]
  if k == 97:  # the neighbours' rows and offsets are those of the run without the flag
    clouds[3] = clouds[3][:96]
    _, ok_vox, _, ok = check_match(PF, clouds, T, radius, what="96 again")
    _same(want["pairs"][:n0], ok["pairs"][:n0], "pair 0 beside a flagged pair")
    assert len(want["pairs"]) == n0 + 1 and len(ok["pairs"]) == n0 + 96 + 1
    assert wv["side_offsets"][:, 2].tolist() == (ok_vox["side_offsets"][:, 2] + [0, 1]).tolist()  # its voxels still count


def test_match_capacity_exact_and_one_short(PF):
  rng = np.random.RandomState(51)
  T = _moves(rng, 2)
  clouds = _moved_pairs(rng, [900, 880, 400, 410], T)
  radius = np.full(2, V * MULT)
  gv, wv, _, want = check_match(PF, clouds, T, radius, what="roomy")
  need = int(want["totals"][0])
  for cap in (need, need - 1):
    buf = torch.full((need + 64, 2), -7, dtype=torch.int32, device=DEV)
    fl = gv["flags"].clone()
    got = PF.pair_match(gv, _dev(T), _dev(radius), cap, flags=fl, pairs=buf)
    assert _host(got["totals"]).tolist() == [need, int(want["totals"][1]), int(cap < need), cap]
    _same(_host(got["pair_counts"]), want["pair_counts"], "pair_counts at capacity %d" % cap)
    rows = _host(buf)
    if cap == need:
      _same(rows[:need], want["pairs"], "pairs at the exact capacity")
      assert (rows[need:] == -7).all()
    else:
      assert (rows == -7).all(), "an overflowing call must write nothing"
      # the fill alone, with the room the count asked for, on what that call left in the workspace
      again = PF.pair_match(gv, _dev(T), _dev(radius), need, flags=fl, pairs=buf, fill_only=True)
      assert _host(again["totals"]).tolist() == [need, int(want["totals"][1]), 0, need]
      _same(_host(again["pair_counts"]), want["pair_counts"], "pair_counts after the fill alone")
      _same(_host(buf)[:need], want["pairs"], "pairs after the fill alone")
      assert (_host(buf)[need:] == -7).all()


# ---- collate --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 3])
def test_collate_equals_restatement(PF, B):
  rng = np.random.RandomState(60 + B)
  clouds = _clouds(rng, SIZES[B], np.float64)
  pts, sizes = np.concatenate(clouds), SIZES[B]
  gv, wv = check_voxelize(PF, pts, sizes, V, what="collate B %d" % B)
  T = _moves(rng, B)
  noise = rng.standard_normal((len(pts), 3)).astype(np.float32)
  on = (np.arange(2 * B) % 3 != 1)
  for nz, mu, sigma in ((noise, 0.0, 0.01), (noise, 0.25, 0.5), (None, 0.0, 0.01)):
    want = pr.pair_collate(wv, T, nz, on, mu, sigma)
    got = PF.pair_collate(gv, _dev(T), None if nz is None else _dev(nz), _dev(on.astype(np.int32)), mu, sigma)
    for key, w in want.items():
      g = _host(got[key])
      _same(g if key == "T_gt" else g[:len(w)], w, "B %d: %s" % (B, key))


# ---- pipeline -------------------------------------------------------------------------------------------------------------------
def _draws(rng, frames, jitter=True):
  from pointcontrast_amd.lib.pair_input import PairDraws
  B = len(frames)
  n = sum(len(a) for f in frames for a in f)
  d = PairDraws(rng.uniform(0.8, 1.2, B), _rotations(rng, 2 * B), np.arange(2 * B) % 3 != 1 if jitter else np.zeros(2 * B, bool))
  d.noise = _dev(rng.standard_normal((n, 3)).astype(np.float32))
  return d


def _ref_batch(frames, d, **kw):
  return pr.pipeline(frames, d.scale, d.rot, d.jitter_on, None if d.noise is None else _host(d.noise), V, MULT, **kw)


def _same_batch(got, want, what):
  assert set(got) == set(want), (sorted(got), sorted(want))
  for k, w in want.items():
    if k in ("len_batch", "n_queries"):
      assert got[k] == w and type(got[k]) is type(w), "%s: %s %r, want %r" % (what, k, got[k], w)
    else:
      assert got[k].is_cuda
      _same(_host(got[k]), w, "%s: %s" % (what, k))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pipeline_equals_restatement(PF, dtype):
  from pointcontrast_amd.lib.pair_input import PairInputPipeline
  frames = make_frames(4, n_pairs=3, dtype=dtype)
  frames[1] = (frames[1][0], frames[1][1] + dtype(30.0))  # no match: the placeholder row
  d = _draws(np.random.RandomState(8), frames)
  want = _ref_batch(frames, d)
  pipe = PairInputPipeline(V, MULT)
  got = pipe(frames, d)
  assert pipe.last_readbacks == 1
  _same_batch(got, want, "pipeline %s" % dtype.__name__)
  again = pipe(frames, d)
  assert pipe.last_readbacks == 1
  for k, w in got.items():
    assert again[k] == w if k in ("len_batch", "n_queries") else torch.equal(again[k], w), "second call: %s" % k
  # too little room for the correspondences: one retry, the same batch
  small = PairInputPipeline(V, MULT, match_capacity=10)
  retried = small(frames, d)
  assert small.last_readbacks == 2
  _same_batch(retried, want, "after the retry")
  assert small(frames, d)["n_queries"] == want["n_queries"] and small.last_readbacks == 1


def test_pipeline_identity_equals_the_per_item_device_path(PF):
  from pointcontrast_amd.lib import device_loader, synthetic
  from pointcontrast_amd.lib.pair_input import PairDraws, PairInputPipeline
  frames = make_frames(6, n_pairs=2)
  got = PairInputPipeline(V, MULT, random_rotation=False, jitter=None)(frames, PairDraws.identity(2))
  items = []
  for a, b in frames:
    g = device_loader.pair_geometry_device(a, b, np.eye(4), V, V * MULT)
    x0, x1 = _host(g["xyz0"]), _host(g["xyz1"])
    items.append((x0, x1, _host(g["coords0"]), _host(g["coords1"]), np.ones((len(x0), 3)), np.ones((len(x1), 3)),
                  _host(g["matches"]).astype(np.int64), np.eye(4)))
  want = synthetic.collate_pairs(items)
  want["n_queries"] = len(np.unique(want["correspondences"][:, 0]))
  _same_batch(got, want, "identity draws")


def test_pipeline_raises_for_a_flagged_pair(PF):
  from pointcontrast_amd._lib import PcmiError
  from pointcontrast_amd.lib.pair_input import PairDraws, PairInputPipeline
  frames = make_frames(6, n_pairs=3)
  bad = frames[2][1].copy()
  bad[3, 0] = np.nan
  with pytest.raises(PcmiError, match=r"pair 2: a point is not finite"):
    PairInputPipeline(V, MULT)([frames[0], frames[1], (frames[2][0], bad)], _draws(np.random.RandomState(1), frames, jitter=False))


# ---- trainers and loader --------------------------------------------------------------------------------------------------------
def _trainer_cfg(tmp_path, extra=()):
  return config(tmp_path, ["net.model=Res16UNet14", "misc.nceT=0.4", "misc.npos=256", "opt.lr=0.1", "misc.prefetch=False",
                           "trainer.num_pos_per_batch=128", "trainer.num_hn_samples_per_batch=64"] + list(extra))


def _two_batches(frames):
  from pointcontrast_amd.lib.pair_input import PairInputPipeline
  d = _draws(np.random.RandomState(12), frames)
  dev = PairInputPipeline(V, MULT)(frames, d)
  ref = _ref_batch(frames, d)
  nq = ref.pop("n_queries")
  assert nq == dev["n_queries"]
  host = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in ref.items()}
  return dev, host, nq


def _step(Trainer, cfg, batch, draws):
  from pointcontrast_amd.lib.ddp_data_loaders import FixedBatchLoader
  from pointcontrast_amd.lib.timer import AverageMeter, Timer
  torch.manual_seed(0)
  tr = Trainer(cfg, FixedBatchLoader([batch], batch_size=2))
  prep = tr._prepare(batch, draws)
  res = tr._train_iter(iter(tr.data_loader), [AverageMeter(), Timer(), Timer()], draws=draws)
  torch.cuda.synchronize()
  return tr, prep, {k: v.detach().cpu() for k, v in res.items()}


def test_nce_trainer_device_batch_equals_host_batch(PF, tmp_path):
  from pointcontrast_amd.lib.ddp_trainer import PointNCELossTrainer
  frames = make_frames(5, n_pairs=2, n=1500)
  write_corpus(tmp_path, frames)
  dev, host, nq = _two_batches(frames)
  rng = np.random.RandomState(2)
  assert nq > 256
  draws = dict(uniform=torch.from_numpy(rng.rand(nq).astype(np.float32)), sampled_inds=rng.choice(nq, 256, replace=False))
  cfg = _trainer_cfg(tmp_path)
  _, pd, rd = _step(PointNCELossTrainer, cfg, dev, draws)
  _, ph, rh = _step(PointNCELossTrainer, cfg, host, draws)
  assert torch.equal(pd["q_idx"].cpu(), ph["q_idx"].cpu()) and torch.equal(pd["k_idx"].cpu(), ph["k_idx"].cpu())
  print("NCE loss from the device batch %r, from the host batch %r" % (float(rd["loss"]), float(rh["loss"])))
  assert torch.equal(rd["loss"].view(torch.int32), rh["loss"].view(torch.int32)), "the losses differ although the inputs are equal"


def test_hardest_trainer_device_batch_equals_host_batch(PF, tmp_path):
  from pointcontrast_amd.lib.ddp_trainer import HardestContrastiveLossTrainer
  frames = make_frames(5, n_pairs=2, n=1500)
  write_corpus(tmp_path, frames)
  dev, host, _ = _two_batches(frames)
  N0, N1, P = host["sinput0_C"].shape[0], host["sinput1_C"].shape[0], host["correspondences"].shape[0]
  rng = np.random.RandomState(3)
  assert P > 256 and min(N0, N1) > 128
  draws = dict(sel0=rng.choice(N0, 128, replace=False), sel1=rng.choice(N1, 128, replace=False), pos_sel=rng.choice(P, 256, replace=False))
  cfg = _trainer_cfg(tmp_path)
  _, _, rd = _step(HardestContrastiveLossTrainer, cfg, dev, draws)
  _, _, rh = _step(HardestContrastiveLossTrainer, cfg, host, draws)
  for k in ("loss", "pos_loss", "neg_loss"):
    print("hardest-contrastive %s from the device batch %r, from the host batch %r" % (k, float(rd[k]), float(rh[k])))
    assert torch.equal(rd[k].view(torch.int32), rh[k].view(torch.int32)), "%s differs although the inputs are equal" % k


@pytest.mark.parametrize("threads", [0, 2])
def test_device_pair_loader_feeds_the_trainer(PF, tmp_path, threads):
  from pointcontrast_amd.lib.ddp_data_loaders import make_data_loader
  from pointcontrast_amd.lib.ddp_trainer import PointNCELossTrainer
  from pointcontrast_amd.lib.pair_input import DevicePairLoader
  from pointcontrast_amd.lib.timer import AverageMeter, Timer
  write_corpus(tmp_path, make_frames(13, n_pairs=3, n=1500))
  cfg = _trainer_cfg(tmp_path, ["data.device_batch=True", "misc.train_num_thread=%d" % threads, "trainer.use_random_scale=True"])
  loader = make_data_loader(cfg, 2, num_threads=cfg.misc.train_num_thread)
  assert isinstance(loader, DevicePairLoader) and loader.batch_size == 2 and loader.loader.num_workers == threads
  it = iter(loader)
  for _ in range(3):  # more than one epoch of the three pairs
    batch = next(it)
    assert batch["sinput0_C"].is_cuda and batch["sinput0_C"].shape[1] == 4 and len(batch["len_batch"]) == 2
    c0 = batch["correspondences"][:, 0]
    assert len(c0) > 100 and bool((c0[1:] >= c0[:-1]).all()) and batch["n_queries"] == len(torch.unique(c0))
  torch.manual_seed(0)
  tr = PointNCELossTrainer(cfg, loader)
  res = tr._train_iter(it, [AverageMeter(), Timer(), Timer()])
  assert np.isfinite(float(res["loss"]))
  loader.close()
