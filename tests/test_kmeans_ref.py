"""tests/kmeans_ref.py (the restatement tests/test_gpu_kmeans.py holds the device to, bit for bit) held to independent ground
on the CPU: the assignment against a float64 argmin, the fixed-point sums against Python big integers, the seeding against
np.cumsum + np.searchsorted, a planted partition, and the rules for empty and dead clusters and inactive rows."""
import math

import numpy as np

import kmeans_ref as kr


def test_fma_chain_is_a_single_rounding():
  # Python's float arithmetic on exact rationals: fma(x, y, z) rounded once to fp32
  from fractions import Fraction
  rng = np.random.default_rng(0)
  x = rng.normal(size=2000).astype(np.float32)
  z = np.abs(rng.normal(size=2000)).astype(np.float32) * np.float32(3.0)
  # force ties of the float64 sum: z far above x * x so that the low bits of the product fall below float64's last place
  z[:500] = (z[:500] * np.float32(2.0 ** 30)).astype(np.float32)
  got = kr.fma32(x, x, z)
  for i in range(len(x)):
    exact = Fraction(float(x[i])) ** 2 + Fraction(float(z[i]))
    lo = np.float32(float(exact))  # float(Fraction) rounds once to float64: only a bracket, refined below
    cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
    errs = [abs(Fraction(float(c)) - exact) for c in cands]
    best = min(errs)
    winners = [c for c, e in zip(cands, errs) if e == best]
    if len(winners) == 2:  # a true tie: to even
      winners = [c for c in winners if (int(np.float32(c).view(np.int32)) & 1) == 0]
    assert got[i] == winners[0], (i, x[i], z[i], got[i], winners)


def test_assignment_is_the_float64_argmin():
  rng = np.random.default_rng(1)
  lens, K, C = [70, 0, 33], 5, 16
  offs = kr.offsets_of(lens)
  feat = rng.normal(size=(offs[-1], C)).astype(np.float32)
  cen = rng.normal(size=(3, K, C)).astype(np.float32)
  live = np.zeros((3, K), dtype=np.int32)
  live[2, 1] = -1
  out = kr.kmeans_assign(feat, offs, cen, live)
  for b in range(3):
    for i in range(offs[b], offs[b + 1]):
      d = ((feat[i].astype(np.float64) - cen[b].astype(np.float64)) ** 2).sum(1)
      d[live[b] < 0] = np.inf
      gap = np.sort(d)[1] - np.sort(d)[0]
      assert gap > 1e-4 * d.min(), "the case must not sit within fp32 rounding of a tie"
      assert out["assign"][i] == int(d.argmin())
      assert abs(float(out["d2"][i]) - d.min()) <= 1e-5 * d.min()
  # the corrected chain and featmatch_ref's agree to one ulp everywhere
  a, b2 = kr.dist2(feat[:70], cen[0]), kr.dist2_f32(feat[:70], cen[0])
  assert (np.abs(a.view(np.int32) - b2.view(np.int32)) <= 1).all()


def test_sums_are_python_big_integer_sums():
  rng = np.random.default_rng(2)
  n, K, C = 300, 3, 16
  feat = (rng.normal(size=(n, C)) * 50).astype(np.float32)
  feat[0] = 1024.0    # the largest magnitude an active row may hold
  feat[1] = -1024.0
  feat[2, 0] = 2.0 ** -8 + 2.0 ** -31  # still exact at 2^-32
  offs = np.array([0, n], dtype=np.int64)
  cen, live, _ = kr.kmeans_init(feat, offs, np.array([[5, 6, 7]], dtype=np.int32))
  st = kr.kmeans_step(feat, offs, cen, live)
  for k in range(K):
    rows = np.flatnonzero(st["assign"] == k)
    assert st["cnt"][0, k] == len(rows)
    for c in range(C):
      big = sum(int(round(float(feat[i, c]) * 2 ** 32)) for i in rows)  # exact: a float times 2^32 is a float
      assert int(st["sum"][0, k, c]) == big
      want = np.float32(np.float64(big) / (np.float64(len(rows)) * 4294967296.0))
      assert st["centroid"][0, k, c] == want
  assert int(round(float(feat[2, 0]) * 2 ** 32)) == 2 ** 24 + 2  # nothing was lost to the quantum
  assert int(st["changed"][0]) == n and int(st["skipped"][0]) == 0
  st2 = kr.kmeans_step(feat, offs, cen, live, st["assign"])
  assert int(st2["changed"][0]) == 0


def test_seeding_is_cumsum_and_searchsorted():
  rng = np.random.default_rng(3)
  lens, C = [200, 1, 0, 77], 16
  offs = kr.offsets_of(lens)
  feat = rng.normal(size=(offs[-1], C)).astype(np.float32)
  feat[13, 2] = np.nan  # an inactive row weighs nothing
  draws = rng.integers(0, 2 ** 64, size=4, dtype=np.uint64)
  mind2 = np.full(len(feat), np.inf, dtype=np.float32)
  first, mind2 = kr.kmeans_pp_step(feat, offs, mind2, None, draws)
  # the first step: uniform over the active rows
  act0 = [i for i in range(200) if i != 13]
  assert first[0] == act0[(len(act0) * int(draws[0])) >> 64] and first[1] == 200 and first[2] == -1
  assert first[3] == 201 + ((77 * int(draws[3])) >> 64)
  nxt, mind2 = kr.kmeans_pp_step(feat, offs, mind2, first, draws[::-1].copy())
  for b in (0, 3):
    lo, hi = offs[b], offs[b + 1]
    d = ((feat[lo:hi].astype(np.float64) - feat[first[b]].astype(np.float64)) ** 2).sum(1)
    w = np.floor(np.minimum(mind2[lo:hi].astype(np.float64), 2.0 ** 20) * 2.0 ** 20)
    w[~np.isfinite(d)] = 0
    assert np.allclose(mind2[lo:hi][np.isfinite(d)], d[np.isfinite(d)], rtol=1e-5)
    total = int(sum(int(x) for x in w))
    target = (total * int(draws[::-1][b])) >> 64
    assert nxt[b] == lo + np.searchsorted(np.cumsum(w.astype(np.uint64)), np.uint64(target), side="right")
    assert nxt[b] != first[b] and nxt[b] != 13
  assert nxt[1] == 200 and nxt[2] == -1  # one row: no weight left, the lowest active row; no row: -1


def test_planted_blobs_are_recovered():
  K, per, C = 8, 48, 16
  feat, label = kr.blobs(K, per, C, seed=7)
  centres = np.stack([feat[label == k].mean(0) for k in range(K)])
  sep = min(np.linalg.norm(centres[i] - centres[j]) for i in range(K) for j in range(i))
  assert sep >= 20 * 0.05
  offs = np.array([0, len(feat)], dtype=np.int64)
  draws = np.random.default_rng(7).integers(0, 2 ** 64, size=(1, K), dtype=np.uint64)
  out = kr.kmeans_select(feat, offs, K, draws, iters=4)
  # the partition is the planted one up to the numbering, and one annotated row falls into every blob
  pairs = set(zip(out["assign"].tolist(), label.tolist()))
  assert len(pairs) == K and len({a for a, _ in pairs}) == K and len({l for _, l in pairs}) == K
  assert sorted(label[out["rows"][0]].tolist()) == list(range(K))
  assert out["cnt"].tolist() == [[per] * K] and int(out["changed"][-1, 0]) == 0
  assert math.isclose(out["inertia"][0], float(out["d2"].astype(np.float64).sum()), rel_tol=1e-12)


def test_empty_cluster_keeps_its_centroid():
  feat = np.zeros((6, 16), dtype=np.float32)
  feat[:3, 0], feat[3:, 0] = 1.0, 2.0
  offs = np.array([0, 6], dtype=np.int64)
  cen = np.zeros((1, 3, 16), dtype=np.float32)
  cen[0, :, 0] = [1.0, 2.0, 9.0]  # nobody is nearest to the third
  live = np.zeros((1, 3), dtype=np.int32)
  st = kr.kmeans_step(feat, offs, cen, live)
  assert st["cnt"].tolist() == [[3, 3, 0]] and np.array_equal(st["centroid"][0, 2], cen[0, 2])
  fin = kr.kmeans_assign(feat, offs, st["centroid"], live)
  assert fin["nearest"].tolist() == [[0, 3, -1]] and fin["inertia"][0] == 0.0


def test_dead_clusters_and_inactive_rows():
  rng = np.random.default_rng(5)
  feat = rng.normal(size=(40, 16)).astype(np.float32)
  feat[4, 1], feat[5, 2], feat[6, 3] = np.nan, np.inf, 1024.5
  feat[7, 3] = -1024.0  # still active
  offs = np.array([0, 25, 40], dtype=np.int64)
  init = np.array([[0, -1, 4, 30], [26, 27, 28, 29]], dtype=np.int32)  # dead, inactive, outside its scene
  cen, live, flags = kr.kmeans_init(feat, offs, init)
  assert live.tolist() == [[0, -1, -1, -1], [26, 27, 28, 29]] and flags.tolist() == [2, 0]
  assert not cen[0, 1:].any()
  st = kr.kmeans_step(feat, offs, cen, live)
  assert st["skipped"].tolist() == [3, 0] and (st["assign"][[4, 5, 6]] == -1).all() and st["assign"][7] == 0
  assert (st["assign"][:25][[i for i in range(25) if i not in (4, 5, 6)]] == 0).all()
  assert not st["centroid"][0, 1:].any() and st["cnt"][0].tolist() == [22, 0, 0, 0]
  fin = kr.kmeans_assign(feat, offs, st["centroid"], live)
  assert np.isnan(fin["d2"][[4, 5, 6]]).all() and not set(fin["nearest"].ravel().tolist()) & {4, 5, 6}
  assert fin["nearest"][0, 1:].tolist() == [-1, -1, -1]
  # a scene cut to its first rows: the rest lies in no scene and is counted with the skipped rows (15 + 3 inactive, 5)
  cut = kr.kmeans_assign(feat, offs, st["centroid"], live, max_rows=10)
  assert (cut["assign"][10:25] == -1).all() and (cut["assign"][35:] == -1).all() and cut["skipped"].tolist() == [18, 5]


def test_inertia_order_is_the_stated_tree():
  rng = np.random.default_rng(6)
  v = rng.uniform(0, 1, 700)
  parts = []
  for p in range(3):
    x = np.zeros(256)
    chunk = v[256 * p:256 * (p + 1)]
    x[:len(chunk)] = chunk
    waves = []
    for w in range(4):
      lane = list(x[64 * w:64 * (w + 1)])
      for d in (1, 2, 4, 8, 16, 32):
        lane = [lane[i] + lane[i ^ d] for i in range(64)]
      assert len(set(lane)) == 1
      waves.append(lane[0])
    parts.append(((waves[0] + waves[1]) + waves[2]) + waves[3])
  lanes = [0.0] * 256
  for p, s in enumerate(parts):
    lanes[p] += s
  # (adding 0.0 lanes changes nothing, so the final block sum is the sum of three lanes through the same tree)
  assert kr.inertia_of(v) == kr.block_sum(np.array(lanes))
  assert kr.inertia_of(np.zeros(0)) == 0.0
