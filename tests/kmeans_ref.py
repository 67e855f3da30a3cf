"""numpy restatement of csrc/kmeans.hip under exactly the rules of include/pcmi.h (pcmi_kmeans_init / _step / _assign /
_pp_step) and of functional.kmeans_pp_init / kmeans_select on top of them.  tests/test_kmeans_ref.py holds it to independent
ground (float64 argmin, Python big integers, np.cumsum + np.searchsorted, a planted partition); tests/test_gpu_kmeans.py holds
the device to it BIT for bit.

The fp32 chain d2 = fma(a_c - b_c, a_c - b_c, d2) is restated exactly here: featmatch_ref.dist2_f32 rounds the float64 sum
to fp32 a second time, which in rare cases is one ulp off a true FMA; fma32 below repairs the float64 sum to round-to-odd
first (53 >= 2 * 24 + 2 bits: the second rounding is then the FMA's single one).  Sums and seeding weights are integers."""
import numpy as np

from featmatch_ref import dist2_f32  # the uncorrected chain: test_kmeans_ref.py compares the two

CLAMP = np.float32(1024.0)
FIX = 4294967296.0  # 2^32
MAX_K, MAX_SCENE_ROWS = 1024, 1 << 20
W_CAP, W_FIX = np.float32(1048576.0), 1048576.0  # the seeding weight: floor(min(mind2, 2^20) 2^20)
PART = 256


def offsets_of(lengths):
  out = np.zeros(len(lengths) + 1, dtype=np.int64)
  np.cumsum(np.asarray(lengths, dtype=np.int64), out=out[1:])
  return out


def fma32(x, y, z):
  """fp32 fma(x, y, z) for fp32 arrays: the product is exact in float64; the float64 sum is repaired to round-to-odd."""
  p = x.astype(np.float64) * y.astype(np.float64)
  z = z.astype(np.float64)
  with np.errstate(invalid="ignore", over="ignore"):
    s = p + z
    bb = s - p
    err = (p - (s - bb)) + (z - bb)  # TwoSum: s + err == p + z exactly
  fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
  toward = np.where(err > 0, np.inf, -np.inf)
  s = np.where(fix, np.nextafter(s, toward), s)
  with np.errstate(over="ignore"):
    return s.astype(np.float32)


def dist2(a, b):
  """[len(a), len(b)] in the device's chain, exactly."""
  a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
  acc = np.zeros((len(a), len(b)), dtype=np.float32)
  with np.errstate(invalid="ignore", over="ignore"):
    for c in range(a.shape[1]):
      df = a[:, None, c] - b[None, :, c]
      acc = fma32(df, df, acc)
  return acc


def scenes(offs, n, max_rows=None):
  """[(lo, hi)] per scene: the segment clamped into [0, n] and cut to its first max_rows rows."""
  offs = np.asarray(offs, dtype=np.int64)
  out = []
  for b in range(len(offs) - 1):
    lo = int(np.clip(offs[b], 0, n))
    hi = int(np.clip(offs[b + 1], lo, n))
    if max_rows is not None:
      hi = min(hi, lo + int(max_rows))
    out.append((lo, hi))
  return out


def row_ok(feat):
  """Per row: every channel has |x| <= 1024 (false for NaN and infinities)."""
  with np.errstate(invalid="ignore"):
    return (np.abs(np.asarray(feat, dtype=np.float32)) <= CLAMP).all(1)


def quantise(x):
  return np.rint(np.asarray(x, dtype=np.float32).astype(np.float64) * FIX).astype(np.int64)


def kmeans_init(feat, offs, init_rows, max_rows=None):
  feat = np.asarray(feat, dtype=np.float32)
  rows = np.asarray(init_rows, dtype=np.int32)
  B, K = rows.shape
  ok = row_ok(feat)
  cen = np.zeros((B, K, feat.shape[1]), dtype=np.float32)
  live = np.full((B, K), -1, dtype=np.int32)
  flags = np.zeros(B, dtype=np.int64)
  for b, (lo, hi) in enumerate(scenes(offs, len(feat), max_rows)):
    for k in range(K):
      r = int(rows[b, k])
      if lo <= r < hi and ok[r]:
        cen[b, k], live[b, k] = feat[r], r
      elif r >= 0:
        flags[b] += 1
  return cen, live, flags


def _assign(feat, offs, cen, live, max_rows):
  """assign [n], d2 [n], skipped [B] by the assignment rule."""
  feat, cen = np.asarray(feat, dtype=np.float32), np.asarray(cen, dtype=np.float32)
  n, (B, K, _) = len(feat), cen.shape
  assign, d2 = np.full(n, -1, dtype=np.int32), np.full(n, np.nan, dtype=np.float32)
  skipped = np.zeros(B, dtype=np.int64)
  ok = row_ok(feat)
  whole = scenes(offs, n)
  for b, (lo, hi) in enumerate(scenes(offs, n, max_rows)):
    skipped[b] = int((~ok[lo:hi]).sum()) + (whole[b][1] - hi)  # the inactive rows and the rows max_rows cut off
    act = lo + np.flatnonzero(ok[lo:hi])
    ks = np.flatnonzero(np.asarray(live)[b] >= 0)
    if len(act) == 0 or len(ks) == 0:
      continue
    D = dist2(feat[act], cen[b, ks]).astype(np.float64)
    D[~np.isfinite(D)] = np.inf
    j = D.argmin(1)  # the first among equals: the lowest k
    best = D[np.arange(len(j)), j]
    fin = np.isfinite(best)
    assign[act[fin]] = ks[j[fin]].astype(np.int32)
    d2[act[fin]] = best[fin].astype(np.float32)
  return assign, d2, skipped


def kmeans_step(feat, offs, cen, live, assign_prev=None, max_rows=None):
  feat, cen = np.asarray(feat, dtype=np.float32), np.asarray(cen, dtype=np.float32)
  n, (B, K, C) = len(feat), cen.shape
  assign, _, skipped = _assign(feat, offs, cen, live, max_rows)
  prev = np.full(n, -1, dtype=np.int32) if assign_prev is None else np.asarray(assign_prev, dtype=np.int32)
  q = quantise(np.where(row_ok(feat)[:, None], feat, np.float32(0)))  # (only assigned rows are ever summed)
  s, cnt = np.zeros((B, K, C), dtype=np.int64), np.zeros((B, K), dtype=np.int32)
  changed = np.zeros(B, dtype=np.int64)
  out = np.zeros_like(cen)
  for b, (lo, hi) in enumerate(scenes(offs, n, max_rows)):
    a = assign[lo:hi]
    changed[b] = int((a != prev[lo:hi]).sum())
    for k in range(K):
      if live[b, k] < 0:
        continue
      m = lo + np.flatnonzero(a == k)
      cnt[b, k] = len(m)
      s[b, k] = q[m].sum(0)
      if len(m):
        out[b, k] = (s[b, k].astype(np.float64) / (np.float64(len(m)) * FIX)).astype(np.float32)
      else:
        out[b, k] = cen[b, k]
  return dict(assign=assign, sum=s, cnt=cnt, centroid=out, changed=changed, skipped=skipped)


def butterfly64(v):
  """[..., 64] -> [...]: v += v[lane ^ d] for d = 1 ... 32 (every lane ends with the same pairwise tree)."""
  v = np.asarray(v, dtype=np.float64)
  while v.shape[-1] > 1:
    v = v[..., 0::2] + v[..., 1::2]
  return v[..., 0]


def block_sum(v256):
  """[..., 256] -> [...]: a butterfly per wave of 64, the four waves in ascending order."""
  w = butterfly64(np.asarray(v256, dtype=np.float64).reshape(v256.shape[:-1] + (4, 64)))
  return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def inertia_of(vals):
  """The fixed-order fp64 sum of one scene's values (non-members as 0)."""
  vals = np.asarray(vals, dtype=np.float64)
  np_ = (len(vals) + PART - 1) // PART
  padded = np.zeros(max(np_, 1) * PART, dtype=np.float64)
  padded[:len(vals)] = vals
  parts = block_sum(padded.reshape(-1, PART))[:np_]
  lanes = np.zeros(PART, dtype=np.float64)
  for p in range(np_):  # lane t adds the partials t, t + 256, ... in that order
    lanes[p % PART] = lanes[p % PART] + parts[p]
  return float(block_sum(lanes))


def kmeans_assign(feat, offs, cen, live, max_rows=None):
  feat = np.asarray(feat, dtype=np.float32)
  n, (B, K, _) = len(feat), np.asarray(cen).shape
  assign, d2, skipped = _assign(feat, offs, cen, live, max_rows)
  nearest, cnt = np.full((B, K), -1, dtype=np.int32), np.zeros((B, K), dtype=np.int32)
  inertia = np.zeros(B, dtype=np.float64)
  for b, (lo, hi) in enumerate(scenes(offs, n, max_rows)):
    a = assign[lo:hi]
    for k in range(K):
      m = lo + np.flatnonzero(a == k)
      cnt[b, k] = len(m)
      if len(m):
        nearest[b, k] = m[np.argmin(d2[m].astype(np.float64))]  # the first among equals: the lowest row
    inertia[b] = inertia_of(np.where(a >= 0, d2[lo:hi].astype(np.float64), 0.0))
  return dict(assign=assign, d2=d2, nearest=nearest, inertia=inertia, cnt=cnt, skipped=skipped)


def seed_weights(mind2, ok):
  """uint64 weights as Python-exact integers in an int64 array (<= 2^40 each)."""
  m = np.fmin(np.asarray(mind2, dtype=np.float32), W_CAP).astype(np.float64) * W_FIX
  return np.where(ok, np.floor(m), 0.0).astype(np.int64)


def kmeans_pp_step(feat, offs, mind2, last, draw, max_rows=None):
  """Returns (next int32 [B], the lowered mind2)."""
  feat = np.asarray(feat, dtype=np.float32)
  mind2 = np.array(mind2, dtype=np.float32)
  n = len(feat)
  sc = scenes(offs, n, max_rows)
  nxt = np.full(len(sc), -1, dtype=np.int32)
  ok = row_ok(feat)
  for b, (lo, hi) in enumerate(sc):
    ctr = -1 if last is None else int(last[b])
    act = lo + np.flatnonzero(ok[lo:hi])
    if lo <= ctr < hi and ok[ctr] and len(act):
      d = dist2(feat[act], feat[ctr:ctr + 1])[:, 0]
      with np.errstate(invalid="ignore"):
        keep = mind2[act] <= d
      mind2[act] = np.where(keep, mind2[act], d)
    if len(act) == 0:
      continue
    w = seed_weights(mind2[lo:hi], ok[lo:hi])
    total = int(w.sum())
    if total == 0:
      nxt[b] = act[0]
      continue
    target = (total * int(np.uint64(draw[b]))) >> 64
    cum = np.cumsum(w)
    nxt[b] = lo + int(np.searchsorted(cum, target, side="right"))
  return nxt, mind2


def as_u64(draws):
  a = np.asarray(draws)
  return a.view(np.uint64) if a.dtype == np.int64 else a.astype(np.uint64)


def kmeans_pp_init(feat, offs, K, draws, max_rows=None):
  draws = as_u64(draws)
  mind2 = np.full(len(feat), np.inf, dtype=np.float32)
  picks, last = [], None
  for k in range(K):
    last, mind2 = kmeans_pp_step(feat, offs, mind2, last, draws[:, k], max_rows)
    picks.append(last)
  rows = np.stack(picks, 1)
  for b in range(rows.shape[0]):
    seen = set()
    for k in range(K):
      if int(rows[b, k]) in seen:
        rows[b, k] = -1
      else:
        seen.add(int(rows[b, k]))
  return rows


def kmeans_select(feat, offs, K, draws=None, iters=10, init_rows=None, max_rows=None):
  if init_rows is None:
    init_rows = kmeans_pp_init(feat, offs, K, draws, max_rows)
  cen, live, _ = kmeans_init(feat, offs, init_rows, max_rows)
  prev, changed = None, []
  for _ in range(iters):
    st = kmeans_step(feat, offs, cen, live, prev, max_rows)
    cen, prev = st["centroid"], st["assign"]
    changed.append(st["changed"])
  fin = kmeans_assign(feat, offs, cen, live, max_rows)
  return dict(rows=fin["nearest"], assign=fin["assign"], centroid=cen, cnt=fin["cnt"], inertia=fin["inertia"],
              changed=np.stack(changed) if changed else np.zeros((0, len(offs) - 1), dtype=np.int64), skipped=fin["skipped"],
              live=live, d2=fin["d2"])


def blobs(K, per, C, seed, sigma=0.05, sep=100.0):
  """K planted blobs of `per` rows each in C dimensions: centres on a lattice of pitch sep * sigma (every two centres at
  least sep sigma >= 20 sigma apart), Gaussian noise of sigma per channel clipped at 4 sigma, rows shuffled.  Returns
  (feat, label)."""
  assert sep >= 20.0
  rng = np.random.default_rng(seed)
  pitch = sep * sigma
  side = int(np.ceil(K ** (1.0 / 3.0)))
  grid = np.array([(i // (side * side), (i // side) % side, i % side) for i in range(K)], dtype=np.float64)
  centres = np.zeros((K, C))
  centres[:, :3] = grid * pitch
  label = np.repeat(np.arange(K), per)
  x = centres[label] + np.clip(rng.normal(0.0, sigma, (K * per, C)), -4 * sigma, 4 * sigma)
  perm = rng.permutation(len(x))
  return x[perm].astype(np.float32), label[perm].astype(np.int32)
