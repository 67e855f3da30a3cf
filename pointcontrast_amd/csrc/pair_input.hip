// The input of contrastive pre-training for a BATCH of frame pairs, on the device: what the reference runs per item on the
// host in pretrain/pointcontrast/lib/ddp_data_loaders.py --
//   * random scale, random rotation about the centroid, trans = T1 inv(T0)                     (:196-225)
//   * ME.utils.sparse_quantize(xyz / voxel_size, return_index=True) of both frames, floor      (:228-239, :258-259)
//   * get_matching_indices within voxel_size * multiplier * scale                             (:36-49, :241)
//   * FeatureJitter and default_collate_pair_fn                                                (:52-112, :248-252)
//   * and, where the reference has its "#dummy color" (:204-206, :248-249), the features of a corpus with colours
// Written from the semantics in include/pcmi.h; gfx950, wave64.  Every random quantity is an input.  A batch of B pairs is
// 2 B clouds in one row-major array; every kernel launches over all rows of the batch and looks its segment up.
//
// Arithmetic, as loader.hip and semseg_input.hip: every fp64 product and sum is an explicit round-to-nearest operation in the
// order pcmi.h states (no FMA contraction).  The only atomics are integer ones whose result does not depend on the order of
// arrival (min, or, add), the compare-and-swap that claims a table slot and the exchange that links a target into its cell's
// list -- neither of which reaches an output: voxels leave in the order of an exclusive scan, matches are sorted per source.
#include <algorithm>
#include <climits>

#include "cubscan.h"
#include "exact.h"
#include "firstrow.h"
#include "internal.h"

#pragma clang fp contract(off)

namespace pcmi {
namespace pairinput {

constexpr int kThreads = 256;
constexpr int kMaxPairs = PCMI_PAIR_MAX_PAIRS;
constexpr int kChunk = PCMI_PAIR_CENTROID_CHUNK;
constexpr int kPerThread = kChunk / kThreads;
constexpr int64_t kMaxRows = 1ll << 29;  // segmented tables of 2 n + 2 B slots, addressed with 32 bits

static_assert(kChunk % kThreads == 0 && (kThreads & (kThreads - 1)) == 0, "one workgroup sums a chunk: whole rounds, then a binary tree");

__device__ inline int64_t chunks_of(int64_t rows) { return (rows + kChunk - 1) / kChunk; }

__device__ inline double raw_at(const void* __restrict__ raw, int f32, int64_t k) {
  return f32 ? (double)((const float*)raw)[k] : ((const double*)raw)[k];
}

// ---- transform -------------------------------------------------------------------------------------------------------------
// One workgroup per centroid chunk (PCMI_PAIR_CENTROID_CHUNK rows of ONE cloud, counted from the cloud's first row); chunks are
// numbered cloud by cloud.  The order of the sum is pcmi.h's: thread t adds rows t, t + 256, ... of the chunk to 0 (a row past the
// cloud's end adds +0), then a binary tree v[t] += v[t + s] for s = 128 .. 1.
__global__ __launch_bounds__(kThreads) void tf_partial_kernel(const void* __restrict__ raw, int f32, int64_t n, const int64_t* __restrict__ offs,
                                                              int nc, const double* __restrict__ scale, double* __restrict__ partial) {
  __shared__ int s_cloud;
  __shared__ int64_t s_lo, s_hi;
  __shared__ double red[3][kThreads];
  const int t = threadIdx.x;
  if (t == 0) {
    int64_t k = blockIdx.x, lo = 0, hi = 0;
    int c = 0;
    for (; c < nc; ++c) {
      segment_rows(offs, c, n, lo, hi);
      const int64_t cnt = chunks_of(hi - lo);
      if (k < cnt) break;
      k -= cnt;
    }
    s_cloud = c < nc ? c : -1;
    s_lo = lo + k * kChunk;
    s_hi = std::min<int64_t>(s_lo + kChunk, hi);
  }
  __syncthreads();
  if (s_cloud < 0) return;  // (the whole workgroup: more workgroups than chunks are launched, the host does not know the offsets)
  const double sc = scale[s_cloud >> 1];
  double v[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < kPerThread; ++q) {
    const int64_t row = s_lo + (int64_t)q * kThreads + t;
#pragma unroll
    for (int a = 0; a < 3; ++a) v[a] = add_rn(v[a], row < s_hi ? mul_rn(sc, raw_at(raw, f32, 3 * row + a)) : 0.0);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) red[a][t] = v[a];
  __syncthreads();
  for (int s = kThreads / 2; s >= 1; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int a = 0; a < 3; ++a) red[a][t] = add_rn(red[a][t], red[a][t + s]);
    }
    __syncthreads();
  }
  if (t < 3) partial[3 * (int64_t)blockIdx.x + t] = red[t][0];
}

// one thread per pair: the two centroids (chunk partials added to 0 in chunk order, divided by the row count), T of both clouds
// and trans = T1 inv(T0) in closed form
__global__ __launch_bounds__(kThreads) void tf_final_kernel(const int64_t* __restrict__ offs, int64_t n, int B, const double* __restrict__ rot,
                                                            int rotate, const double* __restrict__ partial, double* __restrict__ T,
                                                            double* __restrict__ trans) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= B) return;
  double R[2][9], tv[2][3];
  int64_t base = 0;
  if (rotate) {
    for (int c = 0; c < 2 * b; ++c) {
      int64_t lo, hi;
      segment_rows(offs, c, n, lo, hi);
      base += chunks_of(hi - lo);
    }
  }
  for (int s = 0; s < 2; ++s) {
    const int c = 2 * b + s;
    if (rotate) {
      int64_t lo, hi;
      segment_rows(offs, c, n, lo, hi);
      const int64_t cnt = chunks_of(hi - lo);
      double m[3] = {0.0, 0.0, 0.0};
      for (int64_t k = 0; k < cnt; ++k)
        for (int a = 0; a < 3; ++a) m[a] = add_rn(m[a], partial[3 * (base + k) + a]);
      base += cnt;
      for (int a = 0; a < 3; ++a) m[a] = hi > lo ? m[a] / (double)(hi - lo) : 0.0;
      for (int q = 0; q < 9; ++q) R[s][q] = rot[9 * c + q];
      for (int r = 0; r < 3; ++r)
        tv[s][r] = add_rn(add_rn(mul_rn(R[s][3 * r], -m[0]), mul_rn(R[s][3 * r + 1], -m[1])), mul_rn(R[s][3 * r + 2], -m[2]));
    } else {
      for (int q = 0; q < 9; ++q) R[s][q] = (q % 4 == 0) ? 1.0 : 0.0;
      for (int r = 0; r < 3; ++r) tv[s][r] = 0.0;
    }
    double* o = T + 16 * c;
    for (int r = 0; r < 3; ++r) {
      for (int k = 0; k < 3; ++k) o[4 * r + k] = R[s][3 * r + k];
      o[4 * r + 3] = tv[s][r];
    }
    o[12] = o[13] = o[14] = 0.0;
    o[15] = 1.0;
  }
  double* o = trans + 16 * b;
  for (int r = 0; r < 3; ++r) {
    double Rt[3];
    for (int c = 0; c < 3; ++c) {
      Rt[c] = rotate ? add_rn(add_rn(mul_rn(R[1][3 * r], R[0][3 * c]), mul_rn(R[1][3 * r + 1], R[0][3 * c + 1])), mul_rn(R[1][3 * r + 2], R[0][3 * c + 2]))
                     : (r == c ? 1.0 : 0.0);
      o[4 * r + c] = Rt[c];
    }
    o[4 * r + 3] = rotate ? add_rn(tv[1][r], -add_rn(add_rn(mul_rn(Rt[0], tv[0][0]), mul_rn(Rt[1], tv[0][1])), mul_rn(Rt[2], tv[0][2]))) : 0.0;
  }
  o[12] = o[13] = o[14] = 0.0;
  o[15] = 1.0;
}

__global__ __launch_bounds__(kThreads) void tf_point_kernel(const void* __restrict__ raw, int f32, int64_t n, const int64_t* __restrict__ offs, int nc,
                                                            const double* __restrict__ scale, int rotate, const double* __restrict__ T,
                                                            double* __restrict__ out, int32_t* flags) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int c = segment_of(offs, nc, i);
  if (c < 0) {  // a row of no cloud: dropped by pcmi_pair_voxelize
    out[3 * i] = out[3 * i + 1] = out[3 * i + 2] = 0.0;
    return;
  }
  const double sc = scale[c >> 1];
  const double x[3] = {raw_at(raw, f32, 3 * i), raw_at(raw, f32, 3 * i + 1), raw_at(raw, f32, 3 * i + 2)};
  double p[3] = {mul_rn(sc, x[0]), mul_rn(sc, x[1]), mul_rn(sc, x[2])};
  if (rotate) {
    double q[3];
    rigid_apply(T + 16 * c, 4, p, q);
    p[0] = q[0], p[1] = q[1], p[2] = q[2];
  }
  if (!finite3(x[0], x[1], x[2]) || !finite3(p[0], p[1], p[2])) atomicOr(&flags[c >> 1], PCMI_PAIR_FLAG_NONFINITE);
  out[3 * i] = p[0], out[3 * i + 1] = p[1], out[3 * i + 2] = p[2];
}

// ---- voxelise --------------------------------------------------------------------------------------------------------------
// cloud c owns the table slots [2 lo_c + c, 2 hi_c + c + 1): 2 rows + 1 of them
__global__ __launch_bounds__(kThreads) void vx_insert_kernel(const double* __restrict__ pts, int64_t n, const int64_t* __restrict__ offs, int nc,
                                                             double voxel, uint64_t* keys, uint32_t* first, uint32_t* __restrict__ slot_of,
                                                             int32_t* flags) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  uint32_t slot = kNoSlot;
  const int c = segment_of(offs, nc, i);
  int64_t lo = 0, hi = 0;
  if (c >= 0) segment_rows(offs, c, n, lo, hi);
  if (c >= 0 && i >= lo && i < hi) {  // (always, for ascending offsets: a segment never takes more rows than it was sized for)
    const double p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    int64_t v[3];
    if (!finite3(p[0], p[1], p[2])) {
      atomicOr(&flags[c >> 1], PCMI_PAIR_FLAG_NONFINITE);
    } else if (!cells_of(p, voxel, v)) {
      atomicOr(&flags[c >> 1], PCMI_PAIR_FLAG_RANGE);
    } else {
      // the first point of the voxel = its lowest row
      slot = claim_first(keys, (uint32_t)(2 * lo + c), (uint32_t)(2 * (hi - lo) + 1), cell_key(v[0], v[1], v[2]), first, i);
    }
  }
  slot_of[i] = slot;
}

__global__ __launch_bounds__(kThreads) void vx_first_kernel(int64_t n, const int64_t* __restrict__ offs, int nc, const uint32_t* __restrict__ slot_of,
                                                            const uint32_t* __restrict__ first, const int32_t* __restrict__ flags,
                                                            int32_t* __restrict__ is_first) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i > n) return;
  int f = 0;
  if (i < n) {
    if (is_first_row(slot_of[i], first, i)) f = flags[segment_of(offs, nc, i) >> 1] == 0 ? 1 : 0;  // a flagged pair yields no rows
  }
  is_first[i] = f;  // (is_first[n] = 0: the scan over n + 1 items ends in the total)
}

__global__ __launch_bounds__(kThreads) void vx_write_kernel(const double* __restrict__ pts, int64_t n, const int64_t* __restrict__ offs, int nc,
                                                            double voxel, const int32_t* __restrict__ is_first, const int32_t* __restrict__ pos,
                                                            double* __restrict__ out_pts, int32_t* __restrict__ coords, int32_t* __restrict__ first_index,
                                                            int64_t* __restrict__ n_vox, int64_t* __restrict__ vox_offsets) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i <= nc) {
    if (i == nc) {
      vox_offsets[nc] = pos[n];
    } else {
      int64_t lo, hi;
      segment_rows(offs, (int)i, n, lo, hi);
      n_vox[i] = pos[hi] - pos[lo];
      vox_offsets[i] = pos[lo];
    }
  }
  if (i >= n || !is_first[i]) return;
  const int64_t p = pos[i];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double v = pts[3 * i + a];
    out_pts[3 * p + a] = v;
    coords[3 * p + a] = (int32_t)floor(v / voxel);
  }
  first_index[p] = (int32_t)i;
}

// side_offsets [2, B + 1]: the voxels of side s (clouds 2 b' + s) of the pairs before b -- the batch rows of the collate
__global__ void vx_side_kernel(const int64_t* __restrict__ n_vox, int B, int64_t* __restrict__ side) {
  const int s = threadIdx.x;
  if (s >= 2) return;
  int64_t acc = 0;
  for (int b = 0; b < B; ++b) {
    side[s * (B + 1) + b] = acc;
    acc += n_vox[2 * b + s];
  }
  side[s * (B + 1) + B] = acc;
}

// ---- match -----------------------------------------------------------------------------------------------------------------
// the targets (clouds 2 b + 1) into radius[b]-sized cells; cloud c owns the slots [2 lo_c + c, 2 hi_c + c + 1)
__global__ __launch_bounds__(kThreads) void mt_insert_kernel(const double* __restrict__ pts, int64_t m_max, const int64_t* __restrict__ voff, int nc,
                                                             const double* __restrict__ radius, uint64_t* keys, int32_t* head,
                                                             int32_t* __restrict__ next, int32_t* flags) {
  const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j >= m_max) return;
  next[j] = -1;
  const int c = segment_of(voff, nc, j);
  if (c < 0 || !(c & 1)) return;
  int64_t lo, hi;
  segment_rows(voff, c, m_max, lo, hi);
  if (j < lo || j >= hi) return;
  const int b = c >> 1;
  const double r = radius[b];
  const double p[3] = {pts[3 * j], pts[3 * j + 1], pts[3 * j + 2]};
  int64_t v[3];
  if (!finite3(p[0], p[1], p[2])) {
    atomicOr(&flags[b], PCMI_PAIR_FLAG_NONFINITE);
  } else if (!(r > 0.0) || !cells_of(p, r, v)) {
    atomicOr(&flags[b], PCMI_PAIR_FLAG_RANGE);
  } else {
    const uint32_t slot = claim_slot(keys, (uint32_t)(2 * lo + c), (uint32_t)(2 * (hi - lo) + 1), cell_key(v[0], v[1], v[2]));
    next[j] = atomicExch(&head[slot], (int32_t)j);  // list order is arbitrary: the matches are sorted per source point
  }
}

// FILL = false: count[i] = the matches of source row i (0 for every other row, count[m_max] = 0), nq[b] += rows with a match;
// FILL = true: the rows of the pairs that are not flagged, (i, j) with the batch row offsets, j ascending
template <bool FILL>
__global__ __launch_bounds__(128) void mt_match_kernel(const double* __restrict__ pts, int64_t m_max, const int64_t* __restrict__ voff, int nc,
                                                       const double* __restrict__ trans, const double* __restrict__ radius,
                                                       const uint64_t* __restrict__ keys, const int32_t* __restrict__ head,
                                                       const int32_t* __restrict__ next, int64_t* __restrict__ count, int32_t* nq,
                                                       const int64_t* __restrict__ offs, const int64_t* __restrict__ pair_base,
                                                       const int64_t* __restrict__ side, const int64_t* __restrict__ totals,
                                                       int32_t* __restrict__ pairs, int32_t* flags) {
  const int64_t i = (int64_t)blockIdx.x * 128 + threadIdx.x;
  if (FILL && totals[2] != 0) return;  // the rows do not fit: nothing is written
  int b = -1, nf = 0;
  int32_t found[FILL ? kMaxMatches : 1];
  int64_t lo0 = 0, lo1 = 0;
  if (i < m_max) {
    const int c = segment_of(voff, nc, i);
    int64_t hi0 = 0, hi1 = 0;
    if (c >= 0 && !(c & 1)) {
      segment_rows(voff, c, m_max, lo0, hi0);
      segment_rows(voff, c + 1, m_max, lo1, hi1);
      if (i >= lo0 && i < hi0 && (!FILL || (flags[c >> 1] == 0 && count[i] > 0))) b = c >> 1;
    }
    if (b >= 0) {
      const double r = radius[b];
      const double p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
      double q[3];
      int64_t cell[3];
      rigid_apply(trans + 16 * b, 4, p, q);
      if (!finite3(q[0], q[1], q[2])) {  // a source point the transform made non-finite
        if (!FILL) atomicOr(&flags[b], PCMI_PAIR_FLAG_NONFINITE);
      } else if (!(r > 0.0) || !cells_of(q, r, cell)) {
        if (!FILL) atomicOr(&flags[b], PCMI_PAIR_FLAG_RANGE);
      } else if (hi1 > lo1) {
        nf = radius_probe(pts, m_max, q, cell, r, keys, head, next, (uint32_t)(2 * lo1 + 2 * b + 1), (uint32_t)(2 * (hi1 - lo1) + 1), FILL ? found : nullptr);
      }
      if (!FILL && nf > kMaxMatches) atomicOr(&flags[b], PCMI_PAIR_FLAG_MATCHES);
    }
  }
  if (!FILL) {
    if (i <= m_max) count[i] = nf;
    // rows with a match, per pair: one integer add per (wave, pair)
    const bool has = nf > 0;
    unsigned long long rem = __ballot(has);
    while (rem) {
      const int leader = __ffsll((long long)rem) - 1;
      const int lb = __shfl(b, leader, 64);
      const unsigned long long same = __ballot(has && b == lb);
      if ((int)(threadIdx.x & 63) == leader) atomicAdd(&nq[lb], (int32_t)__popcll(same));
      rem &= ~same;
    }
    return;
  }
  if (b < 0) return;
  nf = min(nf, kMaxMatches);
  for (int a = 1; a < nf; ++a) {  // insertion sort, nf is small
    const int32_t v = found[a];
    int k = a - 1;
    while (k >= 0 && found[k] > v) {
      found[k + 1] = found[k];
      --k;
    }
    found[k + 1] = v;
  }
  const int B = nc >> 1;
  const int64_t dst = pair_base[b] + (offs[i] - offs[lo0]);
  if (dst < 0 || dst + nf > totals[3]) return;  // (cannot happen: the counts of this call; totals[3] = the capacity)
  const int64_t s0 = side[b], s1 = side[(B + 1) + b];
  int32_t* out = pairs + 2 * dst;
  for (int a = 0; a < nf; ++a) {
    out[2 * a] = (int32_t)(i - lo0 + s0);
    out[2 * a + 1] = (int32_t)((int64_t)found[a] - lo1 + s1);
  }
}

// one workgroup, thread b = pair b: its rows (0 if flagged, 1 placeholder without a match), their prefix, the totals
__global__ __launch_bounds__(kMaxPairs) void mt_pair_kernel(const int64_t* __restrict__ voff, int64_t m_max, int B, const int64_t* __restrict__ offs,
                                                            const int32_t* __restrict__ nq, const int32_t* __restrict__ flags,
                                                            const int64_t* __restrict__ side, int64_t capacity, int64_t* __restrict__ pair_counts,
                                                            int64_t* __restrict__ pair_base, int64_t* __restrict__ totals, int32_t* __restrict__ pairs) {
  __shared__ int64_t s_rows[kMaxPairs], s_q[kMaxPairs];
  const int b = threadIdx.x;
  int64_t rows = 0, q = 0, pc = 0;
  if (b < B) {
    int64_t lo, hi;
    segment_rows(voff, 2 * b, m_max, lo, hi);
    pc = offs[hi] - offs[lo];
    const bool flagged = flags[b] != 0;
    rows = flagged ? 0 : (pc > 0 ? pc : 1);
    q = flagged ? 0 : (pc > 0 ? (int64_t)nq[b] : 1);
  }
  s_rows[b] = rows;
  s_q[b] = q;
  __syncthreads();
  for (int d = 1; d < kMaxPairs; d <<= 1) {  // inclusive scan
    const int64_t ar = b >= d ? s_rows[b - d] : 0, aq = b >= d ? s_q[b - d] : 0;
    __syncthreads();
    s_rows[b] += ar;
    s_q[b] += aq;
    __syncthreads();
  }
  const int64_t total = s_rows[kMaxPairs - 1];
  const bool fits = total <= capacity;
  if (b < B) {
    const int64_t base = s_rows[b] - rows;
    pair_counts[b] = rows;
    pair_base[b] = base;
    if (fits && rows == 1 && pc == 0) {  // "in case 0 matching": the pair's first rows
      pairs[2 * base] = (int32_t)side[b];
      pairs[2 * base + 1] = (int32_t)side[(B + 1) + b];
    }
  }
  if (b == 0) {
    totals[0] = total;
    totals[1] = s_q[kMaxPairs - 1];
    totals[2] = fits ? 0 : 1;
    totals[3] = capacity;
  }
}

// ---- collate ---------------------------------------------------------------------------------------------------------------
struct CollateOut {
  int32_t* C[2];
  float* pcd[2];
  float* F[2];
};

__global__ __launch_bounds__(kThreads) void co_kernel(const double* __restrict__ pts, const int32_t* __restrict__ coords,
                                                      const int32_t* __restrict__ first_index, int64_t m_max, const int64_t* __restrict__ voff, int B,
                                                      const int64_t* __restrict__ side, const double* __restrict__ trans,
                                                      const float* __restrict__ noise, int64_t n_raw, const int32_t* __restrict__ jitter_on,
                                                      double mu, double sigma, int64_t out_rows, CollateOut out, float* __restrict__ T_gt) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r < 16 * (int64_t)B) T_gt[r] = (float)trans[r];
  if (r >= m_max) return;
  const int c = segment_of(voff, 2 * B, r);
  if (c < 0) return;
  int64_t lo, hi;
  segment_rows(voff, c, m_max, lo, hi);
  if (r < lo || r >= hi) return;
  const int s = c & 1, b = c >> 1;
  const int64_t dst = side[s * (B + 1) + b] + (r - lo);
  if (dst < 0 || dst >= out_rows) return;
  int32_t* C = out.C[s] + 4 * dst;
  C[0] = b;
  const int64_t src = first_index[r];
  const bool on = noise && jitter_on[c] != 0 && src >= 0 && src < n_raw;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    C[1 + a] = coords[3 * r + a];
    out.pcd[s][3 * dst + a] = (float)pts[3 * r + a];
    out.F[s][3 * dst + a] = on ? (float)add_rn(1.0, add_rn(mu, mul_rn(sigma, (double)noise[3 * src + a]))) : 1.0f;
  }
}

// ---- colour features -------------------------------------------------------------------------------------------------------
// co_kernel's rows once more: F = fp32((c / 255 - 0.5) + (mu + sigma z)), c and z of the voxel's first raw point.  A lane owns one
// voxel row: 3 colour bytes and 3 noise words gathered at first_index (ascending inside a cloud, so neighbouring lanes read
// forward through the raw rows), 12 contiguous bytes stored next to its neighbours'.
__global__ __launch_bounds__(kThreads) void cf_kernel(const uint8_t* __restrict__ color, const int32_t* __restrict__ first_index, int64_t m_max,
                                                      const int64_t* __restrict__ voff, int B, const int64_t* __restrict__ side,
                                                      const float* __restrict__ noise, int64_t n_raw, const int32_t* __restrict__ jitter_on,
                                                      double mu, double sigma, int64_t out_rows, float* __restrict__ F0, float* __restrict__ F1) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= m_max) return;
  const int c = segment_of(voff, 2 * B, r);
  if (c < 0) return;
  int64_t lo, hi;
  segment_rows(voff, c, m_max, lo, hi);
  if (r < lo || r >= hi) return;
  const int s = c & 1, b = c >> 1;
  const int64_t dst = side[s * (B + 1) + b] + (r - lo);
  const int64_t src = first_index[r];
  if (dst < 0 || dst >= out_rows || src < 0 || src >= n_raw) return;
  const bool on = noise && jitter_on[c] != 0;
  float* F = (s ? F1 : F0) + 3 * dst;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double v = add_rn((double)color[3 * src + a] / 255.0, -0.5);
    F[a] = (float)(on ? add_rn(v, add_rn(mu, mul_rn(sigma, (double)noise[3 * src + a]))) : v);
  }
}

static bool batch_ok(int64_t n, int64_t B) { return n >= 0 && n < (1ll << 31) - kThreads && B >= 1 && B <= kMaxPairs; }

static int64_t max_chunks(int64_t n, int64_t B) { return ceil_div(n, kChunk) + 2 * B; }
static int64_t table_slots(int64_t n, int64_t B) { return 2 * n + 2 * B; }

}  // namespace pairinput
}  // namespace pcmi

using namespace pcmi;
using namespace pcmi::pairinput;

extern "C" {

size_t pcmi_pair_transform_workspace_bytes(int64_t n, int64_t B) {
  if (!batch_ok(n, B)) return 0;
  return align_up((size_t)max_chunks(n, B) * 3 * 8, 256);
}

// replaces pretrain/pointcontrast/lib/ddp_data_loaders.py:196-225 (scale, sample_random_trans of both frames, T1 inv(T0))
int pcmi_pair_transform(const void* raw, int raw_is_f32, const int64_t* offsets, int64_t n, int64_t B, const double* scale, const double* rot,
                        int rotate, double* points, double* T, double* trans, int32_t* flags, void* ws, size_t ws_bytes,
                        pcmi_stream_t stream) {
  PCMI_REQUIRE(batch_ok(n, B), PCMI_ERR_INVALID, "pair_transform: bad shape (0 <= n %lld < 2^31 - 256; 1 <= B %lld <= %d)", (long long)n,
               (long long)B, kMaxPairs);
  PCMI_REQUIRE(offsets && scale && T && trans && flags && (n == 0 || (raw && points)) && (!rotate || rot), PCMI_ERR_INVALID,
               "pair_transform: null pointer");
  if (int rc = require_ws("pair_transform", ws, ws_bytes, pcmi_pair_transform_workspace_bytes(n, B), 16)) return rc;
  hipStream_t st = as_stream(stream);
  double* partial = static_cast<double*>(ws);
  const int f32 = raw_is_f32 ? 1 : 0, rt = rotate ? 1 : 0;
  if (rt && n > 0) {
    tf_partial_kernel<<<(unsigned)max_chunks(n, B), kThreads, 0, st>>>(raw, f32, n, offsets, (int)(2 * B), scale, partial);
    PCMI_LAUNCH_CHECK();
  }
  tf_final_kernel<<<(unsigned)ceil_div(B, kThreads), kThreads, 0, st>>>(offsets, n, (int)B, rot, rt, partial, T, trans);
  PCMI_LAUNCH_CHECK();
  if (n > 0) {
    tf_point_kernel<<<(unsigned)ceil_div(n, kThreads), kThreads, 0, st>>>(raw, f32, n, offsets, (int)(2 * B), scale, rt, T, points, flags);
    PCMI_LAUNCH_CHECK();
  }
  return PCMI_OK;
}

struct VoxelizeWs { uint64_t* keys; uint32_t *first, *slot_of; int32_t *is_first, *pos; void* temp; size_t temp_bytes, bytes; };
static VoxelizeWs voxelize_ws(void* ws, int64_t n, int64_t B) {
  const size_t slots = (size_t)table_slots(n, B);
  Carve cv{(char*)ws};
  VoxelizeWs L;
  L.keys = cv.take<uint64_t>(slots);
  L.first = cv.take<uint32_t>(slots);
  L.slot_of = cv.take<uint32_t>((size_t)std::max<int64_t>(n, 1));
  L.is_first = cv.take<int32_t>((size_t)n + 1);
  L.pos = cv.take<int32_t>((size_t)n + 1);
  L.temp_bytes = cub_scan_bytes<int32_t>(n + 1);
  L.temp = cv.take<char>(L.temp_bytes);
  L.bytes = cv.used;
  return L;
}

size_t pcmi_pair_voxelize_workspace_bytes(int64_t n, int64_t B) {
  if (!batch_ok(n, B) || n > kMaxRows) return 0;
  return voxelize_ws(nullptr, n, B).bytes;
}

// replaces pretrain/pointcontrast/lib/ddp_data_loaders.py:228-229, :238-239, :258-259 (sparse_quantize of both frames, floor)
int pcmi_pair_voxelize(const double* points, const int64_t* offsets, int64_t n, int64_t B, double voxel_size, double* out_points,
                       int32_t* coords, int32_t* first_index, int64_t* n_vox, int64_t* vox_offsets, int64_t* side_offsets, int32_t* flags,
                       void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_REQUIRE(batch_ok(n, B), PCMI_ERR_INVALID, "pair_voxelize: bad shape (0 <= n %lld < 2^31 - 256; 1 <= B %lld <= %d)", (long long)n,
               (long long)B, kMaxPairs);
  PCMI_REQUIRE(n <= kMaxRows, PCMI_ERR_UNSUPPORTED, "pair_voxelize: %lld rows, at most 2^29", (long long)n);
  PCMI_REQUIRE(voxel_size > 0.0 && voxel_size < 1e300, PCMI_ERR_INVALID, "pair_voxelize: voxel_size must be positive and finite");
  PCMI_REQUIRE(offsets && n_vox && vox_offsets && side_offsets && flags && (n == 0 || (points && out_points && coords && first_index)),
               PCMI_ERR_INVALID, "pair_voxelize: null pointer");
  if (int rc = require_ws("pair_voxelize", ws, ws_bytes, voxelize_ws(nullptr, n, B).bytes, 16)) return rc;
  hipStream_t st = as_stream(stream);
  const int nc = (int)(2 * B);
  if (n == 0) {
    PCMI_HIP_CHECK(hipMemsetAsync(n_vox, 0, (size_t)nc * 8, st));
    PCMI_HIP_CHECK(hipMemsetAsync(vox_offsets, 0, (size_t)(nc + 1) * 8, st));
    PCMI_HIP_CHECK(hipMemsetAsync(side_offsets, 0, (size_t)2 * (B + 1) * 8, st));
    return PCMI_OK;
  }
  const int64_t slots = table_slots(n, B);
  const VoxelizeWs L = voxelize_ws(ws, n, B);
  PCMI_HIP_CHECK(hipMemsetAsync(L.keys, 0xff, (size_t)slots * 8, st));
  PCMI_HIP_CHECK(hipMemsetAsync(L.first, 0xff, (size_t)slots * 4, st));
  const unsigned grid = (unsigned)ceil_div(n, kThreads);
  vx_insert_kernel<<<grid, kThreads, 0, st>>>(points, n, offsets, nc, voxel_size, L.keys, L.first, L.slot_of, flags);
  PCMI_LAUNCH_CHECK();
  vx_first_kernel<<<(unsigned)ceil_div(n + 1, kThreads), kThreads, 0, st>>>(n, offsets, nc, L.slot_of, L.first, flags, L.is_first);
  PCMI_LAUNCH_CHECK();
  if (int rc = cub_scan_excl(L.temp, L.temp_bytes, L.is_first, L.pos, n + 1, st)) return rc;
  vx_write_kernel<<<(unsigned)ceil_div(std::max<int64_t>(n, nc + 1), kThreads), kThreads, 0, st>>>(points, n, offsets, nc, voxel_size, L.is_first, L.pos,
                                                                                                  out_points, coords, first_index, n_vox, vox_offsets);
  PCMI_LAUNCH_CHECK();
  vx_side_kernel<<<1, 64, 0, st>>>(n_vox, (int)B, side_offsets);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

struct MatchWs { uint64_t* keys; int32_t *head, *next; int64_t *count, *offs, *pair_base; int32_t* nq; void* temp; size_t temp_bytes, bytes; };
static MatchWs match_ws(void* ws, int64_t m_max, int64_t B) {
  const size_t slots = (size_t)table_slots(m_max, B);
  Carve cv{(char*)ws};
  MatchWs L;
  L.keys = cv.take<uint64_t>(slots);
  L.head = cv.take<int32_t>(slots);
  L.next = cv.take<int32_t>((size_t)std::max<int64_t>(m_max, 1));
  L.count = cv.take<int64_t>((size_t)m_max + 1);
  L.offs = cv.take<int64_t>((size_t)m_max + 1);
  L.pair_base = cv.take<int64_t>((size_t)B);
  L.nq = cv.take<int32_t>(2 * (size_t)B);  // B values are used; sized as B 8-byte words since the entry was written
  L.temp_bytes = cub_scan_bytes<int64_t>(m_max + 1);
  L.temp = cv.take<char>(L.temp_bytes);
  L.bytes = cv.used;
  return L;
}

size_t pcmi_pair_match_workspace_bytes(int64_t m_max, int64_t B) {
  if (!batch_ok(m_max, B) || m_max > kMaxRows) return 0;
  return match_ws(nullptr, m_max, B).bytes;
}

// replaces pretrain/pointcontrast/lib/ddp_data_loaders.py:36-49, :241 (get_matching_indices) and the offsets of :76-83
int pcmi_pair_match(const double* points, int64_t m_max, const int64_t* vox_offsets, const int64_t* side_offsets, int64_t B,
                    const double* trans, const double* radius, int32_t* pairs, int64_t capacity, int64_t* pair_counts, int64_t* totals,
                    int32_t* flags, int fill_only, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_REQUIRE(batch_ok(m_max, B), PCMI_ERR_INVALID, "pair_match: bad shape (0 <= m_max %lld < 2^31 - 256; 1 <= B %lld <= %d)", (long long)m_max,
               (long long)B, kMaxPairs);
  PCMI_REQUIRE(m_max <= kMaxRows, PCMI_ERR_UNSUPPORTED, "pair_match: %lld rows, at most 2^29", (long long)m_max);
  PCMI_REQUIRE(capacity >= 0 && capacity < (1ll << 31), PCMI_ERR_INVALID, "pair_match: capacity %lld outside [0, 2^31)", (long long)capacity);
  PCMI_REQUIRE(vox_offsets && side_offsets && trans && radius && pair_counts && totals && flags && (m_max == 0 || points) &&
                   (capacity == 0 || pairs), PCMI_ERR_INVALID, "pair_match: null pointer");
  if (int rc = require_ws("pair_match", ws, ws_bytes, match_ws(nullptr, m_max, B).bytes, 16)) return rc;
  hipStream_t st = as_stream(stream);
  const int nc = (int)(2 * B);
  const int64_t slots = table_slots(m_max, B);
  const MatchWs L = match_ws(ws, m_max, B);
  const unsigned g128 = (unsigned)ceil_div(m_max + 1, 128);
  if (!fill_only) {  // (fill_only: the cells, the counts and their scan are in ws, as the call before left them)
    PCMI_HIP_CHECK(hipMemsetAsync(L.keys, 0xff, (size_t)slots * 8, st));
    PCMI_HIP_CHECK(hipMemsetAsync(L.head, 0xff, (size_t)slots * 4, st));  // -1
    PCMI_HIP_CHECK(hipMemsetAsync(L.nq, 0, (size_t)B * 4, st));
    if (m_max > 0) {
      mt_insert_kernel<<<(unsigned)ceil_div(m_max, kThreads), kThreads, 0, st>>>(points, m_max, vox_offsets, nc, radius, L.keys, L.head, L.next, flags);
      PCMI_LAUNCH_CHECK();
    }
    mt_match_kernel<false><<<g128, 128, 0, st>>>(points, m_max, vox_offsets, nc, trans, radius, L.keys, L.head, L.next, L.count, L.nq, nullptr, nullptr,
                                                nullptr, nullptr, nullptr, flags);
    PCMI_LAUNCH_CHECK();
    if (int rc = cub_scan_excl(L.temp, L.temp_bytes, L.count, L.offs, m_max + 1, st)) return rc;
  }
  mt_pair_kernel<<<1, kMaxPairs, 0, st>>>(vox_offsets, m_max, (int)B, L.offs, L.nq, flags, side_offsets, capacity, pair_counts, L.pair_base, totals, pairs);
  PCMI_LAUNCH_CHECK();
  if (m_max > 0 && capacity > 0) {
    mt_match_kernel<true><<<g128, 128, 0, st>>>(points, m_max, vox_offsets, nc, trans, radius, L.keys, L.head, L.next, L.count, L.nq, L.offs, L.pair_base,
                                               side_offsets, totals, pairs, flags);
    PCMI_LAUNCH_CHECK();
  }
  return PCMI_OK;
}

size_t pcmi_pair_collate_workspace_bytes(int64_t m_max, int64_t B) { return batch_ok(m_max, B) ? 256 : 0; }

// replaces pretrain/pointcontrast/lib/ddp_data_loaders.py:52-112 (default_collate_pair_fn) with :248-252 and FeatureJitter
// (lib/transforms.py:21-30)
int pcmi_pair_collate(const double* points, const int32_t* coords, const int32_t* first_index, int64_t m_max, const int64_t* vox_offsets,
                      const int64_t* side_offsets, int64_t B, const double* trans, const float* noise, int64_t n_raw, const int32_t* jitter_on,
                      double mu, double sigma, int64_t out_rows, int32_t* C0, int32_t* C1, float* pcd0, float* pcd1, float* F0, float* F1,
                      float* T_gt, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  (void)ws;
  (void)ws_bytes;
  PCMI_REQUIRE(batch_ok(m_max, B) && n_raw >= 0 && out_rows >= 0, PCMI_ERR_INVALID,
               "pair_collate: bad shape (0 <= m_max %lld < 2^31 - 256; 1 <= B %lld <= %d; n_raw %lld, out_rows %lld >= 0)", (long long)m_max,
               (long long)B, kMaxPairs, (long long)n_raw, (long long)out_rows);
  PCMI_REQUIRE(mu == mu && sigma == sigma && fabs(mu) < 1e300 && fabs(sigma) < 1e300, PCMI_ERR_INVALID, "pair_collate: mu and sigma must be finite");
  PCMI_REQUIRE(vox_offsets && side_offsets && trans && T_gt && (m_max == 0 || (points && coords && first_index)) &&
                   (out_rows == 0 || (C0 && C1 && pcd0 && pcd1 && F0 && F1)) && (!noise || jitter_on), PCMI_ERR_INVALID,
               "pair_collate: null pointer (noise needs jitter_on)");
  CollateOut out;
  out.C[0] = C0, out.C[1] = C1, out.pcd[0] = pcd0, out.pcd[1] = pcd1, out.F[0] = F0, out.F[1] = F1;
  const int64_t threads = std::max<int64_t>(out_rows > 0 ? m_max : 0, 16 * B);
  co_kernel<<<(unsigned)ceil_div(threads, kThreads), kThreads, 0, as_stream(stream)>>>(points, coords, first_index, out_rows > 0 ? m_max : 0,
                                                                                       vox_offsets, (int)B, side_offsets, trans, noise, n_raw,
                                                                                       jitter_on, mu, sigma, out_rows, out, T_gt);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

size_t pcmi_pair_color_features_workspace_bytes(int64_t m_max, int64_t B) { return batch_ok(m_max, B) ? 256 : 0; }

// the features ScanNetMatchPairDataset builds with data.use_color (feats = color / 255 - 0.5 in front of FeatureJitter), where the
// reference has its "#dummy color" (pretrain/pointcontrast/lib/ddp_data_loaders.py:204-206, :248-249)
int pcmi_pair_color_features(const uint8_t* color, const int32_t* first_index, int64_t m_max, const int64_t* vox_offsets,
                             const int64_t* side_offsets, int64_t B, const float* noise, int64_t n_raw, const int32_t* jitter_on, double mu,
                             double sigma, int64_t out_rows, float* F0, float* F1, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  (void)ws;
  (void)ws_bytes;
  PCMI_REQUIRE(batch_ok(m_max, B) && n_raw >= 0 && out_rows >= 0, PCMI_ERR_INVALID,
               "pair_color_features: bad shape (0 <= m_max %lld < 2^31 - 256; 1 <= B %lld <= %d; n_raw %lld, out_rows %lld >= 0)",
               (long long)m_max, (long long)B, kMaxPairs, (long long)n_raw, (long long)out_rows);
  PCMI_REQUIRE(mu == mu && sigma == sigma && fabs(mu) < 1e300 && fabs(sigma) < 1e300, PCMI_ERR_INVALID,
               "pair_color_features: mu and sigma must be finite");
  PCMI_REQUIRE(vox_offsets && side_offsets && (m_max == 0 || first_index) && (n_raw == 0 || color) && (out_rows == 0 || (F0 && F1)) &&
                   (!noise || jitter_on), PCMI_ERR_INVALID, "pair_color_features: null pointer (noise needs jitter_on)");
  if (m_max == 0 || out_rows == 0 || n_raw == 0) return PCMI_OK;  // no row to write
  cf_kernel<<<(unsigned)ceil_div(m_max, kThreads), kThreads, 0, as_stream(stream)>>>(color, first_index, m_max, vox_offsets, (int)B,
                                                                                     side_offsets, noise, n_raw, jitter_on, mu, sigma, out_rows,
                                                                                     F0, F1);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

}  // extern "C"
