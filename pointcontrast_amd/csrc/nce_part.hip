// Spatially partitioned PointInfoNCE (the loss of Hou et al., "Exploring Data-Efficient 3D Scene Understanding with
// Contrastive Scene Contexts", restated in include/pcmi.h): the negatives of every anchor are partitioned by where they lie
// around it (distance shell x elevation half x azimuth sector, an all-integer rule on the voxel coordinates), one InfoNCE per
// partition.  Written from the semantics in include/pcmi.h; gfx950, wave64.
//
// The n x n logits and partitions are never written to memory.  A workgroup of two waves owns 64 rows (lane = row, the
// row's features in registers) and walks a share of the other operand in chunks of 64 rows staged in LDS next to their
// coordinates and scene ids; each wave takes half of a chunk, reads it by broadcast, decides part(i, j) from the integers and
// only then forms the fp32 dot product (ascending channel, explicit fmaf -- the same bits wherever a logit is formed again).
//   forward : P log-sum-exp states (maximum, sum) PER THREAD, indexed by the run-time partition id -- in LDS as [p][thread]
//             (a private column per thread: no races, bank = thread for every p), never in scratch.  A maximum per partition:
//             nothing is assumed about the range of the logits.  States are kept in natural units and lse = m + log(l), so a
//             partition whose negatives are negligible -- or absent -- has lse == l_ii bit for bit and exp(l_ii - lse) - 1 == 0.
//   backward: side 0 owns the rows of q, side 1 the rows of k (part(i, j) is then evaluated from the column's side:
//             d = xyz[own] - xyz[other]); C accumulators per thread, weights w[scene][p] and the lse values it needs in LDS.
// gridDim.y workgroups share a row tile; the last of them to arrive (common.h: arrive_last) merges their partials in split
// order.  The loss: pnce_reduce_kernel sums lse - l_ii per (scene, partition) over the live rows in float64 in a fixed order
// (thread t takes rows t, t + 256, ...; the 256 partials are folded by halving), counts them as integers, and its last
// workgroup forms the loss scene by scene.  No float atomics; every output is the same bits from run to run.
#include <algorithm>

#include "internal.h"

#pragma clang fp contract(off)

namespace pcmi {
namespace pnce {

constexpr int kThreads = 128;   // two waves; lane = own row, wave = half of the staged chunk
constexpr int kRows = 64;       // own rows per workgroup
constexpr int kChunk = 64;      // rows of the other operand per step
constexpr int kHalf = kChunk / 2;
constexpr int kMaxP = 32;
constexpr int kMaxScenes = 1024;
constexpr int kRedThreads = 256;
constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;
constexpr float kFloor = -1e30f;  // "no negative seen yet" (finite: no inf - inf)

struct Rule {
  int64_t r1_sq, r2_sq;
  int n_scenes, A, E, shift;  // shift = 3 - log2(A): the azimuth sector is (4 h + 2 qd + o) >> shift
};

// part(i, j) of include/pcmi.h: (xi, yi, zi, si) the row (anchor), (xj, yj, zj, sj) the column.  THE rule: the loss kernels
// and the test aid call this one function.
__device__ __forceinline__ int part_of(int xi, int yi, int zi, int si, int xj, int yj, int zj, int sj, bool same_index,
                                       const Rule& R) {
  if (same_index || si != sj || (unsigned)si >= (unsigned)R.n_scenes) return -1;
  int dx = xj - xi, dy = yj - yi;
  const int dz = zj - zi;
  const int64_t d2 = (int64_t)dx * dx + (int64_t)dy * dy + (int64_t)dz * dz;
  if (d2 == 0 || d2 > R.r2_sq) return -1;
  const int shell = d2 <= R.r1_sq ? 0 : 1;
  const int el = (R.E == 1 || dz >= 0) ? 0 : 1;
  const int h = (dy > 0 || (dy == 0 && dx > 0)) ? 0 : 1;
  if (h) {
    dx = -dx;
    dy = -dy;
  }
  const int qd = dx > 0 ? 0 : 1;
  if (qd) {
    const int ox = dx;
    dx = dy;
    dy = -ox;
  }
  const int o = dy < dx ? 0 : 1;
  const int az = (4 * h + 2 * qd + o) >> R.shift;
  return (shell * R.E + el) * R.A + az;
}

template <int C>
__device__ __forceinline__ void load_row(const float* __restrict__ x, int64_t row, bool valid, float* out) {
#pragma unroll
  for (int c4 = 0; c4 < C / 4; ++c4) {
    const float4 v = valid ? *reinterpret_cast<const float4*>(x + row * C + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    out[4 * c4 + 0] = v.x;
    out[4 * c4 + 1] = v.y;
    out[4 * c4 + 2] = v.z;
    out[4 * c4 + 3] = v.w;
  }
}

// sum_d own[d] * other[d], ascending d, one fmaf each: the ONE spelling of a logit's product (fmaf(a, b, c) == fmaf(b, a, c),
// so both sides of the backward and the diagonal reproduce the forward's bits)
template <int C>
__device__ __forceinline__ float dot_lds(const float* own, const float4* __restrict__ row) {
  float acc = 0.f;
#pragma unroll
  for (int c4 = 0; c4 < C / 4; ++c4) {
    const float4 f = row[c4];
    acc = fmaf(own[4 * c4 + 0], f.x, acc);
    acc = fmaf(own[4 * c4 + 1], f.y, acc);
    acc = fmaf(own[4 * c4 + 2], f.z, acc);
    acc = fmaf(own[4 * c4 + 3], f.w, acc);
  }
  return acc;
}
template <int C>
__device__ __forceinline__ float dot_global(const float* own, const float* __restrict__ other) {
  return dot_lds<C>(own, reinterpret_cast<const float4*>(other));
}

// the staged chunk: features [kChunk][C] (zero past n), coordinates + scene (scene -1 past n: part == -1)
template <int C>
__device__ __forceinline__ void stage_chunk(const float* __restrict__ f, const int32_t* __restrict__ xyz,
                                            const int32_t* __restrict__ scene, int64_t n, int64_t j0, int t,
                                            float4 (*s_f)[C / 4], int4* s_x) {
  for (int e = t; e < kChunk * (C / 4); e += kThreads) {
    const int row = e / (C / 4), c4 = e % (C / 4);
    const int64_t j = j0 + row;
    s_f[row][c4] = j < n ? *reinterpret_cast<const float4*>(f + j * C + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (t < kChunk) {
    const int64_t j = j0 + t;
    s_x[t] = j < n ? make_int4(xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2], scene[j]) : make_int4(0, 0, 0, -1);
  }
}

__device__ __forceinline__ float exp_nat(float x) { return __builtin_amdgcn_exp2f(x * kLog2e); }

// ---- forward ---------------------------------------------------------------------------------------------------------------
// grid = (row tiles, splits); dynamic LDS: the states, 2 x [P][kThreads] floats.  part_m / part_l: [split][n_pad][P].
template <int C>
__global__ __launch_bounds__(kThreads) void pnce_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                            const int32_t* __restrict__ xyz, const int32_t* __restrict__ scene,
                                                            int64_t n, int64_t n_pad, float inv_T, Rule R, int P, int64_t span,
                                                            float* __restrict__ part_m, float* __restrict__ part_l,
                                                            float* __restrict__ diag, uint32_t* __restrict__ rowmask,
                                                            unsigned* __restrict__ counters, float* __restrict__ lse) {
  extern __shared__ float s_state[];
  __shared__ float4 s_f[kChunk][C / 4];
  __shared__ int4 s_x[kChunk];
  __shared__ float s_diag[kRows];
  __shared__ unsigned s_live[kRows];
  __shared__ unsigned s_flag;
  float* s_m = s_state;
  float* s_l = s_state + P * kThreads;
  const int t = threadIdx.x, r = t & 63, w = t >> 6;
  const int64_t a = (int64_t)blockIdx.x * kRows + r;
  const bool valid = a < n;
  float own[C];
  load_row<C>(q, a, valid, own);
  const int ox = valid ? xyz[3 * a] : 0, oy = valid ? xyz[3 * a + 1] : 0, oz = valid ? xyz[3 * a + 2] : 0;
  const int os = valid ? scene[a] : -1;
  for (int p = 0; p < P; ++p) {
    s_m[p * kThreads + t] = kFloor;
    s_l[p * kThreads + t] = 0.f;
  }
  const int64_t n64 = (n + kChunk - 1) / kChunk * kChunk;
  const int64_t cbeg = (int64_t)blockIdx.y * span, cend = min(n64, cbeg + span);
  for (int64_t j0 = cbeg; j0 < cend; j0 += kChunk) {
    __syncthreads();
    stage_chunk<C>(k, xyz, scene, n, j0, t, s_f, s_x);
    __syncthreads();
    for (int jj = 0; jj < kHalf; ++jj) {
      const int col = w * kHalf + jj;
      const int4 X = s_x[col];
      const int p = part_of(ox, oy, oz, os, X.x, X.y, X.z, X.w, j0 + col == a, R);
      if (p >= 0) {
        const float x = dot_lds<C>(own, s_f[col]) * inv_T;
        const float m0 = s_m[p * kThreads + t], l0 = s_l[p * kThreads + t];
        const float mn = fmaxf(m0, x);
        s_l[p * kThreads + t] = l0 * exp_nat(m0 - mn) + exp_nat(x - mn);
        s_m[p * kThreads + t] = mn;
      }
    }
  }
  if (t < kRows) {
    s_diag[t] = valid ? dot_global<C>(own, k + a * C) * inv_T : 0.f;
    s_live[t] = 0u;
  }
  __syncthreads();
  // the two waves of a row, wave 0 first
  for (int e = t; e < kRows * P; e += kThreads) {
    const int rr = e / P, p = e % P;
    const float m0 = s_m[p * kThreads + rr], l0 = s_l[p * kThreads + rr];
    const float m1 = s_m[p * kThreads + 64 + rr], l1 = s_l[p * kThreads + 64 + rr];
    const float mn = fmaxf(m0, m1);
    const int64_t o = ((int64_t)blockIdx.y * n_pad + (int64_t)blockIdx.x * kRows + rr) * P + p;
    part_m[o] = mn;
    part_l[o] = l0 * exp_nat(m0 - mn) + l1 * exp_nat(m1 - mn);
  }
  // ---- the last workgroup of the row tile: the splits in order behind the diagonal term ----
  const int splits = (int)gridDim.y;
  if (!arrive_last(&counters[blockIdx.x], (unsigned)splits, &s_flag)) return;
  for (int e = t; e < kRows * P; e += kThreads) {
    const int rr = e / P, p = e % P;
    const int64_t row = (int64_t)blockIdx.x * kRows + rr;
    if (row >= n) continue;
    const float lii = s_diag[rr];
    float mm = lii, ll = 1.f;  // exp(l_ii - l_ii)
    bool any = false;
    for (int sp = 0; sp < splits; ++sp) {
      const int64_t o = ((int64_t)sp * n_pad + row) * P + p;
      const float om = part_m[o], ol = part_l[o];
      if (ol > 0.f) {  // (a share that saw a negative of this partition has l >= 1)
        any = true;
        const float mn = fmaxf(mm, om);
        ll = ll * exp_nat(mm - mn) + ol * exp_nat(om - mn);
        mm = mn;
      }
    }
    lse[row * P + p] = any ? mm + __builtin_amdgcn_logf(ll) * kLn2 : lii;  // v_log_f32 = log2; log2(1) == 0
    if (any) atomicOr(&s_live[rr], 1u << p);
  }
  __syncthreads();
  if (t < kRows && valid) {
    rowmask[a] = s_live[t];
    diag[a] = s_diag[t];
  }
}

// One workgroup per (scene, partition): the count of its live rows and the float64 sum of lse - l_ii over them; the last
// workgroup to arrive forms the loss.
__global__ __launch_bounds__(kRedThreads) void pnce_reduce_kernel(const float* __restrict__ lse, const float* __restrict__ diag,
                                                                  const uint32_t* __restrict__ rowmask,
                                                                  const int32_t* __restrict__ scene, int64_t n, int B, int P,
                                                                  double* __restrict__ sums, int32_t* __restrict__ live,
                                                                  unsigned* __restrict__ counter, float* __restrict__ loss) {
  __shared__ double s_sum[kRedThreads];
  __shared__ int s_cnt[kRedThreads];
  __shared__ double s_val[kMaxScenes];
  __shared__ int s_on[kMaxScenes];
  __shared__ unsigned s_flag;
  const int t = threadIdx.x, s = (int)blockIdx.x / P, p = (int)blockIdx.x % P;
  double acc = 0.0;
  int cnt = 0;
  for (int64_t i = t; i < n; i += kRedThreads)
    if (scene[i] == s && (rowmask[i] >> p & 1u)) {
      acc = acc + ((double)lse[i * P + p] - (double)diag[i]);
      ++cnt;
    }
  s_sum[t] = acc;
  s_cnt[t] = cnt;
  __syncthreads();
  for (int st = kRedThreads / 2; st > 0; st >>= 1) {
    if (t < st) {
      s_sum[t] = s_sum[t] + s_sum[t + st];
      s_cnt[t] += s_cnt[t + st];
    }
    __syncthreads();
  }
  if (t == 0) {
    sums[blockIdx.x] = s_sum[0];
    live[blockIdx.x] = s_cnt[0];
  }
  if (!arrive_last(counter, gridDim.x, &s_flag)) return;
  for (int sc = t; sc < B; sc += kRedThreads) {
    double v = 0.0;
    int L = 0;
    for (int pp = 0; pp < P; ++pp) {
      const int c = live[sc * P + pp];
      if (c > 0) {
        v = v + sums[sc * P + pp] / (double)c;
        ++L;
      }
    }
    s_val[sc] = L > 0 ? v / (double)L : 0.0;
    s_on[sc] = L > 0 ? 1 : 0;
  }
  __syncthreads();
  if (t == 0) {
    double total = 0.0;
    int S = 0;
    for (int sc = 0; sc < B; ++sc)
      if (s_on[sc]) {
        total = total + s_val[sc];
        ++S;
      }
    *loss = S > 0 ? (float)(total / (double)S) : 0.f;
  }
}

// ---- backward --------------------------------------------------------------------------------------------------------------
// w[s][p] = 1 / (S L_s |R[s, p]|) for a partition that is live in scene s, else 0
__global__ __launch_bounds__(kRedThreads) void pnce_weights_kernel(const int32_t* __restrict__ live, int B, int P,
                                                                   float* __restrict__ wtab) {
  __shared__ int s_L[kMaxScenes];
  const int t = threadIdx.x;
  for (int sc = t; sc < B; sc += kRedThreads) {
    int L = 0;
    for (int p = 0; p < P; ++p) L += live[sc * P + p] > 0 ? 1 : 0;
    s_L[sc] = L;
  }
  __syncthreads();
  int S = 0;
  for (int sc = 0; sc < B; ++sc) S += s_L[sc] > 0 ? 1 : 0;
  for (int e = t; e < B * P; e += kRedThreads) {
    const int c = live[e];
    wtab[e] = c > 0 ? (float)(1.0 / ((double)S * (double)s_L[e / P] * (double)c)) : 0.f;
  }
}

// grid = (row tiles, splits, side).  side 0: own = q, other = k, row of part() = own;  side 1: own = k, other = q, row of
// part() = other.  part: [side][split][n_pad][C] when splits > 1.
template <int C, bool FOR_K>
__device__ __forceinline__ void pnce_bwd_body(const float* __restrict__ own_f, const float* __restrict__ oth_f,
                                              const int32_t* __restrict__ xyz, const int32_t* __restrict__ scene,
                                              const float* __restrict__ lse, const float* __restrict__ wtab, int64_t n,
                                              int64_t n_pad, float inv_T, const float* __restrict__ gscale, const Rule& R, int P,
                                              int64_t span, float* __restrict__ d_own, float* __restrict__ part,
                                              unsigned* __restrict__ counter, float4 (*s_f)[C / 4], int4* s_x, float* s_w,
                                              float* s_buf, unsigned* s_flag) {
  const int t = threadIdx.x, r = t & 63, w = t >> 6;
  const int64_t tile0 = (int64_t)blockIdx.x * kRows, a = tile0 + r;
  const bool valid = a < n;
  float own[C], acc[C];
  load_row<C>(own_f, a, valid, own);
#pragma unroll
  for (int d = 0; d < C; ++d) acc[d] = 0.f;
  const int ox = valid ? xyz[3 * a] : 0, oy = valid ? xyz[3 * a + 1] : 0, oz = valid ? xyz[3 * a + 2] : 0;
  const int os = valid ? scene[a] : -1;
  // the weights of the own row's scene (a pair in a partition shares the scene).  s_buf holds the lse values of the walk: on
  // side 0 the own rows' as [p][row], for good; on side 1 the staged chunk's as [row][p]; after the walk, wave 1's sums
  for (int e = t; e < kRows * P; e += kThreads) {
    const int rr = e / P, p = e % P;
    const int64_t row = tile0 + rr;
    const int sc = row < n ? scene[row] : -1;
    s_w[p * kRows + rr] = (unsigned)sc < (unsigned)R.n_scenes ? wtab[(int64_t)sc * P + p] : 0.f;
    if (!FOR_K) s_buf[p * kRows + rr] = row < n ? lse[row * P + p] : 0.f;
  }
  const int64_t n64 = (n + kChunk - 1) / kChunk * kChunk;
  const int64_t cbeg = (int64_t)blockIdx.y * span, cend = min(n64, cbeg + span);
  for (int64_t j0 = cbeg; j0 < cend; j0 += kChunk) {
    __syncthreads();
    stage_chunk<C>(oth_f, xyz, scene, n, j0, t, s_f, s_x);
    if (FOR_K)
      for (int e = t; e < kChunk * P; e += kThreads) s_buf[e] = j0 * P + e < n * P ? lse[j0 * P + e] : 0.f;
    __syncthreads();
    for (int jj = 0; jj < kHalf; ++jj) {
      const int col = w * kHalf + jj;
      const int4 X = s_x[col];
      const bool same = j0 + col == a;
      const int p = FOR_K ? part_of(X.x, X.y, X.z, X.w, ox, oy, oz, os, same, R) : part_of(ox, oy, oz, os, X.x, X.y, X.z, X.w, same, R);
      if (p >= 0) {
        const float x = dot_lds<C>(own, s_f[col]) * inv_T;
        const float lv = FOR_K ? s_buf[col * P + p] : s_buf[p * kRows + r];
        const float g = s_w[p * kRows + r] * exp_nat(x - lv);
#pragma unroll
        for (int c4 = 0; c4 < C / 4; ++c4) {
          const float4 f = s_f[col][c4];
          acc[4 * c4 + 0] = fmaf(g, f.x, acc[4 * c4 + 0]);
          acc[4 * c4 + 1] = fmaf(g, f.y, acc[4 * c4 + 1]);
          acc[4 * c4 + 2] = fmaf(g, f.z, acc[4 * c4 + 2]);
          acc[4 * c4 + 3] = fmaf(g, f.w, acc[4 * c4 + 3]);
        }
      }
    }
  }
  // the diagonal: G_ii = sum_p w[i, p] (exp(l_ii - lse[i, p]) - 1), once per row (split 0, wave 0), p ascending
  if (blockIdx.y == 0 && w == 0 && valid) {
    const float lii = dot_global<C>(own, oth_f + a * C) * inv_T;
    float gd = 0.f;
    for (int p = 0; p < P; ++p) {
      const float lv = FOR_K ? lse[a * P + p] : s_buf[p * kRows + r];
      gd = gd + s_w[p * kRows + r] * (exp_nat(lii - lv) - 1.f);
    }
#pragma unroll
    for (int d = 0; d < C; ++d) acc[d] = fmaf(gd, oth_f[a * C + d], acc[d]);
  }
  __syncthreads();  // (the last reads of s_buf as lse values)
  // wave 1 hands its sums to wave 0: [row][C + 1]
  if (w == 1) {
#pragma unroll
    for (int d = 0; d < C; ++d) s_buf[r * (C + 1) + d] = acc[d];
  }
  __syncthreads();
  const float gs = (gscale ? *gscale : 1.f) * inv_T;
  const int splits = (int)gridDim.y;
  if (w == 0) {
#pragma unroll
    for (int d = 0; d < C; ++d) acc[d] = (acc[d] + s_buf[r * (C + 1) + d]) * gs;
    float* __restrict__ dst = splits == 1 ? d_own + a * C : part + ((int64_t)blockIdx.y * n_pad + a) * C;
    if (splits > 1 || valid) {
#pragma unroll
      for (int c4 = 0; c4 < C / 4; ++c4)
        *reinterpret_cast<float4*>(dst + c4 * 4) = make_float4(acc[4 * c4], acc[4 * c4 + 1], acc[4 * c4 + 2], acc[4 * c4 + 3]);
    }
  }
  if (splits == 1) return;
  if (!arrive_last(counter, (unsigned)splits, s_flag)) return;
  // the last workgroup of the row tile: the shares in split order, four channels per thread
  constexpr int F4 = C / 4;
  for (int e = t; e < kRows * F4; e += kThreads) {
    const int row = e / F4, c4 = e % F4;
    const int64_t ra = tile0 + row;
    if (ra >= n) continue;
    float4 s = *reinterpret_cast<const float4*>(part + ra * C + c4 * 4);
    for (int sp = 1; sp < splits; ++sp) {
      const float4 v = *reinterpret_cast<const float4*>(part + ((int64_t)sp * n_pad + ra) * C + c4 * 4);
      s.x = s.x + v.x;
      s.y = s.y + v.y;
      s.z = s.z + v.z;
      s.w = s.w + v.w;
    }
    *reinterpret_cast<float4*>(d_own + ra * C + c4 * 4) = s;
  }
}

template <int C>
__global__ __launch_bounds__(kThreads) void pnce_bwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                            const int32_t* __restrict__ xyz, const int32_t* __restrict__ scene,
                                                            const float* __restrict__ lse, const float* __restrict__ wtab,
                                                            int64_t n, int64_t n_pad, float inv_T,
                                                            const float* __restrict__ gscale, Rule R, int P, int64_t span,
                                                            float* __restrict__ dq, float* __restrict__ dk,
                                                            float* __restrict__ part, unsigned* __restrict__ counters) {
  __shared__ float4 s_f[kChunk][C / 4];
  __shared__ int4 s_x[kChunk];
  __shared__ float s_w[kMaxP * kRows];
  __shared__ float s_buf[kRows * (kMaxP + 1)];  // >= kMaxP * kRows, kChunk * kMaxP and kRows * (C + 1)
  __shared__ unsigned s_flag;
  const int64_t side_part = (int64_t)gridDim.y * n_pad * C;
  if (blockIdx.z == 0)
    pnce_bwd_body<C, false>(q, k, xyz, scene, lse, wtab, n, n_pad, inv_T, gscale, R, P, span, dq, part, &counters[blockIdx.x], s_f,
                            s_x, s_w, s_buf, &s_flag);
  else
    pnce_bwd_body<C, true>(k, q, xyz, scene, lse, wtab, n, n_pad, inv_T, gscale, R, P, span, dk, part + side_part,
                           &counters[gridDim.x + blockIdx.x], s_f, s_x, s_w, s_buf, &s_flag);
}

// ---- the test aid: part(i, j) of every pair ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pnce_partition_kernel(const int32_t* __restrict__ xyz, const int32_t* __restrict__ scene,
                                                             int64_t n, Rule R, int8_t* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (j >= n) return;
  out[i * n + j] = (int8_t)part_of(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], scene[i], xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2],
                                   scene[j], i == j, R);
}

struct Plan {
  int64_t n_pad, span;
  int tiles, splits;
};
// splits: about six two-wave workgroups per CU over the row tiles (what the backward's registers and 26 KB of LDS admit: a
// thread's walk is a chain of dependent LDS reads and transcendental ops, hidden only by other waves), at most one per chunk
static Plan plan_of(int64_t n) {
  Plan p;
  p.tiles = (int)ceil_div(n, kRows);
  p.n_pad = (int64_t)p.tiles * kRows;
  const int64_t chunks = ceil_div(n, kChunk);
  const int64_t want = ceil_div(6 * (int64_t)num_cu(), p.tiles);
  p.splits = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, chunks), 32));
  p.span = ceil_div(chunks, p.splits) * kChunk;
  p.splits = (int)ceil_div(chunks * kChunk, p.span);
  return p;
}

// forward: part_m | part_l ([splits][n_pad][P] floats each) | diag [n_pad] | rowmask [n_pad] | sums [B P] doubles
// backward: wtab [B P] floats (padded to 16 bytes) | part [2][splits][n_pad][C] floats when splits > 1
static size_t fwd_bytes(const Plan& p, int n_scenes, int P) {
  return align_up(((size_t)2 * p.splits * p.n_pad * P + 2 * (size_t)p.n_pad) * sizeof(float), 16) + (size_t)n_scenes * P * sizeof(double);
}
static size_t bwd_bytes(const Plan& p, int c, int n_scenes, int P) {
  return align_up((size_t)n_scenes * P * sizeof(float), 16) + (p.splits > 1 ? (size_t)2 * p.splits * p.n_pad * c * sizeof(float) : 0);
}

static bool rule_of(int n_scenes, int64_t r1_sq, int64_t r2_sq, int A, int E, Rule* R) {
  if (!(A == 1 || A == 2 || A == 4 || A == 8) || !(E == 1 || E == 2) || r1_sq < 0 || r1_sq > r2_sq || n_scenes < 1 ||
      n_scenes > kMaxScenes)
    return false;
  R->r1_sq = r1_sq;
  R->r2_sq = r2_sq;
  R->n_scenes = n_scenes;
  R->A = A;
  R->E = E;
  R->shift = A == 8 ? 0 : A == 4 ? 1 : A == 2 ? 2 : 3;
  return true;
}

}  // namespace pnce
}  // namespace pcmi

using namespace pcmi;
using namespace pcmi::pnce;

extern "C" {

size_t pcmi_pnce_workspace_bytes(int64_t n, int c, int n_scenes, int P) {
  if (n < 1 || n >= (1ll << 31) - 256 || c < 1 || n_scenes < 1 || P < 1) return 0;
  const Plan p = plan_of(n);
  return std::max(fwd_bytes(p, n_scenes, P), bwd_bytes(p, c, n_scenes, P));
}

#define PCMI_PNCE_COMMON(who)                                                                                                          \
  PCMI_REQUIRE(q && k && xyz && scene && lse && live && n > 0 && n < (1ll << 31) - 256, PCMI_ERR_INVALID, who ": bad argument");       \
  PCMI_REQUIRE(c == 16 || c == 32, PCMI_ERR_UNSUPPORTED, who ": feature width %d not in {16,32}", c);                                  \
  Rule R;                                                                                                                              \
  PCMI_REQUIRE(rule_of(n_scenes, r1_sq, r2_sq, A, E, &R), PCMI_ERR_INVALID,                                                            \
               who ": needs A in {1,2,4,8}, E in {1,2}, 0 <= r1_sq <= r2_sq and 1..%d scenes", kMaxScenes);                            \
  const int P = 2 * E * A;                                                                                                             \
  PCMI_REQUIRE(ws && (uintptr_t)ws % 16 == 0 && ws_bytes >= pcmi_pnce_workspace_bytes(n, c, n_scenes, P), PCMI_ERR_WORKSPACE,          \
               who ": workspace of %zu bytes, %zu needed (16-byte aligned)", ws_bytes, pcmi_pnce_workspace_bytes(n, c, n_scenes, P)); \
  hipStream_t st = as_stream(stream);                                                                                                  \
  const Plan pl = plan_of(n)

int pcmi_pnce_fwd(const float* q, const float* k, const int32_t* xyz, const int32_t* scene, int64_t n, int c, int n_scenes, float inv_T,
                  int64_t r1_sq, int64_t r2_sq, int A, int E, float* lse, int32_t* live, float* loss, void* ws, size_t ws_bytes,
                  pcmi_stream_t stream) {
  PCMI_PNCE_COMMON("pnce_fwd");
  PCMI_REQUIRE(loss && (uintptr_t)q % 16 == 0 && (uintptr_t)k % 16 == 0, PCMI_ERR_INVALID, "pnce_fwd: null loss, or q/k not 16-byte aligned");
  const size_t per = (size_t)pl.splits * pl.n_pad * P;
  float* pm = (float*)ws;
  float* plv = pm + per;
  float* diag = plv + per;
  uint32_t* rowmask = (uint32_t*)(diag + pl.n_pad);
  double* sums = (double*)((char*)ws + align_up((2 * per + 2 * (size_t)pl.n_pad) * sizeof(float), 16));
  unsigned* counters = stream_counters(st, (size_t)pl.tiles + 1);
  if (!counters) return PCMI_ERR_HIP;
  const dim3 grid((unsigned)pl.tiles, (unsigned)pl.splits);
  const size_t dyn = (size_t)2 * P * kThreads * sizeof(float);
  if (c == 16)
    pnce_fwd_kernel<16><<<grid, kThreads, dyn, st>>>(q, k, xyz, scene, n, pl.n_pad, inv_T, R, P, pl.span, pm, plv, diag, rowmask, counters, lse);
  else
    pnce_fwd_kernel<32><<<grid, kThreads, dyn, st>>>(q, k, xyz, scene, n, pl.n_pad, inv_T, R, P, pl.span, pm, plv, diag, rowmask, counters, lse);
  PCMI_LAUNCH_CHECK();
  pnce_reduce_kernel<<<(unsigned)(n_scenes * P), kRedThreads, 0, st>>>(lse, diag, rowmask, scene, n, n_scenes, P, sums, live,
                                                                      counters + pl.tiles, loss);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

int pcmi_pnce_bwd(const float* q, const float* k, const int32_t* xyz, const int32_t* scene, const float* lse, const int32_t* live,
                  int64_t n, int c, int n_scenes, float inv_T, int64_t r1_sq, int64_t r2_sq, int A, int E, const float* gscale,
                  float* dq, float* dk, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_PNCE_COMMON("pnce_bwd");
  PCMI_REQUIRE(dq && dk && (uintptr_t)q % 16 == 0 && (uintptr_t)k % 16 == 0 && (uintptr_t)dq % 16 == 0 && (uintptr_t)dk % 16 == 0,
               PCMI_ERR_INVALID, "pnce_bwd: null gradient, or q/k/dq/dk not 16-byte aligned");
  float* wtab = (float*)ws;
  float* part = (float*)((char*)ws + align_up((size_t)n_scenes * P * sizeof(float), 16));
  unsigned* counters = stream_counters(st, (size_t)2 * pl.tiles);
  if (!counters) return PCMI_ERR_HIP;
  pnce_weights_kernel<<<1, kRedThreads, 0, st>>>(live, n_scenes, P, wtab);
  PCMI_LAUNCH_CHECK();
  const dim3 grid((unsigned)pl.tiles, (unsigned)pl.splits, 2);
  if (c == 16)
    pnce_bwd_kernel<16><<<grid, kThreads, 0, st>>>(q, k, xyz, scene, lse, wtab, n, pl.n_pad, inv_T, gscale, R, P, pl.span, dq, dk, part, counters);
  else
    pnce_bwd_kernel<32><<<grid, kThreads, 0, st>>>(q, k, xyz, scene, lse, wtab, n, pl.n_pad, inv_T, gscale, R, P, pl.span, dq, dk, part, counters);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

int pcmi_pnce_partition(const int32_t* xyz, const int32_t* scene, int64_t n, int n_scenes, int64_t r1_sq, int64_t r2_sq, int A, int E,
                        int8_t* part, pcmi_stream_t stream) {
  PCMI_REQUIRE(xyz && scene && part && n > 0, PCMI_ERR_INVALID, "pnce_partition: bad argument");
  PCMI_REQUIRE(n <= 4096, PCMI_ERR_UNSUPPORTED, "pnce_partition: %lld rows, a test aid for at most 4096", (long long)n);
  Rule R;
  PCMI_REQUIRE(rule_of(n_scenes, r1_sq, r2_sq, A, E, &R), PCMI_ERR_INVALID,
               "pnce_partition: needs A in {1,2,4,8}, E in {1,2}, 0 <= r1_sq <= r2_sq and 1..%d scenes", kMaxScenes);
  pnce_partition_kernel<<<dim3((unsigned)ceil_div(n, 256), (unsigned)n), 256, 0, as_stream(stream)>>>(xyz, scene, n, R, part);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

}  // extern "C"
