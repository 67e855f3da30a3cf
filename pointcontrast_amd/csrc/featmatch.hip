// Feature matching between the two clouds of held-out pairs (the validation of FCGF's contrastive trainer, which the
// reference dropped): segmented nearest neighbour in feature space, the geometric check of the matches against the known
// pose, RANSAC hypothesis scoring and the sums of the least-squares refit.  Written from the semantics in include/pcmi.h;
// gfx950, wave64.
//
// Arithmetic.  feat_nn_kernel is fp32: d2 = sum_c fma(a_c - b_c, a_c - b_c, d2) in ascending c, so d2 >= +0 and its bit
// pattern orders like the number; chunks of the reference segment are merged by an integer minimum on (d2 bits << 32 | row),
// which no order of arrival changes.  Everything else is fp64 with every product, sum, quotient and square root rounded on
// its own in the order include/pcmi.h states (no FMA contraction: `fp contract(off)` below; fmaf above is explicit).  The
// only atomics are integer ones.
#include <algorithm>

#include "cellgrid.h"
#include "exact.h"
#include "internal.h"

#pragma clang fp contract(off)

namespace pcmi {
namespace featmatch {

constexpr int kThreads = 256;
constexpr int kTQ = 64, kTS = 64;        // query rows per workgroup, reference rows per tile step (a thread holds 4 x 4)
constexpr int kMaxSeg = 1024;            // every workgroup walks the offsets to find its segment
constexpr int64_t kMinChunk = 256;       // a reference chunk is not cut below this many rows (of the whole call's rows)
constexpr int kMaxChunks = 64;
constexpr unsigned long long kNoKey = ~0ull;
constexpr int kStatCols = PCMI_MATCH_STAT_COLS;
constexpr int kLdsMatches = 512;         // matches staged per step by ransac_score_kernel: 2 x 512 x 3 doubles = 24 KB
constexpr double kDegenerate = 1e-9;

__device__ inline int64_t clampi(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- segmented nearest neighbour in feature space ------------------------------------------------------------------------
// grid.x: the query tiles of all segments, one after the other (ceil(Q / 64) + B bounds their number; a workgroup past the
// last tile leaves); grid.y: the chunks each reference segment is cut into.  The tile's queries stay in LDS, d-major, for
// the whole walk; the reference tile passes through LDS KC channels at a time (32, or 16 where 32 does not divide C), so that C = 128 fits
// (34 + 8.5 KB).
template <int C>
__global__ __launch_bounds__(kThreads) void feat_nn_kernel(const float* __restrict__ qf, int64_t q_ld, int64_t nq,
                                                           const int64_t* __restrict__ q_offs, const float* __restrict__ rf,
                                                           int64_t r_ld, int64_t nr, const int64_t* __restrict__ r_offs,
                                                           const int32_t* __restrict__ query_rows,
                                                           const int64_t* __restrict__ query_offs, int64_t Q, int B, int nch,
                                                           unsigned long long* __restrict__ keys) {
  constexpr int KC = C % 32 == 0 ? 32 : 16;
  static_assert(C % KC == 0 && C % 16 == 0 && C >= 16 && C <= 128, "the channel steps cover the row exactly");
  __shared__ __attribute__((aligned(16))) float sa[C][kTQ + 4];
  __shared__ __attribute__((aligned(16))) float sb[KC][kTS + 4];
  const int t = threadIdx.x, tr = t / 16, tc = t % 16;
  int64_t tile = blockIdx.x, lo = 0, hi = 0;
  int b = 0;
  for (; b < B; ++b) {
    lo = clampi(query_offs[b], 0, Q);
    hi = clampi(query_offs[b + 1], lo, Q);
    const int64_t nt = (hi - lo + kTQ - 1) / kTQ;
    if (tile < nt) break;
    tile -= nt;
  }
  if (b == B) return;
  const int64_t q0 = lo + tile * kTQ;
  const int64_t ql = clampi(q_offs[b], 0, nq), qh = clampi(q_offs[b + 1], ql, nq);
  const int64_t rl = clampi(r_offs[b], 0, nr), rh = clampi(r_offs[b + 1], rl, nr);
  const int64_t cs = ((rh - rl + nch - 1) / nch + kTS - 1) / kTS * kTS;
  const int64_t c_begin = rl + (int64_t)blockIdx.y * cs;
  const int64_t c_end = c_begin + cs < rh ? c_begin + cs : rh;
  if (c_begin >= c_end) return;  // (the whole workgroup: nothing below is reached by a part of it)

  const float fnan = __uint_as_float(0x7fc00000u);
  for (int e = t; e < kTQ * (C / 4); e += kThreads) {
    const int row = e / (C / 4), c4 = e % (C / 4);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    const int64_t qpos = q0 + row;
    if (qpos < hi) {
      const int64_t src = query_rows ? (int64_t)query_rows[qpos] : qpos;
      // a row outside its own segment matches nothing: NaN distances are never chosen
      v = (src >= ql && src < qh) ? *reinterpret_cast<const float4*>(qf + src * q_ld + c4 * 4) : make_float4(fnan, fnan, fnan, fnan);
    }
    sa[c4 * 4 + 0][row] = v.x;
    sa[c4 * 4 + 1][row] = v.y;
    sa[c4 * 4 + 2][row] = v.z;
    sa[c4 * 4 + 3][row] = v.w;
  }
  unsigned long long best[4] = {kNoKey, kNoKey, kNoKey, kNoKey};
  for (int64_t c0 = c_begin; c0 < c_end; c0 += kTS) {
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int kc = 0; kc < C; kc += KC) {
      __syncthreads();
      for (int e = t; e < kTS * (KC / 4); e += kThreads) {
        const int row = e / (KC / 4), c4 = e % (KC / 4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c0 + row < c_end) v = *reinterpret_cast<const float4*>(rf + (c0 + row) * r_ld + kc + c4 * 4);
        sb[c4 * 4 + 0][row] = v.x;
        sb[c4 * 4 + 1][row] = v.y;
        sb[c4 * 4 + 2][row] = v.z;
        sb[c4 * 4 + 3][row] = v.w;
      }
      __syncthreads();
#pragma unroll 8
      for (int d = 0; d < KC; ++d) {
        const float4 av4 = *reinterpret_cast<const float4*>(&sa[kc + d][tr * 4]);
        const float4 bv4 = *reinterpret_cast<const float4*>(&sb[d][tc * 4]);
        const float av[4] = {av4.x, av4.y, av4.z, av4.w}, bv[4] = {bv4.x, bv4.y, bv4.z, bv4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float df = av[i] - bv[j];
            acc[i][j] = fmaf(df, df, acc[i][j]);
          }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t col = c0 + tc * 4 + j;
        if (col < c_end && acc[i][j] < INFINITY) {  // false for NaN and for +inf: such a row is never chosen
          const unsigned long long key = ((unsigned long long)__float_as_uint(acc[i][j]) << 32) | (unsigned long long)(uint32_t)col;
          if (key < best[i]) best[i] = key;
        }
      }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) {
      const unsigned long long o = __shfl_xor(best[i], d, 64);
      if (o < best[i]) best[i] = o;
    }
    const int64_t qpos = q0 + tr * 4 + i;
    if (tc == 0 && qpos < hi && best[i] != kNoKey) atomicMin(&keys[qpos], best[i]);
  }
}

__global__ __launch_bounds__(kThreads) void feat_nn_final_kernel(const unsigned long long* __restrict__ keys, int64_t Q,
                                                                 int32_t* __restrict__ nn, float* __restrict__ d2) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= Q) return;
  const unsigned long long k = keys[i];
  nn[i] = k == kNoKey ? -1 : (int32_t)(uint32_t)(k & 0xffffffffull);
  d2[i] = k == kNoKey ? __uint_as_float(0x7fc00000u) : __uint_as_float((uint32_t)(k >> 32));
}

// ---- the geometric check ---------------------------------------------------------------------------------------------------
struct Taus {
  double t2[PCMI_MATCH_MAX_TAU];
  int n;
};

__global__ __launch_bounds__(kThreads) void match_stats_kernel(const double* __restrict__ xyz0, int64_t n0,
                                                               const double* __restrict__ xyz1, int64_t n1,
                                                               const double* __restrict__ T, int B,
                                                               const int32_t* __restrict__ query_rows,
                                                               const int64_t* __restrict__ query_offs, int64_t Q,
                                                               const int32_t* __restrict__ nn01, const int32_t* __restrict__ nn10,
                                                               const uint8_t* __restrict__ has_gt, Taus taus,
                                                               unsigned long long* __restrict__ counts, double* __restrict__ residual2) {
  __shared__ unsigned s_cnt[kStatCols];
  __shared__ int s_b0;
  const int t = threadIdx.x;
  const int64_t q = (int64_t)blockIdx.x * kThreads + t;
  if (t < kStatCols) s_cnt[t] = 0u;
  if (t == 0) s_b0 = segment_of(query_offs, B, (int64_t)blockIdx.x * kThreads);
  __syncthreads();
  const int b0 = s_b0;
  if (q < Q) {
    const int b = segment_of(query_offs, B, q);
    double r2 = qnan();
    unsigned bits = 0u;  // the columns of counts this query adds one to
    if (b >= 0) {
      bits |= 1u << PCMI_MATCH_N_QUERY;
      const int64_t row = query_rows ? (int64_t)query_rows[q] : q;
      const bool row_ok = row >= 0 && row < n0;
      const bool gt = row_ok && has_gt && has_gt[row] != 0;
      if (gt) bits |= 1u << PCMI_MATCH_N_GT;
      const int64_t j = nn01[q];
      if (row_ok && j >= 0 && j < n1) {
        bits |= 1u << PCMI_MATCH_N_VALID;
        double y[3];
        rigid_apply(T + 16 * b, 4, xyz0 + 3 * row, y);
        r2 = dist2_rn(y, xyz1 + 3 * j);
        for (int k = 0; k < taus.n; ++k)
          if (r2 <= taus.t2[k]) bits |= (1u << (PCMI_MATCH_HITS + k)) | (gt ? 1u << (PCMI_MATCH_HITS_GT + k) : 0u);
        if (nn10 && (int64_t)nn10[q] == row) bits |= 1u << PCMI_MATCH_N_MUTUAL;
      }
    }
    residual2[q] = r2;
    for (int k = 0; k < kStatCols; ++k)
      if (bits >> k & 1u) {
        if (b == b0) atomicAdd(&s_cnt[k], 1u);
        else atomicAdd(&counts[(int64_t)b * kStatCols + k], 1ull);
      }
  }
  __syncthreads();
  if (t < kStatCols && b0 >= 0 && s_cnt[t] != 0u) atomicAdd(&counts[(int64_t)b0 * kStatCols + t], (unsigned long long)s_cnt[t]);
}

// ---- RANSAC ----------------------------------------------------------------------------------------------------------------
// The orthonormal frame of a triangle (include/pcmi.h): e[0] = e1, e[1] = e2, e[2] = e3.  false: degenerate.
__device__ inline bool tri_frame(const double* p0, const double* p1, const double* p2, double e[3][3]) {
  const double u[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
  const double lu = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
  if (!(lu >= kDegenerate)) return false;
#pragma unroll
  for (int k = 0; k < 3; ++k) e[0][k] = u[k] / lu;
  const double v[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
  const double n[3] = {e[0][1] * v[2] - e[0][2] * v[1], e[0][2] * v[0] - e[0][0] * v[2], e[0][0] * v[1] - e[0][1] * v[0]};
  const double ln = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
  if (!(ln >= kDegenerate)) return false;
#pragma unroll
  for (int k = 0; k < 3; ++k) e[2][k] = n[k] / ln;
  e[1][0] = e[2][1] * e[0][2] - e[2][2] * e[0][1];
  e[1][1] = e[2][2] * e[0][0] - e[2][0] * e[0][2];
  e[1][2] = e[2][0] * e[0][1] - e[2][1] * e[0][0];
  return true;
}

// Rt: R row-major in [0, 9), t in [9, 12).  p: three source points, q: their three destinations, 3 doubles each.
__device__ inline bool triple_transform(const double p[3][3], const double q[3][3], double* Rt) {
  double e[3][3], f[3][3];
  if (!tri_frame(p[0], p[1], p[2], e) || !tri_frame(q[0], q[1], q[2], f)) return false;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Rt[3 * i + j] = (f[0][i] * e[0][j] + f[1][i] * e[1][j]) + f[2][i] * e[2][j];
#pragma unroll
  for (int i = 0; i < 3; ++i) Rt[9 + i] = q[0][i] - ((Rt[3 * i] * p[0][0] + Rt[3 * i + 1] * p[0][1]) + Rt[3 * i + 2] * p[0][2]);
  return true;
}

// r2 of one match under Rt
__device__ inline double match_r2(const double* Rt, const double* p, const double* q) {
  double y[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) y[r] = ((Rt[3 * r] * p[0] + Rt[3 * r + 1] * p[1]) + Rt[3 * r + 2] * p[2]) + Rt[9 + r];
  return dist2_rn(y, q);
}

// the hypothesis h of segment [lo, lo + m): false if it is invalid
__device__ inline bool hypothesis(const double* __restrict__ src, const double* __restrict__ dst, int64_t lo, int64_t m,
                                  const int32_t* __restrict__ tri, double* Rt) {
  if (m < 3) return false;
  const int64_t i0 = tri[0], i1 = tri[1], i2 = tri[2];
  if (i0 < 0 || i0 >= m || i1 < 0 || i1 >= m || i2 < 0 || i2 >= m || i0 == i1 || i0 == i2 || i1 == i2) return false;
  const int64_t idx[3] = {lo + i0, lo + i1, lo + i2};
  double p[3][3], q[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      p[a][k] = src[3 * idx[a] + k];
      q[a][k] = dst[3 * idx[a] + k];
    }
  return triple_transform(p, q, Rt);
}

__global__ __launch_bounds__(kThreads) void ransac_score_kernel(const double* __restrict__ src, const double* __restrict__ dst,
                                                                int64_t M, const int64_t* __restrict__ offs, int H,
                                                                const int32_t* __restrict__ triples, double tau2,
                                                                int32_t* __restrict__ counts) {
  __shared__ double sp[kLdsMatches * 3], sq[kLdsMatches * 3];
  const int t = threadIdx.x, b = blockIdx.y;
  const int64_t h = (int64_t)blockIdx.x * kThreads + t;
  const int64_t lo = clampi(offs[b], 0, M), hi = clampi(offs[b + 1], lo, M), m = hi - lo;
  double Rt[12];
  const bool ok = h < H && hypothesis(src, dst, lo, m, triples + ((int64_t)b * H + h) * 3, Rt);
  int32_t cnt = 0;
  for (int64_t base = 0; base < m; base += kLdsMatches) {
    const int n = (int)(m - base < kLdsMatches ? m - base : kLdsMatches);
    __syncthreads();
    for (int e = t; e < 3 * n; e += kThreads) {
      sp[e] = src[3 * (lo + base) + e];
      sq[e] = dst[3 * (lo + base) + e];
    }
    __syncthreads();
    if (ok)
      for (int k = 0; k < n; ++k)
        if (match_r2(Rt, sp + 3 * k, sq + 3 * k) <= tau2) ++cnt;
  }
  if (h < H) counts[(int64_t)b * H + h] = ok ? cnt : -1;
}

// one workgroup per pair: the highest count, the lowest hypothesis among equals; its transform is computed again
__global__ __launch_bounds__(kThreads) void ransac_best_kernel(const double* __restrict__ src, const double* __restrict__ dst,
                                                               int64_t M, const int64_t* __restrict__ offs, int H,
                                                               const int32_t* __restrict__ triples,
                                                               const int32_t* __restrict__ counts, int32_t* __restrict__ best,
                                                               double* __restrict__ Rt_out) {
  __shared__ int32_t s_c[kThreads], s_h[kThreads];
  const int t = threadIdx.x, b = blockIdx.x;
  int32_t bc = -1, bh = 0x7fffffff;
  for (int h = t; h < H; h += kThreads) {
    const int32_t c = counts[(int64_t)b * H + h];
    if (c > bc) {
      bc = c;
      bh = h;
    }
  }
  s_c[t] = bc;
  s_h[t] = bh;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (t < s && (s_c[t + s] > s_c[t] || (s_c[t + s] == s_c[t] && s_h[t + s] < s_h[t]))) {
      s_c[t] = s_c[t + s];
      s_h[t] = s_h[t + s];
    }
    __syncthreads();
  }
  if (t != 0) return;
  double Rt[12];
  bool ok = s_c[0] >= 0;
  if (ok) {
    const int64_t lo = clampi(offs[b], 0, M), hi = clampi(offs[b + 1], lo, M);
    ok = hypothesis(src, dst, lo, hi - lo, triples + ((int64_t)b * H + s_h[0]) * 3, Rt);
  }
  best[b] = ok ? s_h[0] : -1;
  for (int k = 0; k < 12; ++k) Rt_out[12 * b + k] = ok ? Rt[k] : qnan();
}

// ---- sums of the least-squares refit ---------------------------------------------------------------------------------------
// One workgroup per pair, two passes.  Lane t adds the inliers among matches t, t + 256, ... in ascending order; the 256
// partials are folded by halving (x[t] += x[t + s], s = 128 ... 1).  The second pass subtracts the means of the first.
template <int N>
__device__ inline void fold(double (*s)[kThreads], const double* v, int t) {
#pragma unroll
  for (int k = 0; k < N; ++k) s[k][t] = v[k];
  __syncthreads();
  for (int st = kThreads / 2; st > 0; st >>= 1) {
    if (t < st)
#pragma unroll
      for (int k = 0; k < N; ++k) s[k][t] = s[k][t] + s[k][t + st];
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void rigid_sums_kernel(const double* __restrict__ src, const double* __restrict__ dst,
                                                              int64_t M, const int64_t* __restrict__ offs,
                                                              const int32_t* __restrict__ best, const double* __restrict__ Rt_in,
                                                              double tau2, double* __restrict__ out) {
  __shared__ double s[9][kThreads];
  const int t = threadIdx.x, b = blockIdx.x;
  if (best[b] < 0) {  // (the whole workgroup)
    if (t < 16) out[16 * b + t] = 0.0;
    return;
  }
  const int64_t lo = clampi(offs[b], 0, M), hi = clampi(offs[b + 1], lo, M);
  double Rt[12];
  for (int k = 0; k < 12; ++k) Rt[k] = Rt_in[12 * b + k];
  double v[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) v[k] = 0.0;
  for (int64_t i = lo + t; i < hi; i += kThreads)
    if (match_r2(Rt, src + 3 * i, dst + 3 * i) <= tau2) {
      v[0] = v[0] + 1.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        v[1 + k] = v[1 + k] + src[3 * i + k];
        v[4 + k] = v[4 + k] + dst[3 * i + k];
      }
    }
  fold<7>(s, v, t);
  double sums[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) sums[k] = s[k][0];
  __syncthreads();
  double pm[3], qm[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    pm[k] = sums[1 + k] / sums[0];  // (n == 0 only with a tau below round-off: NaN means, no inlier in the second pass, zeros)
    qm[k] = sums[4 + k] / sums[0];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) v[k] = 0.0;
  for (int64_t i = lo + t; i < hi; i += kThreads)
    if (match_r2(Rt, src + 3 * i, dst + 3 * i) <= tau2) {
      double dp[3], dq[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        dp[k] = src[3 * i + k] - pm[k];
        dq[k] = dst[3 * i + k] - qm[k];
      }
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[3 * a + c] = v[3 * a + c] + dp[a] * dq[c];
    }
  fold<9>(s, v, t);
  if (t < 7) out[16 * b + t] = sums[t];
  if (t < 9) out[16 * b + 7 + t] = s[t][0];
}

template <int C>
static void launch_feat_nn(dim3 grid, hipStream_t st, const float* qf, int64_t q_ld, int64_t nq, const int64_t* q_offs,
                           const float* rf, int64_t r_ld, int64_t nr, const int64_t* r_offs, const int32_t* query_rows,
                           const int64_t* query_offs, int64_t Q, int B, int nch, unsigned long long* keys) {
  feat_nn_kernel<C><<<grid, kThreads, 0, st>>>(qf, q_ld, nq, q_offs, rf, r_ld, nr, r_offs, query_rows, query_offs, Q, B, nch, keys);
}

}  // namespace featmatch
}  // namespace pcmi

using namespace pcmi;
using namespace pcmi::featmatch;

extern "C" {

size_t pcmi_feat_nn_workspace_bytes(int64_t n_queries) { return n_queries > 0 ? (size_t)n_queries * sizeof(unsigned long long) : 0; }

int pcmi_feat_nn(const float* qf, int64_t q_ld, int64_t nq, const int64_t* q_offs, const float* rf, int64_t r_ld, int64_t nr,
                 const int64_t* r_offs, int64_t B, int c, const int32_t* query_rows, const int64_t* query_offs,
                 int64_t n_query_rows, int32_t* nn, float* d2, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_REQUIRE(c >= 16 && c <= 128 && c % 16 == 0, PCMI_ERR_UNSUPPORTED, "feat_nn: feature width %d is not a multiple of 16 in 16..128", c);
  PCMI_REQUIRE(B >= 1 && B <= kMaxSeg, PCMI_ERR_UNSUPPORTED, "feat_nn: %lld segments, 1..%d are supported", (long long)B, kMaxSeg);
  PCMI_REQUIRE(nq >= 0 && nr >= 0 && nq < (1ll << 31) - 256 && nr < (1ll << 31) - 256 && q_offs && r_offs, PCMI_ERR_INVALID,
               "feat_nn: bad argument");
  PCMI_REQUIRE((query_rows == nullptr) == (query_offs == nullptr), PCMI_ERR_INVALID, "feat_nn: query_rows and query_offsets go together");
  const int64_t Q = query_rows ? n_query_rows : nq;
  PCMI_REQUIRE(Q >= 0 && Q < (1ll << 31) - 256, PCMI_ERR_INVALID, "feat_nn: bad number of queries");
  if (Q == 0) return PCMI_OK;
  PCMI_REQUIRE(nn && d2 && (nq == 0 || qf) && (nr == 0 || rf), PCMI_ERR_INVALID, "feat_nn: null pointer");
  PCMI_REQUIRE(q_ld >= c && r_ld >= c && q_ld % 4 == 0 && r_ld % 4 == 0 && (uintptr_t)qf % 16 == 0 && (uintptr_t)rf % 16 == 0,
               PCMI_ERR_INVALID, "feat_nn: rows need a stride >= C that is a multiple of 4 floats, and a 16-byte aligned base");
  if (int rc = require_ws("feat_nn", ws, ws_bytes, pcmi_feat_nn_workspace_bytes(Q), 1)) return rc;
  // (this entry reports a misaligned base as a workspace error, not as an invalid argument)
  PCMI_REQUIRE((uintptr_t)ws % 8 == 0, PCMI_ERR_WORKSPACE, "feat_nn: workspace must be 8-byte aligned");
  hipStream_t st = as_stream(stream);
  unsigned long long* keys = static_cast<unsigned long long*>(ws);
  PCMI_HIP_CHECK(hipMemsetAsync(keys, 0xff, (size_t)Q * sizeof(unsigned long long), st));
  const int64_t tiles = ceil_div(Q, kTQ) + B;
  // enough workgroups for the chip: the reference segments are cut where the query tiles alone are too few
  const int nch = (int)std::max<int64_t>(1, std::min<int64_t>({ceil_div(4 * (int64_t)num_cu(), tiles), ceil_div(nr, kMinChunk), (int64_t)kMaxChunks}));
  const dim3 grid((unsigned)tiles, (unsigned)nch);
  const int64_t* qo = query_rows ? query_offs : q_offs;
#define PCMI_FEAT_NN_CASE(W) \
  case W: launch_feat_nn<W>(grid, st, qf, q_ld, nq, q_offs, rf, r_ld, nr, r_offs, query_rows, qo, Q, (int)B, nch, keys); break;
  switch (c) {
    PCMI_FEAT_NN_CASE(16)
    PCMI_FEAT_NN_CASE(32)
    PCMI_FEAT_NN_CASE(48)
    PCMI_FEAT_NN_CASE(64)
    PCMI_FEAT_NN_CASE(80)
    PCMI_FEAT_NN_CASE(96)
    PCMI_FEAT_NN_CASE(112)
    PCMI_FEAT_NN_CASE(128)
  }
#undef PCMI_FEAT_NN_CASE
  PCMI_LAUNCH_CHECK();
  feat_nn_final_kernel<<<(unsigned)ceil_div(Q, kThreads), kThreads, 0, st>>>(keys, Q, nn, d2);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

int pcmi_match_stats(const double* xyz0, int64_t n0, const double* xyz1, int64_t n1, const double* T_gt, int64_t B,
                     const int32_t* query_rows, const int64_t* query_offs, int64_t n_queries, const int32_t* nn01,
                     const int32_t* nn10, const uint8_t* has_gt, const double* tau_host, int n_tau, int64_t* counts,
                     double* residual2, pcmi_stream_t stream) {
  PCMI_REQUIRE(B >= 1 && B <= kMaxSeg, PCMI_ERR_UNSUPPORTED, "match_stats: %lld pairs, 1..%d are supported", (long long)B, kMaxSeg);
  PCMI_REQUIRE(n_tau >= 1 && n_tau <= PCMI_MATCH_MAX_TAU && tau_host, PCMI_ERR_INVALID, "match_stats: 1..%d thresholds", PCMI_MATCH_MAX_TAU);
  PCMI_REQUIRE(n0 >= 0 && n1 >= 0 && n_queries >= 0 && n0 < (1ll << 31) - 256 && n1 < (1ll << 31) - 256 && n_queries < (1ll << 31) - 256,
               PCMI_ERR_INVALID, "match_stats: bad row count");
  PCMI_REQUIRE(query_rows || n_queries == n0, PCMI_ERR_INVALID, "match_stats: without query_rows every row of cloud 0 is a query");
  if (n_queries == 0) return PCMI_OK;
  PCMI_REQUIRE(T_gt && query_offs && nn01 && counts && residual2 && (n0 == 0 || xyz0) && (n1 == 0 || xyz1), PCMI_ERR_INVALID,
               "match_stats: null pointer");
  Taus taus;
  taus.n = n_tau;
  for (int k = 0; k < PCMI_MATCH_MAX_TAU; ++k) taus.t2[k] = k < n_tau ? tau_host[k] * tau_host[k] : 0.0;
  match_stats_kernel<<<(unsigned)ceil_div(n_queries, kThreads), kThreads, 0, as_stream(stream)>>>(
      xyz0, n0, xyz1, n1, T_gt, (int)B, query_rows, query_offs, n_queries, nn01, nn10, has_gt, taus,
      reinterpret_cast<unsigned long long*>(counts), residual2);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

int pcmi_ransac_score(const double* src, const double* dst, int64_t m, const int64_t* offsets, int64_t B, const int32_t* triples,
                      int64_t H, double tau, int32_t* counts, int32_t* best, double* Rt, pcmi_stream_t stream) {
  PCMI_REQUIRE(B >= 1 && B <= kMaxSeg, PCMI_ERR_UNSUPPORTED, "ransac_score: %lld pairs, 1..%d are supported", (long long)B, kMaxSeg);
  PCMI_REQUIRE(H >= 1 && H <= 65536, PCMI_ERR_UNSUPPORTED, "ransac_score: %lld hypotheses, 1..65536 are supported", (long long)H);
  PCMI_REQUIRE(m >= 0 && m < (1ll << 31) - 256 && offsets && triples && counts && best && Rt && (m == 0 || (src && dst)) && tau >= 0.0,
               PCMI_ERR_INVALID, "ransac_score: bad argument");
  hipStream_t st = as_stream(stream);
  ransac_score_kernel<<<dim3((unsigned)ceil_div(H, kThreads), (unsigned)B), kThreads, 0, st>>>(src, dst, m, offsets, (int)H, triples,
                                                                                              tau * tau, counts);
  PCMI_LAUNCH_CHECK();
  ransac_best_kernel<<<(unsigned)B, kThreads, 0, st>>>(src, dst, m, offsets, (int)H, triples, counts, best, Rt);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

int pcmi_rigid_sums(const double* src, const double* dst, int64_t m, const int64_t* offsets, int64_t B, const int32_t* best,
                    const double* Rt, double tau, double* sums, pcmi_stream_t stream) {
  PCMI_REQUIRE(B >= 1 && B <= kMaxSeg, PCMI_ERR_UNSUPPORTED, "rigid_sums: %lld pairs, 1..%d are supported", (long long)B, kMaxSeg);
  PCMI_REQUIRE(m >= 0 && m < (1ll << 31) - 256 && offsets && best && Rt && sums && (m == 0 || (src && dst)) && tau >= 0.0,
               PCMI_ERR_INVALID, "rigid_sums: bad argument");
  rigid_sums_kernel<<<(unsigned)B, kThreads, 0, as_stream(stream)>>>(src, dst, m, offsets, best, Rt, tau * tau, sums);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

}  // extern "C"
