// The PointNet++ backbone's two row kernels beyond csrc/votehead.hip (downstream/votenet_det_new of the reference:
// models/backbone/pointnet2/pointnet2_modules.py PointnetSAModuleVotes.forward:251-257 -- the last SharedMLP layer's
// BatchNorm + ReLU and the max_pool2d over nsample behind it -- and PointnetFPModule.forward:394-409 -- three_interpolate
// and the concatenation with the skip features).  Written from the semantics in include/pcmi.h; gfx950, wave64, fp32 data,
// int32 indices, row-major activations [rows, ld].
//
// bn_maxpool: y = relu(gamma (x - mean) invstd + beta) is never stored.  The forward reads x twice (column sums, then the
// pooling pass that recomputes y per element and keeps the maximum of every ns consecutive rows and its row), the backward
// reads x once and writes dx once; its two column sums run over the R pooled rows only.  Every column sum: fp64 partials per
// (row chunk, column), rows in ascending order inside a chunk, the chunks merged in a fixed order (per lane ascending, then
// an xor butterfly) -- no float atomics, the same bits from run to run.
// interp_rows: one wave per row, as group_rows_fwd; the backward in gather form over pointset.hip's inverse lists.
// Contraction is off for the whole file: each operation is rounded on its own.
#include <algorithm>
#include <cmath>

#include "internal.h"

#pragma clang fp contract(off)

namespace pcmi {
namespace rowspool {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTargetChunks = 1024;  // row chunks of a column sum: about four workgroups per CU at one column tile
constexpr int kMinChunkRows = 32;

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// rows per chunk of a column sum over `rows` rows: a multiple of 8 (both tile shapes' row lanes divide it)
static inline int64_t chunk_rows(int64_t rows) {
  return (std::max<int64_t>(ceil_div(std::max<int64_t>(rows, 1), kTargetChunks), kMinChunkRows) + 7) / 8 * 8;
}
static inline int64_t n_chunks(int64_t rows) { return ceil_div(std::max<int64_t>(rows, 1), chunk_rows(rows)); }

// ---- column sums ----------------------------------------------------------------------------------------------------
// The two addends of element (row, column): x and x^2 for the batch statistics ...
struct StatsOp {
  const float* x;
  int64_t x_ld;
  template <int V>
  __device__ __forceinline__ void load(int64_t row, int c, float (&a)[V], float (&b)[V]) const {
    const float* p = x + row * x_ld + c;
    if constexpr (V == 4) {
      const float4 v = *reinterpret_cast<const float4*>(p);
      a[0] = v.x; a[1 % V] = v.y; a[2 % V] = v.z; a[3 % V] = v.w;
    } else {
      a[0] = p[0];
    }
#pragma unroll
    for (int e = 0; e < V; ++e) b[e] = a[e];
  }
};

// ... and g, g xhat for the parameter gradients: g = gout where out > 0, xhat from the window's argument row of x
struct GradOp {
  const float* gout; int64_t gout_ld;
  const float* out; int64_t out_ld;
  const uint8_t* arg;
  const float* x; int64_t x_ld;
  const float* mean; const float* invstd;
  int ns, C;
  template <int V>
  __device__ __forceinline__ void load(int64_t r, int c, float (&a)[V], float (&b)[V]) const {
    float g[V], o[V];
    int s[V];
    if constexpr (V == 4) {
      const float4 gv = *reinterpret_cast<const float4*>(gout + r * gout_ld + c);
      const float4 ov = *reinterpret_cast<const float4*>(out + r * out_ld + c);
      const uchar4 av = *reinterpret_cast<const uchar4*>(arg + r * C + c);
      g[0] = gv.x; g[1 % V] = gv.y; g[2 % V] = gv.z; g[3 % V] = gv.w;
      o[0] = ov.x; o[1 % V] = ov.y; o[2 % V] = ov.z; o[3 % V] = ov.w;
      s[0] = av.x; s[1 % V] = av.y; s[2 % V] = av.z; s[3 % V] = av.w;
    } else {
      g[0] = gout[r * gout_ld + c];
      o[0] = out[r * out_ld + c];
      s[0] = arg[r * C + c];
    }
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const int se = s[e] < ns ? s[e] : 0;  // an argument outside the window is never followed
      const float xv = x[(r * ns + se) * x_ld + c + e];
      a[e] = o[e] > 0.f ? g[e] : 0.f;
      b[e] = (xv - mean[c + e]) * invstd[c + e];
    }
  }
};

// grid (chunk, column tile); a tile is TC = 128 columns by 8 row lanes (V == 4) or 64 columns by 4 row lanes (V == 1).
// part[chunk][0][c] = sum of a, part[chunk][1][c] = sum of a * b (fp64), rows in ascending order per row lane, the row lanes
// added in ascending order.
template <int V, class Op>
__global__ __launch_bounds__(kThreads) void colsum_kernel(Op op, int64_t rows, int64_t rows_per_chunk, int C, double* __restrict__ part) {
  constexpr int CG = V == 4 ? 32 : 64;  // column groups per tile
  constexpr int RL = kThreads / CG;     // row lanes
  constexpr int TC = CG * V;
  __shared__ double sh[2][RL][TC];
  const int tx = threadIdx.x % CG, ty = threadIdx.x / CG;
  const int c = blockIdx.y * TC + tx * V;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_chunk, r1 = min(r0 + rows_per_chunk, rows);
  double s0[V], s1[V];
#pragma unroll
  for (int e = 0; e < V; ++e) s0[e] = s1[e] = 0.0;
  if (c < C) {
    int64_t r = r0 + ty;
    for (; r + 3 * RL < r1; r += 4 * RL) {  // four rows in flight
      float a[4][V], b[4][V];
#pragma unroll
      for (int u = 0; u < 4; ++u) op.template load<V>(r + u * RL, c, a[u], b[u]);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int e = 0; e < V; ++e) {
          s0[e] += (double)a[u][e];
          s1[e] += (double)a[u][e] * (double)b[u][e];
        }
    }
    for (; r < r1; r += RL) {
      float a[V], b[V];
      op.template load<V>(r, c, a, b);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        s0[e] += (double)a[e];
        s1[e] += (double)a[e] * (double)b[e];
      }
    }
  }
#pragma unroll
  for (int e = 0; e < V; ++e) {
    sh[0][ty][tx * V + e] = s0[e];
    sh[1][ty][tx * V + e] = s1[e];
  }
  __syncthreads();
  for (int o = threadIdx.x; o < 2 * TC; o += kThreads) {
    const int v = o / TC, cc = o - v * TC, col = blockIdx.y * TC + cc;
    if (col >= C) continue;
    double t = 0.0;
#pragma unroll
    for (int l = 0; l < RL; ++l) t += sh[v][l][cc];
    part[((int64_t)blockIdx.x * 2 + v) * C + col] = t;
  }
}

// One wave per column: lane l adds the chunks l, l + 64, ... in ascending order, then the xor butterfly.
__device__ __forceinline__ void merge_column(const double* __restrict__ part, int64_t chunks, int C, int col, double& t0, double& t1) {
  const int lane = threadIdx.x & 63;
  t0 = t1 = 0.0;
  for (int64_t k = lane; k < chunks; k += 64) {
    t0 += part[(k * 2) * C + col];
    t1 += part[(k * 2 + 1) * C + col];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    t0 = t0 + __shfl_xor(t0, off, 64);
    t1 = t1 + __shfl_xor(t1, off, 64);
  }
}

// the batch statistics from (sum x, sum x^2): biased variance for the normalisation, unbiased for the running estimate
// (one row: the biased one, as pcmi_bn_fwd_train), momentum as torch
__global__ __launch_bounds__(kThreads) void stats_merge_kernel(const double* __restrict__ part, int64_t chunks, int64_t n, int C, float eps,
                                                               float momentum, float* __restrict__ running_mean,
                                                               float* __restrict__ running_var, float* __restrict__ save_mean,
                                                               float* __restrict__ save_invstd) {
  const int col = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (col >= C) return;
  double s, q;
  merge_column(part, chunks, C, col, s, q);
  if ((threadIdx.x & 63) != 0) return;
  const double mean = s / (double)n;
  double var = q / (double)n - mean * mean;
  var = var < 0.0 ? 0.0 : var;  // a NaN stays a NaN
  const float meanf = (float)mean, varf = (float)var;
  save_mean[col] = meanf;
  save_invstd[col] = (float)(1.0 / sqrt(var + (double)eps));
  const float unbiased = n > 1 ? (float)(var * ((double)n / (double)(n - 1))) : varf;
  if (running_mean) {
    running_mean[col] = (1.f - momentum) * running_mean[col] + momentum * meanf;
    running_var[col] = (1.f - momentum) * running_var[col] + momentum * unbiased;
  }
}

__global__ __launch_bounds__(kThreads) void grad_merge_kernel(const double* __restrict__ part, int64_t chunks, int C,
                                                              float* __restrict__ dbeta, float* __restrict__ dgamma) {
  const int col = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (col >= C) return;
  double s, q;
  merge_column(part, chunks, C, col, s, q);
  if ((threadIdx.x & 63) != 0) return;
  dbeta[col] = (float)s;
  dgamma[col] = (float)q;
}

// ---- the pooling pass -------------------------------------------------------------------------------------------------
// One thread per (pooled row, V adjacent columns), the window's ns rows in ascending order, four loads in flight.
// y = relu((x - mean) * (invstd * gamma) + beta); strict > keeps the lowest row among equals; a NaN takes the result and is
// never replaced.  FROM_VAR: `stat` holds a variance (the running estimate), invstd = 1 / sqrt(var + eps).
__device__ __forceinline__ float bn_relu(float x, float mean, float scale, float beta) {
  const float y = (x - mean) * scale + beta;
  return y > 0.f ? y : (y != y ? y : 0.f);
}

template <int V, bool FROM_VAR>
__global__ __launch_bounds__(kThreads) void bn_maxpool_fwd_kernel(const float* __restrict__ x, int64_t x_ld, int64_t R, int ns, int C,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  const float* __restrict__ mean, const float* __restrict__ stat, float eps,
                                                                  float* __restrict__ out, int64_t out_ld, uint8_t* __restrict__ arg) {
  const int cg = C / V;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= R * cg) return;
  const int64_t r = i / cg;
  const int c = (int)(i - r * cg) * V;
  float mu[V], sc[V], be[V], m[V];
  uint8_t a[V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
    float is = stat[c + e];
    if (FROM_VAR) is = 1.0f / sqrtf(is + eps);
    mu[e] = mean[c + e];
    sc[e] = is * gamma[c + e];
    be[e] = beta[c + e];
    a[e] = 0;
  }
  const float* p = x + r * ns * x_ld + c;
  auto load = [&](int s, float (&v)[V]) {
    if constexpr (V == 4) {
      const float4 q = *reinterpret_cast<const float4*>(p + s * x_ld);
      v[0] = q.x; v[1 % V] = q.y; v[2 % V] = q.z; v[3 % V] = q.w;
    } else {
      v[0] = p[s * x_ld];
    }
  };
  auto take = [&](int s, const float (&v)[V]) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const float y = bn_relu(v[e], mu[e], sc[e], be[e]);
      if (m[e] == m[e] && (y > m[e] || y != y)) {
        m[e] = y;
        a[e] = (uint8_t)s;
      }
    }
  };
  {
    float v[V];
    load(0, v);
#pragma unroll
    for (int e = 0; e < V; ++e) m[e] = bn_relu(v[e], mu[e], sc[e], be[e]);
  }
  int s = 1;
  for (; s + 3 < ns; s += 4) {
    float v[4][V];
#pragma unroll
    for (int u = 0; u < 4; ++u) load(s + u, v[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) take(s + u, v[u]);
  }
  for (; s < ns; ++s) {
    float v[V];
    load(s, v);
    take(s, v);
  }
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(out + r * out_ld + c) = make_float4(m[0], m[1 % V], m[2 % V], m[3 % V]);
    if (arg) *reinterpret_cast<uchar4*>(arg + r * C + c) = make_uchar4(a[0], a[1 % V], a[2 % V], a[3 % V]);
  } else {
    out[r * out_ld + c] = m[0];
    if (arg) arg[r * C + c] = a[0];
  }
}

// dx[(r ns + s), c] = gamma invstd (g - dbeta / n - xhat dgamma / n), g = gout[r, c] at s == arg[r, c] where out[r, c] > 0,
// else 0: one thread per (pooled row, V columns) writes its window's ns rows, four in flight.
template <int V>
__global__ __launch_bounds__(kThreads) void bn_maxpool_bwd_kernel(const float* __restrict__ gout, int64_t gout_ld, const float* __restrict__ x,
                                                                  int64_t x_ld, const float* __restrict__ out, int64_t out_ld,
                                                                  const uint8_t* __restrict__ arg, int64_t R, int ns, int C,
                                                                  const float* __restrict__ gamma, const float* __restrict__ mean,
                                                                  const float* __restrict__ invstd, const float* __restrict__ dbeta,
                                                                  const float* __restrict__ dgamma, float inv_n, float* __restrict__ dx,
                                                                  int64_t dx_ld) {
  const int cg = C / V;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= R * cg) return;
  const int64_t r = i / cg;
  const int c = (int)(i - r * cg) * V;
  float mu[V], is[V], sc[V], mb[V], mg[V], g[V];
  int a[V];
  if constexpr (V == 4) {
    const float4 gv = *reinterpret_cast<const float4*>(gout + r * gout_ld + c);
    const float4 ov = *reinterpret_cast<const float4*>(out + r * out_ld + c);
    const uchar4 av = *reinterpret_cast<const uchar4*>(arg + r * C + c);
    g[0] = ov.x > 0.f ? gv.x : 0.f; g[1 % V] = ov.y > 0.f ? gv.y : 0.f;
    g[2 % V] = ov.z > 0.f ? gv.z : 0.f; g[3 % V] = ov.w > 0.f ? gv.w : 0.f;
    a[0] = av.x; a[1 % V] = av.y; a[2 % V] = av.z; a[3 % V] = av.w;
  } else {
    g[0] = out[r * out_ld + c] > 0.f ? gout[r * gout_ld + c] : 0.f;
    a[0] = arg[r * C + c];
  }
#pragma unroll
  for (int e = 0; e < V; ++e) {
    mu[e] = mean[c + e];
    is[e] = invstd[c + e];
    sc[e] = gamma[c + e] * is[e];
    mb[e] = dbeta[c + e] * inv_n;
    mg[e] = dgamma[c + e] * inv_n;
    a[e] = a[e] < ns ? a[e] : 0;  // as GradOp
  }
  const float* p = x + r * ns * x_ld + c;
  float* d = dx + r * ns * dx_ld + c;
  auto one = [&](int s, const float (&v)[V]) {
    float o[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const float xh = (v[e] - mu[e]) * is[e];
      o[e] = sc[e] * (((a[e] == s ? g[e] : 0.f) - mb[e]) - xh * mg[e]);
    }
    if constexpr (V == 4)
      *reinterpret_cast<float4*>(d + s * dx_ld) = make_float4(o[0], o[1 % V], o[2 % V], o[3 % V]);
    else
      d[s * dx_ld] = o[0];
  };
  auto load = [&](int s, float (&v)[V]) {
    if constexpr (V == 4) {
      const float4 q = *reinterpret_cast<const float4*>(p + s * x_ld);
      v[0] = q.x; v[1 % V] = q.y; v[2 % V] = q.z; v[3 % V] = q.w;
    } else {
      v[0] = p[s * x_ld];
    }
  };
  int s = 0;
  for (; s + 3 < ns; s += 4) {
    float v[4][V];
#pragma unroll
    for (int u = 0; u < 4; ++u) load(s + u, v[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) one(s + u, v[u]);
  }
  for (; s < ns; ++s) {
    float v[V];
    load(s, v);
    one(s, v);
  }
}

// ---- interp_rows ------------------------------------------------------------------------------------------------------
__global__ void index_flag_kernel(const int32_t* __restrict__ idx, int64_t count, int64_t n, unsigned* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < count && (idx[i] < 0 || idx[i] >= n)) atomicOr(flag, 1u);
}

// One wave per row r = b n + i: out[r, 0:C2] = ((w0 f0) + (w1 f1)) + (w2 f2), f_k = known[b m + idx[r, k]] (0 for an index
// outside [0, m), never dereferenced); out[r, C2:C2 + C1] = skip[r]; zeros up to out_ld.
template <bool VECK, bool VECS>
__global__ __launch_bounds__(kThreads) void interp_rows_fwd_kernel(const float* __restrict__ known, int64_t known_ld,
                                                                   const int32_t* __restrict__ idx, const float* __restrict__ weight,
                                                                   const float* __restrict__ skip, int64_t skip_ld, int64_t rows, int64_t m,
                                                                   int64_t n, int C2, int C1, float* __restrict__ out, int64_t out_ld) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int64_t b = r / n;
  const float* f[3];
  float w[3];
  bool ok[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int32_t t = idx[r * 3 + k];
    ok[k] = t >= 0 && t < m;
    f[k] = known + (b * m + (ok[k] ? t : 0)) * known_ld;
    w[k] = weight[r * 3 + k];
  }
  float* o = out + r * out_ld;
  if (VECK) {
    for (int c = lane * 4; c < C2; c += 256) {
      float4 v[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok[k]) v[k] = *reinterpret_cast<const float4*>(f[k] + c);
      }
      *reinterpret_cast<float4*>(o + c) =
          make_float4(((w[0] * v[0].x) + (w[1] * v[1].x)) + (w[2] * v[2].x), ((w[0] * v[0].y) + (w[1] * v[1].y)) + (w[2] * v[2].y),
                      ((w[0] * v[0].z) + (w[1] * v[1].z)) + (w[2] * v[2].z), ((w[0] * v[0].w) + (w[1] * v[1].w)) + (w[2] * v[2].w));
    }
  } else {
    for (int c = lane; c < C2; c += 64) {
      float v[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) v[k] = ok[k] ? f[k][c] : 0.f;
      o[c] = ((w[0] * v[0]) + (w[1] * v[1])) + (w[2] * v[2]);
    }
  }
  if (C1 > 0) {
    const float* s = skip + r * skip_ld;
    if (VECS) {
      for (int c = lane * 4; c < C1; c += 256) *reinterpret_cast<float4*>(o + C2 + c) = *reinterpret_cast<const float4*>(s + c);
    } else {
      for (int c = lane; c < C1; c += 64) o[C2 + c] = s[c];
    }
  }
  for (int64_t c = (int64_t)C2 + C1 + lane; c < out_ld; c += 64) o[c] = 0.f;
}

// One wave per known point T = b m + t: gknown[T, :] = the sum over the slots pos[start[T] .. start[T + 1]) that named it
// (slot p = (row) 3 + k, ascending) of weight[p] * gout[p / 3, :].  The lists never hold a slot whose index was out of range.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void interp_rows_bwd_kernel(const float* __restrict__ gout, int64_t gout_ld,
                                                                   const float* __restrict__ weight, const int32_t* __restrict__ start,
                                                                   const int32_t* __restrict__ pos, int64_t targets, int C2,
                                                                   float* __restrict__ gknown, int64_t gknown_ld) {
  const int lane = threadIdx.x & 63;
  const int64_t T = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (T >= targets) return;
  const int32_t s = start[T], e = start[T + 1];
  if (VEC) {
    for (int c = lane * 4; c < C2; c += 256) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int32_t i = s; i < e; ++i) {
        const int32_t p = pos[i];
        const float w = weight[p];
        const float4 v = *reinterpret_cast<const float4*>(gout + (int64_t)(p / 3) * gout_ld + c);
        acc.x = acc.x + w * v.x;
        acc.y = acc.y + w * v.y;
        acc.z = acc.z + w * v.z;
        acc.w = acc.w + w * v.w;
      }
      *reinterpret_cast<float4*>(gknown + T * gknown_ld + c) = acc;
    }
  } else {
    for (int c = lane; c < C2; c += 64) {
      float acc = 0.f;
      for (int32_t i = s; i < e; ++i) {
        const int32_t p = pos[i];
        acc = acc + weight[p] * gout[(int64_t)(p / 3) * gout_ld + c];
      }
      gknown[T * gknown_ld + c] = acc;
    }
  }
}

// row and column counts the 32-bit launch grids cover (addresses are 64-bit throughout)
static bool rows_fit(int64_t rows, int64_t ld) { return rows >= 0 && rows < (1ll << 31) && ld >= 0 && ld < (1ll << 31) && rows * ld < (1ll << 38); }

static int maxpool_shape_ok(const char* who, int64_t R, int ns, int C, int64_t x_ld, int64_t out_ld) {
  PCMI_REQUIRE(ns >= 1 && ns <= 256, PCMI_ERR_UNSUPPORTED, "%s: %d rows per window, supported: 1 .. 256", who, ns);
  PCMI_REQUIRE(R >= 0 && C >= 0 && x_ld >= C && out_ld >= C && rows_fit(R * ns, x_ld) && rows_fit(R, out_ld), PCMI_ERR_INVALID,
               "%s: bad shape (R %lld, C %d, x_ld %lld, out_ld %lld)", who, (long long)R, C, (long long)x_ld, (long long)out_ld);
  return PCMI_OK;
}

static size_t maxpool_workspace(int64_t R, int ns, int C) {
  return align_up(sizeof(double) * 2 * (size_t)std::max(C, 1) * (size_t)n_chunks(std::max<int64_t>(R, 1) * std::max(ns, 1)), 256);
}

template <class Op>
static int colsum(const Op& op, bool vec, int64_t rows, int C, double* part, int64_t* chunks_out, hipStream_t st) {
  const int64_t rpc = chunk_rows(rows), chunks = ceil_div(rows, rpc);
  if (vec)
    colsum_kernel<4, Op><<<dim3((unsigned)chunks, (unsigned)ceil_div(C, 128)), kThreads, 0, st>>>(op, rows, rpc, C, part);
  else
    colsum_kernel<1, Op><<<dim3((unsigned)chunks, (unsigned)ceil_div(C, 64)), kThreads, 0, st>>>(op, rows, rpc, C, part);
  PCMI_LAUNCH_CHECK();
  *chunks_out = chunks;
  return PCMI_OK;
}

}  // namespace rowspool
}  // namespace pcmi

using namespace pcmi;
using namespace pcmi::rowspool;

extern "C" {

size_t pcmi_bn_maxpool_workspace_bytes(int64_t R, int ns, int c) { return maxpool_workspace(R, ns, c); }

int pcmi_bn_maxpool_fwd_train(const float* x, int64_t x_ld, int64_t R, int ns, int C, const float* gamma, const float* beta,
                              float* running_mean, float* running_var, float momentum, float eps, float* out, int64_t out_ld,
                              uint8_t* arg, float* save_mean, float* save_invstd, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  const int rc = maxpool_shape_ok("bn_maxpool_fwd_train", R, ns, C, x_ld, out_ld);
  if (rc != PCMI_OK) return rc;
  PCMI_REQUIRE((running_mean == nullptr) == (running_var == nullptr), PCMI_ERR_INVALID,
               "bn_maxpool_fwd_train: running_mean and running_var are given together or not at all");
  if (R == 0 || C == 0) return PCMI_OK;
  PCMI_REQUIRE(x && gamma && beta && out && arg && save_mean && save_invstd, PCMI_ERR_INVALID, "bn_maxpool_fwd_train: null pointer");
  if (int ws_rc = require_ws("bn_maxpool_fwd_train", ws, ws_bytes, maxpool_workspace(R, ns, C), 1)) return ws_rc;
  hipStream_t st = as_stream(stream);
  const int64_t n = R * ns;
  const bool vx = C % 4 == 0 && x_ld % 4 == 0 && aligned16(x);
  double* part = static_cast<double*>(ws);
  int64_t chunks = 0;
  const int rc2 = colsum(StatsOp{x, x_ld}, vx, n, C, part, &chunks, st);
  if (rc2 != PCMI_OK) return rc2;
  stats_merge_kernel<<<(unsigned)ceil_div(C, kWaves), kThreads, 0, st>>>(part, chunks, n, C, eps, momentum, running_mean, running_var,
                                                                        save_mean, save_invstd);
  PCMI_LAUNCH_CHECK();
  if (vx && out_ld % 4 == 0 && aligned16(out) && ((uintptr_t)arg & 3) == 0)
    bn_maxpool_fwd_kernel<4, false><<<(unsigned)ceil_div(R * (C / 4), kThreads), kThreads, 0, st>>>(x, x_ld, R, ns, C, gamma, beta, save_mean,
                                                                                                   save_invstd, eps, out, out_ld, arg);
  else
    bn_maxpool_fwd_kernel<1, false><<<(unsigned)ceil_div(R * C, kThreads), kThreads, 0, st>>>(x, x_ld, R, ns, C, gamma, beta, save_mean,
                                                                                             save_invstd, eps, out, out_ld, arg);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

int pcmi_bn_maxpool_fwd_eval(const float* x, int64_t x_ld, int64_t R, int ns, int C, const float* gamma, const float* beta,
                             const float* running_mean, const float* running_var, float eps, float* out, int64_t out_ld, uint8_t* arg,
                             pcmi_stream_t stream) {
  const int rc = maxpool_shape_ok("bn_maxpool_fwd_eval", R, ns, C, x_ld, out_ld);
  if (rc != PCMI_OK) return rc;
  if (R == 0 || C == 0) return PCMI_OK;
  PCMI_REQUIRE(x && gamma && beta && running_mean && running_var && out, PCMI_ERR_INVALID, "bn_maxpool_fwd_eval: null pointer");
  hipStream_t st = as_stream(stream);
  if (C % 4 == 0 && x_ld % 4 == 0 && out_ld % 4 == 0 && aligned16(x) && aligned16(out) && ((uintptr_t)arg & 3) == 0)
    bn_maxpool_fwd_kernel<4, true><<<(unsigned)ceil_div(R * (C / 4), kThreads), kThreads, 0, st>>>(x, x_ld, R, ns, C, gamma, beta, running_mean,
                                                                                                  running_var, eps, out, out_ld, arg);
  else
    bn_maxpool_fwd_kernel<1, true><<<(unsigned)ceil_div(R * C, kThreads), kThreads, 0, st>>>(x, x_ld, R, ns, C, gamma, beta, running_mean,
                                                                                            running_var, eps, out, out_ld, arg);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

int pcmi_bn_maxpool_bwd(const float* gout, int64_t gout_ld, const float* x, int64_t x_ld, const float* out, int64_t out_ld,
                        const uint8_t* arg, int64_t R, int ns, int C, const float* gamma, const float* save_mean,
                        const float* save_invstd, float* dx, int64_t dx_ld, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                        pcmi_stream_t stream) {
  const int rc = maxpool_shape_ok("bn_maxpool_bwd", R, ns, C, x_ld, out_ld);
  if (rc != PCMI_OK) return rc;
  PCMI_REQUIRE(gout_ld >= C && dx_ld >= C && rows_fit(R * ns, dx_ld) && rows_fit(R, gout_ld), PCMI_ERR_INVALID,
               "bn_maxpool_bwd: bad shape (C %d, gout_ld %lld, dx_ld %lld)", C, (long long)gout_ld, (long long)dx_ld);
  if (R == 0 || C == 0) return PCMI_OK;
  PCMI_REQUIRE(gout && x && out && arg && gamma && save_mean && save_invstd && dx && dgamma && dbeta, PCMI_ERR_INVALID,
               "bn_maxpool_bwd: null pointer");
  if (int ws_rc = require_ws("bn_maxpool_bwd", ws, ws_bytes, maxpool_workspace(R, ns, C), 1)) return ws_rc;
  hipStream_t st = as_stream(stream);
  const bool vec = C % 4 == 0 && x_ld % 4 == 0 && out_ld % 4 == 0 && gout_ld % 4 == 0 && dx_ld % 4 == 0 && aligned16(x) && aligned16(out) &&
                   aligned16(gout) && aligned16(dx) && ((uintptr_t)arg & 3) == 0;
  double* part = static_cast<double*>(ws);
  int64_t chunks = 0;
  const int rc2 = colsum(GradOp{gout, gout_ld, out, out_ld, arg, x, x_ld, save_mean, save_invstd, ns, C}, vec, R, C, part, &chunks, st);
  if (rc2 != PCMI_OK) return rc2;
  grad_merge_kernel<<<(unsigned)ceil_div(C, kWaves), kThreads, 0, st>>>(part, chunks, C, dbeta, dgamma);
  PCMI_LAUNCH_CHECK();
  const float inv_n = 1.0f / (float)(R * ns);
  if (vec)
    bn_maxpool_bwd_kernel<4><<<(unsigned)ceil_div(R * (C / 4), kThreads), kThreads, 0, st>>>(gout, gout_ld, x, x_ld, out, out_ld, arg, R, ns, C,
                                                                                            gamma, save_mean, save_invstd, dbeta, dgamma, inv_n,
                                                                                            dx, dx_ld);
  else
    bn_maxpool_bwd_kernel<1><<<(unsigned)ceil_div(R * C, kThreads), kThreads, 0, st>>>(gout, gout_ld, x, x_ld, out, out_ld, arg, R, ns, C, gamma,
                                                                                      save_mean, save_invstd, dbeta, dgamma, inv_n, dx, dx_ld);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

static int interp_shape_ok(const char* who, int64_t B, int64_t m, int64_t n, int C2) {
  PCMI_REQUIRE(B >= 0 && m >= 0 && n >= 0 && C2 >= 0 && B * n < ((1ll << 31) - 1) / 3 && B * m < (1ll << 31) - 1, PCMI_ERR_INVALID,
               "%s: bad shape (B %lld, m %lld, n %lld, C2 %d)", who, (long long)B, (long long)m, (long long)n, C2);
  return PCMI_OK;
}

int pcmi_interp_rows_fwd(const float* known, int64_t known_ld, const int32_t* idx, const float* weight, const float* skip,
                         int64_t skip_ld, int64_t B, int64_t m, int64_t n, int C2, int C1, float* out, int64_t out_ld, int validate,
                         pcmi_stream_t stream) {
  const int rc = interp_shape_ok("interp_rows_fwd", B, m, n, C2);
  if (rc != PCMI_OK) return rc;
  PCMI_REQUIRE(C1 >= 0 && known_ld >= C2 && out_ld >= (int64_t)C2 + C1 && (C1 == 0 || skip_ld >= C1) && rows_fit(B * n, out_ld) &&
                   rows_fit(B * m, known_ld) && rows_fit(B * n, skip_ld),
               PCMI_ERR_INVALID, "interp_rows_fwd: bad widths (C2 %d, C1 %d, known_ld %lld, skip_ld %lld, out_ld %lld)", C2, C1,
               (long long)known_ld, (long long)skip_ld, (long long)out_ld);
  const int64_t rows = B * n;
  if (rows == 0) return PCMI_OK;
  PCMI_REQUIRE(idx && weight && out && (known || C2 == 0 || m == 0) && (skip || C1 == 0), PCMI_ERR_INVALID, "interp_rows_fwd: null pointer");
  hipStream_t st = as_stream(stream);
  if (validate) {
    unsigned* flag = stream_counters(st, 1);
    if (!flag) return PCMI_ERR_HIP;
    index_flag_kernel<<<(unsigned)ceil_div(rows * 3, kThreads), kThreads, 0, st>>>(idx, rows * 3, m, flag);
    PCMI_LAUNCH_CHECK();
    unsigned bad = 0;
    PCMI_HIP_CHECK(hipMemcpyAsync(&bad, flag, sizeof(bad), hipMemcpyDeviceToHost, st));
    PCMI_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(bad), st));  // the pool's counters are left at zero
    PCMI_HIP_CHECK(hipStreamSynchronize(st));
    PCMI_REQUIRE(!bad, PCMI_ERR_RANGE, "interp_rows_fwd: an index is outside [0, %lld)", (long long)m);
  }
  const bool vo = aligned16(out) && out_ld % 4 == 0;
  const bool vk = vo && C2 > 0 && C2 % 4 == 0 && known_ld % 4 == 0 && aligned16(known);
  const bool vs = vo && C1 > 0 && C1 % 4 == 0 && C2 % 4 == 0 && skip_ld % 4 == 0 && aligned16(skip);
  const unsigned grid = (unsigned)ceil_div(rows, kWaves);
#define PCMI_INTERP_LAUNCH(VK, VS) \
  interp_rows_fwd_kernel<VK, VS><<<grid, kThreads, 0, st>>>(known, known_ld, idx, weight, skip, skip_ld, rows, m, n, C2, C1, out, out_ld)
  if (vk && vs) PCMI_INTERP_LAUNCH(true, true);
  else if (vk) PCMI_INTERP_LAUNCH(true, false);
  else if (vs) PCMI_INTERP_LAUNCH(false, true);
  else PCMI_INTERP_LAUNCH(false, false);
#undef PCMI_INTERP_LAUNCH
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

size_t pcmi_interp_rows_bwd_workspace_bytes(int64_t B, int64_t m, int64_t n) {
  return inverse_lists_workspace(std::max<int64_t>(B * n * 3, 1), std::max<int64_t>(B * m, 1));
}

int pcmi_interp_rows_bwd(const float* gout, int64_t gout_ld, const int32_t* idx, const float* weight, int64_t B, int64_t m, int64_t n,
                         int C2, float* gknown, int64_t gknown_ld, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  const int rc = interp_shape_ok("interp_rows_bwd", B, m, n, C2);
  if (rc != PCMI_OK) return rc;
  PCMI_REQUIRE(gout_ld >= C2 && gknown_ld >= C2 && rows_fit(B * n, gout_ld) && rows_fit(B * m, gknown_ld), PCMI_ERR_INVALID,
               "interp_rows_bwd: bad widths (C2 %d, gout_ld %lld, gknown_ld %lld)", C2, (long long)gout_ld, (long long)gknown_ld);
  const int64_t targets = B * m, rows = B * n;
  if (targets == 0 || C2 == 0) return PCMI_OK;
  PCMI_REQUIRE(gknown && (rows == 0 || (gout && idx && weight)), PCMI_ERR_INVALID, "interp_rows_bwd: null pointer");
  hipStream_t st = as_stream(stream);
  if (rows == 0) {  // nothing was interpolated: the gradient is zero
    PCMI_HIP_CHECK(hipMemset2DAsync(gknown, (size_t)gknown_ld * 4, 0, (size_t)C2 * 4, (size_t)targets, st));
    return PCMI_OK;
  }
  const int32_t *start = nullptr, *pos = nullptr;
  const int rc2 = inverse_lists("interp_rows_bwd", idx, B, n * 3, m, ws, ws_bytes, &start, &pos, st);
  if (rc2 != PCMI_OK) return rc2;
  const unsigned grid = (unsigned)ceil_div(targets, kWaves);
  if (C2 % 4 == 0 && gout_ld % 4 == 0 && gknown_ld % 4 == 0 && aligned16(gout) && aligned16(gknown))
    interp_rows_bwd_kernel<true><<<grid, kThreads, 0, st>>>(gout, gout_ld, weight, start, pos, targets, C2, gknown, gknown_ld);
  else
    interp_rows_bwd_kernel<false><<<grid, kThreads, 0, st>>>(gout, gout_ld, weight, start, pos, targets, C2, gknown, gknown_ld);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

}  // extern "C"
