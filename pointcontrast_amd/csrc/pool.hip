// Pooling over kernel maps, per-instance (batch index) reductions, global pooling / broadcast and instance norm.
//
// Pooling reuses the conv maps of coords.hip.  Everything is a gather -- the backward passes included -- so no result
// depends on the order in which workgroups run:
//   pool fwd           out[j] = sum_k in[nbr[k][j]]                 (average: / number of present k)
//   pool bwd, stride 1 gin[i] = sum_k gout[nbr[mirror[k]][i]] * s    (s = 1, or 1 / count of that output row)
//   pool bwd, stride 2 gin[pair_in[p]] = gout[pair_out[p]] * s       (every fine row has exactly one parent)
//   unpool fwd / bwd   the stride-2 pool bwd / fwd with s = 1
//
// Segment reductions (global pooling, the broadcast gradients, instance norm) follow the partial -> merge shape of
// norm.hip: instance i's rows (pcmi_segments_t, grouped by instance) are cut into chunks of PCMI_SEGMENT_CHUNK rows,
// one workgroup per (chunk, channel tile) writes fp64 partial sums, and a second launch adds the partials of each
// instance in chunk order.  Instances are few and large (the bench batch: ~22 k level-1 rows each), so one workgroup per
// instance would leave most of the device idle.
#include <algorithm>

#include "internal.h"

namespace pcmi {
namespace {

constexpr int kThreads = 256;
constexpr int kChunk = PCMI_SEGMENT_CHUNK;

// ---- V = 4: float4 over channel quads (c % 4 == 0, aligned); V = 1: scalar ----------------------------------------
template <int V>
__device__ inline void load(const float* __restrict__ p, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
    v[0] = *p;
  }
}

template <int V>
__device__ inline void store(float* __restrict__ p, const float (&v)[V]) {
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    *p = v[0];
  }
}

static bool vec4_ok(int c, std::initializer_list<std::pair<const float*, int64_t>> ts) {
  if (c % 4) return false;
  for (const auto& t : ts)
    if (t.first && (((uintptr_t)t.first & 15) || (t.second & 3))) return false;
  return true;
}

struct Sel {
  int8_t k[PCMI_MAX_KERNEL_VOLUME];
};

// out[j] = sum over kk of in[nbr[sel.k[kk]][j]] * (scale ? scale[that row] : 1); average: divided by the count of
// present terms.  One thread per (row, channel group of V).
template <int V>
__global__ __launch_bounds__(kThreads) void gather_pool_kernel(const float* __restrict__ in, int64_t in_ld,
                                                               const int32_t* __restrict__ nbr, int64_t nbr_ld, Sel sel,
                                                               int K, int64_t n_rows, int cv,
                                                               const float* __restrict__ scale, int average,
                                                               float* __restrict__ out, int64_t out_ld) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= n_rows * cv) return;
  const int64_t j = e / cv;
  const int c0 = (int)(e - j * cv) * V;
  float acc[V];
#pragma unroll
  for (int v = 0; v < V; ++v) acc[v] = 0.f;
  int cnt = 0;
  constexpr int U = 9;  // neighbour indices, then their rows, of 9 offsets at a time in flight; added in offset order
  for (int k0 = 0; k0 < K; k0 += U) {
    int32_t idx[U];
#pragma unroll
    for (int u = 0; u < U; ++u) idx[u] = k0 + u < K ? nbr[(int64_t)sel.k[k0 + u] * nbr_ld + j] : -1;
    float x[U][V], sc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (idx[u] < 0) continue;
      load<V>(in + (int64_t)idx[u] * in_ld + c0, x[u]);
      sc[u] = scale ? scale[idx[u]] : 1.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (idx[u] < 0) continue;
      ++cnt;
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] += scale ? x[u][v] * sc[u] : x[u][v];
    }
  }
  if (average && cnt > 0) {
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] /= (float)cnt;
  }
  store<V>(out + j * out_ld + c0, acc);
}

// out[dst[p]] = in[src[p]] * (scale ? scale[src[p]] : 1) for the M pairs of a stride-2 map (dst rows distinct)
template <int V>
__global__ __launch_bounds__(kThreads) void pair_copy_kernel(const float* __restrict__ in, int64_t in_ld,
                                                             const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                                             int64_t M, int cv, const float* __restrict__ scale,
                                                             float* __restrict__ out, int64_t out_ld) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= M * cv) return;
  const int64_t p = e / cv;
  const int c0 = (int)(e - p * cv) * V;
  const int32_t i = src[p];
  float x[V];
  load<V>(in + (int64_t)i * in_ld + c0, x);
  if (scale) {
    const float s = scale[i];
#pragma unroll
    for (int v = 0; v < V; ++v) x[v] *= s;
  }
  store<V>(out + (int64_t)dst[p] * out_ld + c0, x);
}

// inv[j] = 1 / (number of present neighbours of output row j)
__global__ __launch_bounds__(kThreads) void inv_count_kernel(const int32_t* __restrict__ nbr, int K, int64_t n_out,
                                                             float* __restrict__ inv) {
  const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j >= n_out) return;
  int cnt = 0;
  for (int k = 0; k < K; ++k) cnt += nbr[(int64_t)k * n_out + j] >= 0 ? 1 : 0;
  inv[j] = cnt > 0 ? 1.f / (float)cnt : 0.f;
}

static int launch_gather(const float* in, int64_t in_ld, const pcmi_kmap_t* m, const Sel& sel, int64_t n_rows, int c,
                         const float* scale, int average, float* out, int64_t out_ld, hipStream_t st) {
  if (n_rows == 0) return PCMI_OK;
  if (vec4_ok(c, {{in, in_ld}, {out, out_ld}})) {
    const int cv = c / 4;
    gather_pool_kernel<4><<<dim3((unsigned)ceil_div(n_rows * cv, kThreads)), kThreads, 0, st>>>(
        in, in_ld, m->nbr, m->n_out, sel, m->K, n_rows, cv, scale, average, out, out_ld);
  } else {
    gather_pool_kernel<1><<<dim3((unsigned)ceil_div(n_rows * c, kThreads)), kThreads, 0, st>>>(
        in, in_ld, m->nbr, m->n_out, sel, m->K, n_rows, c, scale, average, out, out_ld);
  }
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

static int launch_pair_copy(const float* in, int64_t in_ld, const int32_t* src, const int32_t* dst, int64_t M, int c,
                            const float* scale, float* out, int64_t out_ld, hipStream_t st) {
  if (M == 0) return PCMI_OK;
  if (vec4_ok(c, {{in, in_ld}, {out, out_ld}})) {
    const int cv = c / 4;
    pair_copy_kernel<4><<<dim3((unsigned)ceil_div(M * cv, kThreads)), kThreads, 0, st>>>(in, in_ld, src, dst, M, cv, scale,
                                                                                         out, out_ld);
  } else {
    pair_copy_kernel<1><<<dim3((unsigned)ceil_div(M * c, kThreads)), kThreads, 0, st>>>(in, in_ld, src, dst, M, c, scale,
                                                                                         out, out_ld);
  }
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

static int check_map(const pcmi_kmap_t* m, int c, const char* who) {
  PCMI_REQUIRE(m && m->nbr && c >= 1, PCMI_ERR_INVALID, "%s: bad argument", who);
  PCMI_REQUIRE((m->kernel_size == 3 && m->stride == 1 && m->n_in == m->n_out) || (m->kernel_size == 2 && m->stride == 2),
               PCMI_ERR_UNSUPPORTED, "%s: only (k=3, s=1) and (k=2, s=2) maps are supported", who);
  PCMI_REQUIRE(m->M >= 0, PCMI_ERR_INVALID, "%s: the map's pair counts are not on the host (take it from pcmi_kmap_get)", who);
  PCMI_REQUIRE(m->stride == 1 || m->M == m->n_in, PCMI_ERR_INVALID, "%s: a stride-2 map must give every fine row one parent",
               who);
  PCMI_REQUIRE(m->n_in < (1ll << 31) && m->n_out < (1ll << 31), PCMI_ERR_RANGE, "%s: too many rows", who);
  return PCMI_OK;
}

static Sel identity_sel(int K) {
  Sel s;
  for (int k = 0; k < K; ++k) s.k[k] = (int8_t)k;
  return s;
}

// =====================================================================================================================
// segment reductions
// =====================================================================================================================
struct Seg {
  const int32_t* rows;
  const int32_t* offs;
  const int32_t* inst;
  const int32_t* chunk_offs;
  int n_inst;
};

static Seg seg_of(const pcmi_segments_t* s) { return Seg{s->rows, s->offs, s->inst, s->chunk_offs, (int)s->n_inst}; }

// the instance of chunk `ch`: the largest i with chunk_offs[i] <= ch (every instance has at least one chunk)
__device__ inline int chunk_instance(const Seg& s, int ch) {
  int lo = 0, hi = s.n_inst - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (s.chunk_offs[mid] <= ch) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

enum PartialMode { kSum = 0, kProd = 1, kCentredSq = 2, kNormBwd = 3 };

struct PartialArgs {
  const float* a;  // x (kSum, kProd, kCentredSq) or dy (kNormBwd)
  int64_t a_ld;
  const float* b;  // kProd: the second factor; kNormBwd: x
  int64_t b_ld;
  const float* y;  // kNormBwd: nullable ReLU mask source
  int64_t y_ld;
  const double* dmean;  // kCentredSq: [n_inst, c]
  const float* mean;    // kNormBwd: [n_inst, c]
  const float* invstd;  // kNormBwd
  int c;
  double* part;  // [n_chunks][NV][c]
};

// One workgroup per (chunk, tile of up to 256 channel groups of V).  A tile narrower than the workgroup packs several
// rows into one pass (C = 96, V = 4: 24 lanes per row, 10 rows per pass), and every lane keeps 4 rows' loads in flight;
// the per-lane sums (ascending rows) are then added over the row slots in a fixed order.
template <int MODE, int V>
__global__ __launch_bounds__(kThreads) void seg_partial_kernel(Seg s, PartialArgs a) {
  constexpr int NV = MODE == kNormBwd ? 2 : 1;
  constexpr int U = 4;
  __shared__ double sh[NV][kThreads * V];
  const int ch = blockIdx.x;
  const int cq = a.c / V;                      // channel groups of the tensor
  const int qt = min(cq, kThreads);            // channel groups per tile
  const int rpp = kThreads / qt;               // rows per pass
  const int ql = threadIdx.x % qt, ro = threadIdx.x / qt;
  const int q = blockIdx.y * qt + ql;
  const int c0 = q * V;
  const bool active = ro < rpp && q < cq;
  const int i = chunk_instance(s, ch);
  const int p0 = s.offs[i] + (ch - s.chunk_offs[i]) * kChunk;
  const int p1 = min(p0 + kChunk, s.offs[i + 1]);
  double acc[NV][V];
#pragma unroll
  for (int v = 0; v < NV; ++v)
#pragma unroll
    for (int e = 0; e < V; ++e) acc[v][e] = 0.0;
  if (active) {
    double m[V], is[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      m[e] = MODE == kCentredSq ? a.dmean[(int64_t)i * a.c + c0 + e] : MODE == kNormBwd ? (double)a.mean[(int64_t)i * a.c + c0 + e] : 0.0;
      is[e] = MODE == kNormBwd ? (double)a.invstd[(int64_t)i * a.c + c0 + e] : 0.0;
    }
    for (int p = p0 + ro; p < p1; p += U * rpp) {
      int64_t r[U];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        ok[u] = p + u * rpp < p1;
        r[u] = s.rows[ok[u] ? p + u * rpp : p];
      }
      float xa[U][V], xb[U][V], xy[U][V];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        load<V>(a.a + r[u] * a.a_ld + c0, xa[u]);
        if (MODE == kProd || MODE == kNormBwd) load<V>(a.b + r[u] * a.b_ld + c0, xb[u]);
        if (MODE == kNormBwd && a.y) load<V>(a.y + r[u] * a.y_ld + c0, xy[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (!ok[u]) continue;
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const float x = xa[u][e];
          if (MODE == kSum) {
            acc[0][e] += (double)x;
          } else if (MODE == kProd) {
            acc[0][e] += (double)x * (double)xb[u][e];
          } else if (MODE == kCentredSq) {
            const double d = (double)x - m[e];
            acc[0][e] += d * d;
          } else {
            const float g = (a.y && !(xy[u][e] > 0.f)) ? 0.f : x;
            acc[0][e] += (double)g;
            acc[NV - 1][e] += (double)g * (((double)xb[u][e] - m[e]) * is[e]);
          }
        }
      }
    }
  }
  if (ro < rpp) {
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int e = 0; e < V; ++e) sh[v][(ro * qt + ql) * V + e] = acc[v][e];
  }
  __syncthreads();
  for (int t = threadIdx.x; t < qt * V; t += kThreads) {
    const int c = blockIdx.y * qt * V + t;
    if (c >= a.c) continue;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      double sum = sh[v][t];
      for (int g = 1; g < rpp; ++g) sum += sh[v][g * qt * V + t];
      a.part[((int64_t)ch * NV + v) * a.c + c] = sum;
    }
  }
}

enum MergeMode { kMergeSum = 0, kMergeMean = 1, kMergeInvstd = 2, kMergeTwo = 3 };

struct MergeArgs {
  const double* part;
  int nv;
  int c;
  int mode;
  int average;       // kMergeSum
  float* out;        // kMergeSum: [n_inst, out_ld]; kMergeMean / kMergeInvstd: float copy [n_inst, c]
  int64_t out_ld;
  double* dout;      // kMergeMean / kMergeInvstd / kMergeTwo (2 planes [n_inst, c]): fp64 result
  float eps;
};

// one thread per (instance, channel): the instance's chunk partials in chunk order
__global__ __launch_bounds__(kThreads) void seg_merge_kernel(Seg s, MergeArgs a) {
  const int i = blockIdx.x;
  const int c = blockIdx.y * kThreads + threadIdx.x;
  if (c >= a.c) return;
  double t0 = 0.0, t1 = 0.0;
  const int k1 = s.chunk_offs[i + 1];
  for (int k = s.chunk_offs[i]; k < k1; k += 4) {  // the loads of 4 chunks in flight, added in chunk order
    double v0[4], v1[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int kk = min(k + u, k1 - 1);
      v0[u] = a.part[((int64_t)kk * a.nv) * a.c + c];
      v1[u] = a.nv == 2 ? a.part[((int64_t)kk * a.nv + 1) * a.c + c] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (k + u < k1) t0 += v0[u], t1 += v1[u];
  }
  const double n = (double)(s.offs[i + 1] - s.offs[i]);
  const int64_t o = (int64_t)i * a.c + c;
  if (a.mode == kMergeSum) {
    a.out[(int64_t)i * a.out_ld + c] = (float)(a.average ? t0 / n : t0);
  } else if (a.mode == kMergeMean) {
    a.dout[o] = t0 / n;
    a.out[o] = (float)(t0 / n);
  } else if (a.mode == kMergeInvstd) {
    const double is = 1.0 / sqrt(t0 / n + (double)a.eps);
    a.dout[o] = is;
    a.out[o] = (float)is;
  } else {
    a.dout[o] = t0;
    a.dout[(int64_t)s.n_inst * a.c + o] = t1;
  }
}

template <int V>
static void launch_partial(int mode, dim3 grid, const Seg& s, const PartialArgs& pa, hipStream_t st) {
  switch (mode) {
    case kSum: seg_partial_kernel<kSum, V><<<grid, kThreads, 0, st>>>(s, pa); break;
    case kProd: seg_partial_kernel<kProd, V><<<grid, kThreads, 0, st>>>(s, pa); break;
    case kCentredSq: seg_partial_kernel<kCentredSq, V><<<grid, kThreads, 0, st>>>(s, pa); break;
    default: seg_partial_kernel<kNormBwd, V><<<grid, kThreads, 0, st>>>(s, pa); break;
  }
}

static int seg_reduce(const pcmi_segments_t* seg, int mode, const PartialArgs& pa, hipStream_t st) {
  const bool b_used = mode == kProd || mode == kNormBwd;
  const bool v4 = vec4_ok(pa.c, {{pa.a, pa.a_ld}, {b_used ? pa.b : nullptr, pa.b_ld}, {mode == kNormBwd ? pa.y : nullptr, pa.y_ld}});
  const int V = v4 ? 4 : 1;
  const dim3 grid((unsigned)seg->n_chunks, (unsigned)ceil_div(pa.c / V, kThreads));
  if (v4) launch_partial<4>(mode, grid, seg_of(seg), pa, st);
  else launch_partial<1>(mode, grid, seg_of(seg), pa, st);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

static int seg_merge(const pcmi_segments_t* seg, const MergeArgs& ma, hipStream_t st) {
  seg_merge_kernel<<<dim3((unsigned)seg->n_inst, (unsigned)ceil_div(ma.c, kThreads)), kThreads, 0, st>>>(seg_of(seg), ma);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

// ---- elementwise passes over the rows, with the row's instance ---------------------------------------------------
enum BcastOp { kBcastAdd = 0, kBcastMul = 1, kBcastCopy = 2 };

// out[r] = x[r] op g[inst(r)] (kBcastCopy: g[inst(r)], divided by the instance's rows when `average`)
template <int V>
__global__ __launch_bounds__(kThreads) void bcast_kernel(Seg s, int op, int average, const float* __restrict__ x,
                                                         int64_t x_ld, const float* __restrict__ g, int64_t g_ld,
                                                         int64_t n, int cv, float* __restrict__ out, int64_t out_ld) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= n * cv) return;
  const int64_t r = e / cv;
  const int c0 = (int)(e - r * cv) * V;
  const int i = s.inst[r];
  float gv[V], xv[V];
  load<V>(g + (int64_t)i * g_ld + c0, gv);
  if (op == kBcastCopy) {
    if (average) {
      const float cnt = (float)(s.offs[i + 1] - s.offs[i]);
#pragma unroll
      for (int v = 0; v < V; ++v) gv[v] /= cnt;
    }
    store<V>(out + r * out_ld + c0, gv);
    return;
  }
  load<V>(x + r * x_ld + c0, xv);
#pragma unroll
  for (int v = 0; v < V; ++v) xv[v] = op == kBcastAdd ? xv[v] + gv[v] : xv[v] * gv[v];
  store<V>(out + r * out_ld + c0, xv);
}

static int launch_bcast(const pcmi_segments_t* seg, int op, int average, const float* x, int64_t x_ld, const float* g,
                        int64_t g_ld, int c, float* out, int64_t out_ld, hipStream_t st) {
  const int64_t n = seg->n;
  if (n == 0) return PCMI_OK;
  if (vec4_ok(c, {{x, x_ld}, {g, g_ld}, {out, out_ld}})) {
    const int cv = c / 4;
    bcast_kernel<4><<<dim3((unsigned)ceil_div(n * cv, kThreads)), kThreads, 0, st>>>(seg_of(seg), op, average, x, x_ld, g,
                                                                                     g_ld, n, cv, out, out_ld);
  } else {
    bcast_kernel<1><<<dim3((unsigned)ceil_div(n * c, kThreads)), kThreads, 0, st>>>(seg_of(seg), op, average, x, x_ld, g,
                                                                                    g_ld, n, c, out, out_ld);
  }
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

// instance norm forward epilogue: y = relu?((x - mean) * invstd * w + b (+ res)), statistics in fp64
template <int V>
__global__ __launch_bounds__(kThreads) void in_apply_kernel(Seg s, const float* __restrict__ x, int64_t x_ld, int64_t n,
                                                            int c, int cv, const double* __restrict__ mean,
                                                            const double* __restrict__ invstd, const float* __restrict__ w,
                                                            const float* __restrict__ b, const float* __restrict__ res,
                                                            int64_t res_ld, int relu, float* __restrict__ y, int64_t y_ld) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= n * cv) return;
  const int64_t r = e / cv;
  const int c0 = (int)(e - r * cv) * V;
  const int64_t o = (int64_t)s.inst[r] * c + c0;
  float xv[V], rv[V];
  load<V>(x + r * x_ld + c0, xv);
  if (res) load<V>(res + r * res_ld + c0, rv);
#pragma unroll
  for (int v = 0; v < V; ++v) {
    float t = (float)(((double)xv[v] - mean[o + v]) * invstd[o + v]) * w[c0 + v] + b[c0 + v];
    if (res) t += rv[v];
    xv[v] = relu ? fmaxf(t, 0.f) : t;
  }
  store<V>(y + r * y_ld + c0, xv);
}

// instance norm backward: g = dy * [y > 0]; dres = g; dx = w * invstd * (g - S0 / n_i - xhat * S1 / n_i)
template <int V>
__global__ __launch_bounds__(kThreads) void in_bwd_apply_kernel(Seg s, const float* __restrict__ dy, int64_t dy_ld,
                                                                const float* __restrict__ x, int64_t x_ld,
                                                                const float* __restrict__ ym, int64_t y_ld, int64_t n, int c,
                                                                int cv, const float* __restrict__ mean,
                                                                const float* __restrict__ invstd, const double* __restrict__ sums,
                                                                int n_inst, const float* __restrict__ w, float* __restrict__ dx,
                                                                int64_t dx_ld, float* __restrict__ dres, int64_t dres_ld) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= n * cv) return;
  const int64_t r = e / cv;
  const int c0 = (int)(e - r * cv) * V;
  const int i = s.inst[r];
  const int64_t o = (int64_t)i * c + c0;
  const double inv_n = 1.0 / (double)(s.offs[i + 1] - s.offs[i]);
  float gv[V], xv[V], yv[V];
  load<V>(dy + r * dy_ld + c0, gv);
  load<V>(x + r * x_ld + c0, xv);
  if (ym) load<V>(ym + r * y_ld + c0, yv);
#pragma unroll
  for (int v = 0; v < V; ++v) {
    if (ym && !(yv[v] > 0.f)) gv[v] = 0.f;
    const double is = invstd[o + v];
    const double xhat = ((double)xv[v] - (double)mean[o + v]) * is;
    const double t = (double)gv[v] - sums[o + v] * inv_n - xhat * sums[(int64_t)n_inst * c + o + v] * inv_n;
    xv[v] = (float)((double)w[c0 + v] * is * t);
  }
  store<V>(dx + r * dx_ld + c0, xv);
  if (dres) store<V>(dres + r * dres_ld + c0, gv);
}

// dweight[c] = sum_i S1[i][c], dbias[c] = sum_i S0[i][c], instances in order
__global__ __launch_bounds__(kThreads) void in_param_kernel(const double* __restrict__ sums, int n_inst, int c,
                                                            float* __restrict__ dw, float* __restrict__ db) {
  const int ch = blockIdx.x * kThreads + threadIdx.x;
  if (ch >= c) return;
  double s0 = 0.0, s1 = 0.0;
  for (int i = 0; i < n_inst; ++i) {
    s0 += sums[(int64_t)i * c + ch];
    s1 += sums[(int64_t)(n_inst + i) * c + ch];
  }
  if (db) db[ch] = (float)s0;
  if (dw) dw[ch] = (float)s1;
}

static int check_seg(const pcmi_segments_t* seg, int c, const char* who) {
  PCMI_REQUIRE(seg && c >= 1 && seg->n >= 0 && seg->n_inst >= 0 && (seg->n == 0 || (seg->rows && seg->inst && seg->offs &&
                                                                                       seg->chunk_offs)),
               PCMI_ERR_INVALID, "%s: bad argument", who);
  PCMI_REQUIRE(seg->n * (int64_t)c < (1ll << 40) && seg->n_chunks < (1ll << 31), PCMI_ERR_RANGE, "%s: too many rows", who);
  return PCMI_OK;
}

struct SegWs {
  double* part;   // [n_chunks][2][c]
  double* stats;  // [3][n_inst][c]: mean, invstd (forward) / S0, S1 (backward)
};

static size_t seg_ws_bytes(const pcmi_segments_t* seg, int c) {
  return align_up(sizeof(double) * (size_t)std::max<int64_t>(seg->n_chunks, 1) * 2 * c, 256) +
         align_up(sizeof(double) * (size_t)std::max<int64_t>(seg->n_inst, 1) * 3 * c, 256);
}

static SegWs seg_ws(void* ws, const pcmi_segments_t* seg, int c) {
  SegWs w;
  w.part = (double*)ws;
  w.stats = (double*)((char*)ws + align_up(sizeof(double) * (size_t)std::max<int64_t>(seg->n_chunks, 1) * 2 * c, 256));
  return w;
}

}  // namespace
}  // namespace pcmi

using namespace pcmi;

extern "C" {

size_t pcmi_pool_workspace_bytes(int64_t n_out) { return align_up(sizeof(float) * (size_t)std::max<int64_t>(n_out, 1), 256); }

int pcmi_pool_fwd(const float* in, int64_t in_ld, int c, const pcmi_kmap_t* map, int average, float* out, int64_t out_ld,
                  pcmi_stream_t stream) {
  int rc = check_map(map, c, "pool_fwd");
  if (rc) return rc;
  PCMI_REQUIRE((in || map->n_in == 0) && (out || map->n_out == 0) && in_ld >= c && out_ld >= c, PCMI_ERR_INVALID,
               "pool_fwd: bad tensor");
  return launch_gather(in, in_ld, map, identity_sel(map->K), map->n_out, c, nullptr, average, out, out_ld,
                       as_stream(stream));
}

int pcmi_pool_bwd(const float* gout, int64_t gout_ld, int c, const pcmi_kmap_t* map, int average, float* gin,
                  int64_t gin_ld, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  int rc = check_map(map, c, "pool_bwd");
  if (rc) return rc;
  PCMI_REQUIRE((gout || map->n_out == 0) && (gin || map->n_in == 0) && gout_ld >= c && gin_ld >= c, PCMI_ERR_INVALID,
               "pool_bwd: bad tensor");
  hipStream_t st = as_stream(stream);
  float* inv = nullptr;
  if (average && map->n_out > 0) {
    PCMI_REQUIRE(ws && ws_bytes >= pcmi_pool_workspace_bytes(map->n_out), PCMI_ERR_WORKSPACE, "pool_bwd: workspace too small");
    inv = (float*)ws;
    inv_count_kernel<<<dim3((unsigned)ceil_div(map->n_out, kThreads)), kThreads, 0, st>>>(map->nbr, map->K, map->n_out, inv);
    PCMI_LAUNCH_CHECK();
  }
  if (map->stride == 1) {  // the adjoint of offset k is the mirrored offset on the same key
    Sel sel;
    for (int k = 0; k < map->K; ++k) sel.k[k] = (int8_t)map->mirror[k];
    return launch_gather(gout, gout_ld, map, sel, map->n_in, c, inv, 0, gin, gin_ld, st);
  }
  return launch_pair_copy(gout, gout_ld, map->pair_out, map->pair_in, map->M, c, inv, gin, gin_ld, st);
}

int pcmi_unpool_fwd(const float* in, int64_t in_ld, int c, const pcmi_kmap_t* map, float* out, int64_t out_ld,
                    pcmi_stream_t stream) {
  int rc = check_map(map, c, "unpool_fwd");
  if (rc) return rc;
  PCMI_REQUIRE(map->stride == 2, PCMI_ERR_UNSUPPORTED, "unpool_fwd: only the (k=2, s=2) map of a strided key");
  PCMI_REQUIRE((in || map->n_out == 0) && (out || map->n_in == 0) && in_ld >= c && out_ld >= c, PCMI_ERR_INVALID,
               "unpool_fwd: bad tensor");
  return launch_pair_copy(in, in_ld, map->pair_out, map->pair_in, map->M, c, nullptr, out, out_ld, as_stream(stream));
}

int pcmi_unpool_bwd(const float* gout, int64_t gout_ld, int c, const pcmi_kmap_t* map, float* gin, int64_t gin_ld,
                    pcmi_stream_t stream) {
  int rc = check_map(map, c, "unpool_bwd");
  if (rc) return rc;
  PCMI_REQUIRE(map->stride == 2, PCMI_ERR_UNSUPPORTED, "unpool_bwd: only the (k=2, s=2) map of a strided key");
  PCMI_REQUIRE((gout || map->n_in == 0) && (gin || map->n_out == 0) && gout_ld >= c && gin_ld >= c, PCMI_ERR_INVALID,
               "unpool_bwd: bad tensor");
  return launch_gather(gout, gout_ld, map, identity_sel(map->K), map->n_out, c, nullptr, 0, gin, gin_ld, as_stream(stream));
}

size_t pcmi_segments_workspace_bytes(const pcmi_segments_t* seg, int c) {
  return seg && c > 0 ? seg_ws_bytes(seg, c) : 0;
}

int pcmi_global_pool_fwd(const float* x, int64_t x_ld, int c, const pcmi_segments_t* seg, int average, float* out,
                         int64_t out_ld, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  int rc = check_seg(seg, c, "global_pool_fwd");
  if (rc) return rc;
  PCMI_REQUIRE((x || seg->n == 0) && (out || seg->n_inst == 0) && x_ld >= c && out_ld >= c, PCMI_ERR_INVALID,
               "global_pool_fwd: bad tensor");
  if (seg->n_inst == 0) return PCMI_OK;
  PCMI_REQUIRE(ws && ws_bytes >= seg_ws_bytes(seg, c), PCMI_ERR_WORKSPACE, "global_pool_fwd: workspace too small");
  hipStream_t st = as_stream(stream);
  const SegWs w = seg_ws(ws, seg, c);
  PartialArgs pa{};
  pa.a = x, pa.a_ld = x_ld, pa.c = c, pa.part = w.part;
  rc = seg_reduce(seg, kSum, pa, st);
  if (rc) return rc;
  MergeArgs ma{};
  ma.part = w.part, ma.nv = 1, ma.c = c, ma.mode = kMergeSum, ma.average = average, ma.out = out, ma.out_ld = out_ld;
  return seg_merge(seg, ma, st);
}

int pcmi_global_pool_bwd(const float* gout, int64_t gout_ld, int c, const pcmi_segments_t* seg, int average, float* gin,
                         int64_t gin_ld, pcmi_stream_t stream) {
  int rc = check_seg(seg, c, "global_pool_bwd");
  if (rc) return rc;
  PCMI_REQUIRE((gout || seg->n_inst == 0) && (gin || seg->n == 0) && gout_ld >= c && gin_ld >= c, PCMI_ERR_INVALID,
               "global_pool_bwd: bad tensor");
  return launch_bcast(seg, kBcastCopy, average, nullptr, 0, gout, gout_ld, c, gin, gin_ld, as_stream(stream));
}

int pcmi_broadcast_fwd(const float* x, int64_t x_ld, const float* g, int64_t g_ld, int c, const pcmi_segments_t* seg, int op,
                       float* out, int64_t out_ld, pcmi_stream_t stream) {
  int rc = check_seg(seg, c, "broadcast_fwd");
  if (rc) return rc;
  PCMI_REQUIRE(op == 0 || op == 1, PCMI_ERR_INVALID, "broadcast_fwd: op %d (0: add, 1: multiply)", op);
  PCMI_REQUIRE((x || seg->n == 0) && (g || seg->n_inst == 0) && (out || seg->n == 0) && x_ld >= c && g_ld >= c && out_ld >= c,
               PCMI_ERR_INVALID, "broadcast_fwd: bad tensor");
  return launch_bcast(seg, op == 0 ? kBcastAdd : kBcastMul, 0, x, x_ld, g, g_ld, c, out, out_ld, as_stream(stream));
}

int pcmi_broadcast_bwd(const float* gout, int64_t gout_ld, const float* x, int64_t x_ld, const float* g, int64_t g_ld, int c,
                       const pcmi_segments_t* seg, int op, float* gx, int64_t gx_ld, float* gg, int64_t gg_ld, void* ws,
                       size_t ws_bytes, pcmi_stream_t stream) {
  int rc = check_seg(seg, c, "broadcast_bwd");
  if (rc) return rc;
  PCMI_REQUIRE(op == 0 || op == 1, PCMI_ERR_INVALID, "broadcast_bwd: op %d (0: add, 1: multiply)", op);
  PCMI_REQUIRE((gout || seg->n == 0) && gout_ld >= c && (op == 0 || ((x || seg->n == 0) && (g || seg->n_inst == 0))),
               PCMI_ERR_INVALID, "broadcast_bwd: bad tensor");
  hipStream_t st = as_stream(stream);
  if (gx) {
    PCMI_REQUIRE(gx_ld >= c, PCMI_ERR_INVALID, "broadcast_bwd: bad gx");
    if (op == 0) {
      if (seg->n > 0) PCMI_HIP_CHECK(hipMemcpy2DAsync(gx, sizeof(float) * gx_ld, gout, sizeof(float) * gout_ld,
                                                      sizeof(float) * c, seg->n, hipMemcpyDeviceToDevice, st));
    } else {
      rc = launch_bcast(seg, kBcastMul, 0, gout, gout_ld, g, g_ld, c, gx, gx_ld, st);
      if (rc) return rc;
    }
  }
  if (gg && seg->n_inst > 0) {
    PCMI_REQUIRE(gg_ld >= c, PCMI_ERR_INVALID, "broadcast_bwd: bad gg");
    PCMI_REQUIRE(ws && ws_bytes >= seg_ws_bytes(seg, c), PCMI_ERR_WORKSPACE, "broadcast_bwd: workspace too small");
    const SegWs w = seg_ws(ws, seg, c);
    PartialArgs pa{};
    pa.a = gout, pa.a_ld = gout_ld, pa.b = x, pa.b_ld = x_ld, pa.c = c, pa.part = w.part;
    rc = seg_reduce(seg, op == 0 ? kSum : kProd, pa, st);
    if (rc) return rc;
    MergeArgs ma{};
    ma.part = w.part, ma.nv = 1, ma.c = c, ma.mode = kMergeSum, ma.out = gg, ma.out_ld = gg_ld;
    rc = seg_merge(seg, ma, st);
    if (rc) return rc;
  }
  return PCMI_OK;
}

int pcmi_instnorm_fwd(const float* x, int64_t x_ld, int c, const pcmi_segments_t* seg, const float* weight, const float* bias,
                      float eps, const float* residual, int64_t res_ld, int relu, float* y, int64_t y_ld, float* save_mean,
                      float* save_invstd, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  int rc = check_seg(seg, c, "instnorm_fwd");
  if (rc) return rc;
  PCMI_REQUIRE((x || seg->n == 0) && (y || seg->n == 0) && weight && bias && save_mean && save_invstd && x_ld >= c &&
                   y_ld >= c && (!residual || res_ld >= c) && eps >= 0.f,
               PCMI_ERR_INVALID, "instnorm_fwd: bad argument");
  if (seg->n == 0) return PCMI_OK;
  PCMI_REQUIRE(ws && ws_bytes >= seg_ws_bytes(seg, c), PCMI_ERR_WORKSPACE, "instnorm_fwd: workspace too small");
  hipStream_t st = as_stream(stream);
  const SegWs w = seg_ws(ws, seg, c);
  double* dmean = w.stats;
  double* dinv = w.stats + seg->n_inst * c;
  PartialArgs pa{};
  pa.a = x, pa.a_ld = x_ld, pa.c = c, pa.part = w.part;
  MergeArgs ma{};
  ma.part = w.part, ma.nv = 1, ma.c = c, ma.eps = eps;
  // mean, then the centred second moment (not E[x^2] - E[x]^2)
  rc = seg_reduce(seg, kSum, pa, st);
  if (rc) return rc;
  ma.mode = kMergeMean, ma.out = save_mean, ma.dout = dmean;
  rc = seg_merge(seg, ma, st);
  if (rc) return rc;
  pa.dmean = dmean;
  rc = seg_reduce(seg, kCentredSq, pa, st);
  if (rc) return rc;
  ma.mode = kMergeInvstd, ma.out = save_invstd, ma.dout = dinv;
  rc = seg_merge(seg, ma, st);
  if (rc) return rc;
  const int64_t n = seg->n;
  if (vec4_ok(c, {{x, x_ld}, {y, y_ld}, {residual, res_ld}})) {
    const int cv = c / 4;
    in_apply_kernel<4><<<dim3((unsigned)ceil_div(n * cv, kThreads)), kThreads, 0, st>>>(
        seg_of(seg), x, x_ld, n, c, cv, dmean, dinv, weight, bias, residual, res_ld, relu, y, y_ld);
  } else {
    in_apply_kernel<1><<<dim3((unsigned)ceil_div(n * c, kThreads)), kThreads, 0, st>>>(
        seg_of(seg), x, x_ld, n, c, c, dmean, dinv, weight, bias, residual, res_ld, relu, y, y_ld);
  }
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

int pcmi_instnorm_bwd(const float* dy, int64_t dy_ld, const float* x, int64_t x_ld, const float* relu_mask_y, int64_t y_ld,
                      int c, const pcmi_segments_t* seg, const float* weight, const float* save_mean,
                      const float* save_invstd, float* dx, int64_t dx_ld, float* dres, int64_t dres_ld, float* dweight,
                      float* dbias, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  int rc = check_seg(seg, c, "instnorm_bwd");
  if (rc) return rc;
  PCMI_REQUIRE((dy || seg->n == 0) && (x || seg->n == 0) && (dx || seg->n == 0) && weight && save_mean && save_invstd &&
                   dy_ld >= c && x_ld >= c && dx_ld >= c && (!relu_mask_y || y_ld >= c) && (!dres || dres_ld >= c),
               PCMI_ERR_INVALID, "instnorm_bwd: bad argument");
  hipStream_t st = as_stream(stream);
  if (seg->n == 0) {
    if (dweight) PCMI_HIP_CHECK(hipMemsetAsync(dweight, 0, sizeof(float) * c, st));
    if (dbias) PCMI_HIP_CHECK(hipMemsetAsync(dbias, 0, sizeof(float) * c, st));
    return PCMI_OK;
  }
  PCMI_REQUIRE(ws && ws_bytes >= seg_ws_bytes(seg, c), PCMI_ERR_WORKSPACE, "instnorm_bwd: workspace too small");
  const SegWs w = seg_ws(ws, seg, c);
  PartialArgs pa{};
  pa.a = dy, pa.a_ld = dy_ld, pa.b = x, pa.b_ld = x_ld, pa.y = relu_mask_y, pa.y_ld = y_ld, pa.mean = save_mean;
  pa.invstd = save_invstd, pa.c = c, pa.part = w.part;
  rc = seg_reduce(seg, kNormBwd, pa, st);
  if (rc) return rc;
  MergeArgs ma{};
  ma.part = w.part, ma.nv = 2, ma.c = c, ma.mode = kMergeTwo, ma.dout = w.stats;
  rc = seg_merge(seg, ma, st);
  if (rc) return rc;
  if (dweight || dbias) {
    in_param_kernel<<<dim3((unsigned)ceil_div(c, kThreads)), kThreads, 0, st>>>(w.stats, (int)seg->n_inst, c, dweight, dbias);
    PCMI_LAUNCH_CHECK();
  }
  const int64_t n = seg->n;
  if (vec4_ok(c, {{dy, dy_ld}, {x, x_ld}, {relu_mask_y, y_ld}, {dx, dx_ld}, {dres, dres_ld}})) {
    const int cv = c / 4;
    in_bwd_apply_kernel<4><<<dim3((unsigned)ceil_div(n * cv, kThreads)), kThreads, 0, st>>>(
        seg_of(seg), dy, dy_ld, x, x_ld, relu_mask_y, y_ld, n, c, cv, save_mean, save_invstd, w.stats, (int)seg->n_inst,
        weight, dx, dx_ld, dres, dres_ld);
  } else {
    in_bwd_apply_kernel<1><<<dim3((unsigned)ceil_div(n * c, kThreads)), kThreads, 0, st>>>(
        seg_of(seg), dy, dy_ld, x, x_ld, relu_mask_y, y_ld, n, c, c, save_mean, save_invstd, w.stats, (int)seg->n_inst,
        weight, dx, dx_ld, dres, dres_ld);
  }
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

}  // extern "C"
