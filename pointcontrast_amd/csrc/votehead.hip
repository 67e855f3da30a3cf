// The VoteNet head on row-major activations (downstream/votenet_det_new of the reference: models/voting_module.py,
// models/proposal_module.py through pointnet2_modules.PointnetSAModuleVotes, models/votenet.py:120-121, lib/train.py's Adam).
// Written from the semantics in include/pcmi.h; gfx950, wave64, fp32 data, int32 indices.
//
// Every head activation is fp32 [rows, ld]: feature columns first (so that a row copy is 16-byte aligned), geometric
// columns behind them, zero columns up to ld.  One wave owns one row wherever a row is copied or reduced: lane l takes the
// columns 4 l .. 4 l + 3 (+ 256 j) as one 16-byte access when the feature width is a multiple of 4 and the operands are
// 16-byte aligned, else column l (+ 64 j) as a 4-byte access.  No float atomics: the scatter-adds of the grouping's backward
// run in gather form over the inverse lists of pointset.hip, every target summed in ascending source row; the row norms are
// reduced per lane in ascending column and then by a fixed xor butterfly.  Contraction is off for the whole file, so each
// operation is rounded on its own and the forward of group_rows is reproducible in numpy float32.
#include <algorithm>
#include <cmath>

#include "internal.h"

#pragma clang fp contract(off)

namespace pcmi {
namespace votehead {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;  // rows per workgroup of the one-wave-per-row kernels

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

__global__ void index_flag_kernel(const int32_t* __restrict__ idx, int64_t count, int64_t n, unsigned* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < count && (idx[i] < 0 || idx[i] >= n)) atomicOr(flag, 1u);
}

// ---- group_rows ---------------------------------------------------------------------------------------------------------
// out[r, 0:C] = feat[b n + idx[r]], out[r, C + k] = (xyz[b, idx[r], k] - centre[b, q, k]) / radius_div, zeros up to out_ld;
// r = (b np + q) ns + s.  An index outside [0, n): the whole row is zero, nothing is read through it.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void group_rows_fwd_kernel(const float* __restrict__ xyz, const float* __restrict__ centre,
                                                                  const float* __restrict__ feat, int64_t feat_ld,
                                                                  const int32_t* __restrict__ idx, int64_t rows, int64_t n, int64_t np,
                                                                  int ns, int C, float radius_div, float* __restrict__ out,
                                                                  int64_t out_ld) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int64_t g = r / ns, b = g / np;
  const int32_t t = idx[r];
  const bool ok = t >= 0 && t < n;
  const int64_t src = b * n + (ok ? t : 0);
  float* o = out + r * out_ld;
  if (VEC) {
    float4* d = reinterpret_cast<float4*>(o);
    for (int c = lane; c < C / 4; c += 64) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ok) v = reinterpret_cast<const float4*>(feat + src * feat_ld)[c];
      d[c] = v;
    }
  } else {
    for (int c = lane; c < C; c += 64) {
      float v = 0.f;
      if (ok) v = feat[src * feat_ld + c];
      o[c] = v;
    }
  }
  for (int64_t c = C + lane; c < out_ld; c += 64) {
    const int k = (int)(c - C);
    float v = 0.f;
    if (ok && k < 3) v = (xyz[src * 3 + k] - centre[g * 3 + k]) / radius_div;
    o[c] = v;
  }
}

// One wave per target point T = b n + t: gfeat[T, :] and gxyz[T, :] = the sum over the rows pos[start[T] .. start[T + 1])
// that gathered it, in ascending row (the lists never hold a row whose index was out of range).
template <bool VEC>
__global__ __launch_bounds__(kThreads) void group_rows_bwd_points_kernel(const float* __restrict__ gout, int64_t gout_ld,
                                                                         const int32_t* __restrict__ start,
                                                                         const int32_t* __restrict__ pos, int64_t targets, int C,
                                                                         float radius_div, float* __restrict__ gfeat, int64_t gfeat_ld,
                                                                         float* __restrict__ gxyz) {
  const int lane = threadIdx.x & 63;
  const int64_t T = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (T >= targets) return;
  const int32_t s = start[T], e = start[T + 1];
  if (VEC) {
    for (int c = lane * 4; c < C; c += 256) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int32_t i = s; i < e; ++i) {
        const float4 v = *reinterpret_cast<const float4*>(gout + (int64_t)pos[i] * gout_ld + c);
        acc.x = acc.x + v.x;
        acc.y = acc.y + v.y;
        acc.z = acc.z + v.z;
        acc.w = acc.w + v.w;
      }
      *reinterpret_cast<float4*>(gfeat + T * gfeat_ld + c) = acc;
    }
  } else {
    for (int c = lane; c < C; c += 64) {
      float acc = 0.f;
      for (int32_t i = s; i < e; ++i) acc = acc + gout[(int64_t)pos[i] * gout_ld + c];
      gfeat[T * gfeat_ld + c] = acc;
    }
  }
  if (lane < 3) {
    float acc = 0.f;
    for (int32_t i = s; i < e; ++i) acc = acc + gout[(int64_t)pos[i] * gout_ld + C + lane] / radius_div;
    gxyz[T * 3 + lane] = acc;
  }
}

// gcentre[g, k] = -(sum over the group's ns rows, ascending, of gout[r, C + k] / radius_div); a row whose index is out of
// range (all zero in the forward pass) does not take part
__global__ void group_rows_bwd_centre_kernel(const float* __restrict__ gout, int64_t gout_ld, const int32_t* __restrict__ idx,
                                             int64_t groups, int64_t n, int ns, int C, float radius_div, float* __restrict__ gcentre) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= groups * 3) return;
  const int64_t g = i / 3;
  const int k = (int)(i - g * 3);
  float acc = 0.f;
  for (int s = 0; s < ns; ++s) {
    const int64_t r = g * ns + s;
    const int32_t t = idx[r];
    if (t >= 0 && t < n) acc = acc + gout[r * gout_ld + C + k] / radius_div;
  }
  gcentre[i] = -acc;
}

// ---- rows_maxpool -------------------------------------------------------------------------------------------------------
// One thread per (output row, V adjacent columns); the ns rows of the window are read in ascending order, strict > keeps
// the lowest row among equals, a NaN takes the result and is never replaced.
template <int V>
__global__ __launch_bounds__(kThreads) void rows_maxpool_fwd_kernel(const float* __restrict__ x, int64_t x_ld, int64_t R, int ns, int C,
                                                                    float* __restrict__ out, int64_t out_ld, uint8_t* __restrict__ arg) {
  const int cg = C / V;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= R * cg) return;
  const int64_t r = i / cg;
  const int c = (int)(i - r * cg) * V;
  const float* p = x + r * ns * x_ld + c;
  float m[V];
  uint8_t a[V];
  if constexpr (V == 4) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    m[0] = v.x; m[1 % V] = v.y; m[2 % V] = v.z; m[3 % V] = v.w;
  } else {
    m[0] = p[0];
  }
#pragma unroll
  for (int j = 0; j < V; ++j) a[j] = 0;
  for (int s = 1; s < ns; ++s) {
    float v[V];
    if constexpr (V == 4) {
      const float4 q = *reinterpret_cast<const float4*>(p + s * x_ld);
      v[0] = q.x; v[1 % V] = q.y; v[2 % V] = q.z; v[3 % V] = q.w;
    } else {
      v[0] = p[s * x_ld];
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (m[j] == m[j] && (v[j] > m[j] || v[j] != v[j])) {
        m[j] = v[j];
        a[j] = (uint8_t)s;
      }
    }
  }
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(out + r * out_ld + c) = make_float4(m[0], m[1 % V], m[2 % V], m[3 % V]);
    *reinterpret_cast<uchar4*>(arg + r * C + c) = make_uchar4(a[0], a[1 % V], a[2 % V], a[3 % V]);
  } else {
    out[r * out_ld + c] = m[0];
    arg[r * C + c] = a[0];
  }
}

// gx[(r ns + s), c] = gout[r, c] where arg[r, c] == s, else 0: every element of gx [R ns, C] is written
template <int V>
__global__ __launch_bounds__(kThreads) void rows_maxpool_bwd_kernel(const float* __restrict__ gout, int64_t gout_ld,
                                                                    const uint8_t* __restrict__ arg, int64_t R, int ns, int C,
                                                                    float* __restrict__ gx, int64_t gx_ld) {
  const int cg = C / V;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= R * ns * cg) return;
  const int64_t row = i / cg;
  const int c = (int)(i - row * cg) * V;
  const int64_t r = row / ns;
  const int s = (int)(row - r * ns);
  if constexpr (V == 4) {
    const float4 g = *reinterpret_cast<const float4*>(gout + r * gout_ld + c);
    const uchar4 a = *reinterpret_cast<const uchar4*>(arg + r * C + c);
    *reinterpret_cast<float4*>(gx + row * gx_ld + c) =
        make_float4(a.x == s ? g.x : 0.f, a.y == s ? g.y : 0.f, a.z == s ? g.z : 0.f, a.w == s ? g.w : 0.f);
  } else {
    gx[row * gx_ld + c] = arg[r * C + c] == s ? gout[r * gout_ld + c] : 0.f;
  }
}

// ---- vote ---------------------------------------------------------------------------------------------------------------
// One wave per vote o = r vf + v: u = seed_feat[r] + net[r, v Wb + 0:C], norm = sqrt(sum u^2) (per lane in ascending column,
// then the butterfly), vote_feat[o] = u / norm (no epsilon: a zero row gives NaN, as the reference does),
// vote_xyz[o] = seed_xyz[r] + net[r, v Wb + C + 0:3].
template <bool VEC>
__global__ __launch_bounds__(kThreads) void vote_fwd_kernel(const float* __restrict__ net, int64_t net_ld, const float* __restrict__ seed_xyz,
                                                            const float* __restrict__ seed_feat, int64_t sf_ld, int64_t votes, int vf,
                                                            int C, int Wb, float* __restrict__ vote_xyz, float* __restrict__ vote_feat,
                                                            int64_t vfeat_ld, float* __restrict__ norm) {
  const int lane = threadIdx.x & 63;
  const int64_t o = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (o >= votes) return;
  const int64_t r = o / vf;
  const int v = (int)(o - r * vf);
  const float* nb = net + r * net_ld + (int64_t)v * Wb;
  const float* sf = seed_feat + r * sf_ld;
  float* y = vote_feat + o * vfeat_ld;
  float acc = 0.f;
  if (VEC) {
    for (int c = lane * 4; c < C; c += 256) {
      const float4 a = *reinterpret_cast<const float4*>(sf + c), d = *reinterpret_cast<const float4*>(nb + c);
      const float u0 = a.x + d.x, u1 = a.y + d.y, u2 = a.z + d.z, u3 = a.w + d.w;
      acc = acc + u0 * u0;
      acc = acc + u1 * u1;
      acc = acc + u2 * u2;
      acc = acc + u3 * u3;
    }
  } else {
    for (int c = lane; c < C; c += 64) {
      const float u = sf[c] + nb[c];
      acc = acc + u * u;
    }
  }
  const float nrm = sqrtf(wave_sum(acc));
  if (VEC) {
    for (int c = lane * 4; c < C; c += 256) {
      const float4 a = *reinterpret_cast<const float4*>(sf + c), d = *reinterpret_cast<const float4*>(nb + c);
      *reinterpret_cast<float4*>(y + c) = make_float4((a.x + d.x) / nrm, (a.y + d.y) / nrm, (a.z + d.z) / nrm, (a.w + d.w) / nrm);
    }
  } else {
    for (int c = lane; c < C; c += 64) y[c] = (sf[c] + nb[c]) / nrm;
  }
  if (lane < 3) vote_xyz[o * 3 + lane] = seed_xyz[r * 3 + lane] + nb[C + lane];
  if (lane == 0) norm[o] = nrm;
}

// One wave per seed r.  Per vote: gu = (gy - y (y . gy)) / norm into g_net[r, v Wb + 0:C], g_vote_xyz into the three
// columns behind, zeros up to Wb.  Then the seed's gradients = the sum over v, ascending: each lane re-reads the g_net
// elements it wrote itself.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void vote_bwd_kernel(const float* __restrict__ gfeat, int64_t gf_ld, const float* __restrict__ gxyz,
                                                            const float* __restrict__ y, int64_t y_ld, const float* __restrict__ norm,
                                                            int64_t R, int vf, int C, int Wb, float* g_net, int64_t gnet_ld,
                                                            float* __restrict__ g_seed_feat, int64_t gsf_ld,
                                                            float* __restrict__ g_seed_xyz) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (r >= R) return;
  float* gn = g_net + r * gnet_ld;
  for (int v = 0; v < vf; ++v) {
    const int64_t o = r * vf + v;
    const float* gy = gfeat + o * gf_ld;
    const float* yy = y + o * y_ld;
    float* d = gn + (int64_t)v * Wb;
    float acc = 0.f;
    if (VEC) {
      for (int c = lane * 4; c < C; c += 256) {
        const float4 a = *reinterpret_cast<const float4*>(yy + c), g = *reinterpret_cast<const float4*>(gy + c);
        acc = acc + a.x * g.x;
        acc = acc + a.y * g.y;
        acc = acc + a.z * g.z;
        acc = acc + a.w * g.w;
      }
    } else {
      for (int c = lane; c < C; c += 64) acc = acc + yy[c] * gy[c];
    }
    const float dot = wave_sum(acc), nrm = norm[o];
    if (VEC) {
      for (int c = lane * 4; c < C; c += 256) {
        const float4 a = *reinterpret_cast<const float4*>(yy + c), g = *reinterpret_cast<const float4*>(gy + c);
        *reinterpret_cast<float4*>(d + c) =
            make_float4((g.x - a.x * dot) / nrm, (g.y - a.y * dot) / nrm, (g.z - a.z * dot) / nrm, (g.w - a.w * dot) / nrm);
      }
    } else {
      for (int c = lane; c < C; c += 64) d[c] = (gy[c] - yy[c] * dot) / nrm;
    }
    for (int c = C + lane; c < Wb; c += 64) d[c] = c - C < 3 ? gxyz[o * 3 + (c - C)] : 0.f;
  }
  float* gs = g_seed_feat + r * gsf_ld;
  if (VEC) {
    for (int c = lane * 4; c < C; c += 256) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int v = 0; v < vf; ++v) {
        const float4 g = *reinterpret_cast<const float4*>(gn + (int64_t)v * Wb + c);
        acc.x = acc.x + g.x;
        acc.y = acc.y + g.y;
        acc.z = acc.z + g.z;
        acc.w = acc.w + g.w;
      }
      *reinterpret_cast<float4*>(gs + c) = acc;
    }
  } else {
    for (int c = lane; c < C; c += 64) {
      float acc = 0.f;
      for (int v = 0; v < vf; ++v) acc = acc + gn[(int64_t)v * Wb + c];
      gs[c] = acc;
    }
  }
  if (lane < 3) {
    float acc = 0.f;
    for (int v = 0; v < vf; ++v) acc = acc + gxyz[(r * vf + v) * 3 + lane];
    g_seed_xyz[r * 3 + lane] = acc;
  }
}

// ---- Adam ---------------------------------------------------------------------------------------------------------------
struct AdamArgs {
  float step_size, beta1, one_minus_beta1, beta2, one_minus_beta2, bc2_sqrt, eps, weight_decay;
};

__device__ __forceinline__ void adam_one(float& w, float g, float& m, float& v, const AdamArgs& a) {
  g = g + a.weight_decay * w;
  m = a.beta1 * m + a.one_minus_beta1 * g;
  v = a.beta2 * v + a.one_minus_beta2 * (g * g);
  const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
  w = w - a.step_size * (m / denom);
}

// items [0, n4): four adjacent elements as 16-byte accesses; items behind them: the n - 4 n4 elements of the tail
__global__ __launch_bounds__(kThreads) void adam_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, int64_t n, int64_t n4, AdamArgs a) {
  const int64_t items = n4 + (n - 4 * n4);
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < items; i += (int64_t)gridDim.x * kThreads) {
    if (i < n4) {
      float4 w4 = reinterpret_cast<float4*>(w)[i], m4 = reinterpret_cast<float4*>(m)[i], v4 = reinterpret_cast<float4*>(v)[i];
      const float4 g4 = reinterpret_cast<const float4*>(g)[i];
      adam_one(w4.x, g4.x, m4.x, v4.x, a);
      adam_one(w4.y, g4.y, m4.y, v4.y, a);
      adam_one(w4.z, g4.z, m4.z, v4.z, a);
      adam_one(w4.w, g4.w, m4.w, v4.w, a);
      reinterpret_cast<float4*>(w)[i] = w4;
      reinterpret_cast<float4*>(m)[i] = m4;
      reinterpret_cast<float4*>(v)[i] = v4;
    } else {
      const int64_t e = 4 * n4 + (i - n4);
      adam_one(w[e], g[e], m[e], v[e], a);
    }
  }
}

// row and column counts the 32-bit launch grids cover (addresses are 64-bit throughout)
static bool rows_fit(int64_t rows, int64_t ld) { return rows >= 0 && rows < (1ll << 31) && ld >= 0 && ld < (1ll << 31) && rows * ld < (1ll << 38); }

}  // namespace votehead
}  // namespace pcmi

using namespace pcmi;
using namespace pcmi::votehead;

extern "C" {

int pcmi_group_rows_fwd(const float* xyz, const float* centre, const float* feat, int64_t feat_ld, const int32_t* idx, int64_t B,
                        int64_t n, int64_t np, int64_t ns, int C, float radius_div, float* out, int64_t out_ld, int validate,
                        pcmi_stream_t stream) {
  PCMI_REQUIRE(B >= 0 && n >= 0 && np >= 0 && ns >= 0 && ns < (1ll << 31) && C >= 0 && B * n < (1ll << 31) / 3 &&
                   (ns == 0 || np == 0 || B * np < (1ll << 31) / ns),
               PCMI_ERR_INVALID, "group_rows_fwd: bad shape (B %lld, n %lld, np %lld, ns %lld, C %d)", (long long)B, (long long)n,
               (long long)np, (long long)ns, C);
  PCMI_REQUIRE(out_ld >= (int64_t)C + 3 && out_ld % 4 == 0 && feat_ld >= C, PCMI_ERR_INVALID,
               "group_rows_fwd: out_ld %lld must be a multiple of 4 and at least C + 3 = %d (feat_ld %lld >= C)", (long long)out_ld,
               C + 3, (long long)feat_ld);
  PCMI_REQUIRE(radius_div > 0.f, PCMI_ERR_INVALID, "group_rows_fwd: radius_div %g must be positive", (double)radius_div);
  const int64_t rows = B * np * ns;
  if (rows == 0) return PCMI_OK;
  PCMI_REQUIRE(centre && idx && out && aligned16(out) && (n == 0 || (xyz && (feat || C == 0))), PCMI_ERR_INVALID,
               "group_rows_fwd: null pointer (or out not 16-byte aligned)");
  hipStream_t st = as_stream(stream);
  if (validate) {
    unsigned* flag = stream_counters(st, 1);
    if (!flag) return PCMI_ERR_HIP;
    index_flag_kernel<<<(unsigned)ceil_div(rows, kThreads), kThreads, 0, st>>>(idx, rows, n, flag);
    PCMI_LAUNCH_CHECK();
    unsigned bad = 0;
    PCMI_HIP_CHECK(hipMemcpyAsync(&bad, flag, sizeof(bad), hipMemcpyDeviceToHost, st));
    PCMI_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(bad), st));  // the pool's counters are left at zero
    PCMI_HIP_CHECK(hipStreamSynchronize(st));
    PCMI_REQUIRE(!bad, PCMI_ERR_RANGE, "group_rows_fwd: an index is outside [0, %lld)", (long long)n);
  }
  const unsigned grid = (unsigned)ceil_div(rows, kWaves);
  if (C > 0 && C % 4 == 0 && feat_ld % 4 == 0 && aligned16(feat))
    group_rows_fwd_kernel<true><<<grid, kThreads, 0, st>>>(xyz, centre, feat, feat_ld, idx, rows, n, np, (int)ns, C, radius_div, out, out_ld);
  else
    group_rows_fwd_kernel<false><<<grid, kThreads, 0, st>>>(xyz, centre, feat, feat_ld, idx, rows, n, np, (int)ns, C, radius_div, out, out_ld);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

size_t pcmi_group_rows_bwd_workspace_bytes(int64_t B, int64_t n, int64_t np, int64_t ns) {
  return inverse_lists_workspace(std::max<int64_t>(B * np * ns, 1), std::max<int64_t>(B * n, 1));
}

int pcmi_group_rows_bwd(const float* gout, int64_t gout_ld, const int32_t* idx, int64_t B, int64_t n, int64_t np, int64_t ns, int C,
                        float radius_div, float* gfeat, int64_t gfeat_ld, float* gxyz, float* gcentre, void* ws, size_t ws_bytes,
                        pcmi_stream_t stream) {
  PCMI_REQUIRE(B >= 0 && n >= 0 && np >= 0 && ns >= 0 && ns < (1ll << 31) && C >= 0 && B * n < (1ll << 31) / 3 &&
                   (ns == 0 || np == 0 || B * np < ((1ll << 31) - 1) / ns),
               PCMI_ERR_INVALID, "group_rows_bwd: bad shape (B %lld, n %lld, np %lld, ns %lld, C %d)", (long long)B, (long long)n,
               (long long)np, (long long)ns, C);
  PCMI_REQUIRE(gout_ld >= (int64_t)C + 3 && gfeat_ld >= C, PCMI_ERR_INVALID, "group_rows_bwd: gout_ld %lld < C + 3 or gfeat_ld %lld < C",
               (long long)gout_ld, (long long)gfeat_ld);
  PCMI_REQUIRE(radius_div > 0.f, PCMI_ERR_INVALID, "group_rows_bwd: radius_div %g must be positive", (double)radius_div);
  const int64_t rows = B * np * ns, targets = B * n, groups = B * np;
  PCMI_REQUIRE((targets == 0 || (gxyz && (gfeat || C == 0))) && (groups == 0 || gcentre) && (rows == 0 || (gout && idx)), PCMI_ERR_INVALID,
               "group_rows_bwd: null pointer");
  hipStream_t st = as_stream(stream);
  if (rows == 0) {  // nothing was gathered: the gradients are zero
    if (targets > 0) {
      if (C > 0) PCMI_HIP_CHECK(hipMemset2DAsync(gfeat, (size_t)gfeat_ld * 4, 0, (size_t)C * 4, (size_t)targets, st));
      PCMI_HIP_CHECK(hipMemsetAsync(gxyz, 0, (size_t)targets * 12, st));
    }
    if (groups > 0) PCMI_HIP_CHECK(hipMemsetAsync(gcentre, 0, (size_t)groups * 12, st));
    return PCMI_OK;
  }
  if (targets > 0) {
    const int32_t *start = nullptr, *pos = nullptr;
    const int rc = inverse_lists("group_rows_bwd", idx, B, np * ns, n, ws, ws_bytes, &start, &pos, st);
    if (rc != PCMI_OK) return rc;
    const unsigned grid = (unsigned)ceil_div(targets, kWaves);
    if (C > 0 && C % 4 == 0 && gout_ld % 4 == 0 && gfeat_ld % 4 == 0 && aligned16(gout) && aligned16(gfeat))
      group_rows_bwd_points_kernel<true><<<grid, kThreads, 0, st>>>(gout, gout_ld, start, pos, targets, C, radius_div, gfeat, gfeat_ld, gxyz);
    else
      group_rows_bwd_points_kernel<false><<<grid, kThreads, 0, st>>>(gout, gout_ld, start, pos, targets, C, radius_div, gfeat, gfeat_ld, gxyz);
    PCMI_LAUNCH_CHECK();
  }
  group_rows_bwd_centre_kernel<<<(unsigned)ceil_div(groups * 3, kThreads), kThreads, 0, st>>>(gout, gout_ld, idx, groups, n, (int)ns, C,
                                                                                             radius_div, gcentre);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

int pcmi_rows_maxpool_fwd(const float* x, int64_t x_ld, int64_t R, int ns, int C, float* out, int64_t out_ld, uint8_t* arg,
                          pcmi_stream_t stream) {
  PCMI_REQUIRE(ns >= 1 && ns <= 256, PCMI_ERR_UNSUPPORTED, "rows_maxpool_fwd: %d rows per window, supported: 1 .. 256", ns);
  PCMI_REQUIRE(R >= 0 && C >= 0 && x_ld >= C && out_ld >= C && rows_fit(R * ns, x_ld), PCMI_ERR_INVALID,
               "rows_maxpool_fwd: bad shape (R %lld, C %d, x_ld %lld, out_ld %lld)", (long long)R, C, (long long)x_ld, (long long)out_ld);
  if (R == 0 || C == 0) return PCMI_OK;
  PCMI_REQUIRE(x && out && arg, PCMI_ERR_INVALID, "rows_maxpool_fwd: null pointer");
  hipStream_t st = as_stream(stream);
  if (C % 4 == 0 && x_ld % 4 == 0 && out_ld % 4 == 0 && aligned16(x) && aligned16(out) && ((uintptr_t)arg & 3) == 0)
    rows_maxpool_fwd_kernel<4><<<(unsigned)ceil_div(R * (C / 4), kThreads), kThreads, 0, st>>>(x, x_ld, R, ns, C, out, out_ld, arg);
  else
    rows_maxpool_fwd_kernel<1><<<(unsigned)ceil_div(R * C, kThreads), kThreads, 0, st>>>(x, x_ld, R, ns, C, out, out_ld, arg);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

int pcmi_rows_maxpool_bwd(const float* gout, int64_t gout_ld, const uint8_t* arg, int64_t R, int ns, int C, float* gx, int64_t gx_ld,
                          pcmi_stream_t stream) {
  PCMI_REQUIRE(ns >= 1 && ns <= 256, PCMI_ERR_UNSUPPORTED, "rows_maxpool_bwd: %d rows per window, supported: 1 .. 256", ns);
  PCMI_REQUIRE(R >= 0 && C >= 0 && gx_ld >= C && gout_ld >= C && rows_fit(R * ns, gx_ld), PCMI_ERR_INVALID,
               "rows_maxpool_bwd: bad shape (R %lld, C %d, gout_ld %lld, gx_ld %lld)", (long long)R, C, (long long)gout_ld,
               (long long)gx_ld);
  if (R == 0 || C == 0) return PCMI_OK;
  PCMI_REQUIRE(gout && arg && gx, PCMI_ERR_INVALID, "rows_maxpool_bwd: null pointer");
  hipStream_t st = as_stream(stream);
  if (C % 4 == 0 && gx_ld % 4 == 0 && gout_ld % 4 == 0 && aligned16(gx) && aligned16(gout) && ((uintptr_t)arg & 3) == 0)
    rows_maxpool_bwd_kernel<4><<<(unsigned)ceil_div(R * ns * (C / 4), kThreads), kThreads, 0, st>>>(gout, gout_ld, arg, R, ns, C, gx, gx_ld);
  else
    rows_maxpool_bwd_kernel<1><<<(unsigned)ceil_div(R * ns * C, kThreads), kThreads, 0, st>>>(gout, gout_ld, arg, R, ns, C, gx, gx_ld);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

static int vote_shape_ok(const char* who, int64_t R, int vf, int C, int Wb, int64_t net_ld) {
  PCMI_REQUIRE(R >= 0 && vf >= 1 && C >= 1 && Wb >= C + 3 && Wb % 4 == 0 && net_ld >= (int64_t)vf * Wb && net_ld < (1ll << 31) &&
                   R * vf < (1ll << 31) / 3 && rows_fit(R, net_ld),
               PCMI_ERR_INVALID, "%s: bad shape (R %lld, vote_factor %d, C %d, block width %d, ld %lld)", who, (long long)R, vf, C, Wb,
               (long long)net_ld);
  return PCMI_OK;
}

int pcmi_vote_fwd(const float* net, int64_t net_ld, const float* seed_xyz, const float* seed_feat, int64_t seed_feat_ld, int64_t R, int vf,
                  int C, int Wb, float* vote_xyz, float* vote_feat, int64_t vote_feat_ld, float* norm, pcmi_stream_t stream) {
  const int rc = vote_shape_ok("vote_fwd", R, vf, C, Wb, net_ld);
  if (rc != PCMI_OK) return rc;
  PCMI_REQUIRE(seed_feat_ld >= C && vote_feat_ld >= C, PCMI_ERR_INVALID, "vote_fwd: a leading dimension is below C = %d", C);
  if (R == 0) return PCMI_OK;
  PCMI_REQUIRE(net && seed_xyz && seed_feat && vote_xyz && vote_feat && norm, PCMI_ERR_INVALID, "vote_fwd: null pointer");
  hipStream_t st = as_stream(stream);
  const int64_t votes = R * vf;
  const unsigned grid = (unsigned)ceil_div(votes, kWaves);
  if (C % 4 == 0 && net_ld % 4 == 0 && seed_feat_ld % 4 == 0 && vote_feat_ld % 4 == 0 && aligned16(net) && aligned16(seed_feat) &&
      aligned16(vote_feat))
    vote_fwd_kernel<true><<<grid, kThreads, 0, st>>>(net, net_ld, seed_xyz, seed_feat, seed_feat_ld, votes, vf, C, Wb, vote_xyz, vote_feat,
                                                     vote_feat_ld, norm);
  else
    vote_fwd_kernel<false><<<grid, kThreads, 0, st>>>(net, net_ld, seed_xyz, seed_feat, seed_feat_ld, votes, vf, C, Wb, vote_xyz, vote_feat,
                                                      vote_feat_ld, norm);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

int pcmi_vote_bwd(const float* g_vote_feat, int64_t g_vote_feat_ld, const float* g_vote_xyz, const float* vote_feat, int64_t vote_feat_ld,
                  const float* norm, int64_t R, int vf, int C, int Wb, float* g_net, int64_t g_net_ld, float* g_seed_feat,
                  int64_t g_seed_feat_ld, float* g_seed_xyz, pcmi_stream_t stream) {
  const int rc = vote_shape_ok("vote_bwd", R, vf, C, Wb, g_net_ld);
  if (rc != PCMI_OK) return rc;
  PCMI_REQUIRE(g_vote_feat_ld >= C && vote_feat_ld >= C && g_seed_feat_ld >= C, PCMI_ERR_INVALID,
               "vote_bwd: a leading dimension is below C = %d", C);
  if (R == 0) return PCMI_OK;
  PCMI_REQUIRE(g_vote_feat && g_vote_xyz && vote_feat && norm && g_net && g_seed_feat && g_seed_xyz, PCMI_ERR_INVALID,
               "vote_bwd: null pointer");
  hipStream_t st = as_stream(stream);
  const unsigned grid = (unsigned)ceil_div(R, kWaves);
  if (C % 4 == 0 && g_net_ld % 4 == 0 && g_vote_feat_ld % 4 == 0 && vote_feat_ld % 4 == 0 && g_seed_feat_ld % 4 == 0 && aligned16(g_net) &&
      aligned16(g_vote_feat) && aligned16(vote_feat) && aligned16(g_seed_feat))
    vote_bwd_kernel<true><<<grid, kThreads, 0, st>>>(g_vote_feat, g_vote_feat_ld, g_vote_xyz, vote_feat, vote_feat_ld, norm, R, vf, C, Wb,
                                                     g_net, g_net_ld, g_seed_feat, g_seed_feat_ld, g_seed_xyz);
  else
    vote_bwd_kernel<false><<<grid, kThreads, 0, st>>>(g_vote_feat, g_vote_feat_ld, g_vote_xyz, vote_feat, vote_feat_ld, norm, R, vf, C, Wb,
                                                      g_net, g_net_ld, g_seed_feat, g_seed_feat_ld, g_seed_xyz);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

int pcmi_adam_step(float* w, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                   float weight_decay, int64_t t, pcmi_stream_t stream) {
  PCMI_REQUIRE(n >= 0 && t >= 1 && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f && lr >= 0.f &&
                   weight_decay >= 0.f,
               PCMI_ERR_INVALID, "adam_step: bad argument (n %lld, t %lld, lr %g, betas %g %g, eps %g, weight decay %g)", (long long)n,
               (long long)t, (double)lr, (double)beta1, (double)beta2, (double)eps, (double)weight_decay);
  if (n == 0) return PCMI_OK;
  PCMI_REQUIRE(w && g && m && v, PCMI_ERR_INVALID, "adam_step: null pointer");
  // the bias corrections as torch computes them: in double on the host, used as fp32 scalars on the device
  const double bc1 = 1.0 - std::pow((double)beta1, (double)t), bc2 = 1.0 - std::pow((double)beta2, (double)t);
  AdamArgs a;
  a.step_size = (float)((double)lr / bc1);
  a.beta1 = beta1;
  a.one_minus_beta1 = (float)(1.0 - (double)beta1);
  a.beta2 = beta2;
  a.one_minus_beta2 = (float)(1.0 - (double)beta2);
  a.bc2_sqrt = (float)std::sqrt(bc2);
  a.eps = eps;
  a.weight_decay = weight_decay;
  const int64_t n4 = (aligned16(w) && aligned16(g) && aligned16(m) && aligned16(v)) ? n / 4 : 0;
  const int64_t items = n4 + (n - 4 * n4);
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(items, kThreads), 256 * 8));
  adam_kernel<<<grid, kThreads, 0, as_stream(stream)>>>(w, g, m, v, n, n4, a);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

}  // extern "C"
