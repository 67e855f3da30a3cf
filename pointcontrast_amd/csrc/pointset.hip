// PointNet++ point-set ops of the VoteNet detection fine-tuning path (downstream/votenet_det_new of the reference:
// models/backbone_module.py:159-177 furthest_point_sample per scene, models/proposal_module.py:93 and the set-abstraction /
// feature-propagation modules through models/backbone/pointnet2/pointnet2_utils.py).  Written from the semantics in
// include/pcmi.h; gfx950, wave64, fp32 data, int32 indices.
//
// Arithmetic contract: every squared distance is ((dx*dx) + (dy*dy)) + (dz*dz) with each operation rounded on its own
// (contraction off for the whole file), so tests/pointset_ref.py reproduces every comparison bit for bit in numpy float32.
// No float atomics anywhere: the backward passes build inverse lists (integer count, scan, stable radix placement by flat
// source position) and accumulate every target in gather form, in ascending source position.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "cubscan.h"
#include "internal.h"

#pragma clang fp contract(off)

namespace pcmi {
namespace pointset {

typedef unsigned long long u64;

__device__ __forceinline__ float dist2(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return ((dx * dx) + (dy * dy)) + (dz * dz);
}

// ---- furthest point sampling --------------------------------------------------------------------------------------------
// One workgroup of 1024 threads (16 waves) per cloud; nothing ever waits on another workgroup.  Point p of the cloud lives
// in slot p / 1024 of thread p % 1024 (coalesced).  Tiers by the cloud's size n, one kernel instantiation each:
//   n <= 1024 / 4096 / 8192    coordinates AND running minima in registers (1 / 4 / 8 points per thread: 4 registers a point)
//   larger                     coordinates re-read on every pick from global memory and running minima in the caller's
//                              workspace: 20 bytes a point and pick, resident in the XCD's 4 MiB L2 up to ~200k points
// The 128-register budget of a 1024-thread workgroup sets 8192: 32 registers of points beside the ~75 of the pick's
// reduction (117 in all); 16 points per thread spill, and so did every attempt to keep only the minima of a larger cloud
// in registers (40 to 64 per thread: 464 to 944 bytes of scratch per lane), which is why there is no such tier.
// A pick is ONE 64-bit max of (float bits of the running minimum << 32) | ~index: non-negative floats order as unsigned
// integers, and ~index makes the lowest index win a tie.  In-wave: 6 xor-shuffle steps; across waves: each wave's winner
// (key and coordinates) goes to an LDS slot of buffer (pick & 1), ONE barrier, every thread reduces the 16 slots itself.
// The buffer of pick j is rewritten at pick j + 2, behind the barrier of pick j + 1 that every reader of j has passed.
// A running minimum < 0 marks a point that never takes part: outside the cloud, or within the 1e-3 ball of the origin.
constexpr int kFpsThreads = 1024;
constexpr int kFpsWaves = kFpsThreads / 64;
constexpr int kFpsRegCoordPoints = 8 * kFpsThreads;   // 8192

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const u64 o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

struct FpsShared {
  u64 key[2][kFpsWaves];
  float xyz[2][kFpsWaves][4];
};

// MODE 0: coordinates and minima in registers; 1: both from memory, minima in mind_ws (PPT unused)
template <int PPT, int MODE>
__device__ __forceinline__ void fps_cloud(const float* __restrict__ pts, int n, int m, int32_t* __restrict__ out,
                                          int32_t* __restrict__ out_rows, const int32_t* __restrict__ rows, int64_t start,
                                          float* __restrict__ mind_ws, FpsShared& sh) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float px[PPT], py[PPT], pz[PPT], mind[PPT];
  if constexpr (MODE == 0) {
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      const int p = k * kFpsThreads + tid;
      float x = 0.f, y = 0.f, z = 0.f;
      if (p < n) {
        x = pts[3 * (int64_t)p];
        y = pts[3 * (int64_t)p + 1];
        z = pts[3 * (int64_t)p + 2];
      }
      const float mag = ((x * x) + (y * y)) + (z * z);
      mind[k] = (p < n && mag > 1e-3f) ? 1e10f : -1.f;
      px[k] = x;
      py[k] = y;
      pz[k] = z;
    }
  } else {
    for (int p = tid; p < n; p += kFpsThreads) {
      const float x = pts[3 * (int64_t)p], y = pts[3 * (int64_t)p + 1], z = pts[3 * (int64_t)p + 2];
      const float mag = ((x * x) + (y * y)) + (z * z);
      mind_ws[p] = mag > 1e-3f ? 1e10f : -1.f;  // read back by the same thread only
    }
  }
  const float x0 = pts[0], y0 = pts[1], z0 = pts[2];
  float cx = x0, cy = y0, cz = z0;
  if (tid == 0) {
    out[0] = 0;
    if (out_rows) out_rows[0] = rows ? rows[start] : (int32_t)start;
  }
  int buf = 0;
  for (int j = 1; j < m; ++j) {
    u64 best = 0;
    float bx = 0.f, by = 0.f, bz = 0.f;
    if constexpr (MODE == 0) {
#pragma unroll
      for (int k = 0; k < PPT; ++k) {
        if (mind[k] >= 0.f) {
          const int p = k * kFpsThreads + tid;
          const float x = px[k], y = py[k], z = pz[k];
          const float mn = fminf(mind[k], dist2(x, y, z, cx, cy, cz));
          mind[k] = mn;
          const u64 key = ((u64)__float_as_uint(mn) << 32) | (uint32_t)~(uint32_t)p;
          if (key > best) {
            best = key;
            bx = x;
            by = y;
            bz = z;
          }
        }
      }
    } else {
#pragma unroll 4
      for (int p = tid; p < n; p += kFpsThreads) {
        const float old = mind_ws[p];
        if (old >= 0.f) {
          const float x = pts[3 * (int64_t)p], y = pts[3 * (int64_t)p + 1], z = pts[3 * (int64_t)p + 2];
          const float mn = fminf(old, dist2(x, y, z, cx, cy, cz));
          mind_ws[p] = mn;
          const u64 key = ((u64)__float_as_uint(mn) << 32) | (uint32_t)~(uint32_t)p;
          if (key > best) {
            best = key;
            bx = x;
            by = y;
            bz = z;
          }
        }
      }
    }
    const u64 wbest = wave_max_u64(best);
    // keys of distinct points differ (the index is part of them): one lane owns a non-zero maximum
    if (wbest != 0 ? best == wbest : lane == 0) {
      sh.key[buf][wave] = wbest;
      sh.xyz[buf][wave][0] = bx;
      sh.xyz[buf][wave][1] = by;
      sh.xyz[buf][wave][2] = bz;
    }
    __syncthreads();
    u64 g = 0;
    int gw = 0;
#pragma unroll
    for (int w = 0; w < kFpsWaves; ++w) {
      const u64 k = sh.key[buf][w];
      if (k > g) {
        g = k;
        gw = w;
      }
    }
    int pick = 0;
    if (g != 0) {
      pick = (int)~(uint32_t)g;
      cx = sh.xyz[buf][gw][0];
      cy = sh.xyz[buf][gw][1];
      cz = sh.xyz[buf][gw][2];
    } else {  // no point qualifies: index 0
      cx = x0;
      cy = y0;
      cz = z0;
    }
    if (tid == 0) {
      out[j] = pick;
      if (out_rows) out_rows[j] = rows ? rows[start + pick] : (int32_t)(start + pick);
    }
    buf ^= 1;
  }
}

// One instantiation per tier, so that each gets the registers its own tier needs; a workgroup whose cloud belongs to another
// tier leaves at once.  The host launches the tiers that the bound on the cloud size admits (a dense batch: exactly one).
// LO / HI: cloud sizes of this tier, inclusive (the LO == 0 tier also writes the -1 of empty clouds).
template <int PPT, int MODE, int LO, int HI>
__global__ __launch_bounds__(kFpsThreads) void fps_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ rows,
                                                          const int32_t* __restrict__ offs, int64_t n_points, int n_dense, int m,
                                                          int32_t* __restrict__ out, int32_t* __restrict__ out_rows,
                                                          float* __restrict__ mind_ws) {
  __shared__ FpsShared sh;
  const int i = blockIdx.x;
  int64_t start;
  int64_t cnt;
  if (offs) {
    start = offs[i];
    cnt = (int64_t)offs[i + 1] - start;
  } else {
    start = (int64_t)i * n_dense;
    cnt = n_dense;
  }
  // a segment table that does not fit the array is treated as an empty cloud
  if (start < 0 || cnt < 0 || start + cnt > n_points) cnt = 0;
  if (cnt < LO || cnt > HI) return;
  const int n = (int)cnt;
  out += (int64_t)i * m;
  if (out_rows) out_rows += (int64_t)i * m;
  if (n == 0) {
    for (int j = threadIdx.x; j < m; j += kFpsThreads) {
      out[j] = -1;
      if (out_rows) out_rows[j] = -1;
    }
    return;
  }
  fps_cloud<PPT, MODE>(xyz + 3 * start, n, m, out, out_rows, rows, start, MODE == 1 ? mind_ws + start : nullptr, sh);
}

// compact[q] = xyz[rows[q]] for the q < offs[n_clouds] entries of a segment table: the sampling kernel then reads each cloud
// contiguously on every pick instead of through the row list.  A row outside the array becomes the origin (never chosen).
__global__ void fps_compact_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ rows, const int32_t* __restrict__ offs,
                                   int64_t n_clouds, int64_t n_points, float* __restrict__ compact) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n_points || q >= offs[n_clouds]) return;
  const int32_t r = rows[q];
  const bool ok = r >= 0 && r < n_points;
  compact[3 * q] = ok ? xyz[3 * (int64_t)r] : 0.f;
  compact[3 * q + 1] = ok ? xyz[3 * (int64_t)r + 1] : 0.f;
  compact[3 * q + 2] = ok ? xyz[3 * (int64_t)r + 2] : 0.f;
}

// ---- ball query ---------------------------------------------------------------------------------------------------------
// Grid (query tile, cloud); 4 waves, each wave owns 4 queries.  The cloud streams through LDS in tiles of 1024 candidates
// shared by the workgroup's 16 queries; a wave tests 64 candidates per step, ballot + prefix popcount place the hits in
// ascending index; the workgroup leaves the stream once all of its queries are full.
constexpr int kBqThreads = 256;
constexpr int kBqQueriesPerWave = 4;
constexpr int kBqQueries = (kBqThreads / 64) * kBqQueriesPerWave;
constexpr int kTile = 1024;

__global__ __launch_bounds__(kBqThreads) void ball_query_kernel(const float* __restrict__ xyz, const float* __restrict__ new_xyz, int n,
                                                                int np, float r2, int nsample, int32_t* __restrict__ idx) {
  __shared__ float sx[kTile], sy[kTile], sz[kTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.y;
  const int q0 = blockIdx.x * kBqQueries + wave * kBqQueriesPerWave;
  const float* cloud = xyz + b * n * 3;
  float qx[kBqQueriesPerWave], qy[kBqQueriesPerWave], qz[kBqQueriesPerWave];
  int cnt[kBqQueriesPerWave], first[kBqQueriesPerWave];
#pragma unroll
  for (int k = 0; k < kBqQueriesPerWave; ++k) {
    const int q = q0 + k;
    const float* c = new_xyz + (b * np + (q < np ? q : 0)) * 3;
    qx[k] = c[0];
    qy[k] = c[1];
    qz[k] = c[2];
    cnt[k] = q < np ? 0 : nsample;  // a query past the end is "full" from the start
    first[k] = 0;
  }
  const u64 lanes_below = (1ull << lane) - 1ull;
  for (int t0 = 0; t0 < n; t0 += kTile) {
    const int tn = min(kTile, n - t0);
    for (int i = tid; i < tn; i += kBqThreads) {
      const float* p = cloud + (int64_t)(t0 + i) * 3;
      sx[i] = p[0];
      sy[i] = p[1];
      sz[i] = p[2];
    }
    __syncthreads();
    bool done = true;
#pragma unroll
    for (int k = 0; k < kBqQueriesPerWave; ++k) {
      int32_t* o = idx + (b * np + (q0 + k)) * nsample;  // dereferenced only while cnt < nsample, i.e. for q0 + k < np
      for (int c0 = 0; c0 < tn && cnt[k] < nsample; c0 += 64) {
        const int i = c0 + lane;
        const bool hit = i < tn && dist2(sx[i < tn ? i : 0], sy[i < tn ? i : 0], sz[i < tn ? i : 0], qx[k], qy[k], qz[k]) < r2;
        const u64 mask = __ballot(hit);
        if (mask) {
          if (cnt[k] == 0) first[k] = t0 + c0 + (int)__ffsll((long long)mask) - 1;
          const int slot = cnt[k] + __popcll(mask & lanes_below);
          if (hit && slot < nsample) o[slot] = t0 + i;
          cnt[k] = min(nsample, cnt[k] + (int)__popcll(mask));
        }
      }
      done = done && cnt[k] >= nsample;
    }
    if (__syncthreads_and(done)) break;  // also the barrier in front of the next tile's stores
  }
#pragma unroll
  for (int k = 0; k < kBqQueriesPerWave; ++k) {
    if (q0 + k >= np) continue;
    int32_t* o = idx + (b * np + (q0 + k)) * nsample;
    for (int s = cnt[k] + lane; s < nsample; s += 64) o[s] = first[k];  // no hit: cnt 0, first 0 -> zeros
  }
}

// ---- three nearest neighbours ---------------------------------------------------------------------------------------------
// One thread per unknown point, the known points of its cloud stream through LDS (broadcast reads) in ascending index;
// strict < keeps the lower index of a tie.
__global__ __launch_bounds__(256) void three_nn_kernel(const float* __restrict__ unknown, const float* __restrict__ known, int n, int m,
                                                       float* __restrict__ dist2_out, int32_t* __restrict__ idx_out) {
  __shared__ float sx[kTile], sy[kTile], sz[kTile];
  const int64_t b = blockIdx.y;
  const int u = blockIdx.x * 256 + threadIdx.x;
  const bool valid = u < n;
  const float* up = unknown + (b * n + (valid ? u : 0)) * 3;
  const float ux = up[0], uy = up[1], uz = up[2];
  float d0 = INFINITY, d1 = INFINITY, d2 = INFINITY;
  int i0 = 0, i1 = 0, i2 = 0;
  for (int t0 = 0; t0 < m; t0 += kTile) {
    const int tn = min(kTile, m - t0);
    for (int i = threadIdx.x; i < tn; i += 256) {
      const float* p = known + (b * m + t0 + i) * 3;
      sx[i] = p[0];
      sy[i] = p[1];
      sz[i] = p[2];
    }
    __syncthreads();
    if (valid) {
      for (int i = 0; i < tn; ++i) {
        const float d = dist2(ux, uy, uz, sx[i], sy[i], sz[i]);
        const int k = t0 + i;
        if (d < d0) {
          d2 = d1; i2 = i1;
          d1 = d0; i1 = i0;
          d0 = d; i0 = k;
        } else if (d < d1) {
          d2 = d1; i2 = i1;
          d1 = d; i1 = k;
        } else if (d < d2) {
          d2 = d; i2 = k;
        }
      }
    }
    __syncthreads();
  }
  if (valid) {
    float* dp = dist2_out + (b * n + u) * 3;
    int32_t* ip = idx_out + (b * n + u) * 3;
    dp[0] = d0; dp[1] = d1; dp[2] = d2;
    ip[0] = i0; ip[1] = i1; ip[2] = i2;
  }
}

// ---- channel-first gathers --------------------------------------------------------------------------------------------------
// grid (ceil(L / 256), C, B).  out[b, c, l] = feat[b, c, idx[b, l]]; an index outside [0, N) is never dereferenced (0 is written):
// with validate != 0 the host has refused the call before this launch.
__global__ void gather_cf_kernel(const float* __restrict__ feat, const int32_t* __restrict__ idx, int C, int64_t N, int64_t L,
                                 float* __restrict__ out) {
  const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (l >= L) return;
  const int64_t bc = (int64_t)blockIdx.z * C + blockIdx.y;
  const int32_t t = idx[(int64_t)blockIdx.z * L + l];
  out[bc * L + l] = (t >= 0 && t < N) ? feat[bc * N + t] : 0.f;
}

__global__ void interpolate_cf_kernel(const float* __restrict__ feat, const int32_t* __restrict__ idx, const float* __restrict__ weight,
                                      int C, int64_t M, int64_t n, float* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int64_t bc = (int64_t)blockIdx.z * C + blockIdx.y;
  const int64_t e = ((int64_t)blockIdx.z * n + j) * 3;
  const float* f = feat + bc * M;
  float v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int32_t t = idx[e + k];
    v[k] = weight[e + k] * ((t >= 0 && t < M) ? f[t] : 0.f);
  }
  out[bc * n + j] = (v[0] + v[1]) + v[2];
}

__global__ void index_check_kernel(const int32_t* __restrict__ idx, int64_t count, int64_t N, unsigned* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < count && (idx[i] < 0 || idx[i] >= N)) atomicOr(flag, 1u);
}

// ---- scatter-add in gather form ---------------------------------------------------------------------------------------------
// key[p] = b * N + idx[p] for flat source position p = b * L + l (an index outside [0, N): the dump key B * N, never read,
// and the flag); count[key]++ (integer atomics: the sum does not depend on their order).
__global__ void scatter_keys_kernel(const int32_t* __restrict__ idx, int64_t n_idx, int64_t L, int64_t N, int64_t n_targets,
                                    int32_t* __restrict__ keys, int32_t* __restrict__ iota, int32_t* __restrict__ count,
                                    unsigned* __restrict__ flag) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n_idx) return;
  const int32_t t = idx[p];
  int64_t key = n_targets;
  if (t >= 0 && t < N)
    key = (p / L) * N + t;
  else if (flag)
    atomicOr(flag, 1u);
  keys[p] = (int32_t)key;
  iota[p] = (int32_t)p;
  atomicAdd(&count[key], 1);
}

// grid (ceil(N / 256), C, B).  gin[b, c, t] = sum over the sources of (b, t), in ascending flat position p, of
// (weight[p] *) gout[b, c, (p - b L) / div]  (div: 1 for gather / group, 3 for the interpolation's [n, 3] index).
__global__ void scatter_accumulate_kernel(const float* __restrict__ gout, const float* __restrict__ weight,
                                          const int32_t* __restrict__ start, const int32_t* __restrict__ pos, int C, int64_t N,
                                          int64_t L, int div, float* __restrict__ gin) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= N) return;
  const int64_t b = blockIdx.z, bc = b * C + blockIdx.y;
  const int32_t s = start[b * N + t], e = start[b * N + t + 1];
  const float* g = gout + bc * (L / div);
  float acc = 0.f;
  for (int32_t i = s; i < e; ++i) {
    const int64_t p = pos[i];
    float v = g[(p - b * L) / div];
    if (weight) v = weight[p] * v;
    acc = acc + v;
  }
  gin[bc * N + t] = acc;
}

static size_t sort_bytes(int64_t n) {
  size_t b = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const int32_t*)nullptr, (int32_t*)nullptr, (const int32_t*)nullptr,
                                           (int32_t*)nullptr, (int)std::max<int64_t>(n, 1));
  return b;
}

static bool grid_ok(int64_t B, int C) { return B <= 65535 && C <= 65535; }

// syncs: PCMI_ERR_RANGE if any of idx[0 .. count) is outside [0, N)
static int check_indices(const int32_t* idx, int64_t count, int64_t N, const char* who, hipStream_t st) {
  if (count == 0) return PCMI_OK;
  unsigned* flag = stream_counters(st, 1);
  if (!flag) return PCMI_ERR_HIP;
  index_check_kernel<<<(unsigned)ceil_div(count, 256), 256, 0, st>>>(idx, count, N, flag);
  PCMI_LAUNCH_CHECK();
  unsigned bad = 0;
  PCMI_HIP_CHECK(hipMemcpyAsync(&bad, flag, sizeof(bad), hipMemcpyDeviceToHost, st));
  PCMI_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(bad), st));  // the pool's counters are left at zero
  PCMI_HIP_CHECK(hipStreamSynchronize(st));
  PCMI_REQUIRE(!bad, PCMI_ERR_RANGE, "%s: an index is outside [0, %lld)", who, (long long)N);
  return PCMI_OK;
}

static int gather_fwd(const char* who, const float* feat, const int32_t* idx, int64_t B, int C, int64_t N, int64_t L, float* out,
                      int validate, hipStream_t st) {
  PCMI_REQUIRE(B >= 0 && C >= 0 && N >= 0 && L >= 0 && grid_ok(B, C) && B * L < (1ll << 31) && B * N < (1ll << 31), PCMI_ERR_INVALID,
               "%s: bad shape (B %lld, C %d, N %lld, %lld indices per cloud)", who, (long long)B, C, (long long)N, (long long)L);
  if (B == 0 || C == 0 || L == 0) return PCMI_OK;
  PCMI_REQUIRE(feat && idx && out, PCMI_ERR_INVALID, "%s: null pointer", who);
  if (validate) {
    const int rc = check_indices(idx, B * L, N, who, st);
    if (rc != PCMI_OK) return rc;
  }
  gather_cf_kernel<<<dim3((unsigned)ceil_div(L, 256), (unsigned)C, (unsigned)B), 256, 0, st>>>(feat, idx, C, N, L, out);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

struct ScatterWs { int32_t *keys, *keys_sorted, *iota, *pos, *count, *start; void* temp; size_t temp_bytes, bytes; };
static ScatterWs scatter_ws(void* ws, int64_t n_idx, int64_t n_targets) {
  n_idx = std::max<int64_t>(n_idx, 1);
  n_targets = std::max<int64_t>(n_targets, 1);
  Carve cv{(char*)ws};
  ScatterWs w;
  w.keys = cv.take<int32_t>((size_t)n_idx);
  w.keys_sorted = cv.take<int32_t>((size_t)n_idx);
  w.iota = cv.take<int32_t>((size_t)n_idx);
  w.pos = cv.take<int32_t>((size_t)n_idx);
  w.count = cv.take<int32_t>((size_t)n_targets + 1);
  w.start = cv.take<int32_t>((size_t)n_targets + 1);
  w.temp_bytes = std::max(cub_scan_bytes<int32_t>(n_targets + 1), sort_bytes(n_idx));
  w.temp = cv.take<char>(w.temp_bytes);
  cv.take<char>(256);  // (unused tail the query has always counted)
  w.bytes = cv.used;
  return w;
}
static size_t scatter_workspace(int64_t n_idx, int64_t n_targets) { return scatter_ws(nullptr, n_idx, n_targets).bytes; }

// The inverse lists of idx [B, L] (targets in [0, N)): the flat source positions p = b L + l of target (b, t) are
// pos[start[b N + t] .. start[b N + t + 1]), in ascending p.  n_idx = B L > 0, n_targets = B N > 0; both < 2^31 - 1.
static int build_inverse_lists(const char* who, const int32_t* idx, int64_t B, int64_t L, int64_t N, int validate, void* ws,
                               size_t ws_bytes, const int32_t** start_out, const int32_t** pos_out, hipStream_t st) {
  const int64_t n_idx = B * L, n_targets = B * N;
  if (int rc = require_ws(who, ws, ws_bytes, scatter_workspace(n_idx, n_targets), 1)) return rc;
  const ScatterWs w = scatter_ws(ws, n_idx, n_targets);
  void* temp = w.temp;
  const size_t tb = w.temp_bytes;
  unsigned* flag = nullptr;
  if (validate) {
    flag = stream_counters(st, 1);
    if (!flag) return PCMI_ERR_HIP;
  }
  PCMI_HIP_CHECK(hipMemsetAsync(w.count, 0, (size_t)(n_targets + 1) * 4, st));
  scatter_keys_kernel<<<(unsigned)ceil_div(n_idx, 256), 256, 0, st>>>(idx, n_idx, L, N, n_targets, w.keys, w.iota, w.count, flag);
  PCMI_LAUNCH_CHECK();
  if (validate) {
    unsigned bad = 0;
    PCMI_HIP_CHECK(hipMemcpyAsync(&bad, flag, sizeof(bad), hipMemcpyDeviceToHost, st));
    PCMI_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(bad), st));
    PCMI_HIP_CHECK(hipStreamSynchronize(st));
    PCMI_REQUIRE(!bad, PCMI_ERR_RANGE, "%s: an index is outside [0, %lld)", who, (long long)N);
  }
  if (int rc = cub_scan_excl(temp, tb, w.count, w.start, n_targets + 1, st)) return rc;
  int bits = 1;
  while (bits < 31 && (1ll << bits) <= n_targets) ++bits;  // keys 0 .. n_targets
  // a stable sort of (key, flat position): the sources of a target end up in ascending position
  size_t stb = tb;
  PCMI_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(temp, stb, w.keys, w.keys_sorted, w.iota, w.pos, (int)n_idx, 0, bits, st));
  *start_out = w.start;
  *pos_out = w.pos;
  return PCMI_OK;
}

// idx: [B, L] targets in [0, N); gout: [B, C, L / div]; weight (nullable): [B, L]; gin: [B, C, N], written whole
static int scatter_bwd(const char* who, const float* gout, const int32_t* idx, const float* weight, int need_weight, int64_t B, int C,
                       int64_t N, int64_t L, int div, float* gin, int validate, void* ws, size_t ws_bytes, hipStream_t st) {
  PCMI_REQUIRE(B >= 0 && C >= 0 && N >= 0 && L >= 0 && grid_ok(B, C) && B * L < (1ll << 31) && B * N < (1ll << 31) - 1, PCMI_ERR_INVALID,
               "%s: bad shape (B %lld, C %d, N %lld, %lld indices per cloud)", who, (long long)B, C, (long long)N, (long long)L);
  if (B == 0 || C == 0 || N == 0) return PCMI_OK;
  PCMI_REQUIRE(gin && (L == 0 || (gout && idx && (!need_weight || weight))), PCMI_ERR_INVALID, "%s: null pointer", who);
  if (B * L == 0) {
    PCMI_HIP_CHECK(hipMemsetAsync(gin, 0, (size_t)B * C * N * 4, st));
    return PCMI_OK;
  }
  const int32_t *start = nullptr, *pos = nullptr;
  const int rc = build_inverse_lists(who, idx, B, L, N, validate, ws, ws_bytes, &start, &pos, st);
  if (rc != PCMI_OK) return rc;
  scatter_accumulate_kernel<<<dim3((unsigned)ceil_div(N, 256), (unsigned)C, (unsigned)B), 256, 0, st>>>(gout, weight, start, pos, C, N, L,
                                                                                                      div, gin);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

}  // namespace pointset

size_t inverse_lists_workspace(int64_t n_idx, int64_t n_targets) { return pointset::scatter_workspace(n_idx, n_targets); }
int inverse_lists(const char* who, const int32_t* idx, int64_t B, int64_t L, int64_t N, void* ws, size_t ws_bytes,
                  const int32_t** start, const int32_t** pos, hipStream_t st) {
  return pointset::build_inverse_lists(who, idx, B, L, N, 0, ws, ws_bytes, start, pos, st);
}
}  // namespace pcmi

using namespace pcmi;
using namespace pcmi::pointset;

extern "C" {

// null: a batch without a row list / no cloud beyond the register-resident tiers
struct FpsWs { float *compact, *mind; size_t bytes; };
static FpsWs fps_ws(void* ws, int64_t n_points, int64_t max_cloud, bool with_rows) {
  const size_t n = (size_t)std::max<int64_t>(n_points, 0);
  Carve cv{(char*)ws};
  FpsWs w;
  w.compact = with_rows ? cv.take<float>(n * 3) : nullptr;
  w.mind = max_cloud > kFpsRegCoordPoints ? cv.take<float>(n) : nullptr;
  w.bytes = cv.used;
  return w;
}

size_t pcmi_fps_workspace_bytes(int64_t n_points, int64_t max_cloud, int with_rows) {
  return fps_ws(nullptr, n_points, max_cloud, with_rows != 0).bytes;
}

int pcmi_fps(const float* xyz, int64_t n_points, const int32_t* rows, const int32_t* offs, int64_t n_clouds, int64_t max_cloud,
             int64_t m, int32_t* out, int32_t* out_rows, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_REQUIRE(n_points >= 0 && n_clouds >= 0 && max_cloud >= 0 && m >= 1 && n_points < (1ll << 31) / 3 && m < (1ll << 31) &&
                   n_clouds * m < (1ll << 31) && n_clouds < (1ll << 31),
               PCMI_ERR_INVALID, "fps: bad size (%lld points, %lld clouds of at most %lld, %lld picks)", (long long)n_points,
               (long long)n_clouds, (long long)max_cloud, (long long)m);
  PCMI_REQUIRE(offs || (!rows && n_clouds * max_cloud == n_points), PCMI_ERR_INVALID,
               "fps: a dense batch has no row list and n_clouds * max_cloud == n_points");
  if (n_clouds == 0) return PCMI_OK;
  PCMI_REQUIRE(out && (xyz || n_points == 0), PCMI_ERR_INVALID, "fps: null pointer");
  const size_t need = fps_ws(nullptr, n_points, max_cloud, rows != nullptr).bytes;  // 0: no piece, or no point
  if (need != 0)
    if (int rc = require_ws("fps", ws, ws_bytes, need, 1)) return rc;
  hipStream_t st = as_stream(stream);
  const FpsWs w = fps_ws(ws, n_points, max_cloud, rows != nullptr);
  const float* pts = xyz;
  if (rows && n_points > 0) {
    fps_compact_kernel<<<(unsigned)ceil_div(n_points, 256), 256, 0, st>>>(xyz, rows, offs, n_clouds, n_points, w.compact);
    PCMI_LAUNCH_CHECK();
    pts = w.compact;
  }
  float* mind_ws = w.mind;
  const int nd = offs ? 0 : (int)max_cloud;
  if (offs) {  // a cloud larger than the caller's bound belongs to no launched tier: it reads as empty
    PCMI_HIP_CHECK(hipMemsetAsync(out, 0xff, (size_t)n_clouds * m * 4, st));
    if (out_rows) PCMI_HIP_CHECK(hipMemsetAsync(out_rows, 0xff, (size_t)n_clouds * m * 4, st));
  }
  const int64_t lo = offs ? 0 : max_cloud, hi = max_cloud;  // cloud sizes that can occur
#define PCMI_FPS_TIER(PPT, MODE, LO, HI)                                                                                         \
  if (lo <= (HI) && hi >= (LO)) {                                                                                                \
    fps_kernel<PPT, MODE, LO, HI><<<(unsigned)n_clouds, kFpsThreads, 0, st>>>(pts, rows, offs, n_points, nd, (int)m, out, out_rows, \
                                                                              mind_ws);                                          \
    PCMI_LAUNCH_CHECK();                                                                                                         \
  }
  PCMI_FPS_TIER(1, 0, 0, kFpsThreads)
  PCMI_FPS_TIER(4, 0, kFpsThreads + 1, 4 * kFpsThreads)
  PCMI_FPS_TIER(8, 0, 4 * kFpsThreads + 1, kFpsRegCoordPoints)
  PCMI_FPS_TIER(1, 1, kFpsRegCoordPoints + 1, 0x7fffffff)
#undef PCMI_FPS_TIER
  return PCMI_OK;
}

int pcmi_ball_query(const float* xyz, const float* new_xyz, int64_t B, int64_t n, int64_t np, float radius, int nsample, int32_t* idx,
                    pcmi_stream_t stream) {
  PCMI_REQUIRE(B >= 0 && n >= 0 && np >= 0 && nsample >= 1 && radius >= 0.f && B <= 65535 && B * n < (1ll << 31) / 3 &&
                   B * np * nsample < (1ll << 31),
               PCMI_ERR_INVALID, "ball_query: bad size (B %lld, n %lld, np %lld, nsample %d, radius %g)", (long long)B, (long long)n,
               (long long)np, nsample, (double)radius);
  if (B == 0 || np == 0) return PCMI_OK;
  PCMI_REQUIRE(new_xyz && idx && (xyz || n == 0), PCMI_ERR_INVALID, "ball_query: null pointer");
  const float r2 = radius * radius;
  ball_query_kernel<<<dim3((unsigned)ceil_div(np, kBqQueries), (unsigned)B), kBqThreads, 0, as_stream(stream)>>>(xyz, new_xyz, (int)n,
                                                                                                                 (int)np, r2, nsample, idx);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

int pcmi_three_nn(const float* unknown, const float* known, int64_t B, int64_t n, int64_t m, float* dist2_out, int32_t* idx,
                  pcmi_stream_t stream) {
  PCMI_REQUIRE(B >= 0 && n >= 0 && m >= 0 && B <= 65535 && B * n < (1ll << 31) / 3 && B * m < (1ll << 31) / 3, PCMI_ERR_INVALID,
               "three_nn: bad size (B %lld, n %lld, m %lld)", (long long)B, (long long)n, (long long)m);
  PCMI_REQUIRE(m >= 3, PCMI_ERR_INVALID, "three_nn: %lld known points per cloud, three neighbours need at least 3", (long long)m);
  if (B == 0 || n == 0) return PCMI_OK;
  PCMI_REQUIRE(unknown && known && dist2_out && idx, PCMI_ERR_INVALID, "three_nn: null pointer");
  three_nn_kernel<<<dim3((unsigned)ceil_div(n, 256), (unsigned)B), 256, 0, as_stream(stream)>>>(unknown, known, (int)n, (int)m, dist2_out,
                                                                                                idx);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

size_t pcmi_pointset_scatter_workspace_bytes(int64_t n_idx, int64_t n_targets) { return scatter_workspace(n_idx, n_targets); }

int pcmi_gather_points_fwd(const float* feat, const int32_t* idx, int64_t B, int C, int64_t N, int64_t m, float* out, int validate,
                           pcmi_stream_t stream) {
  return gather_fwd("gather_points_fwd", feat, idx, B, C, N, m, out, validate, as_stream(stream));
}

int pcmi_gather_points_bwd(const float* gout, const int32_t* idx, int64_t B, int C, int64_t N, int64_t m, float* gfeat, int validate,
                           void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  return scatter_bwd("gather_points_bwd", gout, idx, nullptr, 0, B, C, N, m, 1, gfeat, validate, ws, ws_bytes, as_stream(stream));
}

int pcmi_group_points_fwd(const float* feat, const int32_t* idx, int64_t B, int C, int64_t N, int64_t np, int64_t ns, float* out,
                          int validate, pcmi_stream_t stream) {
  PCMI_REQUIRE(np >= 0 && ns >= 0 && (ns == 0 || np < (1ll << 31) / ns), PCMI_ERR_INVALID, "group_points_fwd: bad size (np %lld, ns %lld)",
               (long long)np, (long long)ns);
  return gather_fwd("group_points_fwd", feat, idx, B, C, N, np * ns, out, validate, as_stream(stream));
}

int pcmi_group_points_bwd(const float* gout, const int32_t* idx, int64_t B, int C, int64_t N, int64_t np, int64_t ns, float* gfeat,
                          int validate, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_REQUIRE(np >= 0 && ns >= 0 && (ns == 0 || np < (1ll << 31) / ns), PCMI_ERR_INVALID, "group_points_bwd: bad size (np %lld, ns %lld)",
               (long long)np, (long long)ns);
  return scatter_bwd("group_points_bwd", gout, idx, nullptr, 0, B, C, N, np * ns, 1, gfeat, validate, ws, ws_bytes, as_stream(stream));
}

int pcmi_three_interpolate_fwd(const float* feat, const int32_t* idx, const float* weight, int64_t B, int C, int64_t M, int64_t n,
                               float* out, int validate, pcmi_stream_t stream) {
  PCMI_REQUIRE(B >= 0 && C >= 0 && M >= 0 && n >= 0 && grid_ok(B, C) && B * n < (1ll << 31) / 3 && B * M < (1ll << 31), PCMI_ERR_INVALID,
               "three_interpolate_fwd: bad shape (B %lld, C %d, M %lld, n %lld)", (long long)B, C, (long long)M, (long long)n);
  if (B == 0 || C == 0 || n == 0) return PCMI_OK;
  PCMI_REQUIRE(feat && idx && weight && out, PCMI_ERR_INVALID, "three_interpolate_fwd: null pointer");
  hipStream_t st = as_stream(stream);
  if (validate) {
    const int rc = check_indices(idx, B * n * 3, M, "three_interpolate_fwd", st);
    if (rc != PCMI_OK) return rc;
  }
  interpolate_cf_kernel<<<dim3((unsigned)ceil_div(n, 256), (unsigned)C, (unsigned)B), 256, 0, st>>>(feat, idx, weight, C, M, n, out);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

int pcmi_three_interpolate_bwd(const float* gout, const int32_t* idx, const float* weight, int64_t B, int C, int64_t M, int64_t n,
                               float* gfeat, int validate, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_REQUIRE(n >= 0 && n < (1ll << 31) / 3, PCMI_ERR_INVALID, "three_interpolate_bwd: bad size (n %lld)", (long long)n);
  return scatter_bwd("three_interpolate_bwd", gout, idx, weight, 1, B, C, M, n * 3, 3, gfeat, validate, ws, ws_bytes, as_stream(stream));
}

}  // extern "C"
