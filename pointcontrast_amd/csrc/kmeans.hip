// Active labelling (Hou et al., "Contrastive Scene Contexts", the data-efficient benchmark): batched k-means on per-voxel
// features, one segment of rows per scene, all scenes in one launch sequence -- initialisation from given rows, the Lloyd
// iteration (assignment and fixed-point accumulation in ONE pass over the features), the final pass (member nearest to
// each centre, inertia) and one step of k-means++ seeding with the draws as data.  Written from the semantics in
// include/pcmi.h; gfx950, wave64.
//
// Arithmetic.  Distances are the fp32 chain of feat_nn_kernel (featmatch.hip): d2 = fma(a_c - b_c, a_c - b_c, d2) over
// ascending c, so d2 >= +0 and its bit pattern orders like the number; the choice among clusters (and among rows, for
// `nearest`) is an integer minimum on (d2 bits << 32 | index).  Sums are 2^-32 fixed point in 64-bit integer atomics (LDS
// or global), the seeding weights 2^-20 fixed point in unsigned 64-bit integers: no order of arrival changes a result.
// The inertia is fp64 partials per 256 rows merged in a fixed order.  The only atomics are integer ones.
#include <algorithm>
#include <atomic>

#include "blockscan.h"
#include "exact.h"
#include "internal.h"

#pragma clang fp contract(off)

namespace pcmi {
namespace kmeans {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTQ = 64, kTS = 64;              // rows per tile, clusters per tile step (a thread holds 4 x 4)
constexpr int kMaxK = PCMI_KMEANS_MAX_K;
constexpr int64_t kMaxSceneRows = PCMI_KMEANS_MAX_SCENE_ROWS;
constexpr int kMaxScenes = 65535;              // grid.y of the seeding and inertia launches
constexpr float kClamp = 1024.f;               // |x| beyond this (or not finite): the row is inactive
constexpr double kFix = 4294967296.0;          // 2^32: the fixed point of the sums
constexpr size_t kLdsBudget = 80 << 10;        // LDS of one workgroup of the step: two of them per CU (160 KiB)
constexpr int kSeedChunk = 4096, kSeedSlabs = kSeedChunk / kThreads;  // rows per chunk total of the seeding; its slabs of 256
constexpr int kSeedChunks = (int)(kMaxSceneRows / kSeedChunk);        // 256: one chunk total per thread of the pick
constexpr int kPartRows = 256;                 // rows per inertia partial
constexpr int kParts = (int)(kMaxSceneRows / kPartRows), kPartBlocks = 64;
constexpr unsigned long long kNoKey = ~0ull;
constexpr int kNoRow = 0x7f7f7f7f;             // "no active row": what a memset of 0x7f leaves, above every row index allowed

__device__ inline int64_t clampi(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ inline float fnan() { return __uint_as_float(0x7fc00000u); }

// scene b = the rows [lo, hi): its segment of offs inside [0, n], cut to its first max_rows rows
__device__ inline void scene_bounds(const int64_t* __restrict__ offs, int b, int64_t n, int64_t max_rows, int64_t* lo, int64_t* hi) {
  const int64_t l = clampi(offs[b], 0, n), h = clampi(offs[b + 1], l, n);
  *lo = l;
  *hi = h - l > max_rows ? l + max_rows : h;
}

__device__ inline bool ok4(float4 v) { return fabsf(v.x) <= kClamp && fabsf(v.y) <= kClamp && fabsf(v.z) <= kClamp && fabsf(v.w) <= kClamp; }

// whether the row is active; *d2 = its distance to the centre s_c (nullable) in the fp32 chain
__device__ inline bool row_active_d2(const float* __restrict__ row, int C, const float* s_c, float* d2) {
  bool ok = true;
  float acc = 0.f;
  for (int c = 0; c < C; c += 4) {
    const float4 v = *reinterpret_cast<const float4*>(row + c);
    ok = ok && ok4(v);
    if (s_c) {
      float df = v.x - s_c[c];
      acc = fmaf(df, df, acc);
      df = v.y - s_c[c + 1];
      acc = fmaf(df, df, acc);
      df = v.z - s_c[c + 2];
      acc = fmaf(df, df, acc);
      df = v.w - s_c[c + 3];
      acc = fmaf(df, df, acc);
    }
  }
  *d2 = acc;
  return ok;
}

__global__ __launch_bounds__(kThreads) void km_fill_kernel(int32_t* __restrict__ assign, float* __restrict__ d2, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  assign[i] = -1;
  if (d2) d2[i] = fnan();
}

// ---- initialisation -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void km_init_kernel(const float* __restrict__ feat, int64_t ld, int64_t n, const int64_t* __restrict__ offs,
                                                           int B, int K, int C, int64_t max_rows, const int32_t* __restrict__ init_rows,
                                                           float* __restrict__ centroid, int32_t* __restrict__ live,
                                                           unsigned long long* __restrict__ flags) {
  const int64_t bk = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (bk >= (int64_t)B * K) return;
  const int b = (int)(bk / K);
  int64_t lo, hi;
  scene_bounds(offs, b, n, max_rows, &lo, &hi);
  const int64_t r = init_rows[bk];
  bool ok = r >= lo && r < hi;
  if (ok) {
    float unused;
    ok = row_active_d2(feat + r * ld, C, nullptr, &unused);
  }
  for (int c = 0; c < C; ++c) centroid[bk * C + c] = ok ? feat[r * ld + c] : 0.f;
  live[bk] = ok ? (int32_t)r : -1;
  if (!ok && r >= 0) atomicAdd(&flags[b], 1ull);
}

// ---- the Lloyd iteration and the final pass -----------------------------------------------------------------------------------
struct TileArgs {
  const float* feat; int64_t ld, n;
  const int64_t* offs;
  int K, nch;
  int64_t max_rows;
  const float* centroid;        // [B, K, C]
  const int32_t* live;          // [B, K]
  const int32_t* assign_prev;   // nullable
  int32_t* assign;
  float* d2;                    // the final pass
  unsigned long long* sum;      // [B, K, C], the iteration
  int32_t* cnt;                 // [B, K]
  unsigned long long* changed;  // [B], the iteration
  unsigned long long* skipped;  // [B]
  unsigned long long* near;     // [B, K], the final pass
  int lds_acc;                  // the iteration: sums and counts in LDS (K (8 C + 4) bytes of dynamic LDS), flushed once
};

// grid.x: the scene; grid.y: the row chunks it is cut into.  A workgroup walks its chunk in tiles of 64 rows: the tile stays
// in LDS, channel-major, while the scene's centroids pass through LDS 64 clusters x KC channels at a time (feat_nn_kernel's
// walk: 32 channels, or 16 where 32 does not divide C); the same LDS tile then feeds the fixed-point accumulation, so the
// features are read from memory once.
template <int C, bool FINAL>
__global__ __launch_bounds__(kThreads) void km_tile_kernel(TileArgs a) {
  constexpr int KC = C % 32 == 0 ? 32 : 16;
  static_assert(C % KC == 0 && C % 16 == 0 && C >= 16 && C <= 128, "the channel steps cover the row exactly");
  extern __shared__ unsigned long long s_acc[];  // [K * C] sums, then [K] counts (unsigned)
  __shared__ __attribute__((aligned(16))) float sa[C][kTQ + 4];
  __shared__ __attribute__((aligned(16))) float sb[KC][kTS + 4];
  __shared__ int s_k[kTQ], s_bad[kTQ], s_live[kTS];
  __shared__ unsigned s_changed, s_skipped;
  const int t = threadIdx.x, tr = t / 16, tc = t % 16, b = blockIdx.x, K = a.K;
  int64_t lo, hi;
  scene_bounds(a.offs, b, a.n, a.max_rows, &lo, &hi);
  if (blockIdx.y == 0 && t == 0) {  // the rows that max_scene_rows cut off the scene are skipped rows too: the caller sees the cut
    const int64_t whole = clampi(a.offs[b + 1], lo, a.n);
    if (whole > hi) atomicAdd(&a.skipped[b], (unsigned long long)(whole - hi));
  }
  const int64_t cs = ((hi - lo + a.nch - 1) / a.nch + kTQ - 1) / kTQ * kTQ;
  const int64_t c_begin = lo + (int64_t)blockIdx.y * cs;
  const int64_t c_end = c_begin + cs < hi ? c_begin + cs : hi;
  if (c_begin >= c_end) return;  // (the whole workgroup)
  unsigned* s_cnt = reinterpret_cast<unsigned*>(s_acc + (size_t)K * C);
  const bool lds_acc = !FINAL && a.lds_acc != 0;
  if (lds_acc) {
    for (int e = t; e < K * C; e += kThreads) s_acc[e] = 0ull;
    for (int e = t; e < K; e += kThreads) s_cnt[e] = 0u;
  }
  if (t == 0) s_changed = s_skipped = 0u;
  const float* cen = a.centroid + (int64_t)b * K * C;

  for (int64_t r0 = c_begin; r0 < c_end; r0 += kTQ) {
    __syncthreads();  // the previous tile's accumulation is done with sa and s_k
    if (t < kTQ) s_bad[t] = 0;
    __syncthreads();
    for (int e = t; e < kTQ * (C / 4); e += kThreads) {
      const int row = e / (C / 4), c4 = e % (C / 4);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r0 + row < c_end) {
        v = *reinterpret_cast<const float4*>(a.feat + (r0 + row) * a.ld + c4 * 4);
        if (!ok4(v)) s_bad[row] = 1;  // (every writer stores the same value)
      }
      sa[c4 * 4 + 0][row] = v.x;
      sa[c4 * 4 + 1][row] = v.y;
      sa[c4 * 4 + 2][row] = v.z;
      sa[c4 * 4 + 3][row] = v.w;
    }
    unsigned long long best[4] = {kNoKey, kNoKey, kNoKey, kNoKey};
    for (int k0 = 0; k0 < K; k0 += kTS) {
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
          if (k0 + row < K) v = *reinterpret_cast<const float4*>(cen + (int64_t)(k0 + row) * C + kc + c4 * 4);
          sb[c4 * 4 + 0][row] = v.x;
          sb[c4 * 4 + 1][row] = v.y;
          sb[c4 * 4 + 2][row] = v.z;
          sb[c4 * 4 + 3][row] = v.w;
        }
        if (kc == 0 && t < kTS) s_live[t] = (k0 + t < K && a.live[(int64_t)b * K + k0 + t] >= 0) ? 1 : 0;
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
          const int kk = k0 + tc * 4 + j;
          if (kk < K && s_live[tc * 4 + j] != 0 && acc[i][j] < INFINITY) {  // false for NaN and +inf: never chosen
            const unsigned long long key = ((unsigned long long)__float_as_uint(acc[i][j]) << 32) | (unsigned long long)(uint32_t)kk;
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
      const int row = tr * 4 + i;
      const int64_t r = r0 + row;
      if (tc != 0) continue;
      if (r >= c_end) {
        s_k[row] = -1;
        continue;
      }
      const bool bad = s_bad[row] != 0;
      const int k = (bad || best[i] == kNoKey) ? -1 : (int)(uint32_t)(best[i] & 0xffffffffull);
      const uint32_t bits = (uint32_t)(best[i] >> 32);
      s_k[row] = k;
      a.assign[r] = k;
      if (bad) atomicAdd(&s_skipped, 1u);
      if (FINAL) {
        a.d2[r] = k < 0 ? fnan() : __uint_as_float(bits);
        if (k >= 0) {
          atomicAdd(&a.cnt[(int64_t)b * K + k], 1);
          atomicMin(&a.near[(int64_t)b * K + k], ((unsigned long long)bits << 32) | (unsigned long long)(uint32_t)r);
        }
      } else {
        if ((a.assign_prev ? a.assign_prev[r] : -1) != k) atomicAdd(&s_changed, 1u);
        if (k >= 0) {
          if (lds_acc) atomicAdd(&s_cnt[k], 1u);
          else atomicAdd(&a.cnt[(int64_t)b * K + k], 1);
        }
      }
    }
    if (!FINAL) {
      __syncthreads();
      for (int e = t; e < kTQ * C; e += kThreads) {
        const int row = e % kTQ, c = e / kTQ;
        const int k = s_k[row];
        if (k < 0) continue;
        const long long q = (long long)rint((double)sa[c][row] * kFix);
        if (q == 0) continue;
        if (lds_acc) atomicAdd(&s_acc[(size_t)k * C + c], (unsigned long long)q);
        else atomicAdd(&a.sum[((int64_t)b * K + k) * C + c], (unsigned long long)q);
      }
    }
  }
  __syncthreads();
  if (lds_acc) {
    for (int e = t; e < K * C; e += kThreads) {
      const unsigned long long v = s_acc[e];
      if (v != 0ull) atomicAdd(&a.sum[(int64_t)b * K * C + e], v);
    }
    for (int e = t; e < K; e += kThreads) {
      const unsigned v = s_cnt[e];
      if (v != 0u) atomicAdd(&a.cnt[(int64_t)b * K + e], (int)v);
    }
  }
  if (t == 0) {
    if (!FINAL && s_changed != 0u) atomicAdd(&a.changed[b], (unsigned long long)s_changed);
    if (s_skipped != 0u) atomicAdd(&a.skipped[b], (unsigned long long)s_skipped);
  }
}

__global__ __launch_bounds__(kThreads) void km_centroid_kernel(const long long* __restrict__ sum, const int32_t* __restrict__ cnt,
                                                               const int32_t* __restrict__ live, const float* centroid_in,
                                                               float* centroid_out, int64_t total, int C) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= total) return;
  const int64_t bk = e / C;
  const int32_t c = cnt[bk];
  float v = 0.f;  // a dead cluster
  if (live[bk] >= 0) v = c > 0 ? (float)div_rn((double)sum[e], mul_rn((double)c, kFix)) : centroid_in[e];
  centroid_out[e] = v;
}

// the sum over the workgroup's threads in a fixed order: a butterfly inside each wave, the waves in ascending order
__device__ inline double block_sum(double v, double* s_wave /* [kWaves] */) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
  __syncthreads();  // the previous call's readers are done
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = s_wave[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) t += s_wave[w];
  return t;
}

// partial p of scene b: the rows [lo + 256 p, lo + 256 (p + 1)) of the scene, one per lane, non-members as 0
__global__ __launch_bounds__(kThreads) void km_inertia_partial_kernel(const int32_t* __restrict__ assign, const float* __restrict__ d2, int64_t n,
                                                                      const int64_t* __restrict__ offs, int64_t max_rows,
                                                                      double* __restrict__ part) {
  __shared__ double s_wave[kWaves];
  const int b = blockIdx.y;
  int64_t lo, hi;
  scene_bounds(offs, b, n, max_rows, &lo, &hi);
  const int64_t np = (hi - lo + kPartRows - 1) / kPartRows;
  for (int64_t p = blockIdx.x; p < np; p += kPartBlocks) {  // (uniform over the workgroup)
    const int64_t i = lo + p * kPartRows + threadIdx.x;
    const double v = (i < hi && assign[i] >= 0) ? (double)d2[i] : 0.0;
    const double s = block_sum(v, s_wave);
    if (threadIdx.x == 0) part[(int64_t)b * kParts + p] = s;
  }
}

// one workgroup per scene: thread t adds the partials t, t + 256, ... in that order, then block_sum; and the nearest rows
__global__ __launch_bounds__(kThreads) void km_final_kernel(const double* __restrict__ part, int64_t n, const int64_t* __restrict__ offs,
                                                            int64_t max_rows, int K, const unsigned long long* __restrict__ near,
                                                            double* __restrict__ inertia, int32_t* __restrict__ nearest) {
  __shared__ double s_wave[kWaves];
  const int b = blockIdx.x;
  int64_t lo, hi;
  scene_bounds(offs, b, n, max_rows, &lo, &hi);
  const int64_t np = (hi - lo + kPartRows - 1) / kPartRows;
  double acc = 0.0;
  for (int64_t p = threadIdx.x; p < np; p += kThreads) acc += part[(int64_t)b * kParts + p];
  acc = block_sum(acc, s_wave);
  if (threadIdx.x == 0) inertia[b] = acc;
  for (int k = threadIdx.x; k < K; k += kThreads) {
    const unsigned long long key = near[(int64_t)b * K + k];
    nearest[(int64_t)b * K + k] = key == kNoKey ? -1 : (int32_t)(uint32_t)(key & 0xffffffffull);
  }
}

// ---- k-means++ seeding --------------------------------------------------------------------------------------------------------
__device__ inline unsigned long long seed_weight(float m) { return (unsigned long long)(fminf(m, 1048576.f) * 1048576.f); }

// grid (slabs, B): slab blockIdx.x of scene blockIdx.y, 256 rows, one per lane; 16 slabs make a chunk of 4096 rows.  Lowers
// mind2 to the distance to the scene's last centre and adds the slab's weights to its chunk's total and its lowest active row
// to the chunk's minimum (integer atomics on zeroed / kNoRow-filled words: the order changes nothing).
__global__ __launch_bounds__(kThreads) void km_seed_weights_kernel(const float* __restrict__ feat, int64_t ld, int64_t n,
                                                                   const int64_t* __restrict__ offs, int C, int64_t max_rows,
                                                                   const int32_t* __restrict__ last, float* __restrict__ mind2,
                                                                   unsigned long long* __restrict__ tot, int32_t* __restrict__ firstc) {
  __shared__ __attribute__((aligned(16))) float s_c[128];
  __shared__ int s_cok;
  __shared__ unsigned long long s_wave[kWaves];
  __shared__ int s_first;
  const int t = threadIdx.x, b = blockIdx.y;
  int64_t lo, hi;
  scene_bounds(offs, b, n, max_rows, &lo, &hi);
  const int64_t base = lo + (int64_t)blockIdx.x * kThreads;
  if (base >= hi) return;  // (the whole workgroup)
  const int64_t ctr = last ? (int64_t)last[b] : -1;
  const bool have = ctr >= lo && ctr < hi;
  if (t == 0) {
    s_cok = have ? 1 : 0;
    s_first = kNoRow;
  }
  __syncthreads();
  if (have && t < C) {
    const float v = feat[ctr * ld + t];
    s_c[t] = v;
    if (!(fabsf(v) <= kClamp)) s_cok = 0;
  }
  __syncthreads();
  const bool lower = s_cok != 0;
  unsigned long long w = 0ull;
  const int64_t i = base + t;
  float d2;
  if (i < hi && row_active_d2(feat + i * ld, C, lower ? s_c : nullptr, &d2)) {
    float m = mind2[i];
    if (lower && !(m <= d2)) {  // (a NaN in mind2 is lowered too)
      m = d2;
      mind2[i] = m;
    }
    w = seed_weight(m);
    atomicMin(&s_first, (int)i);
  }
  unsigned long long total;
  (void)block_scan_add64<kWaves>(w, s_wave, &total);  // (its barriers order s_first too)
  if (t == 0) {
    const int64_t slot = (int64_t)b * kSeedChunks + blockIdx.x / kSeedSlabs;
    if (total != 0ull) atomicAdd(&tot[slot], total);
    if (s_first != kNoRow) atomicMin(&firstc[slot], s_first);
  }
}

// one workgroup per scene: scans the chunk totals, then the slabs of the chunk that holds the target
__global__ __launch_bounds__(kThreads) void km_seed_pick_kernel(const float* __restrict__ feat, int64_t ld, int64_t n,
                                                                const int64_t* __restrict__ offs, int C, int64_t max_rows,
                                                                const float* __restrict__ mind2, const unsigned long long* __restrict__ tot,
                                                                const int32_t* __restrict__ firstc, const unsigned long long* __restrict__ draw,
                                                                int32_t* __restrict__ next) {
  __shared__ unsigned long long s_wave[kWaves];
  __shared__ unsigned long long s_rem;
  __shared__ int s_chunk, s_first, s_row;
  const int t = threadIdx.x, b = blockIdx.x;
  int64_t lo, hi;
  scene_bounds(offs, b, n, max_rows, &lo, &hi);
  const int nchunks = (int)((hi - lo + kSeedChunk - 1) / kSeedChunk);  // <= 256
  if (t == 0) {
    s_first = kNoRow;
    s_chunk = -1;
    s_row = -1;
    s_rem = 0ull;
  }
  __syncthreads();
  const unsigned long long v = t < nchunks ? tot[(int64_t)b * kSeedChunks + t] : 0ull;
  const int f = t < nchunks ? firstc[(int64_t)b * kSeedChunks + t] : kNoRow;
  if (f != kNoRow) atomicMin(&s_first, f);
  unsigned long long total;
  const unsigned long long incl = block_scan_add64<kWaves>(v, s_wave, &total);
  const unsigned long long target = total != 0ull ? __umul64hi(total, draw[b]) : 0ull;
  if (total != 0ull && incl > target && incl - v <= target) {  // exactly one thread
    s_chunk = t;
    s_rem = target - (incl - v);
  }
  __syncthreads();
  if (total == 0ull) {  // no weight: the lowest active row, -1 if the scene has none
    if (t == 0) next[b] = s_first == kNoRow ? -1 : s_first;
    return;
  }
  const int64_t base = lo + (int64_t)s_chunk * kSeedChunk;
  unsigned long long rem = s_rem;
  for (int j = 0; j < kSeedSlabs; ++j) {  // (uniform: rem and the slab totals are the same in every thread)
    const int64_t i = base + (int64_t)j * kThreads + t;
    unsigned long long w = 0ull;
    float unused;
    if (i < hi && row_active_d2(feat + i * ld, C, nullptr, &unused)) w = seed_weight(mind2[i]);
    unsigned long long slab;
    const unsigned long long in2 = block_scan_add64<kWaves>(w, s_wave, &slab);
    if (rem < slab) {
      if (in2 > rem && in2 - w <= rem) s_row = (int)i;
      break;
    }
    rem -= slab;
  }
  __syncthreads();
  if (t == 0) next[b] = s_row;
}

template <int C, bool FINAL>
static int launch_tile(dim3 grid, size_t lds, hipStream_t st, const TileArgs& a) {
  if (lds > 0) {  // once per instantiation and device (setting it twice in a race is harmless): dynamic LDS up to the budget
    static std::atomic<unsigned long long> raised{0ull};
    int dev = 0;
    PCMI_HIP_CHECK(hipGetDevice(&dev));
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(raised.load(std::memory_order_relaxed) & bit)) {
      PCMI_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&km_tile_kernel<C, FINAL>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)kLdsBudget));
      raised.fetch_or(bit, std::memory_order_relaxed);
    }
  }
  km_tile_kernel<C, FINAL><<<grid, kThreads, lds, st>>>(a);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

template <bool FINAL>
static int dispatch_tile(int c, dim3 grid, size_t lds, hipStream_t st, const TileArgs& a) {
  switch (c) {
    case 16: return launch_tile<16, FINAL>(grid, lds, st, a);
    case 32: return launch_tile<32, FINAL>(grid, lds, st, a);
    case 48: return launch_tile<48, FINAL>(grid, lds, st, a);
    case 64: return launch_tile<64, FINAL>(grid, lds, st, a);
    case 80: return launch_tile<80, FINAL>(grid, lds, st, a);
    case 96: return launch_tile<96, FINAL>(grid, lds, st, a);
    case 112: return launch_tile<112, FINAL>(grid, lds, st, a);
    case 128: return launch_tile<128, FINAL>(grid, lds, st, a);
  }
  return PCMI_ERR_UNSUPPORTED;
}

// static LDS of km_tile_kernel<C>: the row tile, the centroid tile, the per-row and per-cluster flags
static size_t tile_static_lds(int c) {
  const int kc = c % 32 == 0 ? 32 : 16;
  return (size_t)(c + kc) * (kTQ + 4) * 4 + (2 * kTQ + kTS) * 4 + 16;
}
static size_t acc_lds(int K, int c) { return (size_t)K * c * 8 + (size_t)K * 4; }

// row chunks per scene: tiles of 1024 rows of the whole call, at most two workgroups per CU over all scenes
static int row_chunks(int64_t n, int64_t B) {
  const int64_t by_rows = ceil_div(std::max<int64_t>(n, 1), 1024), by_chip = std::max<int64_t>(1, 2 * (int64_t)num_cu() / B);
  return (int)std::min<int64_t>({by_rows, by_chip, 65535});
}

static int check_common(const char* who, const float* feat, int64_t ld, int64_t n, const int64_t* offs, int64_t B, int K, int c,
                        int64_t max_rows) {
  PCMI_REQUIRE(c >= 16 && c <= 128 && c % 16 == 0, PCMI_ERR_UNSUPPORTED, "%s: feature width %d is not a multiple of 16 in 16..128", who, c);
  PCMI_REQUIRE(K >= 1, PCMI_ERR_INVALID, "%s: K = %d", who, K);
  PCMI_REQUIRE(K <= kMaxK, PCMI_ERR_UNSUPPORTED, "%s: K = %d, at most %d clusters per scene", who, K, kMaxK);
  PCMI_REQUIRE(max_rows >= 0, PCMI_ERR_INVALID, "%s: max_scene_rows = %lld", who, (long long)max_rows);
  PCMI_REQUIRE(max_rows <= kMaxSceneRows, PCMI_ERR_UNSUPPORTED, "%s: %lld rows per scene, at most %lld", who, (long long)max_rows,
               (long long)kMaxSceneRows);
  PCMI_REQUIRE(B >= 1 && B <= kMaxScenes, PCMI_ERR_UNSUPPORTED, "%s: %lld scenes, 1..%d are supported", who, (long long)B, kMaxScenes);
  PCMI_REQUIRE(n >= 0 && n < (1ll << 31) - 256 && offs && (n == 0 || feat), PCMI_ERR_INVALID, "%s: bad argument", who);
  PCMI_REQUIRE(ld >= c && ld % 4 == 0 && (uintptr_t)feat % 16 == 0, PCMI_ERR_INVALID,
               "%s: rows need a stride >= C that is a multiple of 4 floats, and a 16-byte aligned base", who);
  return PCMI_OK;
}

}  // namespace kmeans
}  // namespace pcmi

using namespace pcmi;
using namespace pcmi::kmeans;

extern "C" {

int pcmi_kmeans_init(const float* feat, int64_t ld, int64_t n, const int64_t* offs, int64_t B, int K, int c, int64_t max_scene_rows,
                     const int32_t* init_rows, float* centroid, int32_t* live, int64_t* flags, pcmi_stream_t stream) {
  const int rc = check_common("kmeans_init", feat, ld, n, offs, B, K, c, max_scene_rows);
  if (rc != PCMI_OK) return rc;
  PCMI_REQUIRE(init_rows && centroid && live && flags && init_rows != live, PCMI_ERR_INVALID, "kmeans_init: null or aliased pointer");
  hipStream_t st = as_stream(stream);
  PCMI_HIP_CHECK(hipMemsetAsync(flags, 0, (size_t)B * 8, st));
  km_init_kernel<<<(unsigned)ceil_div(B * K, kThreads), kThreads, 0, st>>>(feat, ld, n, offs, (int)B, K, c, max_scene_rows, init_rows, centroid,
                                                                          live, reinterpret_cast<unsigned long long*>(flags));
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

int pcmi_kmeans_step(const float* feat, int64_t ld, int64_t n, const int64_t* offs, int64_t B, int K, int c, int64_t max_scene_rows,
                     const float* centroid_in, const int32_t* live, const int32_t* assign_prev, int32_t* assign, int64_t* sum,
                     int32_t* cnt, float* centroid_out, int64_t* changed, int64_t* skipped, pcmi_stream_t stream) {
  const int rc = check_common("kmeans_step", feat, ld, n, offs, B, K, c, max_scene_rows);
  if (rc != PCMI_OK) return rc;
  PCMI_REQUIRE(centroid_in && live && sum && cnt && centroid_out && changed && skipped && (n == 0 || assign) && assign != assign_prev,
               PCMI_ERR_INVALID, "kmeans_step: null or aliased pointer");
  PCMI_REQUIRE((uintptr_t)centroid_in % 16 == 0, PCMI_ERR_INVALID, "kmeans_step: centroids need a 16-byte aligned base");
  hipStream_t st = as_stream(stream);
  PCMI_HIP_CHECK(hipMemsetAsync(sum, 0, (size_t)B * K * c * 8, st));
  PCMI_HIP_CHECK(hipMemsetAsync(cnt, 0, (size_t)B * K * 4, st));
  PCMI_HIP_CHECK(hipMemsetAsync(changed, 0, (size_t)B * 8, st));
  PCMI_HIP_CHECK(hipMemsetAsync(skipped, 0, (size_t)B * 8, st));
  if (n > 0) {
    km_fill_kernel<<<(unsigned)ceil_div(n, kThreads), kThreads, 0, st>>>(assign, nullptr, n);
    PCMI_LAUNCH_CHECK();
    TileArgs a = {};
    a.feat = feat; a.ld = ld; a.n = n; a.offs = offs; a.K = K; a.nch = row_chunks(n, B); a.max_rows = max_scene_rows;
    a.centroid = centroid_in; a.live = live; a.assign_prev = assign_prev; a.assign = assign;
    a.sum = reinterpret_cast<unsigned long long*>(sum); a.cnt = cnt;
    a.changed = reinterpret_cast<unsigned long long*>(changed); a.skipped = reinterpret_cast<unsigned long long*>(skipped);
    a.lds_acc = tile_static_lds(c) + acc_lds(K, c) <= kLdsBudget ? 1 : 0;
    const int r2 = dispatch_tile<false>(c, dim3((unsigned)B, (unsigned)a.nch), a.lds_acc ? acc_lds(K, c) : 0, st, a);
    if (r2 != PCMI_OK) return r2;
  }
  const int64_t total = B * K * c;
  km_centroid_kernel<<<(unsigned)ceil_div(total, kThreads), kThreads, 0, st>>>(reinterpret_cast<const long long*>(sum), cnt, live, centroid_in,
                                                                              centroid_out, total, c);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

struct AssignWs { unsigned long long* near; double* part; size_t bytes; };
static AssignWs assign_ws(void* ws, int64_t B, int K) {
  Carve cv{(char*)ws};
  AssignWs w;
  w.near = cv.take<unsigned long long>((size_t)B * K);
  cv.align = 1;  // the last piece is not padded
  w.part = cv.take<double>((size_t)B * kParts);
  w.bytes = cv.used;
  return w;
}

size_t pcmi_kmeans_assign_workspace_bytes(int64_t B, int K) { return B < 1 || K < 1 ? 0 : assign_ws(nullptr, B, K).bytes; }

int pcmi_kmeans_assign(const float* feat, int64_t ld, int64_t n, const int64_t* offs, int64_t B, int K, int c, int64_t max_scene_rows,
                       const float* centroid, const int32_t* live, int32_t* assign, float* d2, int32_t* nearest, double* inertia,
                       int32_t* cnt, int64_t* skipped, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  const int rc = check_common("kmeans_assign", feat, ld, n, offs, B, K, c, max_scene_rows);
  if (rc != PCMI_OK) return rc;
  PCMI_REQUIRE(centroid && live && nearest && inertia && cnt && skipped && (n == 0 || (assign && d2)), PCMI_ERR_INVALID,
               "kmeans_assign: null pointer");
  PCMI_REQUIRE((uintptr_t)centroid % 16 == 0, PCMI_ERR_INVALID, "kmeans_assign: centroids need a 16-byte aligned base");
  if (int ws_rc = require_ws("kmeans_assign", ws, ws_bytes, assign_ws(nullptr, B, K).bytes, 8)) return ws_rc;
  hipStream_t st = as_stream(stream);
  const AssignWs w = assign_ws(ws, B, K);
  PCMI_HIP_CHECK(hipMemsetAsync(w.near, 0xff, (size_t)B * K * 8, st));
  PCMI_HIP_CHECK(hipMemsetAsync(cnt, 0, (size_t)B * K * 4, st));
  PCMI_HIP_CHECK(hipMemsetAsync(skipped, 0, (size_t)B * 8, st));
  if (n > 0) {
    km_fill_kernel<<<(unsigned)ceil_div(n, kThreads), kThreads, 0, st>>>(assign, d2, n);
    PCMI_LAUNCH_CHECK();
    TileArgs a = {};
    a.feat = feat; a.ld = ld; a.n = n; a.offs = offs; a.K = K; a.nch = row_chunks(n, B); a.max_rows = max_scene_rows;
    a.centroid = centroid; a.live = live; a.assign = assign; a.d2 = d2; a.cnt = cnt;
    a.skipped = reinterpret_cast<unsigned long long*>(skipped); a.near = w.near;
    const int r2 = dispatch_tile<true>(c, dim3((unsigned)B, (unsigned)a.nch), 0, st, a);
    if (r2 != PCMI_OK) return r2;
    km_inertia_partial_kernel<<<dim3(kPartBlocks, (unsigned)B), kThreads, 0, st>>>(assign, d2, n, offs, max_scene_rows, w.part);
    PCMI_LAUNCH_CHECK();
  }
  km_final_kernel<<<(unsigned)B, kThreads, 0, st>>>(w.part, n, offs, max_scene_rows, K, w.near, inertia, nearest);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

struct SeedWs { unsigned long long* tot; int32_t* firstc; size_t bytes; };
static SeedWs seed_ws(void* ws, int64_t B) {
  Carve cv{(char*)ws, 1};  // packed: the 8-byte array, then the 4-byte one
  SeedWs w;
  w.tot = cv.take<unsigned long long>((size_t)B * kSeedChunks);
  w.firstc = cv.take<int32_t>((size_t)B * kSeedChunks);
  w.bytes = cv.used;
  return w;
}

size_t pcmi_kmeans_pp_step_workspace_bytes(int64_t B) { return B < 1 ? 0 : seed_ws(nullptr, B).bytes; }

int pcmi_kmeans_pp_step(const float* feat, int64_t ld, int64_t n, const int64_t* offs, int64_t B, int c, int64_t max_scene_rows,
                        const int32_t* last, const uint64_t* draw, float* mind2, int32_t* next, void* ws, size_t ws_bytes,
                        pcmi_stream_t stream) {
  const int rc = check_common("kmeans_pp_step", feat, ld, n, offs, B, 1, c, max_scene_rows);
  if (rc != PCMI_OK) return rc;
  PCMI_REQUIRE(draw && next && (n == 0 || mind2), PCMI_ERR_INVALID, "kmeans_pp_step: null pointer");
  PCMI_REQUIRE(n < kNoRow, PCMI_ERR_UNSUPPORTED, "kmeans_pp_step: %lld rows, fewer than %d are supported", (long long)n, kNoRow);
  if (int ws_rc = require_ws("kmeans_pp_step", ws, ws_bytes, seed_ws(nullptr, B).bytes, 8)) return ws_rc;
  hipStream_t st = as_stream(stream);
  const SeedWs w = seed_ws(ws, B);
  PCMI_HIP_CHECK(hipMemsetAsync(w.tot, 0, (size_t)B * kSeedChunks * 8, st));
  PCMI_HIP_CHECK(hipMemsetAsync(w.firstc, 0x7f, (size_t)B * kSeedChunks * 4, st));
  const int slabs = (int)std::min<int64_t>(kMaxSceneRows / kThreads, ceil_div(std::max<int64_t>(std::min(n, max_scene_rows), 1), kThreads));  // no scene has more
  km_seed_weights_kernel<<<dim3((unsigned)slabs, (unsigned)B), kThreads, 0, st>>>(feat, ld, n, offs, c, max_scene_rows, last, mind2, w.tot, w.firstc);
  PCMI_LAUNCH_CHECK();
  km_seed_pick_kernel<<<(unsigned)B, kThreads, 0, st>>>(feat, ld, n, offs, c, max_scene_rows, mind2, w.tot, w.firstc,
                                                       reinterpret_cast<const unsigned long long*>(draw), next);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

}  // extern "C"
