// Dual-set instance proposals (PointGroup's second half): overlapping proposals as a membership matrix member [n, S], the
// pairwise intersections of the proposals of a scene, and the non-maximum suppression on mask IoU that removes the duplicates
// of the union of the sets.  Written from the semantics in include/pcmi.h; gfx950, wave64.
//
// PointGroup takes the intersections from a dense [proposals, points] float matrix times its transpose; with 8192 slots and
// 1.2 M rows that matrix cannot be built.  Here one lane per row adds its (at most 6) pairs into a [Kmax, Kmax] table per
// scene, addressed by the proposal's index inside its scene.
//
// Arithmetic: integer atomics only (sums), one fp64 division per tested pair (div_rn, no contraction); no output depends on the
// order in which the atomics land.
#include <algorithm>

#include "blockscan.h"
#include "exact.h"
#include "internal.h"

#pragma clang fp contract(off)

namespace pcmi {
namespace proposals {

using u64 = unsigned long long;

constexpr int kThreads = 256;  // 4 waves: one per SIMD of a CU
constexpr int kWaves = kThreads / 64;
constexpr int kMaxSets = 4;
constexpr int kMaxK = 1024;        // proposals of one scene: Kmax x Kmax suppression bits are 128 KiB of LDS
constexpr int kLocalBits = 10;     // code = scene << 10 | local, -1: the proposal is counted nowhere
constexpr int64_t kMaxScenes = 65535;

static inline unsigned grid_for(int64_t n) { return (unsigned)ceil_div(std::max<int64_t>(n, 1), kThreads); }

__global__ __launch_bounds__(kThreads) void po_init_kernel(int64_t P, int32_t* __restrict__ size, int32_t* __restrict__ local,
                                                           int32_t* __restrict__ code) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= P) return;
  size[p] = 0;
  local[p] = -1;
  code[p] = -1;
}

// One workgroup per scene numbers that scene's slots in ascending slot order: a block scan per 256 slots with a carry.
// local / code hold -1 everywhere before the launch; a slot belongs to at most one scene, so nobody writes the same entry.
__global__ __launch_bounds__(kThreads) void po_local_kernel(const int32_t* __restrict__ prop_scene, int64_t P, int Kmax,
                                                            int32_t* __restrict__ local, int32_t* __restrict__ code,
                                                            int32_t* __restrict__ scene_count, u64* dropped) {
  __shared__ int s_wave[kWaves];
  const int b = blockIdx.x;
  int carry = 0;
  for (int64_t base = 0; base < P; base += kThreads) {  // (uniform bounds: every thread scans)
    const int64_t p = base + threadIdx.x;
    const int f = (p < P && prop_scene[p] == b) ? 1 : 0;
    int total;
    const int incl = block_scan_add<kWaves>(f, s_wave, &total);
    if (f) {
      const int l = carry + incl - 1;
      if (l < Kmax) {
        local[p] = l;
        code[p] = (b << kLocalBits) | l;
      }
    }
    carry += total;
  }
  if (threadIdx.x == 0) {
    scene_count[b] = carry;
    if (carry > Kmax && dropped) atomicAdd(dropped, (u64)(carry - Kmax));
  }
}

// One lane per row.  With a trained network the P-cluster and the Q-cluster of one object share thousands of consecutive rows,
// so the lanes of a wave mostly hold ONE value per column: the wave's first active lane then adds the lane count
// (io_count_kernel's aggregation, per column and per pair of columns).  A wave whose values differ adds lane by lane.
template <int S>
__global__ __launch_bounds__(kThreads) void po_count_kernel(const int32_t* __restrict__ member, int64_t ld, int64_t n, int64_t P,
                                                            const int32_t* __restrict__ code, int Kmax, int32_t* size, int32_t* inter) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int lane = threadIdx.x & 63;
  const u64 act = __ballot(1);
  const int leader = __ffsll((long long)act) - 1;
  const int cnt = __popcll(act);
  int32_t m[S], cd[S];
  bool uni[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int32_t v = member[i * ld + s];
    const bool ok = v >= 0 && v < P;
    m[s] = ok ? v : -1;
    cd[s] = ok ? code[v] : -1;
    uni[s] = __ballot(m[s] == __shfl(m[s], leader, 64)) == act;
  }
#pragma unroll
  for (int s = 0; s < S; ++s) {
    if (m[s] < 0) continue;
    if (!uni[s]) {
      atomicAdd(&size[m[s]], 1);
    } else if (lane == leader) {
      atomicAdd(&size[m[s]], cnt);
    }
  }
#pragma unroll
  for (int s = 0; s < S; ++s) {
#pragma unroll
    for (int t = s + 1; t < S; ++t) {
      const int32_t a = cd[s], c = cd[t];
      if (a < 0 || c < 0 || a == c || (a >> kLocalBits) != (c >> kLocalBits)) continue;
      const bool agg = uni[s] && uni[t];
      if (agg && lane != leader) continue;
      const int add = agg ? cnt : 1;
      const int64_t la = a & (kMaxK - 1), lc = c & (kMaxK - 1);  // both < Kmax: po_local_kernel
      int32_t* tab = inter + (int64_t)(a >> kLocalBits) * Kmax * Kmax;
      atomicAdd(&tab[la * Kmax + lc], add);
      atomicAdd(&tab[lc * Kmax + la], add);
    }
  }
}

// ---- non-maximum suppression on mask IoU ---------------------------------------------------------------------------------------
// box_nms_kernel's scheme (detect.hip): one workgroup per scene, the candidates ranked by counting, the suppression matrix as
// bits in LDS (rank r, word w: the ranks [64 w, 64 w + 64) that r suppresses), then ONE wave sweeps the ranks with 64 bits of
// the alive set per lane.
template <int KMAX>
struct NmsShared {
  u64 bits[KMAX * (KMAX / 64)];
  int32_t slot[KMAX];     // by index inside the scene: the proposal's slot, -1 none
  int32_t r_slot[KMAX];   // by rank
  int32_t r_size[KMAX];
  uint16_t r_local[KMAX];
  int n_valid;
};

template <int KMAX>
__global__ __launch_bounds__(KMAX) void pn_nms_kernel(const int32_t* __restrict__ inter, const int32_t* __restrict__ size,
                                                      const int32_t* __restrict__ local, const int32_t* __restrict__ scene_count,
                                                      const int32_t* __restrict__ prop_scene, const int32_t* __restrict__ prop_class,
                                                      const double* __restrict__ score, int64_t P, int Kmax, double thr, double min_score,
                                                      int32_t* __restrict__ keep) {
  __shared__ NmsShared<KMAX> sh;
  constexpr int W = KMAX / 64;
  const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.x;
  // the scores and the candidate flags sit in the matrix's memory while the ranks are taken
  double* s_score = reinterpret_cast<double*>(sh.bits);
  int* s_flag = reinterpret_cast<int*>(s_score + KMAX);
  sh.slot[tid] = -1;
  if (tid == 0) sh.n_valid = 0;
  __syncthreads();
  for (int64_t p = tid; p < P; p += KMAX) {
    if (prop_scene[p] != b) continue;
    const int l = local[p];
    if (l >= 0 && l < Kmax) sh.slot[l] = (int32_t)p;
  }
  __syncthreads();
  const int K = min(max(scene_count[b], 0), Kmax);
  const int32_t mine = sh.slot[tid];  // KMAX threads: at most one proposal per thread
  double s = 0.0;
  bool cand = false;
  if (tid < K && mine >= 0) {
    s = score[mine];
    cand = size[mine] >= 1 && prop_class[mine] >= 0 && isfinite(s) && s >= min_score;
  }
  s_score[tid] = s;
  s_flag[tid] = cand ? 1 : 0;
  __syncthreads();
  int my_rank = -1;
  if (cand) {  // every candidate's score is finite: the ranks are 0 .. n_valid - 1, each once
    int r = 0;
    for (int j = 0; j < K; ++j) {
      const double o = s_score[j];
      r += (s_flag[j] && (o > s || (o == s && j < tid))) ? 1 : 0;  // equal scores: the lower slot first
    }
    my_rank = r;
    atomicAdd(&sh.n_valid, 1);
  }
  __syncthreads();  // every reader of the scores is done: the matrix may be written
  const int nv = sh.n_valid;
  if (my_rank >= 0) {
    sh.r_slot[my_rank] = mine;
    sh.r_size[my_rank] = size[mine];
    sh.r_local[my_rank] = (uint16_t)tid;
  }
  __syncthreads();
  const int32_t* tab = inter + (int64_t)b * Kmax * Kmax;
  const int nw = (nv + 63) >> 6;  // words of a row that hold ranks
  for (int q = tid; q < nw * nv; q += KMAX) {
    const int w = q / nv, r = q - w * nv;
    const int64_t si = sh.r_size[r];
    const int32_t* row = tab + (int64_t)sh.r_local[r] * Kmax;
    u64 word = 0;
    const int c0 = w * 64;
    const int c1 = min(nv, c0 + 64);
    for (int c = max(c0, r + 1); c < c1; ++c) {
      const int64_t it = row[sh.r_local[c]];
      const double iou = div_rn((double)it, (double)(si + (int64_t)sh.r_size[c] - it));
      if (iou > thr) word |= 1ull << (c - c0);  // strict; a NaN suppresses nothing
    }
    sh.bits[r * W + w] = word;
  }
  __syncthreads();
  if (tid >= 64) return;
  // lane l holds the alive ranks [64 l, 64 l + 64)
  u64 alive = 0;
  if (lane < nw) {
    const int left = nv - lane * 64;
    alive = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
  }
  for (int w = 0; w < nw; ++w) {
    u64 a = __shfl(alive, w, 64);
    while (a) {
      const int bit = __ffsll((long long)a) - 1;
      const int r = w * 64 + bit;
      if (lane == 0) keep[sh.r_slot[r]] = 1;
      if (lane < nw) alive &= ~sh.bits[r * W + lane];
      a = __shfl(alive, w, 64);
      a &= bit == 63 ? 0ull : ~((2ull << bit) - 1ull);  // ranks above r only
    }
  }
}

static bool shape_ok(int64_t P, int64_t B, int Kmax) {
  return P >= 0 && P < (1ll << 31) && B >= 1 && B <= kMaxScenes && Kmax >= 1 && (Kmax > kMaxK || B * Kmax * Kmax < (1ll << 31));
}

}  // namespace proposals
}  // namespace pcmi

using namespace pcmi;
using namespace pcmi::proposals;

extern "C" {

size_t pcmi_proposal_overlap_workspace_bytes(int64_t P) {
  return P < 0 || P >= (1ll << 31) ? 0 : align_up((size_t)std::max<int64_t>(P, 1) * 4, 256);
}

int pcmi_proposal_overlap(const int32_t* member, int64_t ld, int64_t n, int S, const int32_t* prop_scene, int64_t P, int64_t B, int Kmax,
                          int32_t* size, int32_t* local, int32_t* scene_count, int32_t* inter, int64_t* dropped, void* ws,
                          size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_REQUIRE(shape_ok(P, B, Kmax) && n >= 0 && n < (1ll << 31) - kThreads && S >= 1 && S <= kMaxSets && ld >= S, PCMI_ERR_INVALID,
               "proposal_overlap: bad shape (n %lld, S %d in 1..%d, ld %lld >= S, P %lld, B %lld, Kmax %d; B Kmax^2 < 2^31)", (long long)n, S,
               kMaxSets, (long long)ld, (long long)P, (long long)B, Kmax);
  PCMI_REQUIRE(Kmax <= kMaxK, PCMI_ERR_UNSUPPORTED, "proposal_overlap: %d proposals per scene, at most %d are supported", Kmax, kMaxK);
  PCMI_REQUIRE(scene_count && inter && (P == 0 || (prop_scene && size && local)) && (n == 0 || member), PCMI_ERR_INVALID,
               "proposal_overlap: null pointer");
  if (int rc = require_ws("proposal_overlap", ws, ws_bytes, pcmi_proposal_overlap_workspace_bytes(P), 4)) return rc;
  hipStream_t st = as_stream(stream);
  int32_t* code = static_cast<int32_t*>(ws);
  PCMI_HIP_CHECK(hipMemsetAsync(inter, 0, (size_t)(B * Kmax * Kmax) * 4, st));
  if (P == 0) {
    PCMI_HIP_CHECK(hipMemsetAsync(scene_count, 0, (size_t)B * 4, st));
    return PCMI_OK;
  }
  po_init_kernel<<<grid_for(P), kThreads, 0, st>>>(P, size, local, code);
  PCMI_LAUNCH_CHECK();
  po_local_kernel<<<(unsigned)B, kThreads, 0, st>>>(prop_scene, P, Kmax, local, code, scene_count, reinterpret_cast<u64*>(dropped));
  PCMI_LAUNCH_CHECK();
  if (n > 0) {
    const unsigned grid = grid_for(n);
    switch (S) {
      case 1: po_count_kernel<1><<<grid, kThreads, 0, st>>>(member, ld, n, P, code, Kmax, size, inter); break;
      case 2: po_count_kernel<2><<<grid, kThreads, 0, st>>>(member, ld, n, P, code, Kmax, size, inter); break;
      case 3: po_count_kernel<3><<<grid, kThreads, 0, st>>>(member, ld, n, P, code, Kmax, size, inter); break;
      default: po_count_kernel<4><<<grid, kThreads, 0, st>>>(member, ld, n, P, code, Kmax, size, inter); break;
    }
    PCMI_LAUNCH_CHECK();
  }
  return PCMI_OK;
}

int pcmi_proposal_nms(const int32_t* inter, const int32_t* size, const int32_t* local, const int32_t* scene_count,
                      const int32_t* prop_scene, const int32_t* prop_class, const double* score, int64_t P, int64_t B, int Kmax,
                      double nms_iou, double min_score, int32_t* keep, pcmi_stream_t stream) {
  PCMI_REQUIRE(shape_ok(P, B, Kmax), PCMI_ERR_INVALID, "proposal_nms: bad shape (P %lld, B %lld, Kmax %d; B Kmax^2 < 2^31)", (long long)P,
               (long long)B, Kmax);
  PCMI_REQUIRE(Kmax <= kMaxK, PCMI_ERR_UNSUPPORTED, "proposal_nms: %d proposals per scene, at most %d are supported", Kmax, kMaxK);
  if (P == 0) return PCMI_OK;
  PCMI_REQUIRE(inter && size && local && scene_count && prop_scene && prop_class && score && keep, PCMI_ERR_INVALID,
               "proposal_nms: null pointer");
  hipStream_t st = as_stream(stream);
  PCMI_HIP_CHECK(hipMemsetAsync(keep, 0, (size_t)P * 4, st));
  if (Kmax <= 256) {
    pn_nms_kernel<256><<<(unsigned)B, 256, 0, st>>>(inter, size, local, scene_count, prop_scene, prop_class, score, P, Kmax, nms_iou, min_score,
                                                    keep);
  } else {
    pn_nms_kernel<1024><<<(unsigned)B, 1024, 0, st>>>(inter, size, local, scene_count, prop_scene, prop_class, score, P, Kmax, nms_iou,
                                                      min_score, keep);
  }
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

}  // extern "C"
