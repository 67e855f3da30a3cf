// Instance masks scored by the protocol of ScanNet's benchmark (evaluate_semantic_instance.py) as include/pcmi.h restates it
// -- restated from the script's rules, never run against the script: the void overlap of the predictions, the matching per
// (threshold, scene, class) with the script's claim rule, and the average precision in its convolution form.  The overlap
// matrix itself is pcmi_instance_overlap's (cluster.hip).  gfx950, wave64.
//
// Arithmetic: every fp64 quotient, product and sum is one round-to-nearest operation in the order include/pcmi.h states (no
// FMA contraction); the only atomics are integer adds, no workgroup waits for another, every output is the same bits from
// run to run.
//
// Who does what.
//   iv_count_kernel   one lane per row; a wave whose rows agree adds once (rows of one instance stand together).
//   ib_match_kernel   ONE WAVE per unit (threshold t, scene b, class c), four units per workgroup, no barrier.  Lane l owns the
//                     predictions p = l, l + 64, ...: every byte of entry_flag [t, p, :] is read and written by that one lane
//                     only, so the walk needs no memory ordering between lanes.  The unit's ground truths are walked in
//                     ascending g by the whole wave (gt_scene / gt_class are wave-uniform loads); per counted g the lanes
//                     test their predictions, write a tentative false positive for each claimant, and two butterflies give
//                     the first claimant (lowest p) and the best one (highest score, lowest p).  While the walk runs a flag
//                     carries two more bits of state: +2 marks "this claim made p visited"; the closing pass over the unit's
//                     predictions strips it and adds the unmatched false positives.
//   ib_ap_kernel      one workgroup of 256 per (class, threshold).  Pass A walks the class's entries in blocks of 1024 with
//                     carries (the last valid score, the counts): a maximum scan finds each entry's previous VALID entry, so
//                     flags of -1 may stand anywhere and a group of equal scores may straddle blocks; each group start writes
//                     the counts in front of it as curve point j.  Pass B forms the terms of 1024 points at a time in LDS and
//                     lane 0 adds them in ascending j: the sum is sequential by definition.
#include <algorithm>

#include "blockscan.h"
#include "exact.h"
#include "internal.h"

#pragma clang fp contract(off)

namespace pcmi {
namespace insbench {

constexpr int kThreads = 256;  // 4 waves: one per SIMD of a CU
constexpr int kWaves = kThreads / 64;
constexpr int kMaxThresholds = 16;
constexpr int kSlots = 3;  // entries per prediction and threshold: fewer than 1 / 0.25 claims
constexpr int kMaxClasses = 64;
constexpr int64_t kMaxScenes = 65535;
constexpr int kApItems = 4, kApChunk = kThreads * kApItems;

struct Thresholds {
  double t[kMaxThresholds];
};

// ---- void overlap -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void iv_count_kernel(const int32_t* __restrict__ pred, const int32_t* __restrict__ gt,
                                                            const int32_t* __restrict__ gt_valid, int64_t n, int64_t P, int64_t G,
                                                            int32_t* void_inter) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int32_t p = pred[i], g = gt[i];
  const bool is_void = !(g >= 0 && g < G) || gt_valid[g] == 0;
  const int32_t key = (p >= 0 && p < P && is_void) ? p : -1;  // -1: the row adds nothing
  const unsigned long long act = __ballot(1);
  const int leader = __ffsll((long long)act) - 1;
  int add = 1;
  if (__ballot(key == __shfl(key, leader, 64)) == act) {
    if ((int)(threadIdx.x & 63) != leader) return;
    add = __popcll(act);
  }
  if (key >= 0) atomicAdd(&void_inter[key], add);
}

// ---- matching -----------------------------------------------------------------------------------------------------------------
struct MatchArgs {
  const int32_t* inter;
  const int32_t* pred_size;
  const int32_t* gt_size;
  const int32_t* void_inter;
  const int32_t* pred_scene;
  const int32_t* pred_class;
  const double* pred_score;
  const int32_t* gt_scene;
  const int32_t* gt_class;
  int64_t P, G;
  int B, Cls, T, min_region;
  int8_t* entry_flag;
  int32_t* gt_state;
  int32_t* npos;
};

__device__ inline int wave_min(int v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v = min(v, __shfl_xor(v, d, 64));
  return v;
}

__global__ __launch_bounds__(kThreads) void ib_match_kernel(MatchArgs a, Thresholds thr) {
  const int lane = threadIdx.x & 63;
  const int64_t unit = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  const int64_t per_t = (int64_t)a.B * a.Cls;
  if (unit >= per_t * a.T) return;  // a whole wave leaves: there is no barrier below
  const int t = (int)(unit / per_t), b = (int)((unit % per_t) / a.Cls), c = (int)(unit % a.Cls);
  const double th = thr.t[t];
  const int64_t P = a.P, G = a.G;
  int8_t* const flags = a.entry_flag + (int64_t)t * P * kSlots;
  int32_t* const state = a.gt_state + (int64_t)t * G;
  const double minus_inf = -pinf();

  int counted = 0;
  for (int64_t g = 0; g < G; ++g) {
    if (a.gt_scene[g] != b || a.gt_class[g] != c) continue;
    const int64_t gs = a.gt_size[g];
    if (gs < a.min_region) continue;  // a small ground truth: not counted, its state stays -1
    ++counted;
    // the claimants of g: each writes a tentative false positive into its next free slot
    double best_s = minus_inf;
    int best_p = INT32_MAX, first_p = INT32_MAX;
    for (int64_t base = 0; base < P; base += 64) {
      const int64_t p = base + lane;
      if (p >= P || a.pred_scene[p] != b || a.pred_class[p] != c) continue;
      const int64_t ps = a.pred_size[p], it = a.inter[p * G + g], un = gs + ps - it;
      if (ps < a.min_region || it <= 0 || un <= 0) continue;
      int8_t* f = flags + p * kSlots;
      const int f0 = f[0], f1 = f[1], f2 = f[2];
      // visited, or three entries already (which overlaps counted by pcmi_instance_overlap cannot produce)
      if (f0 >= 2 || f1 >= 2 || f2 >= 0) continue;
      if (!(div_rn((double)it, (double)un) > th)) continue;
      f[f0 < 0 ? 0 : (f1 < 0 ? 1 : 2)] = 0;
      const double s = a.pred_score[p];
      if (s > best_s || (s == best_s && (int)p < best_p)) {
        best_s = s;
        best_p = (int)p;
      }
      first_p = min(first_p, (int)p);
    }
    first_p = wave_min(first_p);
    if (first_p == INT32_MAX) {
      if (lane == 0) state[g] = 0;
      continue;
    }
    if (lane == 0) state[g] = 1;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const double os = __shfl_xor(best_s, d, 64);
      const int op = __shfl_xor(best_p, d, 64);
      if (os > best_s || (os == best_s && op < best_p)) {
        best_s = os;
        best_p = op;
      }
    }
    // the entry just written is the last used slot of its prediction
    if (best_p != INT32_MAX && (best_p & 63) == lane) {  // (a claim whose scores are all NaN has no best)
      int8_t* f = flags + (int64_t)best_p * kSlots;
      const int s = f[2] >= 0 ? 2 : (f[1] >= 0 ? 1 : 0);
      f[s] = (int8_t)(f[s] | 1);
    }
    if ((first_p & 63) == lane) {
      int8_t* f = flags + (int64_t)first_p * kSlots;
      const int s = f[2] >= 0 ? 2 : (f[1] >= 0 ? 1 : 0);
      f[s] = (int8_t)(f[s] | 2);
    }
  }
  if (t == 0 && lane == 0 && counted > 0) atomicAdd(&a.npos[c], counted);

  // the closing pass: strip the walk's state; a prediction without any ground truth above the threshold is a false
  // positive unless it lies mostly on void and on small ground truths
  for (int64_t base = 0; base < P; base += 64) {
    const int64_t p = base + lane;
    const bool mine = p < P && a.pred_scene[p] == b && a.pred_class[p] == c && a.pred_size[p] >= a.min_region;
    if (__ballot(mine) == 0) continue;  // wave-uniform
    const int64_t ps = mine ? a.pred_size[p] : 1;
    bool matched = false;
    int64_t ignore = mine ? a.void_inter[p] : 0;
    for (int64_t g = 0; g < G; ++g) {
      if (a.gt_scene[g] != b || a.gt_class[g] != c) continue;  // wave-uniform
      if (!mine) continue;
      const int64_t gs = a.gt_size[g], it = a.inter[p * G + g], un = gs + ps - it;
      if (it <= 0 || un <= 0) continue;
      if (div_rn((double)it, (double)un) > th) matched = true;
      if (gs < a.min_region) ignore += it;
    }
    if (!mine) continue;
    int8_t* f = flags + p * kSlots;
    if (!matched) {
      if (div_rn((double)ignore, (double)ps) <= th) f[0] = 0;
      continue;
    }
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
      const int v = f[s];
      if (v >= 2) f[s] = (int8_t)(v & 1);
    }
  }
}

// ---- average precision ----------------------------------------------------------------------------------------------------------
// Curve point j = (tp, n): the true positives and the entries of the groups 1 .. j.  P_j = tp / n (1 for j = 0), R_j = tp / npos.
__device__ inline double ap_prec(int tp, int n) { return n > 0 ? div_rn((double)tp, (double)n) : 1.0; }

__global__ __launch_bounds__(kThreads) void ib_ap_kernel(const int8_t* __restrict__ entry_flag, const double* __restrict__ score,
                                                         const int32_t* __restrict__ cls_offs, const int32_t* __restrict__ npos, int64_t E,
                                                         int Cls, int32_t* pts, double* __restrict__ ap, double* prec, double* rec) {
  __shared__ int s_int[kWaves];
  __shared__ unsigned long long s_u64[kWaves];
  __shared__ double s_term[kApChunk];
  const int c = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
  const int64_t start = min(max((int64_t)cls_offs[c], (int64_t)0), E), end = min(max((int64_t)cls_offs[c + 1], start), E);
  const int64_t n = end - start;
  const int32_t np_i = npos[c];
  if (np_i <= 0) {  // uniform
    if (tid == 0) ap[(int64_t)t * Cls + c] = qnan();
    return;
  }
  const double np = (double)np_i;
  const int8_t* fl = entry_flag + (int64_t)t * E + start;
  const double* sc = score + start;
  const int64_t row = (int64_t)t * E + start;
  // the points of this class and threshold: n + 1 pairs of int32 behind those of the classes before it
  int32_t* pt = pts + 2 * ((int64_t)t * (E + Cls) + start + c);

  // pass A
  int64_t c_prev = -1;  // the last valid entry of the blocks before (an index into the class), -1: none
  double c_score = 0.0;
  int c_tp = 0, c_n = 0, c_groups = 0;
  for (int64_t base = 0; base < n; base += kApChunk) {
    int f[kApItems];
    double s[kApItems];
    int last = 0;  // this thread's last valid item as its position in the block + 1
#pragma unroll
    for (int q = 0; q < kApItems; ++q) {
      const int64_t i = base + (int64_t)tid * kApItems + q;
      f[q] = i < n ? (int)fl[i] : -1;
      s[q] = (i < n && f[q] >= 0) ? sc[i] : 0.0;
      if (f[q] >= 0) last = tid * kApItems + q + 1;
    }
    int all;
    const int before = block_scan_max_excl<kWaves>(last, s_int, &all);
    int64_t prev = before > 0 ? base + before - 1 : c_prev;
    double prev_s = before > 0 ? sc[base + before - 1] : c_score;
    bool st[kApItems];
    int64_t pv[kApItems];
    unsigned long long local = 0;
#pragma unroll
    for (int q = 0; q < kApItems; ++q) {
      st[q] = false;
      pv[q] = prev;
      if (f[q] < 0) continue;
      st[q] = prev < 0 || s[q] != prev_s;
      local += (unsigned long long)(f[q] > 0) | (1ull << 20) | ((unsigned long long)st[q] << 40);
      prev = base + (int64_t)tid * kApItems + q;
      prev_s = s[q];
    }
    unsigned long long total;
    const unsigned long long excl = block_scan_add64<kWaves>(local, s_u64, &total) - local;
    int tp = c_tp + (int)(excl & 0xfffff), cnt = c_n + (int)((excl >> 20) & 0xfffff), groups = c_groups + (int)(excl >> 40);
#pragma unroll
    for (int q = 0; q < kApItems; ++q) {
      if (f[q] < 0) continue;
      if (st[q]) {  // group `groups` + 1 starts here: point `groups` is what stands in front of it
        pt[2 * (int64_t)groups] = tp;
        pt[2 * (int64_t)groups + 1] = cnt;
        if (pv[q] >= 0) {  // ... and the previous valid entry was the last of its group
          if (prec) prec[row + pv[q]] = ap_prec(tp, cnt);
          if (rec) rec[row + pv[q]] = div_rn((double)tp, np);
        }
        ++groups;
      }
      tp += f[q] > 0;
      ++cnt;
    }
    if (all > 0) {
      c_prev = base + all - 1;
      c_score = sc[c_prev];
    }
    c_tp += (int)(total & 0xfffff);
    c_n += (int)((total >> 20) & 0xfffff);
    c_groups += (int)(total >> 40);
  }
  const int64_t m = c_groups;  // groups; the points are 0 .. m
  if (tid == 0) {
    pt[2 * m] = c_tp;
    pt[2 * m + 1] = c_n;
    if (c_prev >= 0) {
      if (prec) prec[row + c_prev] = ap_prec(c_tp, c_n);
      if (rec) rec[row + c_prev] = div_rn((double)c_tp, np);
    }
  }
  __syncthreads();  // the points are read back below by other threads of the workgroup

  // pass B: ap = sum over j = 0 .. m of P_j (0.5 (R_{j+1} - R_{j-1})), R_{-1} = 0, R_{m+1} = R_m, in ascending j
  double sum = 0.0;
  for (int64_t base = 0; base <= m; base += kApChunk) {
#pragma unroll
    for (int q = 0; q < kApItems; ++q) {
      const int64_t j = base + tid + (int64_t)q * kThreads;
      double term = 0.0;
      if (j <= m) {
        const double r_prev = j > 0 ? div_rn((double)pt[2 * (j - 1)], np) : 0.0;
        const double r_next = div_rn((double)pt[2 * min(j + 1, m)], np);
        term = mul_rn(ap_prec(pt[2 * j], pt[2 * j + 1]), mul_rn(0.5, add_rn(r_next, -r_prev)));
      }
      s_term[tid + q * kThreads] = term;
    }
    __syncthreads();
    if (tid == 0) {
      const int k = (int)min((int64_t)kApChunk, m + 1 - base);
      for (int j = 0; j < k; ++j) sum = add_rn(sum, s_term[j]);
    }
    __syncthreads();
  }
  if (tid == 0) ap[(int64_t)t * Cls + c] = sum;
}

static bool match_shape_ok(int64_t P, int64_t G, int64_t B, int Cls, int T) {
  return P >= 0 && G >= 0 && P < (1ll << 31) && G < (1ll << 31) && P * G < (1ll << 31) && B >= 1 && B <= kMaxScenes && Cls >= 1 &&
         Cls <= kMaxClasses && T >= 1 && T <= kMaxThresholds && P * kSlots < (1ll << 31);
}
static bool ap_shape_ok(int64_t E, int Cls, int T) {
  return E >= 0 && E < (1ll << 20) * 1024 && Cls >= 1 && Cls <= kMaxClasses && T >= 1 && T <= kMaxThresholds;
}

}  // namespace insbench
}  // namespace pcmi

using namespace pcmi;
using namespace pcmi::insbench;

extern "C" {

int pcmi_instance_void_overlap(const int32_t* pred_inst, const int32_t* gt_inst, const int32_t* gt_valid, int64_t n, int64_t P, int64_t G,
                               int32_t* void_inter, pcmi_stream_t stream) {
  PCMI_REQUIRE(n >= 0 && n < (1ll << 31) && P >= 0 && G >= 0 && P < (1ll << 31) && G < (1ll << 31), PCMI_ERR_INVALID,
               "instance_void_overlap: bad shape (n %lld, P %lld, G %lld)", (long long)n, (long long)P, (long long)G);
  if (P == 0) return PCMI_OK;
  PCMI_REQUIRE(void_inter && (G == 0 || gt_valid) && (n == 0 || (pred_inst && gt_inst)), PCMI_ERR_INVALID,
               "instance_void_overlap: null pointer");
  hipStream_t st = as_stream(stream);
  PCMI_HIP_CHECK(hipMemsetAsync(void_inter, 0, (size_t)P * 4, st));
  if (n > 0) {
    iv_count_kernel<<<(unsigned)ceil_div(n, kThreads), kThreads, 0, st>>>(pred_inst, gt_inst, gt_valid, n, P, G, void_inter);
    PCMI_LAUNCH_CHECK();
  }
  return PCMI_OK;
}

int pcmi_instance_bench_match(const int32_t* inter, const int32_t* pred_size, const int32_t* gt_size, const int32_t* void_inter,
                              const int32_t* pred_scene, const int32_t* pred_class, const double* pred_score, const int32_t* gt_scene,
                              const int32_t* gt_class, int64_t P, int64_t G, int64_t B, int Cls, int min_region, const double* thresholds,
                              int n_thresholds, int8_t* entry_flag, int32_t* gt_state, int32_t* npos, pcmi_stream_t stream) {
  PCMI_REQUIRE(match_shape_ok(P, G, B, Cls, n_thresholds) && min_region >= 1, PCMI_ERR_INVALID,
               "instance_bench_match: bad shape (P %lld, G %lld, P G < 2^31; 1 <= B %lld <= 65535; 1 <= Cls %d <= %d; 1 <= %d thresholds "
               "<= %d; min_region %d >= 1)",
               (long long)P, (long long)G, (long long)B, Cls, kMaxClasses, n_thresholds, kMaxThresholds, min_region);
  PCMI_REQUIRE(thresholds, PCMI_ERR_INVALID, "instance_bench_match: null pointer");
  Thresholds thr;
  for (int t = 0; t < kMaxThresholds; ++t) {
    thr.t[t] = t < n_thresholds ? thresholds[t] : 0.5;
    PCMI_REQUIRE(thr.t[t] >= 0.25 && thr.t[t] < 1.0, PCMI_ERR_INVALID, "instance_bench_match: threshold %d = %g outside [0.25, 1)", t,
                 thr.t[t]);
  }
  PCMI_REQUIRE(npos && (P == 0 || (entry_flag && pred_size && void_inter && pred_scene && pred_class && pred_score)) &&
                   (G == 0 || (gt_state && gt_size && gt_scene && gt_class)) && (P * G == 0 || inter),
               PCMI_ERR_INVALID, "instance_bench_match: null pointer");
  hipStream_t st = as_stream(stream);
  const int T = n_thresholds;
  if (P > 0) PCMI_HIP_CHECK(hipMemsetAsync(entry_flag, 0xff, (size_t)T * (size_t)P * kSlots, st));
  if (G > 0) PCMI_HIP_CHECK(hipMemsetAsync(gt_state, 0xff, (size_t)T * (size_t)G * 4, st));
  if (P == 0 && G == 0) return PCMI_OK;
  MatchArgs a{inter, pred_size, gt_size, void_inter, pred_scene, pred_class, pred_score, gt_scene, gt_class, P,
              G,     (int)B,    Cls,     T,          min_region, entry_flag, gt_state,   npos};
  const int64_t units = (int64_t)T * B * Cls;
  ib_match_kernel<<<(unsigned)ceil_div(units, kWaves), kThreads, 0, st>>>(a, thr);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

size_t pcmi_instance_bench_ap_workspace_bytes(int64_t E, int Cls, int n_thresholds) {
  if (!ap_shape_ok(E, Cls, n_thresholds)) return 0;
  return align_up((size_t)n_thresholds * (size_t)(E + Cls) * 8, 256);
}

int pcmi_instance_bench_ap(const int8_t* entry_flag, const double* score, const int32_t* cls_offs, const int32_t* npos, int64_t E, int Cls,
                           int n_thresholds, double* ap, double* prec, double* rec, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_REQUIRE(ap_shape_ok(E, Cls, n_thresholds), PCMI_ERR_INVALID, "instance_bench_ap: bad shape (E %lld < 2^30, 1 <= Cls %d <= %d, 1 <= %d "
               "thresholds <= %d)", (long long)E, Cls, kMaxClasses, n_thresholds, kMaxThresholds);
  PCMI_REQUIRE(cls_offs && npos && ap && (E == 0 || (entry_flag && score)), PCMI_ERR_INVALID, "instance_bench_ap: null pointer");
  if (int rc = require_ws("instance_bench_ap", ws, ws_bytes, pcmi_instance_bench_ap_workspace_bytes(E, Cls, n_thresholds), 4)) return rc;
  hipStream_t st = as_stream(stream);
  const size_t curve = (size_t)n_thresholds * (size_t)E * 8;
  if (prec && curve) PCMI_HIP_CHECK(hipMemsetAsync(prec, 0xff, curve, st));  // NaN wherever no group ends
  if (rec && curve) PCMI_HIP_CHECK(hipMemsetAsync(rec, 0xff, curve, st));
  ib_ap_kernel<<<dim3((unsigned)Cls, (unsigned)n_thresholds), kThreads, 0, st>>>(entry_flag, score, cls_offs, npos, E, Cls, static_cast<int32_t*>(ws), ap,
                                                                                 prec, rec);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

}  // extern "C"
