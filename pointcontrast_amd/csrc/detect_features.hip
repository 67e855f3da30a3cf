// The feature columns of VoteNet's detection input for a BATCH of scans, on the device: the height above the floor and the
// normalised colours that the reference adds per scan on the host in downstream/votenet_det_new --
//   * floor_height = np.percentile(point_cloud[:, 2], 0.99), height = z - floor_height
//                                  (lib/datasets/scannet/scannet_detection_dataset.py:90-93, sunrgbd_detection_dataset.py:97-100,147-148)
//   * (rgb - MEAN_COLOR_RGB) / 256 for ScanNet, rgb - 0.5 and the colour augmentation for SUN RGB-D
//                                  (scannet_detection_dataset.py:87-88, sunrgbd_detection_dataset.py:94-95,127-136)
// Written from the semantics in include/pcmi.h; gfx950, wave64.  Every random quantity is an input.
//
// pcmi_segment_quantile is an exact order statistic per scene: a radix select, eight bits a pass, over the order-preserving
// integer image of the floats.  Histograms live in LDS and are merged into the workspace with integer additions; the smallest
// value above the selected one is an integer minimum.  No float atomics: the result is the same bits from run to run.
// Arithmetic as detect_input.hip: every fp64 and fp32 operation is rounded on its own (no FMA contraction).
#include <algorithm>
#include <climits>

#include "exact.h"
#include "internal.h"

#pragma clang fp contract(off)

namespace pcmi {
namespace detfeat {

constexpr int kMaxScenes = 1023;          // as detect_input.hip
constexpr int64_t kMaxRows = 1ll << 29;
constexpr int kBins = 256;                // eight bits a pass, four passes
constexpr int kPasses = 4;
constexpr int kSingleThreads = 1024;      // one workgroup takes a whole scene of up to kSingleMax values
constexpr int kSingleMax = 16384;
constexpr int kChunkThreads = 256;        // larger scenes: one workgroup per chunk of kChunk values, one launch per pass
constexpr int kChunk = 8192;
constexpr int kSceneWords = kPasses * kBins + 4;  // per scene in ws: four histograms, the minimum above, the non-finite mark
constexpr int kThreads = 256;

struct QuantArgs {
  const float* values;
  int64_t stride;
  const int64_t* offs;
  int64_t n;
  int B;
  double q;
  double* out;
  float* stats;
  int32_t* flags;
  uint32_t* ws;
};

// the scene's rows [lo, lo + m); m = 0 for an empty scene and for offsets that are not 0 <= lo <= hi <= n
__device__ inline int64_t scene_rows(const QuantArgs& a, int b, int64_t* lo) {
  const int64_t l = a.offs[b], h = a.offs[b + 1];
  *lo = l;
  return (l >= 0 && h >= l && h <= a.n) ? h - l : 0;
}

// rank k = floor(v) and weight g = v - k of v = (m - 1) (q / 100), all in fp64
__device__ inline uint32_t rank_of(int64_t m, double q, double* g) {
  const double f = q / 100.0;
  const double v = (double)(m - 1) * f;
  double k = floor(v);
  if (k > (double)(m - 1)) k = (double)(m - 1);
  if (k < 0.0) k = 0.0;
  *g = v - k;
  return (uint32_t)k;
}

// One digit of the select, by the whole workgroup (>= 256 threads): the bin of hist [256] that holds rank `rank` among the
// values that carry `prefix`.  prefix takes the bin on, rank becomes the rank inside the bin, less grows by the values below
// it, count is the bin's size.  The caller guarantees rank < the histogram's sum.
__device__ inline void select_digit(const uint32_t* hist, uint32_t* s_wave, uint32_t* s_sel, uint32_t& prefix, uint32_t& rank,
                                    uint32_t& less, uint32_t& count) {
  const int t = threadIdx.x;
  uint32_t v = 0, incl = 0;
  if (t == 0) s_sel[0] = 0, s_sel[1] = 0, s_sel[2] = 0;
  if (t < kBins) {
    v = hist[t];
    incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = __shfl_up(incl, d, 64);
      if ((t & 63) >= d) incl += o;
    }
    if ((t & 63) == 63) s_wave[t >> 6] = incl;
  }
  __syncthreads();
  if (t < kBins) {
    for (int w = 0; w < (t >> 6); ++w) incl += s_wave[w];
    const uint32_t excl = incl - v;
    if (rank >= excl && rank < incl) s_sel[0] = (uint32_t)t, s_sel[1] = excl, s_sel[2] = v;
  }
  __syncthreads();
  const uint32_t bin = s_sel[0], excl = s_sel[1];
  count = s_sel[2];
  prefix = (prefix << 8) | bin;
  rank -= excl;
  less += excl;
  __syncthreads();
}

// hist[d] += 1 for every active lane.  Heights crowd into a few bins, and lanes that hit one LDS word take turns: twice, the
// lanes that share the first live lane's bin send one addition between them.  Every lane of the wave calls this.
__device__ inline void hist_add(uint32_t* hist, bool active, uint32_t d) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const unsigned long long live = __ballot(active);
    if (live == 0ull) return;
    const int leader = __ffsll((long long)live) - 1;
    const uint32_t d0 = __shfl(d, leader, 64);
    const bool same = active && d == d0;
    const unsigned long long mates = __ballot(same);
    if (lane == leader) atomicAdd(&hist[d0], (uint32_t)__popcll(mates));
    if (same) active = false;
  }
  if (active) atomicAdd(&hist[d], 1u);
}

// Pass p over rows [r0, r1) of the scene that starts at lo: the histogram of digit p of the values whose higher digits equal
// prefix.  Pass 0 marks non-finite values; the last pass keeps the smallest image whose upper 24 bits lie above the prefix.
__device__ inline void scan_rows(const QuantArgs& a, int64_t lo, int64_t r0, int64_t r1, int p, uint32_t prefix, uint32_t* s_hist,
                                 uint32_t* above, int* bad) {
  const int shift = 24 - 8 * p;
  for (int64_t base = r0; base < r1; base += blockDim.x) {
    const int64_t r = base + threadIdx.x;
    bool active = r < r1;
    uint32_t u = 0;
    if (active) {
      const float v = a.values[(lo + r) * a.stride];
      if (p == 0 && !isfinite(v)) *bad = 1;
      u = ord32(v);
      if (p > 0) {
        const uint32_t up = u >> (shift + 8);
        if (p == kPasses - 1 && up > prefix) *above = std::min(*above, u);
        active = up == prefix;
      }
    }
    hist_add(s_hist, active, (u >> shift) & 255u);
  }
}

// the answer from the selected image: lo = the value of rank k; hi = the same value while rank k + 1 lies inside its run of
// `count` equal values that starts at rank `less`, the smallest larger value otherwise
__device__ inline void write_result(const QuantArgs& a, int b, int64_t m, uint32_t k, double g, uint32_t image, uint32_t less, uint32_t count,
                                    uint32_t next, bool bad) {
  float lo = 0.f, hi = 0.f;
  double r = 0.0;
  if (bad) {
    atomicOr(&a.flags[b], PCMI_DET_FLAG_FEATURE);
  } else {
    const uint32_t k1 = std::min<uint32_t>(k + 1, (uint32_t)(m - 1));
    lo = unord32(image);
    hi = k1 < less + count ? lo : unord32(next);
    if (lo == 0.f) lo = 0.f;
    if (hi == 0.f) hi = 0.f;
    const double d = (double)hi - (double)lo;
    const double w = d * g;
    r = (double)lo + w;
    if (r == 0.0) r = 0.0;
  }
  a.out[b] = r;
  if (a.stats) a.stats[2 * b] = lo, a.stats[2 * b + 1] = hi;
}

// the smallest image above `image` among the values that share its upper 24 bits, from the last pass's histogram; UINT_MAX if none
__device__ inline void next_in_hist(const uint32_t* hist, uint32_t image, uint32_t* s_next) {
  const int t = threadIdx.x;
  if (t < kBins && (uint32_t)t > (image & 255u) && hist[t] != 0u) atomicMin(s_next, (image & ~255u) | (uint32_t)t);
}

// One workgroup per scene.  It clears the scene's words of ws for the chunked path, answers an empty scene (flag, 0) and
// every scene of up to kSingleMax values; a larger scene is left to the chunked launches.
__global__ __launch_bounds__(kSingleThreads) void quantile_scene_kernel(QuantArgs a) {
  __shared__ uint32_t s_hist[kBins];
  __shared__ uint32_t s_wave[4], s_sel[3], s_next;
  __shared__ int s_bad;
  const int b = blockIdx.x, t = threadIdx.x;
  uint32_t* w = a.ws + (int64_t)b * kSceneWords;
  for (int i = t; i < kSceneWords; i += kSingleThreads) w[i] = i == kPasses * kBins ? 0xffffffffu : 0u;
  int64_t lo;
  const int64_t m = scene_rows(a, b, &lo);
  if (m > kSingleMax) return;
  if (m == 0) {
    if (t == 0) write_result(a, b, m, 0, 0.0, 0, 0, 0, 0, true);
    return;
  }
  double g;
  const uint32_t k = rank_of(m, a.q, &g);
  uint32_t prefix = 0, rank = k, less = 0, count = 0, above = 0xffffffffu;
  int bad = 0;
  if (t == 0) s_next = 0xffffffffu, s_bad = 0;
  for (int p = 0; p < kPasses; ++p) {
    if (t < kBins) s_hist[t] = 0;
    __syncthreads();
    scan_rows(a, lo, 0, m, p, prefix, s_hist, &above, &bad);
    __syncthreads();
    select_digit(s_hist, s_wave, s_sel, prefix, rank, less, count);
  }
  next_in_hist(s_hist, prefix, &s_next);  // the last pass's histogram is still in place
  if (above != 0xffffffffu) atomicMin(&s_next, above);
  if (bad) atomicOr(&s_bad, 1);
  __syncthreads();
  if (t == 0) write_result(a, b, m, k, g, prefix, less, count, s_next, s_bad != 0);
}

// Workgroup w of the chunked launches -> (scene, chunk).  Scene b owns the workgroups from offsets[b] / kChunk + b on: the
// next scene starts at least ceil(m_b / kChunk) later, so no two scenes share one, and floor(n / kChunk) + B + 1 cover all.
__device__ inline int chunk_scene(const QuantArgs& a, int64_t w, int64_t* chunk) {
  int lo = 0, hi = a.B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.offs[mid] / kChunk + mid <= w) lo = mid; else hi = mid - 1;
  }
  *chunk = w - (a.offs[lo] / kChunk + lo);
  return lo;
}

// Pass p of the scenes above kSingleMax: a workgroup replays the select on the finished histograms of the passes before,
// counts its chunk in LDS and adds the bins it filled to the scene's histogram p in ws.
__global__ __launch_bounds__(kChunkThreads) void quantile_pass_kernel(QuantArgs a, int p) {
  __shared__ uint32_t s_hist[kBins];
  __shared__ uint32_t s_wave[4], s_sel[3];
  const int t = threadIdx.x;
  int64_t chunk;
  const int b = chunk_scene(a, blockIdx.x, &chunk);
  int64_t lo;
  const int64_t m = scene_rows(a, b, &lo);
  if (m <= kSingleMax || chunk < 0 || chunk * kChunk >= m) return;
  uint32_t* w = a.ws + (int64_t)b * kSceneWords;
  double g;
  uint32_t prefix = 0, rank = rank_of(m, a.q, &g), less = 0, count = 0, above = 0xffffffffu;
  for (int pp = 0; pp < p; ++pp) select_digit(w + pp * kBins, s_wave, s_sel, prefix, rank, less, count);
  int bad = 0;
  s_hist[t] = 0;
  __syncthreads();
  const int64_t r0 = chunk * kChunk;
  scan_rows(a, lo, r0, std::min<int64_t>(r0 + kChunk, m), p, prefix, s_hist, &above, &bad);
  __syncthreads();
  if (s_hist[t] != 0u) atomicAdd(&w[p * kBins + t], s_hist[t]);
  if (above != 0xffffffffu) atomicMin(&w[kPasses * kBins], above);
  if (bad) atomicOr(&w[kPasses * kBins + 1], 1u);
}

__global__ __launch_bounds__(kChunkThreads) void quantile_finish_kernel(QuantArgs a) {
  __shared__ uint32_t s_wave[4], s_sel[3], s_next;
  const int b = blockIdx.x, t = threadIdx.x;
  int64_t lo;
  const int64_t m = scene_rows(a, b, &lo);
  if (m <= kSingleMax) return;
  const uint32_t* w = a.ws + (int64_t)b * kSceneWords;
  double g;
  const uint32_t k = rank_of(m, a.q, &g);
  uint32_t prefix = 0, rank = k, less = 0, count = 0;
  if (t == 0) s_next = w[kPasses * kBins];
  for (int p = 0; p < kPasses; ++p) select_digit(w + p * kBins, s_wave, s_sel, prefix, rank, less, count);
  next_in_hist(w + (kPasses - 1) * kBins, prefix, &s_next);
  __syncthreads();
  if (t == 0) write_result(a, b, m, k, g, prefix, less, count, s_next, w[kPasses * kBins + 1] != 0u);
}

// ---- the feature columns ---------------------------------------------------------------------------------------------------------
struct FeatArgs {
  const float* pc;        // [B, P, 3]
  const float* xyz;       // [n, 3]
  const float* rgb;       // [n, 3] or null
  const int64_t* offs;
  int64_t n;
  int B;
  int64_t P;
  const int32_t* choices;
  const double* floor;    // [B] or null
  int mode;
  int augment;
  const double* scale;    // [B]
  const double* gain;     // [B, 3] or null
  const double* shift;    // [B, 3] or null
  const double* jitter;   // [B, P] or null
  const uint8_t* keep;    // [B, P] or null
  float* out;             // [B, P, 3 + C]
  int32_t* flags;
};

__global__ __launch_bounds__(kThreads) void features_kernel(FeatArgs a) {
  const int64_t row = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (row >= (int64_t)a.B * a.P) return;
  const int b = (int)(row / a.P);
  const int C = (a.rgb ? 3 : 0) + (a.floor ? 1 : 0);
  const int64_t lo = a.offs[b], hi = a.offs[b + 1];
  const int64_t c = a.choices[row];
  int flag = 0;
  int64_t g = -1;
  if (lo >= 0 && hi >= lo && hi <= a.n && c >= 0 && c < hi - lo) g = lo + c; else flag = PCMI_DET_FLAG_CHOICE;
  float* o = a.out + (3 + C) * row;
#pragma unroll
  for (int r = 0; r < 3; ++r) o[r] = a.pc[3 * row + r];
  float col[3] = {0.f, 0.f, 0.f}, height = 0.f;
  if (g >= 0 && a.rgb) {
    const float s[3] = {a.rgb[3 * g], a.rgb[3 * g + 1], a.rgb[3 * g + 2]};
    if (!(isfinite(s[0]) && isfinite(s[1]) && isfinite(s[2]))) {
      flag |= PCMI_DET_FLAG_FEATURE;
    } else if (a.mode == PCMI_DET_SCANNET) {
      const double mean[3] = {109.8, 97.2, 83.8};
#pragma unroll
      for (int r = 0; r < 3; ++r) col[r] = (float)(((double)s[r] - mean[r]) / 256.0);
    } else {
#pragma unroll
      for (int r = 0; r < 3; ++r) col[r] = (float)((double)s[r] - 0.5);
      if (a.augment) {
        const double jit = a.jitter ? a.jitter[row] : 0.0;
        const double kp = (a.keep && a.keep[row] == 0) ? 0.0 : 1.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          double x = (double)col[r] + 0.5;
          x = x * (a.gain ? a.gain[3 * b + r] : 1.0);
          x = x + (a.shift ? a.shift[3 * b + r] : 0.0);
          x = x + jit;
          x = fmin(fmax(x, 0.0), 1.0);
          x = x * kp;
          col[r] = (float)(x - 0.5);
        }
      }
    }
  }
  if (g >= 0 && a.floor) {
    const float z = a.xyz[3 * g + 2];
    if (!isfinite(z)) {
      flag |= PCMI_DET_FLAG_FEATURE;
    } else {
      height = (float)((double)z - a.floor[b]);
      if (a.mode == PCMI_DET_SUNRGBD && a.augment) height = (float)((double)height * a.scale[b]);
    }
  }
  int at = 3;
  if (a.rgb) {
#pragma unroll
    for (int r = 0; r < 3; ++r) o[at + r] = col[r];
    at += 3;
  }
  if (a.floor) o[at] = height;
  if (flag) atomicOr(&a.flags[b], flag);
}

}  // namespace detfeat
}  // namespace pcmi

using namespace pcmi;
using namespace pcmi::detfeat;

extern "C" {

size_t pcmi_segment_quantile_workspace_bytes(int64_t B) {
  if (B < 1 || B > kMaxScenes) return 0;
  return align_up((size_t)B * kSceneWords * 4, 256);
}

int pcmi_segment_quantile(const float* values, int64_t stride, const int64_t* offsets, int64_t n, int64_t B, double q, double* out,
                          float* out_stats, int32_t* flags, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_REQUIRE(B >= 1 && n >= 0 && stride >= 1 && stride <= 65536, PCMI_ERR_INVALID,
               "segment_quantile: bad shape (B %lld >= 1, n %lld >= 0, 1 <= stride %lld <= 65536)", (long long)B, (long long)n,
               (long long)stride);
  PCMI_REQUIRE(B <= kMaxScenes && n < kMaxRows, PCMI_ERR_RANGE, "segment_quantile: B %lld <= %d and n %lld < 2^29", (long long)B, kMaxScenes,
               (long long)n);
  PCMI_REQUIRE(q >= 0.0 && q <= 100.0, PCMI_ERR_INVALID, "segment_quantile: q %g must lie in [0, 100]", q);
  PCMI_REQUIRE(offsets && out && flags && (n == 0 || values), PCMI_ERR_INVALID, "segment_quantile: null pointer");
  PCMI_REQUIRE((uintptr_t)offsets % 8 == 0 && (uintptr_t)out % 8 == 0 && (uintptr_t)values % 4 == 0 && (uintptr_t)out_stats % 4 == 0 &&
                   (uintptr_t)flags % 4 == 0,
               PCMI_ERR_INVALID, "segment_quantile: misaligned pointer (8 bytes for fp64 and int64, 4 for fp32 and int32)");
  if (int rc = require_ws("segment_quantile", ws, ws_bytes, pcmi_segment_quantile_workspace_bytes(B), 16)) return rc;
  hipStream_t st = as_stream(stream);
  QuantArgs a{values, stride, offsets, n, (int)B, q, out, out_stats, flags, static_cast<uint32_t*>(ws)};
  quantile_scene_kernel<<<(unsigned)B, kSingleThreads, 0, st>>>(a);
  PCMI_LAUNCH_CHECK();
  if (n > kSingleMax) {  // no scene can be larger otherwise
    const unsigned grid = (unsigned)(n / kChunk + B + 1);
    for (int p = 0; p < kPasses; ++p) {
      quantile_pass_kernel<<<grid, kChunkThreads, 0, st>>>(a, p);
      PCMI_LAUNCH_CHECK();
    }
    quantile_finish_kernel<<<(unsigned)B, kChunkThreads, 0, st>>>(a);
    PCMI_LAUNCH_CHECK();
  }
  return PCMI_OK;
}

int pcmi_det_point_features(const float* point_clouds, const float* xyz, const float* rgb, const int64_t* offsets, int64_t n, int64_t B,
                            int64_t num_points, const int32_t* choices, const double* floor_height, int mode, int augment,
                            const double* scale, const double* color_gain, const double* color_shift, const double* color_jitter,
                            const uint8_t* color_keep, float* out, int32_t* flags, pcmi_stream_t stream) {
  PCMI_REQUIRE(B >= 1 && B <= kMaxScenes && num_points >= 1 && num_points <= kMaxRows && B * num_points <= kMaxRows && n >= 0 &&
                   n < (1ll << 31) - kThreads,
               PCMI_ERR_INVALID, "det_point_features: bad shape (1 <= B %lld <= %d; 1 <= num_points %lld, B num_points <= 2^29; 0 <= n %lld < 2^31 - 256)",
               (long long)B, kMaxScenes, (long long)num_points, (long long)n);
  PCMI_REQUIRE(mode == PCMI_DET_SCANNET || mode == PCMI_DET_SUNRGBD, PCMI_ERR_INVALID, "det_point_features: mode %d (0 ScanNet, 1 SUN RGB-D)", mode);
  PCMI_REQUIRE(rgb || floor_height, PCMI_ERR_INVALID, "det_point_features: no feature column asked for (rgb and floor_height both NULL)");
  PCMI_REQUIRE(point_clouds && offsets && choices && out && flags && (n == 0 || !floor_height || xyz), PCMI_ERR_INVALID,
               "det_point_features: null pointer");
  PCMI_REQUIRE(!(augment && mode == PCMI_DET_SUNRGBD && floor_height) || scale, PCMI_ERR_INVALID,
               "det_point_features: the augmented SUN RGB-D height needs scale");
  PCMI_REQUIRE((uintptr_t)offsets % 8 == 0 && (uintptr_t)floor_height % 8 == 0 && (uintptr_t)scale % 8 == 0 && (uintptr_t)color_gain % 8 == 0 &&
                   (uintptr_t)color_shift % 8 == 0 && (uintptr_t)color_jitter % 8 == 0 && (uintptr_t)point_clouds % 4 == 0 &&
                   (uintptr_t)xyz % 4 == 0 && (uintptr_t)rgb % 4 == 0 && (uintptr_t)choices % 4 == 0 && (uintptr_t)out % 4 == 0,
               PCMI_ERR_INVALID, "det_point_features: misaligned pointer (8 bytes for fp64 and int64, 4 for fp32 and int32)");
  FeatArgs a{point_clouds, xyz, rgb, offsets, n, (int)B, num_points, choices, floor_height, mode, augment ? 1 : 0, scale, color_gain,
             color_shift, color_jitter, color_keep, out, flags};
  features_kernel<<<(unsigned)ceil_div(B * num_points, kThreads), kThreads, 0, as_stream(stream)>>>(a);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

}  // extern "C"
