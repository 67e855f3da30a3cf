// The input side of instance-segmentation fine-tuning for a BATCH of scans, on the device, behind pcmi_seg_quantize:
//   * pcmi_instance_relabel   per-scene raw instance ids -> indices that are unique across the batch, numbered by lowest row
//   * pcmi_instance_table     per instance: rows, scene, class, exact coordinate sums, bounding box
//   * pcmi_seg_crop_ladder    a window per scene that bounds its voxels (this project's own rule, see include/pcmi.h)
// Written from the semantics in include/pcmi.h; gfx950, wave64.  The reference has no counterpart.
//
// All arithmetic is integer.  The only atomics are integer sums, minima, maxima and ors, whose result does not depend on the
// order of arrival, and the compare-and-swap that claims a table slot, whose outcome -- WHICH slot a key gets -- never reaches
// an output: ids and rows leave in the order of an exclusive scan over the rows.  Every output is the same bits from run to run.
// offsets [B + 1] is read on the device only, so a call chains behind pcmi_seg_quantize before its counts are read back: the
// launches are sized by the capacity n, and a row outside every scene is neither read nor written.
#include <algorithm>
#include <climits>

#include "firstrow.h"
#include "internal.h"
#include "rowscan.h"

namespace pcmi {
namespace insinput {

using rowscan::kThreads;
using rowscan::scan_blocks;
using rowscan::scan_excl;

constexpr int kMaxScenes = 1023;        // as pcmi_seg_quantize
constexpr int64_t kMaxRows = 1ll << 29; // table of 2 n slots, scanned with 32-bit counts
constexpr int kMaxSteps = 32;           // steps of a crop ladder: one bit each in a row's mask
constexpr int kLdsScenes = 4;           // scenes from a workgroup's first on whose step counts are gathered in LDS
// slot_of: kNoSlot for a row of a scene that belongs to no instance, and
constexpr uint32_t kOutside = 0xfffffffeu;  // a row outside every scene (the table has at most 2^30 slots)

static bool batch_ok(int64_t n, int64_t B) { return n >= 0 && n < (1ll << 31) - kThreads && B >= 1 && B <= kMaxScenes; }
static unsigned grid_for(int64_t n) { return (unsigned)ceil_div(std::max<int64_t>(n, 1), kThreads); }

// true when every lane of the wave holds the same key: one lane then speaks for all.  Every lane must call.
__device__ inline bool wave_same(int key) { return __ballot(key == __shfl(key, 0, 64)) == ~0ull; }

// ---- relabel ---------------------------------------------------------------------------------------------------------------
// pass 1: the row's (scene, raw id) claims its slot; first[slot] = the lowest row of the instance
__global__ __launch_bounds__(kThreads) void rl_insert_kernel(const int32_t* __restrict__ raw, const uint8_t* __restrict__ keep, int64_t n,
                                                             const int64_t* __restrict__ offs, int B, uint64_t* keys, uint32_t cap,
                                                             uint32_t* first, uint32_t* __restrict__ slot_of) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int b = segment_of(offs, B, i);
  uint32_t slot = b < 0 ? kOutside : kNoSlot;
  if (b >= 0) {
    const int32_t r = raw[i];
    if (r >= 0 && (!keep || keep[i])) slot = claim_first(keys, 0, cap, ((uint64_t)(uint32_t)b << 32) | (uint32_t)r, first, i);
  }
  slot_of[i] = slot;
}

// pass 2: is this row the lowest of its instance?  (flag [n + 1]: the last one is 0)
__global__ __launch_bounds__(kThreads) void rl_flag_kernel(int64_t n, const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ first,
                                                           int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i > n) return;
  int f = 0;
  if (i < n) {
    const uint32_t slot = slot_of[i];
    f = (slot < kOutside && first[slot] == (uint32_t)i) ? 1 : 0;
  }
  flag[i] = f;
}

// pass 3 (after the exclusive scan pos of the flags, in their place): a row takes the number of its instance's lowest row
__global__ __launch_bounds__(kThreads) void rl_write_kernel(int64_t n, const int64_t* __restrict__ offs, int B,
                                                            const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ first,
                                                            const int32_t* __restrict__ pos, int32_t* __restrict__ instance,
                                                            int32_t* __restrict__ first_row, int64_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  segment_counts(i, offs, B, n, pos, counts);
  if (i >= n) return;
  const uint32_t slot = slot_of[i];
  if (slot == kOutside) return;
  if (slot == kNoSlot) {
    instance[i] = -1;
    return;
  }
  const uint32_t r = first[slot];
  const int32_t g = pos[r];
  instance[i] = g;
  if (r == (uint32_t)i) first_row[g] = (int32_t)i;
}

// ---- table -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void tb_init_kernel(int64_t G, int32_t* __restrict__ size, int32_t* __restrict__ scene,
                                                           int32_t* __restrict__ cls, unsigned long long* __restrict__ sum,
                                                           int32_t* __restrict__ box_min, int32_t* __restrict__ box_max) {
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= G) return;
  size[g] = 0;
  scene[g] = -1;
  if (cls) cls[g] = -1;
  if (sum) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      sum[3 * g + a] = 0ull;
      box_min[3 * g + a] = INT_MAX;
      box_max[3 * g + a] = INT_MIN;
    }
  }
}

// Rows of one instance mostly stand together, so the 64 lanes of a wave often hold ONE id: the wave then reduces its values
// with shuffles and lane 0 issues the atomics (integer sums, minima and maxima: the grouping changes no result).
__global__ __launch_bounds__(kThreads) void tb_rows_kernel(const int32_t* __restrict__ instance, const int32_t* __restrict__ klass,
                                                           const int32_t* __restrict__ coords, int64_t n, const int64_t* __restrict__ offs,
                                                           int B, int64_t G, int32_t* size, int32_t* scene, int32_t* cls,
                                                           unsigned long long* sum, int32_t* box_min, int32_t* box_max) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int b = i < n ? segment_of(offs, B, i) : -1;
  int32_t k = b >= 0 ? instance[i] : -1;
  if (k < 0 || k >= G) k = -1;
  int cnt = k >= 0 ? 1 : 0, sc = k >= 0 ? b : -1, kl = -1;
  int c[3] = {0, 0, 0};
  if (k >= 0) {
    if (klass) kl = std::max(klass[i], -1);
    if (coords) {
#pragma unroll
      for (int a = 0; a < 3; ++a) c[a] = coords[4 * i + 1 + a];
    }
  }
  long long s[3] = {c[0], c[1], c[2]};
  int lo[3] = {c[0], c[1], c[2]}, hi[3] = {c[0], c[1], c[2]};
  if (wave_same(k)) {
    if (k < 0) return;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      cnt += __shfl_xor(cnt, d, 64);
      sc = std::max(sc, __shfl_xor(sc, d, 64));
      kl = std::max(kl, __shfl_xor(kl, d, 64));
    }
    if (coords) {
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          s[a] += __shfl_xor(s[a], d, 64);
          lo[a] = std::min(lo[a], __shfl_xor(lo[a], d, 64));
          hi[a] = std::max(hi[a], __shfl_xor(hi[a], d, 64));
        }
    }
    if ((threadIdx.x & 63) != 0) return;
  } else if (k < 0) {
    return;
  }
  atomicAdd(&size[k], cnt);
  atomicMax(&scene[k], sc);
  if (cls) atomicMax(&cls[k], kl);
  if (coords) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      atomicAdd(&sum[3 * (int64_t)k + a], (unsigned long long)s[a]);
      atomicMin(&box_min[3 * (int64_t)k + a], lo[a]);
      atomicMax(&box_max[3 * (int64_t)k + a], hi[a]);
    }
  }
}

// ---- crop ladder -----------------------------------------------------------------------------------------------------------
struct Ladder {
  int S, col0, col1;  // the steps; the two horizontal columns of coords (1 ... 3)
  int side[kMaxSteps][2];
};

// ws: ext [B, 2] (the maxima of the two columns), cnt [B, kMaxSteps] (rows inside the window of each step)
__global__ __launch_bounds__(kThreads) void cr_init_kernel(int B, int32_t* __restrict__ ext, int32_t* __restrict__ cnt) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t < 2 * B) ext[t] = INT_MIN;
  if (t < kMaxSteps * B) cnt[t] = 0;
}

__global__ __launch_bounds__(kThreads) void cr_extent_kernel(const int32_t* __restrict__ coords, int64_t n, const int64_t* __restrict__ offs,
                                                             int B, int col0, int col1, int32_t* ext) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int b = i < n ? segment_of(offs, B, i) : -1;
  int e0 = INT_MIN, e1 = INT_MIN;
  if (b >= 0) e0 = coords[4 * i + col0], e1 = coords[4 * i + col1];
  if (wave_same(b)) {
    if (b < 0) return;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      e0 = std::max(e0, __shfl_xor(e0, d, 64));
      e1 = std::max(e1, __shfl_xor(e1, d, 64));
    }
    if ((threadIdx.x & 63) != 0) return;
  } else if (b < 0) {
    return;
  }
  atomicMax(&ext[2 * b], e0);
  atomicMax(&ext[2 * b + 1], e1);
}

// origin [B, kMaxSteps, 2] = (uint64(draw) (slack + 1)) >> 32, slack = max(ext + 1 - side, 0)
__global__ __launch_bounds__(kThreads) void cr_origin_kernel(int B, Ladder L, const int32_t* __restrict__ ext, const uint32_t* __restrict__ draws,
                                                             int32_t* __restrict__ origin) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= B * L.S * 2) return;
  const int a = t & 1, s = (t >> 1) % L.S, b = (t >> 1) / L.S;
  const int64_t slack = std::max<int64_t>((int64_t)ext[2 * b + a] + 1 - L.side[s][a], 0);
  origin[(b * kMaxSteps + s) * 2 + a] = (int32_t)(((uint64_t)draws[(b * L.S + s) * 2 + a] * (uint64_t)(slack + 1)) >> 32);
}

// every row of a scene above max_voxels tests all S windows: mask [n] = bit s set iff the row is inside the window of step s;
// the counts per (scene, step) are gathered in LDS for the kLdsScenes scenes from the workgroup's first on (a wave that stands
// in one scene counts a step with one ballot) and leave with one atomic per counter
__global__ __launch_bounds__(kThreads) void cr_count_kernel(const int32_t* __restrict__ coords, int64_t n, const int64_t* __restrict__ offs, int B,
                                                            Ladder L, int64_t max_voxels, const int32_t* __restrict__ origin,
                                                            uint32_t* __restrict__ mask, int32_t* cnt) {
  __shared__ int s_cnt[kLdsScenes][kMaxSteps];
  __shared__ int s_first;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int b = i < n ? segment_of(offs, B, i) : -1;
  if (threadIdx.x < kLdsScenes * kMaxSteps) (&s_cnt[0][0])[threadIdx.x] = 0;
  if (threadIdx.x == 0) s_first = std::max(b, 0);  // (offsets ascend: no row of the workgroup lies in a lower scene)
  __syncthreads();
  uint32_t m = 0;
  bool big = false;
  if (b >= 0) {
    big = offs[b + 1] - offs[b] > max_voxels;
    if (big) {
      const int64_t c0 = coords[4 * i + L.col0], c1 = coords[4 * i + L.col1];
      for (int s = 0; s < L.S; ++s) {
        const int64_t o0 = origin[(b * kMaxSteps + s) * 2], o1 = origin[(b * kMaxSteps + s) * 2 + 1];
        const bool in = c0 >= o0 && c0 < o0 + L.side[s][0] && c1 >= o1 && c1 < o1 + L.side[s][1];
        m |= in ? (1u << s) : 0u;
      }
    }
    mask[i] = m;
  }
  const int slot = b - s_first;
  const bool lds = slot >= 0 && slot < kLdsScenes;
  if (wave_same(b)) {
    if (big) {  // (wave-uniform: one scene)
      for (int s = 0; s < L.S; ++s) {
        const int c = __popcll(__ballot((m >> s) & 1u));
        if ((threadIdx.x & 63) == 0 && c) {
          if (lds) atomicAdd(&s_cnt[slot][s], c); else atomicAdd(&cnt[b * kMaxSteps + s], c);
        }
      }
    }
  } else {
    for (uint32_t rest = m; rest; rest &= rest - 1) {
      const int s = __ffs(rest) - 1;
      if (lds) atomicAdd(&s_cnt[slot][s], 1); else atomicAdd(&cnt[b * kMaxSteps + s], 1);
    }
  }
  __syncthreads();
  if (threadIdx.x < kLdsScenes * kMaxSteps) {
    const int c = (&s_cnt[0][0])[threadIdx.x], sb = s_first + (int)threadIdx.x / kMaxSteps;
    if (c && sb < B) atomicAdd(&cnt[sb * kMaxSteps + (int)threadIdx.x % kMaxSteps], c);
  }
}

// one thread per scene: -1 for a scene within max_voxels, else the lowest step that fits, else the last one and the flag
__global__ __launch_bounds__(kThreads) void cr_choose_kernel(const int64_t* __restrict__ offs, int B, int S, int64_t max_voxels,
                                                             const int32_t* __restrict__ cnt, int32_t* __restrict__ step, int32_t* flags) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= B) return;
  int s = -1;
  if (offs[b + 1] - offs[b] > max_voxels) {
    for (s = 0; s < S; ++s)
      if (cnt[b * kMaxSteps + s] <= max_voxels) break;
    if (s == S) {
      s = S - 1;
      atomicOr(&flags[b], PCMI_SEG_FLAG_CROP);
    }
  }
  step[b] = s;
}

// kept [n + 1]: the row is in a scene and inside its scene's window (the last one is 0)
__global__ __launch_bounds__(kThreads) void cr_flag_kernel(int64_t n, const int64_t* __restrict__ offs, int B, const uint32_t* __restrict__ mask,
                                                           const int32_t* __restrict__ step, int32_t* __restrict__ kept) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i > n) return;
  int f = 0;
  if (i < n) {
    const int b = segment_of(offs, B, i);
    if (b >= 0) {
      const int s = step[b];
      f = s < 0 ? 1 : (int)((mask[i] >> s) & 1u);
    }
  }
  kept[i] = f;
}

__global__ __launch_bounds__(kThreads) void cr_write_kernel(int64_t n, const int64_t* __restrict__ offs, int B, const int32_t* __restrict__ kept,
                                                            const int32_t* __restrict__ pos, int64_t* __restrict__ rows,
                                                            int64_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  segment_counts(i, offs, B, n, pos, counts);
  if (i < n && kept[i]) rows[pos[i]] = i;
}

}  // namespace insinput
}  // namespace pcmi

using namespace pcmi;
using namespace pcmi::insinput;

extern "C" {

struct RelabelWs { uint64_t* keys; uint32_t *first, *slot_of; int32_t *pos, *sums, *boffs, *total; size_t bytes; };
static RelabelWs relabel_ws(void* ws, int64_t n) {
  const size_t cap = (size_t)table_cap(n), nb = (size_t)scan_blocks(n + 1);
  Carve cv{(char*)ws};
  RelabelWs w;
  w.keys = cv.take<uint64_t>(cap);
  w.first = cv.take<uint32_t>(cap);
  w.slot_of = cv.take<uint32_t>((size_t)std::max<int64_t>(n, 1));
  w.pos = cv.take<int32_t>((size_t)n + 1);
  w.sums = cv.take<int32_t>(nb);
  w.boffs = cv.take<int32_t>(nb);
  w.total = cv.take<int32_t>(1);
  w.bytes = cv.used;
  return w;
}

size_t pcmi_instance_relabel_workspace_bytes(int64_t n) {
  if (n < 0 || n > kMaxRows) return 0;
  return relabel_ws(nullptr, n).bytes;
}

int pcmi_instance_relabel(const int32_t* raw, const uint8_t* keep, const int64_t* offsets, int64_t n, int64_t B, int32_t* instance,
                          int32_t* first_row, int64_t* inst_counts, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_REQUIRE(batch_ok(n, B), PCMI_ERR_INVALID, "instance_relabel: bad shape (0 <= n %lld < 2^31 - 256; 1 <= B %lld <= %d)", (long long)n,
               (long long)B, kMaxScenes);
  PCMI_REQUIRE(n <= kMaxRows, PCMI_ERR_UNSUPPORTED, "instance_relabel: %lld rows, at most 2^29", (long long)n);
  PCMI_REQUIRE(offsets && inst_counts && (n == 0 || (raw && instance && first_row)), PCMI_ERR_INVALID, "instance_relabel: null pointer");
  if (int rc = require_ws("instance_relabel", ws, ws_bytes, relabel_ws(nullptr, n).bytes, 16)) return rc;
  hipStream_t st = as_stream(stream);
  if (n == 0) {
    PCMI_HIP_CHECK(hipMemsetAsync(inst_counts, 0, (size_t)(B + 1) * 8, st));
    return PCMI_OK;
  }
  const int64_t cap = table_cap(n);
  const RelabelWs w = relabel_ws(ws, n);
  PCMI_HIP_CHECK(hipMemsetAsync(w.keys, 0xff, (size_t)cap * 8, st));
  PCMI_HIP_CHECK(hipMemsetAsync(w.first, 0xff, (size_t)cap * 4, st));
  rl_insert_kernel<<<grid_for(n), kThreads, 0, st>>>(raw, keep, n, offsets, (int)B, w.keys, (uint32_t)cap, w.first, w.slot_of);
  PCMI_LAUNCH_CHECK();
  rl_flag_kernel<<<grid_for(n + 1), kThreads, 0, st>>>(n, w.slot_of, w.first, w.pos);
  PCMI_LAUNCH_CHECK();
  if (int rc = scan_excl(w.pos, n + 1, w.pos, w.sums, w.boffs, w.total, st)) return rc;
  rl_write_kernel<<<grid_for(std::max<int64_t>(n, B + 1)), kThreads, 0, st>>>(n, offsets, (int)B, w.slot_of, w.first, w.pos, instance, first_row,
                                                                               inst_counts);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

int pcmi_instance_table(const int32_t* instance, const int32_t* klass, const int32_t* coords, const int64_t* offsets, int64_t n, int64_t B,
                        int64_t G, int32_t* size, int32_t* scene, int32_t* cls, int64_t* sum, int32_t* box_min, int32_t* box_max,
                        pcmi_stream_t stream) {
  PCMI_REQUIRE(batch_ok(n, B) && G >= 0 && G < (1ll << 31), PCMI_ERR_INVALID,
               "instance_table: bad shape (0 <= n %lld < 2^31 - 256; 1 <= B %lld <= %d; 0 <= G %lld < 2^31)", (long long)n, (long long)B,
               kMaxScenes, (long long)G);
  PCMI_REQUIRE(n <= kMaxRows, PCMI_ERR_UNSUPPORTED, "instance_table: %lld rows, at most 2^29", (long long)n);
  if (G == 0) return PCMI_OK;
  PCMI_REQUIRE((sum == nullptr) == (box_min == nullptr) && (sum == nullptr) == (box_max == nullptr) && (klass == nullptr || cls) &&
                   (coords == nullptr || sum) && (n == 0 || ((cls == nullptr || klass) && (sum == nullptr || coords))),
               PCMI_ERR_INVALID, "instance_table: klass goes with cls, coords with sum, box_min and box_max");
  PCMI_REQUIRE(offsets && size && scene && (n == 0 || instance), PCMI_ERR_INVALID, "instance_table: null pointer");
  hipStream_t st = as_stream(stream);
  unsigned long long* usum = reinterpret_cast<unsigned long long*>(sum);
  tb_init_kernel<<<grid_for(G), kThreads, 0, st>>>(G, size, scene, cls, usum, box_min, box_max);
  PCMI_LAUNCH_CHECK();
  if (n > 0) {
    tb_rows_kernel<<<grid_for(n), kThreads, 0, st>>>(instance, klass, coords, n, offsets, (int)B, G, size, scene, cls, usum, box_min, box_max);
    PCMI_LAUNCH_CHECK();
  }
  return PCMI_OK;
}

struct CropWs { int32_t *ext, *cnt, *origin; uint32_t* mask; int32_t *kept, *pos, *sums, *boffs, *total; size_t bytes; };
static CropWs crop_ws(void* ws, int64_t n, int64_t B) {
  const size_t nb = (size_t)scan_blocks(n + 1);
  Carve cv{(char*)ws};
  CropWs w;
  w.ext = cv.take<int32_t>((size_t)B * 2);
  w.cnt = cv.take<int32_t>((size_t)B * kMaxSteps);
  w.origin = cv.take<int32_t>((size_t)B * kMaxSteps * 2);
  w.mask = cv.take<uint32_t>((size_t)std::max<int64_t>(n, 1));
  w.kept = cv.take<int32_t>((size_t)n + 1);
  w.pos = cv.take<int32_t>((size_t)n + 1);
  w.sums = cv.take<int32_t>(nb);
  w.boffs = cv.take<int32_t>(nb);
  w.total = cv.take<int32_t>(1);
  w.bytes = cv.used;
  return w;
}

size_t pcmi_seg_crop_ladder_workspace_bytes(int64_t n, int64_t B) {
  if (n < 0 || n > kMaxRows || B < 1 || B > kMaxScenes) return 0;
  return crop_ws(nullptr, n, B).bytes;
}

int pcmi_seg_crop_ladder(const int32_t* coords, const int64_t* offsets, int64_t n, int64_t B, int axis0, int axis1, const int32_t* sides_host,
                         int S, const uint32_t* draws, int64_t max_voxels, int64_t* rows, int64_t* kept_counts, int32_t* step,
                         int32_t* flags, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_REQUIRE(batch_ok(n, B), PCMI_ERR_INVALID, "seg_crop_ladder: bad shape (0 <= n %lld < 2^31 - 256; 1 <= B %lld <= %d)", (long long)n,
               (long long)B, kMaxScenes);
  PCMI_REQUIRE(n <= kMaxRows, PCMI_ERR_UNSUPPORTED, "seg_crop_ladder: %lld rows, at most 2^29", (long long)n);
  PCMI_REQUIRE(S >= 1 && S <= kMaxSteps, PCMI_ERR_INVALID, "seg_crop_ladder: %d steps, 1 ... %d", S, kMaxSteps);
  PCMI_REQUIRE(axis0 >= 1 && axis0 <= 3 && axis1 >= 1 && axis1 <= 3 && axis0 != axis1, PCMI_ERR_INVALID,
               "seg_crop_ladder: axes (%d, %d): two distinct columns of 1 ... 3", axis0, axis1);
  PCMI_REQUIRE(max_voxels >= 1, PCMI_ERR_INVALID, "seg_crop_ladder: max_voxels %lld, at least 1", (long long)max_voxels);
  PCMI_REQUIRE(sides_host && offsets && draws && kept_counts && step && flags && (n == 0 || (coords && rows)), PCMI_ERR_INVALID,
               "seg_crop_ladder: null pointer");
  Ladder L;
  L.S = S, L.col0 = axis0, L.col1 = axis1;
  for (int s = 0; s < kMaxSteps; ++s)
    for (int a = 0; a < 2; ++a) {
      L.side[s][a] = s < S ? sides_host[2 * s + a] : 1;
      PCMI_REQUIRE(L.side[s][a] >= 1 && (s == 0 || s >= S || L.side[s][a] <= L.side[s - 1][a]), PCMI_ERR_INVALID,
                   "seg_crop_ladder: side [%d][%d] = %d: every side at least 1, each column non-increasing", s, a, L.side[s][a]);
    }
  if (int rc = require_ws("seg_crop_ladder", ws, ws_bytes, crop_ws(nullptr, n, B).bytes, 16)) return rc;
  hipStream_t st = as_stream(stream);
  if (n == 0) {
    PCMI_HIP_CHECK(hipMemsetAsync(kept_counts, 0, (size_t)(B + 1) * 8, st));
    return PCMI_OK;
  }
  const CropWs w = crop_ws(ws, n, B);
  const unsigned grid = grid_for(n);
  cr_init_kernel<<<grid_for(B * kMaxSteps), kThreads, 0, st>>>((int)B, w.ext, w.cnt);
  PCMI_LAUNCH_CHECK();
  cr_extent_kernel<<<grid, kThreads, 0, st>>>(coords, n, offsets, (int)B, axis0, axis1, w.ext);
  PCMI_LAUNCH_CHECK();
  cr_origin_kernel<<<grid_for(B * S * 2), kThreads, 0, st>>>((int)B, L, w.ext, draws, w.origin);
  PCMI_LAUNCH_CHECK();
  cr_count_kernel<<<grid, kThreads, 0, st>>>(coords, n, offsets, (int)B, L, max_voxels, w.origin, w.mask, w.cnt);
  PCMI_LAUNCH_CHECK();
  cr_choose_kernel<<<grid_for(B), kThreads, 0, st>>>(offsets, (int)B, S, max_voxels, w.cnt, step, flags);
  PCMI_LAUNCH_CHECK();
  cr_flag_kernel<<<grid_for(n + 1), kThreads, 0, st>>>(n, offsets, (int)B, w.mask, step, w.kept);
  PCMI_LAUNCH_CHECK();
  if (int rc = scan_excl(w.kept, n + 1, w.pos, w.sums, w.boffs, w.total, st)) return rc;
  cr_write_kernel<<<grid_for(std::max<int64_t>(n, B + 1)), kThreads, 0, st>>>(n, offsets, (int)B, w.kept, w.pos, rows, kept_counts);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

}  // extern "C"
