// Instance segmentation on the device (PointGroup's recipe as Hou et al., "Contrastive Scene Contexts", use it downstream):
// connected components of a radius graph (the clustering of the offset-shifted voxels), their compaction into numbered
// instances, per-instance scores, the overlap / matching of predicted and ground-truth instances that pcmi_det_ap scores,
// integer instance centroids, and the two offset losses.  Written from the semantics in include/pcmi.h; gfx950, wave64.
//
// Arithmetic: every fp64 product and sum is an explicit round-to-nearest operation in the order include/pcmi.h states (no
// FMA contraction), the only atomics are integer ones, and no output depends on the order in which they land.
//
// The union-find of pcmi_radius_components lives in `label` itself: parent[i] = label[i].
//   Invariant: 0 <= parent[i] <= i for every active row, at all times.  A row starts as its own root (parent[i] == i).  The
//   only store that changes a ROOT is the compare-and-swap of unite(), parent[hi]: hi -> lo with lo < hi, both roots when they
//   were read; it fails if hi has been hooked meanwhile.  Every other store (compression) is an atomicMin of parent[x] with a
//   row that was an ancestor of x when it was read, which lowers parent[x] to another ancestor or does nothing.
//   * find_root strictly descends: it follows parent[x] < x until parent[x] == x, so it ends within n steps.  A relaxed load
//     may return an older value; every older value is an ancestor too (a root read late is caught by the compare-and-swap).
//   * a retry of unite() happens only when the compare-and-swap on hi failed, that is hi is no longer a root: the retry
//     continues from the row it was hooked under, which is smaller.  The larger of the two roots strictly decreases from retry
//     to retry, so unite() ends within n retries without waiting for any other lane: nobody spins.
//   * rows are only ever joined along edges of the graph, and every edge is united by the lane of its larger row before the
//     launch ends; a tree's root is its smallest row (roots are hooked under smaller roots only).  So after the last launch
//     find_root(i) is the lowest row of i's connected component whatever the interleaving was.
//   Every loop carries the explicit bound steps < n all the same, as radius_probe (cellgrid.h) does.
//
// Why 27 cells suffice.  Activity is decided with floor(fl(x / r)) as include/pcmi.h states it, but the rows are binned with
// the cell side h = r (1 + 2^-30).  Two rows with dist2_rn <= mul_rn(r, r) have |dx| <= r (1 + 2^-52) on every axis (the
// difference of two widened floats and its square round once each, rounding is monotonic), so |dx| / h < 1 - 2^-31; the two
// quotients fl(x / h) are each off by at most 2^-53 2^20 = 2^-33, so they differ by less than 1 and their floors by at most 1.
// |floor(fl(x / h))| <= |floor(fl(x / r))| (same sign, smaller magnitude, monotonic rounding), so an active row's cell fits.
#include <algorithm>

#include "blockscan.h"
#include "exact.h"
#include "firstrow.h"
#include "internal.h"
#include "rowscan.h"

#pragma clang fp contract(off)

namespace pcmi {
namespace cluster {

constexpr int kThreads = 256;  // 4 waves: one per SIMD of a CU
constexpr int kWaves = kThreads / 64;
constexpr int64_t kMaxRows = 1ll << 29;    // the table has 2 n + B slots, indexed with 32 bits
constexpr int64_t kMaxScenes = 1ll << 20;
constexpr double kFix = 1073741824.0;      // 2^30: the fixed point of pcmi_instance_scores

// the exclusive scan of int32 values in row order (three launches): rowscan.h
using rowscan::scan_blocks;
using rowscan::scan_excl;

// ---- radius components ---------------------------------------------------------------------------------------------------------
struct Rec {  // one binned row: 32 bytes, two 16-byte loads, the records of a cell contiguous
  double x, y, z;
  int32_t row, group;
};

// the scene of row i and its table segment; false if the row lies in no scene (or offs does not describe one inside [0, n])
__device__ inline bool scene_segment(const int64_t* __restrict__ offs, int B, int64_t n, int64_t i, uint32_t* base, uint32_t* size) {
  const int b = segment_of(offs, B, i);
  if (b < 0) return false;
  const int64_t lo = offs[b], hi = offs[b + 1];
  if (!(lo >= 0 && lo <= i && i < hi && hi <= n)) return false;
  *base = (uint32_t)(2 * lo + b);  // as pair_input.hip: the segment of a scene of m rows has 2 m + 1 slots, never full
  *size = (uint32_t)(2 * (hi - lo) + 1);
  return true;
}

__device__ inline int32_t load_parent(const int32_t* parent, int32_t i) {
  return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline int32_t find_root(const int32_t* parent, int32_t i, int64_t n) {
  for (int64_t steps = 0; steps < n; ++steps) {
    const int32_t p = load_parent(parent, i);
    if (p >= i || p < 0) break;  // p == i: a root (the other two never hold for an active row)
    i = p;
  }
  return i;
}
// joins the trees of a and b; returns the root both were under when it returned
__device__ inline int32_t unite(int32_t* parent, int32_t a, int32_t b, int64_t n) {
  for (int64_t steps = 0; steps < n; ++steps) {
    a = find_root(parent, a, n);
    b = find_root(parent, b, n);
    if (a == b) return a;
    const int32_t hi = max(a, b), lo = min(a, b);
    const int32_t old = atomicCAS(&parent[hi], hi, lo);
    if (old == hi) return lo;
    a = old;  // hi was hooked under old < hi meanwhile
    b = lo;
  }
  return min(a, b);
}

// pass 1: activity, label = the row itself (its own root) or -1, the cell's slot and count
__global__ __launch_bounds__(kThreads) void rc_count_kernel(const float* __restrict__ xyz, int64_t ld, int64_t n, const int64_t* __restrict__ offs,
                                                            int B, const int32_t* __restrict__ group, double r, double h, uint64_t* keys,
                                                            int32_t* count, uint32_t* __restrict__ slot_of, int32_t* __restrict__ label,
                                                            unsigned long long* dropped) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  uint32_t slot = kNoSlot, base, size;
  if (group[i] >= 0 && scene_segment(offs, B, n, i, &base, &size)) {
    const double p[3] = {(double)xyz[ld * i], (double)xyz[ld * i + 1], (double)xyz[ld * i + 2]};
    if (finite3(p[0], p[1], p[2])) {
      int64_t c[3];
      if (cells_of(p, r, c) && cells_of(p, h, c)) {
        slot = claim_slot(keys, base, size, cell_key(c[0], c[1], c[2]));
        atomicAdd(&count[slot], 1);
      } else if (dropped) {
        atomicAdd(dropped, 1ull);
      }
    }
  }
  slot_of[i] = slot;
  label[i] = slot == kNoSlot ? -1 : (int32_t)i;
}

// pass 2: the row's record into its cell's range [start[slot], start[slot + 1]) (order inside a cell: arbitrary, and immaterial)
__global__ __launch_bounds__(kThreads) void rc_fill_kernel(const float* __restrict__ xyz, int64_t ld, int64_t n, const int32_t* __restrict__ group,
                                                           const uint32_t* __restrict__ slot_of, const int32_t* __restrict__ start,
                                                           int32_t* count, Rec* __restrict__ rec) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t slot = slot_of[i];
  if (slot == kNoSlot) return;
  const int32_t pos = start[slot] + atomicSub(&count[slot], 1) - 1;
  Rec q;
  q.x = (double)xyz[ld * i];
  q.y = (double)xyz[ld * i + 1];
  q.z = (double)xyz[ld * i + 2];
  q.row = (int32_t)i;
  q.group = group[i];
  rec[pos] = q;
}

// One lane per RECORD, so that the lanes of a wave stand in the same cell and walk the same lists (their loads of the other
// rows' records are then one address per wave).  ALL == 0: the row is united with the first row of its own cell (after which a
// crowded cell is one tree); ALL != 0: with every row below it in the 27 cells around that passes the test.
template <int ALL>
__global__ __launch_bounds__(kThreads) void rc_unite_kernel(const Rec* __restrict__ rec, const int32_t* __restrict__ total, int64_t n,
                                                            const int64_t* __restrict__ offs, int B, double r, double h,
                                                            const uint64_t* __restrict__ keys, const int32_t* __restrict__ start,
                                                            int32_t* label) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= *total) return;
  const Rec me = rec[p];
  const double mp[3] = {me.x, me.y, me.z};
  uint32_t base, size;
  int64_t c[3];
  if (!scene_segment(offs, B, n, me.row, &base, &size) || !cells_of(mp, h, c)) return;  // (never: the row was binned)
  const double r2 = mul_rn(r, r);
  if (!ALL) {
    const int64_t slot = find_slot(keys, base, size, cell_key(c[0], c[1], c[2]));
    if (slot < 0) return;
    const int32_t first = start[slot];
    if (first == p) return;
    const Rec o = rec[first];
    const double op[3] = {o.x, o.y, o.z};
    if (o.group == me.group && dist2_rn(mp, op) <= r2) (void)unite(label, me.row, o.row, n);
    return;
  }
  int32_t mine = load_parent(label, me.row);
  for (int dz = -1; dz <= 1; ++dz)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        if (!cell_ok(c[0] + dx, c[1] + dy, c[2] + dz)) continue;
        const int64_t slot = find_slot(keys, base, size, cell_key(c[0] + dx, c[1] + dy, c[2] + dz));
        if (slot < 0) continue;
        const int32_t e = start[slot + 1];
        for (int32_t q = start[slot]; q < e; ++q) {
          const Rec o = rec[q];
          if (o.row >= me.row || o.group != me.group) continue;  // (the edge belongs to the lane of its larger row)
          const double op[3] = {o.x, o.y, o.z};
          if (!(dist2_rn(mp, op) <= r2)) continue;
          if (load_parent(label, o.row) == mine) continue;  // the same parent: one tree already
          mine = unite(label, me.row, o.row, n);
          atomicMin(&label[me.row], mine);  // compression: `mine` was the root of both
          atomicMin(&label[o.row], mine);
        }
      }
}

// label[i] = the root of i; between the two uniting launches (so that a cell united through its first row shows one parent)
// and as the last launch
__global__ __launch_bounds__(kThreads) void rc_flatten_kernel(int32_t* label, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  if (load_parent(label, (int32_t)i) < 0) return;
  atomicMin(&label[i], find_root(label, (int32_t)i, n));
}

static bool rc_shape_ok(int64_t n, int64_t B) { return n >= 0 && n < (1ll << 31) && B >= 1 && B <= kMaxScenes; }

// ---- compaction ----------------------------------------------------------------------------------------------------------------
__device__ inline bool label_ok(int32_t l, int64_t n) { return l >= 0 && l < n; }

__global__ __launch_bounds__(kThreads) void cc_size_kernel(const int32_t* __restrict__ label, int64_t n, int32_t* size) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int32_t l = label[i];
  if (label_ok(l, n)) atomicAdd(&size[l], 1);
}
__global__ __launch_bounds__(kThreads) void cc_flag_kernel(const int32_t* __restrict__ label, int64_t n, const int32_t* __restrict__ size,
                                                           int min_points, int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  flag[i] = (label[i] == i && size[i] >= min_points) ? 1 : 0;
}
// the kept roots, numbered by `id` (the exclusive scan of the flags, in flag's place): their four attributes
__global__ __launch_bounds__(kThreads) void cc_roots_kernel(const int32_t* __restrict__ label, int64_t n, const int32_t* __restrict__ size,
                                                            int min_points, const int32_t* __restrict__ id, const int64_t* __restrict__ offs,
                                                            int B, const int32_t* __restrict__ group, int64_t max_inst,
                                                            int32_t* __restrict__ inst_root, int32_t* __restrict__ inst_size,
                                                            int32_t* __restrict__ inst_scene, int32_t* __restrict__ inst_group) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  if (!(label[i] == i && size[i] >= min_points)) return;
  const int32_t k = id[i];
  if (k >= max_inst) return;
  inst_root[k] = (int32_t)i;
  inst_size[k] = size[i];
  inst_scene[k] = segment_of(offs, B, i);
  inst_group[k] = group ? group[i] : -1;
}
__global__ __launch_bounds__(kThreads) void cc_rows_kernel(const int32_t* __restrict__ label, int64_t n, const int32_t* __restrict__ size,
                                                           int min_points, const int32_t* __restrict__ id, int64_t max_inst,
                                                           int32_t* __restrict__ inst) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int32_t l = label[i];
  int32_t k = -1;
  if (label_ok(l, n) && label[l] == l && size[l] >= min_points && id[l] < max_inst) k = id[l];
  inst[i] = k;
}
// entries [min(count, max_inst), max_inst) of the four attribute arrays: size 0, the others -1
__global__ __launch_bounds__(kThreads) void cc_tail_kernel(const int32_t* __restrict__ count, int64_t max_inst, int32_t* __restrict__ inst_root,
                                                           int32_t* __restrict__ inst_size, int32_t* __restrict__ inst_scene,
                                                           int32_t* __restrict__ inst_group) {
  const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (k >= max_inst || k < *count) return;
  inst_root[k] = inst_scene[k] = inst_group[k] = -1;
  inst_size[k] = 0;
}

// ---- scores, overlap, match, centroids -----------------------------------------------------------------------------------------
// Rows of one instance stand together, so the 64 lanes of a wave mostly hold ONE id: the wave then sums its values with shuffles
// and lane 0 issues the atomics (integer sums: the grouping changes no result).  Every lane of the wave must call.
__device__ inline bool wave_uniform(int32_t key) { return __ballot(key == __shfl(key, 0, 64)) == ~0ull; }
__device__ inline long long wave_sum(long long v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__global__ __launch_bounds__(kThreads) void is_sum_kernel(const float* __restrict__ score, const int32_t* __restrict__ inst, int64_t n, int64_t P,
                                                          unsigned long long* sum) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  int32_t k = i < n ? inst[i] : -1;
  if (k < 0 || k >= P) k = -1;
  long long q = 0;
  if (k >= 0) {
    const float s = score[i];
    const double c = isfinite(s) ? fmin(fmax((double)s, 0.0), 1.0) : 0.0;
    q = (long long)rint(mul_rn(c, kFix));
  }
  if (wave_uniform(k)) {
    q = wave_sum(q);
    if ((threadIdx.x & 63) != 0) return;
  }
  if (k >= 0) atomicAdd(&sum[k], (unsigned long long)q);
}
__global__ __launch_bounds__(kThreads) void is_mean_kernel(const unsigned long long* __restrict__ sum, const int32_t* __restrict__ inst_size,
                                                           int64_t P, double* __restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (k >= P) return;
  const int32_t s = inst_size[k];
  out[k] = s > 0 ? div_rn((double)sum[k], mul_rn((double)s, kFix)) : 0.0;
}

// Rows of one instance stand together, so a wave's lanes mostly hold ONE (pred, gt) pair: its leader then adds the lane count.
__global__ __launch_bounds__(kThreads) void io_count_kernel(const int32_t* __restrict__ pred, const int32_t* __restrict__ gt, int64_t n, int64_t P,
                                                            int64_t G, int32_t* inter, int32_t* pred_size, int32_t* gt_size) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int32_t p = pred[i], g = gt[i];
  const bool pv = p >= 0 && p < P, gv = g >= 0 && g < G;
  const unsigned long long key = ((unsigned long long)(uint32_t)p << 32) | (uint32_t)g;
  const unsigned long long act = __ballot(1);
  const int leader = __ffsll((long long)act) - 1;
  const unsigned long long first = __shfl(key, leader, 64);
  int add = 1;
  if (__ballot(key == first) == act) {
    if ((int)(threadIdx.x & 63) != leader) return;
    add = __popcll(act);
  }
  if (pv) atomicAdd(&pred_size[p], add);
  if (gv) atomicAdd(&gt_size[g], add);
  if (pv && gv) atomicAdd(&inter[(int64_t)p * G + g], add);
}

__global__ __launch_bounds__(kThreads) void im_match_kernel(const int32_t* __restrict__ inter, const int32_t* __restrict__ pred_size,
                                                            const int32_t* __restrict__ gt_size, const int32_t* __restrict__ pred_scene,
                                                            const int32_t* __restrict__ pred_class, const int32_t* __restrict__ gt_scene,
                                                            const int32_t* __restrict__ gt_class, int64_t P, int64_t G,
                                                            int32_t* __restrict__ best_gt, float* __restrict__ best_iou) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= P) return;
  const int32_t sc = pred_scene[p], cl = pred_class[p];
  const int64_t ps = pred_size[p];
  double best = -pinf();
  int32_t arg = -1;
  for (int64_t g = 0; g < G; ++g) {
    if (gt_scene[g] != sc || gt_class[g] != cl) continue;
    const int64_t it = inter[p * G + g], un = ps + (int64_t)gt_size[g] - it;
    const double iou = un > 0 ? div_rn((double)it, (double)un) : 0.0;
    if (iou > best) {  // strict: the lowest index among equal overlaps
      best = iou;
      arg = (int32_t)g;
    }
  }
  best_gt[p] = arg;
  best_iou[p] = (float)best;
}

__global__ __launch_bounds__(kThreads) void ic_sum_kernel(const int32_t* __restrict__ coords, const int32_t* __restrict__ inst, int64_t n, int64_t G,
                                                          unsigned long long* sum, unsigned long long* cnt) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  int32_t k = i < n ? inst[i] : -1;
  if (k < 0 || k >= G) k = -1;
  long long v[4] = {0, 0, 0, k >= 0 ? 1 : 0};  // x, y, z, 1
  if (k >= 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) v[a] = coords[4 * i + 1 + a];
  }
  if (wave_uniform(k)) {  // (as is_sum_kernel)
#pragma unroll
    for (int a = 0; a < 4; ++a) v[a] = wave_sum(v[a]);
    if ((threadIdx.x & 63) != 0) return;
  }
  if (k < 0) return;
#pragma unroll
  for (int a = 0; a < 3; ++a) atomicAdd(&sum[3 * (int64_t)k + a], (unsigned long long)v[a]);
  atomicAdd(&cnt[k], (unsigned long long)v[3]);
}

// ---- offset losses -------------------------------------------------------------------------------------------------------------
constexpr double kEpsV = 1e-6, kEpsN = 1e-8;

struct OffRow {
  double g[3], p[3], gh[3], pn, A;  // gh = g / (|g| + eps), A = |p| + eps
};
__device__ inline OffRow off_row(const float* __restrict__ p, int64_t ld, const float* __restrict__ g, int64_t i) {
  OffRow o;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    o.p[a] = (double)p[ld * i + a];
    o.g[a] = (double)g[3 * i + a];
  }
  const double gn = sqrt((o.g[0] * o.g[0] + o.g[1] * o.g[1]) + o.g[2] * o.g[2]);
  o.pn = sqrt((o.p[0] * o.p[0] + o.p[1] * o.p[1]) + o.p[2] * o.p[2]);
  o.A = o.pn + kEpsN;
#pragma unroll
  for (int a = 0; a < 3; ++a) o.gh[a] = o.g[a] / (gn + kEpsN);
  return o;
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

__global__ __launch_bounds__(kThreads) void ol_partial_kernel(const float* __restrict__ p, int64_t ld, const float* __restrict__ g,
                                                              const int32_t* __restrict__ inst, int64_t n, double* __restrict__ partial) {
  __shared__ double s_wave[kWaves];
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  double t[3] = {0.0, 0.0, 0.0};
  if (i < n && inst[i] >= 0) {
    const OffRow o = off_row(p, ld, g, i);
    t[0] = (fabs(o.p[0] - o.g[0]) + fabs(o.p[1] - o.g[1])) + fabs(o.p[2] - o.g[2]);
    t[1] = -((o.gh[0] * (o.p[0] / o.A) + o.gh[1] * (o.p[1] / o.A)) + o.gh[2] * (o.p[2] / o.A));
    t[2] = 1.0;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double s = block_sum(t[k], s_wave);
    if (threadIdx.x == 0) partial[3 * (int64_t)blockIdx.x + k] = s;
  }
}
// one workgroup: thread t adds the partials t, t + 256, ... in that order, then block_sum
__global__ __launch_bounds__(kThreads) void ol_final_kernel(const double* __restrict__ partial, int64_t n_blocks, double* __restrict__ out3) {
  __shared__ double s_wave[kWaves];
  double t[3] = {0.0, 0.0, 0.0};
  for (int64_t b = threadIdx.x; b < n_blocks; b += kThreads) {
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] += partial[3 * b + k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = block_sum(t[k], s_wave);
  if (threadIdx.x == 0) {
    out3[0] = t[0] / (t[2] + kEpsV);
    out3[1] = t[1] / (t[2] + kEpsV);
    out3[2] = t[2];
  }
}

__global__ __launch_bounds__(kThreads) void ol_bwd_kernel(const float* __restrict__ p, int64_t ld, const float* __restrict__ g,
                                                          const int32_t* __restrict__ inst, int64_t n, const double* __restrict__ out3,
                                                          const double* __restrict__ gloss2, float* __restrict__ dp, int64_t dp_ld) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  double d[3] = {0.0, 0.0, 0.0};
  if (inst[i] >= 0) {
    const double s = out3[2] + kEpsV, gn = gloss2[0] / s, gd = gloss2[1] / s;
    const OffRow o = off_row(p, ld, g, i);
    const double dot = (o.gh[0] * o.p[0] + o.gh[1] * o.p[1]) + o.gh[2] * o.p[2];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double e = o.p[a] - o.g[a];
      const double sg = e > 0.0 ? 1.0 : (e < 0.0 ? -1.0 : 0.0);
      // d/dp of -<gh, p / A>: -(gh / A - <gh, p> (d|p|/dp) / A^2), d|p|/dp = p / |p|, 0 at p = 0
      double dd = o.gh[a] / o.A;
      if (o.pn > 0.0) dd = dd - (dot * (o.p[a] / o.pn)) / (o.A * o.A);
      d[a] = gn * sg + gd * (-dd);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) dp[dp_ld * i + a] = (float)d[a];
}

}  // namespace cluster
}  // namespace pcmi

using namespace pcmi;
using namespace pcmi::cluster;

static unsigned grid_for(int64_t n) { return (unsigned)ceil_div(n, kThreads); }

extern "C" {

// cells of the hash grid
struct RcWs { int64_t cap; uint64_t* keys; int32_t *count, *start; uint32_t* slot_of; Rec* rec; int32_t *sums, *boffs, *total; size_t bytes; };
static RcWs rc_ws(void* ws, int64_t n, int64_t B) {
  const size_t n1 = (size_t)std::max<int64_t>(n, 1);
  Carve cv{(char*)ws};
  RcWs w;
  w.cap = 2 * n + B;
  const size_t nb = (size_t)scan_blocks(w.cap + 1);
  w.keys = cv.take<uint64_t>((size_t)w.cap);
  w.count = cv.take<int32_t>((size_t)w.cap + 1);
  w.start = cv.take<int32_t>((size_t)w.cap + 1);
  w.slot_of = cv.take<uint32_t>(n1);
  w.rec = cv.take<Rec>(n1);
  w.sums = cv.take<int32_t>(nb);
  w.boffs = cv.take<int32_t>(nb);
  w.total = cv.take<int32_t>(1);
  w.bytes = cv.used;
  return w;
}

size_t pcmi_radius_components_workspace_bytes(int64_t n, int64_t B) {
  if (!rc_shape_ok(n, B) || n > kMaxRows) return 0;
  return rc_ws(nullptr, n, B).bytes;
}

int pcmi_radius_components(const float* xyz, int64_t ld, int64_t n, const int64_t* offs, int64_t B, const int32_t* group, double r,
                           int32_t* label, int64_t* dropped, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_REQUIRE(rc_shape_ok(n, B), PCMI_ERR_INVALID, "radius_components: bad shape (0 <= n %lld < 2^31; 1 <= B %lld <= 2^20)", (long long)n,
               (long long)B);
  PCMI_REQUIRE(n <= kMaxRows, PCMI_ERR_UNSUPPORTED, "radius_components: %lld rows, at most 2^29", (long long)n);
  PCMI_REQUIRE(ld >= 3, PCMI_ERR_INVALID, "radius_components: ld %lld < 3", (long long)ld);
  const double h = r * (1.0 + 0x1p-30);
  PCMI_REQUIRE(r > 0.0 && h < __builtin_inf(), PCMI_ERR_INVALID, "radius_components: r must be positive and finite");
  if (n == 0) return PCMI_OK;
  PCMI_REQUIRE(xyz && offs && group && label, PCMI_ERR_INVALID, "radius_components: null pointer");
  if (int rc = require_ws("radius_components", ws, ws_bytes, rc_ws(nullptr, n, B).bytes, 16)) return rc;
  const RcWs L = rc_ws(ws, n, B);
  hipStream_t st = as_stream(stream);
  PCMI_HIP_CHECK(hipMemsetAsync(L.keys, 0xff, (size_t)L.cap * 8, st));
  PCMI_HIP_CHECK(hipMemsetAsync(L.count, 0, (size_t)(L.cap + 1) * 4, st));
  const unsigned grid = grid_for(n);
  rc_count_kernel<<<grid, kThreads, 0, st>>>(xyz, ld, n, offs, (int)B, group, r, h, L.keys, L.count, L.slot_of, label,
                                             reinterpret_cast<unsigned long long*>(dropped));
  PCMI_LAUNCH_CHECK();
  if (int rc = scan_excl(L.count, L.cap + 1, L.start, L.sums, L.boffs, L.total, st)) return rc;
  rc_fill_kernel<<<grid, kThreads, 0, st>>>(xyz, ld, n, group, L.slot_of, L.start, L.count, L.rec);
  PCMI_LAUNCH_CHECK();
  rc_unite_kernel<0><<<grid, kThreads, 0, st>>>(L.rec, L.total, n, offs, (int)B, r, h, L.keys, L.start, label);
  PCMI_LAUNCH_CHECK();
  rc_flatten_kernel<<<grid, kThreads, 0, st>>>(label, n);
  PCMI_LAUNCH_CHECK();
  rc_unite_kernel<1><<<grid, kThreads, 0, st>>>(L.rec, L.total, n, offs, (int)B, r, h, L.keys, L.start, label);
  PCMI_LAUNCH_CHECK();
  rc_flatten_kernel<<<grid, kThreads, 0, st>>>(label, n);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

struct CompactWs { int32_t *size, *id, *sums, *boffs; size_t bytes; };
static CompactWs compact_ws(void* ws, int64_t n) {
  const int64_t m = std::max<int64_t>(n, 1);
  Carve cv{(char*)ws};
  CompactWs w;
  w.size = cv.take<int32_t>((size_t)m);
  w.id = cv.take<int32_t>((size_t)m);
  w.sums = cv.take<int32_t>((size_t)scan_blocks(m));
  w.boffs = cv.take<int32_t>((size_t)scan_blocks(m));
  w.bytes = cv.used;
  return w;
}

size_t pcmi_components_compact_workspace_bytes(int64_t n) {
  if (n < 0 || n >= (1ll << 31)) return 0;
  return compact_ws(nullptr, n).bytes;
}

int pcmi_components_compact(const int32_t* label, const int64_t* offs, int64_t B, int64_t n, const int32_t* group, int min_points,
                            int64_t max_inst, int32_t* inst, int32_t* count, int32_t* inst_root, int32_t* inst_size, int32_t* inst_scene,
                            int32_t* inst_group, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_REQUIRE(rc_shape_ok(n, B) && max_inst >= 0 && max_inst < (1ll << 31) && min_points >= 1, PCMI_ERR_INVALID,
               "components_compact: bad shape (n %lld, B %lld, max_inst %lld, min_points %d)", (long long)n, (long long)B, (long long)max_inst,
               min_points);
  PCMI_REQUIRE(count && (max_inst == 0 || (inst_root && inst_size && inst_scene && inst_group)), PCMI_ERR_INVALID,
               "components_compact: null pointer");
  hipStream_t st = as_stream(stream);
  if (n == 0) {  // nothing to read: no instance
    PCMI_HIP_CHECK(hipMemsetAsync(count, 0, 4, st));
    if (max_inst > 0) {
      cc_tail_kernel<<<grid_for(max_inst), kThreads, 0, st>>>(count, max_inst, inst_root, inst_size, inst_scene, inst_group);
      PCMI_LAUNCH_CHECK();
    }
    return PCMI_OK;
  }
  PCMI_REQUIRE(label && offs && inst, PCMI_ERR_INVALID, "components_compact: null pointer");
  if (int rc = require_ws("components_compact", ws, ws_bytes, compact_ws(nullptr, n).bytes, 1)) return rc;
  const CompactWs w = compact_ws(ws, n);
  const unsigned grid = grid_for(n);
  PCMI_HIP_CHECK(hipMemsetAsync(w.size, 0, (size_t)n * 4, st));
  cc_size_kernel<<<grid, kThreads, 0, st>>>(label, n, w.size);
  PCMI_LAUNCH_CHECK();
  cc_flag_kernel<<<grid, kThreads, 0, st>>>(label, n, w.size, min_points, w.id);
  PCMI_LAUNCH_CHECK();
  if (int rc = scan_excl(w.id, n, w.id, w.sums, w.boffs, count, st)) return rc;
  if (max_inst > 0) {
    cc_roots_kernel<<<grid, kThreads, 0, st>>>(label, n, w.size, min_points, w.id, offs, (int)B, group, max_inst, inst_root, inst_size, inst_scene,
                                               inst_group);
    PCMI_LAUNCH_CHECK();
    cc_tail_kernel<<<grid_for(max_inst), kThreads, 0, st>>>(count, max_inst, inst_root, inst_size, inst_scene, inst_group);
    PCMI_LAUNCH_CHECK();
  }
  cc_rows_kernel<<<grid, kThreads, 0, st>>>(label, n, w.size, min_points, w.id, max_inst, inst);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

size_t pcmi_instance_scores_workspace_bytes(int64_t P) { return P < 0 ? 0 : align_up((size_t)std::max<int64_t>(P, 1) * 8, 256); }

int pcmi_instance_scores(const float* score, const int32_t* inst, int64_t n, int64_t P, const int32_t* inst_size, double* out, void* ws,
                         size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_REQUIRE(n >= 0 && n < (1ll << 31) && P >= 0 && P < (1ll << 31), PCMI_ERR_INVALID, "instance_scores: bad shape (n %lld, P %lld)",
               (long long)n, (long long)P);
  if (P == 0) return PCMI_OK;
  PCMI_REQUIRE(inst_size && out && (n == 0 || (score && inst)), PCMI_ERR_INVALID, "instance_scores: null pointer");
  if (int rc = require_ws("instance_scores", ws, ws_bytes, pcmi_instance_scores_workspace_bytes(P), 8)) return rc;
  hipStream_t st = as_stream(stream);
  unsigned long long* sum = static_cast<unsigned long long*>(ws);
  PCMI_HIP_CHECK(hipMemsetAsync(sum, 0, (size_t)P * 8, st));
  if (n > 0) {
    is_sum_kernel<<<grid_for(n), kThreads, 0, st>>>(score, inst, n, P, sum);
    PCMI_LAUNCH_CHECK();
  }
  is_mean_kernel<<<grid_for(P), kThreads, 0, st>>>(sum, inst_size, P, out);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

int pcmi_instance_overlap(const int32_t* pred_inst, const int32_t* gt_inst, int64_t n, int64_t P, int64_t G, int32_t* inter,
                          int32_t* pred_size, int32_t* gt_size, pcmi_stream_t stream) {
  PCMI_REQUIRE(n >= 0 && n < (1ll << 31) && P >= 0 && G >= 0 && P < (1ll << 31) && G < (1ll << 31) && P * G < (1ll << 31), PCMI_ERR_INVALID,
               "instance_overlap: bad shape (n %lld, P %lld, G %lld; P G < 2^31)", (long long)n, (long long)P, (long long)G);
  PCMI_REQUIRE((P == 0 || pred_size) && (G == 0 || gt_size) && (P * G == 0 || inter) && (n == 0 || (pred_inst && gt_inst)), PCMI_ERR_INVALID,
               "instance_overlap: null pointer");
  hipStream_t st = as_stream(stream);
  if (P > 0) PCMI_HIP_CHECK(hipMemsetAsync(pred_size, 0, (size_t)P * 4, st));
  if (G > 0) PCMI_HIP_CHECK(hipMemsetAsync(gt_size, 0, (size_t)G * 4, st));
  if (P * G > 0) PCMI_HIP_CHECK(hipMemsetAsync(inter, 0, (size_t)(P * G) * 4, st));
  if (n > 0 && (P > 0 || G > 0)) {
    io_count_kernel<<<grid_for(n), kThreads, 0, st>>>(pred_inst, gt_inst, n, P, G, inter, pred_size, gt_size);
    PCMI_LAUNCH_CHECK();
  }
  return PCMI_OK;
}

int pcmi_instance_match(const int32_t* inter, const int32_t* pred_size, const int32_t* gt_size, const int32_t* pred_scene,
                        const int32_t* pred_class, const int32_t* gt_scene, const int32_t* gt_class, int64_t P, int64_t G, int32_t* best_gt,
                        float* best_iou, pcmi_stream_t stream) {
  PCMI_REQUIRE(P >= 0 && G >= 0 && P < (1ll << 31) && G < (1ll << 31) && P * G < (1ll << 31), PCMI_ERR_INVALID,
               "instance_match: bad shape (P %lld, G %lld; P G < 2^31)", (long long)P, (long long)G);
  if (P == 0) return PCMI_OK;
  PCMI_REQUIRE(pred_size && pred_scene && pred_class && best_gt && best_iou && (G == 0 || (inter && gt_size && gt_scene && gt_class)),
               PCMI_ERR_INVALID, "instance_match: null pointer");
  im_match_kernel<<<grid_for(P), kThreads, 0, as_stream(stream)>>>(inter, pred_size, gt_size, pred_scene, pred_class, gt_scene, gt_class, P, G,
                                                                  best_gt, best_iou);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

int pcmi_instance_centroids(const int32_t* coords, const int32_t* inst, int64_t n, int64_t G, int64_t* sum, int64_t* cnt,
                            pcmi_stream_t stream) {
  PCMI_REQUIRE(n >= 0 && n < (1ll << 31) && G >= 0 && G < (1ll << 31), PCMI_ERR_INVALID, "instance_centroids: bad shape (n %lld, G %lld)",
               (long long)n, (long long)G);
  if (G == 0) return PCMI_OK;
  PCMI_REQUIRE(sum && cnt && (n == 0 || (coords && inst)), PCMI_ERR_INVALID, "instance_centroids: null pointer");
  hipStream_t st = as_stream(stream);
  PCMI_HIP_CHECK(hipMemsetAsync(sum, 0, (size_t)G * 24, st));
  PCMI_HIP_CHECK(hipMemsetAsync(cnt, 0, (size_t)G * 8, st));
  if (n > 0) {
    ic_sum_kernel<<<grid_for(n), kThreads, 0, st>>>(coords, inst, n, G, reinterpret_cast<unsigned long long*>(sum),
                                                    reinterpret_cast<unsigned long long*>(cnt));
    PCMI_LAUNCH_CHECK();
  }
  return PCMI_OK;
}

size_t pcmi_offset_loss_workspace_bytes(int64_t n) {
  return n < 0 ? 0 : align_up((size_t)ceil_div(std::max<int64_t>(n, 1), kThreads) * 24, 256);
}

int pcmi_offset_loss_fwd(const float* p, int64_t ld, const float* g, const int32_t* inst, int64_t n, double* out3, void* ws, size_t ws_bytes,
                         pcmi_stream_t stream) {
  PCMI_REQUIRE(n >= 0 && n < (1ll << 31) - kThreads && ld >= 3, PCMI_ERR_INVALID, "offset_loss_fwd: bad shape (n %lld, ld %lld >= 3)",
               (long long)n, (long long)ld);
  PCMI_REQUIRE(out3 && (n == 0 || (p && g && inst)), PCMI_ERR_INVALID, "offset_loss_fwd: null pointer");
  hipStream_t st = as_stream(stream);
  if (n == 0) {  // no valid row: both losses 0 / 1e-6 = 0, V = 0
    PCMI_HIP_CHECK(hipMemsetAsync(out3, 0, 24, st));
    return PCMI_OK;
  }
  if (int rc = require_ws("offset_loss_fwd", ws, ws_bytes, pcmi_offset_loss_workspace_bytes(n), 8)) return rc;
  const int64_t nb = ceil_div(n, kThreads);
  ol_partial_kernel<<<(unsigned)nb, kThreads, 0, st>>>(p, ld, g, inst, n, (double*)ws);
  PCMI_LAUNCH_CHECK();
  ol_final_kernel<<<1, kThreads, 0, st>>>((const double*)ws, nb, out3);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

int pcmi_offset_loss_bwd(const float* p, int64_t ld, const float* g, const int32_t* inst, int64_t n, const double* out3,
                         const double* gloss2, float* dp, int64_t dp_ld, pcmi_stream_t stream) {
  PCMI_REQUIRE(n >= 0 && n < (1ll << 31) - kThreads && ld >= 3 && dp_ld >= 3, PCMI_ERR_INVALID,
               "offset_loss_bwd: bad shape (n %lld, ld %lld, dp_ld %lld >= 3)", (long long)n, (long long)ld, (long long)dp_ld);
  if (n == 0) return PCMI_OK;
  PCMI_REQUIRE(p && g && inst && out3 && gloss2 && dp, PCMI_ERR_INVALID, "offset_loss_bwd: null pointer");
  ol_bwd_kernel<<<grid_for(n), kThreads, 0, as_stream(stream)>>>(p, ld, g, inst, n, out3, gloss2, dp, dp_ld);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

}  // extern "C"
