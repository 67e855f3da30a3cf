// Evaluation on the ORIGINAL point cloud (downstream/semseg/lib/test.py:85-93,122-123,190-192 of the reference): what
// save_predictions (lib/utils.py:304-344) and dataset.test_pointcloud (lib/datasets/scannet.py:131-171, stanford.py:41-72) do
// on the host through .npy files, a scipy KD-tree per room and fast_hist --
//   * voxel centres back in world coordinates, inv(T) (x + 0.5, y + 0.5, z + 0.5, 1)            (lib/utils.py:322-327)
//   * the nearest voxel centre of every vertex of the scan, KDTree(leafsize=500).query            (scannet.py:154-155)
//   * fast_hist(pred[nearest], label) and the per-vertex prediction                               (scannet.py:156,168)
// Written from the semantics in include/pcmi.h; gfx950, wave64.
//
// Arithmetic, as loader.hip: every fp64 product and sum is an explicit round-to-nearest operation in a fixed order (no FMA
// contraction), so every output is defined by include/pcmi.h's formulas bit for bit.  The only atomics are integer ones and
// none of them decides a value that leaves: binning order, the order of the fallback list and the order of the confusion
// matrix's additions are all invisible in the outputs.
//
// The stopping bound of the ring walk (nn_query_kernel).  Cells are assigned by t = floor(fl(x / h)) per axis, with |t| <
// kCellLimit < 2^17 for every binned reference and every query that walks the grid.  After the cube of Chebyshev radius r
// around the query's cell c has been searched, a reference OUTSIDE it has, on some axis, t >= c + r + 1 or t <= c - r - 1.
// Take the first: D = fl(x / h) - fl(qx / h) > r, both quotients below 2^17 in magnitude.  A correctly rounded quotient v is
// off by at most 2^-52 |fl(v)| (where it is subnormal, by less than 2^-1074), and |fl(x / h)| <= |fl(qx / h)| + D, so
// x / h - qx / h >= D (1 - 2^-52) - 2^-51 |fl(qx / h)| > r (1 - 2^-52) - 2^-34 > r - 2^-33, that is
// |x - qx| > g = h (r - 2^-33); the other case is the mirror image.  The reference's d2 as the rule
// computes it is then at least g^2 (1 - 2^-53)^5: one rounding of the difference, whose square is rounded once, and two
// rounded additions of non-negative terms, rounding being monotonic.  Relative to (r h)^2 both effects together stay below
// 2^-31, and the bound itself -- fl(fl(r h) fl(r h)) times (1 - 2^-30) -- is computed with three roundings, so
//   bound2(r) = (r h)^2 (1 - 2^-30)  <  d2 of every reference outside the cube       (margin: 2^-30 relative, on d2)
// holds with room to spare, and where the product under- or overflows the comparison below can only fail to stop.  The walk
// stops at radius r only if it HAS a candidate and best_d2 < bound2(r), strictly: nothing outside can then win, nor tie and
// win by its lower row.  Whoever has not stopped after kMaxRing goes to the fallback scan, which is the rule itself.
#include <algorithm>

#include "cubscan.h"
#include "exact.h"
#include "firstrow.h"
#include "internal.h"

#pragma clang fp contract(off)

namespace pcmi {
namespace nearest {

constexpr int kThreads = 256;          // 4 waves: one per SIMD of a CU; up to 8 such workgroups per CU hide the walk's latency
constexpr int kMaxRing = 3;            // largest Chebyshev radius walked on the grid: 7^3 = 343 cells
constexpr int kCellLimit = (1 << 17) - 8;  // |cell index| below this: c +- kMaxRing still fits pack_key's 18-bit fields
constexpr int kMaxScenes = 1024;       // pack_key's 10-bit batch field
constexpr int64_t kMaxRef = 1ll << 29; // table of 2 m slots, scanned with 32-bit counts
constexpr int kMaxClasses = 64;        // as segeval.hip: 64 x 64 x 4 bytes = 16 KB of LDS
constexpr int kFallbackGrid = 2048;    // workgroups of the fallback launch (each walks the list with this stride)

// ---- voxel centres -------------------------------------------------------------------------------------------------------------
constexpr int kMatPerLaunch = 32;  // 32 x 12 doubles = 3 KB of kernel arguments
struct InvT {
  double m[kMatPerLaunch][12];  // the first three rows of each row-major 4 x 4 inverse
};

// rows of scenes [b0, b0 + nb) get their centre; with first != 0 the rows of NO scene (b outside [0, B)) get NaN
__global__ __launch_bounds__(kThreads) void voxel_centers_kernel(const int32_t* __restrict__ coords, int64_t n, InvT T, int b0, int nb,
                                                                 int B, int first, double* __restrict__ centers) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int b = coords[4 * i];
  if (b < 0 || b >= B) {
    if (first) centers[3 * i] = centers[3 * i + 1] = centers[3 * i + 2] = qnan();
    return;
  }
  if (b < b0 || b >= b0 + nb) return;
  const double c[3] = {(double)coords[4 * i + 1] + 0.5, (double)coords[4 * i + 2] + 0.5, (double)coords[4 * i + 3] + 0.5};
  rigid_apply(T.m[b - b0], 4, c, centers + 3 * i);
}

// ---- nearest reference row -----------------------------------------------------------------------------------------------------
struct Rec {  // one binned reference: 32 bytes, two 16-byte loads, the records of a cell contiguous
  double x, y, z;
  int64_t row;
};

// the cell of a finite point; false if an index does not fit the key (or h is no usable cell size)
__device__ inline bool cell_of(double x, double y, double z, double h, int* cx, int* cy, int* cz) {
  if (!(h > 0.0) || !isfinite(h)) return false;
  const double fx = floor(x / h), fy = floor(y / h), fz = floor(z / h), lim = (double)kCellLimit;
  if (!(fabs(fx) < lim && fabs(fy) < lim && fabs(fz) < lim)) return false;
  *cx = (int)fx;
  *cy = (int)fy;
  *cz = (int)fz;
  return true;
}

__device__ inline double cell_size(double cell, const double* cell_dev) { return cell_dev ? *cell_dev : cell; }

// pass 1 over the references: claim the cell's slot and count; a finite row whose cell does not fit marks its scene, whose
// queries then all take the fallback scan (scene_flag); a non-finite row is in no cell
__global__ __launch_bounds__(kThreads) void nn_count_kernel(const double* __restrict__ ref, int64_t m, const int64_t* __restrict__ roffs,
                                                            int B, double cell, const double* __restrict__ cell_dev, uint64_t* keys,
                                                            uint32_t mask, int32_t* count, uint32_t* __restrict__ slot_of,
                                                            int32_t* scene_flag) {
  const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j >= m) return;
  uint32_t slot = kNoSlot;
  const int b = segment_of(roffs, B, j);
  const double x = ref[3 * j], y = ref[3 * j + 1], z = ref[3 * j + 2];
  if (b >= 0 && finite3(x, y, z)) {
    int cx, cy, cz;
    if (cell_of(x, y, z, cell_size(cell, cell_dev), &cx, &cy, &cz)) {
      slot = claim_slot(keys, 0, mask + 1, pack_key(b, cx, cy, cz));
      atomicAdd(&count[slot], 1);
    } else {
      atomicOr(&scene_flag[b], 1);
    }
  }
  slot_of[j] = slot;
}

// pass 2: the row's record into its cell's range [start[slot], start[slot + 1]) (order inside a cell: arbitrary, and immaterial)
__global__ __launch_bounds__(kThreads) void nn_fill_kernel(const double* __restrict__ ref, int64_t m, const uint32_t* __restrict__ slot_of,
                                                           const int32_t* __restrict__ start, int32_t* count, Rec* __restrict__ rec) {
  const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j >= m) return;
  const uint32_t slot = slot_of[j];
  if (slot == kNoSlot) return;
  const int32_t pos = start[slot] + atomicSub(&count[slot], 1) - 1;
  Rec r;
  r.x = ref[3 * j];
  r.y = ref[3 * j + 1];
  r.z = ref[3 * j + 2];
  r.row = j;
  rec[pos] = r;
}

struct Best {
  double d2;
  int64_t row;  // INT64_MAX: none yet
};
__device__ inline void consider(Best& best, double qx, double qy, double qz, double rx, double ry, double rz, int64_t row) {
  const double q[3] = {qx, qy, qz}, r[3] = {rx, ry, rz};
  const double d2 = dist2_rn(q, r);
  if (d2 < best.d2 || (d2 == best.d2 && row < best.row)) {
    best.d2 = d2;
    best.row = row;
  }
}

// One lane per query: the 3^3 cube around its cell, then the shells r = 2 .. kMaxRing, until the bound of the header decides.
// Undecided queries (and those the grid cannot serve: cell out of range, scene marked) append themselves to fb_list.
__global__ __launch_bounds__(kThreads) void nn_query_kernel(const double* __restrict__ query, int64_t n, const int64_t* __restrict__ qoffs,
                                                            const int64_t* __restrict__ roffs, int64_t m, int B, double cell,
                                                            const double* __restrict__ cell_dev, const uint64_t* __restrict__ keys,
                                                            uint32_t mask, const int32_t* __restrict__ start, const Rec* __restrict__ rec,
                                                            const int32_t* __restrict__ scene_flag, int32_t* __restrict__ idx,
                                                            double* __restrict__ dist2, int32_t* fb_count, int32_t* __restrict__ fb_list) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const double qx = query[3 * i], qy = query[3 * i + 1], qz = query[3 * i + 2];
  if (!finite3(qx, qy, qz)) {
    idx[i] = -1;
    if (dist2) dist2[i] = qnan();
    return;
  }
  const int b = segment_of(qoffs, B, i);
  const int64_t lo = b >= 0 ? std::max<int64_t>(roffs[b], 0) : 0, hi = b >= 0 ? std::min<int64_t>(roffs[b + 1], m) : 0;
  if (lo >= hi) {  // no scene, or a scene without references
    idx[i] = -1;
    if (dist2) dist2[i] = pinf();
    return;
  }
  const double h = cell_size(cell, cell_dev);
  int cx, cy, cz;
  bool decided = false;
  Best best{pinf(), INT64_MAX};
  if (scene_flag[b] == 0 && cell_of(qx, qy, qz, h, &cx, &cy, &cz)) {
    for (int r = 1; r <= kMaxRing && !decided; ++r) {
      for (int dz = -r; dz <= r; ++dz)
        for (int dy = -r; dy <= r; ++dy)
          for (int dx = -r; dx <= r; ++dx) {
            if (r > 1 && abs(dx) < r && abs(dy) < r && abs(dz) < r) continue;  // searched at a smaller radius
            const int64_t slot = find_slot(keys, 0, mask + 1, pack_key(b, cx + dx, cy + dy, cz + dz));
            if (slot < 0) continue;
            const int32_t e = start[slot + 1];
            for (int32_t p = start[slot]; p < e; ++p) {
              const Rec c = rec[p];
              consider(best, qx, qy, qz, c.x, c.y, c.z, c.row);
            }
          }
      const double g = mul_rn((double)r, h);
      const double bound2 = mul_rn(mul_rn(g, g), 1.0 - 0x1p-30);
      decided = best.row != INT64_MAX && best.d2 < bound2;
    }
  }
  if (decided) {
    idx[i] = (int32_t)best.row;
    if (dist2) dist2[i] = best.d2;
  } else {
    fb_list[atomicAdd(fb_count, 1)] = (int32_t)i;
  }
}

// One workgroup per listed query: the rule itself over the scene's whole segment, then a min-reduction on (d2, row).
__global__ __launch_bounds__(kThreads) void nn_fallback_kernel(const double* __restrict__ ref, int64_t m, const int64_t* __restrict__ roffs,
                                                               const double* __restrict__ query, const int64_t* __restrict__ qoffs,
                                                               int B, const int32_t* __restrict__ fb_count,
                                                               const int32_t* __restrict__ fb_list, int32_t* __restrict__ idx,
                                                               double* __restrict__ dist2, unsigned long long* fallback_total) {
  __shared__ double s_d2[kThreads / 64];
  __shared__ int64_t s_row[kThreads / 64];
  const int tid = threadIdx.x;
  const int32_t n_fb = *fb_count;
  if (blockIdx.x == 0 && tid == 0 && fallback_total && n_fb > 0) atomicAdd(fallback_total, (unsigned long long)n_fb);
  for (int32_t f = blockIdx.x; f < n_fb; f += gridDim.x) {
    const int64_t i = fb_list[f];
    const double qx = query[3 * i], qy = query[3 * i + 1], qz = query[3 * i + 2];
    const int b = segment_of(qoffs, B, i);  // (listed queries have a scene with references)
    const int64_t lo = std::max<int64_t>(roffs[b], 0), hi = std::min<int64_t>(roffs[b + 1], m);
    Best best{pinf(), INT64_MAX};
    for (int64_t j = lo + tid; j < hi; j += kThreads) {
      const double rx = ref[3 * j], ry = ref[3 * j + 1], rz = ref[3 * j + 2];
      if (finite3(rx, ry, rz)) consider(best, qx, qy, qz, rx, ry, rz, j);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const double od = __shfl_xor(best.d2, d, 64);
      const int64_t orow = __shfl_xor((long long)best.row, d, 64);
      if (od < best.d2 || (od == best.d2 && orow < best.row)) {
        best.d2 = od;
        best.row = orow;
      }
    }
    __syncthreads();  // the previous query's readers are done
    if ((tid & 63) == 0) {
      s_d2[tid >> 6] = best.d2;
      s_row[tid >> 6] = best.row;
    }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < kThreads / 64; ++w)
        if (s_d2[w] < best.d2 || (s_d2[w] == best.d2 && s_row[w] < best.row)) {
          best.d2 = s_d2[w];
          best.row = s_row[w];
        }
      const bool found = best.row != INT64_MAX;  // false: every reference of the scene is non-finite
      idx[i] = found ? (int32_t)best.row : -1;
      if (dist2) dist2[i] = best.d2;
    }
  }
}

// ---- confusion matrix on the point cloud ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void seg_hist_kernel(const int32_t* __restrict__ pred, int64_t m, const int32_t* __restrict__ idx,
                                                            const int32_t* __restrict__ label, int64_t n, int c,
                                                            unsigned long long* __restrict__ hist, int32_t* __restrict__ point_pred,
                                                            unsigned long long* __restrict__ missing) {
  __shared__ int s_hist[kMaxClasses * kMaxClasses];
  __shared__ int s_missing;
  const int tid = threadIdx.x;
  for (int e = tid; e < c * c; e += kThreads) s_hist[e] = 0;
  if (tid == 0) s_missing = 0;
  __syncthreads();
  int miss = 0;
  for (int64_t r = (int64_t)blockIdx.x * kThreads + tid; r < n; r += (int64_t)gridDim.x * kThreads) {
    const int64_t src = idx ? (int64_t)idx[r] : r;
    const bool have = src >= 0 && src < m;
    const int32_t p = have ? pred[src] : -1;
    if (point_pred) point_pred[r] = p;
    miss += have ? 0 : 1;
    const int32_t lb = label[r];
    if (have && lb >= 0 && lb < c && p >= 0 && p < c) atomicAdd(&s_hist[lb * c + p], 1);
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) miss += __shfl_xor(miss, d, 64);
  if ((tid & 63) == 0 && miss) atomicAdd(&s_missing, miss);
  __syncthreads();
  for (int e = tid; e < c * c; e += kThreads) {
    const int v = s_hist[e];
    if (v) atomicAdd(&hist[e], (unsigned long long)v);
  }
  if (tid == 0 && missing && s_missing) atomicAdd(missing, (unsigned long long)s_missing);
}

static bool nn_shape_ok(int64_t m, int64_t n, int64_t B) {
  return m >= 0 && n >= 0 && m < (1ll << 31) && n < (1ll << 31) && B >= 1 && B <= kMaxScenes;
}

}  // namespace nearest
}  // namespace pcmi

using namespace pcmi;
using namespace pcmi::nearest;

extern "C" {

int pcmi_voxel_centers(const int32_t* coords, int64_t n, const double* inv_T_host, int64_t B, double* centers, pcmi_stream_t stream) {
  PCMI_REQUIRE(n >= 0 && n < (1ll << 31) - kThreads && B >= 1 && B < (1ll << 31), PCMI_ERR_INVALID,
               "voxel_centers: bad shape (n %lld, B %lld)", (long long)n, (long long)B);
  if (n == 0) return PCMI_OK;
  PCMI_REQUIRE(coords && inv_T_host && centers, PCMI_ERR_INVALID, "voxel_centers: null pointer");
  hipStream_t st = as_stream(stream);
  for (int64_t b0 = 0; b0 < B; b0 += kMatPerLaunch) {
    const int nb = (int)std::min<int64_t>(kMatPerLaunch, B - b0);
    InvT T;
    for (int s = 0; s < nb; ++s)
      for (int q = 0; q < 12; ++q) T.m[s][q] = inv_T_host[(b0 + s) * 16 + q];
    for (int s = nb; s < kMatPerLaunch; ++s)
      for (int q = 0; q < 12; ++q) T.m[s][q] = 0.0;
    voxel_centers_kernel<<<(unsigned)ceil_div(n, kThreads), kThreads, 0, st>>>(coords, n, T, (int)b0, nb, (int)B, b0 == 0 ? 1 : 0, centers);
    PCMI_LAUNCH_CHECK();
  }
  return PCMI_OK;
}

struct NearestWs {
  uint64_t* keys;
  int32_t *count, *start;
  uint32_t* slot_of;
  Rec* rec;
  int32_t *flags, *fb_list;  // flags: [B] scene flags, then the fallback list's length
  void* temp;
  size_t temp_bytes, bytes;
};
static NearestWs nearest_ws(void* ws, int64_t m, int64_t n, int64_t B) {
  const size_t cap = (size_t)table_cap(m), m1 = (size_t)std::max<int64_t>(m, 1);
  Carve cv{(char*)ws};
  NearestWs w;
  w.keys = cv.take<uint64_t>(cap);
  w.count = cv.take<int32_t>(cap + 1);
  w.start = cv.take<int32_t>(cap + 1);
  w.slot_of = cv.take<uint32_t>(m1);
  w.rec = cv.take<Rec>(m1);
  w.flags = cv.take<int32_t>((size_t)B + 1);
  w.fb_list = cv.take<int32_t>((size_t)std::max<int64_t>(n, 1));
  w.temp_bytes = cub_scan_bytes<int32_t>((int64_t)cap + 1);
  w.temp = cv.take<char>(w.temp_bytes);
  w.bytes = cv.used;
  return w;
}

size_t pcmi_nearest_point_workspace_bytes(int64_t m, int64_t n, int64_t B) {
  if (!nn_shape_ok(m, n, B) || m > kMaxRef) return 0;
  return nearest_ws(nullptr, m, n, B).bytes;
}

int pcmi_nearest_point(const double* ref, const int64_t* ref_offs, int64_t m, const double* query, const int64_t* query_offs, int64_t n,
                       int64_t B, double cell, const double* cell_dev, int32_t* idx, double* dist2, int64_t* fallback_count, void* ws,
                       size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_REQUIRE(nn_shape_ok(m, n, B), PCMI_ERR_INVALID, "nearest_point: bad shape (m %lld, n %lld < 2^31; 1 <= B %lld <= %d)",
               (long long)m, (long long)n, (long long)B, kMaxScenes);
  PCMI_REQUIRE(m <= kMaxRef, PCMI_ERR_UNSUPPORTED, "nearest_point: %lld reference rows, at most 2^29", (long long)m);
  PCMI_REQUIRE(cell_dev || (cell > 0.0 && cell < __builtin_inf()), PCMI_ERR_INVALID, "nearest_point: cell must be positive and finite");
  if (n == 0) return PCMI_OK;
  PCMI_REQUIRE(query && query_offs && ref_offs && idx && (m == 0 || ref), PCMI_ERR_INVALID, "nearest_point: null pointer");
  if (int rc = require_ws("nearest_point", ws, ws_bytes, nearest_ws(nullptr, m, n, B).bytes, 16)) return rc;
  const int64_t cap = table_cap(m);
  const NearestWs w = nearest_ws(ws, m, n, B);
  hipStream_t st = as_stream(stream);
  const uint32_t mask = (uint32_t)(cap - 1);
  PCMI_HIP_CHECK(hipMemsetAsync(w.keys, 0xff, (size_t)cap * 8, st));
  PCMI_HIP_CHECK(hipMemsetAsync(w.count, 0, (size_t)(cap + 1) * 4, st));
  PCMI_HIP_CHECK(hipMemsetAsync(w.flags, 0, (size_t)(B + 1) * 4, st));
  if (m > 0) {
    nn_count_kernel<<<(unsigned)ceil_div(m, kThreads), kThreads, 0, st>>>(ref, m, ref_offs, (int)B, cell, cell_dev, w.keys, mask, w.count, w.slot_of,
                                                                           w.flags);
    PCMI_LAUNCH_CHECK();
  }
  if (int rc = cub_scan_excl(w.temp, w.temp_bytes, w.count, w.start, cap + 1, st)) return rc;
  if (m > 0) {
    nn_fill_kernel<<<(unsigned)ceil_div(m, kThreads), kThreads, 0, st>>>(ref, m, w.slot_of, w.start, w.count, w.rec);
    PCMI_LAUNCH_CHECK();
  }
  nn_query_kernel<<<(unsigned)ceil_div(n, kThreads), kThreads, 0, st>>>(query, n, query_offs, ref_offs, m, (int)B, cell, cell_dev, w.keys, mask,
                                                                         w.start, w.rec, w.flags, idx, dist2, w.flags + B, w.fb_list);
  PCMI_LAUNCH_CHECK();
  nn_fallback_kernel<<<(unsigned)std::min<int64_t>(n, kFallbackGrid), kThreads, 0, st>>>(
      ref, m, ref_offs, query, query_offs, (int)B, w.flags + B, w.fb_list, idx, dist2, reinterpret_cast<unsigned long long*>(fallback_count));
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

int pcmi_seg_hist(const int32_t* pred, int64_t m, const int32_t* idx, const int32_t* labels, int64_t n, int c, int64_t* hist,
                  int32_t* point_pred, int64_t* missing, pcmi_stream_t stream) {
  PCMI_REQUIRE(n >= 0 && n < (1ll << 31) && m >= 0 && m < (1ll << 31) && c >= 1 && c <= kMaxClasses, PCMI_ERR_INVALID,
               "seg_hist: bad shape (m %lld, n %lld, c %d; 1 <= c <= %d)", (long long)m, (long long)n, c, kMaxClasses);
  if (n == 0) return PCMI_OK;
  PCMI_REQUIRE(labels && hist && (m == 0 || pred), PCMI_ERR_INVALID, "seg_hist: null pointer");
  seg_hist_kernel<<<(unsigned)std::min<int64_t>(ceil_div(n, kThreads), 4 * num_cu()), kThreads, 0, as_stream(stream)>>>(
      pred, m, idx, labels, n, c, reinterpret_cast<unsigned long long*>(hist), point_pred, reinterpret_cast<unsigned long long*>(missing));
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

}  // extern "C"
