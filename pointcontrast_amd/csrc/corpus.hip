// Pre-training pair corpus on the device: the geometric part of the reference's offline ScanNet preprocessing
// (pretrain/data_preprocess/scannet_pair/), which turns exported depth frames into the 'pcd' npz files and the
// `fileA fileB overlap` list that ScanNetMatchPairDataset reads --
//   * point_cloud_extractor.py:43-75   back-projection of every depth image to world space
//       -> pcmi_corpus_backproject: all frames of a scene in one launch sequence, compacted in row-major pixel order;
//   * compute_full_overlapping.py:15-26,29-31   open3d voxel_down_sample of every frame
//       -> pcmi_corpus_voxel_centroids: per-frame min bound, a per-frame hash of voxel indices, a stable sort of the
//          points by voxel and an ordered sequential sum per voxel;
//   * compute_full_overlapping.py:63-73   one KD-tree radius query per point for every ORDERED pair of frames, in Python
//       -> pcmi_corpus_overlap_counts: one hash grid of r-sized cells over the centroids of all frames; every query point
//          walks its 27 cells once per block of 64 frames and sets one bit per frame it meets; the bits are summed per
//          workgroup in LDS and land in the integer matrix C with one integer atomic per (workgroup, frame).
// Beyond the reference (its reader.py exports the colour frames, its preprocessing never reads them):
//       -> pcmi_corpus_backproject_color: the colour of every back-projected point, from the frame's colour image through
//          the colour intrinsic and the depth-to-colour extrinsic, in the row order of pcmi_corpus_backproject.
// Everything is integer or exactly-rounded fp64 work with a fixed order (explicit round-to-nearest operations, no FMA
// contraction, IEEE division), so the outputs are bit-identical to the numpy restatement in tests/pair_corpus_ref.py.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "common.h"
#include "cubscan.h"
#include "exact.h"
#include "firstrow.h"
#include "internal.h"

#pragma clang fp contract(off)

namespace pcmi {
namespace corpus {

constexpr int kThreads = 256;
constexpr int kMinChunk = 4096;  // points per workgroup of the min-bound partials

__host__ __device__ inline uint32_t pow2_at_least(int64_t n) {
  uint32_t c = 64;
  while ((int64_t)c < n) c <<= 1;
  return c;
}

// ---- back-projection ---------------------------------------------------------------------------------------------
struct Intrinsic {
  double fx, fy, cx, cy, bx, by;
};

__global__ void bp_flag_kernel(const uint16_t* __restrict__ depth, int64_t n, int32_t* __restrict__ flags) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) flags[k] = depth[k] != 0 ? 1 : 0;
}

// d = depth / shift; X = ((u - cx) * d) / fx + bx; Y = ((v - cy) * d) / fy + by; Z = d;
// w_r = ((X P[r,0] + Y P[r,1]) + Z P[r,2]) + P[r,3]   (point_cloud_extractor.py:58-71, our fixed order)
__global__ void bp_points_kernel(const uint16_t* __restrict__ depth, int64_t n_frames, int64_t height, int64_t width,
                                 Intrinsic K, const double* __restrict__ poses, double shift, const int32_t* __restrict__ pos,
                                 double* __restrict__ points, int32_t* __restrict__ nan_count) {
  const int64_t hw = height * width;
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_frames * hw) return;
  const uint16_t raw = depth[k];
  if (raw == 0) return;
  const int64_t f = k / hw, pix = k - f * hw;
  const double u = (double)(pix % width), v = (double)(pix / width);
  const double d = div_rn((double)raw, shift);
  const double X = add_rn(div_rn(mul_rn(add_rn(u, -K.cx), d), K.fx), K.bx);
  const double Y = add_rn(div_rn(mul_rn(add_rn(v, -K.cy), d), K.fy), K.by);
  const double c[3] = {X, Y, d};
  double w[3];
  rigid_apply(poses + 16 * f, 4, c, w);
  double* o = points + 3 * (int64_t)pos[k];
  o[0] = w[0], o[1] = w[1], o[2] = w[2];
  if (isnan(w[0]) || isnan(w[1]) || isnan(w[2])) atomicAdd(&nan_count[f], 1);
}

// offsets[f] = first output row of frame f (f < F), offsets[F] = total
__global__ void bp_offsets_kernel(const int32_t* __restrict__ flags, const int32_t* __restrict__ pos, int64_t n_frames,
                                  int64_t hw, int64_t* __restrict__ offsets) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f < n_frames) offsets[f] = pos[f * hw];
  if (f == n_frames) offsets[f] = (int64_t)pos[n_frames * hw - 1] + flags[n_frames * hw - 1];
}

// ---- colour of every back-projected point --------------------------------------------------------------------------
struct ColorCamera {
  double fx, fy, cx, cy;
  double M[12];  // rows 0..2 of depth_to_color, row-major
};

// One lane per depth pixel, the compaction of bp_points_kernel (pos = the same exclusive scan), so that colour row k is
// point row k.  The camera-space point of the pixel goes through M into the colour camera and onto its image:
//   q_r = ((X M[r,0] + Y M[r,1]) + Z M[r,2]) + M[r,3], uc = (fxc q0) / q2 + cxc, vc = (fyc q1) / q2 + cyc,
//   px = floor(uc + 0.5), py = floor(vc + 0.5); everything is decided on the doubles, the integers come last.
// Neighbouring lanes read neighbouring depth words and, where the depth has no holes, write neighbouring 3-byte rows
// (a wave's rows are one run of at most 192 bytes); the colour fetch is a gather that follows the image's rows as long
// as the two cameras look the same way.  uncolored[f]: one 64-bit integer add per (wave, frame).
__global__ __launch_bounds__(kThreads) void bp_color_kernel(const uint16_t* __restrict__ depth, int64_t n_frames, int64_t height,
                                                            int64_t width, Intrinsic K, double shift,
                                                            const uint8_t* __restrict__ images, int64_t c_height, int64_t c_width,
                                                            ColorCamera cam, const int32_t* __restrict__ pos,
                                                            uint8_t* __restrict__ color, unsigned long long* uncolored) {
  const int64_t hw = height * width;
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint16_t raw = k < n_frames * hw ? depth[k] : (uint16_t)0;
  const int64_t f = raw != 0 ? k / hw : -1;
  bool miss = false;
  if (raw != 0) {
    const int64_t pix = k - f * hw;
    const double u = (double)(pix % width), v = (double)(pix / width);
    const double d = div_rn((double)raw, shift);
    const double X = add_rn(div_rn(mul_rn(add_rn(u, -K.cx), d), K.fx), K.bx);
    const double Y = add_rn(div_rn(mul_rn(add_rn(v, -K.cy), d), K.fy), K.by);
    const double p[3] = {X, Y, d};
    double q[3];
    rigid_apply(cam.M, 4, p, q);
    const double uc = add_rn(div_rn(mul_rn(cam.fx, q[0]), q[2]), cam.cx);
    const double vc = add_rn(div_rn(mul_rn(cam.fy, q[1]), q[2]), cam.cy);
    const double px = floor(add_rn(uc, 0.5)), py = floor(add_rn(vc, 0.5));
    const bool hit = q[2] > 0.0 && isfinite(uc) && isfinite(vc) && px >= 0.0 && px < (double)c_width && py >= 0.0 && py < (double)c_height;
    uint8_t c[3] = {0, 0, 0};
    if (hit) {
      const uint8_t* src = images + 3 * ((f * c_height + (int64_t)py) * c_width + (int64_t)px);
      c[0] = src[0], c[1] = src[1], c[2] = src[2];
    }
    uint8_t* o = color + 3 * (int64_t)pos[k];
    o[0] = c[0], o[1] = c[1], o[2] = c[2];
    miss = !hit;
  }
  unsigned long long rem = __ballot(miss);  // (all lanes arrive here: nothing returned above)
  while (rem) {
    const int leader = __ffsll((long long)rem) - 1;
    const int lf = __shfl((int)f, leader, 64);  // (n_frames < 2^31)
    const unsigned long long same = __ballot(miss && (int)f == lf);
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&uncolored[lf], (unsigned long long)__popcll(same));
    rem &= ~same;
  }
}

// ---- voxel centroids ---------------------------------------------------------------------------------------------
// partial[f][c] = per-axis minimum of chunk c of frame f (grid: chunks x frames)
__global__ void vc_min_partial_kernel(const double* __restrict__ pts, const int64_t* __restrict__ offsets, int64_t n_chunks,
                                      double* __restrict__ partial) {
  const int64_t f = blockIdx.y, c = blockIdx.x;
  const int64_t b = offsets[f] + c * kMinChunk, e = min(offsets[f + 1], b + kMinChunk);
  double m[3] = {INFINITY, INFINITY, INFINITY};
  for (int64_t i = b + threadIdx.x; i < e; i += blockDim.x)
#pragma unroll
    for (int a = 0; a < 3; ++a) m[a] = fmin(m[a], pts[3 * i + a]);
  __shared__ double red[3][kThreads];
#pragma unroll
  for (int a = 0; a < 3; ++a) red[a][threadIdx.x] = m[a];
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s)
#pragma unroll
      for (int a = 0; a < 3; ++a) red[a][threadIdx.x] = fmin(red[a][threadIdx.x], red[a][threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x < 3) partial[3 * (f * n_chunks + c) + threadIdx.x] = red[threadIdx.x][0];
}

// origin[f] = min_bound - 0.5 voxel; one workgroup per frame.  Also lays out the per-frame hash tables (thread 0 of the
// workgroup of frame 0: a serial prefix over the frames, a few hundred at most).
__global__ void vc_origin_kernel(const double* __restrict__ partial, int64_t n_chunks, double half_voxel,
                                 const int64_t* __restrict__ offsets, int64_t n_frames, double* __restrict__ origin,
                                 uint32_t* __restrict__ tbase, uint32_t* __restrict__ tmask) {
  const int64_t f = blockIdx.x;
  double m[3] = {INFINITY, INFINITY, INFINITY};
  for (int64_t c = threadIdx.x; c < n_chunks; c += blockDim.x)
#pragma unroll
    for (int a = 0; a < 3; ++a) m[a] = fmin(m[a], partial[3 * (f * n_chunks + c) + a]);
  __shared__ double red[3][kThreads];
#pragma unroll
  for (int a = 0; a < 3; ++a) red[a][threadIdx.x] = m[a];
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s)
#pragma unroll
      for (int a = 0; a < 3; ++a) red[a][threadIdx.x] = fmin(red[a][threadIdx.x], red[a][threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x < 3) origin[3 * f + threadIdx.x] = add_rn(red[threadIdx.x][0], -half_voxel);
  if (f == 0 && threadIdx.x == 0) {
    uint32_t base = 0;
    for (int64_t g = 0; g < n_frames; ++g) {
      const uint32_t cap = pow2_at_least(2 * (offsets[g + 1] - offsets[g]));
      tbase[g] = base;
      tmask[g] = cap - 1;
      base += cap;
    }
  }
}

// voxel index floor((p - origin) / voxel) per axis; first[slot] = smallest point index of the voxel (grid: chunks x frames)
__global__ void vc_insert_kernel(const double* __restrict__ pts, const int64_t* __restrict__ offsets,
                                 const double* __restrict__ origin, double voxel, const uint32_t* __restrict__ tbase,
                                 const uint32_t* __restrict__ tmask, uint64_t* keys, uint32_t* first, uint32_t* __restrict__ slot_of,
                                 int32_t* err) {
  const int64_t f = blockIdx.y;
  const int64_t b = offsets[f], e = offsets[f + 1];
  for (int64_t i = b + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < e; i += (int64_t)gridDim.x * blockDim.x) {
    const double d[3] = {add_rn(pts[3 * i], -origin[3 * f]), add_rn(pts[3 * i + 1], -origin[3 * f + 1]), add_rn(pts[3 * i + 2], -origin[3 * f + 2])};
    int64_t c[3];
    if (!cells_of(d, voxel, c)) {
      atomicAdd(err, 1);
      slot_of[i] = kNoSlot;
      continue;
    }
    slot_of[i] = claim_first(keys, tbase[f], tmask[f] + 1, cell_key(c[0], c[1], c[2]), first, i);
  }
}

__global__ void vc_flag_kernel(int64_t n, const uint32_t* __restrict__ first, const uint32_t* __restrict__ slot_of,
                               int32_t* __restrict__ flags, int32_t* __restrict__ iota) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  flags[i] = is_first_row(slot_of[i], first, i) ? 1 : 0;
  iota[i] = (int32_t)i;
}

// vid[i] = output row of the voxel of point i (= number of first occurrences before the voxel's first point)
__global__ void vc_vid_kernel(int64_t n, const uint32_t* __restrict__ first, const uint32_t* __restrict__ slot_of,
                              const int32_t* __restrict__ pos, int32_t* __restrict__ vid) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) vid[i] = pos[first[slot_of[i]]];
}

__global__ void vc_voxel_offsets_kernel(const int32_t* __restrict__ pos, const int64_t* __restrict__ offsets, int64_t n_frames,
                                        int64_t n, int64_t n_vox, int64_t* __restrict__ voxel_offsets) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f <= n_frames) voxel_offsets[f] = offsets[f] < n ? (int64_t)pos[offsets[f]] : n_vox;
}

// start[v] = first row of voxel v in the stably sorted order; start[n_vox] = n
__global__ void vc_starts_kernel(const int32_t* __restrict__ sorted_vid, int64_t n, int64_t n_vox, int32_t* __restrict__ start) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  if (k == 0 || sorted_vid[k] != sorted_vid[k - 1]) start[sorted_vid[k]] = (int32_t)k;
  if (k == n - 1) start[n_vox] = (int32_t)n;
}

// centroid = (((0 + p_a) + p_b) + ...) / count over the voxel's points in ascending index order (the stable sort kept it)
__global__ void vc_centroid_kernel(const double* __restrict__ pts, const int32_t* __restrict__ sorted_idx,
                                   const int32_t* __restrict__ start, int64_t n_vox, double* __restrict__ centroids) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_vox) return;
  const int32_t b = start[v], e = start[v + 1];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  int32_t k = b;
  for (; k + 4 <= e; k += 4) {  // loads issued ahead of the dependent additions, which stay in order
    double q[4][3];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t i = sorted_idx[k + u];
      q[u][0] = pts[3 * i];
      q[u][1] = pts[3 * i + 1];
      q[u][2] = pts[3 * i + 2];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      s0 = add_rn(s0, q[u][0]);
      s1 = add_rn(s1, q[u][1]);
      s2 = add_rn(s2, q[u][2]);
    }
  }
  for (; k < e; ++k) {
    const int64_t i = sorted_idx[k];
    s0 = add_rn(s0, pts[3 * i]);
    s1 = add_rn(s1, pts[3 * i + 1]);
    s2 = add_rn(s2, pts[3 * i + 2]);
  }
  const double cnt = (double)(e - b);
  centroids[3 * v] = div_rn(s0, cnt);
  centroids[3 * v + 1] = div_rn(s1, cnt);
  centroids[3 * v + 2] = div_rn(s2, cnt);
}

// ---- all-pairs overlap counts ------------------------------------------------------------------------------------
__global__ void ov_insert_kernel(const double* __restrict__ pts, const int64_t* __restrict__ offsets, double radius,
                                 uint64_t* keys, int32_t* head, uint32_t mask, int32_t* __restrict__ next,
                                 int32_t* __restrict__ frame_of, int32_t* err) {
  const int64_t f = blockIdx.y;
  const int64_t b = offsets[f], e = offsets[f + 1];
  for (int64_t i = b + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < e; i += (int64_t)gridDim.x * blockDim.x) {
    frame_of[i] = (int32_t)f;
    int64_t c[3];
    if (!cells_of(pts + 3 * i, radius, c)) {
      atomicAdd(err, 1);
      next[i] = -1;
      continue;
    }
    const uint32_t slot = claim_slot(keys, 0, mask + 1, cell_key(c[0], c[1], c[2]));
    next[i] = atomicExch(&head[slot], (int32_t)i);
  }
}

// grid: (chunks of the query frame, query frame j, block t of 64 source frames).  Every query point q of frame j walks
// the 27 cells around it once, sets bit (i - 64 t) for every source frame i of the block that holds a point p with
// ((ex ex + ey ey) + ez ez) <= r r, e = q - p (pcmi_match_radius's test), and adds its bits to the workgroup's 64
// LDS counters; the workgroup then adds them to C[i, j] (one global integer atomic per frame of the block).
__global__ void __launch_bounds__(kThreads) ov_count_kernel(const double* __restrict__ pts, const int64_t* __restrict__ offsets,
                                                            int64_t n_frames, double radius, const uint64_t* __restrict__ keys,
                                                            const int32_t* __restrict__ head, uint32_t mask,
                                                            const int32_t* __restrict__ next,
                                                            const int32_t* __restrict__ frame_of, int32_t* __restrict__ counts) {
  __shared__ int32_t acc[64];
  const int64_t j = blockIdx.y, t0 = (int64_t)blockIdx.z * 64;
  if (threadIdx.x < 64) acc[threadIdx.x] = 0;
  __syncthreads();
  const int64_t b = offsets[j], e = offsets[j + 1];
  const int64_t q_i = b + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t bits = 0;
  if (q_i < e) {
    const double q[3] = {pts[3 * q_i], pts[3 * q_i + 1], pts[3 * q_i + 2]};
    const double r2 = mul_rn(radius, radius);
    int64_t c[3];
    // a query outside the grid's range met no cell: ov_insert_kernel counted it as an error already
    if (cells_of(q, radius, c)) {
      for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx) {
            if (!cell_ok(c[0] + dx, c[1] + dy, c[2] + dz)) continue;
            const int64_t slot = find_slot(keys, 0, mask + 1, cell_key(c[0] + dx, c[1] + dy, c[2] + dz));
            if (slot < 0) continue;
            for (int32_t p = head[slot]; p >= 0; p = next[p]) {
              const int64_t bit = (int64_t)frame_of[p] - t0;
              if (bit < 0 || bit >= 64 || ((bits >> bit) & 1ull)) continue;
              if (dist2_rn(q, pts + 3 * (int64_t)p) <= r2) bits |= 1ull << bit;
            }
          }
    }
    if (j >= t0 && j < t0 + 64) bits &= ~(1ull << (j - t0));  // C[j, j] is not an overlap
  }
  while (bits) {
    const int bit = __builtin_ctzll(bits);
    bits &= bits - 1;
    atomicAdd(&acc[bit], 1);
  }
  __syncthreads();
  if (threadIdx.x < 64 && t0 + threadIdx.x < n_frames && acc[threadIdx.x] != 0)
    atomicAdd(&counts[(t0 + threadIdx.x) * n_frames + j], acc[threadIdx.x]);
}

static size_t sort_bytes(int64_t n) {
  size_t b = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const int32_t*)nullptr, (int32_t*)nullptr, (const int32_t*)nullptr,
                                           (int32_t*)nullptr, (int)std::max<int64_t>(n, 1));
  return b;
}
static int64_t max_frame(const int64_t* offsets_host, int64_t n_frames) {
  int64_t m = 0;
  for (int64_t f = 0; f < n_frames; ++f) m = std::max(m, offsets_host[f + 1] - offsets_host[f]);
  return m;
}
static bool offsets_ok(const int64_t* offsets_host, int64_t n_frames) {
  if (offsets_host[0] != 0) return false;
  for (int64_t f = 0; f < n_frames; ++f)
    if (offsets_host[f + 1] < offsets_host[f]) return false;
  return true;
}
// slots of the per-frame voxel tables: sum over frames of pow2 >= 2 n_f (min 64) <= 4 n + 64 F
static int64_t vc_table_slots(int64_t n, int64_t n_frames) { return 4 * n + 64 * n_frames; }

}  // namespace corpus
}  // namespace pcmi

using namespace pcmi;
using namespace pcmi::corpus;

extern "C" {

// the flags of the valid depth pixels, their scan and its temporary: both backprojections
struct BackprojectWs { int32_t *flags, *pos; void* temp; size_t temp_bytes, bytes; };
static BackprojectWs backproject_ws(void* ws, int64_t n_pixels) {
  const int64_t n = std::max<int64_t>(n_pixels, 1);
  Carve cv{(char*)ws};
  BackprojectWs w;
  w.flags = cv.take<int32_t>((size_t)n);
  w.pos = cv.take<int32_t>((size_t)n);
  w.temp_bytes = cub_scan_bytes<int32_t>(n);
  w.temp = cv.take<char>(w.temp_bytes);
  cv.take<char>(1024);  // (unused tail the query has always counted)
  w.bytes = cv.used;
  return w;
}

size_t pcmi_corpus_backproject_workspace_bytes(int64_t n_frames, int64_t height, int64_t width) {
  return backproject_ws(nullptr, n_frames * height * width).bytes;
}

int pcmi_corpus_backproject(const uint16_t* depth, int64_t n_frames, int64_t height, int64_t width, const double* intrinsic_host,
                            const double* poses, double depth_shift, double* points, int64_t* offsets, int32_t* nan_count,
                            int64_t* offsets_host, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_REQUIRE(n_frames > 0 && height > 0 && width > 0 && n_frames * height * width < (1ll << 31) && intrinsic_host && depth &&
                   poses && points && offsets && nan_count && offsets_host && depth_shift > 0,
               PCMI_ERR_INVALID, "corpus_backproject: bad argument (%lld frames of %lld x %lld)", (long long)n_frames,
               (long long)height, (long long)width);
  const int64_t hw = height * width, n = n_frames * hw;
  if (int rc = require_ws("corpus_backproject", ws, ws_bytes, backproject_ws(nullptr, n).bytes, 1)) return rc;
  hipStream_t st = as_stream(stream);
  const BackprojectWs w = backproject_ws(ws, n);
  const double* A = intrinsic_host;  // 4x4 row-major (intrinsic_depth.txt)
  const Intrinsic K{A[0], A[5], A[2], A[6], A[3], A[7]};
  PCMI_HIP_CHECK(hipMemsetAsync(nan_count, 0, (size_t)n_frames * 4, st));
  const unsigned gn = (unsigned)ceil_div(n, kThreads);
  bp_flag_kernel<<<gn, kThreads, 0, st>>>(depth, n, w.flags);
  PCMI_LAUNCH_CHECK();
  if (int rc = cub_scan_excl(w.temp, w.temp_bytes, w.flags, w.pos, n, st)) return rc;
  bp_points_kernel<<<gn, kThreads, 0, st>>>(depth, n_frames, height, width, K, poses, depth_shift, w.pos, points, nan_count);
  PCMI_LAUNCH_CHECK();
  bp_offsets_kernel<<<(unsigned)ceil_div(n_frames + 1, kThreads), kThreads, 0, st>>>(w.flags, w.pos, n_frames, hw, offsets);
  PCMI_LAUNCH_CHECK();
  PCMI_HIP_CHECK(hipMemcpyAsync(offsets_host, offsets, (size_t)(n_frames + 1) * 8, hipMemcpyDeviceToHost, st));
  PCMI_HIP_CHECK(hipStreamSynchronize(st));
  return PCMI_OK;
}

size_t pcmi_corpus_backproject_color_workspace_bytes(int64_t n_frames, int64_t height, int64_t width) {
  return backproject_ws(nullptr, n_frames * height * width).bytes;
}

int pcmi_corpus_backproject_color(const uint16_t* depth, int64_t n_frames, int64_t height, int64_t width, const double* intrinsic_host,
                                  double depth_shift, const uint8_t* color_images, int64_t color_height, int64_t color_width,
                                  const double* color_intrinsic_host, const double* depth_to_color_host, uint8_t* color,
                                  int64_t* uncolored, int64_t* offsets, int64_t* offsets_host, void* ws, size_t ws_bytes,
                                  pcmi_stream_t stream) {
  PCMI_REQUIRE(n_frames > 0 && height > 0 && width > 0 && n_frames * height * width < (1ll << 31) && intrinsic_host && depth && color &&
                   uncolored && offsets && depth_shift > 0,
               PCMI_ERR_INVALID, "corpus_backproject_color: bad argument (%lld frames of %lld x %lld)", (long long)n_frames,
               (long long)height, (long long)width);
  PCMI_REQUIRE(color_height > 0 && color_width > 0 && color_height < (1ll << 31) && color_width < (1ll << 31) &&
                   n_frames * color_height * color_width < (1ll << 40) && color_images && color_intrinsic_host && depth_to_color_host,
               PCMI_ERR_INVALID, "corpus_backproject_color: bad colour images (%lld frames of %lld x %lld x 3)", (long long)n_frames,
               (long long)color_height, (long long)color_width);
  const int64_t hw = height * width, n = n_frames * hw;
  if (int rc = require_ws("corpus_backproject_color", ws, ws_bytes, backproject_ws(nullptr, n).bytes, 1)) return rc;
  hipStream_t st = as_stream(stream);
  const BackprojectWs w = backproject_ws(ws, n);
  const double *A = intrinsic_host, *Ac = color_intrinsic_host;  // 4x4 row-major (intrinsic_depth.txt, intrinsic_color.txt)
  const Intrinsic K{A[0], A[5], A[2], A[6], A[3], A[7]};
  ColorCamera cam{Ac[0], Ac[5], Ac[2], Ac[6], {}};
  for (int q = 0; q < 12; ++q) cam.M[q] = depth_to_color_host[q];
  PCMI_HIP_CHECK(hipMemsetAsync(uncolored, 0, (size_t)n_frames * 8, st));
  const unsigned gn = (unsigned)ceil_div(n, kThreads);
  bp_flag_kernel<<<gn, kThreads, 0, st>>>(depth, n, w.flags);
  PCMI_LAUNCH_CHECK();
  if (int rc = cub_scan_excl(w.temp, w.temp_bytes, w.flags, w.pos, n, st)) return rc;
  bp_color_kernel<<<gn, kThreads, 0, st>>>(depth, n_frames, height, width, K, depth_shift, color_images, color_height, color_width, cam,
                                           w.pos, color, (unsigned long long*)uncolored);
  PCMI_LAUNCH_CHECK();
  bp_offsets_kernel<<<(unsigned)ceil_div(n_frames + 1, kThreads), kThreads, 0, st>>>(w.flags, w.pos, n_frames, hw, offsets);
  PCMI_LAUNCH_CHECK();
  if (offsets_host) {  // the one wait of pcmi_corpus_backproject; without offsets_host the call does not wait at all
    PCMI_HIP_CHECK(hipMemcpyAsync(offsets_host, offsets, (size_t)(n_frames + 1) * 8, hipMemcpyDeviceToHost, st));
    PCMI_HIP_CHECK(hipStreamSynchronize(st));
  }
  return PCMI_OK;
}

struct CentroidsWs {
  uint64_t* keys;
  uint32_t *first, *slot_of;
  int32_t *flags, *pos, *vid, *iota, *svid, *sidx, *start;
  double *partial, *origin;
  uint32_t *tbase, *tmask;
  int32_t* err;
  void* temp;
  size_t temp_bytes, bytes;
};
// n_chunks: the chunks of the longest frame (the entry, which has the offsets on the host) or a bound on them (the query)
static CentroidsWs centroids_ws(void* ws, int64_t n, int64_t n_frames, int64_t n_chunks) {
  const size_t slots = (size_t)vc_table_slots(n, n_frames);
  Carve cv{(char*)ws};
  CentroidsWs w;
  w.keys = cv.take<uint64_t>(slots);
  w.first = cv.take<uint32_t>(slots);
  w.slot_of = cv.take<uint32_t>((size_t)n);
  w.flags = cv.take<int32_t>((size_t)n);
  w.pos = cv.take<int32_t>((size_t)n);
  w.vid = cv.take<int32_t>((size_t)n);
  w.iota = cv.take<int32_t>((size_t)n);
  w.svid = cv.take<int32_t>((size_t)n);
  w.sidx = cv.take<int32_t>((size_t)n);
  w.start = cv.take<int32_t>((size_t)n + 1);
  w.partial = cv.take<double>((size_t)n_frames * n_chunks * 3);
  w.origin = cv.take<double>((size_t)n_frames * 3);
  w.tbase = cv.take<uint32_t>((size_t)n_frames);
  w.tmask = cv.take<uint32_t>((size_t)n_frames);
  w.err = cv.take<int32_t>(64);
  w.temp_bytes = std::max(cub_scan_bytes<int32_t>(n), sort_bytes(n));
  w.temp = cv.take<char>(w.temp_bytes);
  cv.take<char>(1024);  // (unused tail the query has always counted)
  w.bytes = cv.used;
  return w;
}

size_t pcmi_corpus_voxel_centroids_workspace_bytes(int64_t n_points, int64_t n_frames) {
  const int64_t n = std::max<int64_t>(n_points, 1), F = std::max<int64_t>(n_frames, 1);
  return centroids_ws(nullptr, n, F, ceil_div(n, kMinChunk) + F).bytes;  // a bound on the chunks of any one frame
}

int pcmi_corpus_voxel_centroids(const double* points, const int64_t* offsets, const int64_t* offsets_host, int64_t n_frames,
                                double voxel_size, double* centroids, int64_t* voxel_offsets, int64_t* voxel_offsets_host,
                                void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_REQUIRE(n_frames > 0 && n_frames < 65536 && offsets && offsets_host && centroids && voxel_offsets && voxel_offsets_host && voxel_size > 0,
               PCMI_ERR_INVALID, "corpus_voxel_centroids: bad argument");
  PCMI_REQUIRE(offsets_ok(offsets_host, n_frames), PCMI_ERR_INVALID, "corpus_voxel_centroids: offsets must start at 0 and ascend");
  const int64_t n = offsets_host[n_frames];
  PCMI_REQUIRE(n < (1ll << 29) && (n == 0 || points), PCMI_ERR_INVALID,
               "corpus_voxel_centroids: %lld points (at most 2^29 per call)", (long long)n);
  hipStream_t st = as_stream(stream);
  if (n == 0) {
    for (int64_t f = 0; f <= n_frames; ++f) voxel_offsets_host[f] = 0;
    PCMI_HIP_CHECK(hipMemsetAsync(voxel_offsets, 0, (size_t)(n_frames + 1) * 8, st));
    return PCMI_OK;
  }
  if (int rc = require_ws("corpus_voxel_centroids", ws, ws_bytes, pcmi_corpus_voxel_centroids_workspace_bytes(n, n_frames), 1)) return rc;
  const int64_t mf = max_frame(offsets_host, n_frames), n_chunks = std::max<int64_t>(ceil_div(mf, kMinChunk), 1);
  const size_t slots = (size_t)vc_table_slots(n, n_frames);
  const CentroidsWs w = centroids_ws(ws, n, n_frames, n_chunks);
  void* temp = w.temp;
  const size_t tb = w.temp_bytes;
  PCMI_HIP_CHECK(hipMemsetAsync(w.keys, 0xff, slots * 8, st));
  PCMI_HIP_CHECK(hipMemsetAsync(w.first, 0xff, slots * 4, st));
  PCMI_HIP_CHECK(hipMemsetAsync(w.err, 0, 256, st));
  vc_min_partial_kernel<<<dim3((unsigned)n_chunks, (unsigned)n_frames), kThreads, 0, st>>>(points, offsets, n_chunks, w.partial);
  PCMI_LAUNCH_CHECK();
  vc_origin_kernel<<<(unsigned)n_frames, kThreads, 0, st>>>(w.partial, n_chunks, 0.5 * voxel_size, offsets, n_frames, w.origin,
                                                             w.tbase, w.tmask);
  PCMI_LAUNCH_CHECK();
  const unsigned gx = (unsigned)std::min<int64_t>(ceil_div(mf, kThreads), 1024), gn = (unsigned)ceil_div(n, kThreads);
  vc_insert_kernel<<<dim3(std::max(gx, 1u), (unsigned)n_frames), kThreads, 0, st>>>(points, offsets, w.origin, voxel_size, w.tbase,
                                                                                    w.tmask, w.keys, w.first, w.slot_of, w.err);
  PCMI_LAUNCH_CHECK();
  int32_t herr = 0;
  PCMI_HIP_CHECK(hipMemcpyAsync(&herr, w.err, 4, hipMemcpyDeviceToHost, st));
  PCMI_HIP_CHECK(hipStreamSynchronize(st));
  PCMI_REQUIRE(herr == 0, PCMI_ERR_RANGE,
               "corpus_voxel_centroids: %d points fall outside 2^20 voxels of their frame's min bound (or are not finite)", herr);
  vc_flag_kernel<<<gn, kThreads, 0, st>>>(n, w.first, w.slot_of, w.flags, w.iota);
  PCMI_LAUNCH_CHECK();
  if (int rc = cub_scan_excl(temp, tb, w.flags, w.pos, n, st)) return rc;
  int32_t last[2] = {0, 0};
  PCMI_HIP_CHECK(hipMemcpyAsync(&last[0], w.flags + n - 1, 4, hipMemcpyDeviceToHost, st));
  PCMI_HIP_CHECK(hipMemcpyAsync(&last[1], w.pos + n - 1, 4, hipMemcpyDeviceToHost, st));
  PCMI_HIP_CHECK(hipStreamSynchronize(st));
  const int64_t n_vox = (int64_t)last[0] + last[1];
  vc_vid_kernel<<<gn, kThreads, 0, st>>>(n, w.first, w.slot_of, w.pos, w.vid);
  PCMI_LAUNCH_CHECK();
  vc_voxel_offsets_kernel<<<(unsigned)ceil_div(n_frames + 1, kThreads), kThreads, 0, st>>>(w.pos, offsets, n_frames, n, n_vox,
                                                                                          voxel_offsets);
  PCMI_LAUNCH_CHECK();
  int end_bit = 1;
  while ((1ll << end_bit) < n_vox) ++end_bit;
  size_t tb2 = tb;  // stable LSD radix sort: the points of a voxel keep ascending index order
  PCMI_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(temp, tb2, w.vid, w.svid, w.iota, w.sidx, (int)n, 0, end_bit, st));
  vc_starts_kernel<<<gn, kThreads, 0, st>>>(w.svid, n, n_vox, w.start);
  PCMI_LAUNCH_CHECK();
  vc_centroid_kernel<<<(unsigned)ceil_div(n_vox, kThreads), kThreads, 0, st>>>(points, w.sidx, w.start, n_vox, centroids);
  PCMI_LAUNCH_CHECK();
  PCMI_HIP_CHECK(hipMemcpyAsync(voxel_offsets_host, voxel_offsets, (size_t)(n_frames + 1) * 8, hipMemcpyDeviceToHost, st));
  PCMI_HIP_CHECK(hipStreamSynchronize(st));
  return PCMI_OK;
}

struct OverlapWs { uint64_t* keys; int32_t *head, *next, *frame_of, *err; size_t bytes; };
static OverlapWs overlap_ws(void* ws, int64_t n_points) {
  const int64_t n = std::max<int64_t>(n_points, 1);
  const size_t cap = pow2_at_least(2 * n);
  Carve cv{(char*)ws};
  OverlapWs w;
  w.keys = cv.take<uint64_t>(cap);
  w.head = cv.take<int32_t>(cap);
  w.next = cv.take<int32_t>((size_t)n);
  w.frame_of = cv.take<int32_t>((size_t)n);
  w.err = cv.take<int32_t>(64);
  cv.take<char>(1024);  // (unused tail the query has always counted)
  w.bytes = cv.used;
  return w;
}

size_t pcmi_corpus_overlap_workspace_bytes(int64_t n_points, int64_t n_frames) {
  (void)n_frames;
  return overlap_ws(nullptr, n_points).bytes;
}

int pcmi_corpus_overlap_counts(const double* centroids, const int64_t* offsets, const int64_t* offsets_host, int64_t n_frames,
                               double radius, int32_t* counts, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_REQUIRE(n_frames > 0 && n_frames < 65536 && offsets && offsets_host && counts && radius > 0, PCMI_ERR_INVALID,
               "corpus_overlap_counts: bad argument");
  PCMI_REQUIRE(offsets_ok(offsets_host, n_frames), PCMI_ERR_INVALID, "corpus_overlap_counts: offsets must start at 0 and ascend");
  const int64_t n = offsets_host[n_frames];
  PCMI_REQUIRE(n < (1ll << 30) && (n == 0 || centroids), PCMI_ERR_INVALID,
               "corpus_overlap_counts: %lld points (at most 2^30 per call)", (long long)n);
  hipStream_t st = as_stream(stream);
  PCMI_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)n_frames * n_frames * 4, st));
  if (n == 0) return PCMI_OK;
  if (int rc = require_ws("corpus_overlap_counts", ws, ws_bytes, overlap_ws(nullptr, n).bytes, 1)) return rc;
  const uint32_t cap = pow2_at_least(2 * n);
  const OverlapWs w = overlap_ws(ws, n);
  PCMI_HIP_CHECK(hipMemsetAsync(w.keys, 0xff, (size_t)cap * 8, st));
  PCMI_HIP_CHECK(hipMemsetAsync(w.head, 0xff, (size_t)cap * 4, st));  // -1
  PCMI_HIP_CHECK(hipMemsetAsync(w.err, 0, 256, st));
  const int64_t mf = max_frame(offsets_host, n_frames);
  const unsigned gx = (unsigned)std::max<int64_t>(ceil_div(mf, kThreads), 1);
  ov_insert_kernel<<<dim3(std::min(gx, 1024u), (unsigned)n_frames), kThreads, 0, st>>>(centroids, offsets, radius, w.keys, w.head,
                                                                                      cap - 1, w.next, w.frame_of, w.err);
  PCMI_LAUNCH_CHECK();
  int32_t herr = 0;
  PCMI_HIP_CHECK(hipMemcpyAsync(&herr, w.err, 4, hipMemcpyDeviceToHost, st));
  PCMI_HIP_CHECK(hipStreamSynchronize(st));
  PCMI_REQUIRE(herr == 0, PCMI_ERR_RANGE,
               "corpus_overlap_counts: %d points fall outside +-2^20 cells of size %g (or are not finite)", herr, radius);
  const unsigned tiles = (unsigned)ceil_div(n_frames, 64);
  ov_count_kernel<<<dim3(gx, (unsigned)n_frames, tiles), kThreads, 0, st>>>(centroids, offsets, n_frames, radius, w.keys, w.head,
                                                                           cap - 1, w.next, w.frame_of, counts);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

}  // extern "C"
