// Virtual depth views of a whole scan: which points of a point cloud a pinhole camera would see, for F cameras at once.
// No counterpart in the reference (its pre-training corpus starts from recorded depth frames, csrc/corpus.hip); this is the
// stage in front of pcmi_corpus_voxel_centroids / pcmi_corpus_overlap_counts for users who hold reconstructions only.
//   * pcmi_views_zbuffer: every point through every camera; the float32 depth of a projectable point is the candidate of
//     the pixels its splat window covers, kept with a 32-bit integer atomic minimum on the float's bit pattern (positive
//     floats order as unsigned integers), so the buffer does not depend on the order of execution;
//   * pcmi_views_visible: the same projection again, the point's own pixel compared with the buffer; the 64 verdicts of a
//     wave are one ballot word of a [F, ceil(n / 64)] bitmask, the counts are popcounts and their scan gives every word its
//     first output row;
//   * pcmi_views_rows: the compaction -- lane l of a word writes its point index at the word's first row plus the popcount
//     of the bits below l, so a view's rows ascend and neighbouring lanes write neighbouring rows.
// The arithmetic is fp64 with a fixed order (no FMA contraction, IEEE division), so the outputs are bit-identical to the
// numpy restatement in tests/views_ref.py.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "cubscan.h"
#include "internal.h"

// every product and sum is rounded on its own (see csrc/corpus.hip)
#pragma clang fp contract(off)

namespace pcmi {
namespace views {

constexpr int kThreads = 256;
constexpr int kViewsPerBlock = 8;        // views one workgroup walks with its points in registers
constexpr int kMaxSplat = 7;             // splat windows of 1, 3, 5 or 7 pixels
constexpr int64_t kMaxViews = 4096;      // F
constexpr int64_t kMaxItems = 1ll << 31;  // n, F * H * W and F * ceil(n / 64) stay below this
constexpr uint32_t kEmptyDepth = 0x7f800000u;  // +inf: no point in this pixel

struct Camera {
  double fx, fy, cx, cy, z_near, z_far;
  int height, width;
};

struct Projection {
  bool ok;        // projectable: X, Y, Z finite and z_near <= Z <= z_far
  double px, py;  // floor(u + 0.5), floor(v + 0.5) as doubles: compared before any conversion to an integer
  float zf;       // (float)Z
};

// X = ((x M00 + y M01) + z M02) + M03, Y and Z likewise; u = (X fx) / Z + cx, v = (Y fy) / Z + cy.  M is the same for
// all lanes of a wave (the compiler reads it with scalar loads).
__device__ inline Projection project(const double* __restrict__ M, double x, double y, double z, const Camera& cam) {
  const double X = ((x * M[0] + y * M[1]) + z * M[2]) + M[3];
  const double Y = ((x * M[4] + y * M[5]) + z * M[6]) + M[7];
  const double Z = ((x * M[8] + y * M[9]) + z * M[10]) + M[11];
  Projection p;
  p.ok = isfinite(X) && isfinite(Y) && isfinite(Z) && Z >= cam.z_near && Z <= cam.z_far;
  p.px = p.py = 0.0;
  p.zf = 0.f;
  if (p.ok) {
    const double u = (X * cam.fx) / Z + cam.cx;
    const double v = (Y * cam.fy) / Z + cam.cy;
    p.px = floor(u + 0.5);
    p.py = floor(v + 0.5);
    p.zf = (float)Z;
  }
  return p;
}

// grid: (chunks of kThreads points, groups of kViewsPerBlock views).  A lane keeps its point and walks the group's views.
// The plain read in front of the atomic only skips minima that cannot lower the pixel: depths never rise, so a stale value
// is at least the current one.
__global__ __launch_bounds__(kThreads) void views_zbuffer_kernel(const double* __restrict__ points, int64_t ld, int64_t n,
                                                                 const double* __restrict__ w2c, int n_views, Camera cam,
                                                                 int half, uint32_t* zbuf) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const double x = points[i * ld], y = points[i * ld + 1], z = points[i * ld + 2];
  const int f0 = blockIdx.y * kViewsPerBlock, f1 = min(f0 + kViewsPerBlock, n_views);
  const int H = cam.height, W = cam.width;
  for (int f = f0; f < f1; ++f) {
    const Projection p = project(w2c + 16 * (int64_t)f, x, y, z, cam);
    // the window meets the image (false for a pixel that is not finite)
    if (!(p.ok && p.px >= -(double)half && p.px <= (double)(W - 1) + half && p.py >= -(double)half && p.py <= (double)(H - 1) + half))
      continue;
    const int64_t px = (int64_t)p.px, py = (int64_t)p.py;  // (64-bit: W - 1 + 2 half may pass 2^31)
    const int64_t x0 = max(px - half, (int64_t)0), x1 = min(px + half, (int64_t)W - 1);
    const int64_t y0 = max(py - half, (int64_t)0), y1 = min(py + half, (int64_t)H - 1);
    const uint32_t bits = __float_as_uint(p.zf);
    uint32_t* img = zbuf + (int64_t)f * H * W;
    for (int64_t yy = y0; yy <= y1; ++yy)
      for (int64_t xx = x0; xx <= x1; ++xx) {
        uint32_t* q = img + yy * W + xx;
        if (bits < *(volatile uint32_t*)q) atomicMin(q, bits);
      }
  }
}

// grid as above; every lane stays to the end (the ballot needs the whole wave).  mask[f][w] bit l = point 64 w + l is
// visible in view f; count[f][w] = its popcount.
__global__ __launch_bounds__(kThreads) void views_visible_kernel(const double* __restrict__ points, int64_t ld, int64_t n,
                                                                 const double* __restrict__ w2c, int n_views, Camera cam,
                                                                 double tol, const float* __restrict__ zbuf, int64_t n_words,
                                                                 unsigned long long* __restrict__ mask, int64_t* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < n;
  double x = 0.0, y = 0.0, z = 0.0;
  if (live) x = points[i * ld], y = points[i * ld + 1], z = points[i * ld + 2];
  const int f0 = blockIdx.y * kViewsPerBlock, f1 = min(f0 + kViewsPerBlock, n_views);
  const int H = cam.height, W = cam.width;
  const int64_t word = i >> 6;
  for (int f = f0; f < f1; ++f) {
    bool vis = false;
    if (live) {
      const Projection p = project(w2c + 16 * (int64_t)f, x, y, z, cam);
      if (p.ok && p.px >= 0.0 && p.px < (double)W && p.py >= 0.0 && p.py < (double)H) {
        const float zb = zbuf[((int64_t)f * H + (int)p.py) * W + (int)p.px];
        vis = (double)p.zf <= (double)zb * tol;
      }
    }
    const unsigned long long m = __ballot(vis);
    if ((threadIdx.x & 63) == 0 && word < n_words) {
      mask[(int64_t)f * n_words + word] = m;
      count[(int64_t)f * n_words + word] = __popcll(m);
    }
  }
}

// pixels[f] = pixels of view f that hold a depth; grid: (chunks, views), one 64-bit integer add per wave
__global__ __launch_bounds__(kThreads) void views_pixels_kernel(const uint32_t* __restrict__ zbuf, int64_t hw,
                                                                unsigned long long* pixels) {
  const int64_t f = blockIdx.y;
  int c = 0;
  for (int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x; k < hw; k += (int64_t)gridDim.x * kThreads)
    c += zbuf[f * hw + k] != kEmptyDepth ? 1 : 0;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) c += __shfl_xor(c, s, 64);
  if ((threadIdx.x & 63) == 0 && c != 0) atomicAdd(&pixels[f], (unsigned long long)c);
}

// offsets[f] = first row of view f, offsets[F] = all rows
__global__ void views_offsets_kernel(const int64_t* __restrict__ count, const int64_t* __restrict__ word_start, int64_t n_views,
                                     int64_t n_words, int64_t* __restrict__ offsets) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f < n_views) offsets[f] = word_start[f * n_words];
  if (f == n_views) offsets[f] = word_start[n_views * n_words - 1] + count[n_views * n_words - 1];
}

// grid: (chunks of kThreads points, views)
__global__ __launch_bounds__(kThreads) void views_rows_kernel(const unsigned long long* __restrict__ mask,
                                                              const int64_t* __restrict__ word_start, int64_t n, int64_t n_words,
                                                              int32_t* __restrict__ rows) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int64_t w = (int64_t)blockIdx.y * n_words + (i >> 6);
  const unsigned long long m = mask[w];
  const int lane = (int)(i & 63);
  if ((m >> lane) & 1ull) rows[word_start[w] + __popcll(m & ((1ull << lane) - 1ull))] = (int32_t)i;
}

static bool camera_ok(double fx, double fy, double cx, double cy, double z_near, double z_far) {
  return std::isfinite(fx) && std::isfinite(fy) && std::isfinite(cx) && std::isfinite(cy) && fx > 0 && fy > 0 && z_near > 0 &&
         z_near <= z_far && std::isfinite(z_far);
}

// what both projecting entry points refuse, in one place
static int check_shape(const char* who, int64_t n, int64_t ld, int64_t n_views, int64_t height, int64_t width) {
  PCMI_REQUIRE(n >= 0 && n_views >= 0 && ld >= 3, PCMI_ERR_INVALID, "%s: bad argument (%lld points with row stride %lld, %lld views)",
               who, (long long)n, (long long)ld, (long long)n_views);
  PCMI_REQUIRE(height >= 1 && width >= 1, PCMI_ERR_RANGE, "%s: an image of %lld x %lld pixels", who, (long long)height, (long long)width);
  PCMI_REQUIRE(n < kMaxItems && n_views <= kMaxViews && height < kMaxItems && width < kMaxItems &&
                   std::max<int64_t>(n_views, 1) * height < kMaxItems && std::max<int64_t>(n_views, 1) * height * width < kMaxItems &&
                   std::max<int64_t>(n_views, 1) * ceil_div(std::max<int64_t>(n, 1), 64) < kMaxItems,
               PCMI_ERR_RANGE, "%s: %lld points, %lld views of %lld x %lld (n < 2^31, F <= %lld, F H W < 2^31, F ceil(n / 64) < 2^31)", who,
               (long long)n, (long long)n_views, (long long)height, (long long)width, (long long)kMaxViews);
  return PCMI_OK;
}

}  // namespace views
}  // namespace pcmi

using namespace pcmi;
using namespace pcmi::views;

extern "C" {

int pcmi_views_zbuffer(const double* points, int64_t points_ld, int64_t n, const double* w2c, int64_t n_views, double fx, double fy,
                       double cx, double cy, int64_t height, int64_t width, double z_near, double z_far, int splat, float* zbuf,
                       pcmi_stream_t stream) {
  const int rc = check_shape("views_zbuffer", n, points_ld, n_views, height, width);
  if (rc != PCMI_OK) return rc;
  PCMI_REQUIRE(splat >= 1 && splat <= kMaxSplat && (splat & 1), PCMI_ERR_RANGE, "views_zbuffer: splat %d (odd, 1 ... %d)", splat, kMaxSplat);
  PCMI_REQUIRE(camera_ok(fx, fy, cx, cy, z_near, z_far), PCMI_ERR_INVALID,
               "views_zbuffer: camera (finite fx, fy > 0, finite cx, cy, 0 < z_near <= z_far < inf)");
  if (n_views == 0) return PCMI_OK;
  PCMI_REQUIRE(zbuf && w2c && (n == 0 || points), PCMI_ERR_INVALID, "views_zbuffer: null pointer");
  hipStream_t st = as_stream(stream);
  PCMI_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)zbuf, (int)kEmptyDepth, (size_t)(n_views * height * width), st));
  if (n == 0) return PCMI_OK;
  const Camera cam{fx, fy, cx, cy, z_near, z_far, (int)height, (int)width};
  const dim3 grid((unsigned)ceil_div(n, kThreads), (unsigned)ceil_div(n_views, kViewsPerBlock));
  views_zbuffer_kernel<<<grid, kThreads, 0, st>>>(points, points_ld, n, w2c, (int)n_views, cam, splat / 2, (uint32_t*)zbuf);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

struct VisibleWs { int64_t* count; void* temp; size_t temp_bytes, bytes; };
static VisibleWs visible_ws(void* ws, int64_t n, int64_t n_views) {
  const int64_t items = std::max<int64_t>(n_views, 1) * ceil_div(std::max<int64_t>(n, 1), 64);
  Carve cv{(char*)ws};
  VisibleWs w;
  w.count = cv.take<int64_t>((size_t)items);
  w.temp_bytes = cub_scan_bytes<int64_t>(items);
  w.temp = cv.take<char>(w.temp_bytes);
  cv.take<char>(1024);  // (unused tail the query has always counted)
  w.bytes = cv.used;
  return w;
}

size_t pcmi_views_visible_workspace_bytes(int64_t n, int64_t n_views) { return visible_ws(nullptr, n, n_views).bytes; }

int pcmi_views_visible(const double* points, int64_t points_ld, int64_t n, const double* w2c, int64_t n_views, double fx, double fy,
                       double cx, double cy, int64_t height, int64_t width, double z_near, double z_far, double rel_tol,
                       const float* zbuf, uint64_t* mask, int64_t* word_start, int64_t* offsets, int64_t* offsets_host, int64_t* pixels,
                       void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  const int rc = check_shape("views_visible", n, points_ld, n_views, height, width);
  if (rc != PCMI_OK) return rc;
  PCMI_REQUIRE(camera_ok(fx, fy, cx, cy, z_near, z_far) && rel_tol >= 0 && std::isfinite(rel_tol), PCMI_ERR_INVALID,
               "views_visible: camera (finite fx, fy > 0, finite cx, cy, 0 < z_near <= z_far < inf) or rel_tol %g (finite, >= 0)", rel_tol);
  PCMI_REQUIRE(offsets && offsets_host, PCMI_ERR_INVALID, "views_visible: null pointer");
  hipStream_t st = as_stream(stream);
  if (n == 0 || n_views == 0) {  // empty outputs: every view starts and ends at row 0
    for (int64_t f = 0; f <= n_views; ++f) offsets_host[f] = 0;
    PCMI_HIP_CHECK(hipMemsetAsync(offsets, 0, (size_t)(n_views + 1) * 8, st));
    if (n_views > 0) {
      PCMI_REQUIRE(pixels, PCMI_ERR_INVALID, "views_visible: null pointer");
      PCMI_HIP_CHECK(hipMemsetAsync(pixels, 0, (size_t)n_views * 8, st));
    }
    return PCMI_OK;
  }
  PCMI_REQUIRE(points && w2c && zbuf && mask && word_start && pixels, PCMI_ERR_INVALID, "views_visible: null pointer");
  if (int ws_rc = require_ws("views_visible", ws, ws_bytes, visible_ws(nullptr, n, n_views).bytes, 1)) return ws_rc;
  const int64_t n_words = ceil_div(n, 64), items = n_views * n_words, hw = height * width;
  const VisibleWs w = visible_ws(ws, n, n_views);
  const Camera cam{fx, fy, cx, cy, z_near, z_far, (int)height, (int)width};
  const dim3 grid((unsigned)ceil_div(n, kThreads), (unsigned)ceil_div(n_views, kViewsPerBlock));
  views_visible_kernel<<<grid, kThreads, 0, st>>>(points, points_ld, n, w2c, (int)n_views, cam, 1.0 + rel_tol, zbuf, n_words,
                                                  (unsigned long long*)mask, w.count);
  PCMI_LAUNCH_CHECK();
  if (int scan_rc = cub_scan_excl(w.temp, w.temp_bytes, w.count, word_start, items, st)) return scan_rc;
  views_offsets_kernel<<<(unsigned)ceil_div(n_views + 1, kThreads), kThreads, 0, st>>>(w.count, word_start, n_views, n_words, offsets);
  PCMI_LAUNCH_CHECK();
  PCMI_HIP_CHECK(hipMemsetAsync(pixels, 0, (size_t)n_views * 8, st));
  const dim3 pgrid((unsigned)std::min<int64_t>(ceil_div(hw, kThreads), 64), (unsigned)n_views);
  views_pixels_kernel<<<pgrid, kThreads, 0, st>>>((const uint32_t*)zbuf, hw, (unsigned long long*)pixels);
  PCMI_LAUNCH_CHECK();
  PCMI_HIP_CHECK(hipMemcpyAsync(offsets_host, offsets, (size_t)(n_views + 1) * 8, hipMemcpyDeviceToHost, st));
  PCMI_HIP_CHECK(hipStreamSynchronize(st));
  return PCMI_OK;
}

int pcmi_views_rows(const uint64_t* mask, const int64_t* word_start, int64_t n, int64_t n_views, int32_t* rows, pcmi_stream_t stream) {
  PCMI_REQUIRE(n >= 0 && n_views >= 0, PCMI_ERR_INVALID, "views_rows: bad argument (%lld points, %lld views)", (long long)n,
               (long long)n_views);
  PCMI_REQUIRE(n < kMaxItems && n_views <= kMaxViews && std::max<int64_t>(n_views, 1) * ceil_div(std::max<int64_t>(n, 1), 64) < kMaxItems,
               PCMI_ERR_RANGE, "views_rows: %lld points, %lld views (n < 2^31, F <= %lld, F ceil(n / 64) < 2^31)", (long long)n,
               (long long)n_views, (long long)kMaxViews);
  if (n == 0 || n_views == 0) return PCMI_OK;
  PCMI_REQUIRE(mask && word_start && rows, PCMI_ERR_INVALID, "views_rows: null pointer");
  const dim3 grid((unsigned)ceil_div(n, kThreads), (unsigned)n_views);
  views_rows_kernel<<<grid, kThreads, 0, as_stream(stream)>>>((const unsigned long long*)mask, word_start, n, ceil_div(n, 64), rows);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

}  // extern "C"
