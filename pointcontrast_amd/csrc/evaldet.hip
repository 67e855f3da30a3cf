// The scoring of the detection evaluation (downstream/votenet_det_new of the reference): the oriented box overlap of
// lib/utils/box_util.py:92-117 (box3d_iou), the matching loop of lib/utils/eval_det.py:126-139 for a whole batch, and the
// true-positive rule, precision / recall curves and both voc_ap forms of :24-55 and :142-159 for every class and any number
// of overlap thresholds from ONE match.  Written from the semantics in include/pcmi.h; gfx950, wave64.
//
// Arithmetic: the overlaps are float32, every operation rounded on its own (contraction off for the whole file); the counts
// are integers; recall, precision and AP are float64 on those integers, summed in a fixed order.  No float atomics: the only
// atomic is the integer minimum that elects the best-ranked candidate of a ground-truth box, so every output is reproducible
// bit for bit.
#include <algorithm>

#include "blockscan.h"
#include "internal.h"

#pragma clang fp contract(off)

namespace pcmi {
namespace evaldet {

// ---- oriented overlap ---------------------------------------------------------------------------------------------------------
// A polygon of the clipping: a quadrilateral cut by four half planes has at most 8 vertices.  Every loop over it is unrolled
// to constant indices and every dynamic position is a chain of selects, so the polygons live in registers (no scratch).  An
// append beyond kMaxVerts -- only rounding in the strict inside test could ask for one -- is dropped, never written.
constexpr int kMaxVerts = 8;

struct Poly {
  float x[kMaxVerts], y[kMaxVerts];
  int n;
};

__device__ __forceinline__ void poly_push(Poly& p, float x, float y) {
#pragma unroll
  for (int k = 0; k < kMaxVerts; ++k) {
    const bool here = k == p.n;
    p.x[k] = here ? x : p.x[k];
    p.y[k] = here ? y : p.y[k];
  }
  p.n = p.n < kMaxVerts ? p.n + 1 : p.n;
}

__device__ __forceinline__ void poly_last(const Poly& p, float* x, float* y) {
  float lx = p.x[0], ly = p.y[0];
#pragma unroll
  for (int k = 1; k < kMaxVerts; ++k) {
    const bool here = k == p.n - 1;
    lx = here ? p.x[k] : lx;
    ly = here ? p.y[k] : ly;
  }
  *x = lx;
  *y = ly;
}

// 0.5 |sum x_i y_{i-1} - y_i x_{i-1}| (poly_area of box_util.py:64-66), in vertex order
__device__ __forceinline__ float poly_area(const Poly& p) {
  float px, py, a = 0.f, b = 0.f;
  poly_last(p, &px, &py);
#pragma unroll
  for (int i = 0; i < kMaxVerts; ++i) {
    if (i < p.n) {
      a = a + (p.x[i] * py);
      b = b + (p.y[i] * px);
    }
    px = p.x[i];
    py = p.y[i];
  }
  return 0.5f * fabsf(a - b);
}

__device__ __forceinline__ float edge_len(const float* p, const float* q) {
  const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
  return sqrtf(((dx * dx) + (dy * dy)) + (dz * dz));
}

// c1, c2: 8 corners x 3 floats in get_3d_box's order.  The bird's-eye-view rectangles are the corners 3, 2, 1, 0 as (x, z);
// rect1 is the subject and rect2 the clip polygon, as convex_hull_intersection(rect1, rect2) passes them.  Both are moved by
// the same vector (corner 3 of box 1 to the origin) first: the shoelace sums and the line intersections cancel absolute
// coordinates, and a 5 cm box three metres from the origin would otherwise lose three digits of its area.
__device__ void iou_pair(const float* __restrict__ c1, const float* __restrict__ c2, float* iou3d, float* iou2d) {
  const float ox = c1[9], oz = c1[11];
  Poly cur, clip;
  cur.n = clip.n = 4;
#pragma unroll
  for (int i = 0; i < kMaxVerts; ++i) {
    const int src = 3 * (3 - (i & 3));
    cur.x[i] = i < 4 ? c1[src] - ox : 0.f;
    cur.y[i] = i < 4 ? c1[src + 2] - oz : 0.f;
    clip.x[i] = i < 4 ? c2[src] - ox : 0.f;
    clip.y[i] = i < 4 ? c2[src + 2] - oz : 0.f;
  }
  const float area1 = poly_area(cur), area2 = poly_area(clip);
  // Sutherland-Hodgman (polygon_clip, box_util.py:16-62): the same vertex order, the same strict inside test, the same
  // intersection formula; an empty list after any clip edge is the reference's None
  float cp1x = clip.x[3], cp1y = clip.y[3];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float cp2x = clip.x[e], cp2y = clip.y[e];
    if (cur.n > 0) {
      const float ex = cp2x - cp1x, ey = cp2y - cp1y;
      const float dcx = cp1x - cp2x, dcy = cp1y - cp2y;
      const float n1 = (cp1x * cp2y) - (cp1y * cp2x);
      Poly nxt;
      nxt.n = 0;
#pragma unroll
      for (int k = 0; k < kMaxVerts; ++k) nxt.x[k] = nxt.y[k] = 0.f;
      float sx, sy;
      poly_last(cur, &sx, &sy);
      bool s_in = (ex * (sy - cp1y)) > (ey * (sx - cp1x));
#pragma unroll
      for (int v = 0; v < kMaxVerts; ++v) {
        if (v < cur.n) {
          const float vx = cur.x[v], vy = cur.y[v];
          const bool e_in = (ex * (vy - cp1y)) > (ey * (vx - cp1x));
          if (e_in != s_in) {
            const float dpx = sx - vx, dpy = sy - vy;
            const float n2 = (sx * vy) - (sy * vx);
            const float n3 = 1.0f / ((dcx * dpy) - (dcy * dpx));
            poly_push(nxt, ((n1 * dpx) - (n2 * dcx)) * n3, ((n1 * dpy) - (n2 * dcy)) * n3);
          }
          if (e_in) poly_push(nxt, vx, vy);
          sx = vx;
          sy = vy;
          s_in = e_in;
        }
      }
      cur = nxt;
    }
    cp1x = cp2x;
    cp1y = cp2y;
  }
  // the polygon is convex, so its shoelace area is the area of its hull (ConvexHull(...).volume)
  const float inter_area = cur.n > 0 ? poly_area(cur) : 0.f;
  if (iou2d) *iou2d = inter_area / ((area1 + area2) - inter_area);
  const float ymax = fminf(c1[1], c2[1]), ymin = fmaxf(c1[13], c2[13]);
  const float inter_vol = inter_area * fmaxf(0.f, ymax - ymin);
  const float vol1 = (edge_len(c1, c1 + 3) * edge_len(c1 + 3, c1 + 6)) * edge_len(c1, c1 + 12);
  const float vol2 = (edge_len(c2, c2 + 3) * edge_len(c2 + 3, c2 + 6)) * edge_len(c2, c2 + 12);
  *iou3d = inter_vol / ((vol1 + vol2) - inter_vol);
}

// One thread per pair of the flat [n m] matrix: neighbouring lanes share the row box (one broadcast load) and read
// consecutive column boxes.
__global__ __launch_bounds__(256) void box3d_iou_kernel(const float* __restrict__ c1, const float* __restrict__ c2, int64_t n, int64_t m,
                                                        float* __restrict__ iou3d, float* __restrict__ iou2d) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n * m) return;
  const int64_t i = p / m, j = p - i * m;
  float o3, o2;
  iou_pair(c1 + i * 24, c2 + j * 24, &o3, &o2);
  iou3d[p] = o3;
  if (iou2d) iou2d[p] = o2;
}

// ---- matching -----------------------------------------------------------------------------------------------------------------
// grid (tile of kMatchTile predicted boxes, scene).  (1) the threads take the tile's [kMatchTile, G] pairs and leave the
// overlaps in LDS -- every pair once, whatever the number of classes; (2) the threads take the tile's [kMatchTile, Cls]
// entries and scan the scene's boxes of their class in ascending index with strict >, so the lowest index of equal overlaps
// wins, as the reference's loop.  A masked box, or one whose class is outside [0, Cls), belongs to no class.
constexpr int kMatchMaxK = 1024;  // predicted boxes per scene (as the NMS)
constexpr int kMatchMaxG = 256;   // ground-truth boxes per scene (ScanNet labels at most 64)
constexpr int kMatchTile = 32;
constexpr int kMatchThreads = 256;

__global__ __launch_bounds__(kMatchThreads) void det_match_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                  const int32_t* __restrict__ gt_cls, const int32_t* __restrict__ gt_mask,
                                                                  int K, int G, int Cls, int32_t* __restrict__ best_gt,
                                                                  float* __restrict__ best_iou) {
  __shared__ float s_iou[kMatchTile * kMatchMaxG];
  __shared__ int32_t s_cls[kMatchMaxG];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.y;
  const int k0 = blockIdx.x * kMatchTile;
  const int kn = min(kMatchTile, K - k0);
  for (int g = tid; g < G; g += kMatchThreads) {
    const int32_t c = gt_cls[b * G + g];
    s_cls[g] = (gt_mask[b * G + g] != 0 && c >= 0 && c < Cls) ? c : -1;
  }
  __syncthreads();
  for (int p = tid; p < kn * G; p += kMatchThreads) {
    const int k = p / G, g = p - k * G;
    float o = 0.f;
    if (s_cls[g] >= 0) iou_pair(pred + (b * K + k0 + k) * 24, gt + (b * G + g) * 24, &o, nullptr);
    s_iou[p] = o;
  }
  __syncthreads();
  for (int e = tid; e < kn * Cls; e += kMatchThreads) {
    const int k = e / Cls, c = e - k * Cls;
    float best = -INFINITY;
    int bi = -1;
    for (int g = 0; g < G; ++g) {
      const float o = s_iou[k * G + g];
      if (s_cls[g] == c && o > best) {
        best = o;
        bi = g;
      }
    }
    const int64_t at = (b * K + k0) * Cls + e;
    best_gt[at] = bi;
    best_iou[at] = best;
  }
}

// ---- true positives, curves, AP -----------------------------------------------------------------------------------------------
constexpr int kApMaxThresholds = 16;
constexpr int kApThreads = 256;
constexpr int kApItems = 4;
constexpr int kApChunk = kApThreads * kApItems;  // detections one pass of the workgroup covers
constexpr int32_t kNoClaim = 0x7f7f7f7f;         // what hipMemsetAsync(0x7f) leaves: above every rank

struct ApThresholds {
  double t[kApMaxThresholds];
};

__device__ __forceinline__ bool ap_candidate(const float* __restrict__ best_iou, const int32_t* __restrict__ gt_id, int64_t d,
                                             int64_t n_gt, double thr) {
  const int32_t g = gt_id[d];
  return g >= 0 && g < n_gt && (double)best_iou[d] > thr;
}

// grid (detection tile, threshold): a candidate bids its rank -- its position in the class-major, confidence-descending list
// -- for its ground-truth box; the integer minimum is the sequential "first to claim" rule.
__global__ __launch_bounds__(256) void ap_claim_kernel(const float* __restrict__ best_iou, const int32_t* __restrict__ gt_id, int64_t nd,
                                                       int64_t n_gt, ApThresholds thr, int32_t* __restrict__ claim) {
  const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (d >= nd) return;
  const int t = blockIdx.y;
  if (ap_candidate(best_iou, gt_id, d, n_gt, thr.t[t])) atomicMin(&claim[(int64_t)t * n_gt + gt_id[d]], (int32_t)d);
}

// grid (class, threshold), one workgroup each, over the class's detections [offs[c], offs[c + 1]) in rank order.
// Forward pass, kApChunk detections at a time with a carry (so a class may hold any number of them): tp flag = "my bid won",
// inclusive count of true positives -> tp_cum (workspace), rec / prec / flags on request.  Backward pass, again in chunks
// with a carry: the precision envelope (running maximum from the end) and, per thread, the terms
// (rec_i - rec_{i-1}) envelope_i of the detections where recall changes, then one tree sum in a fixed order.
// recall = tp / npos is IEEE: a class without ground truth gives 0 / 0 = NaN in every term, as the reference.
__global__ __launch_bounds__(kApThreads) void ap_curve_kernel(const int32_t* __restrict__ gt_id, const int32_t* __restrict__ cls_offs,
                                                              const int32_t* __restrict__ npos, const int32_t* __restrict__ claim,
                                                              int64_t nd, int64_t n_gt, int Cls, int use_07, int32_t* __restrict__ tp_cum,
                                                              double* __restrict__ ap, double* __restrict__ last_rec,
                                                              double* __restrict__ rec, double* __restrict__ prec,
                                                              int32_t* __restrict__ tp_flag) {
  __shared__ int s_int[kApThreads / 64];
  __shared__ double s_dbl[kApThreads / 64];
  __shared__ double s_sum[kApThreads];
  __shared__ double s_p11[11];
  const int tid = threadIdx.x;
  const int c = blockIdx.x, t = blockIdx.y;
  const int64_t o0 = cls_offs[c], o1 = cls_offs[c + 1];
  const int64_t start = o0 < 0 ? 0 : (o0 > nd ? nd : o0);  // a table that is not a partition of [0, nd) reads nothing outside
  const int64_t end = o1 < start ? start : (o1 > nd ? nd : o1);
  const int64_t n = end - start;
  const double np = (double)npos[c];
  const int32_t* cl = claim + (int64_t)t * n_gt;
  const int64_t row = (int64_t)t * nd;

  int carry = 0;
  for (int64_t base = 0; base < n; base += kApChunk) {
    int f[kApItems], local = 0;
#pragma unroll
    for (int q = 0; q < kApItems; ++q) {
      const int64_t i = base + (int64_t)tid * kApItems + q;
      f[q] = 0;
      if (i < n) {
        const int64_t d = start + i;
        const int32_t g = gt_id[d];
        f[q] = (g >= 0 && g < n_gt && (int64_t)cl[g] == d) ? 1 : 0;
      }
      local += f[q];
    }
    int total;
    int run = carry + block_scan_add<kApThreads / 64>(local, s_int, &total) - local;
#pragma unroll
    for (int q = 0; q < kApItems; ++q) {
      const int64_t i = base + (int64_t)tid * kApItems + q;
      if (i >= n) break;
      run += f[q];
      const int64_t d = start + i;
      tp_cum[row + d] = run;
      if (tp_flag) tp_flag[row + d] = f[q];
      if (rec) rec[row + d] = (double)run / np;
      if (prec) prec[row + d] = (double)run / fmax((double)(i + 1), 2.220446049250313e-16);
    }
    carry += total;
  }
  if (tid == 0) last_rec[t * Cls + c] = n > 0 ? (double)carry / np : 0.0;
  __syncthreads();  // tp_cum of this class is read back below by other threads of the workgroup

  double sum = 0.0, env_carry = 0.0;
  double p11[11];
#pragma unroll
  for (int k = 0; k < 11; ++k) p11[k] = 0.0;
  const int64_t n_chunks = (n + kApChunk - 1) / kApChunk;
  for (int64_t ch = n_chunks - 1; ch >= 0; --ch) {
    const int64_t base = ch * kApChunk;
    double pr[kApItems], local = 0.0;
    int tc[kApItems];
#pragma unroll
    for (int q = kApItems - 1; q >= 0; --q) {
      const int64_t i = base + (int64_t)tid * kApItems + q;
      pr[q] = 0.0;
      tc[q] = 0;
      if (i < n) {
        tc[q] = tp_cum[row + start + i];
        pr[q] = (double)tc[q] / fmax((double)(i + 1), 2.220446049250313e-16);
      }
      local = fmax(local, pr[q]);
    }
    double all;
    // the envelope behind this thread's items: the threads after it in the chunk and everything in the later chunks
    double env = fmax(env_carry, block_rscan_max_excl<kApThreads / 64>(local, s_dbl, &all));
#pragma unroll
    for (int q = kApItems - 1; q >= 0; --q) {
      const int64_t i = base + (int64_t)tid * kApItems + q;
      if (i >= n) continue;
      env = fmax(env, pr[q]);
      const int prev = (q > 0) ? tc[q - 1] : ((i > 0) ? tp_cum[row + start + i - 1] : 0);
      const double r = (double)tc[q] / np, r0 = (i > 0) ? (double)prev / np : 0.0;
      if (r != r0) sum = sum + ((r - r0) * env);
      if (use_07) {
#pragma unroll
        for (int k = 0; k < 11; ++k)
          if (r >= (double)k * 0.1) p11[k] = fmax(p11[k], pr[q]);
      }
    }
    env_carry = fmax(env_carry, all);
  }
  // the closing sentinel pair (recall 1, precision 0) adds (1 - last recall) * 0: nothing, and NaN where recall is NaN already
  s_sum[tid] = sum;
  __syncthreads();
  for (int o = kApThreads / 2; o > 0; o >>= 1) {
    if (tid < o) s_sum[tid] = s_sum[tid] + s_sum[tid + o];
    __syncthreads();
  }
  if (!use_07) {
    if (tid == 0) ap[t * Cls + c] = s_sum[0];
    return;
  }
  // 11-point form: p_k = the largest precision among the detections with recall >= k / 10 (0 if none), ap = sum p_k / 11
  for (int k = 0; k < 11; ++k) {
    __syncthreads();
    s_sum[tid] = p11[k];
    __syncthreads();
    for (int o = kApThreads / 2; o > 0; o >>= 1) {
      if (tid < o) s_sum[tid] = fmax(s_sum[tid], s_sum[tid + o]);
      __syncthreads();
    }
    if (tid == 0) s_p11[k] = s_sum[0];
  }
  if (tid == 0) {
    double a = 0.0;
    for (int k = 0; k < 11; ++k) a = a + s_p11[k] / 11.0;
    ap[t * Cls + c] = a;
  }
}

static bool ap_shape_ok(int64_t nd, int64_t n_gt, int Cls, int T) {
  return nd >= 0 && n_gt >= 0 && Cls >= 1 && Cls <= 65535 && T >= 1 && T <= kApMaxThresholds && nd < (int64_t)kNoClaim &&
         n_gt < (1ll << 31);
}

}  // namespace evaldet
}  // namespace pcmi

using namespace pcmi;
using namespace pcmi::evaldet;

extern "C" {

int pcmi_box3d_iou(const float* corners1, const float* corners2, int64_t n, int64_t m, float* iou3d, float* iou2d,
                   pcmi_stream_t stream) {
  PCMI_REQUIRE(n >= 0 && m >= 0 && n < (1ll << 31) / 24 && m < (1ll << 31) / 24 && (n == 0 || m < (1ll << 40) / n), PCMI_ERR_INVALID,
               "box3d_iou: bad shape (n %lld, m %lld)", (long long)n, (long long)m);
  if (n * m == 0) return PCMI_OK;
  PCMI_REQUIRE(corners1 && corners2 && iou3d, PCMI_ERR_INVALID, "box3d_iou: null pointer");
  box3d_iou_kernel<<<(unsigned)ceil_div(n * m, 256), 256, 0, as_stream(stream)>>>(corners1, corners2, n, m, iou3d, iou2d);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

int pcmi_det_match(const float* pred_corners, const float* gt_corners, const int32_t* gt_cls, const int32_t* gt_mask, int64_t B,
                   int64_t K, int64_t G, int Cls, int32_t* best_gt, float* best_iou, pcmi_stream_t stream) {
  PCMI_REQUIRE(B >= 0 && K >= 0 && G >= 0 && Cls >= 1 && Cls <= 65535 && B <= 65535, PCMI_ERR_INVALID,
               "det_match: bad shape (B %lld, K %lld, G %lld, Cls %d)", (long long)B, (long long)K, (long long)G, Cls);
  PCMI_REQUIRE(K <= kMatchMaxK && G <= kMatchMaxG, PCMI_ERR_UNSUPPORTED,
               "det_match: %lld predicted and %lld ground-truth boxes per scene, at most %d and %d are supported", (long long)K,
               (long long)G, kMatchMaxK, kMatchMaxG);
  if (B * K == 0) return PCMI_OK;
  PCMI_REQUIRE(pred_corners && best_gt && best_iou && (G == 0 || (gt_corners && gt_cls && gt_mask)), PCMI_ERR_INVALID,
               "det_match: null pointer");
  det_match_kernel<<<dim3((unsigned)ceil_div(K, kMatchTile), (unsigned)B), kMatchThreads, 0, as_stream(stream)>>>(
      pred_corners, gt_corners, gt_cls, gt_mask, (int)K, (int)G, Cls, best_gt, best_iou);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

struct ApWs { int32_t *claim, *tp_cum; size_t bytes; };
static ApWs ap_ws(void* ws, int64_t nd, int64_t n_gt, int n_thresholds) {
  Carve cv{(char*)ws};
  ApWs w;
  w.claim = cv.take<int32_t>((size_t)n_thresholds * (size_t)n_gt);
  cv.align = 1;  // the last piece is not padded
  w.tp_cum = cv.take<int32_t>((size_t)n_thresholds * (size_t)nd);
  w.bytes = cv.used;
  return w;
}

size_t pcmi_det_ap_workspace_bytes(int64_t nd, int64_t n_gt, int n_thresholds) {
  if (!ap_shape_ok(nd, n_gt, 1, n_thresholds)) return 0;
  return ap_ws(nullptr, nd, n_gt, n_thresholds).bytes;
}

int pcmi_det_ap(const float* best_iou, const int32_t* gt_id, const int32_t* cls_offs, const int32_t* npos, int64_t nd, int64_t n_gt,
                int Cls, const double* thresholds, int n_thresholds, int use_07_metric, double* ap, double* last_rec, double* rec,
                double* prec, int32_t* tp_flag, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_REQUIRE(ap_shape_ok(nd, n_gt, Cls, n_thresholds), PCMI_ERR_INVALID,
               "det_ap: bad shape (nd %lld, n_gt %lld, Cls %d, %d thresholds of at most %d)", (long long)nd, (long long)n_gt, Cls,
               n_thresholds, kApMaxThresholds);
  PCMI_REQUIRE(thresholds && cls_offs && npos && ap && last_rec && (nd == 0 || (best_iou && gt_id)), PCMI_ERR_INVALID,
               "det_ap: null pointer");
  const size_t need = ap_ws(nullptr, nd, n_gt, n_thresholds).bytes;  // 0 with no detection and no box: no workspace at all
  if (need != 0)
    if (int rc = require_ws("det_ap", ws, ws_bytes, need, 1)) return rc;
  hipStream_t st = as_stream(stream);
  ApThresholds thr;
  for (int t = 0; t < kApMaxThresholds; ++t) thr.t[t] = t < n_thresholds ? thresholds[t] : 0.0;
  const ApWs w = ap_ws(ws, nd, n_gt, n_thresholds);
  if (nd > 0 && n_gt > 0) {
    PCMI_HIP_CHECK(hipMemsetAsync(w.claim, 0x7f, (size_t)n_thresholds * (size_t)n_gt * 4, st));
    ap_claim_kernel<<<dim3((unsigned)ceil_div(nd, 256), (unsigned)n_thresholds), 256, 0, st>>>(best_iou, gt_id, nd, n_gt, thr, w.claim);
    PCMI_LAUNCH_CHECK();
  }
  ap_curve_kernel<<<dim3((unsigned)Cls, (unsigned)n_thresholds), kApThreads, 0, st>>>(gt_id, cls_offs, npos, w.claim, nd, n_gt, Cls,
                                                                                      use_07_metric != 0, w.tp_cum, ap, last_rec, rec, prec,
                                                                                      tp_flag);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

}  // extern "C"
