// The detection head of the VoteNet fine-tuning path (downstream/votenet_det_new of the reference): the nearest-neighbour
// matching of its loss (lib/utils/nn_distance.py, called three times by models/loss_helper.py) forward and backward, and
// the decoding of its predictions (models/ap_helper.py:40-177 parse_predictions): box decode, the empty-box test and the
// per-scene greedy NMS.  Written from the semantics in include/pcmi.h; gfx950, wave64, fp32 data, int32 indices.
//
// Arithmetic contract: every operation is rounded on its own in float32 in the order written in include/pcmi.h (contraction
// off for the whole file), so tests/votenet_ref.py reproduces every argmin bit for bit in numpy float32.  No float atomics:
// the backward pass of the matching accumulates every point in gather form, in ascending index of the other cloud.
#include <algorithm>

#include "internal.h"

#pragma clang fp contract(off)

namespace pcmi {
namespace detect {

typedef unsigned long long u64;

// ---- nn_distance ------------------------------------------------------------------------------------------------------------
// MODE 0: squared L2, 1: L1, 2: Huber (smooth L1) per component.
template <int MODE>
__device__ __forceinline__ float comp(float x, float delta) {
  if constexpr (MODE == 0) {
    return x * x;
  } else if constexpr (MODE == 1) {
    return fabsf(x);
  } else {
    const float ax = fabsf(x);
    const float q = fminf(ax, delta);
    return (0.5f * (q * q)) + (delta * (ax - q));
  }
}

template <int MODE>
__device__ __forceinline__ float pair_dist(float ax, float ay, float az, float bx, float by, float bz, float delta) {
  return (comp<MODE>(ax - bx, delta) + comp<MODE>(ay - by, delta)) + comp<MODE>(az - bz, delta);
}

// derivative of comp with respect to x
template <int MODE>
__device__ __forceinline__ float dcomp(float x, float delta) {
  if constexpr (MODE == 0) {
    return 2.f * x;
  } else if constexpr (MODE == 1) {
    return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f);
  } else {
    return fminf(fmaxf(x, -delta), delta);
  }
}

constexpr int kSmallOther = 32;  // the other cloud is read straight from memory up to this size: many tiny batches
constexpr int kTile = 1024;      // points of the other cloud per LDS tile
constexpr int kRowsPerBlock = 256;

// Many tiny batches: one thread per row of the flat [B * N] list, so a wave covers 64 / N batches; the (at most 32) points of
// the row's other cloud come through the L1.  Scanning in ascending index with strict < keeps the lowest index of a tie.
template <int MODE>
__global__ __launch_bounds__(256) void nn_small_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t rows, int N,
                                                       int M, float delta, float* __restrict__ dist, int32_t* __restrict__ idx) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const float ax = a[3 * r], ay = a[3 * r + 1], az = a[3 * r + 2];
  const float* o = b + (r / N) * M * 3;
  float best = INFINITY;
  int bi = 0;
  for (int j = 0; j < M; ++j) {
    const float d = pair_dist<MODE>(ax, ay, az, o[3 * j], o[3 * j + 1], o[3 * j + 2], delta);
    if (d < best) {
      best = d;
      bi = j;
    }
  }
  dist[r] = best;
  idx[r] = bi;
}

// Few medium batches: grid (row tile, batch); the other cloud streams through LDS in tiles of 1024 points (broadcast reads),
// one thread per row.
template <int MODE>
__global__ __launch_bounds__(kRowsPerBlock) void nn_tiled_kernel(const float* __restrict__ a, const float* __restrict__ b, int N, int M,
                                                                 float delta, float* __restrict__ dist, int32_t* __restrict__ idx) {
  __shared__ float sx[kTile], sy[kTile], sz[kTile];
  const int64_t bt = blockIdx.y;
  const int i = blockIdx.x * kRowsPerBlock + threadIdx.x;
  const bool valid = i < N;
  const float* ap = a + (bt * N + (valid ? i : 0)) * 3;
  const float ax = ap[0], ay = ap[1], az = ap[2];
  float best = INFINITY;
  int bi = 0;
  for (int t0 = 0; t0 < M; t0 += kTile) {
    const int tn = min(kTile, M - t0);
    for (int j = threadIdx.x; j < tn; j += kRowsPerBlock) {
      const float* p = b + (bt * M + t0 + j) * 3;
      sx[j] = p[0];
      sy[j] = p[1];
      sz[j] = p[2];
    }
    __syncthreads();
    if (valid) {
      for (int j = 0; j < tn; ++j) {
        const float d = pair_dist<MODE>(ax, ay, az, sx[j], sy[j], sz[j], delta);
        if (d < best) {
          best = d;
          bi = t0 + j;
        }
      }
    }
    __syncthreads();
  }
  if (valid) {
    dist[bt * N + i] = best;
    idx[bt * N + i] = bi;
  }
}

// The gradient of one cloud `a` [B, N, 3] (the same expression for pc1 and pc2, because the derivative is odd):
//   ga[b, i] = g_a[b, i] d'(a_i - o_{idx_a[i]})  +  sum over the j of the other cloud o [B, M, 3] with idx_o[j] == i, in
//   ascending j, of g_o[b, j] d'(a_i - o_j)
// An index outside its cloud is never dereferenced (the term is dropped).
template <int MODE>
__device__ __forceinline__ void add_term(float& gx, float& gy, float& gz, float g, float ax, float ay, float az, const float* __restrict__ o,
                                         float delta) {
  gx = gx + (g * dcomp<MODE>(ax - o[0], delta));
  gy = gy + (g * dcomp<MODE>(ay - o[1], delta));
  gz = gz + (g * dcomp<MODE>(az - o[2], delta));
}

// direct scan, the other cloud's indices read from memory: M <= kSmallOther, flat rows as nn_small_kernel
template <int MODE>
__global__ __launch_bounds__(256) void nn_bwd_small_kernel(const float* __restrict__ a, const float* __restrict__ o,
                                                           const int32_t* __restrict__ idx_a, const int32_t* __restrict__ idx_o,
                                                           const float* __restrict__ g_a, const float* __restrict__ g_o, int64_t rows, int N,
                                                           int M, float delta, float* __restrict__ ga) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const int64_t bt = r / N;
  const int i = (int)(r - bt * N);
  const float ax = a[3 * r], ay = a[3 * r + 1], az = a[3 * r + 2];
  const float* ob = o + bt * M * 3;
  float gx = 0.f, gy = 0.f, gz = 0.f;
  const int32_t t = idx_a[r];
  if (t >= 0 && t < M) add_term<MODE>(gx, gy, gz, g_a[r], ax, ay, az, ob + 3 * t, delta);
  for (int j = 0; j < M; ++j)
    if (idx_o[bt * M + j] == i) add_term<MODE>(gx, gy, gz, g_o[bt * M + j], ax, ay, az, ob + 3 * j, delta);
  ga[3 * r] = gx;
  ga[3 * r + 1] = gy;
  ga[3 * r + 2] = gz;
}

// direct scan, the other cloud's indices in LDS: M <= kTile, grid (row tile, batch)
template <int MODE>
__global__ __launch_bounds__(kRowsPerBlock) void nn_bwd_scan_kernel(const float* __restrict__ a, const float* __restrict__ o,
                                                                    const int32_t* __restrict__ idx_a, const int32_t* __restrict__ idx_o,
                                                                    const float* __restrict__ g_a, const float* __restrict__ g_o, int N,
                                                                    int M, float delta, float* __restrict__ ga) {
  __shared__ int32_t s_idx[kTile];
  const int64_t bt = blockIdx.y;
  for (int j = threadIdx.x; j < M; j += kRowsPerBlock) s_idx[j] = idx_o[bt * M + j];
  __syncthreads();
  const int i = blockIdx.x * kRowsPerBlock + threadIdx.x;
  if (i >= N) return;
  const int64_t r = bt * N + i;
  const float ax = a[3 * r], ay = a[3 * r + 1], az = a[3 * r + 2];
  const float* ob = o + bt * M * 3;
  float gx = 0.f, gy = 0.f, gz = 0.f;
  const int32_t t = idx_a[r];
  if (t >= 0 && t < M) add_term<MODE>(gx, gy, gz, g_a[r], ax, ay, az, ob + 3 * t, delta);
  for (int j = 0; j < M; ++j)
    if (s_idx[j] == i) add_term<MODE>(gx, gy, gz, g_o[bt * M + j], ax, ay, az, ob + 3 * j, delta);
  ga[3 * r] = gx;
  ga[3 * r + 1] = gy;
  ga[3 * r + 2] = gz;
}

// inverse lists (internal.h: inverse_lists) of idx_o: the sources of row (b, i) are pos[start[r] .. start[r + 1]), flat
// positions b M + j in ascending order
template <int MODE>
__global__ __launch_bounds__(256) void nn_bwd_lists_kernel(const float* __restrict__ a, const float* __restrict__ o,
                                                           const int32_t* __restrict__ idx_a, const float* __restrict__ g_a,
                                                           const float* __restrict__ g_o, const int32_t* __restrict__ start,
                                                           const int32_t* __restrict__ pos, int64_t rows, int N, int M, float delta,
                                                           float* __restrict__ ga) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const int64_t bt = r / N;
  const float ax = a[3 * r], ay = a[3 * r + 1], az = a[3 * r + 2];
  float gx = 0.f, gy = 0.f, gz = 0.f;
  const int32_t t = idx_a[r];
  if (t >= 0 && t < M) add_term<MODE>(gx, gy, gz, g_a[r], ax, ay, az, o + (bt * M + t) * 3, delta);
  const int32_t s = start[r], e = start[r + 1];
  for (int32_t k = s; k < e; ++k) {
    const int64_t p = pos[k];
    add_term<MODE>(gx, gy, gz, g_o[p], ax, ay, az, o + p * 3, delta);
  }
  ga[3 * r] = gx;
  ga[3 * r + 1] = gy;
  ga[3 * r + 2] = gz;
}

static bool nn_shape_ok(int64_t B, int64_t N, int64_t M) {
  return B >= 0 && N >= 1 && M >= 1 && N < (1ll << 31) && M < (1ll << 31) && B < (1ll << 31) && B * N < (1ll << 31) / 3 &&
         B * M < (1ll << 31) / 3;
}

// bytes of inverse lists one direction needs: the other cloud (M points) is scanned directly up to kTile points
static size_t nn_bwd_dir_workspace(int64_t B, int64_t N, int64_t M) {
  return (M > kTile || (M > kSmallOther && B > 65535)) ? inverse_lists_workspace(B * M, B * N) : 0;
}

template <int MODE>
static int nn_fwd_mode(const float* a, const float* b, int64_t B, int64_t N, int64_t M, float delta, float* dist, int32_t* idx,
                       hipStream_t st) {
  if (M <= kSmallOther || B > 65535) {
    nn_small_kernel<MODE><<<(unsigned)ceil_div(B * N, 256), 256, 0, st>>>(a, b, B * N, (int)N, (int)M, delta, dist, idx);
  } else {
    nn_tiled_kernel<MODE><<<dim3((unsigned)ceil_div(N, kRowsPerBlock), (unsigned)B), kRowsPerBlock, 0, st>>>(a, b, (int)N, (int)M, delta,
                                                                                                            dist, idx);
  }
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

template <int MODE>
static int nn_bwd_dir(const float* a, const float* o, const int32_t* idx_a, const int32_t* idx_o, const float* g_a, const float* g_o,
                      int64_t B, int64_t N, int64_t M, float delta, float* ga, void* ws, size_t ws_bytes, hipStream_t st) {
  if (M <= kSmallOther) {
    nn_bwd_small_kernel<MODE><<<(unsigned)ceil_div(B * N, 256), 256, 0, st>>>(a, o, idx_a, idx_o, g_a, g_o, B * N, (int)N, (int)M, delta,
                                                                              ga);
  } else if (M <= kTile && B <= 65535) {
    nn_bwd_scan_kernel<MODE><<<dim3((unsigned)ceil_div(N, kRowsPerBlock), (unsigned)B), kRowsPerBlock, 0, st>>>(a, o, idx_a, idx_o, g_a,
                                                                                                               g_o, (int)N, (int)M, delta, ga);
  } else {
    const int32_t *start = nullptr, *pos = nullptr;
    const int rc = inverse_lists("nn_distance_bwd", idx_o, B, M, N, ws, ws_bytes, &start, &pos, st);
    if (rc != PCMI_OK) return rc;
    nn_bwd_lists_kernel<MODE><<<(unsigned)ceil_div(B * N, 256), 256, 0, st>>>(a, o, idx_a, g_a, g_o, start, pos, B * N, (int)N, (int)M,
                                                                              delta, ga);
  }
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

template <int MODE>
static int nn_bwd_mode(const float* pc1, const float* pc2, const int32_t* idx1, const int32_t* idx2, const float* g1, const float* g2,
                       int64_t B, int64_t N, int64_t M, float delta, float* gpc1, float* gpc2, void* ws, size_t ws_bytes, hipStream_t st) {
  int rc = nn_bwd_dir<MODE>(pc1, pc2, idx1, idx2, g1, g2, B, N, M, delta, gpc1, ws, ws_bytes, st);
  if (rc != PCMI_OK) return rc;
  // the second direction reuses the workspace in stream order
  return nn_bwd_dir<MODE>(pc2, pc1, idx2, idx1, g2, g1, B, M, N, delta, gpc2, ws, ws_bytes, st);
}

// ---- box decode -------------------------------------------------------------------------------------------------------------
// One thread per proposal.  argmax with strict > in ascending index: the lowest index of equal scores, as torch.argmax.
__device__ __forceinline__ int argmax_row(const float* __restrict__ v, int n) {
  float best = v[0];
  int bi = 0;
  for (int k = 1; k < n; ++k) {
    const float x = v[k];
    if (x > best) {
      best = x;
      bi = k;
    }
  }
  return bi;
}

constexpr float kPi = 3.14159265358979323846f;

__global__ __launch_bounds__(256) void box_decode_kernel(const float* __restrict__ center, const float* __restrict__ heading_scores,
                                                         const float* __restrict__ heading_residuals, const float* __restrict__ size_scores,
                                                         const float* __restrict__ size_residuals, const float* __restrict__ sem_scores,
                                                         const float* __restrict__ obj_scores, const float* __restrict__ mean_size,
                                                         int64_t n_box, int H, int S, int Cls, int zero_heading,
                                                         int32_t* __restrict__ heading_class, int32_t* __restrict__ size_class,
                                                         int32_t* __restrict__ sem_cls, float* __restrict__ params, float* __restrict__ corners,
                                                         float* __restrict__ minmax, float* __restrict__ obj_prob, float* __restrict__ sem_probs) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_box) return;
  const int hc = argmax_row(heading_scores + t * H, H);
  const int sc = argmax_row(size_scores + t * S, S);
  const float* sv = sem_scores + t * Cls;
  const int cc = argmax_row(sv, Cls);
  heading_class[t] = hc;
  size_class[t] = sc;
  sem_cls[t] = cc;
  float angle = 0.f;
  if (!zero_heading) {
    angle = (float)hc * ((2.f * kPi) / (float)H) + heading_residuals[t * H + hc];
    if (angle > kPi) angle = angle - 2.f * kPi;
  }
  const float* sr = size_residuals + (t * S + sc) * 3;
  const float l = mean_size[3 * sc] + sr[0], w = mean_size[3 * sc + 1] + sr[1], h = mean_size[3 * sc + 2] + sr[2];
  // upright-depth (x, y, z) -> upright-camera (x, -z, y)
  const float cx = center[3 * t], cy = -center[3 * t + 2], cz = center[3 * t + 1];
  float* pp = params + t * 7;
  pp[0] = cx; pp[1] = cy; pp[2] = cz;
  pp[3] = l; pp[4] = w; pp[5] = h;
  pp[6] = angle;
  const float c = cosf(angle), s = sinf(angle);
  const float hl = 0.5f * l, hw = 0.5f * w, hh = 0.5f * h;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  float* cp = corners + t * 24;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    // get_3d_box's order: x (l) + + - - + + - -, y (h) + + + + - - - -, z (w) + - - + + - - +
    const float x = ((k >> 1) & 1) ? -hl : hl;
    const float y = (k >> 2) ? -hh : hh;
    const float z = (((k + 1) >> 1) & 1) ? -hw : hw;
    const float p[3] = {(c * x + s * z) + cx, y + cy, (c * z - s * x) + cz};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      cp[3 * k + d] = p[d];
      lo[d] = fminf(lo[d], p[d]);
      hi[d] = fmaxf(hi[d], p[d]);
    }
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    minmax[t * 6 + d] = lo[d];
    minmax[t * 6 + 3 + d] = hi[d];
  }
  const float o0 = obj_scores[2 * t], o1 = obj_scores[2 * t + 1];
  const float om = fmaxf(o0, o1);
  const float e0 = expf(o0 - om), e1 = expf(o1 - om);
  obj_prob[t] = e1 / (e0 + e1);
  const float sm = sv[cc];
  float sum = 0.f;
  for (int k = 0; k < Cls; ++k) sum += expf(sv[k] - sm);
  for (int k = 0; k < Cls; ++k) sem_probs[t * Cls + k] = expf(sv[k] - sm) / sum;
}

// ---- points inside the boxes --------------------------------------------------------------------------------------------------
// grid (point tile, scene): every lane keeps 4 points of the scene (in upright-camera coordinates) and walks them over the
// scene's boxes, which come through LDS in tiles of 256 as (centre, cos, sin, half sizes).  A point is inside when, rotated
// into the box's frame, every |coordinate| <= the half size (faces included).  Per box: ballot + popcount over the wave, one
// LDS integer add per wave, one global integer add per workgroup.
constexpr int kCntThreads = 256;
constexpr int kCntPointsPerThread = 4;
constexpr int kCntBoxTile = 256;

__global__ __launch_bounds__(kCntThreads) void box_point_counts_kernel(const float* __restrict__ points, int64_t point_ld, int N,
                                                                       const float* __restrict__ params, int K,
                                                                       int32_t* __restrict__ counts) {
  __shared__ float s_box[kCntBoxTile][8];
  __shared__ int s_cnt[kCntBoxTile];
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t b = blockIdx.y;
  float px[kCntPointsPerThread], py[kCntPointsPerThread], pz[kCntPointsPerThread];
  bool ok[kCntPointsPerThread];
#pragma unroll
  for (int q = 0; q < kCntPointsPerThread; ++q) {
    const int64_t p = ((int64_t)blockIdx.x * kCntPointsPerThread + q) * kCntThreads + tid;
    ok[q] = p < N;
    const float* src = points + (b * N + (ok[q] ? p : 0)) * point_ld;
    px[q] = src[0];
    py[q] = -src[2];
    pz[q] = src[1];
  }
  for (int k0 = 0; k0 < K; k0 += kCntBoxTile) {
    const int kn = min(kCntBoxTile, K - k0);
    __syncthreads();  // the previous tile's readers are done
    for (int k = tid; k < kn; k += kCntThreads) {
      const float* pp = params + (b * K + k0 + k) * 7;
      s_box[k][0] = pp[0];
      s_box[k][1] = pp[1];
      s_box[k][2] = pp[2];
      s_box[k][3] = cosf(pp[6]);
      s_box[k][4] = sinf(pp[6]);
      s_box[k][5] = 0.5f * fabsf(pp[3]);  // l: box x
      s_box[k][6] = 0.5f * fabsf(pp[5]);  // h: box y
      s_box[k][7] = 0.5f * fabsf(pp[4]);  // w: box z
      s_cnt[k] = 0;
    }
    __syncthreads();
    for (int k = 0; k < kn; ++k) {
      const float cx = s_box[k][0], cy = s_box[k][1], cz = s_box[k][2], c = s_box[k][3], s = s_box[k][4];
      const float hx = s_box[k][5], hy = s_box[k][6], hz = s_box[k][7];
      int n_in = 0;
#pragma unroll
      for (int q = 0; q < kCntPointsPerThread; ++q) {
        const float dx = px[q] - cx, dy = py[q] - cy, dz = pz[q] - cz;
        const float lx = (c * dx) - (s * dz), lz = (s * dx) + (c * dz);
        const bool in = ok[q] && fabsf(lx) <= hx && fabsf(dy) <= hy && fabsf(lz) <= hz;
        n_in += (int)__popcll(__ballot(in));
      }
      if (lane == 0 && n_in) atomicAdd(&s_cnt[k], n_in);
    }
    __syncthreads();
    for (int k = tid; k < kn; k += kCntThreads)
      if (s_cnt[k]) atomicAdd(&counts[b * K + k0 + k], s_cnt[k]);
  }
}

// ---- greedy NMS ---------------------------------------------------------------------------------------------------------------
// One workgroup per scene.  (1) every non-empty box takes its rank: the number of non-empty boxes with a larger score, or an
// equal score and a lower index.  (2) the boxes move to LDS in rank order.  (3) bit c of row r of the suppression matrix
// (KMAX x KMAX bits in LDS) says that the box of rank r suppresses the box of rank c > r: the lanes of a wave take consecutive
// rows and the same 64 columns, so the column boxes are broadcast reads.  (4) wave 0 sweeps the ranks in order with one word
// of the alive set per lane: the first alive rank is kept and its row cleared from the set.
constexpr int kNmsMaxK = 1024;
constexpr uint16_t kNoBox = 0xffff;

template <int KMAX>
struct NmsShared {
  u64 bits[KMAX * (KMAX / 64)];
  float box[6][KMAX];
  int32_t cls[KMAX];
  uint16_t order[KMAX];  // box of every rank; kNoBox: none
  int n_valid;
};

// mode 0: 2D on camera x / z, 1: 3D, 2: 3D and the same class
__device__ __forceinline__ bool nms_suppresses(int mode, int old_type, float thr, const float* bi, int ci, const float* bj, int cj) {
  float inter, ai, aj;
  const float lx = fmaxf(0.f, fminf(bi[3], bj[3]) - fmaxf(bi[0], bj[0]));
  const float lz = fmaxf(0.f, fminf(bi[5], bj[5]) - fmaxf(bi[2], bj[2]));
  if (mode == 0) {
    inter = lx * lz;
    ai = (bi[3] - bi[0]) * (bi[5] - bi[2]);
    aj = (bj[3] - bj[0]) * (bj[5] - bj[2]);
  } else {
    const float ly = fmaxf(0.f, fminf(bi[4], bj[4]) - fmaxf(bi[1], bj[1]));
    inter = (lx * ly) * lz;
    ai = ((bi[3] - bi[0]) * (bi[4] - bi[1])) * (bi[5] - bi[2]);
    aj = ((bj[3] - bj[0]) * (bj[4] - bj[1])) * (bj[5] - bj[2]);
  }
  const float o = old_type ? inter / aj : inter / ((ai + aj) - inter);
  return (mode != 2 || ci == cj) && o > thr;  // a NaN overlap (0 / 0 of a zero-volume box) suppresses nothing
}

template <int KMAX>
__global__ __launch_bounds__(KMAX) void box_nms_kernel(const float* __restrict__ minmax, const float* __restrict__ score,
                                                       const int32_t* __restrict__ sem_cls, const int32_t* __restrict__ counts,
                                                       int min_points, int K, int mode, int old_type, float thr,
                                                       int32_t* __restrict__ pred_mask) {
  __shared__ NmsShared<KMAX> sh;
  constexpr int W = KMAX / 64;
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t base = (int64_t)blockIdx.x * K;
  // the scores (and the non-empty flags) sit in the matrix's memory while the ranks are taken
  float* s_score = reinterpret_cast<float*>(sh.bits);
  int* s_flag = reinterpret_cast<int*>(sh.bits) + KMAX;
  if (tid == 0) sh.n_valid = 0;
  for (int i = tid; i < K; i += KMAX) {
    s_score[i] = score[base + i];
    s_flag[i] = counts ? (counts[base + i] >= min_points) : 1;
    pred_mask[base + i] = 0;
  }
  __syncthreads();
  int my_rank = -1;  // KMAX threads: at most one box per thread
  if (tid < K && s_flag[tid]) {
    const float s = s_score[tid];
    int r = 0;
    for (int j = 0; j < K; ++j) {
      const float o = s_score[j];
      r += (s_flag[j] && (o > s || (o == s && j < tid))) ? 1 : 0;
    }
    my_rank = r;
    atomicAdd(&sh.n_valid, 1);
  }
  __syncthreads();  // every reader of the scores is done: the matrix may be written
  const int nv = sh.n_valid;
  // a NaN score compares false with everything and could share a rank: slots nobody takes hold a zero-volume box
  for (int i = tid; i < K; i += KMAX) {
#pragma unroll
    for (int d = 0; d < 6; ++d) sh.box[d][i] = 0.f;
    sh.cls[i] = -1;
    sh.order[i] = kNoBox;
  }
  __syncthreads();
  if (my_rank >= 0 && my_rank < K) {
    const int r = my_rank;
#pragma unroll
    for (int d = 0; d < 6; ++d) sh.box[d][r] = minmax[(base + tid) * 6 + d];
    sh.cls[r] = (mode == 2 && sem_cls) ? sem_cls[base + tid] : 0;
    sh.order[r] = (uint16_t)tid;
  }
  __syncthreads();
  const int nw = (nv + 63) >> 6;  // words of a row that hold ranks
  for (int p = tid; p < nw * nv; p += KMAX) {
    const int w = p / nv, r = p - w * nv;
    float bi[6];
#pragma unroll
    for (int d = 0; d < 6; ++d) bi[d] = sh.box[d][r];
    const int ci = sh.cls[r];
    u64 word = 0;
    const int c0 = w * 64;
    const int c1 = min(nv, c0 + 64);
    for (int c = max(c0, r + 1); c < c1; ++c) {
      float bj[6];
#pragma unroll
      for (int d = 0; d < 6; ++d) bj[d] = sh.box[d][c];
      if (nms_suppresses(mode, old_type, thr, bi, ci, bj, sh.cls[c])) word |= 1ull << (c - c0);
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
      const uint16_t who = sh.order[r];
      if (lane == 0 && who != kNoBox) pred_mask[base + who] = 1;
      if (lane < nw) alive &= ~sh.bits[r * W + lane];
      a = __shfl(alive, w, 64);
      a &= bit == 63 ? 0ull : ~((2ull << bit) - 1ull);  // ranks above r only
    }
  }
}

}  // namespace detect
}  // namespace pcmi

using namespace pcmi;
using namespace pcmi::detect;

extern "C" {

int pcmi_nn_distance_fwd(const float* a, const float* b, int64_t B, int64_t N, int64_t M, int mode, float delta, float* dist,
                         int32_t* idx, pcmi_stream_t stream) {
  PCMI_REQUIRE(nn_shape_ok(B, N, M), PCMI_ERR_INVALID, "nn_distance_fwd: bad size (B %lld, N %lld, M %lld)", (long long)B, (long long)N,
               (long long)M);
  PCMI_REQUIRE(mode >= 0 && mode <= 2, PCMI_ERR_INVALID, "nn_distance_fwd: mode %d is none of 0 (L2), 1 (L1), 2 (Huber)", mode);
  if (B == 0) return PCMI_OK;
  PCMI_REQUIRE(a && b && dist && idx, PCMI_ERR_INVALID, "nn_distance_fwd: null pointer");
  hipStream_t st = as_stream(stream);
  if (mode == 0) return nn_fwd_mode<0>(a, b, B, N, M, delta, dist, idx, st);
  if (mode == 1) return nn_fwd_mode<1>(a, b, B, N, M, delta, dist, idx, st);
  return nn_fwd_mode<2>(a, b, B, N, M, delta, dist, idx, st);
}

size_t pcmi_nn_distance_bwd_workspace_bytes(int64_t B, int64_t N, int64_t M) {
  if (!nn_shape_ok(B, N, M) || B == 0) return 0;
  return std::max(nn_bwd_dir_workspace(B, N, M), nn_bwd_dir_workspace(B, M, N));
}

int pcmi_nn_distance_bwd(const float* pc1, const float* pc2, const int32_t* idx1, const int32_t* idx2, const float* gdist1,
                         const float* gdist2, int64_t B, int64_t N, int64_t M, int mode, float delta, float* gpc1, float* gpc2, void* ws,
                         size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_REQUIRE(nn_shape_ok(B, N, M), PCMI_ERR_INVALID, "nn_distance_bwd: bad size (B %lld, N %lld, M %lld)", (long long)B, (long long)N,
               (long long)M);
  PCMI_REQUIRE(mode >= 0 && mode <= 2, PCMI_ERR_INVALID, "nn_distance_bwd: mode %d is none of 0 (L2), 1 (L1), 2 (Huber)", mode);
  if (B == 0) return PCMI_OK;
  PCMI_REQUIRE(pc1 && pc2 && idx1 && idx2 && gdist1 && gdist2 && gpc1 && gpc2, PCMI_ERR_INVALID, "nn_distance_bwd: null pointer");
  const size_t need = pcmi_nn_distance_bwd_workspace_bytes(B, N, M);  // 0: neither direction builds inverse lists
  if (need != 0)
    if (int rc = require_ws("nn_distance_bwd", ws, ws_bytes, need, 1)) return rc;
  hipStream_t st = as_stream(stream);
  if (mode == 0) return nn_bwd_mode<0>(pc1, pc2, idx1, idx2, gdist1, gdist2, B, N, M, delta, gpc1, gpc2, ws, ws_bytes, st);
  if (mode == 1) return nn_bwd_mode<1>(pc1, pc2, idx1, idx2, gdist1, gdist2, B, N, M, delta, gpc1, gpc2, ws, ws_bytes, st);
  return nn_bwd_mode<2>(pc1, pc2, idx1, idx2, gdist1, gdist2, B, N, M, delta, gpc1, gpc2, ws, ws_bytes, st);
}

int pcmi_box_decode(const float* center, const float* heading_scores, const float* heading_residuals, const float* size_scores,
                    const float* size_residuals, const float* sem_cls_scores, const float* objectness_scores, const float* mean_size_arr,
                    int64_t B, int64_t K, int H, int S, int Cls, int zero_heading, int32_t* heading_class, int32_t* size_class,
                    int32_t* sem_cls, float* box_params, float* corners, float* minmax, float* obj_prob, float* sem_cls_probs,
                    pcmi_stream_t stream) {
  PCMI_REQUIRE(B >= 0 && K >= 0 && H >= 1 && S >= 1 && Cls >= 1 && B * K < (1ll << 31) / 24 &&
                   B * K * std::max(std::max(H, 3 * S), Cls) < (1ll << 40),
               PCMI_ERR_INVALID, "box_decode: bad shape (B %lld, K %lld, H %d, S %d, Cls %d)", (long long)B, (long long)K, H, S, Cls);
  if (B * K == 0) return PCMI_OK;
  PCMI_REQUIRE(center && heading_scores && heading_residuals && size_scores && size_residuals && sem_cls_scores && objectness_scores &&
                   mean_size_arr && heading_class && size_class && sem_cls && box_params && corners && minmax && obj_prob && sem_cls_probs,
               PCMI_ERR_INVALID, "box_decode: null pointer");
  box_decode_kernel<<<(unsigned)ceil_div(B * K, 256), 256, 0, as_stream(stream)>>>(
      center, heading_scores, heading_residuals, size_scores, size_residuals, sem_cls_scores, objectness_scores, mean_size_arr, B * K, H, S,
      Cls, zero_heading, heading_class, size_class, sem_cls, box_params, corners, minmax, obj_prob, sem_cls_probs);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

int pcmi_box_point_counts(const float* points, int64_t point_ld, const float* box_params, int64_t B, int64_t N, int64_t K,
                          int32_t* counts, pcmi_stream_t stream) {
  PCMI_REQUIRE(B >= 0 && N >= 0 && K >= 0 && point_ld >= 3 && B <= 65535 && N < (1ll << 31) - 4096 && B * K < (1ll << 31) / 7 &&
                   B * N < (1ll << 40) / point_ld,
               PCMI_ERR_INVALID, "box_point_counts: bad shape (B %lld, N %lld, K %lld, %lld floats per point)", (long long)B, (long long)N,
               (long long)K, (long long)point_ld);
  if (B * K == 0) return PCMI_OK;
  PCMI_REQUIRE(counts && box_params && (points || N == 0), PCMI_ERR_INVALID, "box_point_counts: null pointer");
  hipStream_t st = as_stream(stream);
  PCMI_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)B * K * 4, st));
  if (N == 0) return PCMI_OK;
  box_point_counts_kernel<<<dim3((unsigned)ceil_div(N, kCntThreads * kCntPointsPerThread), (unsigned)B), kCntThreads, 0, st>>>(
      points, point_ld, (int)N, box_params, (int)K, counts);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

int pcmi_box_nms(const float* minmax, const float* obj_prob, const int32_t* sem_cls, const int32_t* counts, int min_points, int64_t B,
                 int64_t K, int mode, int old_type, float nms_iou, int32_t* pred_mask, pcmi_stream_t stream) {
  PCMI_REQUIRE(B >= 0 && K >= 0 && B < (1ll << 31) / (kNmsMaxK * 6), PCMI_ERR_INVALID, "box_nms: bad shape (B %lld, K %lld)", (long long)B,
               (long long)K);
  PCMI_REQUIRE(K <= kNmsMaxK, PCMI_ERR_UNSUPPORTED, "box_nms: %lld proposals per scene, at most %d are supported", (long long)K, kNmsMaxK);
  PCMI_REQUIRE(mode >= 0 && mode <= 2, PCMI_ERR_INVALID, "box_nms: mode %d is none of 0 (2D), 1 (3D), 2 (3D, same class)", mode);
  if (B * K == 0) return PCMI_OK;
  PCMI_REQUIRE(minmax && obj_prob && pred_mask && (mode != 2 || sem_cls), PCMI_ERR_INVALID, "box_nms: null pointer");
  hipStream_t st = as_stream(stream);
  if (K <= 256) {
    box_nms_kernel<256><<<(unsigned)B, 256, 0, st>>>(minmax, obj_prob, sem_cls, counts, min_points, (int)K, mode, old_type != 0, nms_iou,
                                                     pred_mask);
  } else {
    box_nms_kernel<1024><<<(unsigned)B, 1024, 0, st>>>(minmax, obj_prob, sem_cls, counts, min_points, (int)K, mode, old_type != 0, nms_iou,
                                                       pred_mask);
  }
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

}  // extern "C"
