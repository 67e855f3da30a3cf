// The input side of VoteNet detection fine-tuning for a BATCH of scans, on the device: what the reference does per scan on the
// host in downstream/votenet_det_new --
//   * ScannetDetectionDataset.__getitem__: random_sampling, two flips, rotation, rotate_aligned_boxes, the per-instance vote
//     loop and the box labels                                              (lib/datasets/scannet/scannet_detection_dataset.py:60-172)
//   * SunrgbdDetectionVotesDataset.__getitem__: flip, rotation carried through three stored votes, scale, angle2class,
//     size2class and the hull of my_compute_box_3d                        (lib/datasets/sunrgbd/sunrgbd_detection_dataset.py:68-212)
//   * VoxelizationDataset.__getitem__ and collate_fn                      (models/backbone/sparseconv/voxelized_dataset.py:33-65)
// Written from the semantics in include/pcmi.h; gfx950, wave64.  Every random quantity is an input.
//
// Arithmetic, as semseg_input.hip: every fp64 (and fp32) product and sum is an explicit round-to-nearest operation in the
// order pcmi.h states (no FMA contraction).  The only atomics are integer minima, maxima and ors -- a float is reduced through
// its order-preserving integer image -- whose result does not depend on the order of arrival.  Every output is the same bits
// from run to run.
#include <algorithm>
#include <climits>

#include "exact.h"
#include "internal.h"

#pragma clang fp contract(off)

namespace pcmi {
namespace detinput {

constexpr int kThreads = 256;
constexpr int kMaxScenes = 1023;         // pcmi_seg_quantize's limit: the voxels of a batch go through it
constexpr int kMaxObj = PCMI_DET_MAX_NUM_OBJ;
constexpr int kMaxInst = PCMI_DET_MAX_INSTANCES;
constexpr int kInstRows = 2048;          // rows of one scene that a workgroup of vi_reduce_kernel folds into its LDS table
constexpr int kMaxValid = 1024;
constexpr int kVoxelLimit = 1 << 20;
constexpr int64_t kMaxRows = 1ll << 29;  // pcmi_seg_quantize's limit
constexpr double kPi = 3.141592653589793;  // numpy's np.pi

// ---- sample, flip, rotate, scale (and the stored votes of SUN RGB-D) -----------------------------------------------------------
struct SampleArgs {
  const float* xyz;
  const int64_t* offs;
  int64_t n;
  int B;
  int64_t P;
  const int32_t* choices;
  int augment;
  const int32_t* flip;   // [B, 2]
  const double* rot;     // [B, 9]
  const double* scale;   // [B]
  const int32_t* instance;
  const int32_t* semantic;
  const double* votes;   // [n, 10]
  float* pc;             // [B, P, 3]
  int32_t* out_instance;
  int32_t* out_semantic;
  float* vote_label;     // [B, P, 9]
  int64_t* vote_mask;    // [B, P]
  int32_t* flags;
};

__global__ __launch_bounds__(kThreads) void sample_kernel(SampleArgs a) {
  const int64_t row = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (row >= (int64_t)a.B * a.P) return;
  const int b = (int)(row / a.P);
  const int64_t lo = a.offs[b], hi = a.offs[b + 1];
  const int64_t c = a.choices[row];
  int flag = 0;
  int64_t g = -1;
  if (lo >= 0 && hi >= lo && hi <= a.n && c >= 0 && c < hi - lo) g = lo + c; else flag = PCMI_DET_FLAG_CHOICE;
  float p[3] = {0.f, 0.f, 0.f};
  if (g >= 0) {
    p[0] = a.xyz[3 * g], p[1] = a.xyz[3 * g + 1], p[2] = a.xyz[3 * g + 2];
    if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))) {
      flag = PCMI_DET_FLAG_RANGE;
      g = -1;
    }
  }
  float o[3] = {0.f, 0.f, 0.f};
  double v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  int64_t mask = 0;
  if (g >= 0) {
    if (a.votes) {
      const double* s = a.votes + 10 * g;
      const double m0 = s[0];
      mask = fabs(m0) < 9.0e18 ? (int64_t)m0 : 0;  // astype(np.int64) truncates; a value that does not fit, or NaN, gives 0
#pragma unroll
      for (int q = 0; q < 9; ++q) v[q] = s[1 + q];
    }
    if (a.augment) {
      const bool fx = a.flip[2 * b] != 0, fy = a.flip[2 * b + 1] != 0;
      const double* R = a.rot + 9 * b;
      const double sc = a.scale[b];
      if (fx) p[0] = -p[0];
      if (fy) p[1] = -p[1];
      const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
      float r32[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) r32[r] = (float)((x * R[3 * r] + y * R[3 * r + 1]) + z * R[3 * r + 2]);
      if (a.votes) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          if (fx) v[3 * k] = -v[3 * k];
          if (fy) v[3 * k + 1] = -v[3 * k + 1];
          const double ex = x + v[3 * k], ey = y + v[3 * k + 1], ez = z + v[3 * k + 2];
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            const double end = (ex * R[3 * r] + ey * R[3 * r + 1]) + ez * R[3 * r + 2];
            v[3 * k + r] = (end - (double)r32[r]) * sc;
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 3; ++r) o[r] = (float)((double)r32[r] * sc);
    } else {
#pragma unroll
      for (int r = 0; r < 3; ++r) o[r] = p[r];
    }
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) a.pc[3 * row + r] = o[r];
  if (a.out_instance) a.out_instance[row] = g >= 0 ? a.instance[g] : -1;
  if (a.out_semantic) a.out_semantic[row] = g >= 0 ? a.semantic[g] : -1;
  if (a.vote_label) {
#pragma unroll
    for (int q = 0; q < 9; ++q) a.vote_label[9 * row + q] = (float)v[q];
    a.vote_mask[row] = mask;
  }
  if (flag) atomicOr(&a.flags[b], flag);
}

// ---- votes from instances ----------------------------------------------------------------------------------------------------
// global table, per scene and instance 7 words: the order images of min x, y, z and max x, y, z, and the first row
__global__ __launch_bounds__(kThreads) void vi_init_kernel(uint32_t* __restrict__ tab, int64_t total) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= total) return;
  const int w = (int)(t % 7);
  tab[t] = (w >= 3 && w < 6) ? 0u : 0xffffffffu;
}

// true when the row takes part: a finite point with an instance id in range; the dropped rows of pcmi_det_sample_transform
// (id -1) stay silent, every other id outside the range and every non-finite point is flagged
__device__ inline bool vi_row(const float* __restrict__ pc, const int32_t* __restrict__ inst, int64_t row, float* p, int* id, int* flag) {
  const int i = inst[row];
  p[0] = pc[3 * row], p[1] = pc[3 * row + 1], p[2] = pc[3 * row + 2];
  if (i == -1) return false;
  if (i < 0 || i >= kMaxInst) {
    *flag |= PCMI_DET_FLAG_INSTANCE;
    return false;
  }
  if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))) {
    *flag |= PCMI_DET_FLAG_RANGE;
    return false;
  }
  *id = i;
  return true;
}

__global__ __launch_bounds__(kThreads) void vi_reduce_kernel(const float* __restrict__ pc, const int32_t* __restrict__ inst, int64_t P,
                                                             uint32_t* tab, int32_t* flags) {
  __shared__ uint32_t s_tab[7 * kMaxInst];  // 28 KiB: [word][instance]
  const int b = blockIdx.y;
  for (int t = threadIdx.x; t < 7 * kMaxInst; t += kThreads) {
    const int w = t / kMaxInst;
    s_tab[t] = (w >= 3 && w < 6) ? 0u : 0xffffffffu;
  }
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * kInstRows, r1 = std::min<int64_t>(r0 + kInstRows, P);
  int flag = 0;
  for (int64_t r = r0 + threadIdx.x; r < r1; r += kThreads) {
    float p[3];
    int id = 0;
    if (!vi_row(pc, inst, (int64_t)b * P + r, p, &id, &flag)) continue;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const uint32_t u = ord32(p[a]);
      atomicMin(&s_tab[a * kMaxInst + id], u);
      atomicMax(&s_tab[(3 + a) * kMaxInst + id], u);
    }
    atomicMin(&s_tab[6 * kMaxInst + id], (uint32_t)r);
  }
  if (flag) atomicOr(&flags[b], flag);
  __syncthreads();
  uint32_t* g = tab + (int64_t)b * kMaxInst * 7;
  for (int id = threadIdx.x; id < kMaxInst; id += kThreads) {
    if (s_tab[6 * kMaxInst + id] == 0xffffffffu) continue;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      atomicMin(&g[7 * id + a], s_tab[a * kMaxInst + id]);
      atomicMax(&g[7 * id + 3 + a], s_tab[(3 + a) * kMaxInst + id]);
    }
    atomicMin(&g[7 * id + 6], s_tab[6 * kMaxInst + id]);
  }
}

__global__ __launch_bounds__(kThreads) void vi_apply_kernel(const float* __restrict__ pc, const int32_t* __restrict__ inst,
                                                            const int32_t* __restrict__ sem, int64_t P, int B,
                                                            const int32_t* __restrict__ valid, int n_valid,
                                                            const uint32_t* __restrict__ tab, float* __restrict__ vote_label,
                                                            int64_t* __restrict__ vote_mask) {
  const int64_t row = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (row >= (int64_t)B * P) return;
  const int b = (int)(row / P);
  float p[3], v[3] = {0.f, 0.f, 0.f};
  int id = 0, flag = 0;
  int64_t mask = 0;
  if (vi_row(pc, inst, row, p, &id, &flag)) {
    const uint32_t* g = tab + ((int64_t)b * kMaxInst + id) * 7;
    const int32_t s = sem[(int64_t)b * P + g[6]];
    bool ok = false;
    for (int q = 0; q < n_valid; ++q) ok = ok || valid[q] == s;
    if (ok) {
      mask = 1;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float sum = unord32(g[a]) + unord32(g[3 + a]);
        const float center = 0.5f * sum;
        v[a] = center - p[a];
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 9; ++q) vote_label[9 * row + q] = v[q % 3];
  vote_mask[row] = mask;
}

// ---- box labels -----------------------------------------------------------------------------------------------------------------
// Python's float a % m for m > 0: fmod, moved into [0, m) -- the result takes the divisor's sign, a zero result is +0
__device__ inline double py_mod(double a, double m) {
  double r = fmod(a, m);
  if (r != 0.0) {
    if (r < 0.0) r = r + m;
  } else {
    r = 0.0;
  }
  return r;
}

struct BoxArgs {
  const double* boxes;      // [B, 64, 8]
  const int32_t* n_boxes;   // [B]
  int B;
  int mode;                 // PCMI_DET_SCANNET / PCMI_DET_SUNRGBD
  int augment;
  const int32_t* flip;
  const double* rot;
  const double* rot_angle;
  const double* scale;
  const double* heading_cs; // [B, 64, 2]
  const int32_t* label_to_class;
  int n_lut;
  const double* mean_size;  // [n_class, 3]
  int n_class;
  int num_heading_bin;
  float* center_label;
  int64_t* heading_class;
  float* heading_residual;
  int64_t* size_class;
  float* size_residual;
  int64_t* sem_cls;
  float* box_mask;
  int32_t* flags;
};

__global__ __launch_bounds__(kThreads) void box_kernel(BoxArgs a) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= a.B * kMaxObj) return;
  const int b = t / kMaxObj, i = t % kMaxObj;
  int k = a.n_boxes[b], flag = 0;
  if (k < 0 || k > kMaxObj) {
    k = 0;
    flag = PCMI_DET_FLAG_BOXES;
  }
  const bool live = i < k;
  double c[3] = {0, 0, 0}, l[3] = {0, 0, 0}, h = 0.0, lab = 0.0;
  bool fin = true;  // a live box that is not finite counts as a slot of zeros: class 0, no residual
  if (live) {
    const double* s = a.boxes + 8 * (int64_t)t;
    bool ok = true;
#pragma unroll
    for (int q = 0; q < 8; ++q) ok = ok && isfinite(s[q]);
    if (!ok) flag |= PCMI_DET_FLAG_RANGE;
    fin = ok;
    if (ok) {
#pragma unroll
      for (int q = 0; q < 3; ++q) c[q] = s[q], l[q] = s[3 + q];
      h = s[6], lab = s[7];
    }
  }
  const bool fx = a.augment && a.flip[2 * b] != 0, fy = a.augment && a.flip[2 * b + 1] != 0;
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  if (a.augment)
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] = a.rot[9 * b + q];
  int cls = 0;
  double center[3] = {0, 0, 0}, res[3] = {0, 0, 0}, hres = 0.0;
  int64_t hcls = 0;
  if (a.mode == PCMI_DET_SCANNET) {
    // every slot, the padded ones too, goes through the flips and rotate_aligned_boxes, as in the reference
    if (fx) c[0] = -1.0 * c[0];
    if (fy) c[1] = -1.0 * c[1];
    if (a.augment) {
      double nc[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) nc[r] = (c[0] * R[3 * r] + c[1] * R[3 * r + 1]) + c[2] * R[3 * r + 2];
      const double dx = l[0] / 2.0, dy = l[1] / 2.0;
      const double sx[4] = {-1.0, 1.0, 1.0, -1.0}, sy[4] = {-1.0, -1.0, 1.0, 1.0};
      double mx = 0.0, my = 0.0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double cx = sx[q] * dx, cy = sy[q] * dy;
        const double x = (cx * R[0] + cy * R[1]) + 0.0 * R[2], y = (cx * R[3] + cy * R[4]) + 0.0 * R[5];
        mx = q == 0 ? x : fmax(mx, x);
        my = q == 0 ? y : fmax(my, y);
      }
      c[0] = nc[0], c[1] = nc[1], c[2] = nc[2];
      l[0] = 2.0 * mx, l[1] = 2.0 * my;
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) center[q] = c[q];
    if (live && fin) {
      const int64_t id = fabs(lab) < 2.0e9 ? (int64_t)lab : -1;
      cls = (id >= 0 && id < a.n_lut && (double)id == lab) ? a.label_to_class[id] : -1;
      if (cls < 0 || cls >= a.n_class) {
        flag |= PCMI_DET_FLAG_LABEL;
        cls = 0;
      } else {
#pragma unroll
        for (int q = 0; q < 3; ++q) res[q] = l[q] - a.mean_size[3 * cls + q];
      }
    }
  } else if (live && fin) {
    if (a.augment) {
      const double sc = a.scale[b];
      if (fx) {
        c[0] = -1.0 * c[0];
        h = kPi - h;
      }
      double nc[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) nc[r] = (c[0] * R[3 * r] + c[1] * R[3 * r + 1]) + c[2] * R[3 * r + 2];
      h = h - a.rot_angle[b];
#pragma unroll
      for (int q = 0; q < 3; ++q) c[q] = nc[q] * sc, l[q] = l[q] * sc;
    }
    // angle2class (model_util_sunrgbd.py:49-65)
    const double two_pi = 2.0 * kPi;
    const double ang = py_mod(h, two_pi);
    const double per = two_pi / (double)a.num_heading_bin;
    const double shifted = py_mod(ang + per / 2.0, two_pi);
    hcls = (int64_t)(shifted / per);
    hres = shifted - ((double)hcls * per + per / 2.0);
    // size2class against the caller's mean sizes
    const int64_t id = fabs(lab) < 2.0e9 ? (int64_t)lab : -1;
    cls = (int)id;
    if (id < 0 || id >= a.n_class) {
      flag |= PCMI_DET_FLAG_LABEL;
      cls = 0;
      hcls = 0, hres = 0.0;
    } else {
#pragma unroll
      for (int q = 0; q < 3; ++q) res[q] = l[q] * 2.0 - a.mean_size[3 * cls + q];
      // the axis-aligned hull of my_compute_box_3d's corners (sunrgbd_utils.py:226-236): R' = rotz(-heading), its cosine and
      // sine from the caller
      const double co = a.heading_cs[2 * (int64_t)t], si = a.heading_cs[2 * (int64_t)t + 1];
      const double xs[8] = {-l[0], l[0], l[0], -l[0], -l[0], l[0], l[0], -l[0]};
      const double ys[8] = {l[1], l[1], -l[1], -l[1], l[1], l[1], -l[1], -l[1]};
      const double zs[8] = {l[2], l[2], l[2], l[2], -l[2], -l[2], -l[2], -l[2]};
      double mn[3], mx[3];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        double p[3];
        p[0] = ((co * xs[q] + (-si) * ys[q]) + 0.0 * zs[q]) + c[0];
        p[1] = ((si * xs[q] + co * ys[q]) + 0.0 * zs[q]) + c[1];
        p[2] = ((0.0 * xs[q] + 0.0 * ys[q]) + 1.0 * zs[q]) + c[2];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          mn[r] = q == 0 ? p[r] : fmin(mn[r], p[r]);
          mx[r] = q == 0 ? p[r] : fmax(mx[r], p[r]);
        }
      }
#pragma unroll
      for (int r = 0; r < 3; ++r) center[r] = (mn[r] + mx[r]) / 2.0;
    }
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    a.center_label[3 * (int64_t)t + q] = (float)center[q];
    a.size_residual[3 * (int64_t)t + q] = (float)res[q];
  }
  a.heading_class[t] = hcls;
  a.heading_residual[t] = (float)hres;
  a.size_class[t] = live ? cls : 0;
  a.sem_cls[t] = live ? cls : 0;
  a.box_mask[t] = live ? 1.f : 0.f;
  if (flag) atomicOr(&a.flags[b], flag);
}

// ---- voxelize -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void vx_init_kernel(int32_t* __restrict__ scene_min, int64_t* __restrict__ offs, int B, int64_t P) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t < 3 * B) scene_min[t] = INT_MAX;
  if (t <= B) offs[t] = (int64_t)t * P;
}

__global__ __launch_bounds__(kThreads) void vx_point_kernel(const float* __restrict__ pc, int64_t P, int B, float voxel_size,
                                                            int32_t* __restrict__ vox, uint8_t* __restrict__ keep, int32_t* scene_min,
                                                            int32_t* flags) {
  const int64_t row = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool in = row < (int64_t)B * P;
  const int b = in ? (int)(row / P) : -1;
  int v[3] = {INT_MAX, INT_MAX, INT_MAX};
  bool ok = in;
  if (in) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float f = floorf(__fdiv_rn(pc[3 * row + a], voxel_size));
      if (!(fabsf(f) < (float)kVoxelLimit)) ok = false;  // NaN included
      v[a] = ok ? (int)f : 0;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) vox[3 * row + a] = ok ? v[a] : 0;
    keep[row] = ok ? 1 : 0;
    if (!ok) atomicOr(&flags[b], PCMI_DET_FLAG_RANGE);
  }
  if (!ok) v[0] = v[1] = v[2] = INT_MAX;
  // a wave that lies inside one scene sends one minimum per axis
  if (__all(in && b == __shfl(b, 0, 64)) != 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) v[a] = std::min(v[a], __shfl_xor(v[a], d, 64));
    if ((threadIdx.x & 63) != 0) return;
  } else if (!ok) {
    return;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
    if (v[a] != INT_MAX) atomicMin(&scene_min[3 * b + a], v[a]);
}

__global__ __launch_bounds__(kThreads) void vx_min_kernel(int32_t* __restrict__ scene_min, int B) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t < 3 * B && scene_min[t] == INT_MAX) scene_min[t] = 0;
}

// the rows that pcmi_seg_quantize left: the minimum goes back on, the row index becomes the scene's own
__global__ __launch_bounds__(kThreads) void vx_close_kernel(int32_t* __restrict__ coords, const int64_t* __restrict__ index,
                                                            const int64_t* __restrict__ counts, const int32_t* __restrict__ scene_min, int B,
                                                            int64_t P, int32_t* __restrict__ inds, float* __restrict__ feats) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= counts[B]) return;
  const int b = coords[4 * p];
  if (b < 0 || b >= B) return;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    coords[4 * p + 1 + a] += scene_min[3 * b + a];
    feats[3 * p + a] = 1.f;
  }
  inds[p] = (int32_t)(index[p] - (int64_t)b * P);
}

static bool shape_ok(int64_t B, int64_t P) { return B >= 1 && B <= kMaxScenes && P >= 1 && P <= kMaxRows && B * P <= kMaxRows; }

static int sample_common(const char* who, SampleArgs& a, pcmi_stream_t stream) {
  PCMI_REQUIRE(shape_ok(a.B, a.P) && a.n >= 0 && a.n < (1ll << 31) - kThreads, PCMI_ERR_INVALID,
               "%s: bad shape (1 <= B %d <= %d; 1 <= num_points %lld, B num_points <= 2^29; 0 <= n %lld < 2^31 - 256)", who, a.B,
               kMaxScenes, (long long)a.P, (long long)a.n);
  PCMI_REQUIRE(a.offs && a.choices && a.pc && a.flags && (a.n == 0 || a.xyz), PCMI_ERR_INVALID, "%s: null pointer", who);
  PCMI_REQUIRE(!a.augment || (a.flip && a.rot && a.scale), PCMI_ERR_INVALID, "%s: augment needs flip, rot and scale", who);
  PCMI_REQUIRE((uintptr_t)a.rot % 8 == 0 && (uintptr_t)a.scale % 8 == 0 && (uintptr_t)a.offs % 8 == 0 && (uintptr_t)a.votes % 8 == 0 &&
                   (uintptr_t)a.vote_mask % 8 == 0 && (uintptr_t)a.xyz % 4 == 0 && (uintptr_t)a.pc % 4 == 0 && (uintptr_t)a.choices % 4 == 0,
               PCMI_ERR_INVALID, "%s: misaligned pointer (8 bytes for fp64 and int64, 4 for fp32 and int32)", who);
  sample_kernel<<<(unsigned)ceil_div((int64_t)a.B * a.P, kThreads), kThreads, 0, as_stream(stream)>>>(a);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

}  // namespace detinput
}  // namespace pcmi

using namespace pcmi;
using namespace pcmi::detinput;

extern "C" {

int pcmi_det_sample_transform(const float* xyz, const int64_t* offsets, int64_t n, int64_t B, int64_t num_points, const int32_t* choices,
                              int augment, const int32_t* flip, const double* rot, const double* scale, const int32_t* instance,
                              const int32_t* semantic, float* point_clouds, int32_t* out_instance, int32_t* out_semantic, int32_t* flags,
                              pcmi_stream_t stream) {
  PCMI_REQUIRE(B >= 1 && B <= kMaxScenes, PCMI_ERR_INVALID, "det_sample_transform: 1 <= B %lld <= %d", (long long)B, kMaxScenes);
  PCMI_REQUIRE((instance == nullptr) == (out_instance == nullptr) && (semantic == nullptr) == (out_semantic == nullptr), PCMI_ERR_INVALID,
               "det_sample_transform: a payload and its output go together");
  SampleArgs a{xyz, offsets, n, (int)B, num_points, choices, augment ? 1 : 0, flip, rot, scale, instance, semantic, nullptr,
               point_clouds, out_instance, out_semantic, nullptr, nullptr, flags};
  return sample_common("det_sample_transform", a, stream);
}

int pcmi_det_votes_transform(const float* xyz, const double* votes, const int64_t* offsets, int64_t n, int64_t B, int64_t num_points,
                             const int32_t* choices, int augment, const int32_t* flip, const double* rot, const double* scale,
                             float* point_clouds, float* vote_label, int64_t* vote_label_mask, int32_t* flags, pcmi_stream_t stream) {
  PCMI_REQUIRE(B >= 1 && B <= kMaxScenes, PCMI_ERR_INVALID, "det_votes_transform: 1 <= B %lld <= %d", (long long)B, kMaxScenes);
  PCMI_REQUIRE(vote_label && vote_label_mask && (n == 0 || votes), PCMI_ERR_INVALID, "det_votes_transform: null pointer");
  SampleArgs a{xyz, offsets, n, (int)B, num_points, choices, augment ? 1 : 0, flip, rot, scale, nullptr, nullptr, votes,
               point_clouds, nullptr, nullptr, vote_label, vote_label_mask, flags};
  return sample_common("det_votes_transform", a, stream);
}

size_t pcmi_det_votes_from_instances_workspace_bytes(int64_t B) {
  if (B < 1 || B > kMaxScenes) return 0;
  return align_up((size_t)B * kMaxInst * 7 * 4, 256);
}

int pcmi_det_votes_from_instances(const float* point_clouds, const int32_t* instance, const int32_t* semantic, int64_t B,
                                  int64_t num_points, const int32_t* valid_sem, int n_valid, float* vote_label, int64_t* vote_label_mask,
                                  int32_t* flags, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_REQUIRE(shape_ok(B, num_points), PCMI_ERR_INVALID,
               "det_votes_from_instances: bad shape (1 <= B %lld <= %d; 1 <= num_points %lld, B num_points <= 2^29)", (long long)B,
               kMaxScenes, (long long)num_points);
  PCMI_REQUIRE(n_valid >= 0 && n_valid <= kMaxValid, PCMI_ERR_INVALID, "det_votes_from_instances: 0 <= n_valid %d <= %d", n_valid, kMaxValid);
  PCMI_REQUIRE(point_clouds && instance && semantic && vote_label && vote_label_mask && flags && (n_valid == 0 || valid_sem),
               PCMI_ERR_INVALID, "det_votes_from_instances: null pointer");
  PCMI_REQUIRE((uintptr_t)vote_label_mask % 8 == 0 && (uintptr_t)point_clouds % 4 == 0 && (uintptr_t)vote_label % 4 == 0, PCMI_ERR_INVALID,
               "det_votes_from_instances: misaligned pointer");
  if (int rc = require_ws("det_votes_from_instances", ws, ws_bytes, pcmi_det_votes_from_instances_workspace_bytes(B), 16)) return rc;
  hipStream_t st = as_stream(stream);
  uint32_t* tab = static_cast<uint32_t*>(ws);
  const int64_t total = B * kMaxInst * 7;
  vi_init_kernel<<<(unsigned)ceil_div(total, kThreads), kThreads, 0, st>>>(tab, total);
  PCMI_LAUNCH_CHECK();
  vi_reduce_kernel<<<dim3((unsigned)ceil_div(num_points, kInstRows), (unsigned)B), kThreads, 0, st>>>(point_clouds, instance, num_points, tab,
                                                                                                       flags);
  PCMI_LAUNCH_CHECK();
  vi_apply_kernel<<<(unsigned)ceil_div(B * num_points, kThreads), kThreads, 0, st>>>(point_clouds, instance, semantic, num_points, (int)B,
                                                                                      valid_sem, n_valid, tab, vote_label, vote_label_mask);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

int pcmi_det_box_labels(const double* boxes, const int32_t* n_boxes, int64_t B, int mode, int augment, const int32_t* flip, const double* rot,
                        const double* rot_angle, const double* scale, const double* heading_cs, const int32_t* label_to_class, int n_lut,
                        const double* mean_size, int n_class, int num_heading_bin, float* center_label, int64_t* heading_class_label,
                        float* heading_residual_label, int64_t* size_class_label, float* size_residual_label, int64_t* sem_cls_label,
                        float* box_label_mask, int32_t* flags, pcmi_stream_t stream) {
  PCMI_REQUIRE(B >= 1 && B <= kMaxScenes, PCMI_ERR_INVALID, "det_box_labels: 1 <= B %lld <= %d", (long long)B, kMaxScenes);
  PCMI_REQUIRE(mode == PCMI_DET_SCANNET || mode == PCMI_DET_SUNRGBD, PCMI_ERR_INVALID, "det_box_labels: mode %d (0 ScanNet, 1 SUN RGB-D)", mode);
  PCMI_REQUIRE(n_class >= 1 && n_class <= 65536 && n_lut >= 0 && num_heading_bin >= 1 && num_heading_bin <= 65536, PCMI_ERR_INVALID,
               "det_box_labels: n_class %d, n_lut %d, num_heading_bin %d", n_class, n_lut, num_heading_bin);
  PCMI_REQUIRE(boxes && n_boxes && mean_size && center_label && heading_class_label && heading_residual_label && size_class_label &&
                   size_residual_label && sem_cls_label && box_label_mask && flags,
               PCMI_ERR_INVALID, "det_box_labels: null pointer");
  PCMI_REQUIRE(mode == PCMI_DET_SUNRGBD ? heading_cs != nullptr : (n_lut > 0 && label_to_class), PCMI_ERR_INVALID,
               "det_box_labels: ScanNet needs label_to_class, SUN RGB-D needs heading_cs");
  PCMI_REQUIRE(!augment || (flip && rot && (mode == PCMI_DET_SCANNET || (rot_angle && scale))), PCMI_ERR_INVALID,
               "det_box_labels: augment needs flip and rot, and for SUN RGB-D rot_angle and scale");
  PCMI_REQUIRE((uintptr_t)boxes % 8 == 0 && (uintptr_t)rot % 8 == 0 && (uintptr_t)rot_angle % 8 == 0 && (uintptr_t)scale % 8 == 0 &&
                   (uintptr_t)heading_cs % 8 == 0 && (uintptr_t)mean_size % 8 == 0 && (uintptr_t)heading_class_label % 8 == 0 &&
                   (uintptr_t)size_class_label % 8 == 0 && (uintptr_t)sem_cls_label % 8 == 0,
               PCMI_ERR_INVALID, "det_box_labels: misaligned pointer (8 bytes for fp64 and int64)");
  BoxArgs a{boxes, n_boxes, (int)B, mode, augment ? 1 : 0, flip, rot, rot_angle, scale, heading_cs, label_to_class, n_lut, mean_size, n_class,
            num_heading_bin, center_label, heading_class_label, heading_residual_label, size_class_label, size_residual_label, sem_cls_label,
            box_label_mask, flags};
  box_kernel<<<(unsigned)ceil_div(B * kMaxObj, kThreads), kThreads, 0, as_stream(stream)>>>(a);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

// the workspace of the pcmi_seg_quantize call inside
struct DetVoxWs { int32_t* vox; uint8_t* keep; int32_t* scene_min; int64_t *offs, *index; void* quantize; size_t quantize_bytes, bytes; };
static DetVoxWs det_vox_ws(void* ws, int64_t B, int64_t num_points) {
  const size_t N = (size_t)(B * num_points);
  Carve cv{(char*)ws};
  DetVoxWs w;
  w.vox = cv.take<int32_t>(N * 3);
  w.keep = cv.take<uint8_t>(N);
  w.scene_min = cv.take<int32_t>((size_t)B * 3);
  w.offs = cv.take<int64_t>((size_t)B + 1);
  w.index = cv.take<int64_t>(N);
  w.quantize_bytes = pcmi_seg_quantize_workspace_bytes((int64_t)N);
  w.quantize = cv.take<char>(w.quantize_bytes);
  w.bytes = cv.used;
  return w;
}

size_t pcmi_det_voxelize_workspace_bytes(int64_t B, int64_t num_points) {
  if (!shape_ok(B, num_points)) return 0;
  return det_vox_ws(nullptr, B, num_points).bytes;
}

int pcmi_det_voxelize(const float* point_clouds, int64_t B, int64_t num_points, double voxel_size, int32_t* voxel_coords, int32_t* voxel_inds,
                      float* voxel_feats, int64_t* counts, int32_t* flags, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_REQUIRE(shape_ok(B, num_points), PCMI_ERR_INVALID,
               "det_voxelize: bad shape (1 <= B %lld <= %d; 1 <= num_points %lld, B num_points <= 2^29)", (long long)B, kMaxScenes,
               (long long)num_points);
  const float vs = (float)voxel_size;
  PCMI_REQUIRE(vs > 0.f && vs < 3.0e38f, PCMI_ERR_INVALID, "det_voxelize: voxel_size must be positive and finite in fp32");
  PCMI_REQUIRE(point_clouds && voxel_coords && voxel_inds && voxel_feats && counts && flags, PCMI_ERR_INVALID, "det_voxelize: null pointer");
  PCMI_REQUIRE((uintptr_t)counts % 8 == 0 && (uintptr_t)point_clouds % 4 == 0 && (uintptr_t)voxel_coords % 4 == 0, PCMI_ERR_INVALID,
               "det_voxelize: misaligned pointer");
  if (int rc = require_ws("det_voxelize", ws, ws_bytes, det_vox_ws(nullptr, B, num_points).bytes, 16)) return rc;
  const int64_t N = B * num_points;
  const DetVoxWs w = det_vox_ws(ws, B, num_points);
  hipStream_t st = as_stream(stream);
  const unsigned grid = (unsigned)ceil_div(N, kThreads);
  vx_init_kernel<<<(unsigned)ceil_div(3 * B + 1, kThreads), kThreads, 0, st>>>(w.scene_min, w.offs, (int)B, num_points);
  PCMI_LAUNCH_CHECK();
  vx_point_kernel<<<grid, kThreads, 0, st>>>(point_clouds, num_points, (int)B, vs, w.vox, w.keep, w.scene_min, flags);
  PCMI_LAUNCH_CHECK();
  vx_min_kernel<<<(unsigned)ceil_div(3 * B, kThreads), kThreads, 0, st>>>(w.scene_min, (int)B);
  PCMI_LAUNCH_CHECK();
  const int rc = pcmi_seg_quantize(w.vox, w.keep, nullptr, w.offs, w.scene_min, N, B, 0, voxel_coords, w.index, nullptr, counts, flags, w.quantize,
                                   w.quantize_bytes, stream);
  if (rc != PCMI_OK) return rc;
  vx_close_kernel<<<grid, kThreads, 0, st>>>(voxel_coords, w.index, counts, w.scene_min, (int)B, num_points, voxel_inds, voxel_feats);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

}  // extern "C"
