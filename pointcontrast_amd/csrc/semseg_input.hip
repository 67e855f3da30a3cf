// The input side of semantic-segmentation fine-tuning for a BATCH of scans, on the device: what the reference does per scan
// on the host in downstream/semseg/lib/dataset.py:275-298 --
//   * ElasticDistortion: noise grid from the extent, two rounds of a box filter, trilinear lookup (lib/transforms.py:187-217)
//   * Voxelizer.voxelize: clip, homogeneous transform, floor, alignment to the origin        (lib/voxelizer.py:81-142)
//   * ME.utils.sparse_quantize(coords, feats, labels, ignore_label)                            (lib/voxelizer.py:145-146)
//   * RandomHorizontalFlip, ChromaticAutoContrast, ChromaticTranslation, ChromaticJitter       (lib/transforms.py:23-74,161-179)
//   * feats / 255 - 0.5 and the label map                                                      (lib/train.py:114-115, dataset.py:297-298)
// Written from the semantics in include/pcmi.h; gfx950, wave64.  Every random quantity is an input.
//
// Arithmetic, as nearest.hip: every fp64 product and sum is an explicit round-to-nearest operation in the order pcmi.h states
// (no FMA contraction).  The only atomics are integer minima, maxima and ors (a double or float is reduced through its
// order-preserving integer image), whose result does not depend on the order of arrival, and the compare-and-swap that
// claims a table slot, whose outcome -- WHICH slot a voxel gets -- never reaches an output: rows leave in the order of
// an exclusive scan over "is the lowest row of its voxel".  Every output is the same bits from run to run.
#include <algorithm>
#include <climits>

#include "cubscan.h"
#include "exact.h"
#include "firstrow.h"
#include "internal.h"

#pragma clang fp contract(off)

namespace pcmi {
namespace seginput {

constexpr int kThreads = 256;
constexpr int kMaxScenes = 1023;        // pack_key's 10-bit batch field, minus the one value that could spell the empty key
constexpr int kVoxelLimit = 1 << 20;    // |voxel coordinate| < 2^20 (the loader's range, csrc/loader.hip)
constexpr int kSpan = 1 << 18;          // 0 <= x - min < 2^18: pack_key's 18-bit fields
constexpr int64_t kMaxRows = 1ll << 29; // table of 2 n slots, scanned with 32-bit counts

// true when every lane of the wave is active and carries the same scene b >= 0: one lane then speaks for all
__device__ inline bool wave_uniform(int b, bool active) {
  const int b0 = __shfl(b, 0, 64);
  return __all(active && b == b0 && b >= 0) != 0;
}

// ---- transform and clip ----------------------------------------------------------------------------------------------------
// ws of pcmi_seg_transform: per scene 6 order images, (min x, min y, min z, max x, max y, max z) of its finite points
__global__ __launch_bounds__(kThreads) void tf_init_kernel(unsigned long long* __restrict__ box, int32_t* __restrict__ scene_min, int B) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t < 6 * B) box[t] = (t % 6) < 3 ? ~0ull : 0ull;
  if (t < 3 * B) scene_min[t] = INT_MAX;
}

__global__ __launch_bounds__(kThreads) void tf_box_kernel(const double* __restrict__ xyz, int64_t n, const int64_t* __restrict__ offs, int B,
                                                          unsigned long long* box) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool in = i < n;
  const int b = in ? segment_of(offs, B, i) : -1;
  double p[3] = {0.0, 0.0, 0.0};
  bool ok = false;
  if (b >= 0) {
    p[0] = xyz[3 * i], p[1] = xyz[3 * i + 1], p[2] = xyz[3 * i + 2];
    ok = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
  }
  unsigned long long lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = ok ? ord64(p[a]) : ~0ull;
    hi[a] = ok ? ord64(p[a]) : 0ull;
  }
  if (wave_uniform(b, in)) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        lo[a] = std::min(lo[a], (unsigned long long)__shfl_xor((long long)lo[a], d, 64));
        hi[a] = std::max(hi[a], (unsigned long long)__shfl_xor((long long)hi[a], d, 64));
      }
    if ((threadIdx.x & 63) != 0) return;
  } else if (!ok) {
    return;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (lo[a] != ~0ull) atomicMin(&box[6 * b + a], lo[a]);
    if (hi[a] != 0ull) atomicMax(&box[6 * b + 3 + a], hi[a]);
  }
}

struct Clip {
  int mode;      // 0 none, 1 numeric bound, 2 per-axis bounds
  double lim[6]; // mode 1: lim[0]; mode 2: (lo, hi) per axis
};

__global__ __launch_bounds__(kThreads) void tf_point_kernel(const double* __restrict__ xyz, int64_t n, const int64_t* __restrict__ offs, int B,
                                                            const double* __restrict__ mats, Clip clip,
                                                            const double* __restrict__ ratio, const unsigned long long* __restrict__ box,
                                                            int32_t* __restrict__ vox, uint8_t* __restrict__ keep, int32_t* scene_min,
                                                            int32_t* flags) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool in = i < n;
  const int b = in ? segment_of(offs, B, i) : -1;
  bool kept = false;
  int v[3] = {INT_MAX, INT_MAX, INT_MAX};
  if (b >= 0) {
    const double p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    bool ok = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
    bool bad = !ok;
    if (ok && clip.mode != 0) {
      double size[3], center[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const double mn = unord64(box[6 * b + a]), mx = unord64(box[6 * b + 3 + a]);
        size[a] = add_rn(mx, -mn);
        center[a] = add_rn(mn, mul_rn(size[a], 0.5));
        center[a] = add_rn(center[a], mul_rn(ratio ? ratio[3 * b + a] : 0.0, size[a]));
      }
      if (clip.mode == 1) {
        const double lim = clip.lim[0];
        if (!(fmax(fmax(size[0], size[1]), size[2]) < lim)) {
#pragma unroll
          for (int a = 0; a < 3; ++a) ok = ok && p[a] >= add_rn(-lim, center[a]) && p[a] < add_rn(lim, center[a]);
        }
      } else {
#pragma unroll
        for (int a = 0; a < 3; ++a) ok = ok && p[a] >= add_rn(clip.lim[2 * a], center[a]) && p[a] < add_rn(clip.lim[2 * a + 1], center[a]);
      }
    }
    if (ok) {
      double t[3];
      rigid_apply(mats + 16 * b, 4, p, t);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double f = floor(t[r]);
        if (!(fabs(f) < (double)kVoxelLimit)) {  // NaN included
          bad = true;
          ok = false;
        } else {
          v[r] = (int)f;
        }
      }
    }
    if (bad) atomicOr(&flags[b], PCMI_SEG_FLAG_RANGE);
    kept = ok;
    vox[3 * i] = kept ? v[0] : 0;
    vox[3 * i + 1] = kept ? v[1] : 0;
    vox[3 * i + 2] = kept ? v[2] : 0;
    keep[i] = kept ? 1 : 0;
  } else if (in) {
    vox[3 * i] = vox[3 * i + 1] = vox[3 * i + 2] = 0;
    keep[i] = 0;
  }
  if (!kept) v[0] = v[1] = v[2] = INT_MAX;
  if (wave_uniform(b, in)) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) v[a] = std::min(v[a], __shfl_xor(v[a], d, 64));
    if ((threadIdx.x & 63) != 0) return;
  } else if (!kept) {
    return;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
    if (v[a] != INT_MAX) atomicMin(&scene_min[3 * b + a], v[a]);
}

// a scene without a kept point has the minimum 0; aligned = M_t M with M_t the translation by -min
__global__ __launch_bounds__(kThreads) void tf_final_kernel(const double* __restrict__ mats, int B, int32_t* __restrict__ scene_min,
                                                            double* __restrict__ aligned) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= B) return;
  const double* m = mats + 16 * b;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    int mn = scene_min[3 * b + r];
    if (mn == INT_MAX) scene_min[3 * b + r] = mn = 0;
    const double t = -(double)mn;
    for (int c = 0; c < 4; ++c) aligned[16 * b + 4 * r + c] = add_rn(m[4 * r + c], mul_rn(t, m[12 + c]));
  }
  for (int c = 0; c < 4; ++c) aligned[16 * b + 12 + c] = m[12 + c];
}

// ---- quantize --------------------------------------------------------------------------------------------------------------
// pass 1: the row's voxel claims its slot; first[slot] = the lowest row of the voxel
__global__ __launch_bounds__(kThreads) void q_insert_kernel(const int32_t* __restrict__ vox, const uint8_t* __restrict__ keep, int64_t n,
                                                            const int64_t* __restrict__ offs, int B, const int32_t* __restrict__ scene_min,
                                                            uint64_t* keys, uint32_t mask, uint32_t* first, uint32_t* __restrict__ slot_of,
                                                            int32_t* flags) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  uint32_t slot = kNoSlot;
  const int b = segment_of(offs, B, i);
  if (b >= 0 && (!keep || keep[i])) {
    int64_t d[3];
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      d[a] = (int64_t)vox[3 * i + a] - (int64_t)(scene_min ? scene_min[3 * b + a] : 0);
      ok = ok && d[a] >= 0 && d[a] < kSpan;
    }
    if (ok) {
      slot = claim_first(keys, 0, mask + 1, pack_key(b, (int)d[0] - kCoordBias, (int)d[1] - kCoordBias, (int)d[2] - kCoordBias), first, i);
    } else {
      atomicOr(&flags[b], PCMI_SEG_FLAG_SPAN);
    }
  }
  slot_of[i] = slot;
}

// pass 2: is this row its voxel's first?  does its label differ from the first row's?
__global__ __launch_bounds__(kThreads) void q_label_kernel(int64_t n, const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ first,
                                                           const int32_t* __restrict__ labels, int32_t* mixed, int32_t* __restrict__ is_first) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t slot = slot_of[i];
  const int f = is_first_row(slot, first, i) ? 1 : 0;
  if (labels && !f && slot != kNoSlot && labels[i] != labels[first[slot]]) atomicOr(&mixed[slot], 1);
  is_first[i] = f;
}

// pass 3 (after the exclusive scan pos of is_first over n + 1 items): the first rows leave in ascending order
__global__ __launch_bounds__(kThreads) void q_write_kernel(const int32_t* __restrict__ vox, int64_t n, const int64_t* __restrict__ offs, int B,
                                                           const int32_t* __restrict__ scene_min, const uint32_t* __restrict__ slot_of,
                                                           const int32_t* __restrict__ is_first, const int32_t* __restrict__ pos,
                                                           const int32_t* __restrict__ labels, const int32_t* __restrict__ mixed,
                                                           int32_t ignore_label, int32_t* __restrict__ coords, int64_t* __restrict__ index,
                                                           int32_t* __restrict__ out_labels, int64_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  segment_counts(i, offs, B, n, pos, counts);  // counts[b] = voxels of scene b; counts[B] = all
  if (i >= n || !is_first[i]) return;
  const int b = segment_of(offs, B, i);
  const int64_t p = pos[i];
  coords[4 * p] = b;
#pragma unroll
  for (int a = 0; a < 3; ++a) coords[4 * p + 1 + a] = vox[3 * i + a] - (scene_min ? scene_min[3 * b + a] : 0);
  index[p] = i;
  if (out_labels) out_labels[p] = mixed[slot_of[i]] ? ignore_label : labels[i];
}

// ---- flip, colour, label map -------------------------------------------------------------------------------------------------
// ws of pcmi_seg_color_augment: per scene 9 words -- max x, y, z (int32), then the order images of min r, g, b and max r, g, b
__global__ __launch_bounds__(kThreads) void ca_init_kernel(uint32_t* __restrict__ red, int B) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= 9 * B) return;
  const int w = t % 9;
  red[t] = w < 3 ? (uint32_t)INT_MIN : (w < 6 ? 0xffffffffu : 0u);
}

__device__ inline int64_t src_row(const int64_t* __restrict__ index, int64_t p, int64_t n_src) {
  const int64_t s = index ? index[p] : p;
  return (s >= 0 && s < n_src) ? s : -1;
}

__global__ __launch_bounds__(kThreads) void ca_reduce_kernel(const float* __restrict__ src, int64_t n_src, const int64_t* __restrict__ index,
                                                             const int32_t* __restrict__ coords, int64_t m, int B, uint32_t* red) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool in = p < m;
  int b = in ? coords[4 * p] : -1;
  if (b < 0 || b >= B) b = -1;
  int cmax[3] = {INT_MIN, INT_MIN, INT_MIN};
  uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  if (b >= 0) {
    const int64_t s = src_row(index, p, n_src);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      cmax[a] = coords[4 * p + 1 + a];
      const float f = s >= 0 ? src[3 * s + a] : 0.f;
      if (s >= 0 && !isnan(f)) lo[a] = hi[a] = ord32(f);
    }
  }
  if (wave_uniform(b, in)) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        cmax[a] = std::max(cmax[a], __shfl_xor(cmax[a], d, 64));
        lo[a] = std::min(lo[a], (uint32_t)__shfl_xor((int)lo[a], d, 64));
        hi[a] = std::max(hi[a], (uint32_t)__shfl_xor((int)hi[a], d, 64));
      }
    if ((threadIdx.x & 63) != 0) return;
  } else if (b < 0) {
    return;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    atomicMax(reinterpret_cast<int*>(&red[9 * b + a]), cmax[a]);
    if (lo[a] != 0xffffffffu) atomicMin(&red[9 * b + 3 + a], lo[a]);
    if (hi[a] != 0u) atomicMax(&red[9 * b + 6 + a], hi[a]);
  }
}

__device__ inline double clip255(double v) { return fmin(fmax(v, 0.0), 255.0); }

__global__ __launch_bounds__(kThreads) void ca_apply_kernel(const float* __restrict__ src, int64_t n_src, const int64_t* __restrict__ index,
                                                            int32_t* __restrict__ coords, int32_t* __restrict__ labels, int64_t m, int B,
                                                            const double* __restrict__ params, const float* __restrict__ normals,
                                                            int normalize, const int32_t* __restrict__ lut, int64_t lut_n,
                                                            int32_t ignore_label, const uint32_t* __restrict__ red,
                                                            float* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= m) return;
  const int b = coords[4 * p];
  const bool scene = params && b >= 0 && b < B;
  const double* q = scene ? params + 12 * b : nullptr;
  const int64_t s = src_row(index, p, n_src);
  if (labels && lut) {
    const int32_t l = labels[p];
    labels[p] = (l >= 0 && l < lut_n) ? lut[l] : ignore_label;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (scene && q[a] != 0.0) coords[4 * p + 1 + a] = (int)red[9 * b + a] - coords[4 * p + 1 + a];
    double f = s >= 0 ? (double)src[3 * s + a] : 0.0;
    if (scene) {
      if (q[3] != 0.0) {  // auto-contrast; a channel with hi == lo (or without a number) stays as it is
        const uint32_t ulo = red[9 * b + 3 + a], uhi = red[9 * b + 6 + a];
        if (ulo < uhi) {
          const double lo = (double)unord32(ulo), hi = (double)unord32(uhi);
          const double scale = 255.0 / add_rn(hi, -lo);
          const double cf = mul_rn(add_rn(f, -lo), scale);
          f = add_rn(mul_rn(add_rn(1.0, -q[4]), f), mul_rn(q[4], cf));
        }
      }
      if (q[5] != 0.0) f = clip255(add_rn(q[6 + a], f));
      if (q[9] != 0.0 && normals) f = clip255(add_rn(mul_rn((double)normals[3 * p + a], q[10]), f));
    }
    if (normalize) f = add_rn(f / 255.0, -0.5);
    out[3 * p + a] = (float)f;
  }
}

static bool batch_ok(int64_t n, int64_t B) { return n >= 0 && n < (1ll << 31) - kThreads && B >= 1 && B <= kMaxScenes; }

// ---- elastic distortion (transforms.py:187-217) ---------------------------------------------------------------------------
// numpy's a // b for doubles a >= 0, b > 0 (npy_divmod): the quotient of a - fmod(a, b), floored, and rounded up when it sits
// within 0.5 below an integer
__device__ inline double np_floor_div(double a, double b) {
  const double mod = fmod(a, b);
  const double div = add_rn(a, -mod) / b;
  if (div == 0.0) return 0.0;
  double fl = floor(div);
  if (add_rn(div, -fl) > 0.5) fl = add_rn(fl, 1.0);
  return fl;
}

__global__ __launch_bounds__(kThreads) void el_box_reset_kernel(unsigned long long* __restrict__ box, int B) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t < 6 * B) box[t] = (t % 6) < 3 ? ~0ull : 0ull;  // a minimum of all ones: the scene has no finite point
}

// one thread per scene: grid_min = the box minimum, grid_dims = ((max - min) // g) + 3 and whether the scene is distorted
// (active, has a finite point, fits the capacity); a scene that does not fit is flagged
__global__ __launch_bounds__(kThreads) void el_dims_kernel(const unsigned long long* __restrict__ box, int B, double g,
                                                           const int32_t* __restrict__ active, int cx, int cy, int cz,
                                                           int32_t* __restrict__ grid_dims, double* __restrict__ grid_min,
                                                           int32_t* flags) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= B) return;
  const int cap[3] = {cx, cy, cz};
  const bool has = box[6 * b] != ~0ull;
  bool fits = true;
  int d[3] = {0, 0, 0};
  double mn[3] = {0.0, 0.0, 0.0};
  if (has) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      mn[a] = unord64(box[6 * b + a]);
      const double q = add_rn(np_floor_div(add_rn(unord64(box[6 * b + 3 + a]), -mn[a]), g), 3.0);
      if (!(q <= (double)cap[a])) fits = false; else d[a] = (int)q;
    }
  }
  const bool on = has && (!active || active[b] != 0);
  if (on && !fits) atomicOr(&flags[b], PCMI_SEG_FLAG_ELASTIC);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    grid_dims[4 * b + a] = fits ? d[a] : 0;
    grid_min[3 * b + a] = mn[a];
  }
  grid_dims[4 * b + 3] = (on && fits) ? 1 : 0;
}

// one 3-tap pass along `axis` over the capacity blocks: dst = float(((src[i-1] w + src[i] w) + src[i+1] w)), taps outside the
// scene's dims are 0; elements outside the dims, and scenes that are not distorted, are not written
__global__ __launch_bounds__(kThreads) void el_blur_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t total, int cx,
                                                           int cy, int cz, const int32_t* __restrict__ grid_dims, int axis) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= total) return;
  int64_t r = t / 3;
  const int z = (int)(r % cz);
  r /= cz;
  const int y = (int)(r % cy);
  r /= cy;
  const int x = (int)(r % cx);
  const int b = (int)(r / cx);
  const int32_t* d = grid_dims + 4 * b;
  if (!d[3] || x >= d[0] || y >= d[1] || z >= d[2]) return;
  const int64_t stride = axis == 0 ? (int64_t)cy * cz * 3 : (axis == 1 ? (int64_t)cz * 3 : 3);
  const int i = axis == 0 ? x : (axis == 1 ? y : z);
  const double w = (double)(1.0f / 3.0f);
  const double lo = i > 0 ? (double)src[t - stride] : 0.0;
  const double hi = i + 1 < d[axis] ? (double)src[t + stride] : 0.0;
  dst[t] = (float)add_rn(add_rn(mul_rn(lo, w), mul_rn((double)src[t], w)), mul_rn(hi, w));
}

// np.linspace(start, stop, d)[i]
__device__ inline double el_node(double start, double stop, double step, int i, int d) {
  return i == d - 1 ? stop : add_rn(mul_rn((double)i, step), start);
}

__global__ __launch_bounds__(kThreads) void el_apply_kernel(double* __restrict__ xyz, int64_t n, const int64_t* __restrict__ offs, int B,
                                                            double g, double magnitude, const float* __restrict__ noise, int cx, int cy,
                                                            int cz, const int32_t* __restrict__ grid_dims,
                                                            const double* __restrict__ grid_min) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int b = segment_of(offs, B, i);
  if (b < 0 || !grid_dims[4 * b + 3]) return;
  const int cap[3] = {cx, cy, cz};
#pragma unroll
  for (int a = 0; a < 3; ++a)
    if (grid_dims[4 * b + a] < 3 || grid_dims[4 * b + a] > cap[a]) return;  // not a grid of this block: nothing is read
  const double p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
  int idx[3];
  double wt[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int d = grid_dims[4 * b + a];
    const double start = add_rn(grid_min[3 * b + a], -g);
    const double stop = add_rn(grid_min[3 * b + a], mul_rn(g, (double)(d - 2)));
    const double step = add_rn(stop, -start) / (double)(d - 1);
    if (!(p[a] >= start && p[a] <= stop)) return;  // outside the grid (NaN included): adds 0
    int k = (int)fmin(fmax(floor(add_rn(p[a], -start) / step), 0.0), (double)(d - 2));
    while (k > 0 && el_node(start, stop, step, k, d) > p[a]) --k;
    while (k < d - 2 && el_node(start, stop, step, k + 1, d) <= p[a]) ++k;
    const double x0 = el_node(start, stop, step, k, d), x1 = el_node(start, stop, step, k + 1, d);
    idx[a] = k;
    wt[a] = add_rn(p[a], -x0) / add_rn(x1, -x0);
  }
  const float* vol = noise + (int64_t)b * cx * cy * cz * 3;
  double val[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int c = 0; c < 8; ++c) {  // the corners with x slowest, the low node first; weight = ((1 wx) wy) wz
    const int ox = c >> 2, oy = (c >> 1) & 1, oz = c & 1;
    const double w = mul_rn(mul_rn(ox ? wt[0] : add_rn(1.0, -wt[0]), oy ? wt[1] : add_rn(1.0, -wt[1])), oz ? wt[2] : add_rn(1.0, -wt[2]));
    const float* v = vol + (((int64_t)(idx[0] + ox) * cy + (idx[1] + oy)) * cz + (idx[2] + oz)) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) val[ch] = add_rn(val[ch], mul_rn((double)v[ch], w));
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) xyz[3 * i + a] = add_rn(p[a], mul_rn(val[a], magnitude));
}

static bool cap_ok(int64_t B, int cx, int cy, int cz) {
  return cx >= 3 && cy >= 3 && cz >= 3 && cx <= 4096 && cy <= 4096 && cz <= 4096 && (int64_t)cx * cy * cz * 3 * B < (1ll << 31);
}

}  // namespace seginput
}  // namespace pcmi

using namespace pcmi;
using namespace pcmi::seginput;

extern "C" {

struct BlurWs { unsigned long long* box; float* tmp; size_t bytes; };
static BlurWs blur_ws(void* ws, int64_t B, int cx, int cy, int cz) {
  Carve cv{(char*)ws};
  BlurWs L;
  L.box = cv.take<unsigned long long>((size_t)B * 6);
  L.tmp = cv.take<float>((size_t)B * cx * cy * cz * 3);
  L.bytes = cv.used;
  return L;
}

size_t pcmi_elastic_blur_workspace_bytes(int64_t B, int cx, int cy, int cz) {
  if (B < 1 || B > kMaxScenes || !cap_ok(B, cx, cy, cz)) return 0;
  return blur_ws(nullptr, B, cx, cy, cz).bytes;
}

int pcmi_elastic_blur(const double* xyz, const int64_t* offsets, int64_t n, int64_t B, double granularity, const int32_t* active,
                      float* noise, int cx, int cy, int cz, int32_t* grid_dims, double* grid_min, int32_t* flags, void* ws,
                      size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_REQUIRE(batch_ok(n, B), PCMI_ERR_INVALID, "elastic_blur: bad shape (0 <= n %lld < 2^31 - 256; 1 <= B %lld <= %d)", (long long)n,
               (long long)B, kMaxScenes);
  PCMI_REQUIRE(cap_ok(B, cx, cy, cz), PCMI_ERR_INVALID, "elastic_blur: capacity (%d, %d, %d): 3..4096 each, B cx cy cz 3 < 2^31", cx, cy, cz);
  PCMI_REQUIRE(granularity > 0.0 && granularity < 1e300, PCMI_ERR_INVALID, "elastic_blur: granularity must be positive and finite");
  PCMI_REQUIRE(offsets && noise && grid_dims && grid_min && flags && (n == 0 || xyz), PCMI_ERR_INVALID, "elastic_blur: null pointer");
  if (int rc = require_ws("elastic_blur", ws, ws_bytes, blur_ws(nullptr, B, cx, cy, cz).bytes, 16)) return rc;
  hipStream_t st = as_stream(stream);
  const BlurWs L = blur_ws(ws, B, cx, cy, cz);
  el_box_reset_kernel<<<(unsigned)ceil_div(6 * B, kThreads), kThreads, 0, st>>>(L.box, (int)B);
  PCMI_LAUNCH_CHECK();
  if (n > 0) {
    tf_box_kernel<<<(unsigned)ceil_div(n, kThreads), kThreads, 0, st>>>(xyz, n, offsets, (int)B, L.box);
    PCMI_LAUNCH_CHECK();
  }
  el_dims_kernel<<<(unsigned)ceil_div(B, kThreads), kThreads, 0, st>>>(L.box, (int)B, granularity, active, cx, cy, cz, grid_dims, grid_min, flags);
  PCMI_LAUNCH_CHECK();
  const int64_t total = B * cx * cy * cz * 3;
  const unsigned grid = (unsigned)ceil_div(total, kThreads);
  for (int pass = 0; pass < 6; ++pass) {  // two rounds of x, y, z; an even number of passes ends in `noise`
    const float* src = (pass & 1) ? L.tmp : noise;
    float* dst = (pass & 1) ? noise : L.tmp;
    el_blur_kernel<<<grid, kThreads, 0, st>>>(src, dst, total, cx, cy, cz, grid_dims, pass % 3);
    PCMI_LAUNCH_CHECK();
  }
  return PCMI_OK;
}

int pcmi_elastic_apply(double* xyz, const int64_t* offsets, int64_t n, int64_t B, double granularity, double magnitude,
                       const float* noise, int cx, int cy, int cz, const int32_t* grid_dims, const double* grid_min,
                       pcmi_stream_t stream) {
  PCMI_REQUIRE(batch_ok(n, B), PCMI_ERR_INVALID, "elastic_apply: bad shape (0 <= n %lld < 2^31 - 256; 1 <= B %lld <= %d)", (long long)n,
               (long long)B, kMaxScenes);
  PCMI_REQUIRE(cap_ok(B, cx, cy, cz), PCMI_ERR_INVALID, "elastic_apply: capacity (%d, %d, %d): 3..4096 each, B cx cy cz 3 < 2^31", cx, cy, cz);
  PCMI_REQUIRE(granularity > 0.0 && granularity < 1e300 && magnitude == magnitude && fabs(magnitude) < 1e300, PCMI_ERR_INVALID,
               "elastic_apply: granularity must be positive and finite, magnitude finite");
  PCMI_REQUIRE(offsets && noise && grid_dims && grid_min && (n == 0 || xyz), PCMI_ERR_INVALID, "elastic_apply: null pointer");
  if (n == 0) return PCMI_OK;
  el_apply_kernel<<<(unsigned)ceil_div(n, kThreads), kThreads, 0, as_stream(stream)>>>(xyz, n, offsets, (int)B, granularity, magnitude, noise,
                                                                                        cx, cy, cz, grid_dims, grid_min);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

size_t pcmi_seg_transform_workspace_bytes(int64_t B) {
  if (B < 1 || B > kMaxScenes) return 0;
  return align_up((size_t)B * 6 * 8, 256);
}

int pcmi_seg_transform(const double* xyz, const int64_t* offsets, int64_t n, int64_t B, const double* mats, int clip_mode,
                       const double* clip_host, const double* trans_ratio, int32_t* vox, uint8_t* keep, int32_t* scene_min,
                       double* aligned, int32_t* flags, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_REQUIRE(batch_ok(n, B), PCMI_ERR_INVALID, "seg_transform: bad shape (0 <= n %lld < 2^31 - 256; 1 <= B %lld <= %d)", (long long)n,
               (long long)B, kMaxScenes);
  PCMI_REQUIRE(clip_mode >= 0 && clip_mode <= 2, PCMI_ERR_INVALID, "seg_transform: clip_mode %d (0 none, 1 numeric, 2 per axis)", clip_mode);
  PCMI_REQUIRE(offsets && mats && scene_min && aligned && flags && (n == 0 || (xyz && vox && keep)) && (clip_mode == 0 || clip_host),
               PCMI_ERR_INVALID, "seg_transform: null pointer");
  if (int rc = require_ws("seg_transform", ws, ws_bytes, pcmi_seg_transform_workspace_bytes(B), 16)) return rc;
  Clip clip;
  clip.mode = clip_mode;
  for (int q = 0; q < 6; ++q) clip.lim[q] = 0.0;
  if (clip_mode == 1) {
    clip.lim[0] = clip_host[0];
    PCMI_REQUIRE(clip.lim[0] == clip.lim[0], PCMI_ERR_INVALID, "seg_transform: the clip bound is NaN");
  } else if (clip_mode == 2) {
    for (int q = 0; q < 6; ++q) {
      clip.lim[q] = clip_host[q];
      PCMI_REQUIRE(clip.lim[q] == clip.lim[q], PCMI_ERR_INVALID, "seg_transform: a clip bound is NaN");
    }
  }
  hipStream_t st = as_stream(stream);
  unsigned long long* box = static_cast<unsigned long long*>(ws);
  tf_init_kernel<<<(unsigned)ceil_div(6 * B, kThreads), kThreads, 0, st>>>(box, scene_min, (int)B);
  PCMI_LAUNCH_CHECK();
  if (n > 0) {
    const unsigned grid = (unsigned)ceil_div(n, kThreads);
    if (clip_mode != 0) {
      tf_box_kernel<<<grid, kThreads, 0, st>>>(xyz, n, offsets, (int)B, box);
      PCMI_LAUNCH_CHECK();
    }
    tf_point_kernel<<<grid, kThreads, 0, st>>>(xyz, n, offsets, (int)B, mats, clip, trans_ratio, box, vox, keep, scene_min, flags);
    PCMI_LAUNCH_CHECK();
  }
  tf_final_kernel<<<(unsigned)ceil_div(B, kThreads), kThreads, 0, st>>>(mats, (int)B, scene_min, aligned);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

struct QuantizeWs { uint64_t* keys; uint32_t *first, *slot_of; int32_t *mixed, *is_first, *pos; void* temp; size_t temp_bytes, bytes; };
static QuantizeWs quantize_ws(void* ws, int64_t n) {
  const size_t cap = (size_t)table_cap(n);
  Carve cv{(char*)ws};
  QuantizeWs L;
  L.keys = cv.take<uint64_t>(cap);
  L.first = cv.take<uint32_t>(cap);
  L.mixed = cv.take<int32_t>(cap);
  L.slot_of = cv.take<uint32_t>((size_t)std::max<int64_t>(n, 1));
  L.is_first = cv.take<int32_t>((size_t)n + 1);
  L.pos = cv.take<int32_t>((size_t)n + 1);
  L.temp_bytes = cub_scan_bytes<int32_t>(n + 1);
  L.temp = cv.take<char>(L.temp_bytes);
  L.bytes = cv.used;
  return L;
}

size_t pcmi_seg_quantize_workspace_bytes(int64_t n) {
  if (n < 0 || n > kMaxRows) return 0;
  return quantize_ws(nullptr, n).bytes;
}

int pcmi_seg_quantize(const int32_t* vox, const uint8_t* keep, const int32_t* labels, const int64_t* offsets, const int32_t* scene_min,
                      int64_t n, int64_t B, int32_t ignore_label, int32_t* coords, int64_t* index, int32_t* out_labels, int64_t* counts,
                      int32_t* flags, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_REQUIRE(batch_ok(n, B), PCMI_ERR_INVALID, "seg_quantize: bad shape (0 <= n %lld < 2^31 - 256; 1 <= B %lld <= %d)", (long long)n,
               (long long)B, kMaxScenes);
  PCMI_REQUIRE(n <= kMaxRows, PCMI_ERR_UNSUPPORTED, "seg_quantize: %lld rows, at most 2^29", (long long)n);
  PCMI_REQUIRE(offsets && counts && flags && (n == 0 || (vox && coords && index)) && ((labels == nullptr) == (out_labels == nullptr)),
               PCMI_ERR_INVALID, "seg_quantize: null pointer (labels and out_labels go together)");
  if (int rc = require_ws("seg_quantize", ws, ws_bytes, quantize_ws(nullptr, n).bytes, 16)) return rc;
  hipStream_t st = as_stream(stream);
  if (n == 0) {
    PCMI_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)(B + 1) * 8, st));
    return PCMI_OK;
  }
  const int64_t cap = table_cap(n);
  const QuantizeWs L = quantize_ws(ws, n);
  const uint32_t mask = (uint32_t)(cap - 1);
  PCMI_HIP_CHECK(hipMemsetAsync(L.keys, 0xff, (size_t)cap * 8, st));
  PCMI_HIP_CHECK(hipMemsetAsync(L.first, 0xff, (size_t)cap * 4, st));
  PCMI_HIP_CHECK(hipMemsetAsync(L.mixed, 0, (size_t)cap * 4, st));
  PCMI_HIP_CHECK(hipMemsetAsync(L.is_first + n, 0, 4, st));
  const unsigned grid = (unsigned)ceil_div(n, kThreads);
  q_insert_kernel<<<grid, kThreads, 0, st>>>(vox, keep, n, offsets, (int)B, scene_min, L.keys, mask, L.first, L.slot_of, flags);
  PCMI_LAUNCH_CHECK();
  q_label_kernel<<<grid, kThreads, 0, st>>>(n, L.slot_of, L.first, labels, L.mixed, L.is_first);
  PCMI_LAUNCH_CHECK();
  if (int rc = cub_scan_excl(L.temp, L.temp_bytes, L.is_first, L.pos, n + 1, st)) return rc;
  q_write_kernel<<<(unsigned)ceil_div(std::max<int64_t>(n, B + 1), kThreads), kThreads, 0, st>>>(
      vox, n, offsets, (int)B, scene_min, L.slot_of, L.is_first, L.pos, labels, L.mixed, ignore_label, coords, index, out_labels, counts);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

size_t pcmi_seg_color_augment_workspace_bytes(int64_t B) {
  if (B < 1 || B > kMaxScenes) return 0;
  return align_up((size_t)B * 9 * 4, 256);
}

int pcmi_seg_color_augment(const float* feats_src, int64_t n_src, const int64_t* index, int32_t* coords, int32_t* labels, int64_t m,
                           int64_t B, const double* params, const float* normals, int normalize, const int32_t* lut, int64_t lut_n,
                           int32_t ignore_label, float* feats_out, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_REQUIRE(batch_ok(m, B) && n_src >= 0 && lut_n >= 0, PCMI_ERR_INVALID,
               "seg_color_augment: bad shape (0 <= m %lld < 2^31 - 256; 1 <= B %lld <= %d; n_src %lld, lut_n %lld >= 0)", (long long)m,
               (long long)B, kMaxScenes, (long long)n_src, (long long)lut_n);
  if (m == 0) return PCMI_OK;
  PCMI_REQUIRE(coords && feats_out && (n_src == 0 || feats_src) && (lut_n == 0 || lut), PCMI_ERR_INVALID, "seg_color_augment: null pointer");
  if (int rc = require_ws("seg_color_augment", ws, ws_bytes, pcmi_seg_color_augment_workspace_bytes(B), 16)) return rc;
  hipStream_t st = as_stream(stream);
  uint32_t* red = static_cast<uint32_t*>(ws);
  const unsigned grid = (unsigned)ceil_div(m, kThreads);
  if (params) {
    ca_init_kernel<<<(unsigned)ceil_div(9 * B, kThreads), kThreads, 0, st>>>(red, (int)B);
    PCMI_LAUNCH_CHECK();
    ca_reduce_kernel<<<grid, kThreads, 0, st>>>(feats_src, n_src, index, coords, m, (int)B, red);
    PCMI_LAUNCH_CHECK();
  }
  ca_apply_kernel<<<grid, kThreads, 0, st>>>(feats_src, n_src, index, coords, labels, m, (int)B, params, normals, normalize,
                                              lut_n > 0 ? lut : nullptr, lut_n, ignore_label, red, feats_out);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

}  // extern "C"
