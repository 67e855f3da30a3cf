// Exactly rounded fp64 arithmetic for the kernels whose outputs are defined bit for bit by include/pcmi.h: one IEEE
// round-to-nearest operation per call, in the order the caller writes them, wherever the call is inlined.
//
// hipcc contracts a * b + c into an FMA by default.  Every function here that rounds therefore opens its body with
// `#pragma clang fp contract(off)` and uses the plain operators under it: the pragma travels with the function's
// instructions when it is inlined, so the product and the sum stay two operations even in a translation unit that allows
// contraction.  The __dmul_rn / __dadd_rn intrinsics do NOT give that: they are plain operators in a system header compiled
// with contraction allowed, and once inlined their product and sum are fused again.  There is no file-scope pragma here (it
// would leak into whatever is included next): a .hip file keeps its own for the arithmetic it writes inline.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pcmi {

__device__ inline double mul_rn(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ inline double add_rn(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ inline double div_rn(double a, double b) {
#pragma clang fp contract(off)
  return a / b;
}

__device__ inline bool finite3(double x, double y, double z) { return isfinite(x) && isfinite(y) && isfinite(z); }
__device__ inline double qnan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ inline double pinf() { return __longlong_as_double(0x7ff0000000000000ll); }

// order-preserving integer images: a < b  <=>  image(a) < image(b), for every pair of non-NaN values, so that an integer
// atomic min / max reduces floats.  -0.0 sorts below +0.0
__device__ inline uint32_t ord32(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ inline float unord32(uint32_t u) { return __uint_as_float((u >> 31) ? (u & 0x7fffffffu) : ~u); }
__device__ inline unsigned long long ord64(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ inline double unord64(unsigned long long u) {
  return __longlong_as_double((long long)((u >> 63) ? (u & 0x7fffffffffffffffull) : ~u));
}

// o_r = ((m[r,0] p0 + m[r,1] p1) + m[r,2] p2) + m[r,3] for the rows r = 0 .. 2 of a 3 x 4 block with row stride ld
__device__ inline void rigid_apply(const double* m, int ld, const double* p, double* o) {
#pragma clang fp contract(off)
#pragma unroll
  for (int r = 0; r < 3; ++r) o[r] = ((m[ld * r] * p[0] + m[ld * r + 1] * p[1]) + m[ld * r + 2] * p[2]) + m[ld * r + 3];
}

// (ex ex + ey ey) + ez ez, e = a - b
__device__ inline double dist2_rn(const double* a, const double* b) {
#pragma clang fp contract(off)
  const double ex = a[0] - b[0], ey = a[1] - b[1], ez = a[2] - b[2];
  return (ex * ex + ey * ey) + ez * ez;
}

}  // namespace pcmi
