// Scans of one value per thread over a workgroup of WAVES full waves (wave64), in thread order: a shuffle scan inside each
// wave, the wave totals through s_wave [WAVES] in LDS.  Every scan opens with a barrier, so that a call may reuse the
// s_wave of the call before it (whose readers are then done); all threads of the workgroup must call.
#pragma once
#include <hip/hip_runtime.h>

namespace pcmi {

// inclusive sum; total: the sum over all threads
template <int WAVES>
__device__ __forceinline__ int block_scan_add(int v, int* s_wave, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  __syncthreads();  // the previous call's readers are done
  if (lane == 63) s_wave[wave] = v;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const int x = s_wave[w];
    before += w < wave ? x : 0;
    all += x;
  }
  *total = all;
  return v + before;
}

// the same inclusive sum over unsigned 64-bit values (weights in fixed point: no order of evaluation changes the result)
template <int WAVES>
__device__ __forceinline__ unsigned long long block_scan_add64(unsigned long long v, unsigned long long* s_wave, unsigned long long* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  __syncthreads();  // the previous call's readers are done
  if (lane == 63) s_wave[wave] = v;
  __syncthreads();
  unsigned long long before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const unsigned long long x = s_wave[w];
    before += w < wave ? x : 0;
    all += x;
  }
  *total = all;
  return v + before;
}

// maximum over the threads strictly BEFORE this one (0 for the first: the values are >= 0); all: over all threads
template <int WAVES>
__device__ __forceinline__ int block_scan_max_excl(int v, int* s_wave, int* all) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (lane >= o) v = max(v, u);
  }
  const int prev = __shfl_up(v, 1, 64);
  __syncthreads();  // the previous call's readers are done
  if (lane == 63) s_wave[wave] = v;
  __syncthreads();
  int before = lane > 0 ? prev : 0, m = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const int x = s_wave[w];
    before = w < wave ? max(before, x) : before;
    m = max(m, x);
  }
  *all = m;
  return before;
}

// maximum over the threads strictly AFTER this one (0 for the last: the values are >= 0); all: over all threads
template <int WAVES>
__device__ __forceinline__ double block_rscan_max_excl(double v, double* s_wave, double* all) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double u = __shfl_down(v, o, 64);
    if (lane + o < 64) v = fmax(v, u);
  }
  const double next = __shfl_down(v, 1, 64);
  __syncthreads();  // the previous call's readers are done
  if (lane == 0) s_wave[wave] = v;
  __syncthreads();
  double after = lane < 63 ? next : 0.0, m = 0.0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const double x = s_wave[w];
    after = w > wave ? fmax(after, x) : after;
    m = fmax(m, x);
  }
  *all = m;
  return after;
}

}  // namespace pcmi
