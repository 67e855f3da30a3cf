// Exclusive scan of int32 values v [m] -> out [m] (out may be v) and their sum, in row order, for any m: three launches --
// the sums of kScanBlock values per workgroup, their scan by ONE workgroup (which walks them kThreads at a time, so the
// second level starts at kThreads kScanBlock values), the scan inside each workgroup.  The numbering pass of
// pcmi_components_compact (cluster.hip) and of the instance input (insseg_input.hip).  Integer sums: no order changes a result.
#pragma once
#include <algorithm>

#include "blockscan.h"
#include "common.h"

namespace pcmi {
namespace rowscan {

constexpr int kThreads = 256;  // 4 waves: one per SIMD of a CU
constexpr int kWaves = kThreads / 64;
constexpr int kScanItems = 8, kScanBlock = kThreads * kScanItems;  // values per thread / per workgroup of the scans

static __global__ __launch_bounds__(kThreads) void scan_sums_kernel(const int32_t* __restrict__ v, int64_t m, int32_t* __restrict__ block_sums) {
  __shared__ int s_wave[kWaves];
  const int64_t i0 = (int64_t)blockIdx.x * kScanBlock + (int64_t)threadIdx.x * kScanItems;
  int c = 0;
#pragma unroll
  for (int e = 0; e < kScanItems; ++e) c += i0 + e < m ? v[i0 + e] : 0;
  int tot;
  (void)block_scan_add<kWaves>(c, s_wave, &tot);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = tot;
}

// one workgroup: block_offs = the exclusive scan of block_sums [n_blocks], *total = their sum
static __global__ __launch_bounds__(kThreads) void scan_blocks_kernel(const int32_t* __restrict__ block_sums, int n_blocks,
                                                                      int32_t* __restrict__ block_offs, int32_t* __restrict__ total) {
  __shared__ int s_wave[kWaves];
  __shared__ int s_carry;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (int b0 = 0; b0 < n_blocks; b0 += kThreads) {
    const int b = b0 + (int)threadIdx.x;
    const int v = b < n_blocks ? block_sums[b] : 0;
    int tot;
    const int ex = block_scan_add<kWaves>(v, s_wave, &tot) - v;
    const int carry = s_carry;
    if (b < n_blocks) block_offs[b] = carry + ex;
    __syncthreads();
    if (threadIdx.x == 0) s_carry = carry + tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = s_carry;
}

static __global__ __launch_bounds__(kThreads) void scan_apply_kernel(const int32_t* v, int64_t m, const int32_t* __restrict__ block_offs, int32_t* out) {
  __shared__ int s_wave[kWaves];
  const int64_t i0 = (int64_t)blockIdx.x * kScanBlock + (int64_t)threadIdx.x * kScanItems;
  int x[kScanItems], c = 0;
#pragma unroll
  for (int e = 0; e < kScanItems; ++e) {
    x[e] = i0 + e < m ? v[i0 + e] : 0;
    c += x[e];
  }
  int tot;
  int pos = block_offs[blockIdx.x] + block_scan_add<kWaves>(c, s_wave, &tot) - c;
#pragma unroll
  for (int e = 0; e < kScanItems; ++e) {
    if (i0 + e < m) out[i0 + e] = pos;
    pos += x[e];
  }
}

static inline int64_t scan_blocks(int64_t m) { return ceil_div(std::max<int64_t>(m, 1), kScanBlock); }

// block_sums / block_offs: scan_blocks(m) int32 each; total: device int32 [1]
static inline int scan_excl(const int32_t* v, int64_t m, int32_t* out, int32_t* block_sums, int32_t* block_offs, int32_t* total, hipStream_t st) {
  const int64_t nb = scan_blocks(m);
  scan_sums_kernel<<<(unsigned)nb, kThreads, 0, st>>>(v, m, block_sums);
  PCMI_LAUNCH_CHECK();
  scan_blocks_kernel<<<1, kThreads, 0, st>>>(block_sums, (int)nb, block_offs, total);
  PCMI_LAUNCH_CHECK();
  scan_apply_kernel<<<(unsigned)nb, kThreads, 0, st>>>(v, m, block_offs, out);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

}  // namespace rowscan
}  // namespace pcmi
