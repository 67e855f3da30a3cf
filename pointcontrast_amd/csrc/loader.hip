// Loader-side geometry on the device: the two steps that sit immediately before the hot path in
// the reference's dataset item and dominate its wall clock there --
//   * ME.utils.sparse_quantize(xyz / voxel, return_index=True)     (pc/lib/ddp_data_loaders.py:228-229)
//       -> ascending indices of the FIRST point of every occupied voxel;
//   * get_matching_indices(pcd0, pcd1, trans, 1.5 * voxel)          (pc/lib/ddp_data_loaders.py:36-49, :241)
//       -> all (i, j) with |T p_i - q_j| <= r; the reference walks an open3d KD-tree point by point in Python
//          (~20k radius queries per item), here: a hash grid of r-sized cells over the targets + a 27-cell probe per
//          source point.  Pairs leave sorted by (i, j) -- the order the trainer relies on (sorted by column 0).
// Both are integer / exactly-rounded fp64 work and bit-exact against oracle/loader_ref.py: every product and sum is an
// explicit round-to-nearest operation in a fixed order (no FMA contraction), divisions are IEEE.
#include <algorithm>

#include "common.h"
#include "cubscan.h"
#include "exact.h"
#include "firstrow.h"
#include "internal.h"

#pragma clang fp contract(off)

namespace pcmi {

// ---- voxelisation ----------------------------------------------------------------------------------------------
// A point that is not finite or falls outside +-2^20 voxels has no voxel (cells_of): PCMI_ERR_RANGE.
__global__ void vox_insert_kernel(const double* __restrict__ xyz, int64_t n, double voxel, uint64_t* keys, uint32_t* first,
                                  uint32_t cap, uint32_t* slot_of, int32_t* err) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int64_t c[3];
  if (!cells_of(xyz + 3 * i, voxel, c)) {
    atomicAdd(err, 1);
    slot_of[i] = kNoSlot;
    return;
  }
  slot_of[i] = claim_first(keys, 0, cap, cell_key(c[0], c[1], c[2]), first, i);  // first occurrence = smallest point index of the voxel
}
__global__ void vox_flag_kernel(int64_t n, const uint32_t* __restrict__ first, const uint32_t* __restrict__ slot_of,
                                int32_t* __restrict__ flags) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) flags[i] = is_first_row(slot_of[i], first, i) ? 1 : 0;
}
__global__ void vox_compact_kernel(const double* __restrict__ xyz, int64_t n, double voxel, const int32_t* __restrict__ flags,
                                   const int32_t* __restrict__ pos, int32_t* __restrict__ first_idx, int32_t* __restrict__ coords) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !flags[i]) return;
  const int32_t p = pos[i];
  first_idx[p] = (int32_t)i;
  if (coords) {
    coords[3 * p] = (int32_t)floor(xyz[3 * i] / voxel);
    coords[3 * p + 1] = (int32_t)floor(xyz[3 * i + 1] / voxel);
    coords[3 * p + 2] = (int32_t)floor(xyz[3 * i + 2] / voxel);
  }
}

// ---- radius matching -------------------------------------------------------------------------------------------
struct Rigid {  // row-major 3x4: p' = R p + t (rigid_apply)
  double m[12];
};

__global__ void grid_insert_kernel(const double* __restrict__ dst, int64_t n1, double radius, uint64_t* keys, int32_t* head,
                                   uint32_t cap, int32_t* __restrict__ next, int32_t* err) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n1) return;
  int64_t c[3];
  if (!cells_of(dst + 3 * j, radius, c)) {
    atomicAdd(err, 1);
    next[j] = -1;
    return;
  }
  const uint32_t slot = claim_slot(keys, 0, cap, cell_key(c[0], c[1], c[2]));
  next[j] = atomicExch(&head[slot], (int32_t)j);  // list order is arbitrary: the matches are sorted per source point
}

// FILL = false: count[i] = number of targets within the radius; FILL = true: pairs[offs[i] ..] = (i, j), j ascending
template <bool FILL>
__global__ void match_kernel(const double* __restrict__ src, int64_t n0, Rigid T, const double* __restrict__ dst, int64_t n1, double radius,
                             const uint64_t* __restrict__ keys, const int32_t* __restrict__ head, uint32_t cap,
                             const int32_t* __restrict__ next, int64_t* __restrict__ count, const int64_t* __restrict__ offs,
                             int32_t* __restrict__ pairs, int32_t* err) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n0) return;
  const double p[3] = {src[3 * i], src[3 * i + 1], src[3 * i + 2]};
  double q[3];
  rigid_apply(T.m, 4, p, q);
  if (!finite3(q[0], q[1], q[2])) {  // a non-finite source point, or one the transform made non-finite
    if (!FILL) {
      atomicAdd(err, 1);
      count[i] = 0;
    }
    return;
  }
  // (a source outside the grid's range meets only the cells cell_ok admits: no error, the oracle has no range either)
  const int64_t cell[3] = {(int64_t)floor(q[0] / radius), (int64_t)floor(q[1] / radius), (int64_t)floor(q[2] / radius)};
  int32_t found[FILL ? kMaxMatches : 1];
  int nf = radius_probe(dst, n1, q, cell, radius, keys, head, next, 0, cap, FILL ? found : nullptr);
  if (nf > kMaxMatches) atomicAdd(err, 1);
  if (!FILL) {
    count[i] = nf;
    return;
  }
  nf = min(nf, kMaxMatches);
  for (int a = 1; a < nf; ++a) {  // insertion sort, nf is small
    const int32_t v = found[a];
    int b = a - 1;
    while (b >= 0 && found[b] > v) {
      found[b + 1] = found[b];
      --b;
    }
    found[b + 1] = v;
  }
  int32_t* out = pairs + 2 * offs[i];
  for (int a = 0; a < nf; ++a) {
    out[2 * a] = (int32_t)i;
    out[2 * a + 1] = found[a];
  }
}

}  // namespace pcmi

using namespace pcmi;

extern "C" {

// The two queries of this file are bounds, not sums of padded pieces: measuring (null base) packs the pieces, piece
// alignment 1, and adds kPadSlack, which covers the 256-byte padding of the at most eight pieces the entry carves.
constexpr size_t kPadSlack = 7 * 256 + 1024;

struct VoxWs { uint64_t* keys; uint32_t *first, *slot_of; int32_t *flags, *pos, *err; void* temp; size_t temp_bytes, bytes; };
static VoxWs vox_ws(void* ws, int64_t n) {
  const uint32_t cap = (uint32_t)table_cap(n);
  Carve cv{(char*)ws, ws ? (size_t)256 : (size_t)1};
  VoxWs w;
  w.keys = cv.take<uint64_t>(cap);
  w.first = cv.take<uint32_t>(cap);
  w.slot_of = cv.take<uint32_t>((size_t)n);
  w.flags = cv.take<int32_t>((size_t)n);
  w.pos = cv.take<int32_t>((size_t)n);
  w.err = cv.take<int32_t>(64);
  w.temp_bytes = cub_scan_bytes<int32_t>(n);
  w.temp = cv.take<char>(w.temp_bytes);
  cv.take<int64_t>(2 * (size_t)n);  // (unused: 16 n bytes the query has counted since it was written)
  w.bytes = cv.used + kPadSlack;
  return w;
}

size_t pcmi_voxelize_workspace_bytes(int64_t n) { return vox_ws(nullptr, n).bytes; }

int pcmi_voxelize(const double* xyz, int64_t n, double voxel_size, int32_t* first_index, int32_t* coords,
                  int64_t* n_unique_host, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_REQUIRE(n_unique_host && (n == 0 || (xyz && first_index)) && voxel_size > 0 && n >= 0 && n < (1ll << 31), PCMI_ERR_INVALID,
               "voxelize: bad argument");
  *n_unique_host = 0;
  if (n == 0) return PCMI_OK;
  hipStream_t st = as_stream(stream);
  if (int rc = require_ws("voxelize", ws, ws_bytes, vox_ws(nullptr, n).bytes, 1)) return rc;
  const uint32_t cap = (uint32_t)table_cap(n);
  const VoxWs w = vox_ws(ws, n);
  PCMI_HIP_CHECK(hipMemsetAsync(w.keys, 0xff, (size_t)cap * 8, st));
  PCMI_HIP_CHECK(hipMemsetAsync(w.first, 0xff, (size_t)cap * 4, st));
  PCMI_HIP_CHECK(hipMemsetAsync(w.err, 0, 256, st));
  const unsigned gn = (unsigned)ceil_div(n, 256);
  vox_insert_kernel<<<gn, 256, 0, st>>>(xyz, n, voxel_size, w.keys, w.first, cap, w.slot_of, w.err);
  PCMI_LAUNCH_CHECK();
  vox_flag_kernel<<<gn, 256, 0, st>>>(n, w.first, w.slot_of, w.flags);
  PCMI_LAUNCH_CHECK();
  if (int rc = cub_scan_excl(w.temp, w.temp_bytes, w.flags, w.pos, n, st)) return rc;
  int32_t host[3] = {0, 0, 0};  // last flag, last pos, error count
  PCMI_HIP_CHECK(hipMemcpyAsync(&host[0], w.flags + n - 1, 4, hipMemcpyDeviceToHost, st));
  PCMI_HIP_CHECK(hipMemcpyAsync(&host[1], w.pos + n - 1, 4, hipMemcpyDeviceToHost, st));
  PCMI_HIP_CHECK(hipMemcpyAsync(&host[2], w.err, 4, hipMemcpyDeviceToHost, st));
  PCMI_HIP_CHECK(hipStreamSynchronize(st));
  PCMI_REQUIRE(host[2] == 0, PCMI_ERR_RANGE, "voxelize: %d points are not finite or fall outside +-2^20 voxels", host[2]);
  *n_unique_host = (int64_t)host[0] + host[1];
  vox_compact_kernel<<<gn, 256, 0, st>>>(xyz, n, voxel_size, w.flags, w.pos, first_index, coords);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

struct MatchWs { uint64_t* keys; int32_t *head, *next; int64_t *count, *offs; int32_t* err; void* temp; size_t temp_bytes, bytes; };
static MatchWs match_ws(void* ws, int64_t n0, int64_t n1) {
  const uint32_t cap = (uint32_t)table_cap(n1);
  Carve cv{(char*)ws, ws ? (size_t)256 : (size_t)1};
  MatchWs w;
  w.keys = cv.take<uint64_t>(cap);
  w.head = cv.take<int32_t>(cap);
  w.next = cv.take<int32_t>((size_t)n1);
  w.count = cv.take<int64_t>((size_t)n0);
  w.offs = cv.take<int64_t>((size_t)n0);
  w.err = cv.take<int32_t>(64);
  w.temp_bytes = cub_scan_bytes<int64_t>(n0);
  w.temp = cv.take<char>(w.temp_bytes);
  w.bytes = cv.used + kPadSlack;
  return w;
}

size_t pcmi_match_radius_workspace_bytes(int64_t n0, int64_t n1) { return match_ws(nullptr, n0, n1).bytes; }

int pcmi_match_radius(const double* src, int64_t n0, const double* rigid3x4_host, const double* dst, int64_t n1, double radius,
                      int32_t* pairs, int64_t pairs_capacity, int64_t* n_pairs_host, void* ws, size_t ws_bytes,
                      pcmi_stream_t stream) {
  PCMI_REQUIRE(n_pairs_host && rigid3x4_host && radius > 0 && n0 >= 0 && n1 >= 0 && n0 < (1ll << 31) && n1 < (1ll << 31) &&
                   (n0 == 0 || src) && (n1 == 0 || dst), PCMI_ERR_INVALID, "match_radius: bad argument");
  *n_pairs_host = 0;
  if (n0 == 0 || n1 == 0) return PCMI_OK;
  hipStream_t st = as_stream(stream);
  if (int rc = require_ws("match_radius", ws, ws_bytes, match_ws(nullptr, n0, n1).bytes, 1)) return rc;
  const uint32_t cap = (uint32_t)table_cap(n1);
  const MatchWs w = match_ws(ws, n0, n1);
  Rigid T;
  for (int q = 0; q < 12; ++q) T.m[q] = rigid3x4_host[q];
  PCMI_HIP_CHECK(hipMemsetAsync(w.keys, 0xff, (size_t)cap * 8, st));
  PCMI_HIP_CHECK(hipMemsetAsync(w.head, 0xff, (size_t)cap * 4, st));  // -1
  PCMI_HIP_CHECK(hipMemsetAsync(w.err, 0, 256, st));
  const unsigned g0 = (unsigned)ceil_div(n0, 128), g1 = (unsigned)ceil_div(n1, 256);
  grid_insert_kernel<<<g1, 256, 0, st>>>(dst, n1, radius, w.keys, w.head, cap, w.next, w.err);
  PCMI_LAUNCH_CHECK();
  match_kernel<false><<<g0, 128, 0, st>>>(src, n0, T, dst, n1, radius, w.keys, w.head, cap, w.next, w.count, nullptr, nullptr, w.err);
  PCMI_LAUNCH_CHECK();
  if (int rc = cub_scan_excl(w.temp, w.temp_bytes, w.count, w.offs, n0, st)) return rc;
  int64_t last[2] = {0, 0};
  int32_t herr = 0;
  PCMI_HIP_CHECK(hipMemcpyAsync(&last[0], w.count + n0 - 1, 8, hipMemcpyDeviceToHost, st));
  PCMI_HIP_CHECK(hipMemcpyAsync(&last[1], w.offs + n0 - 1, 8, hipMemcpyDeviceToHost, st));
  PCMI_HIP_CHECK(hipMemcpyAsync(&herr, w.err, 4, hipMemcpyDeviceToHost, st));
  PCMI_HIP_CHECK(hipStreamSynchronize(st));
  PCMI_REQUIRE(herr == 0, PCMI_ERR_RANGE,
               "match_radius: %d points not finite, outside +-2^20 cells or with more than %d matches (is the radius far above the voxel size?)",
               herr, kMaxMatches);
  *n_pairs_host = last[0] + last[1];
  if (!pairs || *n_pairs_host == 0) return PCMI_OK;  // count-only call
  PCMI_REQUIRE(pairs_capacity >= *n_pairs_host, PCMI_ERR_WORKSPACE, "match_radius: %lld pairs but room for %lld",
               (long long)*n_pairs_host, (long long)pairs_capacity);
  match_kernel<true><<<g0, 128, 0, st>>>(src, n0, T, dst, n1, radius, w.keys, w.head, cap, w.next, nullptr, w.offs, pairs, w.err);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

}  // extern "C"
