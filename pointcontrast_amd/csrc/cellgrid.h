// Hash grids of cells over points, as the loader, the pair input, the pair corpus, the segmentation input and the nearest-point
// search build them: the key of a cell, the open-addressing table that maps a key to a slot, the segment of a row in a batch
// of clouds, and the 27-cell radius probe over per-cell lists.
#pragma once
#include "common.h"
#include "exact.h"

namespace pcmi {

constexpr int kCellBias = 1 << 20;  // |cell index| < 2^20 per axis
constexpr int kMaxMatches = 96;     // per source point of a radius probe (r = 1.5 voxels, one target per voxel: <= ~30)

__device__ inline uint64_t cell_key(int64_t x, int64_t y, int64_t z) {
  return ((uint64_t)(x + kCellBias) << 42) | ((uint64_t)(y + kCellBias) << 21) | (uint64_t)(z + kCellBias);
}
__device__ inline bool cell_ok(int64_t x, int64_t y, int64_t z) {
  return x > -kCellBias && x < kCellBias && y > -kCellBias && y < kCellBias && z > -kCellBias && z < kCellBias;
}
// floor(v / cell) per axis as integers inside +-(2^20 - 1); false (nothing converted) for anything else, a NaN or an
// infinity included: floor -> integer is defined only for what passes
__device__ inline bool cells_of(const double* p, double cell, int64_t* out) {
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double f = floor(p[a] / cell);
    ok = ok && fabs(f) < (double)kCellBias;
    out[a] = ok ? (int64_t)f : 0;
  }
  return ok;
}

// ---- key -> slot: open addressing, linear probing, in the table segment [base, base + size) of `keys` -----------------------
// A probe starts at hash_key(key) % size; for a power-of-two size (the test is wave-uniform) that is the mask.
__device__ inline uint32_t slot_start(uint64_t key, uint32_t size) {
  const uint32_t h = hash_key(key);
  return (size & (size - 1)) == 0 ? (h & (size - 1)) : h % size;
}
// the slot of `key`, claimed if absent.  Ends: every caller sizes a segment to at least twice its keys
__device__ inline uint32_t claim_slot(uint64_t* keys, uint32_t base, uint32_t size, uint64_t key) {
  uint32_t s = slot_start(key, size);
  while (true) {
    const unsigned long long prev = atomicCAS((unsigned long long*)&keys[base + s], (unsigned long long)kEmptyKey, (unsigned long long)key);
    if (prev == kEmptyKey || prev == key) return base + s;
    if (++s == size) s = 0;
  }
}
// the slot of `key`, -1 if it has none (a segment always has an empty slot; the bound is for a table that is not one)
__device__ inline int64_t find_slot(const uint64_t* __restrict__ keys, uint32_t base, uint32_t size, uint64_t key) {
  uint32_t s = slot_start(key, size);
  for (uint32_t step = 0; step < size; ++step) {
    const uint64_t k = keys[base + s];
    if (k == key) return (int64_t)base + s;
    if (k == kEmptyKey) return -1;
    if (++s == size) s = 0;
  }
  return -1;
}

// the segment of row i: offs[b] <= i < offs[b + 1] (offs [B + 1] ascending, empty segments allowed); -1 if there is none
__device__ inline int segment_of(const int64_t* __restrict__ offs, int B, int64_t i) {
  int lo = 0, hi = B + 1;  // first position with offs[pos] > i
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (offs[mid] <= i) lo = mid + 1; else hi = mid;
  }
  return (lo == 0 || lo == B + 1) ? -1 : lo - 1;
}

// The rows j < m_max of `pts` with dist2_rn(q, pts_j) <= r r among the lists (head[slot], next[j]) of the 27 cells around
// `cell`, in `found` (the first kMaxMatches of them, in list order) if given; returns their number.
__device__ inline int radius_probe(const double* __restrict__ pts, int64_t m_max, const double* q, const int64_t* cell, double r,
                                   const uint64_t* __restrict__ keys, const int32_t* __restrict__ head, const int32_t* __restrict__ next,
                                   uint32_t base, uint32_t size, int32_t* found) {
  const double r2 = mul_rn(r, r);
  int nf = 0;
  for (int dz = -1; dz <= 1; ++dz)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        if (!cell_ok(cell[0] + dx, cell[1] + dy, cell[2] + dz)) continue;
        const int64_t slot = find_slot(keys, base, size, cell_key(cell[0] + dx, cell[1] + dy, cell[2] + dz));
        if (slot < 0) continue;
        int64_t steps = 0;  // (a list is acyclic and inside the rows; the bounds are for a workspace that holds no lists)
        for (int32_t j = head[slot]; j >= 0 && j < m_max && steps < m_max; j = next[j], ++steps) {
          if (dist2_rn(q, pts + 3 * (int64_t)j) <= r2) {
            if (found && nf < kMaxMatches) found[nf] = j;
            ++nf;
          }
        }
      }
  return nf;
}

}  // namespace pcmi
