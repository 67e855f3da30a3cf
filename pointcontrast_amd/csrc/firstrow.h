// "Keep the lowest row of every key, number those rows by an exclusive scan, report how many fall into each segment": the
// idiom of the loader, the pair corpus, the pair input, the segmentation input and the instance input, above cellgrid.h's
// tables.  first [slots] is uint32, empty = 0xffffffff (hipMemsetAsync 0xff); rows are below 2^31 in every caller.
#pragma once
#include <algorithm>

#include "cellgrid.h"

namespace pcmi {

constexpr uint32_t kNoSlot = 0xffffffffu;  // slot_of[i] of a row that has no key

// slots of an unsegmented table over n keys: the power of two that is at least max(1024, 2 n)
static inline int64_t table_cap(int64_t n) {
  int64_t c = 1024;
  while (c < 2 * n) c <<= 1;
  return c;
}

// claim_slot, and first[slot] = the lowest row that claimed it; returns the slot
__device__ inline uint32_t claim_first(uint64_t* keys, uint32_t base, uint32_t size, uint64_t key, uint32_t* first, int64_t row) {
  const uint32_t slot = claim_slot(keys, base, size, key);
  atomicMin(&first[slot], (uint32_t)row);
  return slot;
}
__device__ inline bool is_first_row(uint32_t slot, const uint32_t* __restrict__ first, int64_t i) {
  return slot != kNoSlot && first[slot] == (uint32_t)i;
}

// rows [lo, hi) of segment b, clipped to [0, n] (offs ascending; a segment may be empty): offsets arrive from the device
// unchecked, and whoever indexes with lo and hi stays inside n + 1 items
__device__ inline void segment_rows(const int64_t* __restrict__ offs, int b, int64_t n, int64_t& lo, int64_t& hi) {
  lo = std::min<int64_t>(std::max<int64_t>(offs[b], 0), n);
  hi = std::min<int64_t>(std::max<int64_t>(offs[b + 1], lo), n);
}
// thread t <= B: counts[t] = pos[hi_t] - pos[lo_t], counts[B] = pos[n]; pos is the exclusive scan over n + 1 flags of which
// the last, and those of rows outside every segment, are 0
__device__ inline void segment_counts(int64_t t, const int64_t* __restrict__ offs, int B, int64_t n, const int32_t* __restrict__ pos,
                                      int64_t* __restrict__ counts) {
  if (t > B) return;
  if (t == B) {
    counts[B] = pos[n];
  } else {
    int64_t lo, hi;
    segment_rows(offs, (int)t, n, lo, hi);
    counts[t] = pos[hi] - pos[lo];
  }
}

}  // namespace pcmi
