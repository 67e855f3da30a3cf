// hipcub's exclusive sum behind one size rule: every workspace formula and every call site asks here, for the type it scans.
// (Apart from rowscan.h, whose includers do not pay for <hipcub/hipcub.hpp>.)
#pragma once
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "common.h"

namespace pcmi {

// temporary bytes of cub_scan_excl over `items` values of T, a multiple of 256: what Carve::take hands out for them
template <class T>
static inline size_t cub_scan_bytes(int64_t items) {
  size_t b = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (const T*)nullptr, (T*)nullptr, (int)std::max<int64_t>(items, 1));
  return align_up(b, 256);
}

// out [items] = the exclusive sum of in [items] (items < 2^31), in order
template <class T>
static inline int cub_scan_excl(void* temp, size_t temp_bytes, const T* in, T* out, int64_t items, hipStream_t st) {
  PCMI_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, in, out, (int)items, st));
  return PCMI_OK;
}

}  // namespace pcmi
