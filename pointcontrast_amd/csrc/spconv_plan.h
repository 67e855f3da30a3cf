// The plan of one gathered convolution launch (spconv.hip: run_gathered): which kernel, its tile shape, the offset split and
// the workspace layout, from the launch's shape and the environment alone.  Host code only: no device memory is touched.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "internal.h"
#include "spconv_args.h"

namespace pcmi {

constexpr int kStreamKDefaultMinTiles = 256;  // unit-balanced launch from 256 tiles (32768 rows); PCMI_SPCONV_STREAMK=0 turns it off

// The switches of the convolution plans, read from the environment once per convolution call and per workspace query
// (not once per process: the parity tests compare both settings in one process) and handed to everything that plans.
//   PCMI_SPCONV_STREAMK  minimum number of 128-row tiles for the unit-balanced launch (0 = never)
//   PCMI_CONV16          the 16-row kernels take the 128-row tiles of levels with at least this many rows (0 = never,
//                        1 = always).  Default 512 since round 3: with the weights of every layer packed for its level's
//                        slice width ahead of the launches (x3_plan_nt), the split-precision kernel also wins on the
//                        coarse levels -- 240 -> 247 pairs/s at 2048, 249 at 512 (profiles/r03e_bench_ab_*.txt); round
//                        2's 8192 was measured with the fp32 form, which lost below it.
//   PCMI_CONV16_X3       the split-precision form (spconv_x3.hip: fp32 operands as three bf16 terms on the bf16 matrix
//                        cores) takes the matrix-bound launches of the 16-row kernel (>= 64 channels on both sides);
//                        0: the fp32-MFMA kernel
//   PCMI_CONV32R         minimum number of output rows for the 32 -> 32 channel kernel of spconv32r.hip (0 = never)
struct ConvEnv {
  int64_t sk_min_tiles, conv16_min_rows, conv32r_min_rows;
  bool x3_on;
};
static ConvEnv conv_env() {
  ConvEnv env;
  const char* e = getenv("PCMI_SPCONV_STREAMK");
  env.sk_min_tiles = e ? (int64_t)atoll(e) : (int64_t)kStreamKDefaultMinTiles;
  e = getenv("PCMI_CONV16");
  env.conv16_min_rows = e ? atoll(e) : 512;
  e = getenv("PCMI_CONV16_X3");
  env.x3_on = !e || atoi(e) != 0;
  e = getenv("PCMI_CONV32R");
  env.conv32r_min_rows = e ? (int64_t)atoll(e) : (int64_t)8192;
  return env;
}

// resident workgroups of the unit-balanced launch at most (4 waves per SIMD, spconv.hip: sk_workgroups), multiple of 8
static int sk_workgroups_max() { return 4 * num_cu() / 8 * 8; }
static bool sk_rows_eligible(const ConvEnv& env, int64_t rows, int K) {
  const int64_t mt = env.sk_min_tiles;
  return K > 1 && mt > 0 && rows >= 4096 /* kSortRowsMin: such maps carry tile units */ && ceil_div(rows, 128) >= mt;
}
static size_t sk_partial_bytes(const ConvEnv& env, int64_t rows, int N, int K) {
  return sk_rows_eligible(env, rows, K) ? (size_t)sk_workgroups_max() * 2 * 128 * N * sizeof(float) : 0;
}

static bool conv16_enabled(const ConvEnv& env, int64_t n_rows, int64_t x_bytes) {
  const int64_t min_rows = env.conv16_min_rows;
  // the pipelined form addresses the gathered operand with 32-bit byte offsets (absent = 2^31)
  return min_rows > 0 && n_rows >= min_rows && x_bytes <= 0x7FFFFF00ll;
}

static bool conv16_x3(const ConvEnv& env, int NT, int C, int N) { return env.x3_on && NT >= 2 && NT <= 4 && C >= 64 && N >= 64; }

// What one gathered launch will do: the ONE place that names the kernel, its tile shape, the offset split and the
// workspace layout.  run_gathered executes it, the workspace query and x3_plan_nt ask it, pcmi_spconv_plan reports it.
struct ConvPlan {
  int kernel;          // PCMI_CONV_KERNEL_* (include/pcmi.h)
  int RW, NT, ksplit;  // row tile / 32, output slice width / 32, offset ranges over blockIdx.z (spconv32r: 0, 0, 1)
  // the workspace, front to back: the partial tensors of a split launch or the partial tiles of a unit-balanced one,
  // then the packed weights of the split-precision form
  size_t split_bytes, sk_bytes, pack_offset, pack_bytes;
  size_t ws_bytes;     // what the call requires
};
constexpr int kMaxKSplit = 27;

// rows: output rows (or pairs in pair mode); x_bytes: size of the gathered operand; C: contraction size; N: output
// channels; K: offsets; form: PCMI_CONV_FORM_*.
// Row tiles stay as large as the row count allows (a tile streams its weight slice once, so small
// tiles multiply the weight traffic: measured 10-20 TFLOP/s with 32-row tiles on the 256-channel
// levels); the parallelism the small levels lack comes from splitting the offset range over
// blockIdx.z into partial sums instead.
static ConvPlan plan_conv(const ConvEnv& env, int64_t rows, int64_t x_bytes, int C, int N, int K, int form) {
  ConvPlan p = {};
  const bool pair = form == PCMI_CONV_FORM_PAIRS, table = form == PCMI_CONV_FORM_TABLE || form == PCMI_CONV_FORM_TABLE_UNITS;
  p.ksplit = 1;
  // 32 -> 32 channels: all weight slices resident in LDS, a wave per 16-row group (spconv32r.hip)
  if (conv32r_eligible(env.conv32r_min_rows, rows, x_bytes, C, N, K, table)) {
    p.kernel = PCMI_CONV_KERNEL_32R;
    return p;
  }
  // wide: the contraction has >= 64 channels (with N >= 64 the launch can take the split-precision kernel, whose slices
  // are at least 64 wide)
  const bool wide = C >= 64;
  const int nt_all = N / 32;
  p.NT = nt_all % 4 == 0 ? 4 : (nt_all % 3 == 0 ? 3 : (nt_all % 2 == 0 ? 2 : 1));
  p.RW = rows >= 96 ? 4 : (rows >= 48 ? 2 : 1);
  if (p.RW == 1 && p.NT > 2) p.NT = (nt_all % 2 == 0) ? 2 : 1;  // the cross-wave reduction lives in LDS
  // small levels: narrow output slices partition the weights (no extra weight traffic) and multiply the
  // number of resident workgroups; the re-gathered rows are L2-resident at these sizes
  const int64_t min16 = env.conv16_min_rows;
  if (rows < 2048)
    p.NT = (wide && !pair && K > 1 && N >= 64 && nt_all % 2 == 0 && env.x3_on && min16 > 0 && rows >= min16 && p.RW == 4) ? 2 : 1;
  else if (rows < 8192 && p.NT > 2)
    p.NT = (nt_all % 2 == 0) ? 2 : 1;
  if (pair) {
    p.kernel = PCMI_CONV_KERNEL_PAIR;
    return p;
  }
  if (K > 1 && rows > 0) {
    const int64_t wgs = ceil_div(rows, 32 * p.RW) * (nt_all / p.NT);
    // workgroups aimed at: 2.5 per CU (measured again under the round-3 default: 1.0 -> 240.3, 1.5 -> 247.0, 2.5 -> 249.1,
    // 4.0 -> 244.6 pairs/s, profiles/r03h_bench_ab_*.txt)
    const int64_t target = (25 * (int64_t)num_cu()) / 10;
    if (wgs < target) p.ksplit = (int)std::min<int64_t>(std::min<int64_t>(K, kMaxKSplit), ceil_div(target, wgs));
    // Round 6: the split by RESIDENCY ROUNDS, for the launches of the 16-row split-precision kernel (whose residency is
    // known: x3_workgroups).  The kernel's run time is that of its longest workgroup chain: rounds x (offsets per workgroup
    // x chunks + a fixed share), and "2.5 workgroups per CU" ignores both factors -- on the bench batch it gives the
    // stride-16 level (28 workgroups per split) ksplit 23, i.e. 4 of the 23 z-slices carry TWO offsets and every launch
    // takes 16 chunk steps where ksplit 27 takes 8; the stride-4 128-channel launches (79 tiles) ksplit 9 = 711 workgroups
    // on 512 slots, a full round and a 40 %-filled second one, where ksplit 6 is ONE round.  cost(ks), in chunk
    // steps: rounds x (ceil(K / ks) C / 32 + 3) x (a penalty under 2 workgroups per CU: nobody hides a step's latency)
    // + the partial tensors' write + read-back (8 B per element and split at ~3 TB/s against ~2 us per step).  Taken only
    // when it beats the rule above by 10 % of its own estimate, and only under 16384 rows: on the stride-2 level it picks
    // ksplit 2, which measured equal in the forward pass and 20 % SLOWER in the backward pass, beside the weight-gradient
    // stream (profiles/r06d_*: 632 workgroups of 42 steps leave nothing for the other stream to slip into).
    if (wide && p.RW == 4 && wgs < target && rows < 16384 && conv16_x3(env, p.NT, C, N) && min16 > 0 && rows >= min16) {
      const double slots = (double)x3_workgroups(p.NT, 3), nch = (double)(C / 32);  // (the fp32 mode's plan in both modes)
      const double traffic = (double)rows * N * 8.0 / 3.0e6 / 2.0;  // chunk steps per partial tensor
      auto cost = [&](int ks) {
        const double w = (double)wgs * ks;
        const double rounds = std::ceil(w / slots);
        const double thin = std::max(1.0, 2.0 * num_cu() / std::min(w, slots));
        return rounds * ((double)ceil_div((int64_t)K, (int64_t)ks) * nch + 3.0) * thin + traffic * ks;
      };
      int best = p.ksplit;
      const int kmax = (int)std::min<int64_t>(K, kMaxKSplit);
      for (int ks = 1; ks <= kmax; ++ks)
        if (cost(ks) < cost(best) - 1e-9) best = ks;
      if (cost(best) < 0.9 * cost(p.ksplit)) p.ksplit = best;
    }
  }
  const bool c16 = p.RW == 4 && conv16_enabled(env, rows, x_bytes), x3 = conv16_x3(env, p.NT, C, N);
  // (32-channel convs are HBM/latency-bound: the partial tiles cost them more than the balance gains -- measured)
  // (the unit-balanced launch exists for the 16-row kernels: an operand of >= 2 GiB, which they cannot address, takes the
  //  whole-tile launch of spconv_mfma_kernel below)
  // (Round 6 measured this launch also on the levels that split their offsets over blockIdx.z -- ksplit > 1: the stride-2 level
  //  of the bench batch, 316 tiles, neutral; the stride-4 level as well, 78 tiles cut into 3-10 pieces each, 0.5 ms per step
  //  SLOWER: profiles/r06a_wgrad_stream_cost_and_sk_mid_ab.txt.  The offset split + split_reduce_kernel stays there.)
  if (form == PCMI_CONV_FORM_TABLE_UNITS && c16 && p.ksplit == 1 && sk_rows_eligible(env, rows, K) && C >= 64 && N >= 64) {
    p.kernel = x3 ? PCMI_CONV_KERNEL_UNITS_X3 : PCMI_CONV_KERNEL_UNITS_16;
    p.sk_bytes = sk_partial_bytes(env, rows, N, K);
    p.pack_offset = p.sk_bytes;
    p.pack_bytes = x3 ? x3_pack_bytes(K, C, N) : 0;
    p.ws_bytes = p.pack_offset + p.pack_bytes;
    return p;
  }
  p.split_bytes = p.ksplit > 1 ? (size_t)p.ksplit * rows * N * sizeof(float) : 0;
  p.ws_bytes = p.split_bytes;
  if (c16 && x3 && form != PCMI_CONV_FORM_NONE) {
    p.kernel = PCMI_CONV_KERNEL_TABLE_X3;
    p.pack_offset = align_up(p.split_bytes, 256);
    p.pack_bytes = x3_pack_bytes(K, C, N);
    p.ws_bytes = p.pack_offset + p.pack_bytes;
  } else if (c16) {
    p.kernel = PCMI_CONV_KERNEL_TABLE_16;
  } else if (p.RW == 4 && p.NT <= 2 && C % 64 == 0) {
    // 128-row tiles, narrow slices (NT <= 2, levels under 8192 rows): 64-channel chunks when the contraction size allows --
    // twice the matrix work and loads in flight per barrier (NT = 1 keeps 4 waves per SIMD, NT = 2 keeps 3; 128-channel
    // chunks cost a wave per SIMD and lost).
    p.kernel = PCMI_CONV_KERNEL_DEEP;
  } else {
    p.kernel = PCMI_CONV_KERNEL_PLAIN;
  }
  return p;
}

}  // namespace pcmi
