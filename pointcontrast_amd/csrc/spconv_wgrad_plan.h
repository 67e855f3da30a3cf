// The plan of one weight-gradient call (spconv_wgrad.hip: spconv_backward_weight_m32): which kernel family, its tile
// shape, how the pairs or rows are cut into workgroups, how their partial sums become gW, and the workspace layout, from
// the call's shape and the environment alone.  Host code only: no device memory is touched, and the answer is the same
// with and without a device (what the HIP runtime has to say -- the residency of a pair-list variant -- is an input).
#pragma once
#include <algorithm>
#include <cstdlib>

#include "internal.h"

namespace pcmi {

// The switches of the weight-gradient plans, read from the environment once per pcmi_spconv_bwd_weight call, per
// wgrad_group_add and per workspace query (not once per process: the parity tests compare both settings in one process).
//   PCMI_WGRAD_X3T        minimum number of rows for the tile-stationary split-precision kernels of spconv_wgrad_x3.hip
//                         (0 = never; 1 = every size).  Measured on the bench batch, ms per launch stand-alone, pair-list
//                         fp32 kernel -> tile-stationary one (profiles/r03b_kbench_*):
//                           40k rows   96->96 0.205 -> 0.139, 128->96 0.253 -> 0.223
//                           175k rows  96->96 0.509 -> 0.514, 128->96 0.732 -> 0.901   (both kernels are bound by the
//                                      gathered-row traffic there: 2.3 GB at 4.4 TB/s against 1.8 GB at 3.4 TB/s; the
//                                      tile-stationary one re-stages the G tile once per offset group)
//                           9.9k rows  64->64 0.026 -> 0.048, 128->128 0.073 -> 0.098, 192->128 0.160 -> 0.121
//                         and in the training step, where it shares the chip with the backward chain
//                         (profiles/r03i_bench_ab_x3t_window.txt, 3 processes each): rows in [16384, 100000] 248.7-250.3
//                         pairs/s, >= 8192 251.4-252.5, >= 16384 **252.0-252.9** -- at 175k rows it is no faster alone but
//                         asks a quarter less of the memory system, which the chain's kernels get.  Round 4, with the
//                         producer / consumer form (profiles/r04n_*, 2 processes each): >= 100000 rows 256.0, >= 16384
//                         257.9, >= 8192 **258.5**, >= 2048 255.7 pairs/s.
//   PCMI_WGRAD_X3T_DENSE  0: the 1x1 convolutions (no map: K = 1, identity table) stay on the pair-list kernel (A/B).
//                         (Round 5: the level-1 128 -> 96 downsample gradient took 350 us in the step on the fp32 pair-list
//                         kernel, 12 TFLOP/s.)
//   PCMI_WGRAD_X3P        1 = the producer / consumer form (wgrad_x3p_kernel: 8 waves, one workgroup per CU; default),
//                         0 = one role (wgrad_x3t_kernel)
//   PCMI_WGRAD_GROUP      0: every layer its own launch instead of wgrad_mfma_group_kernel (round 4's form; A/B)
//   PCMI_WGRAD_BUF        0: always the 64-bit-address form of the pair-list kernel (A/B, parity of the two)
struct WgradEnv {
  int64_t x3t_min_rows;
  bool x3t_dense, x3p, group, buf;
};
static WgradEnv wgrad_env() {
  auto not_zero = [](const char* name) {
    const char* e = getenv(name);
    return !(e && e[0] == '0');
  };
  WgradEnv env;
  const char* e = getenv("PCMI_WGRAD_X3T");
  env.x3t_min_rows = e ? (int64_t)atoll(e) : (int64_t)8192;
  env.x3t_dense = not_zero("PCMI_WGRAD_X3T_DENSE");
  e = getenv("PCMI_WGRAD_X3P");
  env.x3p = e ? atoi(e) != 0 : true;
  env.group = not_zero("PCMI_WGRAD_GROUP");
  env.buf = not_zero("PCMI_WGRAD_BUF");
  return env;
}

// What a plan may depend on, and nothing else.
struct WgradShape {
  int64_t n_in, n_out;  // rows of the call's `in` and `gout`
  int cin, cout, K;
  bool has_map;                 // false: the dense 1x1 form (K = 1, identity pairs)
  int kernel_size, stride;      // of the map
  bool has_nbr, has_perm;       // the map carries the neighbour table / the sorted order (perm + nbr_perm)
  bool transpose, gbias, accumulate;
  int64_t x_bytes, g_bytes;     // rows x leading dimension x 4 of the two operands
  bool aligned;                 // both operands start 16-byte aligned with ld % 4 == 0
  int64_t M;                    // pairs as far as the host knows (kmap_pairs_bound; the rows without a map)
  const int64_t* counts;        // host prefix [K + 1] of the per-offset pair counts once the map has them, else null
  int terms;                    // the calling thread's conv_terms()
  int slots_per_cu;             // resident workgroups per CU of the pair-list variant wgrad_pair_tiles() names
};

enum { kSlabs = PCMI_WGRAD_MODE_SLABS, kDirect = PCMI_WGRAD_MODE_DIRECT, kArrive = PCMI_WGRAD_MODE_ARRIVE };

// What one call will do: the ONE place that names the kernel family, its tile shape, the launch sizes and the workspace
// layout.  spconv_backward_weight_m32 executes it, wgrad_group_add and spconv_wgrad_workspace ask it,
// pcmi_spconv_wgrad_plan reports it.
struct WgradPlan {
  int kernel;          // PCMI_WGRAD_KERNEL_* (include/pcmi.h)
  int tile_c, tile_n;  // pair-list: 32-channel tiles per workgroup and axis (CT, NT); tile-stationary: 16-wide tiles per
                       // wave and axis (MTW, NTW); the stems: 0
  int grid_y, grid_z;  // workgroups along cin and cout
  // pair-list launches (wgrad_mfma_kernel, stem_wgrad_kernel)
  int chunk;           // pairs per workgroup
  int mpk;             // maps: chunk slots per offset (WgradArgs::mpk); 0 without a map
  int64_t nchunks;     // chunk slots = workgroups along x
  int mode;            // kSlabs / kDirect / kArrive (WgradArgs::mode)
  bool buf;            // 32-bit byte offsets (both operands < 2 GiB), else the 64-bit-address form
  int reduce_lanes;    // kSlabs: the wgrad_reduce_kernel instantiation that follows (8 or 1)
  size_t counters;     // kArrive: arrival counters, one per (offset, tile-y, tile-z)
  // tile-stationary launches (wgrad_x3p_kernel, wgrad_x3t_kernel)
  int RB, NG, tiles_per_rb;  // row blocks, offset groups, 64-row tiles per row block
  int terms;                 // bf16 terms per operand element (WgradShape::terms)
  bool sorted_order;         // the rows are walked in the map's sorted order (perm + nbr_perm)
  int stem_wgs;        // stem_wgrad_mfma_kernel: workgroups (= slabs)
  // the workspace, front to back: the slabs, then (256-byte aligned) the partial column sums of gbias
  size_t slab_bytes, colsum_offset, colsum_bytes;
  size_t ws_bytes;     // the smallest workspace the call accepts
  bool groupable;      // wgrad_group_add takes the layer (given room in the group and its tile shape) ...
  int group_chunk;     // ... with this chunk: every offset ONE chunk
};

constexpr int64_t kWgradBufMaxBytes = 0x7FFFFF00ll;  // the largest operand 32-bit byte offsets address (absent = 2^31)
constexpr int kWgradTKG = 4;       // tile-stationary: offsets whose accumulators a workgroup holds
constexpr int kWgradTMaxRB = 128;  // tile-stationary: most row blocks (= slabs per offset)
constexpr int kWgradTMaxPerCu = 2;  // tile-stationary: resident workgroups per CU of the one-role form (the other has one)
constexpr int kStemSlabs = 512;    // workgroups (= slabs) of stem_wgrad_mfma_kernel: two per CU
constexpr int kColsumBlocks = 1024;  // most row blocks (= partial sums per column) of colsum_partial_kernel
constexpr int kArriveMax = 8;      // most chunks per offset the in-kernel (last-arriver) reduction takes
constexpr int kStemSlotsPerCu = 8;  // stem_wgrad_kernel: resident workgroups per CU
// Pairs per workgroup.  Every chunk costs the same, so the launch runs in ceil(workgroups / resident slots) rounds of
// equal length, and a round lasts as long as the wave with the most 64-pair groups: ceil(chunk / 256) groups.  Pick
// the chunk with the smallest rounds x groups (ties: the larger chunk, fewer slabs).  Per-wave cycle accounting
// (scripts/wgrad_prof.py) of the rule this replaces -- "the largest chunk that fills >= 92 % of a whole number of
// rounds" -- on the level-1 96->96 gradient: 3200 pairs = 12.5 groups per wave, i.e. half the waves of every workgroup
// waited one whole group (8 % of the loop) at the reduction barrier, and 480 workgroups on 512 slots.
constexpr int kWgradMinChunk = 256, kWgradMaxChunks = 4096;
constexpr int kWgradChunkStep = 128;  // a chunk is a multiple of 128 pairs (WgradArgs::chunk)
// Longest chunk (pairs).  A workgroup of the level-1 gradients runs ~80 us per 1024 pairs and is never pre-empted: while
// it holds its CU, the latency-critical kernels of the bwd-data chain (higher stream priority, but priority only orders
// the DISPATCH of new workgroups) wait for a slot.
constexpr int kWgradMaxChunk = 4096;

static int wgrad_pair_tiles(int c) {  // pair-list: tiles (of 32 channels) a workgroup covers per axis
  const int tiles32 = c / 32;
  return tiles32 % 3 == 0 ? 3 : (tiles32 % 2 == 0 ? 2 : 1);
}
static int wgrad_x3t_tw(int c) { return c % 96 == 0 ? 3 : (c % 64 == 0 ? 2 : 0); }  // 16-wide tiles per wave and axis

static int wgrad_min_chunk(int64_t M) {
  return (int)std::max<int64_t>(kWgradMinChunk, align_up((size_t)ceil_div(M, kWgradMaxChunks), kWgradChunkStep));
}
// Pairs one offset of a map can have at most: a row takes part in at most one pair per offset on either side.
static int64_t wgrad_offset_bound(int64_t n_in, int64_t n_out) { return std::min(n_in, n_out); }
// Slab slots of a launch: K * ceil(offset bound / chunk) for a map (WgradArgs::mpk), ceil(M / chunk) for the dense case;
// the smallest chunk a launch may pick keeps them under ~4096 + K.
static int wgrad_lo_chunk(int64_t n_in, int64_t n_out, int K, int64_t M) {
  return K > 1 ? wgrad_min_chunk(wgrad_offset_bound(n_in, n_out) * K) : wgrad_min_chunk(M);
}

// Pairs of offset k as far as the host knows (only steers the chunk size): exact once the map's counts have arrived,
// otherwise the typical occupancy of a surface (17 of 27 neighbours) / an even split of the fine rows over the 8 children.
static int64_t wgrad_offset_len(const WgradShape& s, int k) {
  if (s.counts) return s.counts[k + 1] - s.counts[k];
  const int64_t map_in = s.transpose ? s.n_out : s.n_in, map_out = s.transpose ? s.n_in : s.n_out;
  return s.stride == 1 ? map_out * 17 / 27 : ceil_div(map_in, s.K);
}
static int64_t wgrad_num_chunks(const WgradShape& s, int chunk) {
  if (!s.has_map) return ceil_div(s.M, chunk);
  int64_t n = 0;
  for (int k = 0; k < s.K; ++k) n += ceil_div(wgrad_offset_len(s, k), chunk);
  return n;
}
// lo: smallest admissible chunk (keeps the number of chunk slots bounded, see spconv_wgrad_workspace)
static int wgrad_chunk(const WgradShape& s, int lo, int64_t wgs_per_chunk, int64_t slots) {
  auto cost = [&](int c) { return ceil_div(wgrad_num_chunks(s, c) * wgs_per_chunk, slots) * ceil_div(c, 256); };
  int64_t best_cost = -1;
  for (int c = std::max(lo, kWgradMaxChunk); c >= lo; c -= kWgradChunkStep) {
    const int64_t v = cost(c);
    if (best_cost < 0 || v < best_cost) best_cost = v;
  }
  // the largest chunk within 4 % of the best: fewer slabs to write and to sum
  for (int c = std::max(lo, kWgradMaxChunk); c >= lo; c -= kWgradChunkStep)
    if (cost(c) * 100 <= best_cost * 104) return c;
  return lo;
}

// Row blocks of a tile-stationary launch: `per_cu` resident workgroups per CU (wgrad_x3t_kernel: two -- one per CU: 238.6
// against 240 pairs/s in the step; the producer / consumer form is one 8-wave workgroup per CU); one round of them, at
// least 4 tiles per workgroup, a multiple of 8 row blocks.
// (The producer / consumer form takes 8 x NG x (RB / 8) = 224 of the 256 CUs at NG = 7: with every CU used -- 36 row
//  blocks, 252 workgroups -- it is 11 % faster alone (0.501 against 0.560 ms) and SLOWER in the step (253.1-254.6 against
//  256.6-256.9 pairs/s): the CUs it leaves are where the backward chain's kernels run meanwhile; fewer row blocks lose
//  again -- 24: 254.6, 16: 252.7.  profiles/r04jk_wgrad_producer_consumer.txt)
static int wgrad_x3t_rb(int64_t n_rows, int gy, int gz, int per_cu, int K) {
  const int NG = (K + kWgradTKG - 1) / kWgradTKG;
  const int64_t n_tiles = ceil_div(n_rows, 64);
  int64_t rb = (int64_t)per_cu * num_cu() / ((int64_t)NG * gy * gz);
  rb = std::min<int64_t>(rb, n_tiles / 4);
  rb = std::max<int64_t>(8, std::min<int64_t>(kWgradTMaxRB, rb / 8 * 8));
  return (int)rb;
}
// The shape side of the tile-stationary family: a 3^3 / stride-1 map, or none -- a 1x1 convolution is gW = X^T G over all
// rows, the same kernel with K = 1 and the identity table.
static bool wgrad_x3t_shape(const WgradEnv& env, const WgradShape& s) {
  const bool form = s.has_map ? (s.kernel_size == 3 && s.stride == 1) : env.x3t_dense;
  return form && env.x3t_min_rows > 0 && s.n_out >= env.x3t_min_rows && s.n_in == s.n_out && s.cin >= 64 && s.cout >= 64 &&
         wgrad_x3t_tw(s.cin) > 0 && wgrad_x3t_tw(s.cout) > 0 && s.x_bytes <= kWgradBufMaxBytes && s.g_bytes <= kWgradBufMaxBytes;
}

// The kernel family of a call, its tile shape and whether the layer may join a group: everything of the plan but the
// sizes of a pair-list launch (the chunk search is the expensive part of planning, and wgrad_group_add has no use for it).
// Returns PCMI_OK, or the refusal of a shape no kernel takes (the plan is then unspecified).
static int plan_wgrad_family(const WgradEnv& env, const WgradShape& s, WgradPlan* out) {
  WgradPlan p = {};
  const int64_t per_k = (int64_t)s.cin * s.cout;
  if (s.M == 0) {  // nothing to sum: gW (and gbias) are zeroed or left as they are
    p.kernel = PCMI_WGRAD_KERNEL_NONE;
    *out = p;
    return PCMI_OK;
  }
  if (!s.transpose && !s.gbias && s.aligned && wgrad_x3t_shape(env, s)) {
    PCMI_REQUIRE(s.K <= PCMI_MAX_KERNEL_VOLUME, PCMI_ERR_UNSUPPORTED, "wgrad x3t: %d offsets", s.K);
    // The one-term mode takes the one-role kernel: wgrad_x3p_kernel<..., 1> compiles with its producers' register sets on
    // the stack (.private_segment_fixed_size 480 B, scratch loads and stores; the three-term form has none) and measured
    // 1.03 against 0.44 ms for the three-term kernel on the level-1 96 -> 96 launch.
    const bool pc = s.terms != 1 && env.x3p;
    p.kernel = pc ? PCMI_WGRAD_KERNEL_X3P : PCMI_WGRAD_KERNEL_X3T;
    p.terms = s.terms;
    p.tile_c = wgrad_x3t_tw(s.cin);
    p.tile_n = wgrad_x3t_tw(s.cout);
    p.grid_y = s.cin / (32 * p.tile_c);
    p.grid_z = s.cout / (32 * p.tile_n);
    p.NG = (s.K + kWgradTKG - 1) / kWgradTKG;
    p.RB = wgrad_x3t_rb(s.n_out, p.grid_y, p.grid_z, pc ? 1 : kWgradTMaxPerCu, s.K);
    p.tiles_per_rb = (int)ceil_div(ceil_div(s.n_out, 64), p.RB);
    p.sorted_order = s.has_map && s.has_perm;
    p.slab_bytes = (size_t)s.K * p.RB * per_k * sizeof(float);
    p.ws_bytes = p.slab_bytes;
    *out = p;
    return PCMI_OK;
  }
  // the stem's gradient on the matrix cores; the shapes it refuses take the pair-list form (stem_wgrad_kernel)
  if (s.cin == 3 && s.K == 27 && s.has_map && s.has_nbr && !s.transpose && s.stride == 1 && s.n_in == s.n_out && s.cout % 32 == 0 &&
      !s.gbias) {
    p.kernel = PCMI_WGRAD_KERNEL_STEM_MFMA;
    p.grid_z = s.cout / 32;
    p.stem_wgs = (int)std::min<int64_t>(kStemSlabs, ceil_div(s.n_out, 64));
    p.slab_bytes = (size_t)p.stem_wgs * s.K * per_k * sizeof(float);
    p.ws_bytes = p.slab_bytes;
    *out = p;
    return PCMI_OK;
  }
  if (s.cin < 8) {
    PCMI_REQUIRE(s.cin == 3 && s.cout % 32 == 0, PCMI_ERR_UNSUPPORTED, "spconv_bwd_weight: cin=%d only supported as the 3-channel stem",
                 s.cin);
    p.kernel = PCMI_WGRAD_KERNEL_STEM;
    p.grid_y = p.grid_z = 1;
    *out = p;
    return PCMI_OK;
  }
  PCMI_REQUIRE(s.cin % 32 == 0 && s.cout % 32 == 0, PCMI_ERR_UNSUPPORTED, "spconv_bwd_weight: channels (%d, %d) must be multiples of 32",
               s.cin, s.cout);
  PCMI_REQUIRE(s.aligned, PCMI_ERR_INVALID, "spconv_bwd_weight: operands must be 16-byte aligned with ld %% 4 == 0");
  p.kernel = PCMI_WGRAD_KERNEL_PAIRS;
  p.tile_c = wgrad_pair_tiles(s.cin);
  p.tile_n = wgrad_pair_tiles(s.cout);
  p.grid_y = s.cin / (32 * p.tile_c);
  p.grid_z = s.cout / (32 * p.tile_n);
  // In a group every offset is ONE chunk (the workgroup adds its tile straight into the flat gradient: no slabs, no
  // arrival counters): a single launch cuts a 2700-row offset into several chunks to get enough workgroups, a group has
  // them from its other layers.  Up to kWgradMaxChunk pairs per offset (the longest chunk a single launch may take).
  // Candidates: 3^3 / stride-1 maps, accumulating, 32-multiples of channels, 32-bit addressable operands, not taken by
  // the tile-stationary family.
  const int64_t bound = wgrad_offset_bound(s.n_in, s.n_out);
  p.groupable = env.group && s.has_map && s.accumulate && !s.transpose && !s.gbias && s.kernel_size == 3 && s.stride == 1 &&
                s.K <= PCMI_MAX_KERNEL_VOLUME && s.n_in == s.n_out && s.x_bytes <= kWgradBufMaxBytes && s.g_bytes <= kWgradBufMaxBytes &&
                !wgrad_x3t_shape(env, s) && bound <= kWgradMaxChunk;
  p.group_chunk = p.groupable ? (int)align_up((size_t)bound, kWgradChunkStep) : 0;
  *out = p;
  return PCMI_OK;
}

// Returns PCMI_OK and the whole plan, or the family's refusal.
static int plan_wgrad(const WgradEnv& env, const WgradShape& s, WgradPlan* out) {
  WgradPlan p;
  const int rc = plan_wgrad_family(env, s, &p);
  if (rc) return rc;
  const bool stem = p.kernel == PCMI_WGRAD_KERNEL_STEM;
  if (stem || p.kernel == PCMI_WGRAD_KERNEL_PAIRS) {
    // The launch is sized WITHOUT the per-offset pair counts (pcmi_coords_plan_unet leaves them on the device): every
    // offset gets mpk = ceil(bound / chunk) chunk slots and a workgroup whose slot lies behind the offset's last pair
    // leaves at once (WgradArgs::mpk).  The counts, when the host has them, only steer the chunk size.
    const int64_t per_k = (int64_t)s.cin * s.cout;
    const int64_t slots = (int64_t)(stem ? kStemSlotsPerCu : s.slots_per_cu) * num_cu();
    p.chunk = wgrad_chunk(s, wgrad_lo_chunk(s.n_in, s.n_out, s.K, s.M), (int64_t)p.grid_y * p.grid_z, slots);
    p.mpk = s.has_map ? (int)ceil_div(wgrad_offset_bound(s.n_in, s.n_out), p.chunk) : 0;
    p.nchunks = s.has_map ? (int64_t)s.K * p.mpk : ceil_div(s.M, p.chunk);
    const int64_t max_per_k = s.has_map ? p.mpk : p.nchunks;  // bound of the chunks of one offset
    p.mode = stem ? kSlabs : (max_per_k <= 1 ? kDirect : (max_per_k <= kArriveMax ? kArrive : kSlabs));
    p.buf = env.buf && s.x_bytes <= kWgradBufMaxBytes && s.g_bytes <= kWgradBufMaxBytes;
    p.reduce_lanes = p.mode != kSlabs ? 0 : (p.nchunks > 16 * (int64_t)s.K ? 8 : 1);
    p.counters = p.mode == kArrive ? (size_t)s.K * p.grid_y * p.grid_z : 0;
    // (the column sums start at the next 256 bytes)
    p.slab_bytes = p.mode == kDirect ? 0 : (size_t)p.nchunks * per_k * sizeof(float);
    p.colsum_offset = align_up(p.slab_bytes, 256);
    p.colsum_bytes = s.gbias ? (size_t)kColsumBlocks * s.cout * sizeof(float) : 0;
    p.ws_bytes = s.gbias ? p.colsum_offset + p.colsum_bytes : p.slab_bytes;
  }
  *out = p;
  return PCMI_OK;
}

// An upper bound of plan_wgrad(...).ws_bytes over every environment-independent input the caller of
// pcmi_spconv_workspace_bytes does not give (gbias, alignment, counts, residency): the chunk slots at the smallest
// admissible chunk, the tile-stationary slabs at the largest row-block count either form can take, the stem's slabs, and
// the column sums behind the largest of them.
static size_t wgrad_workspace_bound(const WgradEnv& env, int64_t n_in, int64_t n_out, int cin, int cout, int K, int64_t M) {
  if (M <= 0) M = std::max(n_in, n_out);
  const size_t per_k = (size_t)cin * cout * sizeof(float);
  const int lo = wgrad_lo_chunk(n_in, n_out, K, M);
  const int64_t nchunks = K > 1 ? (int64_t)K * ceil_div(wgrad_offset_bound(n_in, n_out), lo) : ceil_div(M, lo);
  const size_t pairwise = (size_t)std::max<int64_t>(nchunks, 1) * per_k;
  size_t tiled = 0;
  if (K == PCMI_MAX_KERNEL_VOLUME && n_in == n_out) {
    const int MTW = wgrad_x3t_tw(cin), NTW = wgrad_x3t_tw(cout);
    if (MTW > 0 && NTW > 0 && env.x3t_min_rows > 0 && n_out >= env.x3t_min_rows && cin >= 64 && cout >= 64)
      tiled = (size_t)K * wgrad_x3t_rb(n_out, cin / (32 * MTW), cout / (32 * NTW), kWgradTMaxPerCu, K) * per_k;
  } else if (K == 1 && n_in == n_out) {
    tiled = (size_t)kWgradTMaxRB * per_k;  // the dense 1x1 form: one slab per row block
  }
  const size_t stem_slabs = cin == 3 ? (size_t)kStemSlabs * K * per_k : 0;  // stem_wgrad_mfma_kernel
  return std::max(std::max(pairwise, tiled), stem_slabs) + (size_t)kColsumBlocks * cout * sizeof(float);
}

}  // namespace pcmi
