/*
 * pcmi.h -- C ABI of libpcmi.so: the MI355X-native (gfx950 / CDNA4) sparse-voxel
 * contrastive pre-training hot path.
 *
 * This library replaces, for the path named by BASELINE.json:north_star, what the
 * reference reaches through MinkowskiEngine 0.4.3's pybind11 backend
 * ("MinkowskiEngineBackend", third-party, not vendored under /root/reference) and
 * a handful of torch ops.  Each entry point cites the reference call site it
 * replaces ("pc/" = /root/reference/pretrain/pointcontrast/).
 *
 * Conventions
 *   - every function returns PCMI_OK (0) or a negative PCMI_ERR_* code; the message
 *     of the last failure on the calling thread is pcmi_last_error();
 *   - every pointer is a DEVICE pointer owned by the caller (e.g. a torch tensor's
 *     data_ptr) unless its name ends in _host;
 *   - every call takes the HIP stream to enqueue on (pcmi_stream_t == hipStream_t);
 *     nothing synchronises except where the comment says "syncs";
 *   - float tensors are row-major fp32 [rows, channels] with an explicit leading
 *     dimension (*_ld, in floats) so producers can write into column slices of a
 *     wider buffer (zero-copy concat, pc/model/res16unet.py:235,242,249,256);
 *   - ops never allocate device memory: scratch comes from the caller through
 *     (ws, ws_bytes), sized by the matching *_workspace_bytes() query.  The one
 *     exception is the coordinate manager, which owns an arena that is reused
 *     across pcmi_coords_reset() calls (one hipMalloc burst in the first
 *     iterations, none in steady state);
 *   - a handle is not thread-safe; distinct handles are independent.
 */
#ifndef PCMI_H_
#define PCMI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCMI_OK 0
#define PCMI_ERR_INVALID (-1)     /* bad argument / shape */
#define PCMI_ERR_HIP (-2)         /* HIP runtime failure */
#define PCMI_ERR_DUPLICATE (-3)   /* duplicate coordinates in pcmi_coords_insert */
#define PCMI_ERR_NOKEY (-4)       /* unknown coords key */
#define PCMI_ERR_RANGE (-5)       /* coordinate outside the packable range */
#define PCMI_ERR_UNSUPPORTED (-6) /* configuration outside the hot path */
#define PCMI_ERR_WORKSPACE (-7)   /* workspace too small */

/* ME.RegionType values used by the path (pc/model/modules/common.py:47-60). */
#define PCMI_REGION_HYPERCUBE 0
#define PCMI_REGION_HYBRID 3

#define PCMI_MAX_KERNEL_VOLUME 27

typedef void* pcmi_stream_t; /* hipStream_t */
typedef struct pcmi_coords pcmi_coords_t;

int pcmi_version(void);
const char* pcmi_last_error(void);
/* Number of compute units / arch name of the current HIP device (gfx950 expected). */
int pcmi_device_info(int* n_cu, char* arch_host, int arch_len);

/* ------------------------------------------------------------------------------------------
 * Coordinate manager -- replaces ME CoordsManager / CoordsKey
 *   ME.SparseTensor(feats, coords=...)             pc/lib/ddp_trainer.py:290-297,392-398
 *   strided coordinates of every stride-2 conv     pc/model/res16unet.py:58-64,75-81,92-98,109-115
 * Coordinates are int32 rows (batch, x, y, z), batch index FIRST
 * (pc/lib/ddp_data_loaders.py:68-76); |x|,|y|,|z| < 2^17, 0 <= batch < 1023 for the inserted rows
 * (PCMI_ERR_RANGE otherwise).  Strided levels may hold -2^17 = floor(-(2^17 - 1) / ts) * ts: its key
 * field is 0, a valid key, and kernel maps find such rows and their neighbours like any other.
 * Key 0 is the inserted set (tensor stride 1); row i of a feature matrix belongs to
 * row i of its key's coordinates.
 * ------------------------------------------------------------------------------------------ */
int pcmi_coords_create(int dimension /* must be 3 */, pcmi_coords_t** out);
int pcmi_coords_destroy(pcmi_coords_t* h);
/* Forget all keys and maps but keep the device arena (one manager per SparseTensor per
 * iteration in the reference; here a pooled handle is reset instead). */
int pcmi_coords_reset(pcmi_coords_t* h);
/* Build the hash of n rows -> key 0.  Syncs (returns PCMI_ERR_DUPLICATE / PCMI_ERR_RANGE). */
int pcmi_coords_insert(pcmi_coords_t* h, const int32_t* bxyz, int64_t n, pcmi_stream_t stream);
/* The same without the synchronisation: the insert is only enqueued, and a duplicate / out-of-range row is reported by
 * the next call on this handle that synchronises `stream` anyway (pcmi_coords_plan_unet, pcmi_coords_stride, a
 * pcmi_kmap_get miss) or by pcmi_coords_check.  For callers that plan the whole network right behind the insert
 * (the training step: one host wait per batch instead of one per call). */
int pcmi_coords_insert_deferred(pcmi_coords_t* h, const int32_t* bxyz, int64_t n, pcmi_stream_t stream);
int pcmi_coords_check(pcmi_coords_t* h, pcmi_stream_t stream); /* syncs if a deferred insert is still unchecked */
/* Two-segment batches (the two point clouds of a contrastive pair processed as ONE sparse tensor: the reference runs
 * its network once per cloud, ddp_trainer.py:404-407, so BatchNorm statistics are per cloud).  The caller inserts the
 * rows of the first cloud before those of the second, with disjoint batch indices, and declares the boundary;
 * pcmi_coords_split returns the boundary of any level (strided levels keep first-occurrence order, so the segments
 * stay contiguous) or -1 when none was declared.  set_split: after insert, before the first stride. */
int pcmi_coords_set_split(pcmi_coords_t* h, int64_t n_first);
int pcmi_coords_split(pcmi_coords_t* h, int key, int64_t* n_first);
/* Strided coordinates: unique floor(c / (stride*ts)) * (stride*ts); rows are in
 * first-occurrence order of the input rows.  Cached per tensor stride.  Syncs on a miss. */
int pcmi_coords_stride(pcmi_coords_t* h, int in_key, int stride, int* out_key, int64_t* n_out,
                       pcmi_stream_t stream);
int pcmi_coords_key_at_stride(pcmi_coords_t* h, int tensor_stride, int* key);
int pcmi_coords_size(pcmi_coords_t* h, int key, int64_t* n, int* tensor_stride);
/* Copy the key's coordinates into out_bxyz [n,4] (device). */
int pcmi_coords_get(pcmi_coords_t* h, int key, int32_t* out_bxyz, pcmi_stream_t stream);
/* Build every level (strides 2,4,..,2^n_down) and the kernel maps a Res16UNet forward
 * uses up front (typically on a side stream while the compute stream is still busy), so
 * the per-layer calls below all hit the cache and never sync.  Pure performance hint.  first_region: region of the 3^3 stem conv (HYPERCUBE),
 * block_region: region of the 3^3 block convs (HYBRID).
 * ONE host synchronisation per call (round 2: 16): the levels of a fresh handle are built as a chain whose kernels take
 * their row counts from the device and whose counts come back together; the maps are then enqueued without waiting for
 * their per-offset pair counts (pcmi_kmap_get hands those out later; no kernel of this library needs them on the
 * host).  The tables are complete when `stream` reaches the end of the call: a consumer on another stream must be
 * ordered behind it (pcmi_net_forward does that itself). */
int pcmi_coords_plan_unet(pcmi_coords_t* h, int n_down, int first_region, int block_region,
                          pcmi_stream_t stream);
/* Bytes currently reserved by the handle's arena (for memory accounting). */
int pcmi_coords_arena_bytes(pcmi_coords_t* h, size_t* bytes);

/* ------------------------------------------------------------------------------------------
 * Kernel maps -- replaces CoordsManager::getInOutMaps (reached from every
 * MinkowskiConvolution / MinkowskiConvolutionTranspose forward,
 * pc/model/modules/common.py:130-139,159-168).
 * Pair (i, j, k): in-row i feeds out-row j through weight slice k iff
 *   c_out[j] + offset_k * tensor_stride(in) == c_in[i].
 * Offsets in weight-slice order come from pcmi_kernel_offsets().
 * All pointers live in the handle's arena and stay valid until reset/destroy.
 * ------------------------------------------------------------------------------------------ */
typedef struct pcmi_kmap {
  int32_t K;               /* kernel volume (27, 8) */
  int32_t kernel_size;     /* 3 or 2 */
  int32_t stride;          /* 1 or 2 */
  int32_t region;
  int64_t n_in, n_out;
  int64_t M;               /* total number of pairs; -1 in a map taken while pcmi_coords_plan_unet's counts were still
                            * on their way (internal use: pcmi_kmap_get always returns it filled in) */
  const int32_t* nbr;      /* [K, n_out]: in-row for (k, out-row) or -1 */
  const int32_t* pair_in;  /* [M] grouped by k, ascending out-row inside a group */
  const int32_t* pair_out; /* [M] */
  const int64_t* offs;     /* [K+1] device prefix of the group sizes */
  int64_t offs_host[PCMI_MAX_KERNEL_VOLUME + 1];
  int32_t mirror[PCMI_MAX_KERNEL_VOLUME]; /* offset_{mirror[k]} == -offset_k (stride 1) */
  /* Processing order for the conv kernels (stride-1 maps of large levels, else NULL): rows sorted by their
   * 27-bit neighbour-occupancy mask so that a 32-row wave group shares its set of occupied offsets.
   * perm[i] = row handled at position i; nbr_perm[k][i] = nbr[k][perm[i]].  Results are unaffected. */
  const int32_t* perm;
  const int32_t* nbr_perm;
  /* Work units of the 128-row tiles of that order (NULL when perm is NULL): tile_mask[t] = OR of the occupancy
   * masks of the tile's rows, tile_pref[t] = number of (tile, occupied offset) units before tile t
   * (tile_pref[n_tiles] = total).  Lets the conv kernel give every workgroup the same number of units. */
  const uint32_t* tile_mask;
  const int32_t* tile_pref;
  int64_t n_tiles;
} pcmi_kmap_t;

/* Host-side enumeration of the kernel offsets in weight-slice order
 * (ME.KernelGenerator, pc/model/modules/common.py:127-128,151-157).  out_host: [K,3]. */
int pcmi_kernel_offsets(int kernel_size, int region, int32_t* out_host, int* K);
/* kernel_size 3 / stride 1 (in_key == out_key) or kernel_size 2 / stride 2
 * (out_key = strided key of in_key).  Cached; one stream sync on a miss (reads back the
 * K+1 group offsets). */
int pcmi_kmap_get(pcmi_coords_t* h, int in_key, int out_key, int kernel_size, int stride,
                  int region, pcmi_kmap_t* out, pcmi_stream_t stream);
/* Copy a map's tables into caller buffers (any may be NULL): nbr [K*n_out], pair_in [M],
 * pair_out [M].  For parity checks and ME-style get_kernel_map(); not on the hot path. */
int pcmi_kmap_export(const pcmi_kmap_t* map, int32_t* nbr, int32_t* pair_in, int32_t* pair_out,
                     pcmi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Instances -- replaces ME's origin coordinates (CoordsManager::getOriginCoords) and the
 * per-batch-index row lists behind
 *   ME.MinkowskiGlobalPooling                      pc/model/res16unet.py:10 (import);
 *                                                  downstream/semseg/lib/layers.py:54-90
 *   ME.MinkowskiInstanceNorm                       pc/model/modules/common.py:22-23
 * An instance is one batch index (column 0 of the coordinates).  Rows need not be sorted
 * by it.  The origin key holds one row (b, 0, 0, 0) per distinct batch index, ascending,
 * tensor stride 0; it has no hash and no kernel maps.
 * ------------------------------------------------------------------------------------------ */
#define PCMI_SEGMENT_CHUNK 256 /* rows per work unit of the segment reductions */
typedef struct pcmi_segments {
  int64_t n;                 /* rows of the key */
  int64_t n_inst;            /* instances: distinct batch indices */
  int64_t n_chunks;          /* chunk_offs[n_inst] */
  const int32_t* rows;       /* [n] the key's rows grouped by instance (ascending batch index), ascending inside one */
  const int32_t* offs;       /* [n_inst + 1] instance i holds rows[offs[i] .. offs[i+1]) */
  const int32_t* inst;       /* [n] instance of every row */
  const int32_t* chunk_offs; /* [n_inst + 1] instance i is split into chunks chunk_offs[i] .. chunk_offs[i+1]) of
                              * PCMI_SEGMENT_CHUNK rows (the last one shorter) */
} pcmi_segments_t;
/* The origin key (built from key 0 on the first call, cached until reset).  Syncs on a miss (n_inst). */
int pcmi_coords_origin(pcmi_coords_t* h, int* key, int64_t* n_inst, pcmi_stream_t stream);
/* Row -> instance CSR of `key`: a 1024-bin histogram of the batch index, a scan and a stable scatter, on the device.
 * Cached in the arena per key until reset.  Syncs on a miss (n_inst, n_chunks). */
int pcmi_coords_segments(pcmi_coords_t* h, int key, pcmi_segments_t* out, pcmi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Sparse convolution -- replaces MEB.Convolution{Forward,Backward}GPU and
 * ConvolutionTranspose{Forward,Backward}GPU (pc/model/modules/common.py:117-168; 63 modules
 * in Res16UNet34C).  weight is [K, cin, cout] fp32 (K == 1: [cin, cout], map == NULL: the
 * dense 1x1 "use_mm" path).  transpose == 0: conv along the map (in = map.n_in rows,
 * out = map.n_out rows).  transpose == 1: transposed conv (in = map.n_out rows,
 * out = map.n_in rows, same weight-slice index).
 *   fwd        out[j]  = sum_k in[i] @ W[k]      (+ bias)
 *   bwd_data   gin[i]  = sum_k gout[j] @ W[k]^T
 *   bwd_weight gW[k]   = sum_pairs in[i]^T gout[j]
 * All three overwrite their outputs (no accumulate) and are deterministic (no float atomics).
 * out_ld / gin_ld may exceed the width (the output as a column slice of a wider buffer): the columns outside the slice
 * are left untouched.  Feature matrices -- inputs and outputs -- start 16-byte aligned with a leading dimension that is a
 * multiple of 4 (PCMI_ERR_INVALID otherwise); ws holds at least pcmi_spconv_workspace_bytes() bytes for the same shape
 * (PCMI_ERR_WORKSPACE otherwise).  A refused call enqueues nothing.  tests/test_gpu_c_contract.py holds all of this.
 * ------------------------------------------------------------------------------------------ */
size_t pcmi_spconv_workspace_bytes(int64_t n_in, int64_t n_out, int cin, int cout, int K,
                                   int64_t M);
int pcmi_spconv_fwd(const float* in, int64_t in_ld, int64_t n_in, int cin, const float* weight,
                    int cout, const pcmi_kmap_t* map, int transpose, const float* bias,
                    float* out, int64_t out_ld, int64_t n_out, void* ws, size_t ws_bytes,
                    pcmi_stream_t stream);
int pcmi_spconv_bwd_data(const float* gout, int64_t gout_ld, int64_t n_out, int cout,
                         const float* weight, int cin, const pcmi_kmap_t* map, int transpose,
                         float* gin, int64_t gin_ld, int64_t n_in, void* ws, size_t ws_bytes,
                         pcmi_stream_t stream);
int pcmi_spconv_bwd_weight(const float* in, int64_t in_ld, int64_t n_in, int cin,
                           const float* gout, int64_t gout_ld, int64_t n_out, int cout,
                           const pcmi_kmap_t* map, int transpose, float* gweight,
                           float* gbias /* nullable [cout] */, void* ws, size_t ws_bytes,
                           pcmi_stream_t stream);
/* 1 if the matrix-bound forward / backward-data launches (>= 64 channels on both sides, >= 512 rows) run the
 * split-precision kernel -- fp32 operands as three bf16 terms each on the bf16 matrix cores, fp32 accumulation,
 * results within fp32 round-off of the fp32-MFMA kernel (csrc/spconv_x3.hip) -- else 0 (environment
 * PCMI_CONV16_X3=0).  The reference has no counterpart: MinkowskiEngine's GEMMs are cuBLAS fp32
 * (pc/model/modules/common.py:117-168 reach them through ME.MinkowskiConvolution). */
int pcmi_spconv_split_precision(void);

/* What one forward / backward-data launch over `rows` output rows will do (csrc/spconv_plan.h: plan_conv, the function
 * the launch itself executes): host code only -- no device memory touched, nothing enqueued, usable without a GPU (the
 * plan then counts the MI355X's 256 compute units).  It reads the environment as a convolution call does.
 *   x_bytes  size of the gathered operand (its rows x leading dimension x 4): from 2 GiB on the kernels that address it
 *            with 32-bit offsets are out
 *   C, N     contraction size and output channels (multiples of 32): cin -> cout in the forward, cout -> cin in the
 *            backward-data launch
 *   K        offsets of the map (1 without one)
 *   form     how the launch gathers, PCMI_CONV_FORM_*:  NONE no map (dense 1x1);  TABLE the neighbour table (forward of
 *            a strided map, both directions of a stride-1 map);  TABLE_UNITS the table of a map that carries the sorted
 *            order and tile units for these rows (perm, nbr_perm, tile_pref, n_tiles == ceil(rows / 128));  PAIRS the
 *            pair lists (backward-data of a strided map, forward of its transposed convolution)
 * Out (each nullable):  kernel PCMI_CONV_KERNEL_*;  rows_per_wave: the row tile is 32 x this (0 for spconv32r);  slice: the
 * output slice of a workgroup is 32 x this channels (0 for spconv32r);  ksplit: offset ranges summed through partial
 * tensors in the workspace (1 = none);  ws_bytes: the smallest workspace the call accepts (at most
 * pcmi_spconv_workspace_bytes() of the convolution).  PCMI_ERR_INVALID for a shape no launch has. */
#define PCMI_CONV_FORM_NONE 0
#define PCMI_CONV_FORM_TABLE 1
#define PCMI_CONV_FORM_TABLE_UNITS 2
#define PCMI_CONV_FORM_PAIRS 3
#define PCMI_CONV_KERNEL_PAIR 0      /* pair tiles (spconv_mfma_kernel, PAIR) */
#define PCMI_CONV_KERNEL_32R 1       /* spconv32r_kernel: 32 -> 32 channels, weights resident in LDS */
#define PCMI_CONV_KERNEL_UNITS_16 2  /* unit-balanced 16-row fp32 (spconv16p_kernel, SK) + sk_fixup_kernel */
#define PCMI_CONV_KERNEL_UNITS_X3 3  /* unit-balanced split-precision (spconv16x_kernel, SK) + sk_fixup_kernel */
#define PCMI_CONV_KERNEL_TABLE_X3 4  /* table split-precision (spconv16x_kernel) */
#define PCMI_CONV_KERNEL_TABLE_16 5  /* table 16-row fp32 (spconv16p_kernel) */
#define PCMI_CONV_KERNEL_DEEP 6      /* 128-row tiles in 64-channel chunks (spconv_mfma_kernel, KC 64) */
#define PCMI_CONV_KERNEL_PLAIN 7     /* 128 / 64 / 32-row tiles (spconv_mfma_kernel) */
int pcmi_spconv_plan(int64_t rows, int64_t x_bytes, int C, int N, int K, int form, int* kernel, int* rows_per_wave,
                     int* slice, int* ksplit, size_t* ws_bytes);

/* What one pcmi_spconv_bwd_weight call will do (csrc/spconv_wgrad_plan.h: plan_wgrad, the function the call itself
 * executes): host code only, as pcmi_spconv_plan.  It reads the environment (PCMI_WGRAD_*) and the calling thread's
 * convolution precision as the call does.
 *   n_in, n_out, cin, cout, transpose, gbias (0 / 1: a bias gradient is wanted)   as in the call
 *   K             offsets of the map (1 without one)
 *   kernel_size, stride   of the map (3, 1 or 2, 2); kernel_size 0: no map (the dense 1x1 form)
 *   map_tables    PCMI_WGRAD_MAP_NBR: the map carries nbr;  PCMI_WGRAD_MAP_PERM: it carries perm and nbr_perm
 *   accumulate    1: the call adds to gweight (the executor's calls; pcmi_spconv_bwd_weight itself overwrites: 0)
 *   x_bytes, g_bytes   size of `in` and `gout` (rows x leading dimension x 4)
 *   aligned       1: both start 16-byte aligned and their leading dimensions are multiples of 4
 *   counts_host   nullable [K + 1]: host prefix of the per-offset pair counts (pcmi_kmap_t::offs_host) when the map has
 *                 them (M >= 0); NULL: the plan works with the bounds a launch takes in front of their arrival
 *   slots_per_cu  resident workgroups per CU of the pair-list kernel's variant; 0: ask the HIP runtime, as a launch does
 *                 (2 where it cannot be asked)
 * Out (each nullable):  kernel PCMI_WGRAD_KERNEL_*;  tile_c, tile_n: per workgroup and axis, the 32-channel tiles of
 * wgrad_mfma_kernel or the 16-wide tiles per wave of the tile-stationary kernels (0 for the stems);  chunk: pairs per
 * workgroup, and slots_per_offset: chunk slots of an offset (0 without a map), of the pair-list kernels;  mode
 * PCMI_WGRAD_MODE_*: how the chunks of an offset become gW;  address_bits: 32 or 64, how wgrad_mfma_kernel addresses its
 * operands (0 for the other kernels);  row_blocks: of the tile-stationary kernels, or the workgroups of
 * stem_wgrad_mfma_kernel;  groupable: 1 if the executor may put the layer into a grouped launch;  ws_bytes: the smallest
 * workspace the call accepts (at most pcmi_spconv_workspace_bytes() of the convolution).
 * PCMI_ERR_INVALID / PCMI_ERR_UNSUPPORTED for a shape no launch has, as the call itself returns them. */
#define PCMI_WGRAD_MAP_NBR 1
#define PCMI_WGRAD_MAP_PERM 2
#define PCMI_WGRAD_KERNEL_NONE 0       /* no pairs: nothing to do but zeroing */
#define PCMI_WGRAD_KERNEL_X3P 1        /* wgrad_x3p_kernel: tile-stationary split precision, producer / consumer */
#define PCMI_WGRAD_KERNEL_X3T 2        /* wgrad_x3t_kernel: the one-role form, and everything in one-term (bf16) mode */
#define PCMI_WGRAD_KERNEL_STEM_MFMA 3  /* stem_wgrad_mfma_kernel: the 3-channel stem on the matrix cores */
#define PCMI_WGRAD_KERNEL_STEM 4       /* stem_wgrad_kernel: the 3-channel stem over the pair list */
#define PCMI_WGRAD_KERNEL_PAIRS 5      /* wgrad_mfma_kernel: the pair list of one offset per workgroup, fp32 MFMA */
#define PCMI_WGRAD_MODE_SLABS 0        /* every workgroup writes a slab, wgrad_reduce_kernel sums them */
#define PCMI_WGRAD_MODE_DIRECT 1       /* one chunk per offset: the workgroup writes gW itself */
#define PCMI_WGRAD_MODE_ARRIVE 2       /* slabs, summed by the last-arriving workgroup of the (offset, tile) */
int pcmi_spconv_wgrad_plan(int64_t n_in, int64_t n_out, int cin, int cout, int K, int kernel_size, int stride, int map_tables,
                           int transpose, int gbias, int accumulate, int64_t x_bytes, int64_t g_bytes, int aligned,
                           const int64_t* counts_host, int slots_per_cu, int* kernel, int* tile_c, int* tile_n, int* chunk,
                           int* slots_per_offset, int* mode, int* address_bits, int* row_blocks, int* groupable, size_t* ws_bytes);

/* Convolution precision mode.  PCMI_CONV_PRECISION_FP32 (the default) is the arithmetic above.  In
 * PCMI_CONV_PRECISION_BF16 the launches the split-precision kernels take by default -- the forward / backward-data
 * launches of spconv16x (>= 64 channels on both sides, >= 512 rows, table and unit-balanced form) and the weight
 * gradients of wgrad_x3t (3^3 stride-1 and dense 1x1 layers, >= 8192 rows, >= 64 channels) -- round both operands to
 * bf16 (round to nearest even) and contract them with ONE bf16 product per 32-channel chunk, fp32 accumulation
 * (relative error of order 2^-9 per product instead of fp32 round-off).  Every other launch, and every other op, is
 * bit-identical in both modes; parameters, activations and gradients stay fp32.  PCMI_CONV16_X3=0 is a diagnostic of
 * the fp32 mode only: with it the forward / backward-data launches take the fp32-MFMA kernel in both modes.  The
 * reference has no counterpart (its GEMMs are cuBLAS fp32); the switch is the analogue of torch's autocast.
 *   pcmi_set_conv_precision: the CALLING THREAD's mode for its eager pcmi_spconv_* calls (thread-local, default fp32).
 *   pcmi_net_set_conv_precision: the mode of every later pcmi_net_forward / pcmi_net_backward of `net`, applied for the
 *     duration of the call (the thread's own mode is restored on return).
 * PCMI_ERR_INVALID for any other value. */
#define PCMI_CONV_PRECISION_FP32 0
#define PCMI_CONV_PRECISION_BF16 1
int pcmi_set_conv_precision(int precision);
int pcmi_get_conv_precision(void);

/* ------------------------------------------------------------------------------------------
 * Normalisation / elementwise
 *   BatchNorm1d inside ME.MinkowskiBatchNorm      pc/model/modules/common.py:19-21
 *   MinkowskiReLU, `out += residual`              pc/model/modules/resnet_block.py:41,57
 *   L2 row normalisation of the output features   pc/model/res16unet.py:262-266
 * bn_fwd_train: batch statistics over the n rows (biased var for normalisation, unbiased
 * for the running estimate, as torch), y = relu?((x-mean)*invstd*gamma+beta (+ residual)).
 * The variance is sum x^2 - (sum x)^2 / n only where that is well conditioned: a row block also
 * sums d = x - K and d^2 with K the column's value in the block's first row, and a column whose
 * M2 is below 1/256 of its sum x^2 (|mean| / std > 16) gets (K + sum d / n_b, sum d^2 -
 * (sum d)^2 / n_b); the blocks are merged with Chan's update; up to 1536 rows the one launch
 * takes a centred second pass.  Tested per column to 1e-4 of float64 at mean / std = 256 and on
 * constant columns, whose mean is their value to the bit and whose variance is exactly 0.
 * bn_bwd: gradients of that fused expression; relu_mask_y (nullable) is the forward output
 * whose sign gives the ReLU mask; dres (nullable) receives the residual-branch gradient.
 * ------------------------------------------------------------------------------------------ */
size_t pcmi_bn_workspace_bytes(int64_t n, int c);
int pcmi_bn_fwd_train(const float* x, int64_t x_ld, int64_t n, int c, const float* gamma,
                      const float* beta, float* running_mean, float* running_var,
                      float momentum, float eps, const float* residual, int64_t res_ld, int relu,
                      float* y, int64_t y_ld, float* save_mean, float* save_invstd, void* ws,
                      size_t ws_bytes, pcmi_stream_t stream);
int pcmi_bn_fwd_eval(const float* x, int64_t x_ld, int64_t n, int c, const float* gamma,
                     const float* beta, const float* running_mean, const float* running_var,
                     float eps, const float* residual, int64_t res_ld, int relu, float* y,
                     int64_t y_ld, pcmi_stream_t stream);
int pcmi_bn_bwd(const float* dy, int64_t dy_ld, const float* x, int64_t x_ld,
                const float* relu_mask_y, int64_t y_ld, int64_t n, int c, const float* gamma,
                const float* save_mean, const float* save_invstd, float* dx, int64_t dx_ld,
                float* dres, int64_t dres_ld, float* dgamma, float* dbeta, void* ws,
                size_t ws_bytes, pcmi_stream_t stream);
int pcmi_relu_fwd(const float* x, int64_t x_ld, int64_t n, int c, float* y, int64_t y_ld,
                  pcmi_stream_t stream);
int pcmi_relu_bwd(const float* dy, int64_t dy_ld, const float* y, int64_t y_ld, int64_t n, int c,
                  float* dx, int64_t dx_ld, pcmi_stream_t stream);
int pcmi_add(const float* a, int64_t a_ld, const float* b, int64_t b_ld, int64_t n, int c,
             float* y, int64_t y_ld, pcmi_stream_t stream);
int pcmi_l2norm_fwd(const float* x, int64_t x_ld, int64_t n, int c, float* y, int64_t y_ld,
                    float* norm /* [n] */, pcmi_stream_t stream);
int pcmi_l2norm_bwd(const float* dy, int64_t dy_ld, const float* y, int64_t y_ld,
                    const float* norm, int64_t n, int c, float* dx, int64_t dx_ld,
                    pcmi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Row gather / scatter-add used by the losses (F0[q_idx], pc/lib/ddp_trainer.py:209-213,409-410)
 * scatter_add accumulates into dst (caller zero-fills); duplicate indices are summed in increasing source-row
 * order, without float atomics (bit-reproducible; n^2 / 64 wave steps: meant for the losses' n of a few thousand).
 * ------------------------------------------------------------------------------------------ */
int pcmi_gather_rows(const float* src, int64_t src_ld, const int64_t* idx, int64_t n, int c,
                     float* dst, int64_t dst_ld, pcmi_stream_t stream);
int pcmi_scatter_add_rows(const float* src, int64_t src_ld, const int64_t* idx, int64_t n, int c,
                          float* dst, int64_t dst_ld, pcmi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Pooling over kernel maps (csrc/pool.hip) -- replaces MEB.{Sum,Avg}Pooling{Forward,Backward}GPU and
 * PoolingTranspose{Forward,Backward}GPU:
 *   ME.MinkowskiSumPooling                         pc/model/modules/common.py:203-214; pc/model/resnet.py:63
 *   ME.MinkowskiAvgPooling                         pc/model/modules/common.py:170-186
 *   ME.MinkowskiAvgUnpooling                       pc/model/modules/common.py:189-200
 * map: a pcmi_kmap_get map, (k=3, s=1) on one key or (k=2, s=2) from a key to its strided key, with its pair
 * counts on the host (M >= 0).  Any c >= 1.
 * pool_fwd: out[j] = sum_k in[nbr[k][j]]; average != 0 divides by the number of present neighbours of j (ME's
 *   "nonzero average": sum_pool(x) / sum_pool(mask)).  out has map.n_out rows.
 * pool_bwd: gin (map.n_in rows) = the adjoint, in gather form: stride 1 through the mirrored offsets, stride 2 one
 *   write per fine row from the pair lists.  ws: pcmi_pool_workspace_bytes(map.n_out) (the counts of the average).
 * unpool_fwd: out[child] = in[parent] onto the finer key (map: fine -> coarse k2/s2, the conv_tr map; sum and
 *   average coincide since every child has one parent); out has map.n_in rows.  unpool_bwd: the 8-way gather
 *   gin[j] = sum_k gout[nbr[k][j]] (map.n_out rows).
 * No float atomics: every result is reproducible bit for bit.
 * ------------------------------------------------------------------------------------------ */
size_t pcmi_pool_workspace_bytes(int64_t n_out);
int pcmi_pool_fwd(const float* in, int64_t in_ld, int c, const pcmi_kmap_t* map, int average, float* out,
                  int64_t out_ld, pcmi_stream_t stream);
int pcmi_pool_bwd(const float* gout, int64_t gout_ld, int c, const pcmi_kmap_t* map, int average, float* gin,
                  int64_t gin_ld, void* ws, size_t ws_bytes, pcmi_stream_t stream);
int pcmi_unpool_fwd(const float* in, int64_t in_ld, int c, const pcmi_kmap_t* map, float* out, int64_t out_ld,
                    pcmi_stream_t stream);
int pcmi_unpool_bwd(const float* gout, int64_t gout_ld, int c, const pcmi_kmap_t* map, float* gin, int64_t gin_ld,
                    pcmi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-instance reductions over pcmi_segments_t (csrc/pool.hip) -- replaces
 *   ME.MinkowskiGlobalPooling(average)             pc/model/res16unet.py:10; downstream/semseg/lib/layers.py:54-90
 *   ME.MinkowskiBroadcast{Addition,Multiplication} downstream/semseg/lib/layers.py:54-90
 *   ME.MinkowskiInstanceNorm                       pc/model/modules/common.py:22-23;
 *                                                  downstream/semseg/models/modules/resnet_block.py:67-72
 * A segment's rows are split over many workgroups (chunks of PCMI_SEGMENT_CHUNK rows, fp64 partial sums) and a second
 * pass adds the partials of each instance in chunk order: no float atomics, reproducible bit for bit.
 * global_pool_fwd: out [n_inst, c] = per-instance sum (average: mean) of x.  global_pool_bwd: gin[r] = gout[inst(r)]
 *   (average: / rows of the instance).
 * broadcast (op 0: add, 1: multiply): out[r] = x[r] op g[inst(r)], g [n_inst, c].  bwd: gx (nullable) and gg
 *   (nullable, [n_inst, c]: the segment sum of gout, resp. of gout * x).
 * instnorm_fwd: per instance and channel mean and biased variance (centred second pass), y = relu?((x - mean) * invstd
 *   * weight + bias (+ residual)), weight / bias [c] shared by the instances; writes mean / invstd [n_inst, c].
 *   instnorm_bwd: dx, dres (nullable), dweight, dbias [c] (summed over the instances in order); y (nullable) is the
 *   forward output whose sign gives the ReLU mask.
 * ws: pcmi_segments_workspace_bytes(seg, c).
 * ------------------------------------------------------------------------------------------ */
size_t pcmi_segments_workspace_bytes(const pcmi_segments_t* seg, int c);
int pcmi_global_pool_fwd(const float* x, int64_t x_ld, int c, const pcmi_segments_t* seg, int average, float* out,
                         int64_t out_ld, void* ws, size_t ws_bytes, pcmi_stream_t stream);
int pcmi_global_pool_bwd(const float* gout, int64_t gout_ld, int c, const pcmi_segments_t* seg, int average,
                         float* gin, int64_t gin_ld, pcmi_stream_t stream);
int pcmi_broadcast_fwd(const float* x, int64_t x_ld, const float* g, int64_t g_ld, int c, const pcmi_segments_t* seg,
                       int op, float* out, int64_t out_ld, pcmi_stream_t stream);
int pcmi_broadcast_bwd(const float* gout, int64_t gout_ld, const float* x, int64_t x_ld, const float* g, int64_t g_ld,
                       int c, const pcmi_segments_t* seg, int op, float* gx, int64_t gx_ld, float* gg, int64_t gg_ld,
                       void* ws, size_t ws_bytes, pcmi_stream_t stream);
int pcmi_instnorm_fwd(const float* x, int64_t x_ld, int c, const pcmi_segments_t* seg, const float* weight,
                      const float* bias, float eps, const float* residual, int64_t res_ld, int relu, float* y,
                      int64_t y_ld, float* save_mean, float* save_invstd, void* ws, size_t ws_bytes,
                      pcmi_stream_t stream);
int pcmi_instnorm_bwd(const float* dy, int64_t dy_ld, const float* x, int64_t x_ld, const float* relu_mask_y,
                      int64_t y_ld, int c, const pcmi_segments_t* seg, const float* weight, const float* save_mean,
                      const float* save_invstd, float* dx, int64_t dx_ld, float* dres, int64_t dres_ld,
                      float* dweight, float* dbias, void* ws, size_t ws_bytes, pcmi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Positive-pair selection of the PointInfoNCE step (pc/lib/ddp_trainer.py:400-417; csrc/pairs.hip):
 *   q_unique, count = pos_pairs[:, 0].unique(return_counts=True); off = floor(uniform * count);
 *   k_sel = pos_pairs[:, 1][off + exclusive_cumsum(count)]; optional sub-sample [sampled] of both.
 * pairs: device int32 [n_pairs, 2] sorted by column 0 (the loader's contract, pc/lib/ddp_data_loaders.py:43-48,85-91);
 * uniform: device fp32 [n_unique] -- the host's torch.rand(n_unique) draws; sampled: nullable device int64 [n_sel] --
 * the host's np.random.choice(n_unique, npos) (NULL: n_sel == n_unique, every query in order).  Writes q_idx / k_idx
 * (device int64 [n_sel]: rows of F0 / F1).  The random draws stay on the host so that the reference's generator streams
 * are consumed identically; for them the host needs n_unique: pcmi_pairs_scan_host, one pass over column 0 of the
 * HOST copy of the correspondences (*sorted_host == 0: the column is not sorted -- sort before using either call).
 * ------------------------------------------------------------------------------------------ */
size_t pcmi_pair_select_workspace_bytes(int64_t n_pairs);
int pcmi_pair_select(const int32_t* pairs, int64_t n_pairs, int64_t n_unique, const float* uniform,
                     const int64_t* sampled, int64_t n_sel, int64_t* q_idx, int64_t* k_idx, void* ws,
                     size_t ws_bytes, pcmi_stream_t stream);
int pcmi_pairs_scan_host(const int32_t* pairs_host, int64_t n_pairs, int64_t* n_runs_host, int* sorted_host);

/* ------------------------------------------------------------------------------------------
 * PointInfoNCE block -- replaces torch.mm + nn.CrossEntropyLoss
 * (pc/lib/ddp_trainer.py:419-426, pc/lib/criterion.py:13-18):
 *   loss = mean_i( logsumexp_j(q_i.k_j / T) - q_i.k_i / T ),  q, k: [n, c] fp32.
 * The n x n logits are never materialised.  fwd writes lse[n] and *loss (device scalar);
 * bwd writes dq, dk for upstream gradient gscale (device scalar, nullable -> 1).
 * ------------------------------------------------------------------------------------------ */
size_t pcmi_nce_workspace_bytes(int64_t n, int c);
int pcmi_nce_fwd(const float* q, const float* k, int64_t n, int c, float inv_T, float* lse,
                 float* loss, void* ws, size_t ws_bytes, pcmi_stream_t stream);
int pcmi_nce_bwd(const float* q, const float* k, const float* lse, int64_t n, int c, float inv_T,
                 const float* gscale, float* dq, float* dk, void* ws, size_t ws_bytes,
                 pcmi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Hardest-contrastive block (pc/lib/ddp_trainer.py:182-238)
 *   pdist_argmin: dmin[p] = min_s sqrt(|a_p - b_s|^2 + 1e-7), amin[p] = first arg min
 *                 (replaces pdist :182-184 + .min(1) :218-219; no [P,S,C] temporary).
 *                 torch.min's order: a NaN distance is below every number, so a row with one has
 *                 dmin = NaN and amin = its first NaN position; exact ties and rows whose distances
 *                 are all +inf go to the lowest index.  0 <= amin[p] < s always.
 *   keyset: device hash set of int64 keys a + b*M (replaces _hash :39-51 + np.isin :231-234)
 *   hardest_loss: pos = mean(relu(|a-b|^2 - pos_thresh)); neg = (mean_masked(relu(nt-D01)^2)
 *                 + mean_masked(relu(nt-D10)^2)) / 2 (fwd), and the gradients w.r.t. the four
 *                 gathered matrices (bwd).  relu is F.relu: a NaN feature or mined distance makes
 *                 the loss it enters NaN (it is not dropped by the hinge).
 * ------------------------------------------------------------------------------------------ */
int pcmi_pdist_argmin(const float* a, int64_t p, const float* b, int64_t s, int c, float* dmin,
                      int32_t* amin, pcmi_stream_t stream);
size_t pcmi_keyset_bytes(int64_t n_keys);
int pcmi_keyset_build(const int32_t* pairs /* [n,2] */, int64_t n, int64_t M, void* set,
                      size_t set_bytes, pcmi_stream_t stream);
/* mask[p] = 1 iff (a[p] + b[p]*M) is NOT in the set (i.e. the mined negative is kept). */
int pcmi_keyset_mask_absent(const void* set, size_t set_bytes, const int64_t* a, const int64_t* b,
                            int64_t n, int64_t M, uint8_t* mask, pcmi_stream_t stream);
int pcmi_hardest_loss_fwd(const float* posF0, const float* posF1, int64_t p, int c,
                          const float* d01min, const uint8_t* mask0, const float* d10min,
                          const uint8_t* mask1, float pos_thresh, float neg_thresh,
                          float* losses /* [2]: pos, neg */, float* stats /* [5], for bwd */,
                          void* ws, size_t ws_bytes, pcmi_stream_t stream);
/* gl: device [2] upstream gradients of (pos, neg).  dsub* are accumulated (caller zero-fills). */
int pcmi_hardest_loss_bwd(const float* posF0, const float* posF1, int64_t p, const float* subF0,
                          const float* subF1, int c, const float* d01min, const int32_t* d01ind,
                          const uint8_t* mask0, const float* d10min, const int32_t* d10ind,
                          const uint8_t* mask1, float pos_thresh, float neg_thresh,
                          const float* stats, const float* gl, float* dposF0, float* dposF1,
                          float* dsubF0, float* dsubF1, pcmi_stream_t stream);
size_t pcmi_hardest_workspace_bytes(int64_t p);

/* ------------------------------------------------------------------------------------------
 * Optimiser -- replaces torch.optim.SGD.step (pc/lib/ddp_trainer.py:107-111,319,435) on a
 * flat fp32 buffer:  g = grad_scale*g + wd*w;  v = mu*v + g;  w -= lr*v.
 * (dampening 0, no Nesterov; a zero-filled v reproduces torch's first-step buffer init.)
 * ------------------------------------------------------------------------------------------ */
/* ---- loader-side geometry on the device (csrc/loader.hip) -------------------------------------
 * pcmi_voxelize  = ME.utils.sparse_quantize(xyz / voxel_size, return_index=True) of the dataset item
 *   (pc/lib/ddp_data_loaders.py:228-229): first_index[0 .. *n_unique) = ascending indices of the first point of every
 *   occupied voxel, coords (nullable, [n_unique, 3]) = floor(xyz[first_index] / voxel_size).  xyz: device fp64 [n, 3].
 * pcmi_match_radius = get_matching_indices (pc/lib/ddp_data_loaders.py:36-49): all (i, j) with
 *   |R src_i + t - dst_j| <= radius, rigid3x4_host = [R | t] row-major (12 host doubles); pairs [*n_pairs, 2] sorted by
 *   (i, j).  pairs == NULL: only counts.  PCMI_ERR_WORKSPACE if pairs_capacity is too small (*n_pairs_host = needed).
 * Both synchronise the stream (they return counts) and are bit-exact against oracle/loader_ref.py.
 * PCMI_ERR_RANGE: a voxel / cell index outside +-(2^20 - 1), more than 96 matches of one source point, or a
 *   NON-FINITE point (NaN, +-inf) in xyz, in dst or in R src_i + t -- tested before the float -> integer conversion,
 *   which is undefined for them; oracle/loader_ref.py raises for the same inputs. */
size_t pcmi_voxelize_workspace_bytes(int64_t n);
int pcmi_voxelize(const double* xyz, int64_t n, double voxel_size, int32_t* first_index, int32_t* coords,
                  int64_t* n_unique_host, void* ws, size_t ws_bytes, pcmi_stream_t stream);
size_t pcmi_match_radius_workspace_bytes(int64_t n0, int64_t n1);
int pcmi_match_radius(const double* src, int64_t n0, const double* rigid3x4_host, const double* dst, int64_t n1,
                      double radius, int32_t* pairs, int64_t pairs_capacity, int64_t* n_pairs_host, void* ws,
                      size_t ws_bytes, pcmi_stream_t stream);

/* ---- pre-training pair corpus (csrc/corpus.hip) -----------------------------------------------------------------
 * The geometric part of the reference's offline preprocessing ("dp/" = pretrain/data_preprocess/scannet_pair/ of the
 * reference), one scene of F frames at a time.  Each call syncs (it returns counts or checks ranges);
 * pcmi_corpus_overlap_counts enqueues its count kernel after its range check, so counts are ready in stream order.
 * Rows of a frame are contiguous: offsets [F+1] (device) / offsets_host [F+1] delimit them.
 * pcmi_corpus_backproject = dp/point_cloud_extractor.py:43-75: depth uint16 [F, H, W] (millimetres), poses fp64
 *   [F, 4, 4] camera-to-world, intrinsic_host = the 4x4 intrinsic_depth.txt row-major (fx, fy, cx, cy, bx, by read
 *   from it as the reference does).  Pixels with depth 0 are dropped; the rest keep row-major pixel order:
 *   d = depth / depth_shift, X = ((u - cx) d) / fx + bx, Y = ((v - cy) d) / fy + by, Z = d,
 *   w_r = ((X P[r,0] + Y P[r,1]) + Z P[r,2]) + P[r,3], every operation rounded on its own (no FMA).
 *   points: fp64 [F*H*W, 3] capacity; nan_count [F] = points of the frame with a NaN coordinate.
 * pcmi_corpus_voxel_centroids = open3d voxel_down_sample (dp/compute_full_overlapping.py:15-26) of every frame:
 *   origin = per-frame min bound - voxel/2, voxel = floor((p - origin) / voxel_size); centroid = sequential sum of the
 *   voxel's points in ascending order / count; rows ordered by first occurrence.  centroids: fp64 [n, 3] capacity,
 *   voxel_offsets / voxel_offsets_host [F+1] delimit the frames' centroids.  At most 2^29 points.
 * pcmi_corpus_overlap_counts = the ordered-pair query loop of dp/compute_full_overlapping.py:63-73 for all pairs at
 *   once: counts [F, F] int32 (device, row-major, written whole), counts[i*F + j] = #{q in frame j : some p in frame i
 *   with ((ex ex + ey ey) + ez ez) <= radius^2, e = q - p} (pcmi_match_radius's test) for i != j; the diagonal is 0.
 * PCMI_ERR_RANGE: a point outside +-2^20 cells (voxels of its frame, or radius-sized cells of the overlap grid).
 * pcmi_corpus_backproject_color = a colour for every row of pcmi_corpus_backproject (the reference exports the colour
 *   frames, reader.py --export_color_images, but its preprocessing never reads them): the same depth stack, depth
 *   intrinsic and depth_shift, with color_images uint8 [F, Hc, Wc, 3] (DEVICE), color_intrinsic_host = the 4x4
 *   intrinsic_color.txt (fxc = Kc[0,0], fyc = Kc[1,1], cxc = Kc[0,2], cyc = Kc[1,2]) and depth_to_color_host = M, the
 *   4x4 inv(extrinsic_color) extrinsic_depth (HOST, row-major; rows 0..2 are read).  Per pixel with depth != 0, fp64,
 *   every operation rounded on its own (no FMA):
 *     d, X, Y, Z = d as above (camera space, no pose);  q_r = ((X M[r,0] + Y M[r,1]) + Z M[r,2]) + M[r,3], r = 0, 1, 2;
 *     uc = (fxc q0) / q2 + cxc, vc = (fyc q1) / q2 + cyc;  px = floor(uc + 0.5), py = floor(vc + 0.5);
 *   the point takes color_images[f, py, px, :] if q2 > 0, uc and vc are finite, 0 <= px < Wc and 0 <= py < Hc (tested
 *   on the doubles, before any conversion to an integer); otherwise it is (0, 0, 0) and adds 1 to uncolored[f].
 *   color: uint8 [F*H*W, 3] capacity, row k = the colour of row k of pcmi_corpus_backproject's points (zero-depth pixels
 *   dropped, the rest row-major, frame after frame); uncolored int64 [F] (DEVICE, integer atomics: the same bits from
 *   run to run); offsets [F+1] (DEVICE) equal pcmi_corpus_backproject's.  offsets_host [F+1] may be NULL: then the
 *   call does not wait for the stream at all; given, it is filled after the one wait pcmi_corpus_backproject has too.
 *   F*H*W < 2^31, Hc, Wc >= 1, F*Hc*Wc < 2^40.  ws: pcmi_corpus_backproject_color_workspace_bytes(F, H, W). */
size_t pcmi_corpus_backproject_workspace_bytes(int64_t n_frames, int64_t height, int64_t width);
int pcmi_corpus_backproject(const uint16_t* depth, int64_t n_frames, int64_t height, int64_t width,
                            const double* intrinsic_host, const double* poses, double depth_shift, double* points,
                            int64_t* offsets, int32_t* nan_count, int64_t* offsets_host, void* ws, size_t ws_bytes,
                            pcmi_stream_t stream);
size_t pcmi_corpus_backproject_color_workspace_bytes(int64_t n_frames, int64_t height, int64_t width);
int pcmi_corpus_backproject_color(const uint16_t* depth, int64_t n_frames, int64_t height, int64_t width,
                                  const double* intrinsic_host, double depth_shift, const uint8_t* color_images,
                                  int64_t color_height, int64_t color_width, const double* color_intrinsic_host,
                                  const double* depth_to_color_host, uint8_t* color, int64_t* uncolored, int64_t* offsets,
                                  int64_t* offsets_host, void* ws, size_t ws_bytes, pcmi_stream_t stream);
size_t pcmi_corpus_voxel_centroids_workspace_bytes(int64_t n_points, int64_t n_frames);
int pcmi_corpus_voxel_centroids(const double* points, const int64_t* offsets, const int64_t* offsets_host,
                                int64_t n_frames, double voxel_size, double* centroids, int64_t* voxel_offsets,
                                int64_t* voxel_offsets_host, void* ws, size_t ws_bytes, pcmi_stream_t stream);
size_t pcmi_corpus_overlap_workspace_bytes(int64_t n_points, int64_t n_frames);
int pcmi_corpus_overlap_counts(const double* centroids, const int64_t* offsets, const int64_t* offsets_host,
                               int64_t n_frames, double radius, int32_t* counts, void* ws, size_t ws_bytes,
                               pcmi_stream_t stream);

/* ---- virtual views of a whole scan (csrc/views.hip) ---------------------------------------------------------------
 * No counterpart in the reference: which points of a scan F pinhole cameras would see (frustum plus z-buffer occlusion),
 * the stage in front of pcmi_corpus_voxel_centroids for a corpus built from reconstructions instead of depth frames.
 * points fp64 [n, 3] world frame, row stride points_ld >= 3 doubles; w2c fp64 [F, 4, 4] world-to-camera (DEVICE; rows
 * 0..2 are read; the caller inverts the poses); the camera is fx, fy, cx, cy with an image of height x width pixels.
 * Per (view f, point i), M = w2c[f], fp64, every operation rounded on its own (no FMA), IEEE division:
 *   X = ((x M00 + y M01) + z M02) + M03, Y and Z likewise from rows 1 and 2;
 *   projectable iff X, Y, Z are finite and z_near <= Z <= z_far;
 *   u = (X fx) / Z + cx, v = (Y fy) / Z + cy, px = floor(u + 0.5), py = floor(v + 0.5), zf = (float)Z.
 * pcmi_views_zbuffer: zbuf float32 [F, H, W] (written whole, +inf where a pixel is empty) = the minimum zf over the
 *   projectable points whose window of splat x splat pixels (odd, 1 ... 7) centred on (px, py), clipped at the image's
 *   borders, covers the pixel.  A 32-bit integer atomic minimum on the bit pattern of the positive float: no float
 *   atomics, the same bits whatever the order of execution.  No synchronisation.
 * pcmi_views_visible: point i is visible in view f iff it is projectable, 0 <= px < W and 0 <= py < H (tested on the
 *   doubles) and (double)zf <= (double)zbuf[f, py, px] * (1.0 + rel_tol) -- the float32-rounded depth on both sides, so
 *   that with rel_tol = 0 the point that set a pixel's minimum sees itself.  nw = ceil(n / 64):
 *     mask uint64 [F, nw]: bit l of mask[f, w] = point 64 w + l is visible in f (bits past n are 0);
 *     word_start int64 [F, nw]: the exclusive prefix sum of the words' popcounts in (f, w) order = the row of
 *       pcmi_views_rows' output where the points of word (f, w) begin;
 *     offsets int64 [F + 1] (device) and offsets_host [F + 1]: offsets[f] = word_start[f, 0], offsets[F] = all rows;
 *     pixels int64 [F]: the pixels of zbuf[f] that hold a depth (integer atomics: the same from run to run).
 *   One synchronisation, behind the copy of offsets to the host.  ws: pcmi_views_visible_workspace_bytes(n, F).
 * pcmi_views_rows: rows int32 [offsets[F]] = the visible points of every view, ascending inside a view, views in
 *   order, from mask and word_start as pcmi_views_visible left them.  No synchronisation.
 * n = 0 or F = 0: success with empty outputs (offsets all 0).  PCMI_ERR_RANGE: splat even or outside 1 ... 7, H or W < 1,
 *   n >= 2^31, F > 4096, F H W >= 2^31, F ceil(n / 64) >= 2^31.  PCMI_ERR_INVALID: a camera with a non-finite entry,
 *   fx or fy <= 0, not 0 < z_near <= z_far < inf, rel_tol negative or not finite, points_ld < 3, a null pointer. */
int pcmi_views_zbuffer(const double* points, int64_t points_ld, int64_t n, const double* w2c, int64_t n_views, double fx,
                       double fy, double cx, double cy, int64_t height, int64_t width, double z_near, double z_far,
                       int splat, float* zbuf, pcmi_stream_t stream);
size_t pcmi_views_visible_workspace_bytes(int64_t n, int64_t n_views);
int pcmi_views_visible(const double* points, int64_t points_ld, int64_t n, const double* w2c, int64_t n_views, double fx,
                       double fy, double cx, double cy, int64_t height, int64_t width, double z_near, double z_far,
                       double rel_tol, const float* zbuf, uint64_t* mask, int64_t* word_start, int64_t* offsets,
                       int64_t* offsets_host, int64_t* pixels, void* ws, size_t ws_bytes, pcmi_stream_t stream);
int pcmi_views_rows(const uint64_t* mask, const int64_t* word_start, int64_t n, int64_t n_views, int32_t* rows,
                    pcmi_stream_t stream);

/* ---- PointNet++ point-set ops (csrc/pointset.hip) -----------------------------------------------------------------
 * What the reference's detection fine-tuning ("vn/" = downstream/votenet_det_new/ of the reference) reaches through its
 * one native extension, vn/models/backbone/pointnet2/pointnet2_utils.py.  fp32 data, int32 indices; feature tensors are
 * channel-first and contiguous, as the reference's: [B, C, N].  A "cloud" is one batch element.  Every squared distance is
 * ((dx dx) + (dy dy)) + (dz dz), each operation rounded on its own, so index outputs are reproducible in float32 on the
 * host (tests/pointset_ref.py).  No float atomics: every result is reproducible bit for bit.  A refused call enqueues nothing.
 *
 * pcmi_fps = furthest_point_sample (pointnet2_utils.py:51-80; called per scene at vn/models/backbone_module.py:166-169 and
 *   from the set-abstraction modules).  Clouds: dense -- offs == NULL, rows == NULL, cloud i = xyz[i * max_cloud ..), and
 *   n_points == n_clouds * max_cloud -- or segments of xyz [n_points, 3]: offs [n_clouds + 1] (device), point p of cloud i
 *   is xyz[rows[offs[i] + p]], or xyz[offs[i] + p] with rows == NULL (pcmi_segments_t's rows / offs); max_cloud is then an
 *   upper bound of any cloud's size known to the host (n_points if nothing better is): it only selects which size tiers are
 *   launched, and no host synchronisation is needed.  One launch covers the whole batch (one workgroup per cloud).
 *   Semantics: the running minimum of every point starts at 1e10; pick 0 is point 0; for each later pick every point with
 *   x^2 + y^2 + z^2 > 1e-3 (the reference's padding convention; others are never updated nor chosen) lowers its minimum by
 *   its squared distance to the previous pick, and the pick is the point with the largest minimum, the LOWEST index among
 *   equals (the reference's tie order depends on its block size), index 0 if no point qualifies.  m > n repeats picks.
 *   out [n_clouds, m]: positions within the cloud, -1 for an empty cloud (or one beyond max_cloud or n_points);
 *   out_rows (nullable, [n_clouds, m]): the same picks as rows of xyz (rows[offs[i] + pick] / offs[i] + pick), -1 likewise.
 *   ws: pcmi_fps_workspace_bytes(n_points, max_cloud, rows != NULL) -- a compacted copy of the coordinates when there is a
 *   row list, and the running minima when max_cloud > 8192 (smaller clouds keep coordinates and minima in registers);
 *   0 bytes (ws may be NULL) for a dense batch of at most 8192 points per cloud.
 * pcmi_ball_query = ball_query (pointnet2_utils.py:260-291; vn/models/proposal_module.py:93 through QueryAndGroup):
 *   idx [B, np, nsample] = the first nsample points of xyz [B, n, 3], in ascending index, with d^2 < radius * radius (the
 *   product in fp32) of centre new_xyz [B, np, 3]; unfilled slots repeat the first hit, no hit: zeros.  No workspace.
 * pcmi_three_nn = three_nn (pointnet2_utils.py:120-149; the feature-propagation modules): for every unknown [B, n, 3] the
 *   three nearest of known [B, m, 3], scanning in ascending index with strict <, so the lower index wins a tie; dist2
 *   [B, n, 3] holds SQUARED distances (the caller takes the root, as the reference's Python does), idx [B, n, 3].
 *   m < 3: PCMI_ERR_INVALID.  No workspace.
 * Gathers, forward (gather_operation :83-117, grouping_operation :209-257, three_interpolate :152-206):
 *   gather_points   out [B, C, m]      = feat [B, C, N] at idx [B, m]
 *   group_points    out [B, C, np, ns] = feat [B, C, N] at idx [B, np, ns]
 *   three_interpolate out [B, C, n]    = (w0 f0 + w1 f1) + w2 f2, f_k = feat [B, C, M] at idx [B, n, 3], weight [B, n, 3]
 * and backward: gfeat [B, C, N] (resp. M), written whole, = the scatter-add of gout over idx, computed in gather form --
 *   inverse lists from an integer count, a scan and a stable radix placement by flat source position, every target summed in
 *   ascending source position (the reference uses float atomics) -- ws: pcmi_pointset_scatter_workspace_bytes(number of
 *   indices = B m / B np ns / 3 B n, number of targets = B N / B M).
 * validate != 0: the indices are checked on the device first and the call SYNCS; an index outside [0, N) returns
 *   PCMI_ERR_RANGE with nothing else launched.  validate == 0 (indices this library produced, or a backward pass whose
 *   forward validated them): no synchronisation; an index outside the range is still never dereferenced -- it reads as 0 in
 *   the forward passes and is dropped by the backward ones. */
size_t pcmi_fps_workspace_bytes(int64_t n_points, int64_t max_cloud, int with_rows);
int pcmi_fps(const float* xyz, int64_t n_points, const int32_t* rows, const int32_t* offs, int64_t n_clouds,
             int64_t max_cloud, int64_t m, int32_t* out, int32_t* out_rows, void* ws, size_t ws_bytes,
             pcmi_stream_t stream);
int pcmi_ball_query(const float* xyz, const float* new_xyz, int64_t B, int64_t n, int64_t np, float radius, int nsample,
                    int32_t* idx, pcmi_stream_t stream);
int pcmi_three_nn(const float* unknown, const float* known, int64_t B, int64_t n, int64_t m, float* dist2, int32_t* idx,
                  pcmi_stream_t stream);
size_t pcmi_pointset_scatter_workspace_bytes(int64_t n_idx, int64_t n_targets);
int pcmi_gather_points_fwd(const float* feat, const int32_t* idx, int64_t B, int C, int64_t N, int64_t m, float* out,
                           int validate, pcmi_stream_t stream);
int pcmi_gather_points_bwd(const float* gout, const int32_t* idx, int64_t B, int C, int64_t N, int64_t m, float* gfeat,
                           int validate, void* ws, size_t ws_bytes, pcmi_stream_t stream);
int pcmi_group_points_fwd(const float* feat, const int32_t* idx, int64_t B, int C, int64_t N, int64_t np, int64_t ns,
                          float* out, int validate, pcmi_stream_t stream);
int pcmi_group_points_bwd(const float* gout, const int32_t* idx, int64_t B, int C, int64_t N, int64_t np, int64_t ns,
                          float* gfeat, int validate, void* ws, size_t ws_bytes, pcmi_stream_t stream);
int pcmi_three_interpolate_fwd(const float* feat, const int32_t* idx, const float* weight, int64_t B, int C, int64_t M,
                               int64_t n, float* out, int validate, pcmi_stream_t stream);
int pcmi_three_interpolate_bwd(const float* gout, const int32_t* idx, const float* weight, int64_t B, int C, int64_t M,
                               int64_t n, float* gfeat, int validate, void* ws, size_t ws_bytes, pcmi_stream_t stream);

/* ---- VoteNet head on row-major activations (csrc/votehead.hip) ---------------------------------------------------------
 * What turns the backbone's seed features into votes and proposals ("vn/" as above: vn/models/voting_module.py,
 * vn/models/proposal_module.py with PointnetSAModuleVotes, vn/models/votenet.py:120-121) and the optimiser step of
 * vn/lib/train.py.  Every activation is fp32 [rows, ld] with the FEATURE columns first, the geometric columns behind them
 * and zero columns up to ld (a multiple of 4; the dense GEMM wants a multiple of 32), so the 1x1 convolution
 * (pcmi_spconv_* with map == NULL) and pcmi_bn_* work on them as they are, with no transposes.  Tensors are contiguous
 * fp32 / int32 apart from the leading dimensions given.  A refused call enqueues nothing.  No float atomics: every result is
 * the same bits from run to run.  Workspace sizes come from the *_workspace_bytes query.
 *
 * pcmi_group_rows_fwd = QueryAndGroup(use_xyz, normalize_xyz) (pointnet2_utils.py:294-351) written straight into rows:
 *   xyz [B, n, 3], centre [B, np, 3], feat [B n, C] (feat_ld), idx [B, np, ns] from pcmi_ball_query;
 *   out [B np ns, out_ld]: out[r, 0:C] = feat[b n + idx[r]], out[r, C + k] = (xyz[b, idx[r], k] - centre[b, q, k]) /
 *   radius_div -- a subtraction, then a division, each rounded on its own (radius_div 1.0: no normalisation) -- and zeros
 *   up to out_ld.  out_ld >= C + 3 and a multiple of 4, out 16-byte aligned, else PCMI_ERR_INVALID.  One wave copies one
 *   row: 16-byte accesses where C % 4 == 0 (and feat is 16-byte aligned with feat_ld % 4 == 0), 4-byte accesses otherwise.
 *   An index outside [0, n) is never dereferenced: its whole row is zero.  validate as for the point-set gathers above
 *   (!= 0: checked on the device first, the call SYNCS, PCMI_ERR_RANGE with nothing else launched).
 * pcmi_group_rows_bwd: gout [B np ns, gout_ld] -> gfeat [B n, C] (gfeat_ld), gxyz [B, n, 3], gcentre [B, np, 3], each
 *   written whole.  gfeat / gxyz: every point sums the rows that gathered it in ascending row, in gather form over the
 *   inverse lists of csrc/pointset.hip (ws: pcmi_group_rows_bwd_workspace_bytes); gcentre = minus the ascending sum over
 *   the group's ns rows; the geometric gradients are divided by radius_div element by element before they are summed.
 *   A row whose index is outside [0, n) is dropped from all three.  No synchronisation.
 * pcmi_rows_maxpool_fwd: out [R, C] (out_ld) = the maximum over the ns consecutive rows of x [R ns, C] (x_ld), arg [R, C]
 *   uint8 (contiguous) = the row within the window that holds it.  The LOWEST row wins among equal values (ball-query
 *   padding repeats rows and ReLU leaves all-zero columns: ties are the common case); a NaN in the window is the result
 *   and the lowest NaN row the argument.  1 <= ns <= 256, else PCMI_ERR_UNSUPPORTED.
 * pcmi_rows_maxpool_bwd: gx [R ns, C] (gx_ld), written whole: gout [R, C] at the argument row, zero elsewhere.
 * pcmi_vote_fwd = the tail of VotingModule.forward (voting_module.py:52-66) and the feature normalisation of
 *   votenet.py:120-121 in one pass.  net [R, vf Wb] (net_ld): block v of a row holds C residual features, then 3 offsets
 *   (Wb >= C + 3, a multiple of 4; the head uses C + 3 rounded up to 32).  vote_xyz [R vf, 3] = seed_xyz [R, 3] + offset,
 *   vote_feat [R vf, C] (vote_feat_ld) = u / ||u||_2 with u = seed_feat [R, C] (seed_feat_ld) + residual, norm [R vf] =
 *   ||u||_2.  No epsilon, as in the reference: a zero row gives the reference's NaN and is not trapped.  The norm is
 *   reduced in a fixed order (per lane in ascending column, then an xor butterfly over the wave).
 * pcmi_vote_bwd: gu = (gy - y (y . gy)) / ||u|| with y = vote_feat, gy = g_vote_feat; g_net [R, vf Wb] (g_net_ld) = gu,
 *   then g_vote_xyz, then zeros in every block; g_seed_feat [R, C] and g_seed_xyz [R, 3] = the sums over v in ascending v.
 * pcmi_adam_step = torch.optim.Adam's single-tensor step (amsgrad off, L2 weight decay) on flat buffers, step number t >= 1:
 *   g' = g + wd w; m = b1 m + (1 - b1) g'; v = b2 v + (1 - b2) g'^2; denom = sqrt(v) / sqrt(1 - b2^t) + eps;
 *   w -= (lr / (1 - b1^t)) (m / denom).  The bias corrections are computed in double on the host, as torch does; g is not
 *   modified.  16-byte accesses when all four buffers are 16-byte aligned. */
int pcmi_group_rows_fwd(const float* xyz, const float* centre, const float* feat, int64_t feat_ld, const int32_t* idx,
                        int64_t B, int64_t n, int64_t np, int64_t ns, int C, float radius_div, float* out, int64_t out_ld,
                        int validate, pcmi_stream_t stream);
size_t pcmi_group_rows_bwd_workspace_bytes(int64_t B, int64_t n, int64_t np, int64_t ns);
int pcmi_group_rows_bwd(const float* gout, int64_t gout_ld, const int32_t* idx, int64_t B, int64_t n, int64_t np, int64_t ns,
                        int C, float radius_div, float* gfeat, int64_t gfeat_ld, float* gxyz, float* gcentre, void* ws,
                        size_t ws_bytes, pcmi_stream_t stream);
int pcmi_rows_maxpool_fwd(const float* x, int64_t x_ld, int64_t R, int ns, int C, float* out, int64_t out_ld, uint8_t* arg,
                          pcmi_stream_t stream);
int pcmi_rows_maxpool_bwd(const float* gout, int64_t gout_ld, const uint8_t* arg, int64_t R, int ns, int C, float* gx,
                          int64_t gx_ld, pcmi_stream_t stream);
int pcmi_vote_fwd(const float* net, int64_t net_ld, const float* seed_xyz, const float* seed_feat, int64_t seed_feat_ld,
                  int64_t R, int vf, int C, int Wb, float* vote_xyz, float* vote_feat, int64_t vote_feat_ld, float* norm,
                  pcmi_stream_t stream);
int pcmi_vote_bwd(const float* g_vote_feat, int64_t g_vote_feat_ld, const float* g_vote_xyz, const float* vote_feat,
                  int64_t vote_feat_ld, const float* norm, int64_t R, int vf, int C, int Wb, float* g_net, int64_t g_net_ld,
                  float* g_seed_feat, int64_t g_seed_feat_ld, float* g_seed_xyz, pcmi_stream_t stream);
int pcmi_adam_step(float* w, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                   float weight_decay, int64_t t, pcmi_stream_t stream);

/* ---- PointNet++ backbone on rows (csrc/rowspool.hip) -------------------------------------------------------------------
 * The two row kernels that vn/models/backbone_module.py's Pointnet2Backbone needs beyond the head's: the last SharedMLP
 * layer's BatchNorm + ReLU fused with the max over nsample behind it (pointnet2_modules.py:251-257), and
 * PointnetFPModule's three_interpolate + concatenation written straight into rows (:394-409).  Layout and conventions as
 * for the head above; no float atomics, every result is the same bits from run to run; a refused call enqueues nothing.
 *
 * pcmi_bn_maxpool_fwd_train: x [R ns, C] (x_ld) -> out [R, C] (out_ld), arg [R, C] uint8 (contiguous), save_mean and
 *   save_invstd [C].  Batch statistics over all n = R ns rows with pcmi_bn_fwd_train's conventions (biased variance for the
 *   normalisation, unbiased for the running estimate -- the biased one when n == 1 --, running = (1 - momentum) running +
 *   momentum batch; running_mean / running_var both NULL: no update), from fp64 (sum x, sum x^2) partials per row chunk
 *   merged in a fixed order.  Then ONE pass computes y = relu((x - mean) * (invstd * gamma) + beta) per element, each
 *   operation rounded on its own, and writes the maximum over every ns consecutive rows and the row that holds it; y is
 *   never stored.  The decision rule is pcmi_rows_maxpool_fwd's on y: rows in ascending order, strict >, so the LOWEST row
 *   wins among equals and a column that is <= 0 in the whole window gives (0, row 0); a NaN y is the result and the lowest
 *   NaN row the argument.  The maximum is over y, not x: a negative gamma reverses the order.
 *   1 <= ns <= 256, else PCMI_ERR_UNSUPPORTED; ws of pcmi_bn_maxpool_workspace_bytes(R, ns, C), else PCMI_ERR_WORKSPACE.
 *   16-byte accesses when C % 4 == 0, the leading dimensions are multiples of 4 and x / out are 16-byte aligned (arg 4-byte
 *   aligned), 4-byte accesses otherwise.
 * pcmi_bn_maxpool_fwd_eval: the same pass on the running estimates, invstd = 1 / sqrt(running_var + eps); arg may be NULL;
 *   no workspace.
 * pcmi_bn_maxpool_bwd: gout [R, C], x, out, arg, gamma, save_mean, save_invstd -> dx [R ns, C] (dx_ld) written whole,
 *   dgamma, dbeta [C].  g(r, c) = gout where out > 0, else 0, and sits at row r ns + arg; xhat = (x - mean) * invstd;
 *   dbeta = sum_r g, dgamma = sum_r g xhat at that row (fp64 partials over the R pooled rows, fixed order),
 *   dx_i = (gamma invstd) ((g_i - dbeta / n) - xhat_i dgamma / n).  An arg outside [0, ns) is read as 0.
 * pcmi_interp_rows_fwd: known [B m, C2] (known_ld), idx int32 / weight fp32 [B, n, 3], skip [B n, C1] (skip_ld; NULL with
 *   C1 == 0) -> out [B n, out_ld]: out[b n + i, 0:C2] = ((w0 f0) + (w1 f1)) + (w2 f2) with f_k = known[b m + idx_k], every
 *   operation rounded on its own; columns C2 .. C2 + C1 a copy of skip; zeros up to out_ld >= C2 + C1.  One wave per row.
 *   validate != 0: the indices are checked on the device first, the call SYNCS, PCMI_ERR_RANGE with nothing else launched;
 *   validate == 0: an index outside [0, m) is never dereferenced and reads as 0.
 * pcmi_interp_rows_bwd: gout [B n, >= C2] (gout_ld) -> gknown [B m, C2] (gknown_ld), written whole: every known point sums
 *   weight * gout over the (row, k) slots that named it, in ascending slot, in gather form over the inverse lists of
 *   csrc/pointset.hip (ws: pcmi_interp_rows_bwd_workspace_bytes); an index outside [0, m) is dropped.  The gradient of skip
 *   is the view gout[:, C2:C2 + C1].  No synchronisation. */
size_t pcmi_bn_maxpool_workspace_bytes(int64_t R, int ns, int c);
int pcmi_bn_maxpool_fwd_train(const float* x, int64_t x_ld, int64_t R, int ns, int C, const float* gamma, const float* beta,
                              float* running_mean, float* running_var, float momentum, float eps, float* out, int64_t out_ld,
                              uint8_t* arg, float* save_mean, float* save_invstd, void* ws, size_t ws_bytes, pcmi_stream_t stream);
int pcmi_bn_maxpool_fwd_eval(const float* x, int64_t x_ld, int64_t R, int ns, int C, const float* gamma, const float* beta,
                             const float* running_mean, const float* running_var, float eps, float* out, int64_t out_ld,
                             uint8_t* arg, pcmi_stream_t stream);
int pcmi_bn_maxpool_bwd(const float* gout, int64_t gout_ld, const float* x, int64_t x_ld, const float* out, int64_t out_ld,
                        const uint8_t* arg, int64_t R, int ns, int C, const float* gamma, const float* save_mean,
                        const float* save_invstd, float* dx, int64_t dx_ld, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                        pcmi_stream_t stream);
int pcmi_interp_rows_fwd(const float* known, int64_t known_ld, const int32_t* idx, const float* weight, const float* skip,
                         int64_t skip_ld, int64_t B, int64_t m, int64_t n, int C2, int C1, float* out, int64_t out_ld, int validate,
                         pcmi_stream_t stream);
size_t pcmi_interp_rows_bwd_workspace_bytes(int64_t B, int64_t m, int64_t n);
int pcmi_interp_rows_bwd(const float* gout, int64_t gout_ld, const int32_t* idx, const float* weight, int64_t B, int64_t m,
                         int64_t n, int C2, float* gknown, int64_t gknown_ld, void* ws, size_t ws_bytes, pcmi_stream_t stream);

/* ---- VoteNet detection head (csrc/detect.hip) ------------------------------------------------------------------------
 * The matching of the detection loss and the decoding of the predictions ("vn/" as above).  fp32 data, int32 indices,
 * contiguous tensors.  Every operation of a distance is rounded on its own in fp32, in the order written here, so the
 * argmins are reproducible in float32 on the host (tests/votenet_ref.py).  No float atomics: every result is reproducible
 * bit for bit.  A refused call enqueues nothing.
 *
 * pcmi_nn_distance_fwd = one direction of nn_distance (vn/lib/utils/nn_distance.py:34-61; called at
 *   vn/models/loss_helper.py:59 -- votes against ground-truth votes, B num_seed batches of vote_factor x 3 points --, :84
 *   and :133): dist [B, N] / idx [B, N] = min / argmin over the M points b [B, M, 3] of the distance to a [B, N, 3], without
 *   the [B, N, M] tensor the reference materialises (the other direction is the same call with a and b swapped).
 *   mode 0: ((dx dx) + (dy dy)) + (dz dz); 1: (|dx| + |dy|) + |dz|; 2 (l1smooth): (h(dx) + h(dy)) + h(dz),
 *   h(x) = 0.5 (q q) + delta (|x| - q), q = min(|x|, delta).  The LOWEST index wins a tie (torch.min's tie order depends
 *   on its backend).  N, M >= 1.  One launch for any B: rows of the flat [B N] list per thread while M <= 32 (thousands of
 *   tiny batches, several per wave), else a workgroup per 256 rows with b streamed through LDS.  No workspace.
 * pcmi_nn_distance_bwd: gpc1 [B, N, 3] and gpc2 [B, M, 3] (written whole) from gdist1 [B, N] and gdist2 [B, M] -- what
 *   autograd derives from the two torch.min of :59-60: every distance routes its gradient to its argmin pair, with
 *   d'(x) = 2 x / sign(x) (0 at 0) / clamp(x, -delta, delta) per component.  idx1 [B, N] indexes pc2, idx2 [B, M] indexes
 *   pc1 (the forward's outputs).  A point's gradient is its own term plus the terms of every point of the other cloud whose
 *   nearest neighbour it is, added in ascending index of the other cloud (gather form): a direct scan of the other cloud's
 *   indices up to 1024 points, the inverse lists of the point-set ops beyond.  An index outside its cloud is never
 *   dereferenced: its term is dropped from both gradients, in every form (no error code, no synchronisation).  ws: pcmi_nn_distance_bwd_workspace_bytes(B, N, M) -- 0 (ws may be NULL) while both clouds have at most
 *   1024 points.
 * pcmi_box_decode = the decoding loop of parse_predictions (vn/models/ap_helper.py:57-83, :102-103: B K calls of
 *   class2angle / class2size / get_3d_box with a .cpu() each): one thread per proposal of center [B, K, 3], heading_scores /
 *   heading_residuals [B, K, H], size_scores [B, K, S], size_residuals [B, K, S, 3], sem_cls_scores [B, K, Cls],
 *   objectness_scores [B, K, 2], mean_size_arr [S, 3].  heading_class / size_class / sem_cls [B, K]: argmax, the lowest index
 *   of equal scores as torch.argmax.  box_params [B, K, 7]: the centre in upright-camera coordinates (x, -z, y), the size
 *   (l, w, h) = mean_size_arr[size_class] + residual, the heading angle = class 2 pi / H + residual, minus 2 pi if above pi
 *   (vn/lib/datasets/sunrgbd/model_util_sunrgbd.py:67-75), 0 with zero_heading != 0 (the axis-aligned boxes of
 *   vn/lib/datasets/scannet/model_util_scannet.py:45-49).  corners [B, K, 8, 3] in get_3d_box's order
 *   (vn/lib/utils/box_util.py:210-225), minmax [B, K, 6] = (min x, y, z, max x, y, z) over the corners, obj_prob [B, K] =
 *   softmax(objectness)[1], sem_cls_probs [B, K, Cls] = softmax(sem_cls_scores).
 * pcmi_box_point_counts = the remove_empty_box loop (ap_helper.py:88-99: B K Delaunay triangulations with find_simplex over
 *   every point of the scene): counts [B, K] (int32, written whole) = points of points [B, N, point_ld >= 3] (upright-depth
 *   x, y, z in the first three columns) inside box_params' boxes -- rotated into the box's frame, every |coordinate| <= half
 *   the size, faces included (the triangulation's answer on a face depends on its tolerance).  Integer atomics only.
 * pcmi_box_nms = nms_2d_faster / nms_3d_faster / nms_3d_faster_samecls (vn/lib/utils/nms.py:44-155; ap_helper.py:104-162),
 *   mode 0 / 1 / 2, one workgroup per scene: the boxes with counts >= min_points (counts == NULL: all) are ranked by
 *   obj_prob descending, equal scores by ascending index (numpy's argsort leaves ties unspecified); in rank order a box
 *   that is still alive is kept and clears every later box it suppresses: overlap o > nms_iou in fp32 (a NaN overlap
 *   suppresses nothing), o = inter / (area_i + area_j - inter), or inter / area_j with old_type != 0, on minmax's camera
 *   x / z rectangle (mode 0) or the whole box (1, 2), in mode 2 only between boxes of the same sem_cls (nullable otherwise).
 *   pred_mask [B, K] (int32, written whole): 1 for a kept box.  K <= 1024 (the K x K suppression bits live in LDS, 128 KiB
 *   at 1024): PCMI_ERR_UNSUPPORTED beyond. */
int pcmi_nn_distance_fwd(const float* a, const float* b, int64_t B, int64_t N, int64_t M, int mode, float delta,
                         float* dist, int32_t* idx, pcmi_stream_t stream);
size_t pcmi_nn_distance_bwd_workspace_bytes(int64_t B, int64_t N, int64_t M);
int pcmi_nn_distance_bwd(const float* pc1, const float* pc2, const int32_t* idx1, const int32_t* idx2,
                         const float* gdist1, const float* gdist2, int64_t B, int64_t N, int64_t M, int mode,
                         float delta, float* gpc1, float* gpc2, void* ws, size_t ws_bytes, pcmi_stream_t stream);
int pcmi_box_decode(const float* center, const float* heading_scores, const float* heading_residuals,
                    const float* size_scores, const float* size_residuals, const float* sem_cls_scores,
                    const float* objectness_scores, const float* mean_size_arr, int64_t B, int64_t K, int H, int S,
                    int Cls, int zero_heading, int32_t* heading_class, int32_t* size_class, int32_t* sem_cls,
                    float* box_params, float* corners, float* minmax, float* obj_prob, float* sem_cls_probs,
                    pcmi_stream_t stream);
int pcmi_box_point_counts(const float* points, int64_t point_ld, const float* box_params, int64_t B, int64_t N,
                          int64_t K, int32_t* counts, pcmi_stream_t stream);
int pcmi_box_nms(const float* minmax, const float* obj_prob, const int32_t* sem_cls, const int32_t* counts,
                 int min_points, int64_t B, int64_t K, int mode, int old_type, float nms_iou, int32_t* pred_mask,
                 pcmi_stream_t stream);

/* ---- detection scoring (csrc/evaldet.hip) ------------------------------------------------------------------------------
 * The last step of the detection evaluation loop (vn/lib/test.py:44,76-92): what APCalculator (vn/models/ap_helper.py:223-276)
 * computes through eval_det_multiprocessing / eval_det_cls / voc_ap (vn/lib/utils/eval_det.py) with get_iou_obb.  Overlaps
 * are fp32 (every operation rounded on its own, in the order of the reference's expressions), counts are integers, recall /
 * precision / AP are fp64 on those integers.  The only atomic is an integer minimum: every output is reproducible bit for
 * bit.  Contiguous tensors, everything on the caller's stream, no synchronisation.  A refused call enqueues nothing.
 *
 * pcmi_box3d_iou = box3d_iou (vn/lib/utils/box_util.py:92-117, called per box pair at eval_det.py:136): corners1 [n, 8, 3],
 *   corners2 [m, 8, 3] in get_3d_box's corner order (what pcmi_box_decode writes) -> iou3d [n, m] and, if not NULL, iou2d
 *   [n, m].  The bird's-eye-view rectangles are corners 3, 2, 1, 0 as (x, z); rect1 is clipped by the edges of rect2 with the
 *   reference's Sutherland-Hodgman walk (same vertex order, same strict inside test, same intersection formula) after both
 *   are moved so that corner 3 of box 1 is the origin (absolute coordinates would cancel in fp32); the area of the result is
 *   its shoelace sum (= the reference's hull area, the polygon being convex).  Vertical overlap max(0, min(c1[0].y, c2[0].y)
 *   - max(c1[4].y, c2[4].y)); volumes |c0 c1| |c1 c2| |c0 c4| (box3d_vol).  Rectangles that are disjoint or merely touch give
 *   exactly 0 (the reference's clipping returns None).  One thread per pair, the polygons (at most 8 vertices) in registers.
 * pcmi_det_match = the inner loop of eval_det_cls (eval_det.py:126-139) for a whole batch and every class at once: per
 *   scene, pred_corners [B, K, 8, 3] against gt_corners [B, G, 8, 3] with gt_cls [B, G] (int32) and gt_mask [B, G] (int32,
 *   0: no box; a class outside [0, Cls) is no box either).  best_iou [B, K, Cls] = the largest overlap of box k with the
 *   scene's boxes of class c, best_gt [B, K, Cls] (int32) = its index, the LOWEST among equal overlaps (the reference's strict
 *   >); -inf and -1 where the scene has no box of the class.  Neither the confidence order nor the threshold enters, so one
 *   match serves every threshold; entry [b, k, c] serves per_class_proposal (all Cls entries of a box) and the plain mode
 *   (entry sem_cls[b, k] only).  The [K, G] overlaps of a scene are computed once (tiles of 32 boxes in LDS) and reduced per
 *   class.  K <= 1024 (as pcmi_box_nms) and G <= 256: PCMI_ERR_UNSUPPORTED beyond; B <= 65535.
 * pcmi_det_ap = eval_det.py:142-159 and voc_ap (:24-55) for Cls classes and n_thresholds <= 16 thresholds from one match.
 *   The nd detections are listed class by class, in descending confidence within a class: class c holds the positions
 *   [cls_offs[c], cls_offs[c + 1]) (device int32 [Cls + 1]; positions outside every range are ignored).  best_iou [nd] and
 *   gt_id [nd] (int32: the detection's best box as an index into the n_gt ground-truth boxes of the whole evaluation, -1 for
 *   none) come from pcmi_det_match; npos [Cls] (device int32) counts the ground-truth boxes of a class.  thresholds is a HOST
 *   array.  Per threshold t: a detection with (double)best_iou > t bids its position for its box (integer atomic min); the
 *   winner is the true positive, every other detection a false positive.  Then inclusive counts, rec = tp / npos, prec =
 *   tp / max(tp + fp, 2^-52), the precision envelope (running maximum from the end) and ap = the sum over the detections
 *   where recall changes of (rec_i - rec_{i-1}) envelope_i, or with use_07_metric != 0 the 11-point form: sum over k = 0..10
 *   of (the largest prec where rec >= k * 0.1, else 0) / 11.  ap [T, Cls], last_rec [T, Cls] (rec of the class's last
 *   detection; 0 for a class without detections, whose ap is 0 too); a class without ground truth has rec = 0 / 0 = NaN and
 *   ap NaN (0 in the 11-point form), as the reference.  Optional (nullable) rec / prec (double) and tp_flag (int32), each
 *   [T, nd] in the list's order.  One workgroup per (class, threshold) walks its detections in blocks of 1024 with a carry, so
 *   a class may hold any number of them.  ws: pcmi_det_ap_workspace_bytes(nd, n_gt, n_thresholds). */
int pcmi_box3d_iou(const float* corners1, const float* corners2, int64_t n, int64_t m, float* iou3d, float* iou2d,
                   pcmi_stream_t stream);
int pcmi_det_match(const float* pred_corners, const float* gt_corners, const int32_t* gt_cls, const int32_t* gt_mask,
                   int64_t B, int64_t K, int64_t G, int Cls, int32_t* best_gt, float* best_iou, pcmi_stream_t stream);
size_t pcmi_det_ap_workspace_bytes(int64_t nd, int64_t n_gt, int n_thresholds);
int pcmi_det_ap(const float* best_iou, const int32_t* gt_id, const int32_t* cls_offs, const int32_t* npos, int64_t nd,
                int64_t n_gt, int Cls, const double* thresholds, int n_thresholds, int use_07_metric, double* ap,
                double* last_rec, double* rec, double* prec, int32_t* tp_flag, void* ws, size_t ws_bytes,
                pcmi_stream_t stream);

/* Softmax cross-entropy over the rows of logits [n, c] with an ignore label -- the loss of the downstream semantic
 * segmentation fine-tuning that reuses this backbone with out_channels = number of classes
 * (downstream/semseg/lib/train.py:64,124: nn.CrossEntropyLoss(ignore_index=config.ignore_label)).
 * out2[0] = mean loss over the counted rows, out2[1] = their number (device).  _bwd: dlogits = gloss[0] * dloss/dlogits.
 * A label that is neither in [0, c) nor the ignore label (torch raises for it) makes the loss and its row of dlogits
 * NaN -- a mis-mapped dataset label fails loudly instead of dropping points from the loss. */
size_t pcmi_softmax_ce_workspace_bytes(int64_t n);
int pcmi_softmax_ce_fwd(const float* logits, int64_t ld, int64_t n, int c, const int32_t* labels,
                        int ignore_label, float* out2, void* ws, size_t ws_bytes, pcmi_stream_t stream);
int pcmi_softmax_ce_bwd(const float* logits, int64_t ld, int64_t n, int c, const int32_t* labels,
                        int ignore_label, const float* out2, const float* gloss, float* dlogits,
                        int64_t d_ld, pcmi_stream_t stream);

/* ---- segmentation validation (csrc/segeval.hip) -----------------------------------------------------------------------
 * What the validation loop of the segmentation fine-tuning (downstream/semseg/lib/test.py:62-196) computes per batch on the
 * host, with nothing read back.  1 <= c <= 64 classes (the workgroup's private confusion matrix is 16 KB of LDS at 64):
 * PCMI_ERR_INVALID beyond; n < 2^31 - 256.  Everything on the caller's stream, no synchronisation; a refused call enqueues
 * nothing.  The only atomics are integer adds and every float64 sum has a fixed order: all outputs are reproducible bit for
 * bit.
 *
 * pcmi_seg_eval_rows = lib/test.py:119,137-140,143 with precision_at_one and fast_hist of lib/utils.py:117-133, one pass over
 *   logits [n, c] (fp32 rows with leading dimension ld >= c, so a column slice of a wider buffer) and labels [n] (int32):
 *   pred [n] (int32) = the arg-max of the row (get_prediction), the LOWEST class among equal logits.
 *   prob_t [c, n] (nullable) = softmax of the row, CLASS-major -- the layout the per-class sort reads contiguously.  exp and the
 *     quotient are fp32, the row's sum of exponentials is fp64 over the classes in ascending order: a row's probabilities
 *     depend on that row's logits only (equal rows give bit-equal probabilities, wherever they stand).
 *   hist [c, c] (int64) += the confusion matrix: a row counts iff 0 <= label < c, at hist[label, pred] (fast_hist).
 *   batch4 [4] (fp64) = sum of logsumexp(x) - x[label] over the counted rows (label != ignore_label), their number, the
 *     number of those with pred == label, and n.  A label that is neither a class nor ignore_label makes the sum NaN, as
 *     pcmi_softmax_ce_fwd.  Workgroup partials merged in workgroup order by the last workgroup to arrive.
 *   totals3 [3] (fp64, nullable) += n * sum / counted, n * (100 * correct / counted), n: the two AverageMeters of
 *     lib/test.py:138-139 (weighted by num_sample = n, ignored rows included) and their common count.  A batch without a
 *     counted row adds nothing to any of the three (the reference's meters would turn NaN for good).
 *   n == 0 enqueues nothing and leaves every output as it is.  ws: pcmi_seg_eval_rows_workspace_bytes(n), 8-byte aligned.
 * pcmi_seg_ap = average_precision(prob, target) of lib/test.py:55-59,144 (label_binarize + sklearn's
 *   average_precision_score(average=None)) for every class of one batch.  sorted_prob [c, n] (fp32) = every class's scores in
 *   descending order and order [c, n] (int64) = the row of each sorted element -- what torch.sort(prob_t, 1, descending=True)
 *   returns; labels [n] (int32).  For class k the positives are the rows with label == k; every other row, ignored and
 *   out-of-range labels included, is a negative (label_binarize gives it a zero row).  With tp = the positives among the
 *   first `rank` elements, at the LAST element of every run of equal scores: P = tp / rank, R = tp / npos, and
 *   ap [k] = sum (R - R_prev) P in fp64.  The order inside a run of equal scores does not matter (the sort need not be stable).
 *   A class without a positive row gets NaN (the reference's scikit-learn; np.nanmean(aps, 0) of lib/test.py:149 relies on
 *   it).  ap_sum [c] (fp64) += ap and ap_cnt [c] (int64) += 1 where ap is not NaN (both nullable): nanmean's numerator and
 *   denominator.  One workgroup per class walks its list in blocks of 4096 with a carry, so n may be anything; n == 0 gives
 *   NaN everywhere.  ws: pcmi_seg_ap_workspace_bytes(c) (the positives per class), 4-byte aligned. */
size_t pcmi_seg_eval_rows_workspace_bytes(int64_t n);
int pcmi_seg_eval_rows(const float* logits, int64_t ld, int64_t n, int c, const int32_t* labels, int ignore_label,
                       int32_t* pred, float* prob_t, int64_t* hist, double* batch4, double* totals3, void* ws,
                       size_t ws_bytes, pcmi_stream_t stream);
size_t pcmi_seg_ap_workspace_bytes(int c);
int pcmi_seg_ap(const float* sorted_prob, const int64_t* order, const int32_t* labels, int64_t n, int c, double* ap,
                double* ap_sum, int64_t* ap_cnt, void* ws, size_t ws_bytes, pcmi_stream_t stream);

/* ---- evaluation on the original point cloud (csrc/nearest.hip) ----------------------------------------------------------
 * What the segmentation test loop does after the forward pass to score the ORIGINAL vertices of a scan (downstream/semseg/
 * lib/test.py:85-93,122-123,190-192): save_predictions (lib/utils.py:304-344) writes the voxel centres in world coordinates
 * with their predictions, dataset.test_pointcloud (lib/datasets/scannet.py:131-171, stanford.py:41-72) builds a scipy KD-tree
 * over them per room, queries it for every vertex and accumulates fast_hist on the host.  Here: three calls, float64
 * throughout, every product and sum rounded on its own in the stated order (no FMA contraction), integer atomics only -- every
 * output is defined by the formulas below bit for bit.  Contiguous tensors, everything on the caller's stream, no
 * synchronisation; a refused call enqueues nothing.
 *
 * pcmi_voxel_centers = lib/utils.py:322-327: coords [n, 4] (int32, batch index FIRST: b, x, y, z), inv_T_host = B x 16 HOST
 *   doubles, the row-major inverse of each scene's voxelizer matrix (rigid_transformation; the caller inverts it) -> centers
 *   [n, 3] (fp64) = inv_T[b] (x + 0.5, y + 0.5, z + 0.5, 1): per output coordinate ((X m0 + Y m1) + Z m2) + m3, the order
 *   csrc/corpus.hip documents.  Whether a row's batch index lies in [0, B) cannot be known without reading the coordinates
 *   back: such a row gets NaN in all three columns and the call succeeds.  The matrices travel as kernel arguments, 32 scenes
 *   per launch.  n < 2^31 - 256; n == 0 enqueues nothing.
 * pcmi_nearest_point = KDTree(pred[:, :3], leafsize=500).query(query_xyz) (scannet.py:154-155), for a batch of scenes: ref
 *   [m, 3] and query [n, 3] (fp64), scene b holding the rows [ref_offs[b], ref_offs[b + 1]) and [query_offs[b],
 *   query_offs[b + 1]) (DEVICE int64 [B + 1], ascending; ref_offs is clamped to [0, m]).  A query searches the references of
 *   its own scene only.  idx [n] (int32) = the GLOBAL row of ref that minimises d2 = (dx dx + dy dy) + dz dz with d = q - r,
 *   every operation rounded in fp64, the LOWEST row among equal d2 (a KD-tree's choice among them is arbitrary); dist2 [n]
 *   (fp64, nullable) = that d2.  This rule defines the result for every input: it equals a brute-force scan.
 *     - a scene without references, or a query row outside [query_offs[0], query_offs[B]): idx -1, dist2 +inf
 *     - a query row with a non-finite coordinate: idx -1, dist2 NaN
 *     - a reference row with a non-finite coordinate is never chosen (a scene of nothing else: idx -1, dist2 +inf)
 *   The references are binned into cubic cells of side `cell` (open-addressing table keyed by scene and cell, records of a
 *   cell contiguous); one lane per query walks the Chebyshev rings around its cell and stops once its best d2 is strictly
 *   below (r cell)^2 (1 - 2^-30), a bound no reference outside the searched cube can reach (justified in the source).
 *   Queries undecided after radius 3 are listed, and a second launch scans their scene's whole segment, one workgroup per
 *   query, with a min-reduction on (d2, row).  The grid only accelerates: neither `cell` nor the ring cap changes an output.
 *   A cell index needs |floor(x / cell)| < 2^17 - 8 per axis.  A finite reference outside that range is not binned, and EVERY
 *   query of its scene takes the whole-segment scan; so does a query whose own cell is outside it: slower, never different.
 *   cell > 0 and finite (PCMI_ERR_INVALID otherwise), unless cell_dev (nullable, DEVICE double [1]) is given, which then
 *   replaces it -- a cell size derived from the data on the device, without reading it back; a cell_dev value that is not
 *   positive and finite sends every query to the scan.  fallback_count [1] (device int64, nullable) += the queries the second
 *   launch scanned.  1 <= B <= 1024; n < 2^31; m <= 2^29 (PCMI_ERR_UNSUPPORTED beyond: the table has 2 m slots).  n == 0
 *   enqueues nothing.  ws: pcmi_nearest_point_workspace_bytes(m, n, B), 16-byte aligned.
 * pcmi_seg_hist = fast_hist(pred[idx], label) of scannet.py:156,168 (lib/utils.py:131-133): pred [m] (int32), idx [n] (int32,
 *   NULL = identity), labels [n] (int32), 1 <= c <= 64 as pcmi_seg_eval_rows (the same workgroup-private matrix in LDS, flushed
 *   with integer atomics).  hist [c, c] (int64) += 1 at [label, pred[idx]] for the rows with 0 <= label < c, 0 <= idx < m and
 *   0 <= pred[idx] < c.  point_pred [n] (int32, nullable) = pred[idx], -1 where idx is outside [0, m) -- the per-vertex labels
 *   the reference writes to <room>.txt; missing [1] (int64, nullable) += the rows with idx outside [0, m).  n == 0 enqueues
 *   nothing. */
int pcmi_voxel_centers(const int32_t* coords, int64_t n, const double* inv_T_host, int64_t B, double* centers,
                       pcmi_stream_t stream);
size_t pcmi_nearest_point_workspace_bytes(int64_t m, int64_t n, int64_t B);
int pcmi_nearest_point(const double* ref, const int64_t* ref_offs, int64_t m, const double* query, const int64_t* query_offs,
                       int64_t n, int64_t B, double cell, const double* cell_dev, int32_t* idx, double* dist2,
                       int64_t* fallback_count, void* ws, size_t ws_bytes, pcmi_stream_t stream);
int pcmi_seg_hist(const int32_t* pred, int64_t m, const int32_t* idx, const int32_t* labels, int64_t n, int c, int64_t* hist,
                  int32_t* point_pred, int64_t* missing, pcmi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The input of segmentation fine-tuning for a batch of scans (csrc/semseg_input.hip) -- what the reference runs per scan on
 * the host in downstream/semseg/lib/dataset.py:289-298: Voxelizer.voxelize (lib/voxelizer.py:81-148) with
 * ME.utils.sparse_quantize(coords, feats, labels, ignore_label), then RandomHorizontalFlip, ChromaticAutoContrast,
 * ChromaticTranslation and ChromaticJitter (lib/transforms.py), feats / 255 - 0.5 (lib/train.py:114-115) and the label map
 * (dataset.py:297-298).  Every random quantity is an INPUT.  Scene b of B holds the rows [offsets[b], offsets[b + 1]) (DEVICE
 * int64 [B + 1], ascending, empty scenes allowed; a row outside [offsets[0], offsets[B]) belongs to no scene and is dropped).
 * 1 <= B <= 1023, row counts < 2^31 - 256.  fp64 arithmetic, every product and sum rounded on its own in the stated order (no
 * FMA contraction); integer atomics only; the same bits from run to run.  Contiguous tensors, everything on the caller's
 * stream, no synchronisation; a refused call enqueues nothing.  Data-dependent errors are ORed into flags [B] (device int32,
 * one word per scene, zeroed by the CALLER so that the calls of a batch share it):
 *   PCMI_SEG_FLAG_RANGE  a point of the scene is not finite, or a voxel coordinate is not inside +-2^20 (pcmi_seg_transform)
 *   PCMI_SEG_FLAG_SPAN   a voxel coordinate minus the scene's minimum is outside [0, 2^18)           (pcmi_seg_quantize)
 *   PCMI_SEG_FLAG_ELASTIC a scene's noise grid does not fit the capacity block; the scene is not distorted  (pcmi_elastic_blur)
 *   PCMI_SEG_FLAG_CROP   no step of the crop ladder brings the scene within max_voxels; it has the last step's window
 *                        (pcmi_seg_crop_ladder, csrc/insseg_input.hip, below)
 * The offending rows are dropped (a scene flagged CROP keeps the rows of its last window).
 *
 * pcmi_seg_transform = voxelizer.py:81-142.  xyz [n, 3] (fp64); mats [B, 16] (DEVICE fp64, row-major 4 x 4: M_r M_v, or M_v
 *   alone without augmentation, voxelizer.py:128-132; the caller builds it).  Clip (voxelizer.py:81-111), if clip_mode != 0,
 *   per scene from the bounding box (mn, mx) of its finite points: size = mx - mn; center = (mn + size 0.5) + ratio size with
 *   ratio = trans_ratio [B, 3] (DEVICE fp64, NULL = 0).  clip_mode 1 (numeric bound L = clip_host[0]): nothing is clipped if
 *   max(size) < L, else a point is kept iff -L + center <= p < L + center on every axis; clip_mode 2 (clip_host = 6 HOST
 *   doubles, (lo, hi) per axis): kept iff lo + center <= p < hi + center.  A kept point gets
 *   vox [n, 3] (int32) = floor(((x m0 + y m1) + z m2) + m3) per matrix row, keep [n] (uint8) = 1; every other row vox 0,
 *   keep 0.  scene_min [B, 3] (int32) = the minimum of vox over the scene's kept rows, 0 for a scene without one (the
 *   reference raises there); aligned [B, 16] (fp64) = M_t M with M_t the translation by -scene_min (voxelizer.py:138-141):
 *   aligned[r][c] = M[r][c] + (-min_r) M[3][c] for r < 3, row 3 copied.  ws: pcmi_seg_transform_workspace_bytes(B), 16-byte
 *   aligned.
 * pcmi_seg_quantize = ME.utils.sparse_quantize(coords - min, feats, labels, ignore_label) for the whole batch (the label rule
 *   as MinkowskiEngine 0.4.3 implements it).  vox [n, 3] (int32), keep [n] (uint8, NULL = all), labels [n] (int32, nullable
 *   together with out_labels), scene_min [B, 3] (NULL = 0).  Two kept rows of a scene are the same voxel iff their vox are
 *   equal (open-addressing table keyed by common.h's pack_key(scene, x - min, y - min, z - min), 2 n slots).  A voxel is
 *   represented by its FIRST row, the lowest; its label is that row's label if every row of the voxel carries the same one,
 *   else ignore_label.  The M voxels leave in ascending order of their first row -- scenes in order, and within a scene the
 *   order of first occurrence (the reference's order is that of a hash-map walk and unspecified): coords [M, 4] (int32; b,
 *   x - min_x, y - min_y, z - min_z), index [M] (int64, the first row), out_labels [M] (int32); the three arrays hold n rows.
 *   counts [B + 1] (DEVICE int64) = the voxels per scene, then M.  n <= 2^29 (PCMI_ERR_UNSUPPORTED beyond).  n == 0 zeroes
 *   counts.  ws: pcmi_seg_quantize_workspace_bytes(n), 16-byte aligned.
 * pcmi_seg_color_augment: one pass over the m voxel rows.  coords [m, 4] (int32, in place; the scene is column 0, a row
 *   whose scene is outside [0, B) is not augmented), source colours feats_src [n_src, 3] (fp32) read at index [m] (int64,
 *   NULL = the row itself; a row outside [0, n_src) reads 0), labels [m] (int32, nullable, in place), params [B, 12] (DEVICE
 *   fp64, NULL = no augmentation): flip x, y, z (non-zero = on) | auto-contrast on, blend | translation on, tr r, g, b |
 *   jitter on, std 255 | unused.  In the reference's order (the input_transform of lib/datasets/scannet.py), per channel in fp64 on
 *   f = the fp32 colour widened:
 *     flip      coords[a] = max_a - coords[a], max_a over the scene's rows                            (transforms.py:173-179)
 *     contrast  (lo, hi) = the channel's extremes over the scene's rows; if hi > lo: scale = 255 / (hi - lo),
 *               f = (1 - blend) f + blend ((f - lo) scale); a channel with hi == lo is left as it is (the reference
 *               divides by zero there)                                                                 (transforms.py:45-61)
 *     translate f = min(max(tr + f, 0), 255)                                                          (transforms.py:32-36)
 *     jitter    f = min(max(normal (std 255) + f, 0), 255), normals [m, 3] (fp32, widened; NULL = off) (transforms.py:69-74)
 *     normalize != 0: f = f / 255 - 0.5                                                                (train.py:114-115)
 *   feats_out [m, 3] (fp32) = f rounded once.  lut [lut_n] (int32, nullable): labels = lut[label] for 0 <= label < lut_n,
 *   ignore_label otherwise (dataset.py:249-259,297-298).  m == 0 enqueues nothing.
 *   ws: pcmi_seg_color_augment_workspace_bytes(B), 16-byte aligned.
 * pcmi_elastic_blur + pcmi_elastic_apply = ONE (granularity g, magnitude) stage of ElasticDistortion (transforms.py:187-217) for
 *   the batch, on the raw points before pcmi_seg_transform; the caller chains the stages, and the second reads the extents the
 *   first left in xyz.  noise [B, cx, cy, cz, 3] (fp32, standard normals, changed in place): scene b's volume [dx, dy, dz, 3]
 *   sits in the corner of its capacity block and is addressed with the capacity strides; 3 <= cx, cy, cz <= 4096 and
 *   B cx cy cz 3 < 2^31.  blur: per scene (mn, mx) = the box of its finite points, grid_min [B, 3] (fp64) = mn, dims =
 *   ((mx - mn) // g) + 3 with numpy's floor division of doubles (the quotient of a - fmod(a, g), floored, plus 1 if it lies more
 *   than 0.5 above its floor); grid_dims [B, 4] (int32) = dx, dy, dz, on.  on = 1 iff active[b] != 0 (DEVICE int32 [B], NULL =
 *   all), the scene has a finite point and dims <= capacity on every axis; an active scene that does not fit gets
 *   PCMI_SEG_FLAG_ELASTIC (its dims are written as 0) and is left undistorted.  Then two rounds of a 3-tap box filter along
 *   x, y, z with zero padding at the DIMS: out = fp32(((v[i-1] w + v[i] w) + v[i+1] w)) in fp64 with w = fp32(1/3) widened, one
 *   rounding per pass.  Elements outside the dims and the volumes of scenes that are not on keep their values.
 *   ws: pcmi_elastic_blur_workspace_bytes(B, cx, cy, cz), 16-byte aligned.
 *   apply: for every row of a scene that is on, per axis the nodes of np.linspace(start, stop, d): start = mn - g, stop = mn +
 *   g (d - 2), step = (stop - start) / (d - 1), node_i = i step + start, node_{d-1} = stop.  A coordinate outside [start, stop]
 *   (or NaN) on any axis adds 0.  Else the interval k with node_k <= p < node_{k+1} (p == stop: k = d - 2, scipy's rule), t = (p -
 *   node_k) / (node_{k+1} - node_k), and value = the sum over the 8 corners -- x slowest, the low node first -- of noise[corner]
 *   ((wx wy) wz) with w = 1 - t at the low node and t at the high one, accumulated from 0 in that order; xyz [n, 3] (fp64, in
 *   place) = p + value magnitude. */
#define PCMI_SEG_FLAG_RANGE 1
#define PCMI_SEG_FLAG_SPAN 2
#define PCMI_SEG_FLAG_ELASTIC 4
#define PCMI_SEG_FLAG_CROP 8
size_t pcmi_elastic_blur_workspace_bytes(int64_t B, int cx, int cy, int cz);
int pcmi_elastic_blur(const double* xyz, const int64_t* offsets, int64_t n, int64_t B, double granularity, const int32_t* active,
                      float* noise, int cx, int cy, int cz, int32_t* grid_dims, double* grid_min, int32_t* flags, void* ws,
                      size_t ws_bytes, pcmi_stream_t stream);
int pcmi_elastic_apply(double* xyz, const int64_t* offsets, int64_t n, int64_t B, double granularity, double magnitude,
                       const float* noise, int cx, int cy, int cz, const int32_t* grid_dims, const double* grid_min,
                       pcmi_stream_t stream);
size_t pcmi_seg_transform_workspace_bytes(int64_t B);
int pcmi_seg_transform(const double* xyz, const int64_t* offsets, int64_t n, int64_t B, const double* mats, int clip_mode,
                       const double* clip_host, const double* trans_ratio, int32_t* vox, uint8_t* keep, int32_t* scene_min,
                       double* aligned, int32_t* flags, void* ws, size_t ws_bytes, pcmi_stream_t stream);
size_t pcmi_seg_quantize_workspace_bytes(int64_t n);
int pcmi_seg_quantize(const int32_t* vox, const uint8_t* keep, const int32_t* labels, const int64_t* offsets,
                      const int32_t* scene_min, int64_t n, int64_t B, int32_t ignore_label, int32_t* coords, int64_t* index,
                      int32_t* out_labels, int64_t* counts, int32_t* flags, void* ws, size_t ws_bytes, pcmi_stream_t stream);
size_t pcmi_seg_color_augment_workspace_bytes(int64_t B);
int pcmi_seg_color_augment(const float* feats_src, int64_t n_src, const int64_t* index, int32_t* coords, int32_t* labels,
                           int64_t m, int64_t B, const double* params, const float* normals, int normalize, const int32_t* lut,
                           int64_t lut_n, int32_t ignore_label, float* feats_out, void* ws, size_t ws_bytes,
                           pcmi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The input of contrastive pre-training for a batch of frame pairs (csrc/pair_input.hip) -- what the reference runs per item on
 * the host in pretrain/pointcontrast/lib/ddp_data_loaders.py ("pc/" below): ScanNetMatchPairDataset.__getitem__ (:196-265) and
 * default_collate_pair_fn (:52-112).  The conventions of "The input of segmentation fine-tuning" above: every random quantity is
 * an INPUT.  A batch holds B pairs = 2 B clouds; cloud c holds the rows [offsets[c], offsets[c + 1]) of one [n, 3] array (DEVICE
 * int64 [2 B + 1], ascending, empty clouds allowed; a row outside [offsets[0], offsets[2 B]) belongs to no cloud and is dropped);
 * clouds 2 b and 2 b + 1 are pair b.  1 <= B <= PCMI_PAIR_MAX_PAIRS, row counts < 2^31 - 256 (PCMI_ERR_INVALID beyond), and at
 * most 2^29 rows where a table is built (PCMI_ERR_UNSUPPORTED beyond).  fp64 arithmetic, every product and sum rounded on its
 * own in the stated order (no FMA contraction); integer atomics only; the same bits from run to run.  Contiguous tensors,
 * everything on the caller's stream, no synchronisation, every kernel launched over all rows of the batch; a refused call
 * enqueues nothing.  Data-dependent errors are ORed into flags [B] (device int32, one word per pair, zeroed by the CALLER so
 * that the calls of a batch share it):
 *   PCMI_PAIR_FLAG_NONFINITE  a point of the pair is not finite, raw, after its transform or after trans
 *   PCMI_PAIR_FLAG_RANGE      a voxel index, or a radius-sized cell index, is outside +-(2^20 - 1) (or radius[b] is not positive)
 *   PCMI_PAIR_FLAG_MATCHES    a source point has more than 96 matches
 * -- the conditions under which pcmi_voxelize / pcmi_match_radius return PCMI_ERR_RANGE.  A pair whose word is not zero when a
 * call writes its rows yields none there: no voxel (pcmi_pair_voxelize), no correspondence (pcmi_pair_match).  The rows and
 * offsets of the other pairs are what they would be without it.
 *
 * pcmi_pair_transform = pc:196-225.  raw [n, 3] (fp32 if raw_is_f32, else fp64; widened to fp64 first), scale [B] (DEVICE fp64; 1
 *   where the reference does not scale), rot [2 B, 9] (DEVICE fp64, row-major rotations R_c; read only if rotate != 0).
 *   x' = scale[b] x.  rotate != 0: the centroid m_c = S_c / n_c (0 for an empty cloud) with S_c summed in this fixed order, which
 *   depends on neither the launch geometry nor the number of compute units: the cloud's rows are cut into chunks of
 *   PCMI_PAIR_CENTROID_CHUNK = 1024 rows from its first row.  Inside a chunk, lane t of 256 adds rows t, t + 256, t + 512, t + 768
 *   to 0 in this order (a row past the cloud's end adds +0), then the 256 lane sums are folded as v[t] = v[t] + v[t + s] for
 *   s = 128, 64 .. 1; S_c = the chunk sums added to 0 in chunk order.  t_c[r] = ((R[r,0] (-m0) + R[r,1] (-m1)) + R[r,2] (-m2)),
 *   p = ((R[r,0] x' + R[r,1] y') + R[r,2] z') + t[r];  trans_b = T_{2b+1} inv(T_{2b}) in the closed form of a rigid matrix:
 *   Rt[r][c] = ((R1[r,0] R0[c,0] + R1[r,1] R0[c,1]) + R1[r,2] R0[c,2]), tt[r] = t1[r] - ((Rt[r,0] t0[0] + Rt[r,1] t0[1]) + Rt[r,2] t0[2]).
 *   rotate == 0: p = x', T = I, trans = I (no centring).  points [n, 3] (fp64), T [2 B, 16], trans [B, 16] (fp64, row-major 4 x 4).
 *   ws: pcmi_pair_transform_workspace_bytes(n, B) (the chunk sums), 16-byte aligned.
 * pcmi_pair_voxelize = pc:228-229, :238-239, :258-259 for all 2 B clouds: the FIRST point (lowest row) of every occupied voxel
 *   floor(p / voxel_size) of each cloud (oracle/loader_ref.sparse_quantize_index per cloud), survivors in ascending row order.
 *   out_points [n, 3] (fp64), coords [n, 3] (int32, floor(p / voxel_size)), first_index [n] (int32, the BATCH row of the point):
 *   the first vox_offsets[2 B] rows are valid.  n_vox [2 B], vox_offsets [2 B + 1] (their prefix) and side_offsets [2, B + 1]
 *   (side_offsets[s][b] = the voxels of clouds 2 b' + s, b' < b: the batch row at which side s of pair b starts in the collate),
 *   all DEVICE int64.  Per cloud an open-addressing table segment of 2 n_c + 1 slots (a 63-bit voxel key has no room for a cloud).
 *   ws: pcmi_pair_voxelize_workspace_bytes(n, B), 16-byte aligned.
 * pcmi_pair_match = pc:36-49, :241 for all B pairs, count -> scan -> fill: every (i, j) with |trans_b p0_i - p1_j| <= radius[b] in
 *   oracle/loader_ref.match_radius's arithmetic (apply_rigid's order, cells floor(. / r), 27-cell probe, (ex ex + ey ey) + ez ez
 *   <= r r), on the voxelised rows: points [m_max, 3] with vox_offsets / side_offsets as pcmi_pair_voxelize left them (m_max >= the
 *   valid rows: the host need not know their number).  radius [B] (DEVICE fp64; the caller's voxel_size * multiplier * scale[b]).
 *   pairs [capacity, 2] (int32): the pairs of the batch concatenated, i and j carrying the batch row offsets side_offsets[0][b],
 *   side_offsets[1][b], sorted by (i, j); a pair without a match contributes the one row (side_offsets[0][b], side_offsets[1][b])
 *   (pc:81-83), a flagged pair none.  pair_counts [B] (DEVICE int64) = the rows per pair; totals [4] (DEVICE int64) = the rows
 *   needed, n_queries (the distinct values of column 0), overflow (1 if the rows needed exceed capacity: then NOTHING is written
 *   to pairs; call again with room for totals[0] rows), capacity.  The counts are exact whatever the capacity.
 *   fill_only != 0 is that second call: it repeats only the per-pair pass and the fill, on the cells, counts and scan that the
 *   call before left in ws -- same arguments but pairs and capacity, the same ws, nothing else run in ws in between, flags as
 *   that call left them.
 *   ws: pcmi_pair_match_workspace_bytes(m_max, B), 16-byte aligned.
 * pcmi_pair_collate = pc:52-112 with pc:248-252 and FeatureJitter (pc/lib/transforms.py:21-30), one launch: voxel row r of cloud
 *   2 b + s goes to row side_offsets[s][b] + (r - vox_offsets[2 b + s]) of side s: C{s} [out_rows, 4] (int32; b, x, y, z),
 *   pcd{s} [out_rows, 3] = fp32(p), F{s} [out_rows, 3] = fp32(1 + (mu + sigma z)) where jitter_on[2 b + s] != 0 (DEVICE int32
 *   [2 B]) and noise is given, else 1; z = noise [n_raw, 3] (fp32 standard normals, widened; NULL = no jitter) at the row
 *   first_index[r] -- the noise belongs to the RAW point, so it is defined before the voxel counts are known.  T_gt [4 B, 4] =
 *   fp32(trans).  A row that would fall outside out_rows is not written.  ws: unused (pcmi_pair_collate_workspace_bytes).
 * pcmi_pair_color_features = the features of a corpus built with colours (data.use_color; the reference has its "#dummy color"
 *   here, pc:204-206, :248-249), one launch after pcmi_pair_collate in stream order, over the same F{s}: color [n_raw, 3] (uint8,
 *   the RGB of the raw rows of the batch), first_index / m_max / vox_offsets / side_offsets / B as pcmi_pair_voxelize left them,
 *   noise / n_raw / jitter_on / mu / sigma / out_rows as in pcmi_pair_collate.  Voxel row r of cloud 2 b + s goes to the row
 *   pcmi_pair_collate sends it to; per channel k, F{s}[k] = fp32((c_k / 255 - 0.5) + (mu + sigma z_k)) where jitter_on[2 b + s] != 0
 *   and noise is given, else fp32(c_k / 255 - 0.5): c (widened to fp64) and z at the raw row first_index[r] -- a voxel has the
 *   colour of its first point, as it has that point's position.  A row outside out_rows, or whose first_index is outside
 *   [0, n_raw), is not written.  Nothing but F0 and F1 is written.  ws: unused (pcmi_pair_color_features_workspace_bytes). */
#define PCMI_PAIR_FLAG_NONFINITE 1
#define PCMI_PAIR_FLAG_RANGE 2
#define PCMI_PAIR_FLAG_MATCHES 4
#define PCMI_PAIR_MAX_PAIRS 512
#define PCMI_PAIR_CENTROID_CHUNK 1024
size_t pcmi_pair_transform_workspace_bytes(int64_t n, int64_t B);
int pcmi_pair_transform(const void* raw, int raw_is_f32, const int64_t* offsets, int64_t n, int64_t B, const double* scale,
                        const double* rot, int rotate, double* points, double* T, double* trans, int32_t* flags, void* ws,
                        size_t ws_bytes, pcmi_stream_t stream);
size_t pcmi_pair_voxelize_workspace_bytes(int64_t n, int64_t B);
int pcmi_pair_voxelize(const double* points, const int64_t* offsets, int64_t n, int64_t B, double voxel_size, double* out_points,
                       int32_t* coords, int32_t* first_index, int64_t* n_vox, int64_t* vox_offsets, int64_t* side_offsets,
                       int32_t* flags, void* ws, size_t ws_bytes, pcmi_stream_t stream);
size_t pcmi_pair_match_workspace_bytes(int64_t m_max, int64_t B);
int pcmi_pair_match(const double* points, int64_t m_max, const int64_t* vox_offsets, const int64_t* side_offsets, int64_t B,
                    const double* trans, const double* radius, int32_t* pairs, int64_t capacity, int64_t* pair_counts,
                    int64_t* totals, int32_t* flags, int fill_only, void* ws, size_t ws_bytes, pcmi_stream_t stream);
size_t pcmi_pair_collate_workspace_bytes(int64_t m_max, int64_t B);
int pcmi_pair_collate(const double* points, const int32_t* coords, const int32_t* first_index, int64_t m_max,
                      const int64_t* vox_offsets, const int64_t* side_offsets, int64_t B, const double* trans, const float* noise,
                      int64_t n_raw, const int32_t* jitter_on, double mu, double sigma, int64_t out_rows, int32_t* C0, int32_t* C1,
                      float* pcd0, float* pcd1, float* F0, float* F1, float* T_gt, void* ws, size_t ws_bytes, pcmi_stream_t stream);
size_t pcmi_pair_color_features_workspace_bytes(int64_t m_max, int64_t B);
int pcmi_pair_color_features(const uint8_t* color, const int32_t* first_index, int64_t m_max, const int64_t* vox_offsets,
                             const int64_t* side_offsets, int64_t B, const float* noise, int64_t n_raw, const int32_t* jitter_on,
                             double mu, double sigma, int64_t out_rows, float* F0, float* F1, void* ws, size_t ws_bytes,
                             pcmi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The input of VoteNet detection fine-tuning for a batch of scans (csrc/detect_input.hip) -- what the reference runs per scan on
 * the host in downstream/votenet_det_new: ScannetDetectionDataset.__getitem__
 * (lib/datasets/scannet/scannet_detection_dataset.py:60-172), SunrgbdDetectionVotesDataset.__getitem__
 * (lib/datasets/sunrgbd/sunrgbd_detection_dataset.py:68-212), and VoxelizationDataset.__getitem__ with collate_fn
 * (models/backbone/sparseconv/voxelized_dataset.py:33-65), for the sparse-backbone recipe: xyz only (no colour, no height).
 * Every random quantity is an INPUT.  Scene b of B holds the raw rows [offsets[b], offsets[b + 1]) (DEVICE int64 [B + 1]) and
 * yields exactly num_points = P output rows, [b P, (b + 1) P) of every [B, P, ...] output.  1 <= B <= 1023, P >= 1, B P <= 2^29,
 * n < 2^31 - 256.  Every product and sum below is rounded on its own, in the stated order and precision (no FMA contraction);
 * integer atomics only; the same bits from run to run.  Contiguous tensors, everything on the caller's stream, no
 * synchronisation; a refused call enqueues nothing.  Pointers to fp64 and int64 data are 8-byte aligned, the others 4-byte
 * (PCMI_ERR_INVALID otherwise).  Data-dependent errors are ORed into flags [B] (device int32, one word per scene, zeroed by
 * the CALLER so that the calls of a batch share it):
 *   PCMI_DET_FLAG_RANGE    a chosen point or a live box is not finite, or a voxel coordinate is not inside +-2^20
 *   PCMI_DET_FLAG_SPAN     a voxel coordinate minus the scene's minimum is outside [0, 2^18) (= PCMI_SEG_FLAG_SPAN, which the
 *                          shared pcmi_seg_quantize sets)
 *   PCMI_DET_FLAG_CHOICE   a choice is outside [0, n_b) (every choice of an empty scene is), or the scene's offsets are not
 *                          0 <= offsets[b] <= offsets[b + 1] <= n
 *   PCMI_DET_FLAG_INSTANCE an instance id is outside [0, PCMI_DET_MAX_INSTANCES) and is not -1
 *   PCMI_DET_FLAG_LABEL    a live box's label id has no class in label_to_class, or its class is outside [0, n_class)
 *   PCMI_DET_FLAG_BOXES    n_boxes[b] is outside [0, PCMI_DET_MAX_NUM_OBJ]; the scene then has no box
 * Common inputs: choices [B, P] (int32, the row WITHIN the scene; repeats allowed -- the reference's random_sampling with
 * replacement, pc_util.py:35-43); augment (0: no flip, rotation or scale is applied and flip, rot, rot_angle, scale may be
 * NULL, the reference's augment=False); flip [B, 2] (int32: flip x, flip y; non-zero = on); rot [B, 9] (fp64, row-major R =
 * rotz(rot_angle), built by the caller with numpy's cos and sin so that both sides use the same bits); scale [B] (fp64; 1
 * for ScanNet).
 *
 * pcmi_det_sample_transform = scannet_detection_dataset.py:103-108,115-128 and sunrgbd_detection_dataset.py:104-106,120,
 *   139-141,193 for the points.  xyz [n, 3] is fp32, as the arrays on disk are.  Per output row, p = xyz[offsets[b] + choice]:
 *     flip      x = -x, y = -y (exact)
 *     rotate    p R^T in fp64 on the widened coordinates: r_i = (x R[i][0] + y R[i][1]) + z R[i][2], rounded to fp32 ONCE -- the
 *               reference assigns np.dot's float64 result into the float32 array.  (np.dot's own order of the three terms is
 *               the BLAS's; it can move the fp32 rounding by one step.)  An identity R returns the inputs, a -0.0 as +0.0.
 *     scale     fp32(fp64(r_i) scale): `point_cloud[:,0:3] *= scale_ratio` multiplies a float32 array by a float64 array in
 *               place -- numpy computes in float64 and rounds the product to float32 (sunrgbd_detection_dataset.py:138-141).
 *   point_clouds [B, P, 3] (fp32).  Optional payloads gathered with the same choice: instance, semantic [n] (int32) ->
 *   out_instance, out_semantic [B, P] (a payload and its output are NULL together).  A row whose choice is out of range
 *   (PCMI_DET_FLAG_CHOICE) or whose point is not finite (PCMI_DET_FLAG_RANGE) is DROPPED: its point is 0, its payloads -1,
 *   which pcmi_det_votes_from_instances passes over silently, so it never gets a vote.
 * pcmi_det_votes_transform = the same for SUN RGB-D, with the stored votes [n, 10] (fp64 -- sunrgbd_data.py writes
 *   np.zeros((N, 10)): the mask, then three votes) carried along (sunrgbd_detection_dataset.py:109,115-125,144-146,194-195,
 *   208-209).  In fp64, per vote v with (x, y, z) the FLIPPED point widened: flip v_x = -v_x, v_y = -v_y; e = p + v per
 *   coordinate; end_i = (e_x R[i][0] + e_y R[i][1]) + e_z R[i][2]; v_i = end_i - fp64(fp32(r_i)) -- the rotated point AFTER
 *   its rounding to fp32, BEFORE the scale; v_i = v_i scale; vote_label [B, P, 9] (fp32) = v rounded once;
 *   vote_label_mask [B, P] (int64) = column 0 truncated (astype).  augment == 0: the votes are only rounded to fp32.  A
 *   dropped row has vote 0 and mask 0.
 * pcmi_det_votes_from_instances = scannet_detection_dataset.py:137-148 on the sampled, augmented points: point_clouds
 *   [B, P, 3] (fp32), instance, semantic [B, P] (int32).  Per scene and instance id, (mn, mx) = the bounding box of the
 *   instance's rows and first = its lowest row (the reference's ind[0]).  If semantic[first] is one of valid_sem [n_valid]
 *   (int32, n_valid <= 1024; the reference's nyu40ids), every row of the instance gets vote = fp32(0.5 fp32(mn + mx)) - x,
 *   all in fp32 as in the reference, and mask 1; every other row vote 0, mask 0.  An instance id decides nothing by itself:
 *   id 0 is left out only because its semantic label is not valid.  vote_label [B, P, 9] (fp32, the vote three times),
 *   vote_label_mask [B, P] (int64).  The extremes are integer atomic minima and maxima of the order-preserving image of
 *   the float (-0.0 sorts below +0.0, where numpy may return either zero: only the SIGN of a zero vote can differ), in an
 *   LDS table per workgroup of 2048 rows, merged into the table in ws.  PCMI_DET_MAX_INSTANCES = 1024: 7 words per id, 28
 *   KiB of the 64 KiB of LDS a workgroup may declare, which leaves two workgroups per CU room beside it.  Id -1 (a dropped
 *   row) gets no vote; another id outside the range, PCMI_DET_FLAG_INSTANCE and no vote; a non-finite point,
 *   PCMI_DET_FLAG_RANGE and no vote.  ws: pcmi_det_votes_from_instances_workspace_bytes(B), 16-byte aligned.
 * pcmi_det_box_labels: one thread per slot of boxes [B, 64, 8] (fp64; cx, cy, cz, then ScanNet: dx, dy, dz, unused, label id --
 *   SUN RGB-D: HALF sizes l, w, h, heading, class), of which the first n_boxes[b] (DEVICE int32 [B]) are live; in fp64, each
 *   output rounded once to its dtype.
 *   mode PCMI_DET_SCANNET (scannet_detection_dataset.py:110-129,150-167, model_util_scannet.py:70-91): on ALL 64 slots, live
 *     or padded (zero): flip cx = -1 cx, cy = -1 cy (a padded zero becomes -0.0, as in the reference); rotate_aligned_boxes: c
 *     = ((cx R[i][0] + cy R[i][1]) + cz R[i][2]); with hx = dx / 2, hy = dy / 2 and the corners (-hx, -hy), (hx, -hy), (hx,
 *     hy), (-hx, hy): X = (u R[0][0] + v R[0][1]) + 0 R[0][2], Y = (u R[1][0] + v R[1][1]) + 0 R[1][2]; dx = 2 max X, dy = 2 max
 *     Y, dz kept.  center_label = c.  Live slots: class = label_to_class[label id] (int32 [n_lut], -1 = none; the reference's
 *     nyu40id2class), size_class = sem_cls = class, size_residual = size - mean_size[class] (fp64 [n_class, 3]); heading 0.
 *   mode PCMI_DET_SUNRGBD (sunrgbd_detection_dataset.py:107-108,121-122,142-143,151-191, model_util_sunrgbd.py:38-65,
 *     sunrgbd_utils.py:226-236): live slots only, the padded ones stay +0.  flip cx = -1 cx, heading = pi - heading (flip y
 *     does not touch a SUN RGB-D box: the reference has none); c = p R^T as above; heading = heading - rot_angle[b] (fp64 [B]);
 *     c = c scale, (l, w, h) = (l, w, h) scale.  angle2class with Python's float %: a % m = fmod(a, m), plus m if that is
 *     negative -- the result takes the divisor's sign, a zero result is +0: ang = heading % 2pi; per = 2pi / num_heading_bin;
 *     shifted = (ang + per / 2) % 2pi; class = trunc(shifted / per); residual = shifted - (class per + per / 2).  size_class =
 *     sem_cls = the box's class; size_residual = (l, w, h) 2 - mean_size[class].  center_label = ((min + max) / 2) per axis
 *     over the eight corners of my_compute_box_3d: with (co, si) = heading_cs [B, 64, 2] (fp64: cos and sin of -1 heading, the
 *     FINAL heading, from the caller's numpy -- the device's cos is not numpy's) and corner offsets x = (-l, l, l, -l, -l, l,
 *     l, -l), y = (w, w, -w, -w, w, w, -w, -w), z = (h, h, h, h, -h, -h, -h, -h): X = ((co x + (-si) y) + 0 z) + cx, Y = ((si x
 *     + co y) + 0 z) + cy, Z = ((0 x + 0 y) + 1 z) + cz.
 *   Outputs [B, 64(, 3)]: center_label, size_residual_label (fp32 [.., 3]), heading_class_label, size_class_label,
 *   sem_cls_label (int64), heading_residual_label, box_label_mask (fp32; 1 for a live slot).  A live box that is not finite
 *   counts as a slot of zeros with mask 1 -- class 0, no residual, no heading (PCMI_DET_FLAG_RANGE); one without a class gets
 *   class 0 and zero residuals (PCMI_DET_FLAG_LABEL).
 * pcmi_det_voxelize = voxelized_dataset.py:37-63 for the batch.  vox = floor(p / fp32(voxel_size)) in fp32 -- numpy divides a
 *   float32 array by a Python float in float32 -- as int32; a row outside +-2^20 (or NaN) is dropped with
 *   PCMI_DET_FLAG_RANGE.  Then pcmi_seg_quantize on (vox, offsets b P, the scenes' minima) without labels, and the minimum is
 *   added back: voxel_coords [M, 4] (int32: b, x, y, z), voxel_inds [M] (int32: the voxel's FIRST row, minus b P), voxel_feats
 *   [M, 3] (fp32 ones); the three arrays hold B P rows, of which the first M = counts[B] are written; counts [B + 1] (DEVICE
 *   int64) = the voxels per scene, then M.  Scenes in order; within a scene the order of first occurrence (the reference's
 *   is that of a hash-map walk and unspecified).  ws: pcmi_det_voxelize_workspace_bytes(B, P), 16-byte aligned. */
#define PCMI_DET_FLAG_RANGE 1
#define PCMI_DET_FLAG_SPAN 2
#define PCMI_DET_FLAG_CHOICE 4
#define PCMI_DET_FLAG_INSTANCE 8
#define PCMI_DET_FLAG_LABEL 16
#define PCMI_DET_FLAG_BOXES 32
#define PCMI_DET_MAX_INSTANCES 1024
#define PCMI_DET_MAX_NUM_OBJ 64
#define PCMI_DET_SCANNET 0
#define PCMI_DET_SUNRGBD 1
int pcmi_det_sample_transform(const float* xyz, const int64_t* offsets, int64_t n, int64_t B, int64_t num_points,
                              const int32_t* choices, int augment, const int32_t* flip, const double* rot, const double* scale,
                              const int32_t* instance, const int32_t* semantic, float* point_clouds, int32_t* out_instance,
                              int32_t* out_semantic, int32_t* flags, pcmi_stream_t stream);
int pcmi_det_votes_transform(const float* xyz, const double* votes, const int64_t* offsets, int64_t n, int64_t B,
                             int64_t num_points, const int32_t* choices, int augment, const int32_t* flip, const double* rot,
                             const double* scale, float* point_clouds, float* vote_label, int64_t* vote_label_mask,
                             int32_t* flags, pcmi_stream_t stream);
size_t pcmi_det_votes_from_instances_workspace_bytes(int64_t B);
int pcmi_det_votes_from_instances(const float* point_clouds, const int32_t* instance, const int32_t* semantic, int64_t B,
                                  int64_t num_points, const int32_t* valid_sem, int n_valid, float* vote_label,
                                  int64_t* vote_label_mask, int32_t* flags, void* ws, size_t ws_bytes, pcmi_stream_t stream);
int pcmi_det_box_labels(const double* boxes, const int32_t* n_boxes, int64_t B, int mode, int augment, const int32_t* flip,
                        const double* rot, const double* rot_angle, const double* scale, const double* heading_cs,
                        const int32_t* label_to_class, int n_lut, const double* mean_size, int n_class, int num_heading_bin,
                        float* center_label, int64_t* heading_class_label, float* heading_residual_label,
                        int64_t* size_class_label, float* size_residual_label, int64_t* sem_cls_label, float* box_label_mask,
                        int32_t* flags, pcmi_stream_t stream);
size_t pcmi_det_voxelize_workspace_bytes(int64_t B, int64_t num_points);
int pcmi_det_voxelize(const float* point_clouds, int64_t B, int64_t num_points, double voxel_size, int32_t* voxel_coords,
                      int32_t* voxel_inds, float* voxel_feats, int64_t* counts, int32_t* flags, void* ws, size_t ws_bytes,
                      pcmi_stream_t stream);

/* ---- The feature columns of the detection input (csrc/detect_features.hip): height above the floor, normalised colour -------
 * What the reference adds per scan on the host with use_height / use_color (downstream/votenet_det_new); nothing here
 * synchronises or reads back.  One more flag bit, set per scene in the same flags [B] as above:
 *   PCMI_DET_FLAG_FEATURE  the scene is empty (or its offsets are not 0 <= offsets[b] <= offsets[b + 1] <= n) or holds a
 *                          non-finite value where a quantile is asked for; or a chosen row's raw colour or raw z is not finite
 *
 * pcmi_segment_quantile = np.percentile(point_cloud[:, 2], 0.99) (scannet_detection_dataset.py:91,
 *   sunrgbd_detection_dataset.py:98) for every scene of a batch.  values[i stride] (fp32) is element i -- the z column of xyz
 *   [n, 3] is read in place with values = xyz + 2, stride = 3 (1 <= stride <= 65536); offsets [B + 1] (DEVICE int64) delimit
 *   the scenes; q in [0, 100].  For a scene of m values, numpy's method="linear" on its own terms, in fp64, every operation
 *   rounded on its own:  v = (m - 1) (q / 100);  k = floor(v);  g = v - k;  lo = the k-th smallest value (from 0), hi = the
 *   min(k + 1, m - 1)-th smallest;  out[b] = lo + (hi - lo) g  (fp64 [B]).  lo and hi are EXACT order statistics, the values a
 *   full sort would put at those ranks; a zero (lo, hi or out) is returned as +0.  out_stats [B, 2] (fp32; may be NULL) = lo, hi.
 *   numpy's own float32 path rounds hi - lo, the product and the sum to fp32 and so differs by up to 3 fp32 ulps of
 *   max(|lo|, |hi|).  An empty scene or one that holds a NaN or an infinity: PCMI_DET_FLAG_FEATURE, out = 0, out_stats = 0.
 *   A radix select, eight bits a pass, over the order-preserving integer image of the floats (-0.0 sorts below +0.0):
 *   histograms in LDS with integer atomics.  One launch with one workgroup per scene serves every scene of up to 16384
 *   values; when n > 16384 four launches (one a pass) of one workgroup per 8192 values and a closing launch serve the larger
 *   scenes, merging into ws with integer additions and one integer minimum -- the same bits from run to run.
 *   B <= 1023 and n < 2^29, PCMI_ERR_RANGE beyond.  ws: pcmi_segment_quantile_workspace_bytes(B), 16-byte aligned.
 * pcmi_det_point_features writes the final point_clouds [B, P, 3 + C] (fp32) in the reference's column order: xyz -- copied
 *   from point_clouds_xyz [B, P, 3], the output of pcmi_det_sample_transform / pcmi_det_votes_transform --, then rgb if rgb
 *   [n, 3] (fp32, raw) is given, then the height if floor_height [B] (DEVICE fp64, e.g. out of pcmi_segment_quantile) is
 *   given; C = 1, 3 or 4 (both NULL: PCMI_ERR_INVALID).  Row (b, p) reads raw row offsets[b] + choices[b, p]; xyz [n, 3] is
 *   the raw scan (only z is read, only with floor_height).
 *     height  fp32(fp64(z) - floor_height[b]); mode PCMI_DET_SUNRGBD with augment: then fp32(fp64(height) scale[b])
 *             (sunrgbd_detection_dataset.py:147-148: a float32 column times a float64 scalar in place, which numpy >= 2
 *             computes in float64).  ScanNet's flips and rotation about z leave it alone.  The reference subtracts numpy's
 *             float32 percentile in float32: one more fp32 rounding beside the quantile's bound.
 *     colour  PCMI_DET_SCANNET: fp32((fp64(rgb) - MEAN) / 256), MEAN = (109.8, 97.2, 83.8) (scannet_detection_dataset.py:24,
 *             88); no augmentation.  PCMI_DET_SUNRGBD: c = fp32(fp64(rgb) - 0.5) (sunrgbd_detection_dataset.py:38,95); with
 *             augment, in fp64 (:129-136): x = c + 0.5; x = x color_gain[b, j]; x = x + color_shift[b, j]; x = x +
 *             color_jitter[b, p]; x = min(max(x, 0), 1); x = x * (color_keep[b, p] != 0); out = fp32(x - 0.5).  color_gain,
 *             color_shift [B, 3], color_jitter [B, P] (fp64), color_keep [B, P] (uint8) may each be NULL: 1, 0, 0, 1.  The
 *             reference draws jitter and keep per RAW point before sampling; here they are per CHOSEN point.
 *   A row whose choice is out of range (PCMI_DET_FLAG_CHOICE) has feature columns 0; a non-finite raw colour, or a
 *   non-finite raw z with floor_height, sets PCMI_DET_FLAG_FEATURE and leaves those columns 0.  scale [B] (fp64) is read only
 *   for the augmented SUN RGB-D height. */
#define PCMI_DET_FLAG_FEATURE 64
size_t pcmi_segment_quantile_workspace_bytes(int64_t B);
int pcmi_segment_quantile(const float* values, int64_t stride, const int64_t* offsets, int64_t n, int64_t B, double q,
                          double* out, float* out_stats, int32_t* flags, void* ws, size_t ws_bytes, pcmi_stream_t stream);
int pcmi_det_point_features(const float* point_clouds_xyz, const float* xyz, const float* rgb, const int64_t* offsets, int64_t n,
                            int64_t B, int64_t num_points, const int32_t* choices, const double* floor_height, int mode,
                            int augment, const double* scale, const double* color_gain, const double* color_shift,
                            const double* color_jitter, const uint8_t* color_keep, float* out, int32_t* flags,
                            pcmi_stream_t stream);

int pcmi_sgd_step(float* w, const float* g, float* v, int64_t n, float lr, float momentum,
                  float weight_decay, float grad_scale, pcmi_stream_t stream);
/* The same with torch's dampening (the downstream fine-tuning's optimiser: SGD(lr, sgd_momentum, dampening =
 * sgd_dampening 0.1, weight_decay), downstream/semseg/lib/solvers.py:52-60, config/default.yaml:16-19):
 *   v = mu*v + (1 - dampening)*g, except on the optimiser's first step (first_step != 0, v zero-filled), where torch
 *   initialises the buffer with g itself. */
int pcmi_sgd_step_dampened(float* w, const float* g, float* v, int64_t n, float lr, float momentum,
                           float dampening, float weight_decay, float grad_scale, int first_step,
                           pcmi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Network executor -- the reference drives the 63 convs / 62 BNs of Res16UNet34C from Python
 * (pc/model/res16unet.py:206-268, autograd for the backward).  Here a model is lowered ONCE into
 * a static program (tensors + ops, built by tracing the Python module tree) and a whole forward
 * or backward is ONE call that enqueues every kernel from C++: no per-layer host overhead,
 * activations in a per-pass arena, concatenations as column slices of a shared buffer
 * (zero copy), gradients accumulated straight into the flat gradient buffer.
 *   tensor: (level, channels) rows = voxels of that level (tensor stride 2^level); parent >= 0
 *           makes it the column slice [col_off, col_off + channels) of tensor `parent`.
 *   op    : CONV (MinkowskiConvolution / Transpose), BN (+ residual, + ReLU), L2NORM.
 * The training step of the reference needs two passes per iteration (one per point cloud,
 * pc/lib/ddp_trainer.py:392-398): activations of pass p stay valid until pcmi_net_backward(p).
 * ------------------------------------------------------------------------------------------ */
#define PCMI_OP_CONV 0
#define PCMI_OP_BN 1
#define PCMI_OP_L2NORM 2

typedef struct pcmi_net pcmi_net_t;
typedef struct pcmi_net_tensor {
  int32_t level, channels, parent, col_off;
} pcmi_net_tensor_t;
typedef struct pcmi_net_op {
  int32_t type, in, in2, out;   /* tensor ids; in2 = residual input of a BN or -1 */
  int32_t cin, cout, kernel_size, stride, region, transpose, relu, has_bias;
  int64_t w_off, b_off;         /* flat-parameter offsets: conv kernel / bias, BN gamma / beta */
  float* running_mean;          /* BN buffers (device pointers; not part of the flat parameters) */
  float* running_var;
  float momentum, eps;
} pcmi_net_op_t;
/* Called from pcmi_net_backward as soon as every gradient of parameter range `bucket` has been ENQUEUED -- on the
 * backward stream and, for the weight gradients, on the executor's own low-priority stream.  The backward chain does not
 * wait for that stream at a bucket boundary; a consumer (the gradient all-reduce, pc/lib/ddp_trainer.py:96-102 = what
 * DistributedDataParallel's bucket hooks do) orders ITS stream behind both from inside the callback with
 * pcmi_net_stream_wait_bucket. */
typedef void (*pcmi_ready_fn)(void* ctx, int bucket);

int pcmi_net_create(const pcmi_net_tensor_t* tensors, int n_tensors, const pcmi_net_op_t* ops,
                    int n_ops, int input_tensor, int output_tensor, int n_passes, pcmi_net_t** out);
int pcmi_net_destroy(pcmi_net_t* net);
/* in_feats [n_rows, in_ld] and out_feats [n_rows, out_ld] are caller memory; coords must hold
 * key 0 with n_rows rows.  May sync the first times (arena growth, coordinate planning).
 * training: 0 = eval (running BN estimates), 1 = train (batch statistics, running estimates
 * updated in place as torch's BatchNorm1d), 1 | PCMI_NET_DEFER_RUNNING_STATS = train, but the
 * running-estimate updates of this pass are only applied by pcmi_net_apply_running_stats: two
 * passes (the two clouds of a pair, ddp_trainer.py:404-407) can then be forwarded concurrently
 * on two streams and still update the estimates in the reference's order (pass 0, then 1). */
#define PCMI_NET_DEFER_RUNNING_STATS 2
int pcmi_net_forward(pcmi_net_t* net, int pass, pcmi_coords_t* coords, const float* in_feats,
                     int64_t in_ld, int64_t n_rows, const float* params, int training,
                     float* out_feats, int64_t out_ld, pcmi_stream_t stream);
/* d_out: gradient w.r.t. out_feats.  Parameter gradients are ACCUMULATED into grads (flat, same
 * layout as params; the caller zero-fills it once per iteration).  bucket_lo_host: ascending
 * flat offsets splitting the parameters into n_buckets ranges (may be NULL / 0 with ready). */
int pcmi_net_backward(pcmi_net_t* net, int pass, const float* d_out, int64_t d_ld,
                      const float* params, float* grads, const int64_t* bucket_lo_host,
                      int n_buckets, pcmi_ready_fn ready, void* ready_ctx, pcmi_stream_t stream);
/* Inside a pcmi_ready_fn callback: `stream` waits (device side, no host wait) for everything that produced the bucket
 * the callback announces.  PCMI_ERR_INVALID outside a backward pass that has announced a bucket. */
int pcmi_net_stream_wait_bucket(pcmi_net_t* net, pcmi_stream_t stream);
/* The convolution precision mode (PCMI_CONV_PRECISION_*, see pcmi_set_conv_precision) of every later forward and backward
 * pass of `net`; a backward pass uses the mode set when it is called.  Default fp32.  PCMI_ERR_INVALID for other values. */
int pcmi_net_set_conv_precision(pcmi_net_t* net, int precision);
/* Applies, on `stream` (ordered behind that forward), the running-estimate updates a forward of `pass` with
 * PCMI_NET_DEFER_RUNNING_STATS left pending, once; with nothing pending it does nothing.  While they are pending the pass
 * is closed: pcmi_net_forward of the same pass, in any mode, returns PCMI_ERR_INVALID before it enqueues or changes
 * anything (it would overwrite the table and the updates would be lost).  Other passes are not affected, and
 * pcmi_net_backward of the pass does not need the updates applied.  A forward that returns an error leaves nothing
 * pending on its pass. */
int pcmi_net_apply_running_stats(pcmi_net_t* net, int pass, pcmi_stream_t stream);
/* The momentum of every BatchNorm op of `net` for later training forwards (the detection fine-tuning's BNMomentumScheduler,
 * vn/lib/train.py: a new value per epoch); a net that never calls it keeps the momenta it was created with.  Passes already
 * enqueued are not affected.  PCMI_ERR_INVALID outside [0, 1]. */
int pcmi_net_set_bn_momentum(pcmi_net_t* net, float momentum);
/* Copy of one activation tensor of the last forward of `pass` (they stay in the pass's arena until its next forward)
 * into caller memory out [rows, out_ld]; rows / channels (nullable) report its shape, out == NULL only queries.  For
 * inspection and for tests that hand the device's ReLU patterns to the oracle (the reference has no counterpart: its
 * activations are autograd-owned torch tensors). */
int pcmi_net_export_tensor(pcmi_net_t* net, int pass, int tensor, int64_t* rows, int* channels, float* out,
                           int64_t out_ld, pcmi_stream_t stream);
int pcmi_net_memory_bytes(pcmi_net_t* net, size_t* bytes);
/* Measurement (bench.py roofline.in_step_ms; the reference has no counterpart: torch.autograd.profiler would be its
 * tool): timing events around the convolution launches of the ops `ops[0..n_ops)` (indices into the program) INSIDE the
 * passes -- forward, the backward(-data) launch and (on the executor's weight-gradient stream) the weight-gradient launch
 * of the same op; any op type -- in a ring of n_sets event sets, one per forward pass enqueued after this call (networks run as one
 * pass per iteration; the backward pass records into the set of the forward before it).  n_ops == 0 stops timing.
 * Synchronises the device.  pcmi_net_timed_ms waits for set `set` and returns the elapsed stream time per op in ms
 * (-1: not recorded). */
int pcmi_net_time_ops(pcmi_net_t* net, const int* ops, int n_ops, int n_sets);
int pcmi_net_timed_ms(pcmi_net_t* net, int set, float* fwd_ms, float* bwd_ms, float* wgrad_ms, int n_ops);
/* The same for EVERY op of the program (convolutions, BatchNorms, the L2 normalisation: forward and backward launches on
 * the pass's stream, weight gradients on the executor's side stream) -- bench.py's per-layer times and `families[]`.  The
 * weight gradients the executor collects into grouped launches (coarse levels) stay grouped; those launches are timed as
 * such: pcmi_net_timed_groups_ms returns up to `cap` of them for set `set` (n_out = how many).  n_sets == 0 stops timing.
 * pcmi_net_timed_ms then takes n_ops = the number of ops of the program. */
int pcmi_net_time_all(pcmi_net_t* net, int n_sets);
int pcmi_net_timed_groups_ms(pcmi_net_t* net, int set, float* ms, int cap, int* n_out);
/* Kernel launches each timed call of set `set` enqueued (forward, backward(-data), weight gradient; 0 = not recorded), and
 * -- groups != NULL after pcmi_net_time_all -- of its first groups_cap grouped weight-gradient launches. */
int pcmi_net_timed_launches(pcmi_net_t* net, int set, int* fwd, int* bwd, int* wgrad, int n_ops, int* groups, int groups_cap);

/* ------------------------------------------------------------------------------------------
 * Validation of the pre-training on held-out pairs (csrc/featmatch.hip).  The reference has none: its trainers descend from
 * FCGF's contrastive trainer, whose validation matches features between the two clouds of a pair and checks every match
 * against the known relative pose; pc/lib/ddp_trainer.py dropped that step.  Pair b of B holds the rows [offsets[b],
 * offsets[b + 1]) of each of its arrays (DEVICE int64 [B + 1], ascending, offsets[0] = 0, empty segments allowed; the kernels
 * clamp every offset into its array, so a malformed table gives wrong answers, never an access outside).  1 <= B <= 1024
 * (PCMI_ERR_UNSUPPORTED beyond), row counts < 2^31 - 256.  Nothing synchronises; every random quantity is an INPUT.
 *
 * pcmi_feat_nn: the nearest neighbour in feature space of every query, inside its own pair, for all pairs in one call.
 *   qf [nq, c] (row stride q_ld) with q_offs, rf [nr, c] (r_ld) with r_offs.  query_rows == NULL: row i of qf is query i (Q =
 *   nq).  Else query_rows [n_query_rows] (int32) with query_offs [B + 1]: query i of pair b (query_offs[b] <= i <
 *   query_offs[b + 1]) is row query_rows[i] of qf, which must lie in [q_offs[b], q_offs[b + 1]); repeats and any order are
 *   fine.  Per query: d2(j) = sum over c ascending of fma(a_c - b_c, a_c - b_c, d2) in fp32, over the rows j of rf in the
 *   query's pair; nn = the row j (GLOBAL row of rf) with the smallest d2, the LOWEST row among equal d2; d2 = that minimum.
 *     - a d2(j) that is not finite in fp32 is never chosen: a reference row with a NaN / inf feature never wins
 *     - a query for which no row can be chosen gets nn = -1 and d2 = NaN: its pair has no reference rows, the query has a
 *       non-finite feature, or query_rows[i] lies outside its pair's segment of qf (so -1 is a legal entry of query_rows)
 *   c a multiple of 16 in 16 ... 128, else PCMI_ERR_UNSUPPORTED.  q_ld, r_ld >= c and multiples of 4, qf and rf 16-byte aligned
 *   (PCMI_ERR_INVALID otherwise).  Launch: 64 queries per workgroup (4 x 4 distances per thread, fp32 FMAs on LDS tiles) times
 *   nch chunks of every reference segment, nch = min(ceil(4 CUs / (ceil(Q / 64) + B)), ceil(nr / 256), 64), at least 1; the
 *   chunks meet in an unsigned 64-bit minimum over (bits of d2) << 32 | row -- d2 >= +0, so its bits order like the number --
 *   which makes the result independent of the order of arrival: the same bits from run to run.  ws: 8 Q bytes
 *   (pcmi_feat_nn_workspace_bytes), 8-byte aligned, else PCMI_ERR_WORKSPACE.  Q == 0 enqueues nothing.
 *
 * pcmi_match_stats: the geometric check.  xyz0 [n0, 3], xyz1 [n1, 3] (fp64, voxel coordinate x voxel size), T_gt [B, 4, 4]
 *   (fp64, DEVICE, row-major), queries as above (query_rows NULL: n_queries == n0 and query_offs are cloud 0's offsets; query_offs
 *   is always given), nn01 [n_queries] (int32, rows of xyz1), nn10 [n_queries] (int32, nullable: the nearest row of cloud 0 of
 *   the MATCHED row nn01[i]), has_gt [n0] (uint8, nullable), tau_host[n_tau], 1 <= n_tau <= PCMI_MATCH_MAX_TAU.  Per query i of
 *   pair b with row r: valid = 0 <= r < n0 and 0 <= nn01[i] < n1; then y = T_gt[b] x0[r] as ((R0 x + R1 y) + R2 z) + t per
 *   coordinate (lib/ddp_data_loaders.py: _apply_rigid), d = y - x1[nn01[i]], residual2[i] = (dx dx + dy dy) + dz dz, every
 *   operation rounded on its own; residual2[i] = NaN if not valid.  counts [B, PCMI_MATCH_STAT_COLS] (int64) += per pair:
 *     [PCMI_MATCH_N_QUERY] every query          [PCMI_MATCH_N_VALID] the valid ones       [PCMI_MATCH_N_MUTUAL] valid and nn10[i] == r
 *     [PCMI_MATCH_N_GT] 0 <= r < n0 and has_gt[r] != 0                                    [PCMI_MATCH_HITS + t] valid and residual2 <= fl(tau_t tau_t)
 *     [PCMI_MATCH_HITS_GT + t] both.  Columns of thresholds not given, and of inputs that are NULL, are left as they are.
 *   Integer atomics only, so several calls add up.  A query outside [query_offs[0], query_offs[B]) counts nowhere.
 *
 * pcmi_ransac_score: src, dst [m, 3] (fp64: the matched points of cloud 0 and cloud 1) with offsets; triples [B, H, 3] (int32,
 *   indices LOCAL to the pair's segment); 1 <= H <= 65536 (PCMI_ERR_UNSUPPORTED beyond); tau >= 0.  Hypothesis (b, h) with
 *   p_k = src[offsets[b] + triples[b, h, k]], q_k likewise from dst.  The frame of a triangle (a0, a1, a2), every operation
 *   rounded on its own, sums of three terms as (x + y) + z, a cross product a x b = (ay bz - az by, az bx - ax bz, ax by - ay bx):
 *     u = a1 - a0, lu = sqrt(u.u), e1 = u / lu;  n = e1 x (a2 - a0), ln = sqrt(n.n), e3 = n / ln;  e2 = e3 x e1.
 *   With (e1, e2, e3) of p and (f1, f2, f3) of q: R[i][j] = (f1[i] e1[j] + f2[i] e2[j]) + f3[i] e3[j],
 *   t[i] = q0[i] - ((R[i][0] p0x + R[i][1] p0y) + R[i][2] p0z).  Invalid, counts = -1: a repeated index, an index outside
 *   [0, segment length), a segment of fewer than 3 matches, or lu or ln below 1e-9 (or NaN) in either cloud.  Else counts [B, H]
 *   (int32) = the matches k of the segment with |R src_k + t - dst_k|^2 <= fl(tau tau), computed as in pcmi_match_stats.  best
 *   [B] (int32) = the hypothesis of the highest count, the LOWEST among equals, -1 if none is valid; Rt [B, 12] (fp64) = its R
 *   row-major, then t (NaN where best is -1).  Launch: one thread per hypothesis, 256 per workgroup, the segment's matches
 *   staged through LDS 512 at a time (m is unbounded); then one workgroup per pair for best.
 *
 * pcmi_rigid_sums: over the inliers (the same test, against Rt[b]) of each pair's best hypothesis, sums [B, 16] (fp64) = n,
 *   sum p (3), sum q (3), S (9, row-major) with S[i][j] = sum (p_i - pm_i)(q_j - qm_j).  TWO PASSES: the first gives n, sum p,
 *   sum q and the means pm = sum p / n, qm = sum q / n; the second sums the products of the centred coordinates.  In both, lane
 *   t of one 256-lane workgroup per pair adds the inliers among matches t, t + 256, ... in ascending order (from +0), and the
 *   256 partials are folded by halving: x[t] = x[t] + x[t + s] for s = 128, 64, ... 1.  All zeros where best is -1.  The 3 x 3
 *   SVD (Kabsch) is the caller's, on the host. */
#define PCMI_MATCH_MAX_TAU 4
#define PCMI_MATCH_N_QUERY 0
#define PCMI_MATCH_N_VALID 1
#define PCMI_MATCH_N_MUTUAL 2
#define PCMI_MATCH_N_GT 3
#define PCMI_MATCH_HITS 4
#define PCMI_MATCH_HITS_GT 8
#define PCMI_MATCH_STAT_COLS 12
size_t pcmi_feat_nn_workspace_bytes(int64_t n_queries);
int pcmi_feat_nn(const float* qf, int64_t q_ld, int64_t nq, const int64_t* q_offs, const float* rf, int64_t r_ld, int64_t nr,
                 const int64_t* r_offs, int64_t B, int c, const int32_t* query_rows, const int64_t* query_offs,
                 int64_t n_query_rows, int32_t* nn, float* d2, void* ws, size_t ws_bytes, pcmi_stream_t stream);
int pcmi_match_stats(const double* xyz0, int64_t n0, const double* xyz1, int64_t n1, const double* T_gt, int64_t B,
                     const int32_t* query_rows, const int64_t* query_offs, int64_t n_queries, const int32_t* nn01,
                     const int32_t* nn10, const uint8_t* has_gt, const double* tau_host, int n_tau, int64_t* counts,
                     double* residual2, pcmi_stream_t stream);
int pcmi_ransac_score(const double* src, const double* dst, int64_t m, const int64_t* offsets, int64_t B, const int32_t* triples,
                      int64_t H, double tau, int32_t* counts, int32_t* best, double* Rt, pcmi_stream_t stream);
int pcmi_rigid_sums(const double* src, const double* dst, int64_t m, const int64_t* offsets, int64_t B, const int32_t* best,
                    const double* Rt, double tau, double* sums, pcmi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Spatially partitioned PointInfoNCE (csrc/nce_part.hip) -- the objective of Hou et al., "Exploring Data-Efficient 3D Scene
 * Understanding with Contrastive Scene Contexts", stated here (the reference has no counterpart): the negatives of every anchor are
 * partitioned by where they lie around it, one InfoNCE per partition.
 *
 * Inputs.  q, k [n, c] (fp32, c in {16, 32}, 16-byte aligned; row i of k is the positive of row i of q); xyz [n, 3] (int32, the
 * voxel coordinates of the queries, 18-bit signed); scene [n] (int32, the batch index of each query); n_scenes B in 1..1024;
 * inv_T; r1_sq <= r2_sq (int64 >= 0, squared radii in voxel units); A in {1, 2, 4, 8} azimuth sectors about the z axis; E in
 * {1, 2} elevation halves; P = 2 E A <= 32.  Anything else: PCMI_ERR_INVALID (PCMI_ERR_UNSUPPORTED for c), nothing enqueued.
 *
 * part(i, j), the partition of column j as seen from row i -- all integers, d = xyz[j] - xyz[i], d2 = dx dx + dy dy + dz dz
 * in int64:
 *   part = -1 (j is a negative of i in no partition) if i == j, d2 == 0, d2 > r2_sq, scene[i] != scene[j], or either scene id
 *   lies outside [0, B).  Otherwise
 *   shell = 0 if d2 <= r1_sq, else 1;   el = 0 if E == 1 or dz >= 0, else 1;   the azimuth sector, on (dx, dy):
 *     1. h = 0 if dy > 0 or (dy == 0 and dx > 0), else 1; if h == 1, (dx, dy) <- (-dx, -dy);
 *     2. qd = 0 if dx > 0, else 1; if qd == 1, (dx, dy) <- (dy, -dx);
 *     3. o = 0 if dy < dx, else 1;
 *   az = 0, h, 2 h + qd, 4 h + 2 qd + o for A = 1, 2, 4, 8 (floor(atan2(dy, dx) mod 2 pi / (2 pi / A)) with half-open sectors;
 *   dx == dy == 0 gives A - 1);   part = (shell E + el) A + az.   part(i, j) is not symmetric.
 *
 * Loss.  With l_ij = inv_T q_i.k_j:  lse[i, p] = log(exp(l_ii) + sum_{j: part(i, j) = p} exp(l_ij)).  Row i is live in p if at
 * least one j has part(i, j) = p; R[s, p] = the live rows of scene s in partition p; p is live in s if R[s, p] is not empty;
 * L_s = the live partitions of scene s; S = the scenes with L_s > 0:
 *   loss = (1 / S) sum_{s: L_s > 0} (1 / L_s) sum_{p live in s} (1 / |R[s, p]|) sum_{i in R[s, p]} (lse[i, p] - l_ii),
 * and 0 if S == 0.  With w[i, p] = 1 / (S L_s |R[s, p]|) for live (i, p), 0 otherwise:
 *   G_ij = w[i, part(i, j)] exp(l_ij - lse[i, part(i, j)]) for part(i, j) >= 0,  G_ii = sum_p w[i, p] (exp(l_ii - lse[i, p]) - 1),
 *   every other entry 0;  dq = gscale inv_T G k,  dk = gscale inv_T G^T q  (gscale: device scalar, nullable -> 1).
 *
 * pcmi_pnce_fwd writes lse [n, P], live [B, P] (int32: live[s, p] = |R[s, p]|, 0 for a dead partition) and *loss (device
 * scalar).  lse of a (row, partition) that is NOT live is written as l_ii, the value of the definition over an empty set, in the
 * bits the backward forms l_ii with (so its term exp(l_ii - lse) - 1 is exactly 0).  pcmi_pnce_bwd reads them back.
 * The n x n logits and partitions are never written; fp32 products (one fmaf per channel, ascending), a maximum per (row,
 * partition), no float atomics; the per-partition sums and the loss are reduced in float64 in a fixed order, counts are
 * integers; every output is the same bits from run to run.  ws: pcmi_pnce_workspace_bytes(n, c, B, P) bytes, 16-byte aligned,
 * else PCMI_ERR_WORKSPACE.  Any n >= 1.
 *
 * pcmi_pnce_partition: a test aid, n <= 4096 (PCMI_ERR_UNSUPPORTED beyond): part [n, n] (int8) = part(i, j) from the same device
 * function as the loss kernels.
 * ------------------------------------------------------------------------------------------ */
size_t pcmi_pnce_workspace_bytes(int64_t n, int c, int n_scenes, int P);
int pcmi_pnce_fwd(const float* q, const float* k, const int32_t* xyz, const int32_t* scene, int64_t n, int c, int n_scenes,
                  float inv_T, int64_t r1_sq, int64_t r2_sq, int A, int E, float* lse, int32_t* live, float* loss, void* ws,
                  size_t ws_bytes, pcmi_stream_t stream);
int pcmi_pnce_bwd(const float* q, const float* k, const int32_t* xyz, const int32_t* scene, const float* lse, const int32_t* live,
                  int64_t n, int c, int n_scenes, float inv_T, int64_t r1_sq, int64_t r2_sq, int A, int E, const float* gscale,
                  float* dq, float* dk, void* ws, size_t ws_bytes, pcmi_stream_t stream);
int pcmi_pnce_partition(const int32_t* xyz, const int32_t* scene, int64_t n, int n_scenes, int64_t r1_sq, int64_t r2_sq, int A,
                        int E, int8_t* part, pcmi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Instance segmentation (csrc/cluster.hip) -- the downstream task of Hou et al., "Contrastive Scene Contexts", in PointGroup's
 * recipe, stated here (the reference has no counterpart): the network predicts a class and an offset to its instance's centre
 * per voxel, the voxels are shifted by their offsets, and shifted voxels of one class within a radius of each other are grouped.
 * Every call: one stream, no host synchronisation; a refused call enqueues nothing; integer atomics only, float64 sums in a
 * fixed order: every output is the same bits from run to run.  Every `offs` is DEVICE int64 [B + 1], ascending, inside [0, n]:
 * scene b holds the rows [offs[b], offs[b + 1]) (empty scenes allowed).  n == 0 reads nothing.
 *
 * pcmi_radius_components = the connected components of a radius graph.  xyz [n, 3] (fp32, leading dimension ld >= 3 floats),
 *   group [n] (int32), r > 0 and finite (PCMI_ERR_INVALID otherwise).  A row is ACTIVE if it lies in a scene, group >= 0, its
 *   three coordinates are finite and |floor(x / r)| < 2^20 on every axis (x widened to fp64, the quotient rounded once).  Two
 *   active rows i != j are joined by an edge if they share their scene and their group and
 *     d2 = (dx dx + dy dy) + dz dz <= r r,   d = p_i - p_j,
 *   the coordinates widened to fp64 and every difference, product and sum rounded on its own (dist2_rn / mul_rn of
 *   csrc/exact.h: the rule of the radius probe).  label [n] (int32) = the LOWEST row of the row's connected component, -1 for a
 *   row that is not active.  dropped [1] (int64, nullable) += the finite in-scene rows with group >= 0 whose cell does not fit.
 *   Against PointGroup's ball query + breadth-first search: no cap on the neighbours of a row (theirs: 50, which makes the
 *   result depend on the row order) and <= where they have <.  This rule defines the result for every input: it equals a
 *   brute-force scan of all pairs.
 *   The rows are binned into cells of side r (1 + 2^-30) (the margin makes the 27 cells around a row hold every neighbour: see
 *   the source) in an open-addressing table with one segment per scene; one lane per binned row unites itself, in a lock-free
 *   union-find kept in `label`, first with the first row of its own cell and then with every lower row in the 27 cells that
 *   passes the test.  A root is only ever hooked under a smaller root (compare-and-swap), so parent[i] <= i always, every walk
 *   descends, every retry lowers the larger root, nothing waits for another lane, and the final root is the component's lowest
 *   row whatever the interleaving.  1 <= B <= 2^20; n <= 2^29 (PCMI_ERR_UNSUPPORTED beyond: 2 n + B table slots, int32 rows).
 *   ws: pcmi_radius_components_workspace_bytes(n, B), 16-byte aligned.
 * pcmi_components_compact: label [n] as above (any value outside [0, n) is a row of no component), group [n] (nullable) ->
 *   the components with at least min_points >= 1 rows, numbered 0 .. P - 1 in ascending order of their lowest row (scene-major,
 *   the rows being so).  inst [n] (int32) = the row's number, -1 for every other row; count [1] (int32) = P, the true number even
 *   beyond max_inst: components numbered >= max_inst are written nowhere and their rows get -1.  inst_root / inst_size /
 *   inst_scene / inst_group [max_inst] (int32) = the component's lowest row, its rows, the scene and the group of that row;
 *   entries from min(P, max_inst) on are -1 (size: 0).  Sizes by integer atomics, the numbering by a scan in row order.
 *   ws: pcmi_components_compact_workspace_bytes(n), 4-byte aligned.
 * pcmi_instance_scores: out [P] (fp64) = the mean of score [n] (fp32) over the rows with inst == k, in fixed point:
 *   q = (int64) rint((double) min(max(score, 0), 1) 2^30), a non-finite score counting as 0, summed by 64-bit integer atomics;
 *   out = (double) sum / ((double) inst_size[k] 2^30), 0 where inst_size[k] <= 0.  Ids outside [0, P) count nowhere.
 *   ws: pcmi_instance_scores_workspace_bytes(P), 8-byte aligned.
 * pcmi_instance_overlap: pred_inst / gt_inst [n] (int32) -> inter [P, G], pred_size [P], gt_size [G] (int32), all zeroed by the
 *   call: the rows per id and per pair of ids; an id outside [0, P) / [0, G) counts nowhere.  P G < 2^31.
 * pcmi_instance_match: per predicted instance the ground-truth instance g with gt_scene[g] == pred_scene[p] and gt_class[g] ==
 *   pred_class[p] that maximises inter / (pred_size + gt_size - inter), the quotient of the two integers in fp64 (0 where the
 *   denominator is 0), the LOWEST g among equal quotients; best_gt [P] (int32) = g, best_iou [P] (fp32) = the quotient rounded
 *   once; -1 and -inf without such a g: the contract of pcmi_det_match, so pcmi_det_ap consumes the result unchanged.
 * pcmi_instance_centroids: coords [n, 4] (int32: b, x, y, z), inst [n] -> sum [G, 3] (int64) = the sums of x, y, z over the
 *   rows with inst == k and cnt [G] (int64) their number, both zeroed by the call; ids outside [0, G) count nowhere.
 * pcmi_offset_loss_fwd / _bwd: PointGroup's two offset losses on p [n, 3] (fp32, leading dimension ld: a column slice of the
 *   logits), g [n, 3] (fp32, contiguous: the targets) and inst [n] (a row is valid iff inst >= 0), V = the valid rows:
 *     norm = sum_valid ((|p0 - g0| + |p1 - g1|) + |p2 - g2|) / (V + 1e-6)
 *     dir  = sum_valid -((gh0 ph0 + gh1 ph1) + gh2 ph2) / (V + 1e-6),   gh = g / (|g| + 1e-8), ph = p / (|p| + 1e-8),
 *     |v| = sqrt((v0 v0 + v1 v1) + v2 v2),
 *   per row in fp64 from the fp32 inputs, every operation rounded on its own in this order; the sums are fp64 partials per 256
 *   rows merged in a fixed order.  out3 [3] (fp64) = norm, dir, V.  _bwd: dp [n, 3] (fp32, leading dimension dp_ld) =
 *   (gloss2[0] sign(p - g) + gloss2[1] d(row's dir term)/dp) / (V + 1e-6) rounded once, 0 for an invalid row; sign(0) = 0 and the
 *   gradient of |p| at p = 0 is 0 (torch's conventions).  gloss2 [2] (fp64, device): the two upstream gradients; out3 as _fwd
 *   wrote it.  ws: pcmi_offset_loss_workspace_bytes(n), 8-byte aligned.
 * ------------------------------------------------------------------------------------------ */
size_t pcmi_radius_components_workspace_bytes(int64_t n, int64_t B);
int pcmi_radius_components(const float* xyz, int64_t ld, int64_t n, const int64_t* offs, int64_t B, const int32_t* group, double r,
                           int32_t* label, int64_t* dropped, void* ws, size_t ws_bytes, pcmi_stream_t stream);
size_t pcmi_components_compact_workspace_bytes(int64_t n);
int pcmi_components_compact(const int32_t* label, const int64_t* offs, int64_t B, int64_t n, const int32_t* group, int min_points,
                            int64_t max_inst, int32_t* inst, int32_t* count, int32_t* inst_root, int32_t* inst_size,
                            int32_t* inst_scene, int32_t* inst_group, void* ws, size_t ws_bytes, pcmi_stream_t stream);
size_t pcmi_instance_scores_workspace_bytes(int64_t P);
int pcmi_instance_scores(const float* score, const int32_t* inst, int64_t n, int64_t P, const int32_t* inst_size, double* out,
                         void* ws, size_t ws_bytes, pcmi_stream_t stream);
int pcmi_instance_overlap(const int32_t* pred_inst, const int32_t* gt_inst, int64_t n, int64_t P, int64_t G, int32_t* inter,
                          int32_t* pred_size, int32_t* gt_size, pcmi_stream_t stream);
int pcmi_instance_match(const int32_t* inter, const int32_t* pred_size, const int32_t* gt_size, const int32_t* pred_scene,
                        const int32_t* pred_class, const int32_t* gt_scene, const int32_t* gt_class, int64_t P, int64_t G,
                        int32_t* best_gt, float* best_iou, pcmi_stream_t stream);
int pcmi_instance_centroids(const int32_t* coords, const int32_t* inst, int64_t n, int64_t G, int64_t* sum, int64_t* cnt,
                            pcmi_stream_t stream);
size_t pcmi_offset_loss_workspace_bytes(int64_t n);
int pcmi_offset_loss_fwd(const float* p, int64_t ld, const float* g, const int32_t* inst, int64_t n, double* out3, void* ws,
                         size_t ws_bytes, pcmi_stream_t stream);
int pcmi_offset_loss_bwd(const float* p, int64_t ld, const float* g, const int32_t* inst, int64_t n, const double* out3,
                         const double* gloss2, float* dp, int64_t dp_ld, pcmi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The input of instance-segmentation fine-tuning (csrc/insseg_input.hip): what stands between pcmi_seg_quantize and a batch
 * that InstanceSegmentationTrainer.train_iter takes -- ground-truth instance indices that are unique across the scenes of a
 * batch, the per-instance table both instance evaluators need, and a per-scene crop.  The reference has no counterpart; the
 * rules are stated here.  All arithmetic is integer; integer atomics only (sums, minima, maxima, ors, and the compare-and-swap
 * that claims a table slot, whose outcome reaches no output); every output is the same bits from run to run.  One stream, no
 * host synchronisation, a refused call enqueues nothing.
 * In all three calls offsets [B + 1] is DEVICE int64, ascending: scene b holds the rows [offsets[b], offsets[b + 1]).  The
 * arrays hold n rows of capacity; a row outside every scene -- at or beyond offsets[B], or below offsets[0] -- is neither read
 * nor written, so the calls chain behind pcmi_seg_quantize (offsets = the running sums of its counts) before those counts are
 * read back.  1 <= B <= 1023; n < 2^31 - 256 (PCMI_ERR_INVALID beyond) and n <= 2^29 (PCMI_ERR_UNSUPPORTED beyond, as
 * pcmi_seg_quantize).  n == 0 enqueues nothing beyond zeroing the counts.
 *
 * pcmi_instance_relabel: raw [n] (int32) = per-scene instance ids as datasets store them: arbitrary non-negative integers,
 *   the same id in two scenes meaning two instances; keep [n] (uint8, NULL = all).  A row with raw < 0 or keep == 0 belongs to
 *   no instance.  Two remaining rows are the same instance iff they share their scene and their raw id.  Instances are numbered
 *   0, 1, ... in ascending order of their LOWEST row: scenes in order, within a scene the order of first occurrence -- the
 *   convention of pcmi_components_compact.  instance [n] (int32) = the row's number, -1 for a row in no instance; first_row [n]
 *   (int32): the lowest row of instance g at position g, valid up to the count; inst_counts [B + 1] (DEVICE int64) = the
 *   instances whose lowest row lies in each scene, then their sum.  Ids are always < n: there is no capacity to exceed.
 *   An open-addressing table of 2 n slots keyed by (scene << 32) | raw, an atomic minimum of the row per slot, a flag per row
 *   that is its key's minimum, the three-launch scan of the flags (csrc/rowscan.h, shared with pcmi_components_compact), one
 *   lookup per row.  ws: pcmi_instance_relabel_workspace_bytes(n), 16-byte aligned.
 * pcmi_instance_table: instance [n] (int32), klass [n] (int32, nullable together with cls), coords [n, 4] (int32: b, x, y, z;
 *   nullable together with sum, box_min and box_max) -> per instance g in [0, G), all initialised by the call:
 *     size [G] (int32)      its rows
 *     scene [G] (int32)     the largest scene among its rows, -1 without rows
 *     cls [G] (int32)       max(-1, the maximum of klass over its rows), any value of klass included -- what
 *                           scatter_reduce("amax", include_self=True) into a tensor of -1 gives
 *     sum [G, 3] (int64)    the exact sums of coords[:, 1:4]: pcmi_instance_centroids' sum, as size is its cnt
 *     box_min / box_max [G, 3] (int32)  the extremes of coords[:, 1:4]; INT32_MAX / INT32_MIN without rows
 *   An id outside [0, G) counts nowhere.  0 <= G < 2^31; G == 0 enqueues nothing.  No workspace.
 * pcmi_seg_crop_ladder: a window per scene that bounds its voxels.  THIS RULE IS THE PROJECT'S OWN: it is in the spirit of the
 *   crop in PointGroup's recipe, NOT a restatement of it, and its parameters are untuned.  It works on voxel rows after
 *   quantization.  coords [n, 4] (int32; the min-shifted coordinates pcmi_seg_quantize writes), axis0 != axis1 in 1 ... 3 (the
 *   horizontal columns of coords), sides [S, 2] (HOST int32, 1 <= S <= 32, window sides in voxels, every side >= 1, each
 *   column non-increasing), draws [B, S, 2] (DEVICE uint32), max_voxels >= 1; anything else: PCMI_ERR_INVALID.  Per scene, with
 *   ext_a = the maximum of column a over its rows: a scene of at most max_voxels rows keeps all of them, step = -1.  Otherwise,
 *   for step s,
 *     slack_a = max(ext_a + 1 - side[s][a], 0),   origin_a = (uint64(draw[b][s][a]) (slack_a + 1)) >> 32,
 *     a row is inside iff origin_a <= c_a < origin_a + side[s][a] on both axes,
 *   and the scene takes the LOWEST s whose inside count is <= max_voxels; if no step fits it takes step S - 1 and gets
 *   PCMI_SEG_FLAG_CROP (flags [B], ORed in).  Coordinates are NOT shifted again, so the batch's transformation stays valid.
 *   rows [n] (int64) = the kept rows in ascending order; kept_counts [B + 1] (DEVICE int64) = the kept rows per scene, then
 *   their sum; step [B] (int32).  Launches: the scene extents; the origins; one pass in which every row of a scene above
 *   max_voxels tests all S windows (a 32-bit mask per row) and the per-step counts are gathered per scene in LDS; the choice;
 *   the scan and scatter of the kept rows.  ws: pcmi_seg_crop_ladder_workspace_bytes(n, B), 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
size_t pcmi_instance_relabel_workspace_bytes(int64_t n);
int pcmi_instance_relabel(const int32_t* raw, const uint8_t* keep, const int64_t* offsets, int64_t n, int64_t B, int32_t* instance,
                          int32_t* first_row, int64_t* inst_counts, void* ws, size_t ws_bytes, pcmi_stream_t stream);
int pcmi_instance_table(const int32_t* instance, const int32_t* klass, const int32_t* coords, const int64_t* offsets, int64_t n,
                        int64_t B, int64_t G, int32_t* size, int32_t* scene, int32_t* cls, int64_t* sum, int32_t* box_min,
                        int32_t* box_max, pcmi_stream_t stream);
size_t pcmi_seg_crop_ladder_workspace_bytes(int64_t n, int64_t B);
int pcmi_seg_crop_ladder(const int32_t* coords, const int64_t* offsets, int64_t n, int64_t B, int axis0, int axis1,
                         const int32_t* sides_host, int S, const uint32_t* draws, int64_t max_voxels, int64_t* rows,
                         int64_t* kept_counts, int32_t* step, int32_t* flags, void* ws, size_t ws_bytes, pcmi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Instance masks by the benchmark protocol (csrc/insbench.hip) -- the scoring rules of ScanNet's
 * evaluate_semantic_instance.py, RESTATED FROM THE SCRIPT'S RULES, NEVER RUN AGAINST THE SCRIPT (the reference has no instance
 * segmentation).  They differ from pcmi_instance_match + pcmi_det_ap (VOC-style) in four ways: predictions below a minimum
 * region size are dropped, unmatched predictions that lie mostly on void or on small regions are ignored, duplicate
 * predictions claim by the script's own rule, and the precision-recall curve is integrated in the script's way.
 * Every call: one stream, no host synchronisation; a refused call enqueues nothing; integer atomics only, no workgroup waits
 * for another, float64 operations rounded one by one in the stated order: every output is the same bits from run to run.
 * NULL is accepted for an array without elements.
 *
 * pcmi_instance_void_overlap: pred_inst / gt_inst [n] (int32), gt_valid [G] (int32) -> void_inter [P] (int32, zeroed by the
 *   call) = the rows of prediction p that are VOID: gt_inst outside [0, G), or gt_valid[gt_inst] == 0 (the caller sets
 *   gt_valid = gt_class >= 0).  An id outside [0, P) counts nowhere.  One pass over the rows; a wave whose rows agree adds
 *   once (pcmi_instance_overlap's aggregation).  The overlap matrix is pcmi_instance_overlap's.
 *
 * pcmi_instance_bench_match.  One batch of B scenes: inter [P, G], pred_size [P], gt_size [G] (pcmi_instance_overlap),
 *   void_inter [P], pred_scene / pred_class [P] (int32), pred_score [P] (fp64, not NaN: a NaN score is never `best`),
 *   gt_scene / gt_class [G] (int32; gt_class = -1: an instance that is not scored), min_region >= 1 (the benchmark: 100),
 *   thresholds: a HOST array of 1 <= T <= 16 values in [0.25, 1) (PCMI_ERR_INVALID otherwise).
 *     kept prediction       0 <= class < Cls, 0 <= scene < B, pred_size >= min_region; any other produces nothing
 *     counted ground truth  0 <= class < Cls, 0 <= scene < B, gt_size >= min_region;  npos[c] += their number per class
 *     small ground truth    gt_class >= 0 and gt_size < min_region
 *     iou(p, g) = (double) inter / (double) (gt_size + pred_size - inter), ONE division, compared with a strict > against the
 *       threshold; defined where inter > 0 and p and g share scene and class
 *   Per scene, class and threshold th, independently:
 *     visited = {}
 *     for g ascending over the counted ground truths:
 *       claim = [p ascending over the kept predictions: inter[p, g] > 0, p not visited, iou(p, g) > th]
 *       if claim is not empty: visited += claim[0] (ONLY the first claimant, whatever its score -- the script's behaviour: at
 *         0.25 a duplicate claimant may claim the next instance too); best = the claimant of the highest score, the lowest p
 *         among equal scores; every p of claim emits an entry (score[p], true = (p == best))
 *     for p over the kept predictions with no ground truth g of ANY size (same scene and class) with iou(p, g) > th:
 *       ignore = void_inter[p] + the sum of inter[p, g] over the SMALL ground truths of p's scene and class
 *       p emits (score[p], false) if (double) ignore / (double) pred_size[p] <= th, and is ignored otherwise
 *   The multiset of entries is the script's (its running max / min of confidences gives the true positive the highest
 *   claimant's score).  Disjoint ground truths above th each cover more than th pred_size rows, so a prediction claims fewer
 *   than 1 / th <= 4 times: at most 3 entries (a prediction holding 3 claims no further -- unreachable with overlaps counted by
 *   pcmi_instance_overlap).  At th >= 0.5 a prediction claims once and `visited` never acts.
 *   entry_flag [T, P, 3] (int8): -1 none, 0 false positive, 1 true positive; slot s of p is its s-th claim in walk order, the
 *   unmatched false positive goes into slot 0.  gt_state [T, G] (int32): 1 matched, 0 counted and unmatched, -1 not counted.
 *   Both are written in full; npos [Cls] (int32) is INCREMENTED.
 *   One wave per (threshold, scene, class) walks that unit's ground truths in order -- sequential by definition, tens of
 *   instances per scene -- with its lanes over the predictions and two wave reductions per claim (first, best).
 *   Limits: P G < 2^31 (the overlap matrix), 1 <= B <= 65535, 1 <= Cls <= 64.
 *
 * pcmi_instance_bench_ap: the entries of all accumulated batches, listed by the caller class by class in descending score as
 *   pcmi_det_ap's detections: entry_flag [T, E] (int8), score [E] (fp64), class c at [cls_offs[c], cls_offs[c + 1]) (int32
 *   [Cls + 1]), npos [Cls] (int32) -> ap [T, Cls] (fp64).  Flags of -1 are skipped, wherever they stand.
 *     npos <= 0: NaN.  Otherwise the K remaining entries in list order, equal scores (== on the doubles) forming one group,
 *     groups j = 1 .. m; tp_j / fp_j = the counts up to the end of group j; P_j = tp_j / (tp_j + fp_j), R_j = tp_j / npos;
 *     P_0 = 1, R_0 = 0, R_-1 = 0, R_m+1 = R_m;
 *       ap = sum over j = 0 .. m of P_j (0.5 (R_j+1 - R_j-1)),  from 0 in ascending j
 *     -- the script's np.convolve(recall, [-0.5, 0, 0.5], 'valid') written out; K = 0 gives 0.
 *   prec / rec [T, E] (fp64, nullable): P_j and R_j at the LAST entry of group j, NaN (all bits set) everywhere else.
 *   One workgroup per (class, threshold) walks its range in blocks of 1024 with a carry (a class may hold any number of
 *   entries, a group may straddle blocks), then adds the terms in order.  E < 2^30, 1 <= Cls <= 64, 1 <= T <= 16.
 *   ws: pcmi_instance_bench_ap_workspace_bytes(E, Cls, n_thresholds), 4-byte aligned.
 * ------------------------------------------------------------------------------------------ */
int pcmi_instance_void_overlap(const int32_t* pred_inst, const int32_t* gt_inst, const int32_t* gt_valid, int64_t n, int64_t P,
                               int64_t G, int32_t* void_inter, pcmi_stream_t stream);
int pcmi_instance_bench_match(const int32_t* inter, const int32_t* pred_size, const int32_t* gt_size, const int32_t* void_inter,
                              const int32_t* pred_scene, const int32_t* pred_class, const double* pred_score,
                              const int32_t* gt_scene, const int32_t* gt_class, int64_t P, int64_t G, int64_t B, int Cls,
                              int min_region, const double* thresholds, int n_thresholds, int8_t* entry_flag, int32_t* gt_state,
                              int32_t* npos, pcmi_stream_t stream);
size_t pcmi_instance_bench_ap_workspace_bytes(int64_t E, int Cls, int n_thresholds);
int pcmi_instance_bench_ap(const int8_t* entry_flag, const double* score, const int32_t* cls_offs, const int32_t* npos, int64_t E,
                           int Cls, int n_thresholds, double* ap, double* prec, double* rec, void* ws, size_t ws_bytes,
                           pcmi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Active labelling (csrc/kmeans.hip) -- the point selection of the data-efficient benchmark of Hou et al., "Contrastive
 * Scene Contexts", stated here (the reference has no counterpart): k-means with K = the annotation budget on the per-voxel
 * features of every scene, the voxel nearest to each centre is annotated.  All scenes of a batch in one launch sequence.
 * Every call: one stream, no read-back, no host synchronisation; a refused call enqueues nothing; integer atomics only;
 * every output is the same bits from run to run.
 *
 * Common.  feat [n, C] (fp32, leading dimension ld >= C, ld a multiple of 4, base 16-byte aligned), C a multiple of 16 in
 * 16..128 (pcmi_feat_nn's rule, PCMI_ERR_UNSUPPORTED otherwise).  offs: DEVICE int64 [B + 1], ascending; scene b holds the
 * rows [offs[b], offs[b + 1]) clamped into [0, n] and CUT to its first max_scene_rows rows (a host number: the caller's bound
 * on the rows of a scene; rows beyond it lie in no scene).  max_scene_rows <= PCMI_KMEANS_MAX_SCENE_ROWS = 2^20 and
 * 1 <= K <= PCMI_KMEANS_MAX_K = 1024 clusters per scene, PCMI_ERR_UNSUPPORTED beyond; 1 <= B <= 65535.
 *   A row is ACTIVE if it lies in a scene and every channel has |x| <= 1024 (which a NaN or an infinity fails).
 *   Cluster k of scene b is LIVE if live[b, k] >= 0 (int32 [B, K], as pcmi_kmeans_init writes it).  A dead cluster is never
 *   assigned and its centroid is written as 0.
 *   Distance: the fp32 chain of pcmi_feat_nn, d2 = fma(a_c - b_c, a_c - b_c, d2) over ascending c.  An active row goes to the
 *   live cluster of its scene with the smallest d2, the LOWEST k among equal d2 (a d2 that is not finite -- a centroid given
 *   with a NaN -- is never chosen): the choice pcmi_feat_nn makes among the scene's centroids, bit for bit.  A row that is not
 *   active, or has no cluster to go to, gets assign = -1 (d2 = NaN); skipped [B] (int64) = the rows of the scene that are not active
 *   PLUS the rows of its segment that max_scene_rows cut off (so a cut shows: those rows get assign = -1 like rows in no scene).
 *   Sums: q = (int64) rint((double) x 2^32) per channel of an assigned row (exact for |x| >= 2^-8), added by 64-bit integer
 *   atomics; at most 2^20 rows of 2^42 each: 2^62.  centroid = (float) ((double) sum / ((double) cnt 2^32)), the product and the
 *   quotient rounded once each; a live cluster with cnt == 0 keeps its previous centroid.
 *
 * pcmi_kmeans_init: centroid [B, K, C] = the feature rows init_rows [B, K] (int32, GLOBAL rows; -1: a dead cluster).
 *   live [B, K] = init_rows where the row lies in scene b and is active, else -1 (centroid 0); flags [B] (int64) = the entries
 *   >= 0 that were refused so.  live must not alias init_rows.
 * pcmi_kmeans_step: one Lloyd iteration.  Assigns every row against centroid_in -> assign [n] (int32; not aliasing assign_prev),
 *   sum [B, K, C] (int64), cnt [B, K] (int32), centroid_out [B, K, C], changed [B] (int64) = the rows of the scene whose
 *   assignment differs from assign_prev (nullable: all -1), skipped [B].  One pass over feat does the assignment and the sums
 *   (no [n, K] distance matrix): sums and counts are kept in LDS and flushed once per workgroup where K (8 C + 4) bytes fit
 *   beside the tiles (80 KiB per workgroup in all), else added to memory directly.
 * pcmi_kmeans_assign: the final pass.  assign [n], d2 [n] (fp32), cnt [B, K], skipped [B];  nearest [B, K] (int32) = the
 *   GLOBAL row of the member nearest to the cluster's centroid, a 64-bit minimum on (d2 bits << 32 | row): the lowest row among
 *   equal d2; -1 for a cluster without members.  inertia [B] (fp64) = the sum of the members' d2 widened to fp64: partial p of a
 *   scene covers its rows [256 p, 256 (p + 1)), one per lane (non-members as 0), summed by a butterfly inside each wave of 64
 *   (v += v[lane ^ d], d = 1 ... 32) and the four waves in ascending order; lane t of one workgroup adds the partials t,
 *   t + 256, ... in that order from 0, and the 256 lanes are summed the same way (pcmi_offset_loss_fwd's rule, per scene).
 *   ws: pcmi_kmeans_assign_workspace_bytes(B, K), 8-byte aligned.
 * pcmi_kmeans_pp_step: one step of k-means++ seeding with the draw as data, in integers.  mind2 [n] (fp32, >= 0; +inf before
 *   the first step), last [B] (int32, nullable: the centre chosen last, a global row), draw [B] (uint64).  Where last[b] is an
 *   active row of scene b, mind2 of every active row of the scene is lowered to min(mind2, d2 to that row) (otherwise the
 *   scene's mind2 stays).  w = (uint64) floor(min(mind2, 2^20) 2^20) for an active row, 0 otherwise; total = sum w (<= 2^60);
 *   target = the high 64 bits of total x draw[b];  next [B] (int32) = the first row of the scene, in row order, whose inclusive
 *   cumulative weight exceeds target; the lowest active row if total == 0; -1 if the scene has no active row.  The FIRST
 *   centre is a step with last = NULL (or -1) and mind2 = +inf: every active row weighs 2^40, so the draw picks uniformly.
 *   Weights and totals are integers (a block scan per 256 rows, integer atomics per 4096): no order changes the result.
 *   n < 0x7f7f7f7f (PCMI_ERR_UNSUPPORTED beyond).  ws: pcmi_kmeans_pp_step_workspace_bytes(B), 8-byte aligned.
 * ------------------------------------------------------------------------------------------ */
#define PCMI_KMEANS_MAX_K 1024
#define PCMI_KMEANS_MAX_SCENE_ROWS (1 << 20)
int pcmi_kmeans_init(const float* feat, int64_t ld, int64_t n, const int64_t* offs, int64_t B, int K, int c, int64_t max_scene_rows,
                     const int32_t* init_rows, float* centroid, int32_t* live, int64_t* flags, pcmi_stream_t stream);
int pcmi_kmeans_step(const float* feat, int64_t ld, int64_t n, const int64_t* offs, int64_t B, int K, int c, int64_t max_scene_rows,
                     const float* centroid_in, const int32_t* live, const int32_t* assign_prev, int32_t* assign, int64_t* sum,
                     int32_t* cnt, float* centroid_out, int64_t* changed, int64_t* skipped, pcmi_stream_t stream);
size_t pcmi_kmeans_assign_workspace_bytes(int64_t B, int K);
int pcmi_kmeans_assign(const float* feat, int64_t ld, int64_t n, const int64_t* offs, int64_t B, int K, int c, int64_t max_scene_rows,
                       const float* centroid, const int32_t* live, int32_t* assign, float* d2, int32_t* nearest, double* inertia,
                       int32_t* cnt, int64_t* skipped, void* ws, size_t ws_bytes, pcmi_stream_t stream);
size_t pcmi_kmeans_pp_step_workspace_bytes(int64_t B);
int pcmi_kmeans_pp_step(const float* feat, int64_t ld, int64_t n, const int64_t* offs, int64_t B, int c, int64_t max_scene_rows,
                        const int32_t* last, const uint64_t* draw, float* mind2, int32_t* next, void* ws, size_t ws_bytes,
                        pcmi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Dual-set instance proposals (csrc/proposals.hip) -- the second half of PointGroup's grouping: the voxels are clustered where
 * they are AND where their offsets send them, the union of the sets is reduced by non-maximum suppression on mask IoU, and
 * the survivors are OVERLAPPING masks.  The reference has no counterpart; the rules are stated here.
 * Overlapping proposals are a membership matrix member [n, S] (int32, leading dimension ld >= S): column s is one partition
 * of the rows into proposals, -1 for none; 1 <= S <= 4 (PCMI_ERR_INVALID otherwise).  By the convention of cluster_proposals
 * column s names the slots [s M, (s + 1) M) of the per-proposal arrays [P = S M]; the two calls below only need the values
 * to lie in [0, P).  prop_scene [P] (int32): the proposal's scene, a value outside [0, B) for an unused slot.
 * Every call: one stream, no host synchronisation; a refused call enqueues nothing; integer atomics only; every output is the
 * same bits from run to run.  1 <= B <= 65535, 1 <= Kmax (a HOST bound on the proposals of one scene), B Kmax^2 < 2^31
 * (PCMI_ERR_INVALID otherwise); Kmax > 1024: PCMI_ERR_UNSUPPORTED (Kmax x Kmax suppression bits are 128 KiB of LDS).
 *
 * pcmi_proposal_overlap -> all outputs initialised by the call but `dropped`:
 *     size [P] (int32)         the entries of member equal to p (a row naming p in two columns counts twice)
 *     scene_count [B] (int32)  the USED slots of scene b: the p with prop_scene[p] == b -- the true number, also beyond Kmax
 *     local [P] (int32)        the proposal's index within its scene: its rank among the used slots of that scene in
 *                              ascending slot order; -1 for an unused slot and for every slot of rank >= Kmax: a scene with
 *                              more than Kmax used slots keeps its first Kmax, and dropped [1] (int64, nullable) += the rest
 *     inter [B, Kmax, Kmax] (int32)  inter[b, i, j] = the rows that name both proposal i and proposal j of scene b (by
 *                              `local`) in two DIFFERENT columns: symmetric, the diagonal zero
 *   A member value outside [0, P) counts nowhere; a pair of proposals of different scenes, a pair with a dropped or unused
 *   proposal and a pair (a, a) count nowhere.
 *   Launches: one workgroup per scene scans prop_scene in slot order (a block scan per 256 slots with a carry); one lane per
 *   row adds its S sizes and its at most S (S - 1) / 2 pairs (both orientations).  Rows of one object stand together, so a
 *   wave's lanes mostly hold one value per column: where a column is uniform over the wave's rows its first lane adds the lane
 *   count, and so for a pair of uniform columns (pcmi_instance_overlap's aggregation); any other wave adds lane by lane.
 *   n < 2^31 - 256.  ws: pcmi_proposal_overlap_workspace_bytes(P), 4-byte aligned.
 * pcmi_proposal_nms: inter, size, local, scene_count as above, prop_class [P] (int32), score [P] (fp64) -> keep [P] (int32): 1
 *   for a kept proposal, 0 for every other slot (suppressed, not a candidate, unused, dropped).  Per scene:
 *     candidates  local >= 0, size >= 1, class >= 0, score finite and >= min_score
 *     rank        descending score (compared as fp64), ascending slot among equal scores
 *     in rank order, a candidate that is still alive is kept and clears every LATER candidate j with
 *       (double) inter / (double) (size_i + size_j - inter) > nms_iou
 *     -- one fp64 division, a strict comparison, a NaN quotient suppresses nothing.  A suppressed candidate suppresses nobody.
 *   The test does not look at classes (PointGroup's rule).  One workgroup per scene: ranks by counting, the suppression matrix
 *   as bits in LDS, one wave sweeping it (pcmi_box_nms's scheme); 256 threads for Kmax <= 256, 1024 beyond.
 * ------------------------------------------------------------------------------------------ */
size_t pcmi_proposal_overlap_workspace_bytes(int64_t P);
int pcmi_proposal_overlap(const int32_t* member, int64_t ld, int64_t n, int S, const int32_t* prop_scene, int64_t P, int64_t B,
                          int Kmax, int32_t* size, int32_t* local, int32_t* scene_count, int32_t* inter, int64_t* dropped, void* ws,
                          size_t ws_bytes, pcmi_stream_t stream);
int pcmi_proposal_nms(const int32_t* inter, const int32_t* size, const int32_t* local, const int32_t* scene_count,
                      const int32_t* prop_scene, const int32_t* prop_class, const double* score, int64_t P, int64_t B, int Kmax,
                      double nms_iou, double min_score, int32_t* keep, pcmi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PCMI_H_ */
