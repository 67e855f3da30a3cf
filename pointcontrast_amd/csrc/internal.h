// Cross-file internal entry points (same semantics as the C ABI, plus accumulate flags).
#pragma once
#include "common.h"

namespace pcmi {

int spconv_forward(const float* in, int64_t in_ld, int64_t n_in, int cin, const float* weight, int cout,
                   const pcmi_kmap_t* map, int transpose, const float* bias, float* out, int64_t out_ld,
                   int64_t n_out, int accumulate, void* ws, size_t ws_bytes, hipStream_t st);
int spconv_backward_data(const float* gout, int64_t gout_ld, int64_t n_out, int cout, const float* weight, int cin,
                         const pcmi_kmap_t* map, int transpose, float* gin, int64_t gin_ld, int64_t n_in,
                         int accumulate, void* ws, size_t ws_bytes, hipStream_t st);
int spconv_backward_weight(const float* in, int64_t in_ld, int64_t n_in, int cin, const float* gout,
                           int64_t gout_ld, int64_t n_out, int cout, const pcmi_kmap_t* map, int transpose,
                           float* gweight, float* gbias, int accumulate, void* ws, size_t ws_bytes, hipStream_t st);
// the same three on the MFMA path proper (channel counts multiples of 32, or the 3-channel stem); the entry points
// above add zero-padded staging for any other width (widths.hip)
int spconv_forward_m32(const float* in, int64_t in_ld, int64_t n_in, int cin, const float* weight, int cout,
                       const pcmi_kmap_t* map, int transpose, const float* bias, float* out, int64_t out_ld,
                       int64_t n_out, int accumulate, void* ws, size_t ws_bytes, hipStream_t st);
int spconv_backward_data_m32(const float* gout, int64_t gout_ld, int64_t n_out, int cout, const float* weight, int cin,
                             const pcmi_kmap_t* map, int transpose, float* gin, int64_t gin_ld, int64_t n_in,
                             int accumulate, void* ws, size_t ws_bytes, hipStream_t st);
int spconv_backward_weight_m32(const float* in, int64_t in_ld, int64_t n_in, int cin, const float* gout,
                               int64_t gout_ld, int64_t n_out, int cout, const pcmi_kmap_t* map, int transpose,
                               float* gweight, float* gbias, int accumulate, void* ws, size_t ws_bytes, hipStream_t st);
size_t spconv_workspace_m32(int64_t n_in, int64_t n_out, int cin, int cout, int K, int64_t M);
// Weight gradients of several layers in ONE launch (spconv_wgrad.hip: wgrad_mfma_group_kernel).  add() == true: the layer's
// gradient is enqueued by the next flush() on the stream given there (its operands must exist on that stream by then and
// stay untouched until it); false: not a candidate, launch it with spconv_backward_weight.
struct WgradGroupBuilder;
WgradGroupBuilder* wgrad_group_create();
void wgrad_group_destroy(WgradGroupBuilder* b);
int wgrad_group_size(const WgradGroupBuilder* b);
void wgrad_group_drop(WgradGroupBuilder* b);  // forget what was collected (a backward pass that failed half-way)
bool wgrad_group_add(WgradGroupBuilder* b, const float* in, int64_t in_ld, int64_t n_in, int cin, const float* gout,
                     int64_t gout_ld, int64_t n_out, int cout, const pcmi_kmap_t* map, float* gweight, int accumulate,
                     hipStream_t st);
int wgrad_group_flush(WgradGroupBuilder* b, hipStream_t st);

// ---- BatchNorm (norm.hip): ONE training-forward and ONE backward entry point for one- and two-segment row sets ----------
// Rows [0, split) and [split, n) are two segments with their own statistics (the two clouds of a pair in one sparse tensor);
// split == n: one segment.  The kernels are the same either way (gridDim.y, seg_split and the *_stride arguments); what
// differs between the two forms is decided in norm.hip (bn_path and the numbered notes (1)-(5) beside it):
//   (1) row blocks: red_geom(n), the wide final kernels beyond kFinalMergeBlocks | red_geom(longest segment) re-cut to
//       <= kFinalMergeBlocks blocks, always colreduce_final_kernel;
//   (2) parameter gradients are accumulated (acc_*) in the merge | in the apply launch;
//   (3) running estimates: updated by the merge when the pointers are given | never (BnRunningUpdate with mean2);
//   (4) the lean backward statistics are chosen by the TOTAL row count in both forms;
//   (5) statistics / sums of the second segment lie stat_stride / 2 c floats behind the first's | strides 0.
// relu_bits (nullable, norm.hip "relu_bits"): the ReLU pattern of a fused BatchNorm(+residual)+ReLU output as one bit per
// element, [rows][c / 32] words, c a multiple of 32 -- written by the forward when relu != 0, read by the backward INSTEAD
// of relu_mask_y (which may then be null).
struct BnTrainForward {
  const float* x; int64_t x_ld;
  const float* residual; int64_t res_ld;  // nullable
  float* y; int64_t y_ld;
  int64_t n, split;
  int c;
  const float* gamma; const float* beta;
  float eps;
  int relu;
  float* save_mean; float* save_invstd;
  float* save_unbiased;  // nullable
  int stat_stride;       // two segments: floats from a save_* block of segment 0 to that of segment 1
  // one segment only, nullable: updated in place.  Null with save_unbiased set: the executor applies the update later, in
  // program order, with bn_running_update (two passes forwarded concurrently, and every two-segment pass).
  float* running_mean; float* running_var;
  float momentum;
  uint32_t* relu_bits;   // nullable
};
int bn_forward_train(const BnTrainForward& a, void* ws, size_t ws_bytes, hipStream_t st);

struct BnBackwardArgs {
  const float* dy; int64_t dy_ld;
  const float* x; int64_t x_ld;
  const float* relu_mask_y; int64_t y_ld;  // nullable: no ReLU (or relu_bits)
  int64_t n, split;
  int c;
  const float* gamma; const float* save_mean; const float* save_invstd;
  int stat_stride;  // as in the forward
  float* dx; int64_t dx_ld;
  float* dres; int64_t dres_ld;  // nullable: gradient of the residual, stored or (dres_accumulate) added to
  int dres_accumulate;
  // this call's sums (scratch, overwritten): EITHER dgamma and dbeta, c floats each (one segment: the C ABI), OR `sums`,
  // 2 c floats per segment, laid out inside: [dgamma | dbeta] for one segment, [segment][dbeta | dgamma] for two
  float* dgamma; float* dbeta;
  float* sums;
  float* acc_dgamma; float* acc_dbeta;  // nullable: += the sums (segment 0, then segment 1)
  const uint32_t* relu_bits;            // nullable
};
int bn_backward(const BnBackwardArgs& a, void* ws, size_t ws_bytes, hipStream_t st);

// deferred running-estimate update of one BatchNorm layer: running = (1 - momentum) * running + momentum * batch
struct BnRunningUpdate {
  float* running_mean;
  float* running_var;
  const float* mean;
  const float* unbiased;
  int c;
  float momentum;
  const float* mean2;      // nullable: statistics of the second segment of a two-segment pass, applied after the first
  const float* unbiased2;
};
int bn_running_update(const BnRunningUpdate* table_dev, int n_entries, hipStream_t st);

// coords.hip: a cached map as it is -- M == -1 / offs_host unset when pcmi_coords_plan_unet built it and nobody has asked
// for the counts yet (the kernels size their launches by bounds and read the device-side offsets); and the ordering of a
// consumer stream behind the handle's last plan
int kmap_get_nosync(pcmi_coords_t* h, int in_key, int out_key, int kernel_size, int stride, int region, pcmi_kmap_t* out,
                    pcmi_stream_t stream);
int coords_wait_plan(pcmi_coords_t* h, hipStream_t st);
// pairs of a map as far as the host knows: exact once the counts have arrived, else the bound (every output row of a
// stride-1 map has at most K neighbours; every fine row of a stride-2 map exactly one parent)
static inline int64_t kmap_pairs_bound(const pcmi_kmap_t& m) {
  return m.M >= 0 ? m.M : (m.stride == 1 ? (int64_t)m.K * m.n_out : m.n_in);
}

// The calling thread's convolution arithmetic (spconv.hip; pcmi_set_conv_precision, and the executor for the duration of
// a pass): PCMI_CONV_PRECISION_FP32 or _BF16.  conv_terms(): the bf16 terms per operand element the split-precision
// kernels (spconv16x_kernel, wgrad_x3t / x3p_kernel) use in that mode.  Every other kernel ignores it.
int conv_precision();
void conv_precision_set(int precision);  // precision already validated
static inline int conv_terms() { return conv_precision() == PCMI_CONV_PRECISION_BF16 ? 1 : 3; }
// Sets the calling thread's mode for a scope and restores the previous one.
struct ConvPrecisionScope {
  explicit ConvPrecisionScope(int precision) : saved(conv_precision()) { conv_precision_set(precision); }
  ~ConvPrecisionScope() { conv_precision_set(saved); }
  ConvPrecisionScope(const ConvPrecisionScope&) = delete;
  ConvPrecisionScope& operator=(const ConvPrecisionScope&) = delete;
  int saved;
};

// spconv_wgrad_x3.hip: weight gradients of the 3^3 / stride-1 convolutions, output-tile stationary on the bf16 matrix cores
struct WgradPlan;  // spconv_wgrad_plan.h: plan_wgrad decides which calls take these kernels and sizes their launches
int wgrad_x3t_run(const float* in, int64_t in_ld, const float* gout, int64_t gout_ld, int64_t n_rows, int cin, int cout,
                  const pcmi_kmap_t* map, const WgradPlan& plan, float* gweight, int accumulate, void* ws, hipStream_t st);

// nce_x3.hip: PointInfoNCE forward / backward on the bf16 matrix cores (three-term split); c in {16, 32}, q / k contiguous
// and 16-byte aligned, ws of pcmi_nce_workspace_bytes and 16-byte aligned.  PCMI_NCE_X3=0 keeps the fp32 VALU kernels of loss.hip.
bool nce_x3_on();
size_t nce_x3_workspace_bytes(int64_t n);
int nce_x3_fwd(const float* q, const float* k, int64_t n, int c, float inv_T, float* lse, float* loss, void* ws, hipStream_t st);
int nce_x3_bwd(const float* q, const float* k, const float* lse, int64_t n, int c, float inv_T, const float* gscale, float* dq,
               float* dk, void* ws, hipStream_t st);

size_t sort_rows_temp_bytes(int64_t n);
int sort_rows_by_mask(const int32_t* nbr, int K, int64_t n, int64_t chunk_rows, uint32_t* mask_in, uint32_t* mask_out,
                      int32_t* iota, void* temp, size_t temp_bytes, int32_t* perm, int32_t* nbr_perm, hipStream_t st);
int tile_units(const uint32_t* sorted_key, int K, int64_t n, uint32_t* tile_mask, int32_t* cnt, int32_t* tile_pref,
               hipStream_t st);
// rows of the contiguous tile range one XCD processes (tile swizzle of the conv kernel, 128-row tiles)
static inline int64_t xcd_chunk_rows(int64_t n) { return ceil_div(ceil_div(n, 128), 8) * 128; }

// pointset.hip: the inverse lists of an index tensor idx [B, L] with targets in [0, N) -- integer count, scan and a stable
// radix placement by flat source position: the sources p = b L + l of target (b, t) are pos[start[b N + t] ..
// start[b N + t + 1]) in ascending p; an index outside the range is dropped.  B L and B N in [1, 2^31 - 1); start / pos
// point into ws (inverse_lists_workspace bytes) and stay valid until it is reused.  No synchronisation.
size_t inverse_lists_workspace(int64_t n_idx, int64_t n_targets);
int inverse_lists(const char* who, const int32_t* idx, int64_t B, int64_t L, int64_t N, void* ws, size_t ws_bytes,
                  const int32_t** start, const int32_t** pos, hipStream_t st);

// n zero-initialised arrival counters (common.h: arrive_last) for launches on `st`: one pool per stream -- launches
// on a stream are serialised and every kernel leaves its counters at zero.  nullptr on allocation failure.
unsigned* stream_counters(hipStream_t st, size_t n);

// A caller's workspace cut into typed pieces, each rounded up to `align` bytes.  A null base measures: take() returns
// nullptr and only `used` advances.  Every entry point that carves two or more pieces has ONE static layout function
// beside it, layout(base, shape...) -> a struct of typed pointers plus `bytes` (= used): the size query is
// layout(nullptr, shape...).bytes and the entry point checks that many bytes (require_ws) before it calls layout(ws, ...),
// so the byte count and the pointers come out of the same lines.
struct Carve {
  char* base;
  size_t align = 256;
  size_t used = 0;
  template <class T>
  T* take(size_t count) {
    T* r = base ? reinterpret_cast<T*>(base + used) : nullptr;
    used += align_up(count * sizeof(T), align);
    return r;
  }
};

// The workspace check of the C entry points (`if (int rc = require_ws(...)) return rc;`): null or short -> PCMI_ERR_WORKSPACE,
// then a base that is not `align`-byte aligned -> PCMI_ERR_INVALID (align 1: no requirement).
static inline int require_ws(const char* who, const void* ws, size_t ws_bytes, size_t need, size_t align) {
  PCMI_REQUIRE(ws && ws_bytes >= need, PCMI_ERR_WORKSPACE, "%s: workspace too small (%zu bytes, %zu needed)", who, ws_bytes, need);
  PCMI_REQUIRE((uintptr_t)ws % align == 0, PCMI_ERR_INVALID, "%s: workspace must be %zu-byte aligned", who, align);
  return PCMI_OK;
}

// compute units of the current device (cached; 256 on MI355X)
static inline int num_cu() {
  static int n = 0;
  if (n == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n = prop.multiProcessorCount;
    if (n <= 0) n = 256;
  }
  return n;
}

}  // namespace pcmi
