// The validation loop of the semantic-segmentation fine-tuning (downstream/semseg/lib/test.py:62-196 of the reference) per
// batch, on the device: get_prediction, CrossEntropyLoss(ignore_index), precision_at_one and fast_hist (lib/test.py:119,
// 137-140, lib/utils.py:117-133) in ONE pass over the logits, which also leaves the softmax probabilities class-major for
// the per-class sort; and average_precision (lib/test.py:55-59,143-145) of every class from the sorted probabilities.
// Written from the semantics in include/pcmi.h; gfx950, wave64.
//
// Arithmetic: exponentials and probabilities are float32 (the sum of a row's exponentials is kept in float64, classes in
// ascending order, so a row's probabilities depend on that row alone); counts are integers; the loss sum, recall, precision and
// AP are float64, summed in a fixed order.  The only atomics are integer adds (confusion matrix, positives per class): every
// output is reproducible bit for bit.
#include <algorithm>

#include "blockscan.h"
#include "internal.h"

#pragma clang fp contract(off)

namespace pcmi {
namespace segeval {

constexpr int kMaxClasses = 64;  // the workgroup's private confusion matrix: 64 x 64 x 4 bytes = 16 KB of LDS
constexpr int kRowThreads = 256;

struct RowPartial {  // one per workgroup of seg_rows_kernel
  double loss;       // sum of the counted rows' losses
  int32_t counted;   // rows with label != ignore
  int32_t correct;   // of those, rows with pred == label
};

// One thread per row (softmax_ce_fwd's mapping: a wave reads 64 consecutive rows, and writes 64 consecutive elements of a
// class's row of prob_t).  The workgroup counts its rows' (label, pred) pairs in LDS and adds the non-zero cells to hist with
// integer atomics; its (loss, counted, correct) go to part[block], and the last workgroup to arrive merges the partials in block
// order -- strided over its threads, then one tree -- into batch4 and the running totals3.
__global__ __launch_bounds__(kRowThreads) void seg_rows_kernel(const float* __restrict__ x, int64_t ld, int64_t n, int c,
                                                               const int32_t* __restrict__ label, int ignore,
                                                               int32_t* __restrict__ pred, float* __restrict__ prob_t,
                                                               unsigned long long* __restrict__ hist, RowPartial* part,
                                                               unsigned* counter, double* __restrict__ batch4,
                                                               double* __restrict__ totals3) {
  __shared__ int s_hist[kMaxClasses * kMaxClasses];
  __shared__ double s_loss[kRowThreads];
  __shared__ long long s_counted[kRowThreads], s_correct[kRowThreads];
  __shared__ unsigned s_last;
  const int tid = threadIdx.x;
  for (int e = tid; e < c * c; e += kRowThreads) s_hist[e] = 0;
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * kRowThreads + tid;
  double loss = 0.0;
  int counted = 0, correct = 0;
  if (r < n) {
    const float* xr = x + r * ld;
    float m = xr[0];
    int am = 0;
    for (int j = 1; j < c; ++j) {  // strict >: the lowest index of equal logits
      const float v = xr[j];
      if (v > m) {
        m = v;
        am = j;
      }
    }
    double se = 0.0;
    for (int j = 0; j < c; ++j) se = se + (double)expf(xr[j] - m);
    const float sef = (float)se;
    pred[r] = am;
    if (prob_t)
      for (int j = 0; j < c; ++j) prob_t[(int64_t)j * n + r] = expf(xr[j] - m) / sef;
    const int32_t lb = label[r];
    const bool is_class = lb >= 0 && lb < c;
    if (is_class) atomicAdd(&s_hist[lb * c + am], 1);
    if (lb != ignore) {
      counted = 1;
      // a label that is neither a class nor the ignore label poisons the batch loss (ce_fwd_kernel, loss.hip)
      // (float64 logarithm of the float64 sum: a confident row's loss is log(1 + a few 1e-5), lost in a float32 sum near 1)
      loss = is_class ? ((double)m + log(se)) - (double)xr[lb] : (double)__builtin_nanf("");
      correct = (is_class && am == lb) ? 1 : 0;
    }
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    loss = loss + __shfl_xor(loss, d, 64);
    counted += __shfl_xor(counted, d, 64);
    correct += __shfl_xor(correct, d, 64);
  }
  if ((tid & 63) == 0) {
    s_loss[tid >> 6] = loss;
    s_counted[tid >> 6] = counted;
    s_correct[tid >> 6] = correct;
  }
  __syncthreads();  // (also: every count of this workgroup is in s_hist)
  for (int e = tid; e < c * c; e += kRowThreads) {
    const int v = s_hist[e];
    if (v) atomicAdd(&hist[e], (unsigned long long)v);
  }
  if (tid == 0) {
    RowPartial p;
    p.loss = ((s_loss[0] + s_loss[1]) + s_loss[2]) + s_loss[3];
    p.counted = (int32_t)(s_counted[0] + s_counted[1] + s_counted[2] + s_counted[3]);
    p.correct = (int32_t)(s_correct[0] + s_correct[1] + s_correct[2] + s_correct[3]);
    part[blockIdx.x] = p;
  }
  if (!arrive_last(counter, gridDim.x, &s_last)) return;
  double l = 0.0;
  long long cn = 0, co = 0;
  for (unsigned b = tid; b < gridDim.x; b += kRowThreads) {
    const RowPartial p = part[b];
    l = l + p.loss;
    cn += p.counted;
    co += p.correct;
  }
  s_loss[tid] = l;
  s_counted[tid] = cn;
  s_correct[tid] = co;
  __syncthreads();
  for (int o = kRowThreads / 2; o > 0; o >>= 1) {
    if (tid < o) {
      s_loss[tid] = s_loss[tid] + s_loss[tid + o];
      s_counted[tid] += s_counted[tid + o];
      s_correct[tid] += s_correct[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double nd = (double)n, cnt = (double)s_counted[0], cor = (double)s_correct[0];
    batch4[0] = s_loss[0];
    batch4[1] = cnt;
    batch4[2] = cor;
    batch4[3] = nd;
    // AverageMeter.update(value, num_sample) of lib/test.py:138-139, for both meters; a batch without a counted row has
    // neither a loss nor a score and adds nothing
    if (totals3 && s_counted[0] > 0) {
      totals3[0] = totals3[0] + nd * (s_loss[0] / cnt);
      totals3[1] = totals3[1] + nd * ((100.0 * cor) / cnt);
      totals3[2] = totals3[2] + nd;
    }
  }
}

// ---- per-class average precision ----------------------------------------------------------------------------------------------
constexpr int kApThreads = 1024;
constexpr int kApWaves = kApThreads / 64;
constexpr int kApItems = 4;
constexpr int kApChunk = kApThreads * kApItems;  // sorted elements one pass of the workgroup covers

// npos[k] = rows with label == k: private counts in LDS, flushed with integer atomics
__global__ __launch_bounds__(256) void seg_npos_kernel(const int32_t* __restrict__ label, int64_t n, int c, int32_t* __restrict__ npos) {
  __shared__ int s_cnt[kMaxClasses];
  const int tid = threadIdx.x;
  if (tid < c) s_cnt[tid] = 0;
  __syncthreads();
  for (int64_t r = (int64_t)blockIdx.x * 256 + tid; r < n; r += (int64_t)gridDim.x * 256) {
    const int32_t lb = label[r];
    if (lb >= 0 && lb < c) atomicAdd(&s_cnt[lb], 1);
  }
  __syncthreads();
  if (tid < c && s_cnt[tid]) atomicAdd(&npos[tid], s_cnt[tid]);
}

// grid (class), one workgroup each, over the class's n scores in descending order, kApChunk at a time with a carry (so n may
// be anything): positive flag = "the row's label is this class", inclusive count of positives tp; an element is a threshold
// if it is the last of its run of equal scores (it differs from its successor, or is the last of all); a threshold where tp
// grew since the previous threshold adds (tp / npos - tp_prev / npos) (tp / rank).  The carry: tp so far and tp at the last
// threshold so far (tp never decreases, so "the previous threshold's tp" is a running maximum).  Per thread the terms are
// added in rank order, then one tree sum in a fixed order.
__global__ __launch_bounds__(kApThreads) void seg_ap_kernel(const float* __restrict__ sorted_prob, const int64_t* __restrict__ order,
                                                            const int32_t* __restrict__ label, const int32_t* __restrict__ npos,
                                                            int64_t n, double* __restrict__ ap, double* __restrict__ ap_sum,
                                                            long long* __restrict__ ap_cnt) {
  __shared__ int s_int[kApWaves];
  __shared__ double s_sum[kApThreads];
  const int tid = threadIdx.x;
  const int k = blockIdx.x;
  const float* s = sorted_prob + (int64_t)k * n;
  const int64_t* ord = order + (int64_t)k * n;
  const double np = (double)npos[k];
  double sum = 0.0;
  int carry_tp = 0, carry_prev = 0;
  for (int64_t base = 0; base < n; base += kApChunk) {
    int f[kApItems], end[kApItems], local = 0;
#pragma unroll
    for (int q = 0; q < kApItems; ++q) {
      const int64_t i = base + (int64_t)tid * kApItems + q;
      f[q] = 0;
      end[q] = 0;
      if (i < n) {
        const int64_t row = ord[i];
        f[q] = (row >= 0 && row < n && label[row] == k) ? 1 : 0;
        end[q] = (i + 1 == n || s[i] != s[i + 1]) ? 1 : 0;
      }
      local += f[q];
    }
    int total, top;
    int tp = carry_tp + block_scan_add<kApWaves>(local, s_int, &total) - local;
    int tpq[kApItems], last_end = 0;
#pragma unroll
    for (int q = 0; q < kApItems; ++q) {
      tp += f[q];
      tpq[q] = tp;
      last_end = end[q] ? tp : last_end;
    }
    int prev = max(carry_prev, block_scan_max_excl<kApWaves>(last_end, s_int, &top));
#pragma unroll
    for (int q = 0; q < kApItems; ++q) {
      const int64_t i = base + (int64_t)tid * kApItems + q;
      if (end[q]) {
        if (tpq[q] > prev) sum = sum + (((double)tpq[q] / np) - ((double)prev / np)) * ((double)tpq[q] / (double)(i + 1));
        prev = tpq[q];
      }
    }
    carry_tp += total;
    carry_prev = max(carry_prev, top);
  }
  s_sum[tid] = sum;
  __syncthreads();
  for (int o = kApThreads / 2; o > 0; o >>= 1) {
    if (tid < o) s_sum[tid] = s_sum[tid] + s_sum[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    // a class without a positive row: recall is 0 / 0 at every threshold (np.nanmean of lib/test.py:149 skips the batch)
    const bool scored = npos[k] > 0;
    ap[k] = scored ? s_sum[0] : (double)__builtin_nanf("");
    if (scored && ap_sum) ap_sum[k] = ap_sum[k] + s_sum[0];
    if (scored && ap_cnt) ap_cnt[k] += 1;
  }
}

static bool rows_shape_ok(int64_t n, int c) { return n >= 0 && n < (1ll << 31) - kRowThreads && c >= 1 && c <= kMaxClasses; }

}  // namespace segeval
}  // namespace pcmi

using namespace pcmi;
using namespace pcmi::segeval;

extern "C" {

size_t pcmi_seg_eval_rows_workspace_bytes(int64_t n) {
  if (n < 0) return 0;
  return align_up((size_t)ceil_div(n > 0 ? n : 1, kRowThreads) * sizeof(RowPartial), 256);
}

int pcmi_seg_eval_rows(const float* logits, int64_t ld, int64_t n, int c, const int32_t* labels, int ignore_label, int32_t* pred,
                       float* prob_t, int64_t* hist, double* batch4, double* totals3, void* ws, size_t ws_bytes,
                       pcmi_stream_t stream) {
  PCMI_REQUIRE(rows_shape_ok(n, c), PCMI_ERR_INVALID, "seg_eval_rows: bad shape (n %lld, c %d; 1 <= c <= %d)", (long long)n, c,
               kMaxClasses);
  PCMI_REQUIRE(ld >= c, PCMI_ERR_INVALID, "seg_eval_rows: leading dimension %lld below the %d classes", (long long)ld, c);
  if (n == 0) return PCMI_OK;
  PCMI_REQUIRE(logits && labels && pred && hist && batch4, PCMI_ERR_INVALID, "seg_eval_rows: null pointer");
  if (int rc = require_ws("seg_eval_rows", ws, ws_bytes, pcmi_seg_eval_rows_workspace_bytes(n), 8)) return rc;
  hipStream_t st = as_stream(stream);
  unsigned* counter = stream_counters(st, 1);
  if (!counter) return PCMI_ERR_HIP;
  seg_rows_kernel<<<(unsigned)ceil_div(n, kRowThreads), kRowThreads, 0, st>>>(
      logits, ld, n, c, labels, ignore_label, pred, prob_t, reinterpret_cast<unsigned long long*>(hist), static_cast<RowPartial*>(ws),
      counter, batch4, totals3);
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

size_t pcmi_seg_ap_workspace_bytes(int c) {
  if (c < 1 || c > kMaxClasses) return 0;
  return align_up((size_t)c * sizeof(int32_t), 256);
}

int pcmi_seg_ap(const float* sorted_prob, const int64_t* order, const int32_t* labels, int64_t n, int c, double* ap, double* ap_sum,
                int64_t* ap_cnt, void* ws, size_t ws_bytes, pcmi_stream_t stream) {
  PCMI_REQUIRE(rows_shape_ok(n, c), PCMI_ERR_INVALID, "seg_ap: bad shape (n %lld, c %d; 1 <= c <= %d)", (long long)n, c, kMaxClasses);
  PCMI_REQUIRE(ap && (n == 0 || (sorted_prob && order && labels)), PCMI_ERR_INVALID, "seg_ap: null pointer");
  if (int rc = require_ws("seg_ap", ws, ws_bytes, pcmi_seg_ap_workspace_bytes(c), 4)) return rc;
  hipStream_t st = as_stream(stream);
  int32_t* npos = static_cast<int32_t*>(ws);
  PCMI_HIP_CHECK(hipMemsetAsync(npos, 0, (size_t)c * sizeof(int32_t), st));
  if (n > 0) {
    seg_npos_kernel<<<(unsigned)std::min<int64_t>(ceil_div(n, 256), 256), 256, 0, st>>>(labels, n, c, npos);
    PCMI_LAUNCH_CHECK();
  }
  seg_ap_kernel<<<(unsigned)c, kApThreads, 0, st>>>(sorted_prob, order, labels, npos, n, ap, ap_sum,
                                                    reinterpret_cast<long long*>(ap_cnt));
  PCMI_LAUNCH_CHECK();
  return PCMI_OK;
}

}  // extern "C"
