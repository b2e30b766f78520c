// Span-extraction head of --task question-answering: the softmax along the SEQUENCE, its loss, the best span and the
// per-row gradient table, after the classifier pass of token_head.hip.
//
//   HF: BertForQuestionAnswering / RobertaForQuestionAnswering / DistilBertForQuestionAnswering
//       logits = qa_outputs(dropout(sequence_output)) [rows, 2]; column 0 = start logit, column 1 = end logit;
//       CrossEntropyLoss over the positions of each sequence, once per column, averaged.
//
//   logits   tok_fwd_kernel in its logits-only mode with C = 2 (launch_token_head_fwd, labels = null): the one
//            streaming pass over h, bf16 logits [R][2].
//   span_ce_kernel    one 256-thread workgroup per sequence b (rows cu[b] .. cu[b+1]-1, an optional per-row mask
//            takes rows out: the padded layout is cu = arange(B+1)·S plus the flat attention mask). The sequence's two
//            logit columns go to LDS once (fp32, -inf on the masked rows: 8 KB at the 1,024-row limit); per column
//            max, Σ exp, lse = max + log Σ and the target logit; best span = first maximum in (s, e) order of
//            start[s] + end[e] (one fp32 add of the bf16-rounded logits) over real rows with
//            s <= e <= s + max_answer_length - 1. A position is ignored when it is < 0, >= the segment length or on
//            a masked row. Per sequence: record {loss_start, loss_end, valid_start, valid_end, hit, both valid,
//            start hit, end hit} and pred [2]; with labels also g0 [R][2] fp32 = softmax - onehot, exact zeros on
//            masked rows, on the columns whose position is ignored and (last workgroup) on the rows past cu[B].
//   span_stats_kernel one workgroup: the B records summed in index order ->
//            stats [8] = {loss, hits, n, loss·n, n_start, n_end, start hits, end hits},
//            loss = ½ (Σ loss_start / max(n_start, 1) + Σ loss_end / max(n_end, 1)).
//   backward launch_token_head_bwd_given (token_head.hip, tok_bwd_kernel<true>):
//            g[row][c] = g0[row][c] · dloss · ½ / max(n_c, 1) with n_c = stats[4 + c]; from g on it is the
//            token-classification backward (dh once per row, fp32 slabs, fixed-order reducer into main_grad).
//
// No atomics and no memset: every output element has one writer, so two runs give the same bits. A sequence longer
// than 1,024 rows does not fit the LDS image: its record carries a NaN loss (the loss is then NaN, loudly) and its
// rows of g0 are zero; the callers (ops/hip.py qa_head_ok) keep such batches on the composed path.
//
// hipcc -Rpass-analysis=kernel-resource-usage (gfx950, -O3):
//   span_ce_kernel     22 VGPRs, scratch 0, LDS 8,256 B;  span_stats_kernel 39 VGPRs, scratch 0, LDS 8,224 B
#include "common.h"
#include "launchers.h"

namespace hsd {
namespace qa {

constexpr int MAXL = 1024;  // rows of one sequence held in LDS

// max / sum over the 256 threads of the workgroup; red holds one float per wave. Every thread gets the result.
__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  return v;
}

__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return v;
}

__global__ __launch_bounds__(256) void span_ce_kernel(const bf16_t* __restrict__ logits, const int* __restrict__ cu,
                                                      const int64_t* __restrict__ mask,
                                                      const int64_t* __restrict__ pos, int max_len,
                                                      float* __restrict__ rec, int* __restrict__ pred,
                                                      float* __restrict__ g0, int R, int B) {
  __shared__ float sl[2][MAXL];
  __shared__ float red[4];
  __shared__ float bsc[4];
  __shared__ int bss[4], bse[4];
  const int b = blockIdx.x, t = threadIdx.x;
  // the segment, clamped to the buffer (nothing below indexes outside [0, R) whatever cu holds)
  int start = cu[b], stop = cu[b + 1];
  start = min(max(start, 0), R);
  stop = min(max(stop, start), R);
  const int Lraw = stop - start;
  const bool too_long = Lraw > MAXL;
  const int L = min(Lraw, MAXL);

  float m0 = -INFINITY, m1 = -INFINITY;
  for (int i = t; i < L; i += 256) {
    const int row = start + i;
    const bool real = mask == nullptr || mask[row] != 0;
    const uint32_t w = *reinterpret_cast<const uint32_t*>(logits + 2 * (int64_t)row);
    const float a = real ? lo_bf(w) : -INFINITY, e = real ? hi_bf(w) : -INFINITY;
    sl[0][i] = a;
    sl[1][i] = e;
    m0 = fmaxf(m0, a);
    m1 = fmaxf(m1, e);
  }
  m0 = block_max(m0, red);  // (its barriers also publish sl)
  m1 = block_max(m1, red);
  const bool has_real = m0 > -INFINITY || m1 > -INFINITY;
  const float z0 = m0 > -INFINITY ? m0 : 0.f, z1 = m1 > -INFINITY ? m1 : 0.f;
  float s0 = 0.f, s1 = 0.f;
  for (int i = t; i < L; i += 256) {
    s0 += __expf(sl[0][i] - z0);  // exp(-inf) = 0 on the masked rows
    s1 += __expf(sl[1][i] - z1);
  }
  s0 = block_sum(s0, red);
  s1 = block_sum(s1, red);
  const float lse0 = z0 + __logf(s0), lse1 = z1 + __logf(s1);

  // labels
  int p0 = -1, p1 = -1;
  bool v0 = false, v1 = false;
  if (pos != nullptr && has_real && !too_long) {
    const int64_t q0 = pos[2 * (int64_t)b], q1 = pos[2 * (int64_t)b + 1];
    if (q0 >= 0 && q0 < L && (mask == nullptr || mask[start + q0] != 0)) { v0 = true; p0 = (int)q0; }
    if (q1 >= 0 && q1 < L && (mask == nullptr || mask[start + q1] != 0)) { v1 = true; p1 = (int)q1; }
  }

  if (g0 != nullptr) {
    for (int i = t; i < Lraw; i += 256) {
      const int row = start + i;
      float ga = 0.f, ge = 0.f;
      if (i < L && (mask == nullptr || mask[row] != 0)) {
        if (v0) ga = __expf(sl[0][i] - lse0) - (i == p0 ? 1.f : 0.f);
        if (v1) ge = __expf(sl[1][i] - lse1) - (i == p1 ? 1.f : 0.f);
      }
      *reinterpret_cast<float2*>(g0 + 2 * (int64_t)row) = float2{ga, ge};
    }
    if (b == B - 1)  // the dead rows of a packed buffer
      for (int row = stop + t; row < R; row += 256) *reinterpret_cast<float2*>(g0 + 2 * (int64_t)row) = float2{0.f, 0.f};
    if (b == 0)
      for (int row = t; row < start; row += 256) *reinterpret_cast<float2*>(g0 + 2 * (int64_t)row) = float2{0.f, 0.f};
  }

  // best span: this thread's start rows in increasing order, strict > keeps the first maximum
  float best = -INFINITY;
  int bs = 0, be = 0;
  for (int s = t; s < L; s += 256) {
    const float a = sl[0][s];
    if (!(a > -INFINITY)) continue;
    const int n = min(L - s, max(max_len, 1));  // e = s .. s + n - 1
    for (int e = s; e < s + n; ++e) {
      const float sc = a + sl[1][e];
      if (sc > best) { best = sc; bs = s; be = e; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int os = __shfl_xor(bs, o, 64), oe = __shfl_xor(be, o, 64);
    if (ob > best || (ob == best && os < bs)) { best = ob; bs = os; be = oe; }
  }
  if ((t & 63) == 0) { bsc[t >> 6] = best; bss[t >> 6] = bs; bse[t >> 6] = be; }
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int w = 1; w < 4; ++w)
      if (bsc[w] > best || (bsc[w] == best && bss[w] < bs)) { best = bsc[w]; bs = bss[w]; be = bse[w]; }
    if (!(best > -INFINITY)) bs = be = 0;
    pred[2 * b] = bs;
    pred[2 * b + 1] = be;
    if (rec != nullptr) {
      float* const r = rec + 8 * (int64_t)b;
      const float nan = __uint_as_float(0x7fc00000u);
      r[0] = too_long ? nan : (v0 ? lse0 - sl[0][p0] : 0.f);
      r[1] = too_long ? nan : (v1 ? lse1 - sl[1][p1] : 0.f);
      r[2] = v0 ? 1.f : 0.f;
      r[3] = v1 ? 1.f : 0.f;
      r[4] = v0 && v1 && bs == p0 && be == p1 ? 1.f : 0.f;
      r[5] = v0 && v1 ? 1.f : 0.f;
      r[6] = v0 && bs == p0 ? 1.f : 0.f;
      r[7] = v1 && be == p1 ? 1.f : 0.f;
    }
  }
}

// stats = {loss, hits, n, loss·n, n_start, n_end, start hits, end hits}. The records pass through LDS 256 at a time
// (coalesced loads); field k is summed by thread k in index order.
constexpr int STATS_CHUNK = 256;
__global__ __launch_bounds__(256) void span_stats_kernel(const float* __restrict__ rec, int B,
                                                         float* __restrict__ stats) {
  __shared__ float buf[STATS_CHUNK * 8];
  __shared__ float tot[8];
  float s = 0.f;
  for (int b0 = 0; b0 < B; b0 += STATS_CHUNK) {
    const int nb = min(STATS_CHUNK, B - b0);
    for (int i = threadIdx.x; i < nb * 8; i += 256) buf[i] = rec[8 * (int64_t)b0 + i];
    __syncthreads();
    if (threadIdx.x < 8) {
#pragma unroll 8
      for (int b = 0; b < nb; ++b) s += buf[8 * b + threadIdx.x];
    }
    __syncthreads();
  }
  if (threadIdx.x < 8) tot[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float loss = 0.5f * (tot[0] / fmaxf(tot[2], 1.0f) + tot[1] / fmaxf(tot[3], 1.0f));
    stats[0] = loss;
    stats[1] = tot[4];
    stats[2] = tot[5];
    stats[3] = loss * tot[5];
    stats[4] = tot[2];
    stats[5] = tot[3];
    stats[6] = tot[6];
    stats[7] = tot[7];
  }
}

}  // namespace qa

void launch_span_ce(const bf16_t* logits, const int* cu, const int64_t* mask, const int64_t* pos, int max_answer_length,
                    float* rec, int* pred, float* g0, float* stats, int R, int B, hipStream_t st) {
  hipLaunchKernelGGL(qa::span_ce_kernel, dim3(B), dim3(256), 0, st, logits, cu, mask, pos, max_answer_length,
                     pos != nullptr ? rec : nullptr, pred, pos != nullptr ? g0 : nullptr, R, B);
  HSD_CHECK_LAUNCH();
  if (pos != nullptr) {
    hipLaunchKernelGGL(qa::span_stats_kernel, dim3(1), dim3(256), 0, st, (const float*)rec, B, stats);
    HSD_CHECK_LAUNCH();
  }
}

}  // namespace hsd
