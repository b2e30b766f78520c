// Fused token-classification head (--task token-classification): the classifier over EVERY encoder row, with its
// dropout, cross-entropy and accuracy, in one forward and one backward kernel plus two small reducers.
//
//   HF: BertForTokenClassification / RobertaForTokenClassification / DistilBertForTokenClassification
//       logits = classifier(dropout(sequence_output)), CrossEntropyLoss over the rows whose label is not -100.
//
//   forward   d       = bf16(h · keep · 1/(1-p))      the hash dropout of ops/rng.py, element (row, col) of [R, H]
//             logits  = bf16(d·Wᵀ + b)                [R, C], 2 <= C <= 16
//             per valid row: logsumexp(logits) - logits[label], first-maximum argmax hit (from the rounded logits)
//             per-block partial sums -> head_stats_kernel (head_stats.hip) -> stats = {mean loss, hits, n_valid,
//             loss sum}
//   backward  g       = (softmax(logits) - onehot(label)) · dloss / max(n_valid, 1)      0 on ignored rows
//   label smoothing eps > 0 (--label_smoothing_factor; the kSmooth instantiations, eps a host constant of the launch):
//             loss = lse - (1-eps)·logits[label] - (eps/C)·Σ_c logits[c],  g = (softmax - (1-eps)·onehot - eps/C) · ...
//             over the C real classes; everything from g on is the same code. eps = 0 launches the <false> forms.
//             dh      = bf16((g·W) · keep · 1/(1-p))   every row written once, 16-byte stores
//             dW, db  : per-block fp32 partial slabs [C][H] + [C] -> tok_reduce_kernel adds them in a fixed order
//                       INTO the gradient buffers (+=: main_grad accumulates over micro-batches). No float atomics, so
//                       two runs give the same bits.
//
// Matrix cores, not VALU dot products. The products here are [R, H] x [H, C] with C <= 16: on the VALU a wave-per-row
// GEMV needs C cross-lane reductions per row (6 shuffle steps each) and the backward's dW accumulators are C x 16
// fp32 per lane (256 registers at C = 16, the cls_head.hip layout); with the class dimension padded to 16 one MFMA
// sums over the hidden (forward) or the row (dW) dimension with no shuffle at all, and the accumulators of a 16-row
// tile are 4 registers (forward) or, for dW, split by COLUMNS over the 4 waves of a block: 64 registers per lane at
// H = 1024. The forward uses gfx950's mfma_f32_16x16x32_bf16 (K = 32 hidden columns), the backward
// mfma_f32_16x16x16_bf16 (K = 16 classes for dh, K = 16 rows for dW). The padding classes hold zeros.
//
// Tile = 16 consecutive rows. Lane l of a wave: r = l & 15 (row of the tile), q = l >> 4. In 32-column slice s the
// lane owns the 8 columns s·32 + q·8 .. +7 of its row: one 16-byte load (forward and backward), one 16-byte store
// (dh), and exactly the 16x16x32 operand map (k = 8q + j), so h goes from the load to the MFMA through the dropout
// arithmetic only. The logits come out as lane (row r, classes 4q .. 4q+3); softmax statistics cross 4 lanes (xor 16,
// xor 32).
//
// W on chip: the forward keeps W (classes padded to 16, rows padded by 16 B against bank conflicts) in LDS for the
// whole kernel, 33 KB per block; the backward keeps Wᵀ [H][16] (40-byte rows) in LDS, 40 KB. Both kernels are
// persistent: the grid is capped (768 forward / 512 backward blocks: what the 256 CUs hold at once) and walks the tiles with a
// grid stride, so W is staged once per block and the dW accumulators live in registers across all of a block's tiles.
//
// Backward, per tile and per wave w (slices s = w, w+4, ...): d is rebuilt from h and the mask, written row-major to
// a 1.25 KB per-wave LDS tile and read back transposed (ds_read_b64_tr_b16) as the B operand of dW += gᵀ·d; g goes
// through a 640-byte tile the same way (A operand). dh = Wᵀ-fragment x gᵀ puts 8 consecutive columns of one row in a
// lane (two MFMAs whose output rows interleave 4 + 4 columns). The next tile's h is loaded before this tile is
// processed. A tile whose 16 rows are all ignored stores zeros and skips everything else (wave-uniform branch).
//
// g is rounded to bf16 for the two backward products (as a bf16 autograd chain rounds dlogits); db sums the fp32 g.
//
// hipcc -Rpass-analysis=kernel-resource-usage (gfx950, -O3; C and H are run-time values; profiles/label_smoothing/
// resource_usage.txt):
//   tok_fwd_kernel<false>         152 VGPRs + 4 AGPRs, scratch 0, occupancy 3 waves / SIMD, LDS 33,072 B
//   tok_fwd_kernel<true>          154 VGPRs + 4 AGPRs, scratch 0, occupancy 3,              LDS 33,072 B   (kSmooth)
//   tok_bwd_kernel<false, false>  233 VGPRs,           scratch 0, occupancy 2 waves / SIMD, LDS 48,640 B
//   tok_bwd_kernel<false, true>   235 VGPRs,           scratch 0, occupancy 2,              LDS 48,640 B   (kSmooth)
//   tok_bwd_kernel<true, false> (the given-gradient entry of qa_head.hip): 235 VGPRs, scratch 0, LDS 48,640 B
//   tok_reduce_kernel   12 VGPRs,           scratch 0
#include "head_common.h"
#include "launchers.h"

namespace hsd {
namespace tok {

constexpr int TR = 16;                 // rows per tile
constexpr int CP = 16;                 // classes, padded
constexpr int MAXH = 1024;
constexpr int FWD_MAX_BLOCKS = 768;    // 3 blocks per CU: 33 KB LDS each, 152 VGPRs (3 waves per SIMD)
constexpr int BWD_MAX_BLOCKS = 512;    // 2 blocks per CU: 47 KB LDS each, <= 256 VGPRs
constexpr int WROW_PAD = 8;            // forward W image: row stride H + 8 elements
constexpr int WT_STRIDE = 20;          // backward Wᵀ image: 16 classes + 4 elements (40 B) per column
constexpr int D_STRIDE = 40;           // per-wave d tile: 32 columns + 8 elements (80 B) per row
constexpr int G_STRIDE = 20;           // per-wave g tile: 16 classes + 4 elements (40 B) per row
constexpr int BWD_SLICES = MAXH / 32 / 4;  // 32-column slices per wave

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

using head::keep8;
using head::pack8;
using head::unpack8;

// the bf16 classifier input d = bf16(h · keep · scale) of one lane's 8 columns (h itself without dropout)
__device__ __forceinline__ u32x4 dropped8(const u32x4& raw, uint32_t rw, int h0, const DropoutParams& dp) {
  if (!dp.enabled) return raw;
  float v[8], kf[8];
  unpack8(raw, v);
  keep8(rw, h0, dp, kf);
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] *= kf[k];
  return pack8(v);
}

// the LDS tiles below are written and read by ONE wave: the LDS executes a wave's instructions in order, so only
// the compiler has to keep the order
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ------------------------------------------------------------------------------------------------ forward
// kSmooth: the row's loss is lse - (1-eps)·logit[label] - (eps/C)·Σ_c logit[c] (label smoothing over the C real classes);
// an instantiation of its own, so that <false> is the code it was before eps existed
template <bool kSmooth>
__global__ __launch_bounds__(256) void tok_fwd_kernel(const bf16_t* __restrict__ h, const bf16_t* __restrict__ W,
                                                      const bf16_t* __restrict__ bias,
                                                      const int64_t* __restrict__ labels, bf16_t* __restrict__ logits,
                                                      float* __restrict__ partials, int R, int H, int C,
                                                      DropoutParams dp, float eps) {
  dp = resolve_seed(dp);
  __shared__ __attribute__((aligned(16))) bf16_t Wimg[CP * (MAXH + WROW_PAD)];
  __shared__ float red[4][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int wstride = H + WROW_PAD;
  const int nch = H >> 3;
  for (int idx = threadIdx.x; idx < CP * nch; idx += 256) {
    const int c = idx / nch, ch = idx - c * nch;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (c < C) v = *reinterpret_cast<const u32x4*>(W + (int64_t)c * H + ch * 8);
    *reinterpret_cast<u32x4*>(Wimg + c * wstride + ch * 8) = v;
  }
  float bj[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) bj[j] = 4 * q + j < C ? bf2f(bias[4 * q + j]) : 0.f;
  __syncthreads();

  const int ntiles = (R + TR - 1) / TR;
  float loss_sum = 0.f, hits = 0.f, nvalid = 0.f;
  for (int tile = blockIdx.x * 4 + wave; tile < ntiles; tile += gridDim.x * 4) {
    const int row = tile * TR + r;
    const bool rvalid = row < R;
    const uint32_t rw = dropout_row((uint32_t)row, dp);
    const bf16_t* hrow = h + (int64_t)row * H;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0; s0 * 32 < H; s0 += 8) {
      u32x4 raw[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int h0 = (s0 + u) * 32 + q * 8;
        raw[u] = u32x4{0u, 0u, 0u, 0u};
        if (rvalid && h0 < H) raw[u] = *reinterpret_cast<const u32x4*>(hrow + h0);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int h0 = (s0 + u) * 32 + q * 8;
        if ((s0 + u) * 32 < H) {  // wave-uniform
          const u32x4 d = dropped8(raw[u], rw, h0, dp);  // zero where the lane is outside the matrix
          u32x4 wf = {0u, 0u, 0u, 0u};
          if (h0 < H) wf = *reinterpret_cast<const u32x4*>(Wimg + r * wstride + h0);  // class r, this lane's k range
          // A = W [class][k], B = d [k][row]: D[class 4q + reg][row r]
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf), __builtin_bit_cast(bf16x8, d),
                                                        acc, 0, 0, 0);
        }
      }
    }
    // this lane: classes 4q .. 4q+3 of row r, rounded to the bf16 values that are stored
    float lg[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      lg[j] = bf2f(f2bf(acc[j] + bj[j]));
      if (rvalid && 4 * q + j < C) logits[(int64_t)row * C + 4 * q + j] = f2bf(lg[j]);
    }
    if (labels != nullptr) {  // kernel-uniform
      const int64_t lab = rvalid ? labels[row] : -100;
      const bool valid = lab >= 0 && lab < C;
      float m = -INFINITY;
      int am = 0x7fffffff;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (4 * q + j < C && lg[j] > m) { m = lg[j]; am = 4 * q + j; }  // first maximum, as torch.argmax
#pragma unroll
      for (int o = 16; o <= 32; o <<= 1) {
        const float om = __shfl_xor(m, o, 64);
        const int oa = __shfl_xor(am, o, 64);
        if (om > m || (om == m && oa < am)) { m = om; am = oa; }
      }
      float se = 0.f, picked = 0.f, zs = 0.f;  // zs (kSmooth): Σ lg over the row's classes
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (4 * q + j < C) {
          se += __expf(lg[j] - m);
          if constexpr (kSmooth) zs += lg[j];
        }
        if (4 * q + j == lab) picked = lg[j];
      }
#pragma unroll
      for (int o = 16; o <= 32; o <<= 1) {
        se += __shfl_xor(se, o, 64);
        picked += __shfl_xor(picked, o, 64);
        if constexpr (kSmooth) zs += __shfl_xor(zs, o, 64);
      }
      if (q == 0 && valid) {
        if constexpr (kSmooth) loss_sum += __logf(se) + m - (1.0f - eps) * picked - eps / (float)C * zs;
        else loss_sum += __logf(se) + m - picked;
        hits += am == (int)lab ? 1.f : 0.f;
        nvalid += 1.f;
      }
    }
  }
  loss_sum = wave_sum(loss_sum);
  hits = wave_sum(hits);
  nvalid = wave_sum(nvalid);
  if (lane == 0) {
    red[wave][0] = loss_sum;
    red[wave][1] = hits;
    red[wave][2] = nvalid;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int k = threadIdx.x;
    partials[(int64_t)blockIdx.x * 4 + k] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
  }
}

// ------------------------------------------------------------------------------------------------ backward
// this wave's slices of one tile's h rows: slice k is columns (wave + 4k)·32 + q·8 .. +7 of row `row`
__device__ __forceinline__ void load_tile(const bf16_t* __restrict__ h, int tile, int ntiles, int R, int H, int wave,
                                          int r, int q, u32x4 (&raw)[BWD_SLICES]) {
  const int row = tile * TR + r;
  const bool ok = tile < ntiles && row < R;
#pragma unroll
  for (int k = 0; k < BWD_SLICES; ++k) {
    const int h0 = (wave + 4 * k) * 32 + q * 8;
    raw[k] = u32x4{0u, 0u, 0u, 0u};
    if (ok && h0 < H) raw[k] = *reinterpret_cast<const u32x4*>(h + (int64_t)row * H + h0);
  }
}

// GIVEN = false: g from the logits and the labels (the token-classification loss above). GIVEN = true: the caller's
// per-row gradient table g0 [R][C] fp32 (launch_token_head_bwd_given: the span head of qa_head.hip, whose softmax runs
// along the sequence), g[row][c] = g0[row][c] · dloss · gmul / max(cnt[c], 1); logits, labels and stats are not read.
// A row of zeros in g0 is an ignored row. Everything from g on is the same code.
// kSmooth (GIVEN = false only): g = (softmax - (1-eps)·onehot - eps/C) · scale, the label-smoothed CE's gradient.
template <bool GIVEN, bool kSmooth>
__global__ __launch_bounds__(256, 2) void tok_bwd_kernel(const bf16_t* __restrict__ h, const bf16_t* __restrict__ W,
                                                         const bf16_t* __restrict__ logits,
                                                         const int64_t* __restrict__ labels,
                                                         const float* __restrict__ stats,
                                                         const float* __restrict__ dloss, bf16_t* __restrict__ dh,
                                                         float* __restrict__ part, int R, int H, int C, int write_dh,
                                                         DropoutParams dp, const float* __restrict__ g0,
                                                         const float* __restrict__ cnt, float gmul, float eps) {
  static_assert(!(GIVEN && kSmooth), "a given gradient table is not smoothed");
  dp = resolve_seed(dp);
  __shared__ __attribute__((aligned(16))) bf16_t Wt[MAXH * WT_STRIDE];
  __shared__ __attribute__((aligned(16))) bf16_t Dst[4][TR * D_STRIDE];
  __shared__ __attribute__((aligned(16))) bf16_t Gst[4][TR * G_STRIDE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  // Wᵀ image: Wt[col][class], zeros in the padding classes
  for (int idx = threadIdx.x; idx < CP * H; idx += 256) {
    const int c = idx / H, col = idx - c * H;
    Wt[col * WT_STRIDE + c] = c < C ? W[(int64_t)c * H + col] : (bf16_t)0;
  }
  __syncthreads();

  float scale = 0.f, cscale[4] = {0.f, 0.f, 0.f, 0.f};  // GIVEN: one factor per class 4q + j of this lane
  if constexpr (GIVEN) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * q + j < C) cscale[j] = dloss[0] * gmul / fmaxf(cnt[4 * q + j], 1.0f);
  } else {
    scale = dloss[0] / fmaxf(stats[2], 1.0f);
  }
  // transposed-read addresses (ds_read_b64_tr_b16): lane 4a + p of a 16-lane group supplies row a, columns 4p .. 4p+3
  // of the group's 4-row block (rows 4q .. 4q+3 of the tile); lane i of the group receives column i of those rows
  const int ta = r >> 2, tp = r & 3;
  bf16_t* const dst = Dst[wave];
  bf16_t* const gst = Gst[wave];
  const lds_bf16x4* const g_tr = (const lds_bf16x4*)(gst + (4 * q + ta) * G_STRIDE + 4 * tp);
  const lds_bf16x4* const d_tr0 = (const lds_bf16x4*)(dst + (4 * q + ta) * D_STRIDE + 4 * tp);
  const lds_bf16x4* const d_tr1 = (const lds_bf16x4*)(dst + (4 * q + ta) * D_STRIDE + 16 + 4 * tp);

  f32x4 accw[BWD_SLICES][2];  // dW: classes 4q + reg, column (wave + 4k)·32 + cb·16 + r
#pragma unroll
  for (int k = 0; k < BWD_SLICES; ++k) {
    accw[k][0] = f32x4{0.f, 0.f, 0.f, 0.f};
    accw[k][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  float accb[4] = {0.f, 0.f, 0.f, 0.f};  // db: classes 4q + j, this lane's row of every tile

  const int ntiles = (R + TR - 1) / TR;
  u32x4 cur[BWD_SLICES];
  load_tile(h, blockIdx.x, ntiles, R, H, wave, r, q, cur);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    u32x4 nxt[BWD_SLICES];
    load_tile(h, tile + gridDim.x, ntiles, R, H, wave, r, q, nxt);
    const int row = tile * TR + r;
    const bool rvalid = row < R;
    int64_t lab = -100;
    bool valid;
    float gv[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (GIVEN) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (rvalid && 4 * q + j < C) gv[j] = g0[(int64_t)row * C + 4 * q + j];
      valid = gv[0] != 0.f || gv[1] != 0.f || gv[2] != 0.f || gv[3] != 0.f;  // this lane's classes of its row
    } else {
      lab = rvalid ? labels[row] : -100;
      valid = lab >= 0 && lab < C;
    }
    if (__ballot(valid) == 0ull) {
      // every row of the tile is ignored: zeros, nothing else (the branch is wave-uniform)
      if (write_dh) {
#pragma unroll
        for (int k = 0; k < BWD_SLICES; ++k) {
          const int h0 = (wave + 4 * k) * 32 + q * 8;
          if (rvalid && h0 < H) *reinterpret_cast<u32x4*>(dh + (int64_t)row * H + h0) = u32x4{0u, 0u, 0u, 0u};
        }
      }
    } else {
      // g of this lane's 4 classes of its row
      float g[4];
      if constexpr (GIVEN) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          g[j] = gv[j] * cscale[j];
          accb[j] += g[j];
        }
      } else {
        float e[4], m = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          e[j] = rvalid && 4 * q + j < C ? bf2f(logits[(int64_t)row * C + 4 * q + j]) : -INFINITY;
          m = fmaxf(m, e[j]);
        }
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        if (!rvalid) m = 0.f;
        float se = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          e[j] = __expf(e[j] - m);  // exp(-inf) = 0 in the padding classes
          se += e[j];
        }
        se += __shfl_xor(se, 16, 64);
        se += __shfl_xor(se, 32, 64);
        const float inv = 1.0f / se;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int c = 4 * q + j;
          if constexpr (kSmooth)
            g[j] = valid && c < C ? (e[j] * inv - (c == (int)lab ? 1.0f - eps : 0.f) - eps / (float)C) * scale : 0.f;
          else g[j] = valid && c < C ? (e[j] * inv - (c == (int)lab ? 1.f : 0.f)) * scale : 0.f;
          accb[j] += g[j];
        }
      }
      const u32x2 gpk = {pack_bf2(g[0], g[1]), pack_bf2(g[2], g[3])};
      const bf16x4 gb = __builtin_bit_cast(bf16x4, gpk);  // B operand of dh: [k = class 4q + j][n = row r]
      *reinterpret_cast<u32x2*>(gst + r * G_STRIDE + 4 * q) = gpk;
      wave_lds_fence();
      const bf16x4 ga = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)g_tr);  // A of dW: [m = class r][k = row 4q + j]
      const uint32_t rw = dropout_row((uint32_t)row, dp);
#pragma unroll
      for (int k = 0; k < BWD_SLICES; ++k) {
        const int s = wave + 4 * k;
        if (s * 32 < H) {  // wave-uniform
          const int h0 = s * 32 + q * 8;
          const bool ok = rvalid && h0 < H;
          float kf[8] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
          if (dp.enabled) keep8(rw, h0, dp, kf);
          u32x4 d = cur[k];  // zero outside the matrix
          if (dp.enabled) {
            float v[8];
            unpack8(cur[k], v);
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] *= kf[i];
            d = pack8(v);
          }
          *reinterpret_cast<u32x4*>(dst + r * D_STRIDE + q * 8) = d;
          wave_lds_fence();
          // dW[class][col] += Σ_row g[row][class] · d[row][col]: B = d transposed, [k = row 4q + j][n = column]
          const bf16x4 db0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)d_tr0);
          const bf16x4 db1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)d_tr1);
          accw[k][0] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(ga, db0, accw[k][0], 0, 0, 0);
          accw[k][1] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(ga, db1, accw[k][1], 0, 0, 0);
          wave_lds_fence();  // the next slice overwrites the d tile
          if (write_dh) {
            // dh[row][col] = Σ_class W[class][col] · g[row][class]: A = Wᵀ fragment [m][k = class 4q + j] with output
            // row m = 4a + b of MFMA t standing for column s·32 + a·8 + t·4 + b, so that a lane (which gets output
            // rows 4q .. 4q+3) collects the 8 consecutive columns s·32 + q·8 .. +7 of its row from t = 0, 1
            float o[8];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
              const int col = s * 32 + (r >> 2) * 8 + t * 4 + (r & 3);
              u32x2 wa = {0u, 0u};
              if (col < H) wa = *reinterpret_cast<const u32x2*>(Wt + col * WT_STRIDE + 4 * q);
              const f32x4 od = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(bf16x4, wa), gb,
                                                                         f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
              for (int i = 0; i < 4; ++i) o[4 * t + i] = od[i] * kf[4 * t + i];
            }
            if (ok) *reinterpret_cast<u32x4*>(dh + (int64_t)row * H + h0) = pack8(o);
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < BWD_SLICES; ++k) cur[k] = nxt[k];
  }

  // this block's partial slab: [C][H] then [C]
  float* const slab = part + (int64_t)blockIdx.x * ((int64_t)C * H + C);
#pragma unroll
  for (int k = 0; k < BWD_SLICES; ++k) {
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      const int col = (wave + 4 * k) * 32 + cb * 16 + r;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = 4 * q + i;
        if (c < C && col < H) slab[(int64_t)c * H + col] = accw[k][cb][i];
      }
    }
  }
  if (wave == 0) {  // every wave holds the same g: one of them sums db over the tile rows (lanes r = 0 .. 15)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v = accb[j];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
      if (r == 0 && 4 * q + j < C) slab[(int64_t)C * H + 4 * q + j] = v;
    }
  }
}

// dW (then db) += the nblk partial slabs. RED_X outputs x RED_G groups of consecutive blocks per workgroup; a
// group's blocks are added in block order and the group sums in group order: the same bits every run.
constexpr int RED_X = 16, RED_G = 16;
__global__ __launch_bounds__(256) void tok_reduce_kernel(const float* __restrict__ part, int nblk, int n, int nw,
                                                         float* __restrict__ dW, float* __restrict__ db) {
  __shared__ float red[RED_G][RED_X];
  const int x = threadIdx.x % RED_X, grp = threadIdx.x / RED_X;
  const int e = blockIdx.x * RED_X + x;
  const int per = (nblk + RED_G - 1) / RED_G;
  const int b0 = grp * per, b1 = min(nblk, b0 + per);
  float s = 0.f;
  if (e < n)
    for (int b = b0; b < b1; ++b) s += part[(int64_t)b * n + e];
  red[grp][x] = s;
  __syncthreads();
  if (grp == 0 && e < n) {
    float t = red[0][x];
#pragma unroll
    for (int k = 1; k < RED_G; ++k) t += red[k][x];
    float* const dst = e < nw ? dW + e : db + (e - nw);
    *dst += t;
  }
}

}  // namespace tok

int token_head_fwd_blocks(int R) {
  const int ntiles = (R + tok::TR - 1) / tok::TR;
  return std::max(1, std::min((ntiles + 3) / 4, tok::FWD_MAX_BLOCKS));
}

int token_head_bwd_blocks(int R) {
  const int ntiles = (R + tok::TR - 1) / tok::TR;
  return std::max(1, std::min(ntiles, tok::BWD_MAX_BLOCKS));
}

void launch_token_head_fwd(const bf16_t* h, const bf16_t* W, const bf16_t* b, const int64_t* labels, bf16_t* logits,
                           float* partials, float* stats, int R, int H, int C, double p, uint64_t seed,
                           hipStream_t st, float label_smoothing) {
  const int nblk = token_head_fwd_blocks(R);
  const DropoutParams dp = make_dropout(p, seed);
  if (labels != nullptr && label_smoothing > 0.f)
    hipLaunchKernelGGL(tok::tok_fwd_kernel<true>, dim3(nblk), dim3(256), 0, st, h, W, b, labels, logits, partials, R, H,
                       C, dp, label_smoothing);
  else
    hipLaunchKernelGGL(tok::tok_fwd_kernel<false>, dim3(nblk), dim3(256), 0, st, h, W, b, labels, logits, partials, R,
                       H, C, dp, 0.f);
  HSD_CHECK_LAUNCH();
  if (labels != nullptr) launch_head_stats(partials, nblk, stats, st);
}

void launch_token_head_bwd(const bf16_t* h, const bf16_t* W, const bf16_t* logits, const int64_t* labels,
                           const float* stats, const float* dloss, bf16_t* dh, float* part, float* dW, float* db,
                           int R, int H, int C, double p, uint64_t seed, hipStream_t st, float label_smoothing) {
  const int nblk = token_head_bwd_blocks(R);
  const DropoutParams dp = make_dropout(p, seed);
  if (label_smoothing > 0.f)
    hipLaunchKernelGGL((tok::tok_bwd_kernel<false, true>), dim3(nblk), dim3(256), 0, st, h, W, logits, labels, stats,
                       dloss, dh, part, R, H, C, dh != nullptr ? 1 : 0, dp, (const float*)nullptr,
                       (const float*)nullptr, 0.f, label_smoothing);
  else
    hipLaunchKernelGGL((tok::tok_bwd_kernel<false, false>), dim3(nblk), dim3(256), 0, st, h, W, logits, labels, stats,
                       dloss, dh, part, R, H, C, dh != nullptr ? 1 : 0, dp, (const float*)nullptr,
                       (const float*)nullptr, 0.f, 0.f);
  HSD_CHECK_LAUNCH();
  const int n = C * H + C;
  hipLaunchKernelGGL(tok::tok_reduce_kernel, dim3((n + tok::RED_X - 1) / tok::RED_X), dim3(tok::RED_X * tok::RED_G), 0,
                     st, (const float*)part, nblk, n, C * H,
                     dW, db);
  HSD_CHECK_LAUNCH();
}

void launch_token_head_bwd_given(const bf16_t* h, const bf16_t* W, const float* g0, const float* cnt, float gmul,
                                 const float* dloss, bf16_t* dh, float* part, float* dW, float* db, int R, int H,
                                 int C, double p, uint64_t seed, hipStream_t st) {
  const int nblk = token_head_bwd_blocks(R);
  const DropoutParams dp = make_dropout(p, seed);
  hipLaunchKernelGGL((tok::tok_bwd_kernel<true, false>), dim3(nblk), dim3(256), 0, st, h, W, (const bf16_t*)nullptr,
                     (const int64_t*)nullptr, (const float*)nullptr, dloss, dh, part, R, H, C, dh != nullptr ? 1 : 0,
                     dp, g0, cnt, gmul, 0.f);
  HSD_CHECK_LAUNCH();
  const int n = C * H + C;
  hipLaunchKernelGGL(tok::tok_reduce_kernel, dim3((n + tok::RED_X - 1) / tok::RED_X), dim3(tok::RED_X * tok::RED_G), 0,
                     st, (const float*)part, nblk, n, C * H,
                     dW, db);
  HSD_CHECK_LAUNCH();
}

}  // namespace hsd
