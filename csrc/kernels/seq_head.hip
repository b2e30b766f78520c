// Fused sequence-level head for --problem_type (single-label CE with 5..64 classes, multi-label BCE-with-logits and
// regression MSE with 1..64 columns): everything after the pooler / pre-classifier dense GEMM, where cls_head.hip sits
// for single-label C <= 4. H % 8 == 0, H <= 1024, bf16.
//
//   forward   t       = bf16(act(pre))                stored for the backward
//             d       = bf16(t · keep · 1/(1-p))      the hash dropout of ops/rng.py (element e = row·H + h)
//             z       = bf16(d·W2ᵀ + b2)              a runtime loop over classes in groups of 4; lane c keeps z[c]
//             CE      loss = logsumexp(z) - z[label]                    hit = first-maximum argmax == label
//             BCE     loss = Σ_c max(z,0) - z·y + log1p(exp(-|z|)) / C  hit = (z > 0) == (y > 0.5) for every c
//             MSE     loss = Σ_c (z - y)² / C                           hit = |z - y| <= tol for every c
//             ignored rows: label not in [0, C) (CE), first label NaN (BCE / MSE); they add nothing anywhere
//   backward  g       = softmax(z) - onehot | sigmoid(z) - y | 2(z - y), times dloss / max(n,1) (and 1/C for BCE / MSE)
//             label smoothing eps > 0 (CE only, the kSmooth instantiations; eps a host constant of the launch):
//                     loss = lse - (1-eps)·z[label] - (eps/C)·Σ_c z[c],  g = softmax(z) - (1-eps)·onehot - eps/C.
//                     With eps > 0 ops.cls_head sends every single-label head of 1..64 classes here (cls_head.hip
//                     has no smoothed form); eps = 0 launches the <false> instantiations, the code as it was
//             dpre    = (g·W2 · keep · 1/(1-p)) · act'(t)   bf16; g goes to an fp32 [R][C] table as well
//             dW2    += gᵀ·d, db2 += Σ g     seq_wgrad_kernel: register tiles of 8 columns x 8 classes over a row
//                                            split, one fp32 slab per split; seq_wgrad_reduce_kernel adds the slabs
//                                            into main_grad in index order. No atomics: the same bits every run.
//
// Forward and dpre: one wave per row, lanes own 8-element (16-B) chunks lane + 64·i, block = 4 waves x 4 rows, per-block
// partials {loss, hits, n_valid} in the [nblk][4] layout of head_stats.hip.
//
// hipcc -Rpass-analysis=kernel-resource-usage (gfx950, -O3), scratch 0 in each:
//   seq_fwd_kernel<false> 152 VGPRs (<true>: 154), LDS 48 B; seq_bwd_kernel<false> 66 VGPRs (<true>: 68), LDS 0;
//   seq_wgrad_kernel 97 VGPRs, LDS 0; seq_wgrad_reduce_kernel 6 VGPRs, LDS 0
#include "head_common.h"
#include "launchers.h"

namespace hsd {
namespace seq {

using head::keep8;
using head::pack8;
using head::unpack8;

constexpr int ROWS_PER_WAVE = 4;
constexpr int ROWS_PER_BLOCK = 4 * ROWS_PER_WAVE;
constexpr int MAXC = 64;       // one lane per class
constexpr int MAX_CHUNKS = 2;  // H <= 1024 (8 elements x 64 lanes x 2)
constexpr int WG_CLASSES = 8;  // seq_wgrad_kernel: classes per register tile
constexpr int WG_MIN_ROWS = 32;
constexpr int WG_MAX_SPLITS = 32;

enum Mode { CE = 0, BCE = 1, MSE = 2 };

__device__ __forceinline__ float act_fwd(float x, int act) { return act == 0 ? tanhf(x) : fmaxf(x, 0.0f); }
__device__ __forceinline__ float act_bwd(float t, int act) { return act == 0 ? 1.0f - t * t : (t > 0.0f ? 1.0f : 0.0f); }

// labels: int64 [R] (CE) or fp32 [R][C] (BCE / MSE); either may be null (logits only)
// kSmooth (CE only): loss = lse - (1-eps)·z[label] - (eps/C)·Σ_c z[c]; an instantiation of its own, <false> is the
// code as it was before eps existed
template <bool kSmooth>
__global__ __launch_bounds__(256) void seq_fwd_kernel(const bf16_t* __restrict__ pre, int64_t ld_pre,
                                                      const bf16_t* __restrict__ W2, const bf16_t* __restrict__ b2,
                                                      const int64_t* __restrict__ lab_i, const float* __restrict__ lab_f,
                                                      bf16_t* __restrict__ t_out, bf16_t* __restrict__ logits,
                                                      float* __restrict__ partials, int R, int H, int C, int mode,
                                                      float tol, int act, DropoutParams dp, float eps) {
  dp = resolve_seed(dp);
  __shared__ float red[4][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nch = H >> 3;
  const bool mine = lane < C;
  const float invC = 1.0f / (float)C;
  float loss_sum = 0.f, hits = 0.f, nvalid = 0.f;
  for (int rr = 0; rr < ROWS_PER_WAVE; ++rr) {
    const int row = blockIdx.x * ROWS_PER_BLOCK + wave * ROWS_PER_WAVE + rr;
    if (row >= R) break;
    float v[MAX_CHUNKS][8];
#pragma unroll
    for (int i = 0; i < MAX_CHUNKS; ++i) {
      const int ch = lane + 64 * i;
#pragma unroll
      for (int k = 0; k < 8; ++k) v[i][k] = 0.f;
      if (ch < nch) {
        const int h0 = ch * 8;
        unpack8(*reinterpret_cast<const u32x4*>(pre + (int64_t)row * ld_pre + h0), v[i]);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[i][k] = bf2f(f2bf(act_fwd(v[i][k], act)));  // the bf16 activation the backward sees
        *reinterpret_cast<u32x4*>(t_out + (int64_t)row * H + h0) = pack8(v[i]);
        if (dp.enabled) {  // bf16(t · keep · scale)
          float kf[8];
          keep8(dropout_row((uint32_t)row, dp), h0, dp, kf);
#pragma unroll
          for (int k = 0; k < 8; ++k) v[i][k] = bf2f(f2bf(v[i][k] * kf[k]));
        }
      }
    }
    float z = 0.f;  // lane c: logit c
    for (int c0 = 0; c0 < C; c0 += 4) {
      float dot[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < MAX_CHUNKS; ++i) {
        const int ch = lane + 64 * i;
        if (ch < nch) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int c = min(c0 + j, C - 1);  // a group's remainder recomputes the last class; its sum is dropped
            float w[8];
            unpack8(*reinterpret_cast<const u32x4*>(W2 + (int64_t)c * H + ch * 8), w);
#pragma unroll
            for (int k = 0; k < 8; ++k) dot[j] = fmaf(v[i][k], w[k], dot[j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float s = wave_sum(dot[j]);
        if (lane == c0 + j) z = s;
      }
    }
    if (mine) {
      z = bf2f(f2bf(z + bf2f(b2[lane])));
      logits[(int64_t)row * C + lane] = f2bf(z);
    }
    float loss = 0.f;
    bool valid = false, hit = false;
    if (mode == CE) {
      const int64_t lab = lab_i != nullptr ? lab_i[row] : -100;
      valid = lab >= 0 && lab < C;
      if (valid) {
        const float m = wave_max(mine ? z : -3.0e38f);
        const float am = -wave_max(mine && z == m ? -(float)lane : -64.f);  // first maximum, as torch.argmax
        const float s = wave_sum(mine ? __expf(z - m) : 0.f);
        const float zl = wave_sum(lane == (int)lab ? z : 0.f);
        if constexpr (kSmooth) {
          const float zs = wave_sum(mine ? z : 0.f);
          loss = __logf(s) + m - (1.0f - eps) * zl - eps * invC * zs;
        } else {
          loss = __logf(s) + m - zl;
        }
        hit = (int)am == (int)lab;
      }
    } else {
      valid = lab_f != nullptr && !isnan(lab_f[(int64_t)row * C]);
      if (valid) {
        const float y = mine ? lab_f[(int64_t)row * C + lane] : 0.f;
        float term, miss;
        if (mode == BCE) {
          term = fmaxf(z, 0.f) - z * y + log1pf(__expf(-fabsf(z)));
          miss = (z > 0.f) != (y > 0.5f) ? 1.f : 0.f;
        } else {
          term = (z - y) * (z - y);
          miss = fabsf(z - y) <= tol ? 0.f : 1.f;
        }
        loss = wave_sum(mine ? term : 0.f) * invC;
        hit = wave_sum(mine ? miss : 0.f) == 0.f;
      }
    }
    if (valid) {
      loss_sum += loss;
      hits += hit ? 1.f : 0.f;
      nvalid += 1.f;
    }
  }
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

// g [R][C] fp32 (zero rows: ignored rows) and dpre [R][H] bf16
// kSmooth (CE only): g = (softmax - (1-eps)·onehot - eps/C) · scale
template <bool kSmooth>
__global__ __launch_bounds__(256) void seq_bwd_kernel(const bf16_t* __restrict__ t_in, const bf16_t* __restrict__ W2,
                                                      const bf16_t* __restrict__ logits, const int64_t* __restrict__ lab_i,
                                                      const float* __restrict__ lab_f, const float* __restrict__ stats,
                                                      const float* __restrict__ dloss, bf16_t* __restrict__ dpre,
                                                      float* __restrict__ g_out, int R, int H, int C, int mode, int act,
                                                      DropoutParams dp, float eps) {
  dp = resolve_seed(dp);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nch = H >> 3;
  const bool mine = lane < C;
  const float scale = dloss[0] / fmaxf(stats[2], 1.0f) * (mode == CE ? 1.0f : 1.0f / (float)C);
  for (int rr = 0; rr < ROWS_PER_WAVE; ++rr) {
    const int row = blockIdx.x * ROWS_PER_BLOCK + wave * ROWS_PER_WAVE + rr;
    if (row >= R) break;
    bool valid;
    int lab = 0;
    if (mode == CE) {
      const int64_t l = lab_i[row];
      valid = l >= 0 && l < C;
      lab = (int)l;
    } else {
      valid = !isnan(lab_f[(int64_t)row * C]);
    }
    float g = 0.f;
    if (valid) {
      const float z = mine ? bf2f(logits[(int64_t)row * C + lane]) : 0.f;
      if (mode == CE) {
        const float m = wave_max(mine ? z : -3.0e38f);
        const float e = mine ? __expf(z - m) : 0.f;
        const float s = wave_sum(e);
        if constexpr (kSmooth) g = e / s - (lane == lab ? 1.0f - eps : 0.f) - eps / (float)C;
        else g = e / s - (lane == lab ? 1.f : 0.f);
      } else {
        const float y = mine ? lab_f[(int64_t)row * C + lane] : 0.f;
        g = mode == BCE ? 1.0f / (1.0f + __expf(-z)) - y : 2.0f * (z - y);
      }
      g = mine ? g * scale : 0.f;
    }
    if (mine) g_out[(int64_t)row * C + lane] = g;
    float dd[MAX_CHUNKS][8];
#pragma unroll
    for (int i = 0; i < MAX_CHUNKS; ++i)
#pragma unroll
      for (int k = 0; k < 8; ++k) dd[i][k] = 0.f;
    if (valid) {
      for (int c = 0; c < C; ++c) {
        const float gc = __shfl(g, c, 64);
#pragma unroll
        for (int i = 0; i < MAX_CHUNKS; ++i) {
          const int ch = lane + 64 * i;
          if (ch < nch) {
            float w[8];
            unpack8(*reinterpret_cast<const u32x4*>(W2 + (int64_t)c * H + ch * 8), w);
#pragma unroll
            for (int k = 0; k < 8; ++k) dd[i][k] = fmaf(gc, w[k], dd[i][k]);
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < MAX_CHUNKS; ++i) {
      const int ch = lane + 64 * i;
      if (ch >= nch) break;
      const int h0 = ch * 8;
      const int64_t e0 = (int64_t)row * H + h0;
      float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (valid) {  // an ignored row's dpre is exact zeros
        float t[8], kf[8] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
        unpack8(*reinterpret_cast<const u32x4*>(t_in + e0), t);
        if (dp.enabled) keep8(dropout_row((uint32_t)row, dp), h0, dp, kf);
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = dd[i][k] * kf[k] * act_bwd(t[k], act);
      }
      *reinterpret_cast<u32x4*>(dpre + e0) = pack8(o);
    }
  }
}

// slab[split][c·H + h] = Σ_{rows of the split} g[r][c] · d[r][h], slab[split][C·H + c] = Σ g[r][c]; d = bf16(t·keep·scale).
// One wave per block: lane = column chunk blockIdx.x·64 + lane, blockIdx.y = group of 8 classes, blockIdx.z = split.
__global__ __launch_bounds__(64) void seq_wgrad_kernel(const bf16_t* __restrict__ t_in, const float* __restrict__ g,
                                                       float* __restrict__ slab, int64_t stride, int R, int H, int C,
                                                       int rows_per_split, DropoutParams dp) {
  dp = resolve_seed(dp);
  const int ch = blockIdx.x * 64 + threadIdx.x;
  const int c0 = blockIdx.y * WG_CLASSES;
  const bool has = ch < (H >> 3);
  const int h0 = ch * 8;
  const int r0 = blockIdx.z * rows_per_split;
  const int r1 = min(R, r0 + rows_per_split);
  float aw[WG_CLASSES][8], ab[WG_CLASSES];
#pragma unroll
  for (int c = 0; c < WG_CLASSES; ++c) {
    ab[c] = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) aw[c][k] = 0.f;
  }
  for (int r = r0; r < r1; ++r) {
    float gc[WG_CLASSES];
#pragma unroll
    for (int c = 0; c < WG_CLASSES; ++c) {
      gc[c] = c0 + c < C ? g[(int64_t)r * C + c0 + c] : 0.f;
      ab[c] += gc[c];
    }
    if (has) {
      float t[8];
      unpack8(*reinterpret_cast<const u32x4*>(t_in + (int64_t)r * H + h0), t);
      if (dp.enabled) {
        float kf[8];
        keep8(dropout_row((uint32_t)r, dp), h0, dp, kf);
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = bf2f(f2bf(t[k] * kf[k]));  // the dropped activation (classifier input)
      }
#pragma unroll
      for (int c = 0; c < WG_CLASSES; ++c)
#pragma unroll
        for (int k = 0; k < 8; ++k) aw[c][k] = fmaf(gc[c], t[k], aw[c][k]);
    }
  }
  float* out = slab + (int64_t)blockIdx.z * stride;  // stride % 4 == 0: the 16-B stores below stay aligned
#pragma unroll
  for (int c = 0; c < WG_CLASSES; ++c) {
    if (c0 + c >= C) break;
    if (has) {
      float4* p = reinterpret_cast<float4*>(out + (int64_t)(c0 + c) * H + h0);
      p[0] = float4{aw[c][0], aw[c][1], aw[c][2], aw[c][3]};
      p[1] = float4{aw[c][4], aw[c][5], aw[c][6], aw[c][7]};
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) out[(int64_t)C * H + c0 + c] = ab[c];
  }
}

// dW2 [C·H] and db2 [C] += the slabs, in split order
__global__ __launch_bounds__(256) void seq_wgrad_reduce_kernel(const float* __restrict__ slab, int nsplit, int64_t stride,
                                                               float* __restrict__ dW2, float* __restrict__ db2, int CH,
                                                               int C) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= CH + C) return;
  float s = 0.f;
  for (int sp = 0; sp < nsplit; ++sp) s += slab[(int64_t)sp * stride + i];
  if (i < CH) dW2[i] += s;
  else db2[i - CH] += s;
}

}  // namespace seq

int seq_head_blocks(int R) { return (R + seq::ROWS_PER_BLOCK - 1) / seq::ROWS_PER_BLOCK; }

static int seq_rows_per_split(int R) {
  const int rps = (R + seq::WG_MAX_SPLITS - 1) / seq::WG_MAX_SPLITS;
  return rps < seq::WG_MIN_ROWS ? seq::WG_MIN_ROWS : rps;
}

int seq_head_splits(int R) {
  const int rps = seq_rows_per_split(R);
  return (R + rps - 1) / rps;
}

// a slab's stride in floats: C·H + C rounded up to 4, so that every slab's 16-B stores stay aligned
int64_t seq_head_slab(int H, int C) { return (((int64_t)C * H + C) + 3) / 4 * 4; }

void launch_seq_head_fwd(const bf16_t* pre, int64_t ld_pre, const bf16_t* W2, const bf16_t* b2, const int64_t* lab_i,
                         const float* lab_f, bf16_t* t_out, bf16_t* logits, float* partials, float* stats, int R, int H,
                         int C, int mode, float tol, int act, double p, uint64_t seed, hipStream_t st,
                         float label_smoothing) {
  const int nblk = seq_head_blocks(R);
  const DropoutParams dp = make_dropout(p, seed);
  if (mode == seq::CE && label_smoothing > 0.f)
    hipLaunchKernelGGL(seq::seq_fwd_kernel<true>, dim3(nblk), dim3(256), 0, st, pre, ld_pre, W2, b2, lab_i, lab_f, t_out,
                       logits, partials, R, H, C, mode, tol, act, dp, label_smoothing);
  else
    hipLaunchKernelGGL(seq::seq_fwd_kernel<false>, dim3(nblk), dim3(256), 0, st, pre, ld_pre, W2, b2, lab_i, lab_f,
                       t_out, logits, partials, R, H, C, mode, tol, act, dp, 0.f);
  HSD_CHECK_LAUNCH();
  launch_head_stats(partials, nblk, stats, st);
}

void launch_seq_head_bwd(const bf16_t* t_in, const bf16_t* W2, const bf16_t* logits, const int64_t* lab_i,
                         const float* lab_f, const float* stats, const float* dloss, bf16_t* dpre, float* g, float* slab,
                         float* dW2, float* db2, int R, int H, int C, int mode, int act, double p, uint64_t seed,
                         hipStream_t st, float label_smoothing) {
  const DropoutParams dp = make_dropout(p, seed);
  if (mode == seq::CE && label_smoothing > 0.f)
    hipLaunchKernelGGL(seq::seq_bwd_kernel<true>, dim3(seq_head_blocks(R)), dim3(256), 0, st, t_in, W2, logits, lab_i,
                       lab_f, stats, dloss, dpre, g, R, H, C, mode, act, dp, label_smoothing);
  else
    hipLaunchKernelGGL(seq::seq_bwd_kernel<false>, dim3(seq_head_blocks(R)), dim3(256), 0, st, t_in, W2, logits, lab_i,
                       lab_f, stats, dloss, dpre, g, R, H, C, mode, act, dp, 0.f);
  HSD_CHECK_LAUNCH();
  const int nsplit = seq_head_splits(R);
  const int64_t stride = seq_head_slab(H, C);
  const dim3 grid(((H >> 3) + 63) / 64, (C + seq::WG_CLASSES - 1) / seq::WG_CLASSES, nsplit);
  hipLaunchKernelGGL(seq::seq_wgrad_kernel, grid, dim3(64), 0, st, t_in, g, slab, stride, R, H, C,
                     seq_rows_per_split(R), dp);
  HSD_CHECK_LAUNCH();
  const int n = C * H + C;
  hipLaunchKernelGGL(seq::seq_wgrad_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, st, slab, nsplit, stride, dW2,
                     db2, C * H, C);
  HSD_CHECK_LAUNCH();
}

}  // namespace hsd
