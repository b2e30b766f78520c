// Sentence-embedding head of --task sentence-embedding: masked mean pooling + L2 normalisation of every sequence of the
// flat encoder output, and the in-batch-negatives contrastive loss (sentence-transformers'
// MultipleNegativesRankingLoss) on the (anchor, positive) pairs, forward and backward.
//
//   h [R][H] bf16 holds n = 2B sequences (rows cu[s] .. cu[s+1]-1, an optional per-row mask takes rows out); sequence
//   2i is anchor i, 2i+1 its positive. e [n][H] fp32 = mean / max(|mean|, 1e-12); s_ij = scale <a_i, p_j>;
//   loss = Σ_{i valid} (logsumexp_{j valid} s_ij - s_ii) / max(n_valid, 1).
//
//   pool_fwd_kernel   grid (128-row chunk, sequence), 256 threads; blocks past a sequence's end exit at once. Thread t
//            owns the 8 columns of group t % (H/8) (one 16-byte load per row) and the rows rg, rg + nrg, ... of its chunk
//            (rg = t / (H/8), nrg = 256 / (H/8) row groups), summed in fp32 in that order; the row groups meet in LDS
//            and are added in index order. A sequence of at most 128 rows is finished right there (mean, Σ m² by a
//            wave + 4-slot reduction, e, 1/|m|, live rows); a longer one leaves one partial row per chunk in the
//            workspace and pool_finalize_kernel (one workgroup per sequence) adds the chunks in order. The order depends
//            on the position inside the sequence only: padded and packed layouts of the same rows give the same bits.
//   pool_bwd_kernel   the same grid plus one grid row for the rows outside every sequence. Each workgroup recomputes
//            g = (de - e <e, de>) / |m| / count (one H-length dot product) and stores bf16(g) to the live rows of
//            its chunk, zeros to the masked and dead ones, 16 bytes at a time: dh is written exactly once.
//   score_kernel<0>   one workgroup per 32-anchor tile. The anchors' fp32 MFMA fragments stay in registers (wave w of
//            the 4 owns 32 of every 128 columns); the positives stream in 32-row steps through a double-buffered LDS
//            tile of 128 columns at a time. s = a pᵀ on v_mfma_f32_32x32x2_f32, the 4 K-partials meet in LDS in a fixed
//            order; max / sum online in the log2 domain: the max m is kept on the raw product and every term is
//            exp2((s - m) · scale·log2 e), the scale folded in once on a difference that is exact near the max; the sum
//            leaves the max's own term (exactly 1) out, so row i's record {m, rest} gives logsumexp - max = log1p(rest)
//            and the softmax 1 / (1 + rest) without a cancellation. The diagonal and the first argmax are captured on
//            the way. Invalid candidates are skipped, invalid anchors write zeros. No B x B tensor
//            leaves the chip. score_stats_kernel sums the per-row records in index order into
//            stats = {mean loss, hits, n_valid, loss sum}.
//   score_kernel<1>   launched twice with the roles swapped: the owner tile (anchors, then positives) recomputes its
//            score tile against every 32-row step of the other side exactly as the forward does, forms the weights
//            w = (exp2((s - m) · scale·log2 e) - δ (1 + rest)) / (1 + rest) of the anchor's record (0 where either
//            pair is invalid; exactly 0 for a lone candidate) in LDS and multiplies them into the
//            streamed rows with the same instruction. Grid.y splits H into 256-column slabs (32 accumulator registers
//            a wave). The result · dloss · scale / max(n_valid, 1) lands interleaved in de [n][H]; rows of invalid
//            pairs are exact zeros.
//
// No atomics, no memset: every output element has one writer and every sum a fixed order, so two runs give the same
// bits. Limits: H % 8 == 0, H <= 1024; any n, B, sequence length.
//
// hipcc -Rpass-analysis=kernel-resource-usage (gfx950, -O3): profiles/sent_head/resource_usage.txt (scratch 0 everywhere)
#include "head_common.h"
#include "launchers.h"

namespace hsd {
namespace sent {

constexpr int ROWS = 128;  // rows of one pooling chunk

__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return v;
}

// rows of sequence s, clamped to the buffer (nothing below indexes outside [0, R) whatever cu holds)
__device__ __forceinline__ void seq_rows(const int* cu, int s, int R, int& start, int& stop) {
  start = min(max(cu[s], 0), R);
  stop = min(max(cu[s + 1], start), R);
}

// threads t < H/8 hold the 8 column sums of their group and the live-row count: e, 1/|m| and the count of sequence s
__device__ __forceinline__ void pool_finish(float (&s8)[8], int cnt, int seq, int H, float* e, float* aux, float* red) {
  const int t = threadIdx.x;
  const bool own = t < H / 8;
  const float inv_cnt = 1.0f / (float)max(cnt, 1);
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    s8[k] = own ? s8[k] * inv_cnt : 0.f;
    ss += s8[k] * s8[k];
  }
  ss = block_sum(ss, red);
  const float nrm = fmaxf(sqrtf(ss), 1e-12f);
  if (own) {
    float* dst = e + (int64_t)seq * H + 8 * t;
    *reinterpret_cast<f32x4*>(dst) = f32x4{s8[0] / nrm, s8[1] / nrm, s8[2] / nrm, s8[3] / nrm};
    *reinterpret_cast<f32x4*>(dst + 4) = f32x4{s8[4] / nrm, s8[5] / nrm, s8[6] / nrm, s8[7] / nrm};
  }
  if (t == 0) {
    aux[2 * (int64_t)seq] = cnt > 0 ? 1.0f / nrm : 0.f;
    aux[2 * (int64_t)seq + 1] = (float)cnt;
  }
}

__global__ __launch_bounds__(256) void pool_fwd_kernel(const bf16_t* __restrict__ h, const int* __restrict__ cu,
                                                       const int64_t* __restrict__ mask, float* __restrict__ e,
                                                       float* __restrict__ aux, float* __restrict__ ws,
                                                       int* __restrict__ wsc, int R, int H, int maxch) {
  __shared__ float part[2048];  // [row group][H]: nrg · H <= 256 · 8
  __shared__ int pcnt[256];
  __shared__ int tot_s;
  __shared__ float red[4];
  const int seq = blockIdx.y, ch = blockIdx.x, t = threadIdx.x;
  int start, stop;
  seq_rows(cu, seq, R, start, stop);
  // (an understated longest sequence: the rows past maxch chunks are not read, as in pool_finalize_kernel)
  const int nch = min(max((stop - start + ROWS - 1) / ROWS, 1), maxch);
  if (ch >= nch) return;
  const int r0 = start + ch * ROWS, r1 = min(r0 + ROWS, stop);
  const int ncg = H / 8, nrg = 256 / ncg, rg = t / ncg, c = t - rg * ncg;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int cnt = 0;
  if (rg < nrg) {
    for (int row = r0 + rg; row < r1; row += nrg) {
      if (mask != nullptr && mask[row] == 0) continue;
      float v[8];
      head::unpack8(*reinterpret_cast<const u32x4*>(h + (int64_t)row * H + 8 * c), v);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] += v[k];
      ++cnt;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) part[rg * H + 8 * c + k] = acc[k];
    if (c == 0) pcnt[rg] = cnt;
  }
  __syncthreads();
  float s8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int total = 0;
  if (t < ncg) {
    for (int g = 0; g < nrg; ++g) {
#pragma unroll
      for (int k = 0; k < 8; ++k) s8[k] += part[g * H + 8 * t + k];
      total += pcnt[g];
    }
  }
  if (nch == 1) {
    if (t == 0) tot_s = total;
    __syncthreads();
    pool_finish(s8, tot_s, seq, H, e, aux, red);
  } else if (t < ncg) {
    float* dst = ws + ((int64_t)seq * maxch + ch) * H + 8 * t;
    *reinterpret_cast<f32x4*>(dst) = f32x4{s8[0], s8[1], s8[2], s8[3]};
    *reinterpret_cast<f32x4*>(dst + 4) = f32x4{s8[4], s8[5], s8[6], s8[7]};
    if (t == 0) wsc[(int64_t)seq * maxch + ch] = total;
  }
}

__global__ __launch_bounds__(256) void pool_finalize_kernel(const int* __restrict__ cu, const float* __restrict__ ws,
                                                            const int* __restrict__ wsc, float* __restrict__ e,
                                                            float* __restrict__ aux, int R, int H, int maxch) {
  __shared__ float red[4];
  const int seq = blockIdx.x, t = threadIdx.x;
  int start, stop;
  seq_rows(cu, seq, R, start, stop);
  const int nch = min((stop - start + ROWS - 1) / ROWS, maxch);
  if (nch <= 1) return;  // finished by pool_fwd_kernel
  float s8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int cnt = 0;
  for (int ch = 0; ch < nch; ++ch) {
    if (t < H / 8) {
      const float* src = ws + ((int64_t)seq * maxch + ch) * H + 8 * t;
      const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + 4);
      s8[0] += a.x; s8[1] += a.y; s8[2] += a.z; s8[3] += a.w;
      s8[4] += b.x; s8[5] += b.y; s8[6] += b.z; s8[7] += b.w;
    }
    cnt += wsc[(int64_t)seq * maxch + ch];
  }
  pool_finish(s8, cnt, seq, H, e, aux, red);
}

__global__ __launch_bounds__(256) void pool_bwd_kernel(const float* __restrict__ de, const float* __restrict__ e,
                                                       const float* __restrict__ aux, const int* __restrict__ cu,
                                                       const int64_t* __restrict__ mask, bf16_t* __restrict__ dh,
                                                       int R, int H, int n) {
  __shared__ float red[4];
  const int seq = blockIdx.y, ch = blockIdx.x, t = threadIdx.x;
  const int ncg = H / 8, nrg = 256 / ncg, rg = t / ncg, c = t - rg * ncg;
  const u32x4 zero = u32x4{0u, 0u, 0u, 0u};
  if (seq == n) {  // the rows outside every sequence: [0, cu[0]) and [cu[n], R)
    const int begin = min(max(cu[0], 0), R), end = min(max(cu[n], begin), R);
    const int dead = begin + (R - end);
    if (rg < nrg)
      for (int base = ch * ROWS; base < dead; base += ROWS * (int)gridDim.x)
        for (int v = base + rg; v < min(base + ROWS, dead); v += nrg) {
          const int row = v < begin ? v : end + (v - begin);
          *reinterpret_cast<u32x4*>(dh + (int64_t)row * H + 8 * c) = zero;
        }
    return;
  }
  int start, stop;
  seq_rows(cu, seq, R, start, stop);
  if (ch * ROWS >= stop - start) return;
  const int r0 = start + ch * ROWS, r1 = min(r0 + ROWS, stop);
  float ev[8], dv[8];
  {
    const float* ep = e + (int64_t)seq * H + 8 * c;
    const float* dp = de + (int64_t)seq * H + 8 * c;
    const f32x4 a = *reinterpret_cast<const f32x4*>(ep), b = *reinterpret_cast<const f32x4*>(ep + 4);
    const f32x4 x = *reinterpret_cast<const f32x4*>(dp), y = *reinterpret_cast<const f32x4*>(dp + 4);
    ev[0] = a.x; ev[1] = a.y; ev[2] = a.z; ev[3] = a.w; ev[4] = b.x; ev[5] = b.y; ev[6] = b.z; ev[7] = b.w;
    dv[0] = x.x; dv[1] = x.y; dv[2] = x.z; dv[3] = x.w; dv[4] = y.x; dv[5] = y.y; dv[6] = y.z; dv[7] = y.w;
  }
  float dot = 0.f;
  if (rg == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) dot += ev[k] * dv[k];
  }
  dot = block_sum(dot, red);
  const float inv = aux[2 * (int64_t)seq], cnt = aux[2 * (int64_t)seq + 1];
  const float f = cnt > 0.f ? inv / cnt : 0.f;
  float g[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) g[k] = (dv[k] - ev[k] * dot) * f;
  const u32x4 gw = head::pack8(g);
  if (rg < nrg)
    for (int row = r0 + rg; row < r1; row += nrg) {
      const bool live = mask == nullptr || mask[row] != 0;
      *reinterpret_cast<u32x4*>(dh + (int64_t)row * H + 8 * c) = live ? gw : zero;
    }
  // the rows past the grid's last chunk (an understated longest sequence: the forward did not read them)
  if (ch == (int)gridDim.x - 1 && rg < nrg)
    for (int row = r0 + ROWS + rg; row < stop; row += nrg)
      *reinterpret_cast<u32x4*>(dh + (int64_t)row * H + 8 * c) = zero;
}

// ------------------------------------------------------------------------------------------------ scores
constexpr int TS = 32;    // rows of an owner tile and of a streamed step
constexpr int KC = 128;   // columns of one streamed LDS tile
constexpr int LDT = 130;  // its row stride in floats (2 j + k: the 64 lanes of a fragment read hit 64 banks)
constexpr int LDW = 33;

struct Chunk {
  f32x4 v[4];
};

// rows row0 .. row0+31 (below nrows), columns k0 .. k0+127 (below H) of X (row stride ld); zeros outside
__device__ __forceinline__ void chunk_load(Chunk& p, const float* __restrict__ X, int64_t ld, int row0, int nrows,
                                           int k0, int H) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int idx = (int)threadIdx.x + 256 * q, r = idx >> 5, c = (idx & 31) * 4;
    const bool ok = row0 + r < nrows && k0 + c < H;
    p.v[q] = ok ? *reinterpret_cast<const f32x4*>(X + (int64_t)(row0 + r) * ld + k0 + c) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

__device__ __forceinline__ void chunk_store(const Chunk& p, float* buf) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int idx = (int)threadIdx.x + 256 * q, r = idx >> 5, c = (idx & 31) * 4;
    *reinterpret_cast<f32x2*>(buf + r * LDT + c) = f32x2{p.v[q].x, p.v[q].y};
    *reinterpret_cast<f32x2*>(buf + r * LDT + c + 2) = f32x2{p.v[q].z, p.v[q].w};
  }
}

// MODE 0: forward (lse2 [B][2] = {m, rest} / rec out). MODE 1: backward of one side (lse2 in, dout out). NC: 128-column
// chunks of H held as fragments. own / str: the owner's and the streamed side's row 0 of e (row stride ld = 2 H).
template <int MODE, int NC>
__global__ __launch_bounds__(256) void score_kernel(const float* __restrict__ own, const float* __restrict__ str,
                                                    int64_t ld, const int* __restrict__ valid, float scale2,
                                                    float* __restrict__ lse2, float* __restrict__ rec,
                                                    float* __restrict__ dout, const float* __restrict__ stats,
                                                    const float* __restrict__ dloss, float scale, int lse_streamed,
                                                    int B, int H) {
  __shared__ float buf[2][TS * LDT];
  __shared__ float red[4 * TS * LDW];
  __shared__ float wt[MODE == 1 ? TS * LDW : 1];
  const int t = threadIdx.x, w = t >> 6, l = t & 63, lj = l & 31, lk = l >> 5;
  const int tile0 = blockIdx.x * TS;
  const int nch = (H + KC - 1) / KC;
  const int slab0 = MODE == 1 ? (int)blockIdx.y * 2 * KC : 0;
  const int snch = MODE == 1 ? min(2, (H - slab0 + KC - 1) / KC) : 0;
  const int NI = nch + snch;
  const int nsteps = (B + TS - 1) / TS;
  const int total = nsteps * NI;

  // the owner tile's A fragments: row tile0 + lj, columns c·128 + w·32 + 2 s + lk
  float a[NC][16];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const int col = c * KC + w * 32 + 2 * s + lk, row = tile0 + lj;
      a[c][s] = (row < B && col < H) ? own[(int64_t)row * ld + col] : 0.f;
    }

  auto issue = [&](int it, Chunk& p) {
    const int step = it / NI, r = it - step * NI;
    const int k0 = r < nch ? r * KC : slab0 + (r - nch) * KC;
    chunk_load(p, str, ld, step * TS, B, k0, H);
  };

  Chunk p;
  issue(0, p);
  chunk_store(p, buf[0]);
  __syncthreads();

  // forward: the online state of row tile0 + t (threads 0 .. 31)
  float m = -INFINITY, rest = 0.f, diag = 0.f;
  int bidx = -1;
  f32x16 acc2[2];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc2[q][r] = 0.f;

  int it = 0;
  for (int step = 0; step < nsteps; ++step) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (c < nch) {
        const bool more = it + 1 < total;
        if (more) issue(it + 1, p);
        const float* cur = buf[it & 1] + lj * LDT + w * 32 + lk;
#pragma unroll
        for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[c][s], cur[2 * s], acc, 0, 0, 0);
        if (more) chunk_store(p, buf[(it + 1) & 1]);
        __syncthreads();
        ++it;
      }
    }
    // the 4 K-partials of the [owner][streamed] tile
#pragma unroll
    for (int r = 0; r < 16; ++r) red[(w * TS + 8 * (r >> 2) + 4 * lk + (r & 3)) * LDW + lj] = acc[r];
    __syncthreads();
    const int st0 = step * TS;
    // (s is the same sum of the same partials in both modes: the backward's s - m is exactly 0 at the forward's max)
    if constexpr (MODE == 0) {
      if (w == 0) {
        const int gj0 = st0 + lj;
        const bool vj = lk == 0 && gj0 < B && valid[gj0] != 0;
        const uint32_t live = (uint32_t)__ballot(vj);
        const int gi = tile0 + lj;
        if (lk == 0) {
          for (int j = 0; j < TS; ++j) {
            if (!((live >> j) & 1u)) continue;
            const float* rp = red + lj * LDW + j;
            const float s = (rp[0] + rp[TS * LDW]) + (rp[2 * TS * LDW] + rp[3 * TS * LDW]);
            if (st0 + j == gi) diag = s;
            if (s > m) {  // a new max (scale > 0: the first argmax of the logits too); the old one joins the rest
              rest = bidx < 0 ? 0.f : (rest + 1.0f) * exp2f((m - s) * scale2);
              m = s;
              bidx = st0 + j;
            } else {
              rest += exp2f((s - m) * scale2);
            }
          }
        }
      }
    } else {
      const int o = t >> 3, go = tile0 + o;
      const bool vo = go < B && valid[go] != 0;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = (t & 7) * 4 + u, gs = st0 + j;
        const float* rp = red + o * LDW + j;
        const float s = (rp[0] + rp[TS * LDW]) + (rp[2 * TS * LDW] + rp[3 * TS * LDW]);
        float wv = 0.f;
        if (vo && gs < B && valid[gs] != 0) {
          const float* rc = lse2 + 2 * (int64_t)(lse_streamed ? gs : go);
          const float ex = exp2f((s - rc[0]) * scale2);
          wv = (go == gs ? (ex - 1.0f) - rc[1] : ex) / (1.0f + rc[1]);
        }
        wt[o * LDW + j] = wv;
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (q < snch) {
          const bool more = it + 1 < total;
          if (more) issue(it + 1, p);
          const float* cur = buf[it & 1] + lk * LDT + w * 32 + lj;
          const float* wp = wt + lj * LDW + lk;
#pragma unroll
          for (int s = 0; s < 16; ++s)
            acc2[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(wp[2 * s], cur[2 * s * LDT], acc2[q], 0, 0, 0);
          if (more) chunk_store(p, buf[(it + 1) & 1]);
          __syncthreads();
          ++it;
        }
      }
    }
  }

  if constexpr (MODE == 0) {
    const int gi = tile0 + t;
    if (t < TS && gi < B) {
      const bool ok = valid[gi] != 0;
      lse2[2 * (int64_t)gi] = ok ? m : 0.f;
      lse2[2 * (int64_t)gi + 1] = ok ? rest : 0.f;
      rec[2 * (int64_t)gi] = ok ? log1pf(rest) + (m - diag) * scale : 0.f;
      rec[2 * (int64_t)gi + 1] = ok && bidx == gi ? 1.0f : 0.f;
    }
  } else {
    const float coef = dloss[0] * scale / fmaxf(stats[2], 1.0f);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if (q < snch) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int go = tile0 + 8 * (r >> 2) + 4 * lk + (r & 3), col = slab0 + q * KC + w * 32 + lj;
          if (go < B && col < H) dout[(int64_t)go * ld + col] = acc2[q][r] * coef;
        }
      }
    }
  }
}

// stats = {mean loss, hits, n_valid, loss sum}: the B records pass through LDS 256 at a time, field k summed by thread
// k in index order
__global__ __launch_bounds__(256) void score_stats_kernel(const float* __restrict__ rec, const int* __restrict__ valid,
                                                          int B, float* __restrict__ stats) {
  __shared__ float fb[3][256];
  __shared__ double tot[3];
  double s = 0.0;  // B fp32 records: the sum rounds once, on the way out
  for (int b0 = 0; b0 < B; b0 += 256) {
    const int nb = min(256, B - b0), i = threadIdx.x;
    if (i < nb) {
      fb[0][i] = rec[2 * (int64_t)(b0 + i)];
      fb[1][i] = rec[2 * (int64_t)(b0 + i) + 1];
      fb[2][i] = valid[b0 + i] != 0 ? 1.0f : 0.f;
    }
    __syncthreads();
    if (threadIdx.x < 3)
      for (int b = 0; b < nb; ++b) s += (double)fb[threadIdx.x][b];
    __syncthreads();
  }
  if (threadIdx.x < 3) tot[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    stats[0] = (float)(tot[0] / fmax(tot[2], 1.0));
    stats[1] = (float)tot[1];
    stats[2] = (float)tot[2];
    stats[3] = (float)tot[0];
  }
}

template <int MODE>
static void launch_score(dim3 grid, hipStream_t st, const float* own, const float* str, int64_t ld, const int* valid,
                         float scale, float* lse2, float* rec, float* dout, const float* stats, const float* dloss,
                         int lse_streamed, int B, int H) {
  const float scale2 = (float)((double)scale * 1.4426950408889634);
  if (H <= 2 * KC)
    hipLaunchKernelGGL((score_kernel<MODE, 2>), grid, dim3(256), 0, st, own, str, ld, valid, scale2, lse2, rec, dout,
                       stats, dloss, scale, lse_streamed, B, H);
  else if (H <= 6 * KC)
    hipLaunchKernelGGL((score_kernel<MODE, 6>), grid, dim3(256), 0, st, own, str, ld, valid, scale2, lse2, rec, dout,
                       stats, dloss, scale, lse_streamed, B, H);
  else
    hipLaunchKernelGGL((score_kernel<MODE, 8>), grid, dim3(256), 0, st, own, str, ld, valid, scale2, lse2, rec, dout,
                       stats, dloss, scale, lse_streamed, B, H);
  HSD_CHECK_LAUNCH();
}

}  // namespace sent

int sent_pool_chunks(int max_seqlen) { return std::max((max_seqlen + sent::ROWS - 1) / sent::ROWS, 1); }

void launch_sent_pool_fwd(const bf16_t* h, const int* cu, const int64_t* mask, float* e, float* aux, float* ws,
                          int* wsc, int R, int H, int n, int maxch, hipStream_t st) {
  hipLaunchKernelGGL(sent::pool_fwd_kernel, dim3(maxch, n), dim3(256), 0, st, h, cu, mask, e, aux, ws, wsc, R, H, maxch);
  HSD_CHECK_LAUNCH();
  if (maxch > 1) {
    hipLaunchKernelGGL(sent::pool_finalize_kernel, dim3(n), dim3(256), 0, st, cu, (const float*)ws, (const int*)wsc, e,
                       aux, R, H, maxch);
    HSD_CHECK_LAUNCH();
  }
}

void launch_sent_pool_bwd(const float* de, const float* e, const float* aux, const int* cu, const int64_t* mask,
                          bf16_t* dh, int R, int H, int n, int maxch, hipStream_t st) {
  hipLaunchKernelGGL(sent::pool_bwd_kernel, dim3(maxch, n + 1), dim3(256), 0, st, de, e, aux, cu, mask, dh, R, H, n);
  HSD_CHECK_LAUNCH();
}

void launch_sent_score_fwd(const float* e, const int* valid, float scale, float* lse2, float* rec, float* stats, int B,
                           int H, hipStream_t st) {
  sent::launch_score<0>(dim3((B + sent::TS - 1) / sent::TS), st, e, e + H, 2 * (int64_t)H, valid, scale, lse2, rec,
                        nullptr, nullptr, nullptr, 0, B, H);
  hipLaunchKernelGGL(sent::score_stats_kernel, dim3(1), dim3(256), 0, st, (const float*)rec, valid, B, stats);
  HSD_CHECK_LAUNCH();
}

void launch_sent_score_bwd(const float* e, const int* valid, float scale, const float* lse2, const float* stats,
                           const float* dloss, float* de, int B, int H, hipStream_t st) {
  const dim3 grid((B + sent::TS - 1) / sent::TS, (H + 2 * sent::KC - 1) / (2 * sent::KC));
  float* const lse = const_cast<float*>(lse2);
  // anchors own: da_i = Σ_j w_ij p_j (lse of the owner); then positives own: dp_j = Σ_i w_ij a_i (lse of the streamed)
  sent::launch_score<1>(grid, st, e, e + H, 2 * (int64_t)H, valid, scale, lse, nullptr, de, stats, dloss, 0, B, H);
  sent::launch_score<1>(grid, st, e + H, e, 2 * (int64_t)H, valid, scale, lse, nullptr, de + H, stats, dloss, 1, B, H);
}

}  // namespace hsd
