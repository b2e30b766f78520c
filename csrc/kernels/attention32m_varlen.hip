// fp32 variable-length (padding-free) attention on the bf16 matrix cores: the split products of attention32m.hip walked
// over a packed buffer by the offsets of attention_varlen.hip (--pack_sequences true --dtype fp32). head_dim 64.
//
// Input  qkv [T, 3H] fp32 carried as its two bf16 halves qkv_hi + qkv_lo (split2): B sequences packed back to back,
// sequence b in rows cu[b] .. cu[b+1]-1 (cu = cu_seqlens, device int32 [B+1]); rows cu[B] .. T-1 are dead. No mask
// tensor: a key is visible iff it lies in the query's own sequence. Dropout element (head h, packed row t, key j within
// the sequence) is row h*T + t, column j of the site (ops/rng.py), the site of the bf16 varlen kernels; the backward
// re-hashes the bits. out [T, H] and dqkv [T, 3H] are fp32, lse2 and delta are [heads, T].
//
// Three kernels on a (ceil(max_seqlen / 128), B * heads) grid, one workgroup = 128 rows of one (sequence, head), a wave
// = 32 rows on the MFMA lane; a workgroup whose block starts at or past its sequence's length L exits before its first
// barrier (a zero-length sequence writes nothing):
//   forward   queries on lanes, K/V streamed in 64-key tiles, online softmax in fp32;
//   dK / dV   keys on lanes, Q/dO streamed in 64-query tiles together with the tile's lse2 / delta / dropout row words;
//   dQ        queries on lanes, K/V streamed: every dqkv element is written once by one thread, no atomics, the same
//             bits from run to run.
// Every product is mma3 (ah·bh + al·bh + ah·bl), P and dS are split on the fly (pack8_split).
//
// Data movement. The streamed hi / lo pair is 4 [64][64] images per tile, double-buffered (2 x 4 x 8 KB = 64 KB, two
// workgroups per CU) and filled by the LDS DMA of attention32m.hip: tile t + 1 is requested right after the barrier
// that hands over tile t and lands under tile t's MFMAs. The ragged tail: the DMA takes its source address PER LANE,
// so every lane clamps its source row into the sequence (row min(j, L-1)) -- the last tile is filled by the same 8
// instructions per image as a full one, its rows >= L holding copies of row L-1. That keeps the asynchronous path for
// every tile (register staging with zero fill, as attention_varlen.hip's stage_kv does, would put a global load, a
// wait and an LDS store of the whole tile on the waves that are to issue MFMAs), and it keeps every address inside the
// sequence: no row of another sequence, no dead row and no row >= T is ever read, so no result depends on them. The
// copies are finite and never reach a result: scores of keys >= L are set to -inf before the softmax (P = 0 exactly),
// P and dS of keys >= L (dQ) and of query rows >= L (dK/dV) are set to 0 by a compare against the tile's row limit.
// Lanes whose own row is >= L work on a copy of row L-1 and store nothing. The dK/dV kernel's per-row lse2 and delta
// take the same road, 64 clamped rows per tile by one 4-byte-per-lane DMA each, so no register holds them over a tile.
//
// Sequence bounds are clamped into [0, T] on the device (seq_span), so no load or store touches a row >= T whatever
// cu holds. Dead rows of out / lse2 (forward) and dqkv (dQ kernel) are written as zeros by the x = 0 workgroups of the
// last sequence, one per head. There is no limit on max_seqlen: nothing of O(L) lives in LDS.
#include "attn32m_common.h"

namespace hsd {
namespace a32mv {

using namespace a32m;

struct Span {
  int start, len;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ Span seq_span(const int* __restrict__ cu, int b, int T) {
  const int s = clampi(cu[b], 0, T);
  const int e = clampi(cu[b + 1], s, T);
  return {s, e - s};
}

// LDS DMA of one wave: lane i's 16 B (X4) or 4 B at `src` (per lane) land at lds + i * 16 (or 4); lds is wave-uniform
template <bool X4, typename T>
__device__ __forceinline__ void dma_lanes(T* lds, const T* src) {
  const uint32_t dst =
      (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(size_t)(__attribute__((address_space(3))) T*)lds);
  unsigned keep;
  if constexpr (X4)
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(src), "s"(dst)
                 : "memory");
  else
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(src), "s"(dst)
                 : "memory");
}

// rows row0 .. row0+63 of the sequence at `base` (row stride ld, 64 columns), each clamped to row `last`, into a
// [64][64] image: dma_tile with the clamp on the per-lane source row
__device__ __forceinline__ void dma_tile_seq(bf16_t* img, const bf16_t* __restrict__ base, int64_t ld, int row0,
                                             int last, int wave, int lane) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int g = wave * 2 + i;
    const int row = g * 8 + (lane >> 3);
    const int lc = (lane & 7) ^ swz(row);
    dma_lanes<true>(img + g * 512, base + (int64_t)min(row0 + row, last) * ld + lc * 8);
  }
}

// zero rows t0 .. T-1, columns col0 .. col0+63 of a [T][ld] fp32 matrix (256 threads)
__device__ __forceinline__ void zero_rows64(float* __restrict__ m, int64_t ld, int col0, int t0, int T, int tid) {
  const int n = (T - t0) * 16;
  for (int i = tid; i < n; i += 256) {
    const int row = t0 + (i >> 4), ch = i & 15;
    *reinterpret_cast<f32x4*>(m + (int64_t)row * ld + col0 + ch * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

// ------------------------------------------------------------------------------------------------ forward
template <bool DROP>
__global__ __launch_bounds__(256, 2) void attn32m_varlen_fwd_kernel(const bf16_t* __restrict__ qh_all,
                                                                    const bf16_t* __restrict__ ql_all,
                                                                    const int* __restrict__ cu, float* __restrict__ out,
                                                                    float* __restrict__ lse2, int T, int B, int heads,
                                                                    float sl2, DropoutParams dp) {
  dp = resolve_seed(dp);
  __shared__ __attribute__((aligned(16))) bf16_t lds[2 * 4 * TILE];  // 2 stages x [Kh Kl Vh Vl]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hf = lane >> 5;
  const int b = blockIdx.y / heads, hh = blockIdx.y % heads;
  const int H = heads * D, ld = 3 * H;
  if (blockIdx.x == 0 && b == B - 1) {  // dead rows of this head
    const int t0 = clampi(cu[B], 0, T);
    zero_rows64(out, H, hh * D, t0, T, tid);
    for (int t = t0 + tid; t < T; t += 256) lse2[(int64_t)hh * T + t] = 0.f;
  }
  const Span sp = seq_span(cu, b, T);
  const int L = sp.len, last = L - 1;
  if ((int)blockIdx.x * 128 >= L) return;
  const bf16_t* bh_ = qh_all + (int64_t)sp.start * ld + hh * D;
  const bf16_t* bl_ = ql_all + (int64_t)sp.start * ld + hh * D;
  const int q0 = blockIdx.x * 128 + wave * 32;
  const int q = q0 + r, qc = min(q, last);
  const int nt = (L + 63) / 64;
  auto dma = [&](int stg, int kt) {
    bf16_t* st = lds + stg * 4 * TILE;
    dma_tile_seq(st, bh_ + H, ld, kt * 64, last, wave, lane);
    dma_tile_seq(st + TILE, bl_ + H, ld, kt * 64, last, wave, lane);
    dma_tile_seq(st + 2 * TILE, bh_ + 2 * H, ld, kt * 64, last, wave, lane);
    dma_tile_seq(st + 3 * TILE, bl_ + 2 * H, ld, kt * 64, last, wave, lane);
  };
  dma(0, 0);
  bf16x8 qh[4], ql[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    qh[s] = *reinterpret_cast<const bf16x8*>(bh_ + (int64_t)qc * ld + 16 * s + 8 * hf);
    ql[s] = *reinterpret_cast<const bf16x8*>(bl_ + (int64_t)qc * ld + 16 * s + 8 * hf);
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    settle(qh[s]);
    settle(ql[s]);
  }
  f32x16 o0 = {}, o1 = {};
  float m = -INFINITY, l = 0.f;
  // dropout: row word of (head, packed row) with the hf term folded in; the tile's column word is XORed in per tile
  uint32_t xq = 0;
  if constexpr (DROP)
    xq = dropout_row((uint32_t)hh * (uint32_t)T + (uint32_t)(sp.start + qc), dp) ^ drop_col(2u * (uint32_t)hf);
#pragma unroll 1
  for (int kt = 0; kt < nt; ++kt) {
    tile_sync();  // tile kt landed (the only DMA in flight); every wave is done with tile kt - 1's stage
    if (kt + 1 < nt) dma((kt + 1) & 1, kt + 1);
    const bf16_t* Kh = lds + (kt & 1) * 4 * TILE;
    const bf16_t* Kl = Kh + TILE;
    const bf16_t* Vh = Kh + 2 * TILE;
    const bf16_t* Vl = Kh + 3 * TILE;
    f32x16 st[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      st[kb] = f32x16{};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int o = toff(kb * 32 + r, 16 * s + 8 * hf);
        st[kb] = mma3(*reinterpret_cast<const bf16x8*>(Kh + o), *reinterpret_cast<const bf16x8*>(Kl + o), qh[s], ql[s],
                      st[kb]);
      }
    }
    // register reg of st[kb] is key kt*64 + kb*32 + (reg & 3) + 8 (reg >> 2) + 4 hf of the sequence: visible iff < L
    const int lim = L - kt * 64 - 4 * hf;
    float mx = m;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const float x = kb * 32 + (reg & 3) + 8 * (reg >> 2) < lim ? st[kb][reg] * sl2 : -INFINITY;
        st[kb][reg] = x;
        mx = fmaxf(mx, x);
      }
    mx = max_xor32(mx);  // finite: key kt*64 of every tile is < L
    const float alpha = __builtin_amdgcn_exp2f(m - mx);
    m = mx;
    float ls = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const float p = __builtin_amdgcn_exp2f(st[kb][reg] - mx);
        ls += p;
        st[kb][reg] = p;
      }
    l = fmaf(l, alpha, ls);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      o0[reg] *= alpha;
      o1[reg] *= alpha;
    }
    if constexpr (DROP) {
      const uint32_t xt = xq ^ drop_col(32u * (uint32_t)kt);
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int reg = 0; reg < 16; reg += 2) {
          const uint32_t bits = drop_fin(xt ^ drop_col((uint32_t)(16 * kb + 4 * (reg >> 2) + ((reg >> 1) & 1))));
          st[kb][reg] = keep_lo(bits, dp.thr) ? st[kb][reg] : 0.f;
          st[kb][reg + 1] = keep_hi(bits, dp.thr) ? st[kb][reg + 1] : 0.f;
        }
    }
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8 ph, pl;
        pack8_split(st[kb], s, ph, pl);
        o0 = mma3(trA(Vh, kb * 32, s, 0, lane), trA(Vl, kb * 32, s, 0, lane), ph, pl, o0);
        o1 = mma3(trA(Vh, kb * 32, s, 1, lane), trA(Vl, kb * 32, s, 1, lane), ph, pl, o1);
      }
  }
  l = sum_xor32(l);
  if (q < L) {
    if (hf == 0) lse2[(int64_t)hh * T + sp.start + q] = m + __log2f(l);
    const float oscale = (DROP ? dp.scale : 1.0f) / l;
    store_rows32(o0, o1, oscale, out + (int64_t)(sp.start + q0) * H + hh * D, H, lane);
  }
}

// ------------------------------------------------------------------------------------------------ backward dK, dV
template <bool DROP>
__global__ __launch_bounds__(256, 2) void attn32m_varlen_bwd_kv_kernel(
    const bf16_t* __restrict__ qh_all, const bf16_t* __restrict__ ql_all, const bf16_t* __restrict__ doh_all,
    const bf16_t* __restrict__ dol_all, const int* __restrict__ cu, const float* __restrict__ lse2,
    const float* __restrict__ delta, float* __restrict__ dqkv, int T, int heads, float sl2, float scale,
    DropoutParams dp) {
  dp = resolve_seed(dp);
  // 2 stages x [Qh Ql dOh dOl], and per stage the 64 lse2 / delta / dropout row words of the tile's query rows
  __shared__ __attribute__((aligned(16))) bf16_t lds[2 * 4 * TILE];
  __shared__ __attribute__((aligned(16))) float lse_s[2 * 64], del_s[2 * 64];
  __shared__ uint32_t rw_s[2 * 64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hf = lane >> 5;
  const int b = blockIdx.y / heads, hh = blockIdx.y % heads;
  const int H = heads * D, ld = 3 * H;
  const Span sp = seq_span(cu, b, T);
  const int L = sp.len, last = L - 1;
  if ((int)blockIdx.x * 128 >= L) return;
  const int64_t boff = (int64_t)sp.start * ld + hh * D;
  const int64_t doff = (int64_t)sp.start * H + hh * D;
  const int64_t roff = (int64_t)hh * T + sp.start;  // lse2 / delta / dropout row of the sequence's first query
  const int k0 = blockIdx.x * 128 + wave * 32;
  const int key = k0 + r, kc = min(key, last);
  const int nt = (L + 63) / 64;
  auto dma = [&](int stg, int qt) {
    bf16_t* st = lds + stg * 4 * TILE;
    dma_tile_seq(st, qh_all + boff, ld, qt * 64, last, wave, lane);
    dma_tile_seq(st + TILE, ql_all + boff, ld, qt * 64, last, wave, lane);
    dma_tile_seq(st + 2 * TILE, doh_all + doff, H, qt * 64, last, wave, lane);
    dma_tile_seq(st + 3 * TILE, dol_all + doff, H, qt * 64, last, wave, lane);
  };
  // the tile's 64 query rows (clamped like the images' rows): lse2 by wave 0's DMA, delta by wave 1's, and the dropout
  // row words hashed by wave 2 (stored at once: the stage was last read in tile qt - 2)
  auto meta = [&](int stg, int qt) {
    const int64_t i = roff + min(qt * 64 + lane, last);
    if (wave == 0) dma_lanes<false>(lse_s + stg * 64, lse2 + i);
    if (wave == 1) dma_lanes<false>(del_s + stg * 64, delta + i);
    if (DROP && wave == 2) rw_s[stg * 64 + lane] = dropout_row((uint32_t)i, dp);
  };
  dma(0, 0);
  meta(0, 0);
  bf16x8 kh[4], kl[4], vh[4], vl[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int64_t o = boff + (int64_t)kc * ld + 16 * s + 8 * hf;
    kh[s] = *reinterpret_cast<const bf16x8*>(qh_all + o + H);
    kl[s] = *reinterpret_cast<const bf16x8*>(ql_all + o + H);
    vh[s] = *reinterpret_cast<const bf16x8*>(qh_all + o + 2 * H);
    vl[s] = *reinterpret_cast<const bf16x8*>(ql_all + o + 2 * H);
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    settle(kh[s]);
    settle(kl[s]);
    settle(vh[s]);
    settle(vl[s]);
  }
  f32x16 dk0 = {}, dk1 = {}, dv0 = {}, dv1 = {};
  const bool odd = (lane & 1) != 0;
  // dropout: the 32-bit word of (query, key pair) is shared by lanes l, l ^ 1: the even lane computes query qi0's, the
  // odd lane query qi0 + 1's, and they swap (one DPP move)
  const uint32_t ck = drop_col((uint32_t)kc >> 1);
  const int qsel = 4 * hf + (odd ? 1 : 0);
#pragma unroll 1
  for (int qt = 0; qt < nt; ++qt) {
    tile_sync();  // tile qt's images and row values landed; every wave is done with tile qt - 1's stage
    if (qt + 1 < nt) {
      dma((qt + 1) & 1, qt + 1);
      meta((qt + 1) & 1, qt + 1);
    }
    const int limq = L - qt * 64 - 4 * hf;  // a register's query offset in the tile (less 4 hf) < limq: a real row
    const int so = (qt & 1) * 64;
    const bf16_t* Qh = lds + (qt & 1) * 4 * TILE;
    const bf16_t* Ql = Qh + TILE;
    const bf16_t* dOh = Qh + 2 * TILE;
    const bf16_t* dOl = Qh + 3 * TILE;
#pragma unroll 1  // 48 MFMAs per trip; unrolled, the dropout instantiation spills three times as much
    for (int qs = 0; qs < 2; ++qs) {
      f32x16 sacc = {}, dpacc = {};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int o = toff(qs * 32 + r, 16 * s + 8 * hf);
        sacc = mma3(*reinterpret_cast<const bf16x8*>(Qh + o), *reinterpret_cast<const bf16x8*>(Ql + o), kh[s], kl[s],
                    sacc);
        dpacc = mma3(*reinterpret_cast<const bf16x8*>(dOh + o), *reinterpret_cast<const bf16x8*>(dOl + o), vh[s],
                     vl[s], dpacc);
      }
      // rows: query qi = (reg & 3) + 8 (reg >> 2) + 4 hf of the sub-block; column (lane): key
      f32x16 pd, ds;
#pragma unroll
      for (int reg = 0; reg < 16; reg += 2) {
        const int qi0 = so + qs * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * hf;
        const f32x2 lse = *reinterpret_cast<const f32x2*>(lse_s + qi0);
        const f32x2 del = *reinterpret_cast<const f32x2*>(del_s + qi0);
        const int qo = qs * 32 + (reg & 3) + 8 * (reg >> 2);  // even; reg + 1 is the next query
        const float p0 = qo < limq ? __builtin_amdgcn_exp2f(sacc[reg] * sl2 - lse[0]) : 0.f;
        const float p1 = qo + 1 < limq ? __builtin_amdgcn_exp2f(sacc[reg + 1] * sl2 - lse[1]) : 0.f;
        float f0 = 1.f, f1 = 1.f;
        if constexpr (DROP) {
          const uint32_t bits = drop_fin(rw_s[so + qs * 32 + (reg & 3) + 8 * (reg >> 2) + qsel] ^ ck);
          const uint32_t other = dpp_xor1(bits);
          f0 = keep_factor(odd ? other : bits, kc & 1, dp);
          f1 = keep_factor(odd ? bits : other, kc & 1, dp);
        }
        pd[reg] = p0 * f0;
        pd[reg + 1] = p1 * f1;
        ds[reg] = p0 * fmaf(dpacc[reg], f0, -del[0]);
        ds[reg + 1] = p1 * fmaf(dpacc[reg + 1], f1, -del[1]);
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8 ph, pl, sh, sl;
        pack8_split(pd, s, ph, pl);
        pack8_split(ds, s, sh, sl);
        dv0 = mma3(trA(dOh, qs * 32, s, 0, lane), trA(dOl, qs * 32, s, 0, lane), ph, pl, dv0);
        dv1 = mma3(trA(dOh, qs * 32, s, 1, lane), trA(dOl, qs * 32, s, 1, lane), ph, pl, dv1);
        dk0 = mma3(trA(Qh, qs * 32, s, 0, lane), trA(Ql, qs * 32, s, 0, lane), sh, sl, dk0);
        dk1 = mma3(trA(Qh, qs * 32, s, 1, lane), trA(Ql, qs * 32, s, 1, lane), sh, sl, dk1);
      }
    }
  }
  if (key < L) {
    float* rowbase = dqkv + (int64_t)(sp.start + k0) * ld + hh * D;
    store_rows32(dv0, dv1, 1.0f, rowbase + 2 * H, ld, lane);
    store_rows32(dk0, dk1, scale, rowbase + H, ld, lane);
  }
}

// ------------------------------------------------------------------------------------------------ backward dQ
template <bool DROP>
__global__ __launch_bounds__(256, 2) void attn32m_varlen_bwd_q_kernel(
    const bf16_t* __restrict__ qh_all, const bf16_t* __restrict__ ql_all, const bf16_t* __restrict__ doh_all,
    const bf16_t* __restrict__ dol_all, const int* __restrict__ cu, const float* __restrict__ lse2,
    const float* __restrict__ delta, float* __restrict__ dqkv, int T, int B, int heads, float sl2, float scale,
    DropoutParams dp) {
  dp = resolve_seed(dp);
  __shared__ __attribute__((aligned(16))) bf16_t lds[2 * 4 * TILE];  // 2 stages x [Kh Kl Vh Vl]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hf = lane >> 5;
  const int b = blockIdx.y / heads, hh = blockIdx.y % heads;
  const int H = heads * D, ld = 3 * H;
  if (blockIdx.x == 0 && b == B - 1) {  // dead rows: the q, k and v columns of this head
    const int t0 = clampi(cu[B], 0, T);
#pragma unroll
    for (int part = 0; part < 3; ++part) zero_rows64(dqkv, ld, part * H + hh * D, t0, T, tid);
  }
  const Span sp = seq_span(cu, b, T);
  const int L = sp.len, last = L - 1;
  if ((int)blockIdx.x * 128 >= L) return;
  const int64_t boff = (int64_t)sp.start * ld + hh * D;
  const int64_t doff = (int64_t)sp.start * H + hh * D;
  const int q0 = blockIdx.x * 128 + wave * 32;
  const int q = q0 + r, qc = min(q, last);
  const int nt = (L + 63) / 64;
  auto dma = [&](int stg, int kt) {
    bf16_t* st = lds + stg * 4 * TILE;
    dma_tile_seq(st, qh_all + boff + H, ld, kt * 64, last, wave, lane);
    dma_tile_seq(st + TILE, ql_all + boff + H, ld, kt * 64, last, wave, lane);
    dma_tile_seq(st + 2 * TILE, qh_all + boff + 2 * H, ld, kt * 64, last, wave, lane);
    dma_tile_seq(st + 3 * TILE, ql_all + boff + 2 * H, ld, kt * 64, last, wave, lane);
  };
  dma(0, 0);
  bf16x8 qh[4], ql[4], dh[4], dl[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int64_t o = boff + (int64_t)qc * ld + 16 * s + 8 * hf;
    const int64_t od = doff + (int64_t)qc * H + 16 * s + 8 * hf;
    qh[s] = *reinterpret_cast<const bf16x8*>(qh_all + o);
    ql[s] = *reinterpret_cast<const bf16x8*>(ql_all + o);
    dh[s] = *reinterpret_cast<const bf16x8*>(doh_all + od);
    dl[s] = *reinterpret_cast<const bf16x8*>(dol_all + od);
  }
  const int64_t ri = (int64_t)hh * T + sp.start + qc;
  const float lse_q = lse2[ri];
  const float del_q = delta[ri];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    settle(qh[s]);
    settle(ql[s]);
    settle(dh[s]);
    settle(dl[s]);
  }
  settle(lse_q);
  settle(del_q);
  f32x16 dq0 = {}, dq1 = {};
  uint32_t xq = 0;
  if constexpr (DROP) xq = dropout_row((uint32_t)ri, dp) ^ drop_col(2u * (uint32_t)hf);
#pragma unroll 1
  for (int kt = 0; kt < nt; ++kt) {
    tile_sync();
    if (kt + 1 < nt) dma((kt + 1) & 1, kt + 1);
    const bf16_t* Kh = lds + (kt & 1) * 4 * TILE;
    const bf16_t* Kl = Kh + TILE;
    const bf16_t* Vh = Kh + 2 * TILE;
    const bf16_t* Vl = Kh + 3 * TILE;
    const uint32_t xt = DROP ? xq ^ drop_col(32u * (uint32_t)kt) : 0u;
    const int lim = L - kt * 64 - 4 * hf;  // as the forward: a register's key offset in the tile (less 4 hf) < lim
#pragma unroll 1  // 36 MFMAs per trip; unrolled, the dropout instantiation needs more than 256 VGPRs
    for (int kb = 0; kb < 2; ++kb) {
      // Sᵀ[key][q] = K·Qᵀ, dPᵀ[key][q] = V·dOᵀ (query on the lane, key in the registers)
      f32x16 sacc = {}, dpacc = {};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int o = toff(kb * 32 + r, 16 * s + 8 * hf);
        sacc = mma3(*reinterpret_cast<const bf16x8*>(Kh + o), *reinterpret_cast<const bf16x8*>(Kl + o), qh[s], ql[s],
                    sacc);
        dpacc = mma3(*reinterpret_cast<const bf16x8*>(Vh + o), *reinterpret_cast<const bf16x8*>(Vl + o), dh[s], dl[s],
                     dpacc);
      }
      f32x16 ds;
#pragma unroll
      for (int reg = 0; reg < 16; reg += 2) {
        const int ko = kb * 32 + (reg & 3) + 8 * (reg >> 2);  // even; reg + 1 is the next key
        const float p0 = ko < lim ? __builtin_amdgcn_exp2f(sacc[reg] * sl2 - lse_q) : 0.f;
        const float p1 = ko + 1 < lim ? __builtin_amdgcn_exp2f(sacc[reg + 1] * sl2 - lse_q) : 0.f;
        float f0 = 1.f, f1 = 1.f;
        if constexpr (DROP) {
          const uint32_t bits = drop_fin(xt ^ drop_col((uint32_t)(16 * kb + 4 * (reg >> 2) + ((reg >> 1) & 1))));
          f0 = keep_factor(bits, 0, dp);
          f1 = keep_factor(bits, 1, dp);
        }
        ds[reg] = p0 * fmaf(dpacc[reg], f0, -del_q);
        ds[reg + 1] = p1 * fmaf(dpacc[reg + 1], f1, -del_q);
      }
      // dQᵀ[d][q] += Σ_key Kᵀ[d][key] dSᵀ[key][q]
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8 sh, sl;
        pack8_split(ds, s, sh, sl);
        dq0 = mma3(trA(Kh, kb * 32, s, 0, lane), trA(Kl, kb * 32, s, 0, lane), sh, sl, dq0);
        dq1 = mma3(trA(Kh, kb * 32, s, 1, lane), trA(Kl, kb * 32, s, 1, lane), sh, sl, dq1);
      }
    }
  }
  if (q < L) store_rows32(dq0, dq1, scale, dqkv + (int64_t)(sp.start + q0) * ld + hh * D, ld, lane);
}

}  // namespace a32mv

void launch_attn32m_varlen_fwd(const bf16_t* qkv_hi, const bf16_t* qkv_lo, const int* cu_seqlens, float* out,
                               float* lse2, int T, int B, int max_seqlen, int heads, double p, uint64_t seed,
                               hipStream_t st) {
  DropoutParams dp = make_dropout(p, seed);
  const float sl2 = attn::kLog2e / sqrtf((float)attn::D);
  const dim3 grid((max_seqlen + 127) / 128, B * heads);
  if (dp.enabled)
    hipLaunchKernelGGL(a32mv::attn32m_varlen_fwd_kernel<true>, grid, dim3(256), 0, st, qkv_hi, qkv_lo, cu_seqlens, out,
                       lse2, T, B, heads, sl2, dp);
  else
    hipLaunchKernelGGL(a32mv::attn32m_varlen_fwd_kernel<false>, grid, dim3(256), 0, st, qkv_hi, qkv_lo, cu_seqlens, out,
                       lse2, T, B, heads, sl2, dp);
  HSD_CHECK_LAUNCH();
}

// delta: fp32 [heads, T] = rowsum(dO∘O) (launch_attn32_delta with B = 1, S = T)
void launch_attn32m_varlen_bwd(const bf16_t* qkv_hi, const bf16_t* qkv_lo, const bf16_t* do_hi, const bf16_t* do_lo,
                               const int* cu_seqlens, const float* lse2, const float* delta, float* dqkv, int T, int B,
                               int max_seqlen, int heads, double p, uint64_t seed, hipStream_t st) {
  DropoutParams dp = make_dropout(p, seed);
  const float sl2 = attn::kLog2e / sqrtf((float)attn::D);
  const float scale = 1.0f / sqrtf((float)attn::D);
  const dim3 grid((max_seqlen + 127) / 128, B * heads);
  if (dp.enabled) {
    hipLaunchKernelGGL(a32mv::attn32m_varlen_bwd_kv_kernel<true>, grid, dim3(256), 0, st, qkv_hi, qkv_lo, do_hi, do_lo,
                       cu_seqlens, lse2, delta, dqkv, T, heads, sl2, scale, dp);
    HSD_CHECK_LAUNCH();
    hipLaunchKernelGGL(a32mv::attn32m_varlen_bwd_q_kernel<true>, grid, dim3(256), 0, st, qkv_hi, qkv_lo, do_hi, do_lo,
                       cu_seqlens, lse2, delta, dqkv, T, B, heads, sl2, scale, dp);
  } else {
    hipLaunchKernelGGL(a32mv::attn32m_varlen_bwd_kv_kernel<false>, grid, dim3(256), 0, st, qkv_hi, qkv_lo, do_hi, do_lo,
                       cu_seqlens, lse2, delta, dqkv, T, heads, sl2, scale, dp);
    HSD_CHECK_LAUNCH();
    hipLaunchKernelGGL(a32mv::attn32m_varlen_bwd_q_kernel<false>, grid, dim3(256), 0, st, qkv_hi, qkv_lo, do_hi, do_lo,
                       cu_seqlens, lse2, delta, dqkv, T, B, heads, sl2, scale, dp);
  }
  HSD_CHECK_LAUNCH();
}

}  // namespace hsd
