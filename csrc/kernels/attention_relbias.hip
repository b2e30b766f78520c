// Self-attention with a relative-position (Toeplitz) bias on the scores, head_dim 64, bf16, CDNA4 MFMA
// (v_mfma_f32_32x32x16_bf16): the attention of the MPNet family. For one (sequence, head h) with L keys
//     s[i][j] = q_i.k_j / sqrt(64) + rel[h][j - i + (R-1)/2] + keybias[j],  P = softmax_j(s),  out = dropout(P).V
// rel is fp32 [heads, R], R odd and R >= 2 S - 1: a bias by distance. The kernels know nothing about buckets; the model
// gathers its bucket table into rel once per forward. The backward returns dqkv and drel[h][d] = sum_b sum_i dS[b,h,i,i+d]
// with dS = P o (dP - delta) (the bias enters after the 1/sqrt(d) scale, so drel takes dS before that factor).
//
// One kernel family for both layouts (the template switch kPacked is the addressing only, as in attention_d32.hip):
//   padded  qkv [B*S, 3H], S even, optional fp32 key bias [B, S] (scaled by log2 e, clamped at -1e30), lse2 [B, heads, S],
//           dropout row (b*heads + h)*S + i;
//   packed  qkv [T, 3H], cu_seqlens int32 [B+1] clamped into [0, T] and each length into [0, S = max_seqlen] on the
//           device, lse2 [heads, T], dropout row h*T + t; dead rows (cu[B] .. T-1) of out / lse2 / dqkv are written as
//           zeros by the x = 0 workgroups of the last sequence. Both are column j of the site (ops/reference.py).
// Grid and tiling are attention_varlen.hip's: (ceil(S / 128), B * heads) workgroups of 256 threads = 4 waves;
//   forward  128 queries of one (sequence, head), a wave = 32 queries on the MFMA lane (S^T = K.Q^T), K / V tiles of 64
//            keys in swizzled LDS images, P stays in registers as the next MFMA's B operand;
//   dK / dV  128 keys of one (sequence, head), a wave = 32 keys on the lane, dK^T / dV^T accumulate in registers over the
//            sequence's 32-query blocks; this kernel also forms drel (below);
//   dQ       queries on the lanes as the forward, so every dqkv element is written once by one thread: no fp32 atomics;
//   reduce   sums the drel partial rows of all workgroups in a fixed order.
//
// Bias read. A workgroup can reach L + 127 distances: d = j - i with its 128 rows on one side and the sequence's L rows
// on the other. It stages that window of the head's rel row, times log2 e (the kernels work in the log2 domain; the
// factor is applied here once, not per score), into LDS once: relw[x], x = d - d0, at most (1024 + 191) * 4 B = 4.7 KiB;
// distances outside the table read 0. Every score element then takes one LDS word. In the 32x32 accumulator layout the
// lane is the query (forward, dQ) or the key (dK/dV) and the register is the other index, so for a fixed register the 32
// lanes of a half-wave read 32 consecutive words -- descending addresses in the forward and dQ, ascending in dK/dV --
// which are 32 different banks: conflict-free. The other half-wave (hf = 1) sits 4 words further on; where both halves
// are served together the 28 shared words are the same address (a broadcast) and the rest distinct banks. The four
// registers of a group are consecutive words but start at any alignment, so they are four 32-bit reads (or two
// ds_read2_b32), not one 128-bit read.
//
// drel: dS through LDS, one thread per diagonal (the first design the feature's issue proposes; the alternative, a
// cross-lane skew that rotates each accumulator register by its row offset until diagonals line up on lanes, needs 16
// rotations by different lane counts per tile -- ds_bpermute round trips -- plus a tree over registers, and was not
// built or measured). The dK/dV kernel already holds each 32-query x 128-key dS tile in registers (fp32, before the bf16
// pack). Every wave stores its 32 x 32 part into dSs[32][136] (row = query; stride 136 words puts the hf = 1 half-wave's
// rows, 4 further down, 32 banks away from the hf = 0 rows: conflict-free stores). After a barrier thread t < 159 walks
// diagonal d' = t - 31 (key - query inside the tile) over the 32 query rows in ascending order: address
// 137 qi + t - 31, so consecutive threads read consecutive words, conflict-free, and adds the sum into dacc[t + 32 *
// (nqb - 1 - qb)], the workgroup's accumulator by distance in the same window coordinates as relw. During one pass a
// slot has exactly one owner and passes are separated by barriers, so the order of every addition is fixed. At its end
// the workgroup writes one full partial row [R] (zeros outside its window) to slab[(b * heads + h) * nblk + blk][R];
// a workgroup past its sequence's end writes zeros. The reducer adds the B * nblk rows of a head: 8 row groups (row
// index mod 8) in ascending order each, then the 8 group sums in ascending order. Same bits from run to run, and the
// same bits padded or packed, since both forms index the slab alike. Entries of rel no sequence reaches get exactly 0.
// Slab bytes: B * heads * ceil(S/128) * R * 4 (12.5 MB at B = 1024, S = 128, 12 heads), from the ops' shared workspace.
// Cost of the drel pass per 32-query block: 16 LDS stores per lane, one more barrier, 32 LDS loads in 159 of 256
// threads. Not tuned (by scope): the walk could be split over the idle threads, or moved to the dQ kernel.
//
// A padded sequence whose keys are ALL masked: as in the other kernels (common.h all_masked_scale) the scores are
// absorbed by the clamped bias, P is uniform, and the backward scales dqkv and the drel partial row by 1/S.
//
// Resource usage (hipcc -Rpass-analysis=kernel-resource-usage, built without the packed fp32 VALU forms, _build.py):
// see profiles/attn_relbias/resource_usage.txt; scratch is 0 in all seven kernels.
#include "attn_common.h"

namespace hsd {

using namespace attn;

namespace {

constexpr int kMaxLen = 1024;            // longest sequence (the window below is static LDS)
constexpr int kWin = kMaxLen + 192;      // distances one workgroup can reach, rounded: see the two window layouts
constexpr int kDsLd = 136;               // row stride (words) of the dS tile

__device__ __forceinline__ int clampr(int v, int lo, int hi) { return min(max(v, lo), hi); }

// one (sequence, head): first row, length, and where query 0 sits in lse2 / the dropout site
struct SeqHead {
  int start, len;
  uint32_t row0;
};

template <bool kPacked>
__device__ __forceinline__ SeqHead seq_head(const int* __restrict__ cu, int b, int h, int heads, int T, int S) {
  if (kPacked) {
    const int s = clampr(cu[b], 0, T);
    const int e = clampr(cu[b + 1], s, T);
    return {s, min(e - s, S), (uint32_t)h * (uint32_t)T + (uint32_t)s};
  }
  return {b * S, S, (uint32_t)(b * heads + h) * (uint32_t)S};
}

// additive score bias of key `key` (log2 domain)
__device__ __forceinline__ float key_bias2(const float* __restrict__ mask, int b, int S, int key, int L) {
  if (key >= L) return -INFINITY;
  if (!mask) return 0.f;
  return fmaxf(mask[(size_t)b * S + key] * kLog2e, -1e30f);
}

// relw[x] = log2(e) * rel_h[c + d0 + x], x in [0, n): the workgroup's window of the head's bias row (0 off the table)
__device__ __forceinline__ void stage_rel(float* relw, const float* __restrict__ rel_h, int R, int d0, int n, int tid) {
  const int c = (R - 1) >> 1;
  for (int x = tid; x < n; x += 256) {
    const int i = c + d0 + x;
    relw[x] = (i >= 0 && i < R) ? rel_h[i] * kLog2e : 0.f;
  }
}

// keys kt*64 .. kt*64+63 of the sequence at `base` into the [64][64] K / V images (rows >= L zero), their key biases
// into kbias
__device__ __forceinline__ void stage_kvb(bf16_t* Ks, bf16_t* Vs, float* kbias, const bf16_t* __restrict__ base, int ld,
                                          int H, int kt, int L, const float* __restrict__ mask, int b, int S, int tid) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = tid + 256 * i, row = c >> 3, ch = c & 7;
    const int key = kt * 64 + row;
    u32x4 kv = {0, 0, 0, 0}, vv = {0, 0, 0, 0};
    if (key < L) {
      const bf16_t* src = base + (size_t)key * ld + ch * 8;
      kv = *reinterpret_cast<const u32x4*>(src + H);
      vv = *reinterpret_cast<const u32x4*>(src + 2 * H);
    }
    *reinterpret_cast<u32x4*>(Ks + toff(row, ch * 8)) = kv;
    *reinterpret_cast<u32x4*>(Vs + toff(row, ch * 8)) = vv;
  }
  if (tid < 64) kbias[tid] = key_bias2(mask, b, S, kt * 64 + tid, L);
}

// acc pair (row on the lane, d = 32*blk + 8i + 4hf + 0..3 in registers) * scale -> 64 bf16 of one row
__device__ __forceinline__ void store_row(bf16_t* dst, const f32x16& a0, const f32x16& a1, float scale, int hf) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int d = 8 * i + 4 * hf;
    u32x2 w0, w1;
    w0.x = pack_bf2(a0[4 * i] * scale, a0[4 * i + 1] * scale);
    w0.y = pack_bf2(a0[4 * i + 2] * scale, a0[4 * i + 3] * scale);
    w1.x = pack_bf2(a1[4 * i] * scale, a1[4 * i + 1] * scale);
    w1.y = pack_bf2(a1[4 * i + 2] * scale, a1[4 * i + 3] * scale);
    *reinterpret_cast<u32x2*>(dst + d) = w0;
    *reinterpret_cast<u32x2*>(dst + 32 + d) = w1;
  }
}

// zero rows t0 .. T-1, columns col0 .. col0+63 of a [T][ld] bf16 matrix (256 threads)
__device__ __forceinline__ void zero_rows(bf16_t* __restrict__ m, int ld, int col0, int t0, int T, int tid) {
  const int n = (T - t0) * 8;
  for (int i = tid; i < n; i += 256) {
    const int row = t0 + (i >> 3), ch = i & 7;
    *reinterpret_cast<u32x4*>(m + (size_t)row * ld + col0 + ch * 8) = u32x4{0, 0, 0, 0};
  }
}

// ------------------------------------------------------------------------------------------------
// Window of the forward and dQ kernels (queries q0 .. q0+127 on the lanes): x = key - (query - q0) + 127, d0 = -q0 - 127,
// n = 64 ntiles + 127 <= 1024 + 63 + 127.
template <bool kPacked>
__global__ __launch_bounds__(256) void attn_relbias_fwd_kernel(const bf16_t* __restrict__ qkv, const int* __restrict__ cu,
                                                               const float* __restrict__ mask,
                                                               const float* __restrict__ rel, bf16_t* __restrict__ out,
                                                               float* __restrict__ lse2, int T, int B, int S, int heads,
                                                               int R, float sl2, DropoutParams dp) {
  dp = resolve_seed(dp);
  __shared__ __attribute__((aligned(16))) bf16_t Ks[64 * D];
  __shared__ __attribute__((aligned(16))) bf16_t Vs[64 * D];
  __shared__ __attribute__((aligned(16))) float kbias[64];
  __shared__ float relw[kWin];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hf = lane >> 5;
  const int b = blockIdx.y / heads, hh = blockIdx.y % heads;
  const int H = heads * D, ld = 3 * H;
  if (kPacked && blockIdx.x == 0 && b == B - 1) {  // dead rows of this head
    const int t0 = clampr(cu[B], 0, T);
    zero_rows(out, H, hh * D, t0, T, tid);
    for (int t = t0 + tid; t < T; t += 256) lse2[(size_t)hh * T + t] = 0.f;
  }
  const SeqHead sq = seq_head<kPacked>(cu, b, hh, heads, T, S);
  const int L = sq.len;
  const int q0 = blockIdx.x * 128;
  if (q0 >= L) return;
  const int q = q0 + wave * 32 + r;
  const int qc = min(q, L - 1);
  const bf16_t* base = qkv + (size_t)sq.start * ld + hh * D;
  const uint32_t drow = sq.row0 + (uint32_t)qc;
  const int ntiles = (L + 63) / 64;
  stage_rel(relw, rel + (size_t)hh * R, R, -q0 - 127, ntiles * 64 + 127, tid);  // visible after the loop's barriers
  const float* relq = relw + 127 - (wave * 32 + r);                             // + key

  bf16x8 qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(base + (size_t)qc * ld + 16 * s + 8 * hf);

  f32x16 o0 = {}, o1 = {};
  float m = -INFINITY, l = 0.f;
  for (int kt = 0; kt < ntiles; ++kt) {
    __syncthreads();
    stage_kvb(Ks, Vs, kbias, base, ld, H, kt, L, mask, b, S, tid);
    __syncthreads();
    f32x16 st[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      st[kb] = f32x16{};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        bf16x8 a = *reinterpret_cast<const bf16x8*>(Ks + toff(kb * 32 + r, 16 * s + 8 * hf));
        st[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, qf[s], st[kb], 0, 0, 0);
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k0 = 32 * kb + 8 * i + 4 * hf;  // keys k0 .. k0+3 of the tile in registers 4i .. 4i+3
        const f32x4 kb4 = *reinterpret_cast<const f32x4*>(kbias + k0);
        const float* rw = relq + kt * 64 + k0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float x = st[kb][4 * i + e] * sl2 + rw[e] + kb4[e];
          st[kb][4 * i + e] = x;
          mx = fmaxf(mx, x);
        }
      }
    mx = max_xor32(mx);  // finite: every tile holds at least one key < L, and the mask bias is clamped
    const float mn = fmaxf(m, mx);
    const float alpha = exp2f(m - mn);  // m = -inf on the first tile -> 0
    float ls = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const float p = exp2f(st[kb][reg] - mn);
        ls += p;
        st[kb][reg] = p;
      }
    ls = sum_xor32(ls);
    l = l * alpha + ls;
    m = mn;
    o0 *= alpha;
    o1 *= alpha;
    if (dp.enabled) {
      // column pair key / 2 = 32 kt + 16 kb + 4 (reg >> 2) + (reg >> 1 & 1) + 2 hf (disjoint bits)
      const uint32_t xt = dropout_row(drow, dp) ^ drop_col(32u * (uint32_t)kt + 2u * (uint32_t)hf);
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int reg = 0; reg < 16; reg += 2) {
          const uint32_t bits = drop_fin(xt ^ drop_col((uint32_t)(16 * kb + 4 * (reg >> 2) + ((reg >> 1) & 1))));
          st[kb][reg] *= keep_factor(bits, 0, dp);
          st[kb][reg + 1] *= keep_factor(bits, 1, dp);
        }
    }
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8 pb = pack8(st[kb], s);
        o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(trA(Vs, kb * 32, s, 0, lane), pb, o0, 0, 0, 0);
        o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(trA(Vs, kb * 32, s, 1, lane), pb, o1, 0, 0, 0);
      }
  }
  if (q < L) {
    store_row(out + (size_t)(sq.start + q) * H + hh * D, o0, o1, 1.0f / l, hf);
    if (hf == 0) lse2[(size_t)sq.row0 + q] = m + log2f(l);
  }
}

// ------------------------------------------------------------------------------------------------
// dK / dV and the drel partial row. Window (keys k0 .. k0+127 on the lanes, queries 0 .. 32 nqb - 1 in registers):
// x = (key - k0) - query + Qmax with Qmax = 32 nqb - 1, d0 = k0 - Qmax, n = 32 nqb + 127 <= 1024 + 31 + 127.
template <bool kPacked>
__global__ __launch_bounds__(256) void attn_relbias_bwd_kv_kernel(
    const bf16_t* __restrict__ qkv, const int* __restrict__ cu, const float* __restrict__ mask,
    const float* __restrict__ rel, const bf16_t* __restrict__ o, const bf16_t* __restrict__ dout,
    const float* __restrict__ lse2, bf16_t* __restrict__ dqkv, float* __restrict__ slab, int T, int S, int heads, int R,
    float sl2, float scale, DropoutParams dp) {
  dp = resolve_seed(dp);
  __shared__ __attribute__((aligned(16))) bf16_t Qs[32 * D];
  __shared__ __attribute__((aligned(16))) bf16_t dOs[32 * D];
  __shared__ float lse_s[32], del_s[32];
  __shared__ float relw[kWin];
  __shared__ float dacc[kWin];
  __shared__ float dSs[32 * kDsLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hf = lane >> 5;
  const int b = blockIdx.y / heads, hh = blockIdx.y % heads;
  const int H = heads * D, ld = 3 * H;
  const SeqHead sq = seq_head<kPacked>(cu, b, hh, heads, T, S);
  const int L = sq.len;
  const int kbase = blockIdx.x * 128;
  float* srow = slab + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * R;
  if (kbase >= L) {  // no keys here: a zero partial row
    for (int i = tid; i < R; i += 256) srow[i] = 0.f;
    return;
  }
  const int key = kbase + wave * 32 + r;
  const int kc = min(key, L - 1);
  const uint32_t ck = drop_col((uint32_t)kc >> 1);  // dropout column word of this lane's key
  const float kb2 = key_bias2(mask, b, S, kc, L);
  const bf16_t* base = qkv + (size_t)sq.start * ld + hh * D;
  const size_t obase = (size_t)sq.start * H + hh * D;
  // a padded sequence with every key masked: p below is 1 where 1/S is meant, folded into the output scales (common.h)
  const float pw = kPacked ? 1.0f : all_masked_scale(lse2[sq.row0], S);
  const int nqb = (L + 31) / 32;
  const int qmax = 32 * nqb - 1, nwin = 32 * nqb + 127, d0 = kbase - qmax;
  stage_rel(relw, rel + (size_t)hh * R, R, d0, nwin, tid);  // visible after the loop's barriers
  for (int x = tid; x < nwin; x += 256) dacc[x] = 0.f;
  const float* relk = relw + wave * 32 + r + qmax;  // - query

  // per-wave K and V B-fragments (key on the lane)
  bf16x8 kf[4], vf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    kf[s] = *reinterpret_cast<const bf16x8*>(base + (size_t)kc * ld + H + 16 * s + 8 * hf);
    vf[s] = *reinterpret_cast<const bf16x8*>(base + (size_t)kc * ld + 2 * H + 16 * s + 8 * hf);
  }
  const bool kvalid = key < L;
  f32x16 dk0 = {}, dk1 = {}, dv0 = {}, dv1 = {};
  for (int qb = 0; qb < nqb; ++qb) {
    __syncthreads();  // (also: the previous block's diagonal walk is done with dSs)
    {
      // Q / dO tiles (32 rows x 8 chunks = 256 chunks: one per thread), lse, delta = rowsum(dO*O)
      const int row = tid >> 3, ch = tid & 7;
      const int qq = qb * 32 + row;
      u32x4 qv = {0, 0, 0, 0}, dv = {0, 0, 0, 0}, ov = {0, 0, 0, 0};
      if (qq < L) {
        qv = *reinterpret_cast<const u32x4*>(base + (size_t)qq * ld + ch * 8);
        const size_t oo = obase + (size_t)qq * H + ch * 8;
        dv = *reinterpret_cast<const u32x4*>(dout + oo);
        ov = *reinterpret_cast<const u32x4*>(o + oo);
      }
      *reinterpret_cast<u32x4*>(Qs + toff(row, ch * 8)) = qv;
      *reinterpret_cast<u32x4*>(dOs + toff(row, ch * 8)) = dv;
      const float part = sum8_dpp(dot8_bf16(dv, ov));
      if (ch == 0) {
        del_s[row] = part;
        lse_s[row] = qq < L ? lse2[(size_t)sq.row0 + qq] : 0.f;
      }
    }
    __syncthreads();
    f32x16 sacc = {}, dpacc = {};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      bf16x8 aq = *reinterpret_cast<const bf16x8*>(Qs + toff(r, 16 * s + 8 * hf));
      sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aq, kf[s], sacc, 0, 0, 0);
      bf16x8 ad = *reinterpret_cast<const bf16x8*>(dOs + toff(r, 16 * s + 8 * hf));
      dpacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ad, vf[s], dpacc, 0, 0, 0);
    }
    // sacc / dpacc: col = key (lane), row qi = (reg&3) + 8*(reg>>2) + 4*hf
    f32x16 pd, ds;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int qi = (reg & 3) + 8 * (reg >> 2) + 4 * hf;
      const int qq = qb * 32 + qi;
      const float p = (kvalid && qq < L) ? exp2f(sacc[reg] * sl2 + relk[-qq] + kb2 - lse_s[qi]) : 0.f;
      float kf_ = 1.0f;
      if (dp.enabled) {
        kf_ = keep_factor(drop_fin(dropout_row(sq.row0 + (uint32_t)min(qq, L - 1), dp) ^ ck), kc & 1, dp);
      }
      pd[reg] = p * kf_;
      ds[reg] = p * (dpacc[reg] * kf_ - del_s[qi]);
      dSs[qi * kDsLd + wave * 32 + r] = ds[reg];
    }
    // dV^T += dO^T . Pd ; dK^T += Q^T . dS   (B operands straight from the accumulators)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 pb = pack8(pd, s);
      bf16x8 sb = pack8(ds, s);
      dv0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(trA(dOs, 0, s, 0, lane), pb, dv0, 0, 0, 0);
      dv1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(trA(dOs, 0, s, 1, lane), pb, dv1, 0, 0, 0);
      dk0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(trA(Qs, 0, s, 0, lane), sb, dk0, 0, 0, 0);
      dk1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(trA(Qs, 0, s, 1, lane), sb, dk1, 0, 0, 0);
    }
    __syncthreads();
    if (tid < 159) {  // diagonal key - query = tid - 31 of the 32 x 128 tile, rows in ascending order
      float acc = 0.f;
#pragma unroll 8
      for (int qi = 0; qi < 32; ++qi) {
        const int kl = qi + tid - 31;
        if (kl >= 0 && kl < 128) acc += dSs[qi * kDsLd + kl];
      }
      dacc[tid + 32 * (nqb - 1 - qb)] += acc;
    }
  }
  if (kvalid) {
    bf16_t* row = dqkv + (size_t)(sq.start + key) * ld + hh * D;
    store_row(row + H, dk0, dk1, scale * pw, hf);
    store_row(row + 2 * H, dv0, dv1, pw, hf);
  }
  __syncthreads();
  const int c = (R - 1) >> 1;
  for (int i = tid; i < R; i += 256) {
    const int x = i - c - d0;
    srow[i] = (x >= 0 && x < nwin) ? dacc[x] * pw : 0.f;
  }
}

// dQ: queries on the lanes, as the forward; S^T = K.Q^T and dP^T = V.dO^T per 64-key tile, dS^T stays in registers as
// the B operand of dQ^T += K^T . dS^T.
template <bool kPacked>
__global__ __launch_bounds__(256) void attn_relbias_bwd_q_kernel(
    const bf16_t* __restrict__ qkv, const int* __restrict__ cu, const float* __restrict__ mask,
    const float* __restrict__ rel, const bf16_t* __restrict__ o, const bf16_t* __restrict__ dout,
    const float* __restrict__ lse2, bf16_t* __restrict__ dqkv, int T, int B, int S, int heads, int R, float sl2,
    float scale, DropoutParams dp) {
  dp = resolve_seed(dp);
  __shared__ __attribute__((aligned(16))) bf16_t Ks[64 * D];
  __shared__ __attribute__((aligned(16))) bf16_t Vs[64 * D];
  __shared__ __attribute__((aligned(16))) float kbias[64];
  __shared__ float relw[kWin];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hf = lane >> 5;
  const int b = blockIdx.y / heads, hh = blockIdx.y % heads;
  const int H = heads * D, ld = 3 * H;
  if (kPacked && blockIdx.x == 0 && b == B - 1) {  // dead rows: the q, k and v columns of this head
    const int t0 = clampr(cu[B], 0, T);
#pragma unroll
    for (int part = 0; part < 3; ++part) zero_rows(dqkv, ld, part * H + hh * D, t0, T, tid);
  }
  const SeqHead sq = seq_head<kPacked>(cu, b, hh, heads, T, S);
  const int L = sq.len;
  const int q0 = blockIdx.x * 128;
  if (q0 >= L) return;
  const int q = q0 + wave * 32 + r;
  const int qc = min(q, L - 1);
  const bf16_t* base = qkv + (size_t)sq.start * ld + hh * D;
  const uint32_t drow = sq.row0 + (uint32_t)qc;
  const float pw = kPacked ? 1.0f : all_masked_scale(lse2[sq.row0], S);
  const int ntiles = (L + 63) / 64;
  stage_rel(relw, rel + (size_t)hh * R, R, -q0 - 127, ntiles * 64 + 127, tid);
  const float* relq = relw + 127 - (wave * 32 + r);

  bf16x8 qf[4], dof[4];
  float delta = 0.f;  // rowsum(dO * O): this lane holds half of the row, lane ^ 32 the other half
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    qf[s] = *reinterpret_cast<const bf16x8*>(base + (size_t)qc * ld + 16 * s + 8 * hf);
    const size_t oo = (size_t)(sq.start + qc) * H + hh * D + 16 * s + 8 * hf;
    const u32x4 dv = *reinterpret_cast<const u32x4*>(dout + oo);
    const u32x4 ov = *reinterpret_cast<const u32x4*>(o + oo);
    dof[s] = __builtin_bit_cast(bf16x8, dv);
    delta += dot8_bf16(dv, ov);
  }
  delta = sum_xor32(delta);
  const float lse = lse2[(size_t)sq.row0 + qc];

  f32x16 dq0 = {}, dq1 = {};
  for (int kt = 0; kt < ntiles; ++kt) {
    __syncthreads();
    stage_kvb(Ks, Vs, kbias, base, ld, H, kt, L, mask, b, S, tid);
    __syncthreads();
    f32x16 st[2], dpt[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      st[kb] = f32x16{};
      dpt[kb] = f32x16{};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        bf16x8 ak = *reinterpret_cast<const bf16x8*>(Ks + toff(kb * 32 + r, 16 * s + 8 * hf));
        st[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ak, qf[s], st[kb], 0, 0, 0);
        bf16x8 av = *reinterpret_cast<const bf16x8*>(Vs + toff(kb * 32 + r, 16 * s + 8 * hf));
        dpt[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, dof[s], dpt[kb], 0, 0, 0);
      }
    }
    uint32_t xt = 0;
    if (dp.enabled) xt = dropout_row(drow, dp) ^ drop_col(32u * (uint32_t)kt + 2u * (uint32_t)hf);
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k0 = 32 * kb + 8 * i + 4 * hf;
        const f32x4 kb4 = *reinterpret_cast<const f32x4*>(kbias + k0);  // -inf past the length: p = 0
        const float* rw = relq + kt * 64 + k0;
#pragma unroll
        for (int e = 0; e < 4; e += 2) {
          const int reg = 4 * i + e;
          float kp0 = 1.0f, kp1 = 1.0f;
          if (dp.enabled) {
            const uint32_t bits = drop_fin(xt ^ drop_col((uint32_t)(16 * kb + 4 * (reg >> 2) + ((reg >> 1) & 1))));
            kp0 = keep_factor(bits, 0, dp);
            kp1 = keep_factor(bits, 1, dp);
          }
          const float p0 = exp2f(st[kb][reg] * sl2 + rw[e] + kb4[e] - lse);
          const float p1 = exp2f(st[kb][reg + 1] * sl2 + rw[e + 1] + kb4[e + 1] - lse);
          st[kb][reg] = p0 * (dpt[kb][reg] * kp0 - delta);
          st[kb][reg + 1] = p1 * (dpt[kb][reg + 1] * kp1 - delta);
        }
      }
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8 sb = pack8(st[kb], s);
        dq0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(trA(Ks, kb * 32, s, 0, lane), sb, dq0, 0, 0, 0);
        dq1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(trA(Ks, kb * 32, s, 1, lane), sb, dq1, 0, 0, 0);
      }
  }
  if (q < L) store_row(dqkv + (size_t)(sq.start + q) * ld + hh * D, dq0, dq1, scale * pw, hf);
}

// drel[h][i] = sum over the head's B * nblk partial rows slab[(b * heads + h) * nblk + blk][i], in a fixed order: thread
// (g, c) adds rows g, g + 8, ... of column c ascending, then the 8 group sums are added ascending. Grid (ceil(R / 32),
// heads), 256 threads = 8 row groups x 32 columns.
__global__ __launch_bounds__(256) void attn_relbias_reduce_kernel(const float* __restrict__ slab,
                                                                  float* __restrict__ drel, int B, int nblk, int heads,
                                                                  int R) {
  __shared__ float part[8][32];
  const int g = threadIdx.x >> 5, c = threadIdx.x & 31;
  const int i = blockIdx.x * 32 + c, hh = blockIdx.y;
  float acc = 0.f;
  if (i < R) {
    const int rows = B * nblk;
    for (int row = g; row < rows; row += 8) {
      const int b = row / nblk, blk = row - b * nblk;
      acc += slab[((size_t)(b * heads + hh) * nblk + blk) * R + i];
    }
  }
  part[g][c] = acc;
  __syncthreads();
  if (g == 0 && i < R) {
    float s = part[0][c];
#pragma unroll
    for (int k = 1; k < 8; ++k) s += part[k][c];
    drel[(size_t)hh * R + i] = s;
  }
}

template <bool kPacked>
void launch_fwd(const bf16_t* qkv, const int* cu, const float* mask, const float* rel, bf16_t* out, float* lse2, int T,
                int B, int S, int heads, int R, float sl2, const DropoutParams& dp, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL(attn_relbias_fwd_kernel<kPacked>, grid, dim3(256), 0, st, qkv, cu, mask, rel, out, lse2, T, B, S,
                     heads, R, sl2, dp);
  HSD_CHECK_LAUNCH();
}

template <bool kPacked>
void launch_bwd(const bf16_t* qkv, const int* cu, const float* mask, const float* rel, const bf16_t* o,
                const bf16_t* dout, const float* lse2, bf16_t* dqkv, float* slab, int T, int B, int S, int heads, int R,
                float sl2, float scale, const DropoutParams& dp, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL(attn_relbias_bwd_kv_kernel<kPacked>, grid, dim3(256), 0, st, qkv, cu, mask, rel, o, dout, lse2,
                     dqkv, slab, T, S, heads, R, sl2, scale, dp);
  HSD_CHECK_LAUNCH();
  hipLaunchKernelGGL(attn_relbias_bwd_q_kernel<kPacked>, grid, dim3(256), 0, st, qkv, cu, mask, rel, o, dout, lse2, dqkv,
                     T, B, S, heads, R, sl2, scale, dp);
  HSD_CHECK_LAUNCH();
}

}  // namespace

bool attn_relbias_supported(int head_dim, int S, int R) {
  return head_dim == D && S >= 1 && S <= kMaxLen && R % 2 == 1 && R >= 2 * S - 1;
}

// fp32 words of the drel workspace slab
int64_t attn_relbias_slab_numel(int B, int S, int heads, int R) {
  return (int64_t)B * heads * ((S + 127) / 128) * R;
}

// cu_seqlens != nullptr: packed qkv [T, 3H], B sequences, S = max_seqlen, no mask. cu_seqlens == nullptr: padded qkv
// [B*S, 3H] (T = B*S, S even), mask = optional additive key bias [B, S]. rel: fp32 [heads, R].
void launch_attn_relbias_fwd(const bf16_t* qkv, const int* cu_seqlens, const float* mask, const float* rel, bf16_t* out,
                             float* lse2, int T, int B, int S, int heads, int R, double p, uint64_t seed,
                             hipStream_t st) {
  const DropoutParams dp = make_dropout(p, seed);
  const float sl2 = kLog2e / sqrtf((float)D);
  const dim3 grid((S + 127) / 128, B * heads);
  if (cu_seqlens)
    launch_fwd<true>(qkv, cu_seqlens, nullptr, rel, out, lse2, T, B, S, heads, R, sl2, dp, grid, st);
  else
    launch_fwd<false>(qkv, nullptr, mask, rel, out, lse2, T, B, S, heads, R, sl2, dp, grid, st);
}

// slab: attn_relbias_slab_numel fp32 words of workspace (every word is written); drel: fp32 [heads, R], overwritten
void launch_attn_relbias_bwd(const bf16_t* qkv, const int* cu_seqlens, const float* mask, const float* rel,
                             const bf16_t* o, const bf16_t* dout, const float* lse2, bf16_t* dqkv, float* drel,
                             float* slab, int T, int B, int S, int heads, int R, double p, uint64_t seed,
                             hipStream_t st) {
  const DropoutParams dp = make_dropout(p, seed);
  const float sl2 = kLog2e / sqrtf((float)D);
  const float scale = 1.0f / sqrtf((float)D);
  const dim3 grid((S + 127) / 128, B * heads);
  if (cu_seqlens)
    launch_bwd<true>(qkv, cu_seqlens, nullptr, rel, o, dout, lse2, dqkv, slab, T, B, S, heads, R, sl2, scale, dp, grid,
                     st);
  else
    launch_bwd<false>(qkv, nullptr, mask, rel, o, dout, lse2, dqkv, slab, T, B, S, heads, R, sl2, scale, dp, grid, st);
  hipLaunchKernelGGL(attn_relbias_reduce_kernel, dim3((R + 31) / 32, heads), dim3(256), 0, st, slab, drel, B,
                     (S + 127) / 128, heads, R);
  HSD_CHECK_LAUNCH();
}

}  // namespace hsd
