// Self-attention for head_dim 32 on CDNA4 MFMA (v_mfma_f32_32x32x16_bf16): MiniLM-class encoders (H = 384 / 12 heads,
// H = 256 / 8 heads), padded batches (optional additive key bias) and packed batches (cu_seqlens), bf16 in / out, fp32
// softmax and accumulation.
//
// Work split: ONE WORKGROUP WORKS ON A PAIR OF ADJACENT HEADS. Heads 2j and 2j+1 occupy 64 contiguous bf16 columns
// (128 B) of a qkv row, exactly the footprint of one head of the d = 64 kernels, so K / V / Q / dO tiles are staged by
// the same 16-byte loads into the same XOR-swizzled [rows][64] LDS image (attn_common.h toff), transposed fragments
// come from trA (its colblk argument now selects the HEAD: columns 0..31 are head A = 2j, 32..63 head B = 2j+1) and
// output rows are stored 128 B wide. The math on top of the image is what differs from a d = 64 head, which is why
// this is a file of its own and not a head-dim template parameter of attention_varlen.hip:
//   * Q.K^T of head A contracts k-steps 0-1 of the image (d 0..31), head B k-steps 2-3: two MFMAs per 32x32 score tile
//     per head, two independent score tiles per 32 keys;
//   * two (m, l) softmax states, two dropout rows (head stride apart in the site), two lse2 values per query;
//   * in O^T = V^T.P^T accumulator block 0 takes P_A (V columns 0..31), block 1 takes P_B (columns 32..63);
//   * MFMAs per (query, key, head pair) equal the d = 64 kernels' count per head (8 + 8 per 64-key tile forward); the
//     VALU work (scale, max, exp2, dropout hash) is per score and so doubles.
// Kernels (256 threads = 4 waves; grid (ceil(max_len / 128), B * heads / 2); no atomics, every output element is
// written once by one thread, so results are bit-identical from run to run):
//   forward  128 queries of one (sequence, head pair); a wave = 32 queries on the MFMA lane (swapped S^T = K.Q^T), K/V
//            tiles of 64 keys in LDS, P stays in registers as the next MFMA's B operand; writes out and lse2;
//   dK / dV  128 keys of one (sequence, head pair); a wave = 32 keys on the lane; dK_A, dK_B, dV_A, dV_B accumulate in
//            registers over the sequence's 32-query blocks (Q / dO tiles, lse2 and delta = sum_d dO.O per (head, row)
//            in LDS); P is rebuilt from lse2, the dropout bits are regenerated from the seed;
//   dQ       its own queries-on-lanes pass: the forward's loop with dS in place of P and K in place of V.
// Addressing is the one template switch (kPacked), everything else is shared:
//   padded  qkv [B*S, 3H]: sequence b = rows b*S .. b*S+S-1 (S even), optional fp32 key bias [B, S] scaled by log2(e)
//           and clamped at -1e30 (attention.hip mask_bias2), lse2 [B, heads, S], dropout row (b*heads + h)*S + q;
//   packed  qkv [T, 3H], cu_seqlens int32 [B+1] clamped into [0, T] on the device, lse2 [heads, T], dropout row h*T + t;
//           dead rows (cu[B] .. T-1) of out / lse2 / dqkv are written as zeros by the x = 0 workgroups of the last
//           sequence. Both are column `key` of the site, bit for bit ops/rng.py keep_mask.
// A workgroup whose 128-row block starts at or past its sequence's end exits before its first barrier.
// LDS: forward / dQ 2 x 8 KiB K and V images + 256 B key bias (additive, log2 domain: 0, the clamped mask bias, or
//      -inf for keys past the length -- the only place the length enters the score math); dK/dV 2 x 4 KiB Q and dO
//      images + 512 B lse2 / delta.
// Registers: the source handles one head at a time inside a tile (two score tiles of 16 fp32, not four), but the head
// loop is fully unrolled and the compiler interleaves both heads, so what is compiled is larger than that plan:
// forward 200 VGPRs + 48 AGPRs (2 waves/SIMD), dK/dV 226 + 64 (1 wave/SIMD), dQ 246-248 + 80 (1 wave/SIMD), scratch 0
// in all six instantiations (profiles/attn_d32/resource_usage.txt). The file is built without the packed fp32 VALU
// forms (_build.py FILE_FLAGS); with them the forward takes 221 VGPRs and drops to 1 wave/SIMD.
// Not here (by scope): keep-mask buffer, bias-gradient epilogue, fp8 hand-off, any other head dim, odd head counts.
#include "attn_common.h"

namespace hsd {

using namespace attn;

namespace {

constexpr int kD32 = 32;  // head dim; a pair of heads is one D = 64 column block

__device__ __forceinline__ int clampi32(int v, int lo, int hi) { return min(max(v, lo), hi); }

// one (sequence, head pair): first row, length, and where head A's query 0 sits in lse2 / the dropout site (head B is
// `hstride` rows further on)
struct PairSeq {
  int start, len;
  uint32_t row0, hstride;
};

template <bool kPacked>
__device__ __forceinline__ PairSeq pair_seq(const int* __restrict__ cu, int b, int hA, int heads, int T, int S) {
  if (kPacked) {
    const int s = clampi32(cu[b], 0, T);
    const int e = clampi32(cu[b + 1], s, T);
    return {s, e - s, (uint32_t)hA * (uint32_t)T + (uint32_t)s, (uint32_t)T};
  }
  return {b * S, S, (uint32_t)(b * heads + hA) * (uint32_t)S, (uint32_t)S};
}

// additive score bias of key `key` (log2 domain)
__device__ __forceinline__ float key_bias2(const float* __restrict__ mask, int b, int S, int key, int L) {
  if (key >= L) return -INFINITY;
  if (!mask) return 0.f;
  return fmaxf(mask[(size_t)b * S + key] * kLog2e, -1e30f);
}

// keys kt*64 .. kt*64+63 of the sequence at `base` (row stride ld, the pair's column block applied) into the [64][64]
// K / V images (rows >= L zero) and their score biases into kbias
__device__ __forceinline__ void stage_kv32(bf16_t* Ks, bf16_t* Vs, float* kbias, const bf16_t* __restrict__ base, int ld,
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

// accumulators of head A and head B (row on the lane, d = 8i + 4hf + 0..3 in registers), each times its own scale ->
// the pair's 64 bf16 of one row
__device__ __forceinline__ void store_pair_row(bf16_t* dst, const f32x16& a, const f32x16& b, float sa, float sb,
                                               int hf) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int d = 8 * i + 4 * hf;
    u32x2 w0, w1;
    w0.x = pack_bf2(a[4 * i] * sa, a[4 * i + 1] * sa);
    w0.y = pack_bf2(a[4 * i + 2] * sa, a[4 * i + 3] * sa);
    w1.x = pack_bf2(b[4 * i] * sb, b[4 * i + 1] * sb);
    w1.y = pack_bf2(b[4 * i + 2] * sb, b[4 * i + 3] * sb);
    *reinterpret_cast<u32x2*>(dst + d) = w0;
    *reinterpret_cast<u32x2*>(dst + kD32 + d) = w1;
  }
}

// zero rows t0 .. T-1, columns col0 .. col0+63 of a [T][ld] bf16 matrix (256 threads)
__device__ __forceinline__ void zero_pair_rows(bf16_t* __restrict__ m, int ld, int col0, int t0, int T, int tid) {
  const int n = (T - t0) * 8;
  for (int i = tid; i < n; i += 256) {
    const int row = t0 + (i >> 3), ch = i & 7;
    *reinterpret_cast<u32x4*>(m + (size_t)row * ld + col0 + ch * 8) = u32x4{0, 0, 0, 0};
  }
}

// the four score biases of accumulator registers 4i .. 4i+3 of key block kb (keys 32 kb + 8i + 4hf + 0..3)
__device__ __forceinline__ f32x4 bias4(const float* kbias, int kb, int i, int hf) {
  return *reinterpret_cast<const f32x4*>(kbias + 32 * kb + 8 * i + 4 * hf);
}

// ------------------------------------------------------------------------------------------------
template <bool kPacked>
__global__ __launch_bounds__(256) void attn_d32_fwd_kernel(const bf16_t* __restrict__ qkv, const int* __restrict__ cu,
                                                           const float* __restrict__ mask, bf16_t* __restrict__ out,
                                                           float* __restrict__ lse2, int T, int B, int S, int heads,
                                                           float sl2, DropoutParams dp) {
  dp = resolve_seed(dp);
  __shared__ __attribute__((aligned(16))) bf16_t Ks[64 * D];
  __shared__ __attribute__((aligned(16))) bf16_t Vs[64 * D];
  __shared__ __attribute__((aligned(16))) float kbias[64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hf = lane >> 5;
  const int hp = heads >> 1;
  const int b = blockIdx.y / hp, j = blockIdx.y % hp;
  const int H = heads * kD32, ld = 3 * H, col0 = j * D;
  if (kPacked && blockIdx.x == 0 && b == B - 1) {  // dead rows of this head pair
    const int t0 = clampi32(cu[B], 0, T);
    zero_pair_rows(out, H, col0, t0, T, tid);
    for (int i = tid; i < 2 * (T - t0); i += 256) {
      const int hd = i & 1, t = t0 + (i >> 1);
      lse2[(size_t)(2 * j + hd) * T + t] = 0.f;
    }
  }
  const PairSeq sq = pair_seq<kPacked>(cu, b, 2 * j, heads, T, S);
  const int L = sq.len;
  if ((int)blockIdx.x * 128 >= L) return;
  const int q = blockIdx.x * 128 + wave * 32 + r;
  const int qc = min(q, L - 1);
  const bf16_t* base = qkv + (size_t)sq.start * ld + col0;

  bf16x8 qf[4];  // k-steps 0-1: head A, 2-3: head B
#pragma unroll
  for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(base + (size_t)qc * ld + 16 * s + 8 * hf);

  f32x16 o[2] = {};
  float m[2] = {-INFINITY, -INFINITY}, l[2] = {0.f, 0.f};
  const int ntiles = (L + 63) / 64;
  for (int kt = 0; kt < ntiles; ++kt) {
    __syncthreads();
    stage_kv32(Ks, Vs, kbias, base, ld, H, kt, L, mask, b, S, tid);
    __syncthreads();
#pragma unroll
    for (int hd = 0; hd < 2; ++hd) {
      f32x16 st[2];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        st[kb] = f32x16{};
#pragma unroll
        for (int s = 2 * hd; s < 2 * hd + 2; ++s) {
          bf16x8 a = *reinterpret_cast<const bf16x8*>(Ks + toff(kb * 32 + r, 16 * s + 8 * hf));
          st[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, qf[s], st[kb], 0, 0, 0);
        }
      }
      float mx = -INFINITY;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const f32x4 kb4 = bias4(kbias, kb, i, hf);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float x = st[kb][4 * i + e] * sl2 + kb4[e];
            st[kb][4 * i + e] = x;
            mx = fmaxf(mx, x);
          }
        }
      mx = max_xor32(mx);  // finite: every tile holds at least one key < L, and the mask bias is clamped
      const float mn = fmaxf(m[hd], mx);
      const float alpha = exp2f(m[hd] - mn);  // m = -inf on the first tile -> 0
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
      l[hd] = l[hd] * alpha + ls;
      m[hd] = mn;
      o[hd] *= alpha;
      if (dp.enabled) {
        // column pair key / 2 = 32 kt + 16 kb + 4 (reg >> 2) + (reg >> 1 & 1) + 2 hf (disjoint bits)
        const uint32_t drow = sq.row0 + (uint32_t)hd * sq.hstride + (uint32_t)qc;
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
      // O_hd^T += V_hd^T . P_hd^T: V columns 32 hd .. 32 hd + 31 of the image
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int s = 0; s < 2; ++s)
          o[hd] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(trA(Vs, kb * 32, s, hd, lane), pack8(st[kb], s), o[hd], 0, 0,
                                                          0);
    }
  }
  if (q < L) {
    store_pair_row(out + (size_t)(sq.start + q) * H + col0, o[0], o[1], 1.0f / l[0], 1.0f / l[1], hf);
    // lane r writes head A's value, lane r + 32 head B's
    lse2[(size_t)sq.row0 + (size_t)hf * sq.hstride + q] = hf == 0 ? m[0] + log2f(l[0]) : m[1] + log2f(l[1]);
  }
}

// ------------------------------------------------------------------------------------------------
template <bool kPacked>
__global__ __launch_bounds__(256) void attn_d32_bwd_kv_kernel(const bf16_t* __restrict__ qkv, const int* __restrict__ cu,
                                                              const float* __restrict__ mask,
                                                              const bf16_t* __restrict__ o,
                                                              const bf16_t* __restrict__ dout,
                                                              const float* __restrict__ lse2, bf16_t* __restrict__ dqkv,
                                                              int T, int S, int heads, float sl2, float scale,
                                                              DropoutParams dp) {
  dp = resolve_seed(dp);
  __shared__ __attribute__((aligned(16))) bf16_t Qs[32 * D];
  __shared__ __attribute__((aligned(16))) bf16_t dOs[32 * D];
  __shared__ float lse_s[2][32], del_s[2][32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hf = lane >> 5;
  const int hp = heads >> 1;
  const int b = blockIdx.y / hp, j = blockIdx.y % hp;
  const int H = heads * kD32, ld = 3 * H, col0 = j * D;
  const PairSeq sq = pair_seq<kPacked>(cu, b, 2 * j, heads, T, S);
  const int L = sq.len;
  const int kbase = blockIdx.x * 128;
  if (kbase >= L) return;
  const int key = kbase + wave * 32 + r;
  const int kc = min(key, L - 1);
  const uint32_t ck = drop_col((uint32_t)kc >> 1);  // dropout column word of this lane's key
  const float kb2 = key_bias2(mask, b, S, kc, L);
  const bf16_t* base = qkv + (size_t)sq.start * ld + col0;
  const size_t obase = (size_t)sq.start * H + col0;
  // a padded sequence with every key masked: p below is 1 where 1/S is meant, folded into the output scales (common.h)
  const float pw = kPacked ? 1.0f : all_masked_scale(lse2[sq.row0], S);

  // per-wave K and V B-fragments (key on the lane); k-steps 0-1: head A, 2-3: head B
  bf16x8 kf[4], vf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    kf[s] = *reinterpret_cast<const bf16x8*>(base + (size_t)kc * ld + H + 16 * s + 8 * hf);
    vf[s] = *reinterpret_cast<const bf16x8*>(base + (size_t)kc * ld + 2 * H + 16 * s + 8 * hf);
  }
  const bool kvalid = key < L;
  f32x16 dk[2] = {}, dv[2] = {};
  const int nqb = (L + 31) / 32;
  for (int qb = 0; qb < nqb; ++qb) {
    __syncthreads();
    {
      // Q / dO tiles (32 rows x 8 chunks = 256 chunks: one per thread; chunks 0-3 head A, 4-7 head B), lse2 and
      // delta = rowsum(dO*O) of each (head, row): the sum of a head's four chunks
      const int row = tid >> 3, ch = tid & 7;
      const int qq = qb * 32 + row;
      u32x4 qv = {0, 0, 0, 0}, dv4 = {0, 0, 0, 0}, ov = {0, 0, 0, 0};
      if (qq < L) {
        qv = *reinterpret_cast<const u32x4*>(base + (size_t)qq * ld + ch * 8);
        const size_t oo = obase + (size_t)qq * H + ch * 8;
        dv4 = *reinterpret_cast<const u32x4*>(dout + oo);
        ov = *reinterpret_cast<const u32x4*>(o + oo);
      }
      *reinterpret_cast<u32x4*>(Qs + toff(row, ch * 8)) = qv;
      *reinterpret_cast<u32x4*>(dOs + toff(row, ch * 8)) = dv4;
      float part = dot8_bf16(dv4, ov);
      part += dpp_xor1(part);
      part += dpp_xor2(part);
      if ((ch & 3) == 0) {
        const int hd = ch >> 2;
        del_s[hd][row] = part;
        lse_s[hd][row] = qq < L ? lse2[(size_t)sq.row0 + (size_t)hd * sq.hstride + qq] : 0.f;
      }
    }
    __syncthreads();
#pragma unroll
    for (int hd = 0; hd < 2; ++hd) {
      f32x16 sacc = {}, dpacc = {};
#pragma unroll
      for (int s = 2 * hd; s < 2 * hd + 2; ++s) {
        bf16x8 aq = *reinterpret_cast<const bf16x8*>(Qs + toff(r, 16 * s + 8 * hf));
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aq, kf[s], sacc, 0, 0, 0);
        bf16x8 ad = *reinterpret_cast<const bf16x8*>(dOs + toff(r, 16 * s + 8 * hf));
        dpacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ad, vf[s], dpacc, 0, 0, 0);
      }
      // sacc / dpacc: col = key (lane), row qi = (reg&3) + 8*(reg>>2) + 4*hf
      const uint32_t drow0 = sq.row0 + (uint32_t)hd * sq.hstride;
      f32x16 pd, ds;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int qi = (reg & 3) + 8 * (reg >> 2) + 4 * hf;
        const int qq = qb * 32 + qi;
        const float p = (kvalid && qq < L) ? exp2f(sacc[reg] * sl2 + kb2 - lse_s[hd][qi]) : 0.f;
        float kf_ = 1.0f;
        if (dp.enabled) {
          kf_ = keep_factor(drop_fin(dropout_row(drow0 + (uint32_t)min(qq, L - 1), dp) ^ ck), kc & 1, dp);
        }
        pd[reg] = p * kf_;
        ds[reg] = p * (dpacc[reg] * kf_ - del_s[hd][qi]);
      }
      // dV_hd^T += dO_hd^T . Pd ; dK_hd^T += Q_hd^T . dS   (B operands straight from the accumulators)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        dv[hd] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(trA(dOs, 0, s, hd, lane), pack8(pd, s), dv[hd], 0, 0, 0);
        dk[hd] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(trA(Qs, 0, s, hd, lane), pack8(ds, s), dk[hd], 0, 0, 0);
      }
    }
  }
  if (kvalid) {
    bf16_t* row = dqkv + (size_t)(sq.start + key) * ld + col0;
    store_pair_row(row + H, dk[0], dk[1], scale * pw, scale * pw, hf);
    store_pair_row(row + 2 * H, dv[0], dv[1], pw, pw, hf);
  }
}

// dQ: queries on the lanes, as the forward; per head S^T = K.Q^T and dP^T = V.dO^T per 64-key tile, dS^T stays in
// registers as the B operand of dQ^T += K^T . dS^T.
template <bool kPacked>
__global__ __launch_bounds__(256) void attn_d32_bwd_q_kernel(const bf16_t* __restrict__ qkv, const int* __restrict__ cu,
                                                             const float* __restrict__ mask,
                                                             const bf16_t* __restrict__ o,
                                                             const bf16_t* __restrict__ dout,
                                                             const float* __restrict__ lse2, bf16_t* __restrict__ dqkv,
                                                             int T, int B, int S, int heads, float sl2, float scale,
                                                             DropoutParams dp) {
  dp = resolve_seed(dp);
  __shared__ __attribute__((aligned(16))) bf16_t Ks[64 * D];
  __shared__ __attribute__((aligned(16))) bf16_t Vs[64 * D];
  __shared__ __attribute__((aligned(16))) float kbias[64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hf = lane >> 5;
  const int hp = heads >> 1;
  const int b = blockIdx.y / hp, j = blockIdx.y % hp;
  const int H = heads * kD32, ld = 3 * H, col0 = j * D;
  if (kPacked && blockIdx.x == 0 && b == B - 1) {  // dead rows: the q, k and v columns of this head pair
    const int t0 = clampi32(cu[B], 0, T);
#pragma unroll
    for (int part = 0; part < 3; ++part) zero_pair_rows(dqkv, ld, part * H + col0, t0, T, tid);
  }
  const PairSeq sq = pair_seq<kPacked>(cu, b, 2 * j, heads, T, S);
  const int L = sq.len;
  if ((int)blockIdx.x * 128 >= L) return;
  const int q = blockIdx.x * 128 + wave * 32 + r;
  const int qc = min(q, L - 1);
  const bf16_t* base = qkv + (size_t)sq.start * ld + col0;
  const float pw = kPacked ? 1.0f : all_masked_scale(lse2[sq.row0], S);

  bf16x8 qf[4], dof[4];
  float delta[2] = {0.f, 0.f};  // rowsum(dO * O) of each head: this lane holds half of the row, lane ^ 32 the other half
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    qf[s] = *reinterpret_cast<const bf16x8*>(base + (size_t)qc * ld + 16 * s + 8 * hf);
    const size_t oo = (size_t)(sq.start + qc) * H + col0 + 16 * s + 8 * hf;
    const u32x4 dv4 = *reinterpret_cast<const u32x4*>(dout + oo);
    const u32x4 ov = *reinterpret_cast<const u32x4*>(o + oo);
    dof[s] = __builtin_bit_cast(bf16x8, dv4);
    delta[s >> 1] += dot8_bf16(dv4, ov);
  }
  float lse[2];
#pragma unroll
  for (int hd = 0; hd < 2; ++hd) {
    delta[hd] = sum_xor32(delta[hd]);
    lse[hd] = lse2[(size_t)sq.row0 + (size_t)hd * sq.hstride + qc];
  }

  f32x16 dq[2] = {};
  const int ntiles = (L + 63) / 64;
  for (int kt = 0; kt < ntiles; ++kt) {
    __syncthreads();
    stage_kv32(Ks, Vs, kbias, base, ld, H, kt, L, mask, b, S, tid);
    __syncthreads();
#pragma unroll
    for (int hd = 0; hd < 2; ++hd) {
      f32x16 st[2], dpt[2];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        st[kb] = f32x16{};
        dpt[kb] = f32x16{};
#pragma unroll
        for (int s = 2 * hd; s < 2 * hd + 2; ++s) {
          bf16x8 ak = *reinterpret_cast<const bf16x8*>(Ks + toff(kb * 32 + r, 16 * s + 8 * hf));
          st[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ak, qf[s], st[kb], 0, 0, 0);
          bf16x8 av = *reinterpret_cast<const bf16x8*>(Vs + toff(kb * 32 + r, 16 * s + 8 * hf));
          dpt[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, dof[s], dpt[kb], 0, 0, 0);
        }
      }
      uint32_t xt = 0;
      if (dp.enabled) {
        const uint32_t drow = sq.row0 + (uint32_t)hd * sq.hstride + (uint32_t)qc;
        xt = dropout_row(drow, dp) ^ drop_col(32u * (uint32_t)kt + 2u * (uint32_t)hf);
      }
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const f32x4 kb4 = bias4(kbias, kb, i, hf);  // -inf past the length: p = 0
#pragma unroll
          for (int e = 0; e < 4; e += 2) {
            const int reg = 4 * i + e;
            float k0 = 1.0f, k1 = 1.0f;
            if (dp.enabled) {
              const uint32_t bits = drop_fin(xt ^ drop_col((uint32_t)(16 * kb + 4 * (reg >> 2) + ((reg >> 1) & 1))));
              k0 = keep_factor(bits, 0, dp);
              k1 = keep_factor(bits, 1, dp);
            }
            const float p0 = exp2f(st[kb][reg] * sl2 + kb4[e] - lse[hd]);
            const float p1 = exp2f(st[kb][reg + 1] * sl2 + kb4[e + 1] - lse[hd]);
            st[kb][reg] = p0 * (dpt[kb][reg] * k0 - delta[hd]);
            st[kb][reg + 1] = p1 * (dpt[kb][reg + 1] * k1 - delta[hd]);
          }
        }
      // dQ_hd^T += K_hd^T . dS_hd^T: K columns 32 hd .. 32 hd + 31 of the image
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int s = 0; s < 2; ++s)
          dq[hd] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(trA(Ks, kb * 32, s, hd, lane), pack8(st[kb], s), dq[hd], 0,
                                                           0, 0);
    }
  }
  if (q < L) store_pair_row(dqkv + (size_t)(sq.start + q) * ld + col0, dq[0], dq[1], scale * pw, scale * pw, hf);
}

template <bool kPacked>
void launch_fwd(const bf16_t* qkv, const int* cu, const float* mask, bf16_t* out, float* lse2, int T, int B, int S,
                int heads, float sl2, const DropoutParams& dp, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL(attn_d32_fwd_kernel<kPacked>, grid, dim3(256), 0, st, qkv, cu, mask, out, lse2, T, B, S, heads,
                     sl2, dp);
  HSD_CHECK_LAUNCH();
}

template <bool kPacked>
void launch_bwd(const bf16_t* qkv, const int* cu, const float* mask, const bf16_t* o, const bf16_t* dout,
                const float* lse2, bf16_t* dqkv, int T, int B, int S, int heads, float sl2, float scale,
                const DropoutParams& dp, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL(attn_d32_bwd_kv_kernel<kPacked>, grid, dim3(256), 0, st, qkv, cu, mask, o, dout, lse2, dqkv, T, S,
                     heads, sl2, scale, dp);
  HSD_CHECK_LAUNCH();
  hipLaunchKernelGGL(attn_d32_bwd_q_kernel<kPacked>, grid, dim3(256), 0, st, qkv, cu, mask, o, dout, lse2, dqkv, T, B,
                     S, heads, sl2, scale, dp);
  HSD_CHECK_LAUNCH();
}

}  // namespace

bool attn_d32_supported(int heads, int head_dim, int S) {
  return head_dim == kD32 && heads >= 2 && heads % 2 == 0 && S >= 2 && S % 2 == 0;
}

// cu_seqlens != nullptr: packed qkv [T, 3H], B sequences, S = max_seqlen, no mask. cu_seqlens == nullptr: padded qkv
// [B*S, 3H] (T = B*S), mask = optional additive key bias [B, S].
void launch_attn_d32_fwd(const bf16_t* qkv, const int* cu_seqlens, const float* mask, bf16_t* out, float* lse2, int T,
                         int B, int S, int heads, double p, uint64_t seed, hipStream_t st) {
  const DropoutParams dp = make_dropout(p, seed);
  const float sl2 = kLog2e / sqrtf((float)kD32);
  const dim3 grid((S + 127) / 128, B * (heads / 2));
  if (cu_seqlens)
    launch_fwd<true>(qkv, cu_seqlens, nullptr, out, lse2, T, B, S, heads, sl2, dp, grid, st);
  else
    launch_fwd<false>(qkv, nullptr, mask, out, lse2, T, B, S, heads, sl2, dp, grid, st);
}

void launch_attn_d32_bwd(const bf16_t* qkv, const int* cu_seqlens, const float* mask, const bf16_t* o,
                         const bf16_t* dout, const float* lse2, bf16_t* dqkv, int T, int B, int S, int heads, double p,
                         uint64_t seed, hipStream_t st) {
  const DropoutParams dp = make_dropout(p, seed);
  const float sl2 = kLog2e / sqrtf((float)kD32);
  const float scale = 1.0f / sqrtf((float)kD32);
  const dim3 grid((S + 127) / 128, B * (heads / 2));
  if (cu_seqlens)
    launch_bwd<true>(qkv, cu_seqlens, nullptr, o, dout, lse2, dqkv, T, B, S, heads, sl2, scale, dp, grid, st);
  else
    launch_bwd<false>(qkv, nullptr, mask, o, dout, lse2, dqkv, T, B, S, heads, sl2, scale, dp, grid, st);
}

}  // namespace hsd
