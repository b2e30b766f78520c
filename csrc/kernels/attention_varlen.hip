// Variable-length (padding-free) self-attention for head_dim 64 on CDNA4 MFMA (v_mfma_f32_32x32x16_bf16).
//
// Input  qkv [T, 3H]: B sequences packed back to back, sequence b in rows cu[b] .. cu[b+1]-1 (cu = cu_seqlens,
// device int32 [B+1], cu[0] = 0); rows cu[B] .. T-1 are dead (they belong to no sequence: data/packing.py rounds T
// up). No mask tensor: a key is visible iff it lies in the query's own sequence. Dropout on the probabilities:
// element (head h, packed query row t, key j within the sequence) is row h*T + t, column j of the site (ops/rng.py);
// the backward regenerates the bits. lse2 is [heads, T].
//
// The kernels are the tiled generic ones of attention.hip walked by offsets instead of b*S:
//   forward   one workgroup = 128 queries of one (sequence, head), a wave = 32 queries on the MFMA lane, K/V tiles of
//             64 keys in LDS, keys >= L_b of the last tile masked to -inf;
//   dK / dV   one workgroup = 128 keys of one (sequence, head), a wave = 32 keys on the lane, dK^T / dV^T accumulated in
//             registers over the sequence's query blocks;
//   dQ        its own queries-on-lanes pass (the forward's loop with dS in place of P and K in place of V), so every
//             dqkv element is written once by one thread: no fp32 atomics, bit-identical from run to run.
// Work decomposition: a (ceil(max_seqlen / 128), B * heads) grid; a workgroup whose 128-row block starts at or past
// L_b exits before its first barrier. Row indices are clamped into [0, T] on the device, so no load or store touches
// a row >= T whatever cu holds. Dead rows of out / lse2 / dqkv are written as zeros by the x = 0 workgroups of the
// last sequence (one per head).
#include "attn_common.h"

namespace hsd {

using namespace attn;

void launch_colsum(const bf16_t* x, float* dbias, int rows, int N, hipStream_t st);

namespace {

struct Span {
  int start, len;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ Span seq_span(const int* __restrict__ cu, int b, int T) {
  const int s = clampi(cu[b], 0, T);
  const int e = clampi(cu[b + 1], s, T);
  return {s, e - s};
}

// stage keys kt*64 .. kt*64+63 of the sequence at `base` (row stride ld, head column block already applied) into the
// [64][64] K / V images; rows >= L are zero
__device__ __forceinline__ void stage_kv(bf16_t* Ks, bf16_t* Vs, const bf16_t* __restrict__ base, int ld, int H, int kt,
                                         int L, int tid) {
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
}

// acc pair (query on the lane, d = 32*blk + 8i + 4hf + 0..3 in registers) * scale -> 64 bf16 of one row
__device__ __forceinline__ void store_row64(bf16_t* dst, const f32x16& a0, const f32x16& a1, float scale, int hf) {
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
__device__ __forceinline__ void zero_rows64(bf16_t* __restrict__ m, int ld, int col0, int t0, int T, int tid) {
  const int n = (T - t0) * 8;
  for (int i = tid; i < n; i += 256) {
    const int row = t0 + (i >> 3), ch = i & 7;
    *reinterpret_cast<u32x4*>(m + (size_t)row * ld + col0 + ch * 8) = u32x4{0, 0, 0, 0};
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attn_varlen_fwd_kernel(const bf16_t* __restrict__ qkv, const int* __restrict__ cu,
                                                              bf16_t* __restrict__ out, float* __restrict__ lse2, int T,
                                                              int B, int heads, float sl2, DropoutParams dp) {
  dp = resolve_seed(dp);
  __shared__ __attribute__((aligned(16))) bf16_t Ks[64 * D];
  __shared__ __attribute__((aligned(16))) bf16_t Vs[64 * D];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hf = lane >> 5;
  const int b = blockIdx.y / heads, hh = blockIdx.y % heads;
  const int H = heads * D, ld = 3 * H;
  if (blockIdx.x == 0 && b == B - 1) {  // dead rows of this head
    const int t0 = clampi(cu[B], 0, T);
    zero_rows64(out, H, hh * D, t0, T, tid);
    for (int t = t0 + tid; t < T; t += 256) lse2[(size_t)hh * T + t] = 0.f;
  }
  const Span sp = seq_span(cu, b, T);
  const int L = sp.len;
  if ((int)blockIdx.x * 128 >= L) return;
  const int q = blockIdx.x * 128 + wave * 32 + r;
  const int qc = min(q, L - 1);
  const bf16_t* base = qkv + (size_t)sp.start * ld + hh * D;
  const uint32_t drow = (uint32_t)hh * (uint32_t)T + (uint32_t)(sp.start + qc);

  bf16x8 qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(base + (size_t)qc * ld + 16 * s + 8 * hf);

  f32x16 o0 = {}, o1 = {};
  float m = -INFINITY, l = 0.f;
  const int ntiles = (L + 63) / 64;
  for (int kt = 0; kt < ntiles; ++kt) {
    __syncthreads();
    stage_kv(Ks, Vs, base, ld, H, kt, L, tid);
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
      for (int reg = 0; reg < 16; ++reg) {
        const int key = kt * 64 + kb * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * hf;
        float x = key < L ? st[kb][reg] * sl2 : -INFINITY;
        st[kb][reg] = x;
        mx = fmaxf(mx, x);
      }
    mx = max_xor32(mx);  // finite: every tile holds at least one key < L
    const float mn = fmaxf(m, mx);
    const float alpha = exp2f(m - mn);  // m = -inf on the first tile -> 0
    float ls = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        float p = exp2f(st[kb][reg] - mn);
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
    store_row64(out + (size_t)(sp.start + q) * H + hh * D, o0, o1, 1.0f / l, hf);
    if (hf == 0) lse2[(size_t)hh * T + sp.start + q] = m + log2f(l);
  }
}

// ------------------------------------------------------------------------------------------------
// dK / dV: the key-block kernel of attention.hip without its dQ part.
__global__ __launch_bounds__(256) void attn_varlen_bwd_kv_kernel(const bf16_t* __restrict__ qkv,
                                                                 const int* __restrict__ cu,
                                                                 const bf16_t* __restrict__ o,
                                                                 const bf16_t* __restrict__ dout,
                                                                 const float* __restrict__ lse2,
                                                                 bf16_t* __restrict__ dqkv, int T, int heads, float sl2,
                                                                 float scale, DropoutParams dp) {
  dp = resolve_seed(dp);
  __shared__ __attribute__((aligned(16))) bf16_t Qs[32 * D];
  __shared__ __attribute__((aligned(16))) bf16_t dOs[32 * D];
  __shared__ float lse_s[32], del_s[32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hf = lane >> 5;
  const int b = blockIdx.y / heads, hh = blockIdx.y % heads;
  const int H = heads * D, ld = 3 * H;
  const Span sp = seq_span(cu, b, T);
  const int L = sp.len;
  const int kbase = blockIdx.x * 128;
  if (kbase >= L) return;
  const int key = kbase + wave * 32 + r;
  const int kc = min(key, L - 1);
  const uint32_t ck = drop_col((uint32_t)kc >> 1);  // dropout column word of this lane's key
  const bf16_t* base = qkv + (size_t)sp.start * ld + hh * D;
  const size_t obase = (size_t)sp.start * H + hh * D;
  const uint32_t drow0 = (uint32_t)hh * (uint32_t)T + (uint32_t)sp.start;

  // per-wave K and V B-fragments (key on the lane)
  bf16x8 kf[4], vf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    kf[s] = *reinterpret_cast<const bf16x8*>(base + (size_t)kc * ld + H + 16 * s + 8 * hf);
    vf[s] = *reinterpret_cast<const bf16x8*>(base + (size_t)kc * ld + 2 * H + 16 * s + 8 * hf);
  }
  const bool kvalid = key < L;
  f32x16 dk0 = {}, dk1 = {}, dv0 = {}, dv1 = {};
  const int nqb = (L + 31) / 32;
  for (int qb = 0; qb < nqb; ++qb) {
    __syncthreads();
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
      float part = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) part += lo_bf(dv[k]) * lo_bf(ov[k]) + hi_bf(dv[k]) * hi_bf(ov[k]);
      part = sum8_dpp(part);
      if (ch == 0) {
        del_s[row] = part;
        lse_s[row] = qq < L ? lse2[(size_t)hh * T + sp.start + qq] : 0.f;
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
    // sacc/dpacc: col = key (lane), row qi = (reg&3) + 8*(reg>>2) + 4*hf
    f32x16 pd, ds;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int qi = (reg & 3) + 8 * (reg >> 2) + 4 * hf;
      const int qq = qb * 32 + qi;
      float p = (kvalid && qq < L) ? exp2f(sacc[reg] * sl2 - lse_s[qi]) : 0.f;
      float kf_ = 1.0f;
      if (dp.enabled) {
        kf_ = keep_factor(drop_fin(dropout_row(drow0 + (uint32_t)min(qq, L - 1), dp) ^ ck), kc & 1, dp);
      }
      pd[reg] = p * kf_;
      ds[reg] = p * (dpacc[reg] * kf_ - del_s[qi]);
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
  }
  if (kvalid) {
    bf16_t* row = dqkv + (size_t)(sp.start + key) * ld + hh * D;
    store_row64(row + H, dk0, dk1, scale, hf);
    store_row64(row + 2 * H, dv0, dv1, 1.0f, hf);
  }
}

// dQ: queries on the lanes, as the forward; S^T = K.Q^T and dP^T = V.dO^T per 64-key tile, dS^T stays in registers as
// the B operand of dQ^T += K^T . dS^T.
__global__ __launch_bounds__(256) void attn_varlen_bwd_q_kernel(const bf16_t* __restrict__ qkv,
                                                                const int* __restrict__ cu,
                                                                const bf16_t* __restrict__ o,
                                                                const bf16_t* __restrict__ dout,
                                                                const float* __restrict__ lse2,
                                                                bf16_t* __restrict__ dqkv, int T, int B, int heads,
                                                                float sl2, float scale, DropoutParams dp) {
  dp = resolve_seed(dp);
  __shared__ __attribute__((aligned(16))) bf16_t Ks[64 * D];
  __shared__ __attribute__((aligned(16))) bf16_t Vs[64 * D];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hf = lane >> 5;
  const int b = blockIdx.y / heads, hh = blockIdx.y % heads;
  const int H = heads * D, ld = 3 * H;
  if (blockIdx.x == 0 && b == B - 1) {  // dead rows: the q, k and v columns of this head
    const int t0 = clampi(cu[B], 0, T);
#pragma unroll
    for (int part = 0; part < 3; ++part) zero_rows64(dqkv, ld, part * H + hh * D, t0, T, tid);
  }
  const Span sp = seq_span(cu, b, T);
  const int L = sp.len;
  if ((int)blockIdx.x * 128 >= L) return;
  const int q = blockIdx.x * 128 + wave * 32 + r;
  const int qc = min(q, L - 1);
  const bf16_t* base = qkv + (size_t)sp.start * ld + hh * D;
  const uint32_t drow = (uint32_t)hh * (uint32_t)T + (uint32_t)(sp.start + qc);

  bf16x8 qf[4], dof[4];
  float delta = 0.f;  // rowsum(dO * O): this lane holds half of the row, lane ^ 32 the other half
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    qf[s] = *reinterpret_cast<const bf16x8*>(base + (size_t)qc * ld + 16 * s + 8 * hf);
    const size_t oo = (size_t)(sp.start + qc) * H + hh * D + 16 * s + 8 * hf;
    const u32x4 dv = *reinterpret_cast<const u32x4*>(dout + oo);
    const u32x4 ov = *reinterpret_cast<const u32x4*>(o + oo);
    dof[s] = __builtin_bit_cast(bf16x8, dv);
#pragma unroll
    for (int k = 0; k < 4; ++k) delta += lo_bf(dv[k]) * lo_bf(ov[k]) + hi_bf(dv[k]) * hi_bf(ov[k]);
  }
  delta = sum_xor32(delta);
  const float lse = lse2[(size_t)hh * T + sp.start + qc];

  f32x16 dq0 = {}, dq1 = {};
  const int ntiles = (L + 63) / 64;
  for (int kt = 0; kt < ntiles; ++kt) {
    __syncthreads();
    stage_kv(Ks, Vs, base, ld, H, kt, L, tid);
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
      for (int reg = 0; reg < 16; reg += 2) {
        float k0 = 1.0f, k1 = 1.0f;
        if (dp.enabled) {
          const uint32_t bits = drop_fin(xt ^ drop_col((uint32_t)(16 * kb + 4 * (reg >> 2) + ((reg >> 1) & 1))));
          k0 = keep_factor(bits, 0, dp);
          k1 = keep_factor(bits, 1, dp);
        }
        const int key = kt * 64 + kb * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * hf;  // even; reg + 1 is key + 1
        const float p0 = key < L ? exp2f(st[kb][reg] * sl2 - lse) : 0.f;
        const float p1 = key + 1 < L ? exp2f(st[kb][reg + 1] * sl2 - lse) : 0.f;
        st[kb][reg] = p0 * (dpt[kb][reg] * k0 - delta);
        st[kb][reg + 1] = p1 * (dpt[kb][reg + 1] * k1 - delta);
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
  if (q < L) store_row64(dqkv + (size_t)(sp.start + q) * ld + hh * D, dq0, dq1, scale, hf);
}

// ------------------------------------------------------------------------------------------------
void launch_attn_varlen_fwd(const bf16_t* qkv, const int* cu_seqlens, bf16_t* out, float* lse2, int T, int B,
                            int max_seqlen, int heads, double p, uint64_t seed, hipStream_t st) {
  DropoutParams dp = make_dropout(p, seed);
  const float sl2 = kLog2e / sqrtf((float)D);
  dim3 grid((max_seqlen + 127) / 128, B * heads);
  hipLaunchKernelGGL(attn_varlen_fwd_kernel, grid, dim3(256), 0, st, qkv, cu_seqlens, out, lse2, T, B, heads, sl2, dp);
  HSD_CHECK_LAUNCH();
}

void launch_attn_varlen_bwd(const bf16_t* qkv, const int* cu_seqlens, const bf16_t* o, const bf16_t* dout,
                            const float* lse2, bf16_t* dqkv, float* dbias, int T, int B, int max_seqlen, int heads,
                            double p, uint64_t seed, hipStream_t st) {
  DropoutParams dp = make_dropout(p, seed);
  const float sl2 = kLog2e / sqrtf((float)D);
  const float scale = 1.0f / sqrtf((float)D);
  dim3 grid((max_seqlen + 127) / 128, B * heads);
  hipLaunchKernelGGL(attn_varlen_bwd_kv_kernel, grid, dim3(256), 0, st, qkv, cu_seqlens, o, dout, lse2, dqkv, T, heads,
                     sl2, scale, dp);
  HSD_CHECK_LAUNCH();
  hipLaunchKernelGGL(attn_varlen_bwd_q_kernel, grid, dim3(256), 0, st, qkv, cu_seqlens, o, dout, lse2, dqkv, T, B, heads,
                     sl2, scale, dp);
  HSD_CHECK_LAUNCH();
  if (dbias) launch_colsum(dqkv, dbias, T, 3 * heads * D, st);
}

}  // namespace hsd
