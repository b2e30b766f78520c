// Self-attention of ONE query row (position 0, the [CLS] / <s> token) per (batch, head), head_dim 64: the last encoder
// layer of a sequence-classification model feeds only its first-token rows to the head (ops/hip.py _AttnBlockCls), so
// everything downstream of the attention scores is one row per sequence. K and V are still needed at every position.
//
// Both kernels are memory-bound row passes, one 256-thread workgroup per (batch, head): thread (kr, c) = (tid >> 3,
// tid & 7) owns the 16-B chunk c of the head's 64 columns of keys kr, kr + 32, ...; a key row is one 128-B segment
// read (or written) by 8 adjacent lanes. A dot product over the head is 8 in-lane FMAs and a DPP sum over the 8-lane
// group; sums over keys go through the stride-8 lane reduction and one LDS exchange between the 4 waves. The first
// 128 keys' K / V chunks are loaded up front and stay in registers (the whole problem at the headline's S = 128), so
// K and V are read from HBM once; later keys are re-read for the second pass (L2).
//   forward : reads q0, K, V, the mask row               -> ctx0 [B, H], lse2 [B * heads]
//   backward: reads q0, K, V, dctx0, lse2, the mask row  -> dqkv [B * S, 3H]: dK, dV of every key, dQ of row 0, exact
//             zeros in every other dQ row (the QKV weight gradient and dgrad read the whole buffer), and the fp32
//             column sums of dqkv (the QKV bias gradient) by atomicAdd, as attention128.hip does.
// No inter-workgroup synchronisation. Conventions are attention.hip's: scores in the log2 domain, the additive key
// bias clamped at -1e30, lse2 saved for the backward, all_masked_scale (common.h) for a sequence with every key
// masked, and dropout element (b, head, query 0, key j) = row (b * heads + head) * S, column j of the site -- the bits
// the full kernels draw for that row (attention128.hip), re-hashed in the backward.
#include "common.h"

namespace hsd {
namespace acls {

constexpr int D = 64;
constexpr int kPre = 4;  // key passes (32 keys each) whose K / V chunks stay in registers
constexpr float kLog2e = 1.4426950408889634f;

__device__ __forceinline__ u32x4 ld16(const bf16_t* p) { return *reinterpret_cast<const u32x4*>(p); }

__device__ __forceinline__ bool keep_key(uint32_t rw, int j, uint32_t thr) {
  const uint32_t bits = drop_fin(rw ^ drop_col((uint32_t)j >> 1));
  return (j & 1) ? keep_hi(bits, thr) : keep_lo(bits, thr);
}

// acc[0..7] += w * (the 8 bf16 of v)
__device__ __forceinline__ void axpy8(float* acc, float w, const u32x4& v) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    acc[2 * k] = fmaf(w, lo_bf(v[k]), acc[2 * k]);
    acc[2 * k + 1] = fmaf(w, hi_bf(v[k]), acc[2 * k + 1]);
  }
}

// w * (the 8 bf16 of v), rounded to bf16; sum[0..7] += the rounded values
__device__ __forceinline__ u32x4 scale8(float w, const u32x4& v, float* sum) {
  u32x4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    o[k] = pack_bf2(w * lo_bf(v[k]), w * hi_bf(v[k]));
    sum[2 * k] += lo_bf(o[k]);
    sum[2 * k + 1] += hi_bf(o[k]);
  }
  return o;
}

__global__ __launch_bounds__(256) void attn_cls_fwd_kernel(const bf16_t* __restrict__ qkv,
                                                           const float* __restrict__ mask, bf16_t* __restrict__ out,
                                                           float* __restrict__ lse2, int S, int heads, float sl2,
                                                           DropoutParams dp) {
  dp = resolve_seed(dp);
  extern __shared__ float sc[];  // [S] scores, then the kept probabilities
  __shared__ float red[8];
  __shared__ float osum[4][D];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = tid & 7, kr = tid >> 3;
  const int bh = blockIdx.x, b = bh / heads, hh = bh % heads;
  const int H = heads * D;
  const int64_t ld = 3 * (int64_t)H;
  const bf16_t* base = qkv + (int64_t)b * S * ld + hh * D + c * 8;
  const u32x4 qv = ld16(base);
  u32x4 kpre[kPre], vpre[kPre];
#pragma unroll
  for (int i = 0; i < kPre; ++i) {
    const int j = kr + 32 * i;
    kpre[i] = vpre[i] = u32x4{0, 0, 0, 0};
    if (j < S) {
      kpre[i] = ld16(base + j * ld + H);
      vpre[i] = ld16(base + j * ld + 2 * H);
    }
  }
  float mx = -INFINITY;
  auto score = [&](int j, const u32x4& kv) {
    const float d = sum8_dpp(dot8_bf16(qv, kv));
    const float mb = mask ? fmaxf(mask[(int64_t)b * S + j] * kLog2e, -1e30f) : 0.f;
    const float x = fmaf(d, sl2, mb);
    if (c == 0) sc[j] = x;
    mx = fmaxf(mx, x);
  };
#pragma unroll
  for (int i = 0; i < kPre; ++i)
    if (kr + 32 * i < S) score(kr + 32 * i, kpre[i]);
  for (int j = kr + 32 * kPre; j < S; j += 32) score(j, ld16(base + j * ld + H));
  mx = wave_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  // exact softmax over the S keys; P is kept or zeroed (the 1/(1-p) scale rides on the output normalisation)
  const uint32_t rw = dp.enabled ? dropout_row((uint32_t)(bh * S), dp) : 0u;
  float l = 0.f;
  for (int j = tid; j < S; j += 256) {
    const float p = __builtin_amdgcn_exp2f(sc[j] - mx);
    l += p;
    sc[j] = (!dp.enabled || keep_key(rw, j, dp.thr)) ? p : 0.f;
  }
  l = wave_sum(l);
  if (lane == 0) red[4 + wave] = l;
  __syncthreads();
  l = (red[4] + red[5]) + (red[6] + red[7]);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < kPre; ++i)
    if (kr + 32 * i < S) axpy8(acc, sc[kr + 32 * i], vpre[i]);
  for (int j = kr + 32 * kPre; j < S; j += 32) axpy8(acc, sc[j], ld16(base + j * ld + 2 * H));
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = sum_stride8(acc[k]);
  if (lane < 8) {
#pragma unroll
    for (int k = 0; k < 8; ++k) osum[wave][lane * 8 + k] = acc[k];
  }
  __syncthreads();
  if (tid < 8) {
    const float os = (dp.enabled ? dp.scale : 1.0f) / l;
    u32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int d0 = tid * 8 + 2 * k;
      o[k] = pack_bf2(((osum[0][d0] + osum[1][d0]) + (osum[2][d0] + osum[3][d0])) * os,
                      ((osum[0][d0 + 1] + osum[1][d0 + 1]) + (osum[2][d0 + 1] + osum[3][d0 + 1])) * os);
    }
    *reinterpret_cast<u32x4*>(out + (int64_t)b * H + hh * D + tid * 8) = o;
  }
  if (tid == 0) lse2[bh] = mx + __log2f(l);
}

__global__ __launch_bounds__(256) void attn_cls_bwd_kernel(const bf16_t* __restrict__ qkv,
                                                           const float* __restrict__ mask,
                                                           const bf16_t* __restrict__ dctx,
                                                           const float* __restrict__ lse2, bf16_t* __restrict__ dqkv,
                                                           float* __restrict__ dbias, int S, int heads, float sl2,
                                                           float scale, DropoutParams dp) {
  dp = resolve_seed(dp);
  extern __shared__ float sm[];  // [3][S]: P, dP (dropout applied), the kept-and-scaled P
  float* ps = sm;
  float* dps = sm + S;
  float* pds = sm + 2 * S;
  __shared__ float red[4];
  __shared__ float csum[3][4][D];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = tid & 7, kr = tid >> 3;
  const int bh = blockIdx.x, b = bh / heads, hh = bh % heads;
  const int H = heads * D;
  const int64_t ld = 3 * (int64_t)H;
  const int64_t off = (int64_t)b * S * ld + hh * D + c * 8;
  const bf16_t* base = qkv + off;
  bf16_t* dbase = dqkv + off;
  const u32x4 qv = ld16(base);
  const u32x4 dov = ld16(dctx + (int64_t)b * H + hh * D + c * 8);
  const float L = lse2[bh];
  u32x4 kpre[kPre], vpre[kPre];
#pragma unroll
  for (int i = 0; i < kPre; ++i) {
    const int j = kr + 32 * i;
    kpre[i] = vpre[i] = u32x4{0, 0, 0, 0};
    if (j < S) {
      kpre[i] = ld16(base + j * ld + H);
      vpre[i] = ld16(base + j * ld + 2 * H);
    }
  }
  const float ams = all_masked_scale(L, S);
  const float dsc = dp.enabled ? dp.scale : 1.0f;
  const uint32_t rw = dp.enabled ? dropout_row((uint32_t)(bh * S), dp) : 0u;
  // pass 1: P_j from the saved lse2, dP_j = dO . V_j through the dropout mask, delta = sum_j P_j dP_j
  float dl = 0.f;
  auto probs = [&](int j, const u32x4& kv, const u32x4& vv) {
    const float s = sum8_dpp(dot8_bf16(qv, kv));
    const float dpd = sum8_dpp(dot8_bf16(dov, vv));
    const float mb = mask ? fmaxf(mask[(int64_t)b * S + j] * kLog2e, -1e30f) : 0.f;
    const float p = __builtin_amdgcn_exp2f(fmaf(s, sl2, mb) - L);
    const bool keep = !dp.enabled || keep_key(rw, j, dp.thr);
    const float dpj = keep ? dpd * dsc : 0.f;
    if (c == 0) {
      ps[j] = p;
      dps[j] = dpj;
      pds[j] = keep ? p * dsc : 0.f;
      dl = fmaf(p, dpj, dl);
    }
  };
#pragma unroll
  for (int i = 0; i < kPre; ++i)
    if (kr + 32 * i < S) probs(kr + 32 * i, kpre[i], vpre[i]);
  for (int j = kr + 32 * kPre; j < S; j += 32) probs(j, ld16(base + j * ld + H), ld16(base + j * ld + 2 * H));
  dl = wave_sum(dl);
  if (lane == 0) red[wave] = dl;
  __syncthreads();
  const float delta = ams * ((red[0] + red[1]) + (red[2] + red[3]));
  // pass 2: dS_j = P_j (dP_j - delta) / sqrt(d); dK_j = dS_j q0, dV_j = Pd_j dO, dQ_0 = sum_j dS_j K_j
  float qacc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float ksum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float vsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  auto grads = [&](int j, const u32x4& kv) {
    const float ds = ams * ps[j] * (dps[j] - delta) * scale;
    axpy8(qacc, ds, kv);
    bf16_t* row = dbase + j * ld;
    if (j > 0) *reinterpret_cast<u32x4*>(row) = u32x4{0, 0, 0, 0};
    *reinterpret_cast<u32x4*>(row + H) = scale8(ds, qv, ksum);
    *reinterpret_cast<u32x4*>(row + 2 * H) = scale8(ams * pds[j], dov, vsum);
  };
#pragma unroll
  for (int i = 0; i < kPre; ++i)
    if (kr + 32 * i < S) grads(kr + 32 * i, kpre[i]);
  for (int j = kr + 32 * kPre; j < S; j += 32) grads(j, ld16(base + j * ld + H));
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    qacc[k] = sum_stride8(qacc[k]);
    ksum[k] = sum_stride8(ksum[k]);
    vsum[k] = sum_stride8(vsum[k]);
  }
  if (lane < 8) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      csum[0][wave][lane * 8 + k] = qacc[k];
      csum[1][wave][lane * 8 + k] = ksum[k];
      csum[2][wave][lane * 8 + k] = vsum[k];
    }
  }
  __syncthreads();
  if (tid < D) {
    const int col = hh * D + tid;
    const bf16_t dq = f2bf((csum[0][0][tid] + csum[0][1][tid]) + (csum[0][2][tid] + csum[0][3][tid]));
    dqkv[(int64_t)b * S * ld + col] = dq;
    if (dbias != nullptr) {
      atomicAdd(dbias + col, bf2f(dq));
      atomicAdd(dbias + H + col, (csum[1][0][tid] + csum[1][1][tid]) + (csum[1][2][tid] + csum[1][3][tid]));
      atomicAdd(dbias + 2 * H + col, (csum[2][0][tid] + csum[2][1][tid]) + (csum[2][2][tid] + csum[2][3][tid]));
    }
  }
}

}  // namespace acls

// dynamic LDS of the backward: 3 fp32 per key
bool attn_cls_supported(int S, int head_dim) { return head_dim == acls::D && S >= 2 && S % 2 == 0 && S <= 4096; }

void launch_attn_cls_fwd(const bf16_t* qkv, const float* mask, bf16_t* out, float* lse2, int B, int S, int heads,
                         double p, uint64_t seed, hipStream_t st) {
  if (!attn_cls_supported(S, acls::D)) abort();
  const DropoutParams dp = make_dropout(p, seed);
  const float sl2 = acls::kLog2e / sqrtf((float)acls::D);
  hipLaunchKernelGGL(acls::attn_cls_fwd_kernel, dim3(B * heads), dim3(256), (size_t)S * sizeof(float), st, qkv, mask,
                     out, lse2, S, heads, sl2, dp);
  HSD_CHECK_LAUNCH();
}

void launch_attn_cls_bwd(const bf16_t* qkv, const float* mask, const bf16_t* dctx, const float* lse2, bf16_t* dqkv,
                         float* dbias, int B, int S, int heads, double p, uint64_t seed, hipStream_t st) {
  if (!attn_cls_supported(S, acls::D)) abort();
  const DropoutParams dp = make_dropout(p, seed);
  const float sl2 = acls::kLog2e / sqrtf((float)acls::D);
  const float scale = 1.0f / sqrtf((float)acls::D);
  hipLaunchKernelGGL(acls::attn_cls_bwd_kernel, dim3(B * heads), dim3(256), (size_t)3 * S * sizeof(float), st, qkv,
                     mask, dctx, lse2, dqkv, dbias, S, heads, sl2, scale, dp);
  HSD_CHECK_LAUNCH();
}

}  // namespace hsd
