// Fused Adam / AdamW over the flat parameter store (optim/adam.py).
//
// Replaces TF's ResourceApplyAdam, launched once per variable (393 launches for bert-large,
// SURVEY.md §2.10 K17), with ONE launch over flat buffers: 16-B vector IO on master/m/v/grad,
// DP 1/N (and grad-accum 1/k) folded into `grad_scale`, decoupled weight decay gated per
// 64-element block (segments are 64-aligned, so a block never straddles two parameters), and the
// bf16 compute copy written in the same pass (no separate cast kernel).
//
//   m = b1 m + (1-b1) g ;  v = b2 v + (1-b2) g² ;  θ = θ(1 - lr·wd·mask) - step·m/(√v + eps)
#include "common.h"

#include <stdlib.h>

namespace hsd {

template <bool kGradBf16, bool kWriteBf16>
__device__ __forceinline__ f32x4 load_grad(const void* __restrict__ g_, int64_t i) {
  if constexpr (kGradBf16) {
    const u32x2 w = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(g_) + i);
    return f32x4{lo_bf(w.x), hi_bf(w.x), lo_bf(w.y), hi_bf(w.y)};
  } else {
    return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g_) + i);
  }
}

// A scalar that carries the learning rate, times a parameter's multiplier: one fp32 multiply the compiler may not fuse
// into the operation that consumes it (kLrMul below).
__device__ __forceinline__ float lr_scaled(float s, float mu) {
#pragma clang fp contract(off)
  return s * mu;
}

// kLo (fp32 compute, ops/hip32.py): `out` / `out_lo` receive the bf16 hi / lo halves of the updated weight (hi =
// bf16(θ), lo = bf16(θ - hi), exactly split2's), which the split-product GEMMs read directly -- the weights are split
// once per optimizer step instead of at every use in forward and backward.
// zero_g: the kernel also clears the gradient it consumed (16-B stores of the slot it just read), so the next step
// needs no separate memset pass over the whole gradient buffer ahead of its forward (optim/adam.py: set by the
// Trainer's eager steps; the store then skips its zero_grad once).
// U chunks of 4 elements per thread per trip, all U x 4 loads issued before the first use (a one-chunk trip
// leaves ~4 loads in flight per thread, too few to cover HBM latency at the occupancy a CU holds). Every
// byte is touched once per step, so loads and stores are non-temporal (no L2 / MALL pollution).
// kClip (launched when `clip` is given): an instantiation of its own for clipped steps. As a run-time branch the one
// extra load cost the unclipped bf16-compute kernel 4 VGPRs and a wave of occupancy (72 -> 76, 7 -> 6 waves/SIMD) and
// the headline 0.2-0.7 % (profiles/grad_clip_cost.log); this way the unclipped kernels keep the code they had.
// kLrMul (launched when `lr_mul` is given; optim/groups.py, --layerwise_lr_decay): per-parameter learning-rate
// multipliers, an fp32 table with one entry per 64-element block indexed as `decay` is. The learning rate appears in
// `step` and in `lr_wd`; each is scaled by ONE fp32 multiply (lr_scaled: never contracted into the 1 - lr_wd that
// follows), so a segment gets the bits the kernel without the table gives it when launched on that segment alone with
// the host scalars float32(step * mu), float32(lr_wd * mu), and a table of ones gives the bits of no table. An
// instantiation of its own for kClip's reason: the kernels without the table keep the code they had.
// kEma (launched when `ema` is given; --ema_decay): the exponential moving average of the weights, one fp32 buffer laid
// out as `p`. Its chunk is loaded with the other U loads and updated from the weight the kernel is about to store,
// ema += w·(θ - ema) with w = float32(1 - decay) (ema_lerp: three rounded operations), and stored next to `p`: one more
// 16-B load and store per chunk instead of a second pass over weights that were in registers a moment earlier. Nothing
// else reads it: p, m, v, the outputs and the cleared gradient are the bits of the launch without it. `ema_w` is a
// kernel argument; captured steps read it from coef[4]. An instantiation of its own for kClip's reason.
template <bool kGradBf16, bool kWriteBf16, int U, bool kLo = false, bool kClip = false, bool kLrMul = false,
          bool kEma = false>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, float* __restrict__ m,
                                                   float* __restrict__ v, void* __restrict__ g_,
                                                   bf16_t* __restrict__ out, const uint8_t* __restrict__ decay,
                                                   int64_t n4, float step, float eps, float b1, float b2,
                                                   float gscale, float lr_wd, const float* __restrict__ coef,
                                                   bf16_t* __restrict__ out_lo, int zero_g,
                                                   const float* __restrict__ clip,
                                                   const float* __restrict__ lr_mul,
                                                   float* __restrict__ ema, float ema_w) {
  if (coef != nullptr) {  // HIP-graph replays: this step's scalars live on the device (train/graph.py)
    step = coef[0];
    eps = coef[1];
    gscale = coef[2];
    lr_wd = coef[3];
    if constexpr (kEma) ema_w = coef[4];
  }
  // global-norm clipping (gradnorm.hip): the step's clip coefficient, computed on the device, folded into the
  // gradient scale by ONE fp32 multiply (a host replay with float32(gscale) * float32(coef) gives the same bits)
  if constexpr (kClip) gscale *= clip[0];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < n4; i0 += stride * U) {
    f32x4 g[U], pp[U], mm[U], vv[U], ee[U];
    float mu[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * stride;
      if (i < n4) {
        if constexpr (kLrMul) mu[u] = lr_mul[(i * 4) >> 6];
        g[u] = load_grad<kGradBf16, kWriteBf16>(g_, i);
        pp[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p) + i);
        mm[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(m) + i);
        vv[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(v) + i);
        if constexpr (kEma) ee[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(ema) + i);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * stride;
      if (i >= n4) break;
      float wdf = 1.0f;
      float step_g = step, lrwd_g = lr_wd;
      if constexpr (kLrMul) {
        step_g = lr_scaled(step, mu[u]);
        lrwd_g = lr_scaled(lr_wd, mu[u]);
      }
      if (decay != nullptr && lr_wd != 0.0f) wdf = decay[(i * 4) >> 6] ? (1.0f - lrwd_g) : 1.0f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float gk = g[u][k] * gscale;
        mm[u][k] = b1 * mm[u][k] + (1.0f - b1) * gk;
        vv[u][k] = b2 * vv[u][k] + (1.0f - b2) * gk * gk;
        pp[u][k] = pp[u][k] * wdf - step_g * mm[u][k] / (sqrtf(vv[u][k]) + eps);
      }
      __builtin_nontemporal_store(pp[u], reinterpret_cast<f32x4*>(p) + i);
      __builtin_nontemporal_store(mm[u], reinterpret_cast<f32x4*>(m) + i);
      __builtin_nontemporal_store(vv[u], reinterpret_cast<f32x4*>(v) + i);
      if (zero_g) {
        if constexpr (kGradBf16) __builtin_nontemporal_store(u32x2{0u, 0u}, reinterpret_cast<u32x2*>(g_) + i);
        else __builtin_nontemporal_store(f32x4{0.f, 0.f, 0.f, 0.f}, reinterpret_cast<f32x4*>(g_) + i);
      }
      if constexpr (kWriteBf16) {
        u32x2 o;
        o.x = pack_bf2(pp[u][0], pp[u][1]);
        o.y = pack_bf2(pp[u][2], pp[u][3]);
        reinterpret_cast<u32x2*>(out)[i] = o;
        if constexpr (kLo) {
          u32x2 l;
          l.x = pack_bf2(pp[u][0] - lo_bf(o.x), pp[u][1] - hi_bf(o.x));
          l.y = pack_bf2(pp[u][2] - lo_bf(o.y), pp[u][3] - hi_bf(o.y));
          reinterpret_cast<u32x2*>(out_lo)[i] = l;
        }
      }
    }
    // the average, from the weights stored above, in a loop of its own: in the loop above the compiler made other
    // contraction choices for the weight update with this code beside it, and p would not be the bits of the kernel
    // without kEma
    if constexpr (kEma) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t i = i0 + u * stride;
        if (i >= n4) break;
#pragma unroll
        for (int k = 0; k < 4; ++k) ee[u][k] = ema_lerp(ee[u][k], ema_w, pp[u][k]);
        __builtin_nontemporal_store(ee[u], reinterpret_cast<f32x4*>(ema) + i);
      }
    }
  }
}

void launch_adam(float* p, float* m, float* v, void* g, bool grad_bf16, bf16_t* out_bf16,
                 const uint8_t* decay, int64_t n, float step, float eps, float b1, float b2, float gscale,
                 float lr_wd, const float* coef, hipStream_t stream, bf16_t* out_lo, bool zero_grad,
                 const float* clip, const float* lr_mul, float* ema, float ema_w) {
  const int zg = zero_grad ? 1 : 0;
  int64_t n4 = n / 4;  // n is a multiple of 1024 (FlatParamStore)
  int threads = 256;
  int64_t blocks = (n4 + threads - 1) / threads;
  if (blocks > 256 * 8) blocks = 256 * 8;  // grid-stride: 8 blocks (32 waves) per CU over 256 CUs
  // two 16-B chunks per thread per trip (1 and 4 measured slower: profiles/bench_adam_r2.json)
#define HSD_ADAM_E(GB, WB, LO, CL, LM, EM)                                                                          \
  hipLaunchKernelGGL((adam_kernel<GB, WB, 2, LO, CL, LM, EM>), dim3((unsigned)blocks), dim3(threads), 0, stream, p, \
                     m, v, g, out_bf16, decay, n4, step, eps, b1, b2, gscale, lr_wd, coef, out_lo, zg, clip, lr_mul, \
                     ema, ema_w)
#define HSD_ADAM_K(GB, WB, LO, CL, LM)                                                                              \
  do {                                                                                                              \
    if (ema != nullptr) HSD_ADAM_E(GB, WB, LO, CL, LM, true); else HSD_ADAM_E(GB, WB, LO, CL, LM, false);          \
  } while (0)
#define HSD_ADAM_C(GB, WB, LO, LM)                                                                                  \
  do {                                                                                                              \
    if (clip != nullptr) HSD_ADAM_K(GB, WB, LO, true, LM); else HSD_ADAM_K(GB, WB, LO, false, LM);                 \
  } while (0)
#define HSD_ADAM(GB, WB, LO)                                                                                        \
  do {                                                                                                              \
    if (lr_mul != nullptr) HSD_ADAM_C(GB, WB, LO, true); else HSD_ADAM_C(GB, WB, LO, false);                       \
  } while (0)
  if (out_lo != nullptr) {
    if (out_bf16 == nullptr) abort();
    if (grad_bf16) HSD_ADAM(true, true, true); else HSD_ADAM(false, true, true);
    HSD_CHECK_LAUNCH();
    return;
  }
  if (grad_bf16) {
    if (out_bf16) HSD_ADAM(true, true, false); else HSD_ADAM(true, false, false);
  } else {
    if (out_bf16) HSD_ADAM(false, true, false); else HSD_ADAM(false, false, false);
  }
#undef HSD_ADAM
#undef HSD_ADAM_C
#undef HSD_ADAM_K
#undef HSD_ADAM_E
  HSD_CHECK_LAUNCH();
}

}  // namespace hsd
