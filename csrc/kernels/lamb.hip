// Fused LAMB over the flat parameter store (optim/lamb.py, --optimizer lamb): TF Addons' LAMB.
//
//   m = b1 m + (1-b1) g ;  v = b2 v + (1-b2) g² ;  m̂ = m / (1-b1ᵗ) ;  v̂ = v / (1-b2ᵗ)
//   u = m̂ / (√v̂ + eps)  [+ wd · w on segments with decay]
//   r = ‖w‖₂ / ‖u‖₂ if ‖w‖₂ > 0 and ‖u‖₂ > 0 else 1     per segment (r = 1 and no decay on excluded segments)
//   w -= lr · r · u                                       (lr · μ with per-segment multipliers: lamb_stage2's kLrMul)
//
// The norms are per parameter (segment), so a slice of whole segments is stepped on its own (under the backward). Each
// segment's 64-aligned span is cut into tiles of kLambTile elements anchored at the segment's own offset (the last one
// short), so a tile never straddles two segments and the tiling does not depend on how the buffer is sliced:
//
//   lamb_stage1   one workgroup per tile: reads g, w, m, v, writes m, v (and clears g), computes u in registers and
//                 writes the tile's fp32 partial pair (Σw², Σu²)
//   lamb_ratio    one workgroup per segment: the segment's tile partials in index order in fp64 -> (r, Σw², Σu²)
//   lamb_stage2   one workgroup per tile: reads w, m, v, recomputes u with the SAME inline function (lamb_u, FP
//                 contraction off: the u applied is the u measured, bit for bit), writes w and the bf16 copy / halves
//
// No atomics: every partial has one writer and the combine order is fixed, so two runs, and a slice-by-slice run against
// a whole-buffer one, give identical bits. Nothing returns to the host: the launches capture into a whole-step graph.
// Alignment padding between segments is zero in w, g, m, v; it gives u = 0 and adds nothing to either norm.
#include "common.h"

namespace hsd {

constexpr int kLambThreads = 256;
constexpr int kLambU = 2;  // 16-B chunks per thread per trip (adam_kernel's U-chunk pattern)
constexpr int kLambTileElems = 4096;  // 2 trips of 256 threads x 2 chunks x 4 elements
constexpr int kLambRatioThreads = 256;

int lamb_tile() { return kLambTileElems; }

// Per-step scalars of a captured step, fp32 [8] on the device (LAMB's own layout, optim/lamb.py):
//   [0] lr  [1] 1/(1-b1ᵗ)  [2] 1/(1-b2ᵗ)  [3] eps  [4] grad_scale  [5] wd  [6] 1 - ema decay (kEma)  [7] unused
struct LambScalars {
  float lr, ibc1, ibc2, eps, gscale, wd;
};

__device__ __forceinline__ LambScalars lamb_scalars(LambScalars s, const float* __restrict__ coef) {
  if (coef != nullptr) {
    s.lr = coef[0];
    s.ibc1 = coef[1];
    s.ibc2 = coef[2];
    s.eps = coef[3];
    s.gscale = coef[4];
    s.wd = coef[5];
  }
  return s;
}

// u of one element from the UPDATED moments and the not yet updated weight. Both stages call this one function with
// contraction off, so the compiler cannot fuse a multiply-add in one of them and not in the other.
__device__ __forceinline__ float lamb_u(float w, float m, float v, float ibc1, float ibc2, float eps, float wd) {
#pragma clang fp contract(off)
  const float mh = m * ibc1;
  const float vh = v * ibc2;
  const float q = mh / (sqrtf(vh) + eps);
  const float d = wd * w;
  return q + d;
}

template <bool kGradBf16>
__device__ __forceinline__ f32x4 lamb_load_grad(const void* __restrict__ g_, int64_t i) {
  if constexpr (kGradBf16) {
    const u32x2 w = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(g_) + i);
    return f32x4{lo_bf(w.x), hi_bf(w.x), lo_bf(w.y), hi_bf(w.y)};
  } else {
    return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g_) + i);
  }
}

// tiles: int64 [*, 3] = (start element, length, segment); segs: int64 [*, 3] = (first tile, tiles, adapt / decay flag).
// Block b works on tile tile0 + b. Every thread keeps kLambU x 4 independent fp32 accumulators per norm, so its longest
// addition chain is the trip count (2 for a full tile), then 2 (lanes) + 1 (slots) + 6 (wave) + 3 (the 4 waves).
template <bool kGradBf16, bool kClip>
__global__ __launch_bounds__(kLambThreads) void lamb_stage1_kernel(
    const float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, void* __restrict__ g_,
    const int64_t* __restrict__ tiles, const int64_t* __restrict__ segs, int64_t tile0, float* __restrict__ partials,
    LambScalars s, float b1, float b2, const float* __restrict__ coef, const float* __restrict__ clip, int zero_g) {
  s = lamb_scalars(s, coef);
  float gscale = s.gscale;
  // global-norm clipping (gradnorm.hip): ONE fp32 multiply, as adam_kernel's kClip
  if constexpr (kClip) gscale *= clip[0];
  const int64_t t = tile0 + blockIdx.x;
  const int64_t base4 = tiles[t * 3] >> 2;
  const int n4 = (int)(tiles[t * 3 + 1] >> 2);
  const int64_t seg = tiles[t * 3 + 2];
  const float wd = segs[seg * 3 + 2] ? s.wd : 0.0f;
  f32x4 aw[kLambU], au[kLambU];
#pragma unroll
  for (int u = 0; u < kLambU; ++u) aw[u] = au[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int i0 = threadIdx.x; i0 < n4; i0 += kLambThreads * kLambU) {
    f32x4 g[kLambU], pp[kLambU], mm[kLambU], vv[kLambU];
#pragma unroll
    for (int u = 0; u < kLambU; ++u) {
      const int i = i0 + u * kLambThreads;
      if (i < n4) {
        g[u] = lamb_load_grad<kGradBf16>(g_, base4 + i);
        pp[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p) + base4 + i);
        mm[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(m) + base4 + i);
        vv[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(v) + base4 + i);
      }
    }
#pragma unroll
    for (int u = 0; u < kLambU; ++u) {
      const int i = i0 + u * kLambThreads;
      if (i >= n4) break;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float gk = g[u][k] * gscale;
        mm[u][k] = b1 * mm[u][k] + (1.0f - b1) * gk;
        vv[u][k] = b2 * vv[u][k] + (1.0f - b2) * gk * gk;
      }
      // plain stores: stage 2 reads the moments back within the same slice
      reinterpret_cast<f32x4*>(m)[base4 + i] = mm[u];
      reinterpret_cast<f32x4*>(v)[base4 + i] = vv[u];
      if (zero_g) {
        if constexpr (kGradBf16) __builtin_nontemporal_store(u32x2{0u, 0u}, reinterpret_cast<u32x2*>(g_) + base4 + i);
        else __builtin_nontemporal_store(f32x4{0.f, 0.f, 0.f, 0.f}, reinterpret_cast<f32x4*>(g_) + base4 + i);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float uk = lamb_u(pp[u][k], mm[u][k], vv[u][k], s.ibc1, s.ibc2, s.eps, wd);
        aw[u][k] = fmaf(pp[u][k], pp[u][k], aw[u][k]);
        au[u][k] = fmaf(uk, uk, au[u][k]);
      }
    }
  }
  static_assert(kLambU == 2, "slot combine below is written for 2 load slots");
  const float sw = ((aw[0][0] + aw[0][1]) + (aw[0][2] + aw[0][3])) + ((aw[1][0] + aw[1][1]) + (aw[1][2] + aw[1][3]));
  const float su = ((au[0][0] + au[0][1]) + (au[0][2] + au[0][3])) + ((au[1][0] + au[1][1]) + (au[1][2] + au[1][3]));
  const float tw = wave_sum(sw), tu = wave_sum(su);
  __shared__ float lds[2][kLambThreads / kWave];
  if ((threadIdx.x & (kWave - 1)) == 0) {
    lds[0][threadIdx.x / kWave] = tw;
    lds[1][threadIdx.x / kWave] = tu;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float bw = lds[0][0], bu = lds[1][0];
#pragma unroll
    for (int w = 1; w < kLambThreads / kWave; ++w) {
      bw += lds[0][w];
      bu += lds[1][w];
    }
    partials[t * 2] = bw;
    partials[t * 2 + 1] = bu;
  }
}

// One workgroup per segment seg0 + blockIdx.x: thread t adds the segment's tile partials t, t + T, ... in index order in
// fp64, then a fixed pairwise tree in LDS (grad_clip_finalize_kernel's). ratio[seg] = (r, Σw², Σu²), fp32.
__global__ __launch_bounds__(kLambRatioThreads) void lamb_ratio_kernel(const float* __restrict__ partials,
                                                                       const int64_t* __restrict__ segs, int64_t seg0,
                                                                       float* __restrict__ ratio) {
  const int64_t seg = seg0 + blockIdx.x;
  const int64_t first = segs[seg * 3], nt = segs[seg * 3 + 1];
  const bool adapt = segs[seg * 3 + 2] != 0;
  double a = 0.0, b = 0.0;
  for (int64_t i = threadIdx.x; i < nt; i += kLambRatioThreads) {
    a += (double)partials[(first + i) * 2];
    b += (double)partials[(first + i) * 2 + 1];
  }
  __shared__ double lds[2][kLambRatioThreads];
  lds[0][threadIdx.x] = a;
  lds[1][threadIdx.x] = b;
  __syncthreads();
#pragma unroll
  for (int h = kLambRatioThreads / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
      lds[0][threadIdx.x] += lds[0][threadIdx.x + h];
      lds[1][threadIdx.x] += lds[1][threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double wn = sqrt(lds[0][0]), un = sqrt(lds[1][0]);
    // a NaN norm compares false and leaves 1 (as gradnorm.hip's coefficient); excluded segments take 1
    ratio[seg * 3] = (adapt && wn > 0.0 && un > 0.0) ? (float)(wn / un) : 1.0f;
    ratio[seg * 3 + 1] = (float)lds[0][0];
    ratio[seg * 3 + 2] = (float)lds[1][0];
  }
}

// kWriteBf16 / kLo: the bf16 compute copy, or the fp32 run's hi / lo halves, exactly as adam_kernel writes them.
// kLrMul (launched when `lr_mul` is given; optim/groups.py, --layerwise_lr_decay): fp32 [segments], the tile's segment
// takes the learning rate lr * lr_mul[seg], ONE fp32 multiply ahead of the existing lr * r -- the bits of a launch
// without the table on that segment alone with the host scalar float32(lr * mu). u, the norms and r do not see it. An
// instantiation of its own (adam_kernel's kClip): the kernels without the table keep the code they had.
// kEma (launched when `ema` is given; --ema_decay): the weight average, exactly as adam_kernel's kEma -- the tile's
// chunk of `ema` (indexed base4 + i, as p) loaded with the other loads, updated by ema_lerp from the weight about to be
// stored, stored next to it. Captured steps read w from coef[6]. u, the norms, r and every other output do not see it.
template <bool kWriteBf16, bool kLo, bool kLrMul = false, bool kEma = false>
__global__ __launch_bounds__(kLambThreads) void lamb_stage2_kernel(
    float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v, bf16_t* __restrict__ out,
    bf16_t* __restrict__ out_lo, const int64_t* __restrict__ tiles, const int64_t* __restrict__ segs, int64_t tile0,
    const float* __restrict__ ratio, LambScalars s, const float* __restrict__ coef,
    const float* __restrict__ lr_mul, float* __restrict__ ema, float ema_w) {
  s = lamb_scalars(s, coef);
  if constexpr (kEma) {
    if (coef != nullptr) ema_w = coef[6];
  }
  const int64_t t = tile0 + blockIdx.x;
  const int64_t base4 = tiles[t * 3] >> 2;
  const int n4 = (int)(tiles[t * 3 + 1] >> 2);
  const int64_t seg = tiles[t * 3 + 2];
  const float wd = segs[seg * 3 + 2] ? s.wd : 0.0f;
  float lr = s.lr;
  if constexpr (kLrMul) lr *= lr_mul[seg];
  const float step = lr * ratio[seg * 3];
  for (int i0 = threadIdx.x; i0 < n4; i0 += kLambThreads * kLambU) {
    f32x4 pp[kLambU], mm[kLambU], vv[kLambU], ee[kLambU];
#pragma unroll
    for (int u = 0; u < kLambU; ++u) {
      const int i = i0 + u * kLambThreads;
      if (i < n4) {
        pp[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p) + base4 + i);
        mm[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(m) + base4 + i);
        vv[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(v) + base4 + i);
        if constexpr (kEma) ee[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(ema) + base4 + i);
      }
    }
#pragma unroll
    for (int u = 0; u < kLambU; ++u) {
      const int i = i0 + u * kLambThreads;
      if (i >= n4) break;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float uk = lamb_u(pp[u][k], mm[u][k], vv[u][k], s.ibc1, s.ibc2, s.eps, wd);
        pp[u][k] = fmaf(-step, uk, pp[u][k]);
      }
      __builtin_nontemporal_store(pp[u], reinterpret_cast<f32x4*>(p) + base4 + i);
      if constexpr (kWriteBf16) {
        u32x2 o;
        o.x = pack_bf2(pp[u][0], pp[u][1]);
        o.y = pack_bf2(pp[u][2], pp[u][3]);
        reinterpret_cast<u32x2*>(out)[base4 + i] = o;
        if constexpr (kLo) {
          u32x2 l;
          l.x = pack_bf2(pp[u][0] - lo_bf(o.x), pp[u][1] - hi_bf(o.x));
          l.y = pack_bf2(pp[u][2] - lo_bf(o.y), pp[u][3] - hi_bf(o.y));
          reinterpret_cast<u32x2*>(out_lo)[base4 + i] = l;
        }
      }
    }
    // the average, from the weights stored above, in a loop of its own (adam_kernel's reason)
    if constexpr (kEma) {
#pragma unroll
      for (int u = 0; u < kLambU; ++u) {
        const int i = i0 + u * kLambThreads;
        if (i >= n4) break;
#pragma unroll
        for (int k = 0; k < 4; ++k) ee[u][k] = ema_lerp(ee[u][k], ema_w, pp[u][k]);
        __builtin_nontemporal_store(ee[u], reinterpret_cast<f32x4*>(ema) + base4 + i);
      }
    }
  }
}

void launch_lamb(float* p, float* m, float* v, void* g, bool grad_bf16, bf16_t* out_bf16, bf16_t* out_lo,
                 const int64_t* tiles, const int64_t* segs, int64_t tile0, int64_t ntiles, int64_t seg0, int64_t nsegs,
                 float* partials, float* ratio, float lr, float ibc1, float ibc2, float eps, float b1, float b2,
                 float gscale, float wd, const float* coef, const float* clip, bool zero_grad, hipStream_t stream,
                 const float* lr_mul, float* ema, float ema_w) {
  if (ntiles <= 0 || nsegs <= 0) return;
  if (out_lo != nullptr && out_bf16 == nullptr) abort();
  const LambScalars s{lr, ibc1, ibc2, eps, gscale, wd};
  const int zg = zero_grad ? 1 : 0;
  const dim3 grid((unsigned)ntiles), block(kLambThreads);
#define HSD_LAMB1(GB, CL)                                                                                       \
  hipLaunchKernelGGL((lamb_stage1_kernel<GB, CL>), grid, block, 0, stream, p, m, v, g, tiles, segs, tile0, partials, \
                     s, b1, b2, coef, clip, zg)
  if (grad_bf16) {
    if (clip != nullptr) HSD_LAMB1(true, true); else HSD_LAMB1(true, false);
  } else {
    if (clip != nullptr) HSD_LAMB1(false, true); else HSD_LAMB1(false, false);
  }
#undef HSD_LAMB1
  HSD_CHECK_LAUNCH();
  hipLaunchKernelGGL(lamb_ratio_kernel, dim3((unsigned)nsegs), dim3(kLambRatioThreads), 0, stream, partials, segs,
                     seg0, ratio);
  HSD_CHECK_LAUNCH();
#define HSD_LAMB2_E(WB, LO, LM, EM)                                                                                   \
  hipLaunchKernelGGL((lamb_stage2_kernel<WB, LO, LM, EM>), grid, block, 0, stream, p, m, v, out_bf16, out_lo, tiles, \
                     segs, tile0, ratio, s, coef, lr_mul, ema, ema_w)
#define HSD_LAMB2_K(WB, LO, LM)                                                                                   \
  do {                                                                                                            \
    if (ema != nullptr) HSD_LAMB2_E(WB, LO, LM, true); else HSD_LAMB2_E(WB, LO, LM, false);                      \
  } while (0)
#define HSD_LAMB2(WB, LO)                                                                                         \
  do {                                                                                                            \
    if (lr_mul != nullptr) HSD_LAMB2_K(WB, LO, true); else HSD_LAMB2_K(WB, LO, false);                           \
  } while (0)
  if (out_lo != nullptr) HSD_LAMB2(true, true);
  else if (out_bf16 != nullptr) HSD_LAMB2(true, false);
  else HSD_LAMB2(false, false);
#undef HSD_LAMB2
#undef HSD_LAMB2_K
#undef HSD_LAMB2_E
  HSD_CHECK_LAUNCH();
}

}  // namespace hsd
