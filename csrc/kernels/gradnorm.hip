// Global-norm gradient clipping for the fused Adam (optim/adam.py, --max_grad_norm).
//
//   norm = ||g · gscale||₂ over the whole flat gradient buffer;  coef = C / norm if norm > C else 1
//
// (tf.clip_by_global_norm, the math of Keras' global_clipnorm: no epsilon; an infinite norm gives 0, a NaN norm
// compares false and leaves 1.) Exact clipping needs the whole norm before any weight moves, so the step is
//
//   grad_sumsq          per flat-buffer slice, as the slice's gradients become final (under the backward): one fp32
//                       partial per block into the slice's own slots of a partials buffer
//   grad_clip_finalize  one workgroup: all partials -> [norm, coef] on the device
//   adam_kernel         reads coef (adam.hip `clip`) and folds it into grad_scale
//
// No atomics anywhere: every partial has one writer and the combine order is fixed, so the norm is bit-reproducible
// from run to run. Nothing returns to the host, so the three launches capture into a whole-step HIP graph.
#include "common.h"

namespace hsd {

constexpr int kSumsqThreads = 256;
constexpr int kSumsqU = 4;            // 16-B loads in flight per thread per trip (adam_kernel's U-chunk pattern)
constexpr int kSumsqMaxBlocks = 512;  // 2 blocks (8 waves) per CU over 256 CUs: fixes the partial count per slice
constexpr int kFinalizeThreads = 1024;

// Blocks (= partials written) of a grad_sumsq launch over n elements: the host sizes the partials buffer from this.
int grad_sumsq_blocks(int64_t n, bool grad_bf16) {
  const int64_t chunks = n / (grad_bf16 ? 8 : 4);  // 16-B chunks
  int64_t blocks = (chunks + kSumsqThreads - 1) / kSumsqThreads;
  if (blocks > kSumsqMaxBlocks) blocks = kSumsqMaxBlocks;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

// Sum of squares of n16 16-B chunks (4 fp32 or 8 bf16 gradients each) starting at g_. Every thread keeps kSumsqU x 4
// independent fp32 accumulators (one per 16-B load slot and vector lane), so its longest addition chain is the trip
// count (twice that for bf16: two squares per lane per chunk), not the element count; they are combined pairwise, then
// across the wave (wave_sum), then across the block's 4 waves in LDS in wave order.
template <bool kGradBf16>
__global__ __launch_bounds__(kSumsqThreads) void grad_sumsq_kernel(const void* __restrict__ g_, int64_t n16,
                                                                   float* __restrict__ partials) {
  f32x4 acc[kSumsqU];
#pragma unroll
  for (int u = 0; u < kSumsqU; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < n16; i0 += stride * kSumsqU) {
    if constexpr (kGradBf16) {
      u32x4 w[kSumsqU];
#pragma unroll
      for (int u = 0; u < kSumsqU; ++u) {
        const int64_t i = i0 + u * stride;
        w[u] = i < n16 ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(g_) + i) : u32x4{0u, 0u, 0u, 0u};
      }
#pragma unroll
      for (int u = 0; u < kSumsqU; ++u) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float a = lo_bf(w[u][k]), b = hi_bf(w[u][k]);
          acc[u][k] = fmaf(a, a, acc[u][k]);
          acc[u][k] = fmaf(b, b, acc[u][k]);
        }
      }
    } else {
      f32x4 g[kSumsqU];
#pragma unroll
      for (int u = 0; u < kSumsqU; ++u) {
        const int64_t i = i0 + u * stride;
        g[u] = i < n16 ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g_) + i) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int u = 0; u < kSumsqU; ++u) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[u][k] = fmaf(g[u][k], g[u][k], acc[u][k]);
      }
    }
  }
  float s[kSumsqU];
#pragma unroll
  for (int u = 0; u < kSumsqU; ++u) s[u] = (acc[u][0] + acc[u][1]) + (acc[u][2] + acc[u][3]);
  static_assert(kSumsqU == 4, "pairwise combine below is written for 4 load slots");
  float t = wave_sum((s[0] + s[1]) + (s[2] + s[3]));
  __shared__ float lds[kSumsqThreads / kWave];
  if ((threadIdx.x & (kWave - 1)) == 0) lds[threadIdx.x / kWave] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    float b = lds[0];
#pragma unroll
    for (int w = 1; w < kSumsqThreads / kWave; ++w) b += lds[w];
    partials[blockIdx.x] = b;
  }
}

// One workgroup: thread t adds partials t, t + T, t + 2T, ... in index order in fp64, then a fixed pairwise tree in
// LDS; norm = sqrt(sum · gscale²). gscale is the host argument, or coef[2] when the step's scalars live on the device
// (captured steps: exactly adam_kernel's override). out[0] = norm, out[1] = coef, both fp32.
__global__ __launch_bounds__(kFinalizeThreads) void grad_clip_finalize_kernel(const float* __restrict__ partials,
                                                                              int64_t nparts, float gscale,
                                                                              const float* __restrict__ coef,
                                                                              float max_norm, float* __restrict__ out) {
  if (coef != nullptr) gscale = coef[2];
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < nparts; i += kFinalizeThreads) a += (double)partials[i];
  __shared__ double lds[kFinalizeThreads];
  lds[threadIdx.x] = a;
  __syncthreads();
#pragma unroll
  for (int h = kFinalizeThreads / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) lds[threadIdx.x] += lds[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double norm = sqrt(lds[0] * (double)gscale * (double)gscale);
    const double c = (double)max_norm;
    out[0] = (float)norm;
    out[1] = norm > c ? (float)(c / norm) : 1.0f;  // inf norm -> 0; NaN norm compares false -> 1; C = inf never clips
  }
}

void launch_grad_sumsq(const void* g, bool grad_bf16, int64_t n, float* partials, hipStream_t stream) {
  const int64_t n16 = n / (grad_bf16 ? 8 : 4);  // n is a multiple of 64
  const int blocks = grad_sumsq_blocks(n, grad_bf16);
  if (grad_bf16)
    hipLaunchKernelGGL((grad_sumsq_kernel<true>), dim3((unsigned)blocks), dim3(kSumsqThreads), 0, stream, g, n16,
                       partials);
  else
    hipLaunchKernelGGL((grad_sumsq_kernel<false>), dim3((unsigned)blocks), dim3(kSumsqThreads), 0, stream, g, n16,
                       partials);
  HSD_CHECK_LAUNCH();
}

void launch_grad_clip_finalize(const float* partials, int64_t nparts, float gscale, const float* coef, float max_norm,
                               float* out, hipStream_t stream) {
  hipLaunchKernelGGL(grad_clip_finalize_kernel, dim3(1), dim3(kFinalizeThreads), 0, stream, partials, nparts, gscale,
                     coef, max_norm, out);
  HSD_CHECK_LAUNCH();
}

}  // namespace hsd
