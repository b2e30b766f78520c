// The stats reducer of the fused classification heads (cls_head.hip, token_head.hip): their forward kernels write
// per-block partial sums {loss sum, hits, n_valid} into partials [nblk][4]; one workgroup adds them, no memset, no
// atomics, the same bits every run. (The span head's span_stats_kernel, qa_head.hip, is a different reduction.)
//
// hipcc -Rpass-analysis=kernel-resource-usage (gfx950, -O3): head_stats_kernel 14 VGPRs, scratch 0, LDS 48 B
#include "common.h"
#include "launchers.h"

namespace hsd {

// stats = {loss_sum / max(n_valid, 1), hits, n_valid, loss_sum}
__global__ __launch_bounds__(256) void head_stats_kernel(const float* __restrict__ partials, int nblk,
                                                         float* __restrict__ stats) {
  __shared__ float red[4][3];
  float s[3] = {0.f, 0.f, 0.f};
  for (int b = threadIdx.x; b < nblk; b += blockDim.x) {
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] += partials[(int64_t)b * 4 + k];
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 3; ++k) s[k] = wave_sum(s[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) red[wave][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float t[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
    stats[0] = t[0] / fmaxf(t[2], 1.0f);
    stats[1] = t[1];
    stats[2] = t[2];
    stats[3] = t[0];
  }
}

void launch_head_stats(const float* partials, int nblk, float* stats, hipStream_t st) {
  hipLaunchKernelGGL(head_stats_kernel, dim3(1), dim3(256), 0, st, partials, nblk, stats);
  HSD_CHECK_LAUNCH();
}

}  // namespace hsd
