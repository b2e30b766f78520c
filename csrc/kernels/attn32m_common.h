// Shared device core of the split-product fp32 attention kernels (attention32m.hip: dense [B, S] batches;
// attention32m_varlen.hip: packed batches): the LDS-DMA of one [64][64] bf16 image, the stage hand-over barrier, the
// on-the-fly hi / lo split of accumulator values, the three-term split product and the fp32 row store.
#pragma once
#include "attn_common.h"

namespace hsd {
namespace a32m {

using namespace attn;
constexpr int TILE = 64 * D;  // one [64][64] bf16 image

// 64 rows x 64 cols starting at src0 into a [64][64] image: 8 DMA instructions, 2 per wave (attentionS.hip dma_tile)
__device__ __forceinline__ void dma_tile(bf16_t* img, const bf16_t* __restrict__ src0, int64_t ld, int wave, int lane) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int g = wave * 2 + i;
    const int row = g * 8 + (lane >> 3);
    const int lc = (lane & 7) ^ swz(row);
    const bf16_t* src = src0 + (int64_t)row * ld + lc * 8;
    const uint32_t dst = (uint32_t)__builtin_amdgcn_readfirstlane(
        (int)(uint32_t)(size_t)(__attribute__((address_space(3))) bf16_t*)(img + g * 512));
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(src), "s"(dst)
                 : "memory");
  }
}

// every wave's DMA of the current tile landed; every wave done with the stage the next DMA overwrites
__device__ __forceinline__ void tile_sync() {
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

template <typename T>
__device__ __forceinline__ void settle(const T& v) {
  asm volatile("" ::"v"(v));
}

// hi / lo bf16 fragments of 8 fp32 accumulator values (registers 8s .. 8s+7): hi = bf16(x), lo = bf16(x - hi)
__device__ __forceinline__ void pack8_split(const f32x16& acc, int s, bf16x8& hi, bf16x8& lo) {
  u32x4 h, l;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float a = acc[8 * s + 2 * j], b = acc[8 * s + 2 * j + 1];
    h[j] = pack_bf2(a, b);
    l[j] = pack_bf2(a - lo_bf(h[j]), b - hi_bf(h[j]));
  }
  hi = __builtin_bit_cast(bf16x8, h);
  lo = __builtin_bit_cast(bf16x8, l);
}

__device__ __forceinline__ f32x16 mma(const bf16x8& a, const bf16x8& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
// ah·bh + al·bh + ah·bl
__device__ __forceinline__ f32x16 mma3(const bf16x8& ah, const bf16x8& al, const bf16x8& bh, const bf16x8& bl,
                                       f32x16 c) {
  c = mma(ah, bh, c);
  c = mma(al, bh, c);
  return mma(ah, bl, c);
}

// acc (32 rows on the lane x 64 d in registers: d = 32 blk + (reg & 3) + 8 (reg >> 2) + 4 hf) * scale -> fp32 rows of
// dst (row stride ld): four 16-B stores per accumulator. A lane writes its own row only (no cross-lane step), so a
// caller may predicate the call per lane.
__device__ __forceinline__ void store_rows32(const f32x16& a0, const f32x16& a1, float scale, float* __restrict__ dst,
                                             int64_t ld, int lane) {
  const int r = lane & 31, h = lane >> 5;
  float* row = dst + (int64_t)r * ld + 4 * h;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    *reinterpret_cast<f32x4*>(row + 8 * g) =
        f32x4{a0[4 * g] * scale, a0[4 * g + 1] * scale, a0[4 * g + 2] * scale, a0[4 * g + 3] * scale};
    *reinterpret_cast<f32x4*>(row + 32 + 8 * g) =
        f32x4{a1[4 * g] * scale, a1[4 * g + 1] * scale, a1[4 * g + 2] * scale, a1[4 * g + 3] * scale};
  }
}

}  // namespace a32m
}  // namespace hsd
