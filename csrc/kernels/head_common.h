// Device helpers shared by the fused task heads (cls_head.hip, token_head.hip): a lane's 8 bf16 elements (16 B) as
// floats and back, and their dropout keep factors. head_stats.hip holds the heads' common stats reducer.
#pragma once

#include "common.h"

namespace hsd {
namespace head {

__device__ __forceinline__ void unpack8(const u32x4& w, float (&v)[8]) {
  v[0] = lo_bf(w.x); v[1] = hi_bf(w.x); v[2] = lo_bf(w.y); v[3] = hi_bf(w.y);
  v[4] = lo_bf(w.z); v[5] = hi_bf(w.z); v[6] = lo_bf(w.w); v[7] = hi_bf(w.w);
}

__device__ __forceinline__ u32x4 pack8(const float (&v)[8]) {
  return u32x4{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7])};
}

// keep factors (0 or 1/(1-p)) of the 8 elements from column h0 (h0 % 8 == 0) of the row whose row word is rw
// (dropout_row of the row: [R][H] site, mask rows of width H; a caller hoists it out of its column loop)
__device__ __forceinline__ void keep8(uint32_t rw, int h0, const DropoutParams& dp, float (&kf)[8]) {
  const uint32_t x = rw ^ drop_col((uint32_t)h0 >> 1);
#pragma unroll
  for (int j = 0; j < 4; ++j) {  // (h0 / 2) % 4 == 0: pair h0 / 2 + j = h0 / 2 ^ j
    const uint32_t b = drop_fin(x ^ drop_col((uint32_t)j));
    kf[2 * j] = keep_factor(b, 0, dp);
    kf[2 * j + 1] = keep_factor(b, 1, dp);
  }
}

}  // namespace head
}  // namespace hsd
