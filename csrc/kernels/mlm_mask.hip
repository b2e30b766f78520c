// Dynamic masked-LM masking on the device (--mlm_masking dynamic; definition: ops/rng.py "MLM mask", bit-identical).
//
// A batch is a flat buffer of N token ids ([B*S] padded, or the [T] rows of a packed batch). Token t draws the two
// 32-bit words w0 = bits(t, 0) and w1 = bits(t, 1) of the dropout hash (common.h) under the mask seed's key:
//
//   maskable(t) = attention_mask[t] != 0  &&  id[t] is no special id  &&  labels_in[t] != -100
//   selected(t) = maskable(t)  &&  (w0 & 0xFFFF) < thr                       thr = round(p * 65536)
//   a = w0 >> 16:  a < 52429 -> <mask>;  a < 58982 -> rand_lo + ((w1 * (rand_hi - rand_lo)) >> 32);  else unchanged
//
// Ordered compaction without ordering atomics and without a host sync: the selected positions go in ascending t (the
// order nonzero() gives) into sel[cap] / tgt[cap]; a selection of rank >= cap is dropped (id kept, label -100,
// inv -1) and counted. Two launches:
//
//   pass 1  one token per thread: the decision, a wave64 ballot + popcount, one count per block into ws[block]
//   pass 2  every block re-derives its decisions (two hashes per token: cheaper than a flag buffer round trip), sums
//           the counts of the blocks before it and of all blocks (a few thousand int32 at most, L2-resident), adds
//           the ballot prefix inside the block and writes ids_out, labels_out, inv, sel, tgt; the ranks n .. cap-1 get
//           sel = 0 / tgt = -100 from a grid-stride loop; block 0 writes counts = {n, dropped} and n_valid = float(n).
//
// Integer sums only, so two runs give the same bits.
//
// mlm_scatter_rows: the fixed-capacity head's backward, dh[t] = inv[t] >= 0 ? dx[inv[t]] : 0 over [N, H] bf16 in
// 16-B accesses; every row of dh is written exactly once (no memset pass, no index_copy_).
#include "common.h"
#include "launchers.h"

namespace hsd {

constexpr int kMlmBlock = 256;
constexpr uint32_t kMlmMaskShare = 52429u;  // round(0.8 * 65536)
constexpr uint32_t kMlmRandShare = 58982u;  // round(0.9 * 65536)

__device__ __forceinline__ uint32_t mlm_key(const MlmMaskParams& p) {
  uint32_t lo = p.seed_lo, hi = p.seed_hi;
  if (p.dev_seed != nullptr) {  // the process-wide device step seed, folded in as resolve_seed does for dropout
    lo ^= p.dev_seed[0];
    hi ^= p.dev_seed[1];
  }
  return dropout_key(lo, hi);
}

// the decision for token t (t < N): selected or not, and w0 / w1 for the replacement
__device__ __forceinline__ bool mlm_selected(const MlmMaskParams& p, uint32_t key, int64_t t, int64_t id, uint32_t& w0,
                                             uint32_t& w1) {
  const uint32_t rw = drop_row((uint32_t)t, key);
  w0 = drop_fin(rw);  // column pair 0: C(0) = 0
  w1 = drop_fin(rw ^ drop_col(1));
  bool ok = p.labels_in == nullptr || p.labels_in[t] != -100;
  if (p.attention_mask != nullptr) ok = ok && p.attention_mask[t] != 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) ok = ok && !(k < p.n_special && id == p.special[k]);
  return ok && (w0 & 0xFFFFu) < p.thr;
}

// block-wide exclusive prefix of a 0/1 flag (4 waves of 64) and the block's total; smem: int[4]
__device__ __forceinline__ int block_flag_prefix(bool flag, int* smem, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long b = __ballot(flag);
  if (lane == 0) smem[wave] = __popcll(b);
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kMlmBlock / 64; ++w) {
    const int c = smem[w];
    before += w < wave ? c : 0;
    total += c;
  }
  return before + __popcll(b & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(kMlmBlock) void mlm_count_kernel(MlmMaskParams p) {
  __shared__ int smem[kMlmBlock / 64];
  const uint32_t key = mlm_key(p);
  const int64_t t = (int64_t)blockIdx.x * kMlmBlock + threadIdx.x;
  bool s = false;
  if (t < p.N) {
    uint32_t w0, w1;
    s = mlm_selected(p, key, t, p.ids[t], w0, w1);
  }
  int total;
  block_flag_prefix(s, smem, total);
  if (threadIdx.x == 0) p.ws[blockIdx.x] = total;
}

__global__ __launch_bounds__(kMlmBlock) void mlm_write_kernel(MlmMaskParams p) {
  __shared__ int smem[kMlmBlock / 64];
  __shared__ int red[2][kMlmBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // counts of the blocks before this one, and of all blocks
  int before = 0, all = 0;  // <= N < 2^31
  for (int i = threadIdx.x; i < (int)gridDim.x; i += kMlmBlock) {
    const int c = p.ws[i];
    all += c;
    if (i < (int)blockIdx.x) before += c;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    before += __shfl_xor(before, o, 64);
    all += __shfl_xor(all, o, 64);
  }
  if (lane == 0) {
    red[0][wave] = before;
    red[1][wave] = all;
  }
  __syncthreads();
  before = all = 0;
#pragma unroll
  for (int w = 0; w < kMlmBlock / 64; ++w) {
    before += red[0][w];
    all += red[1][w];
  }
  const int cap = p.cap;
  const int n = all < cap ? all : cap;

  const uint32_t key = mlm_key(p);
  const int64_t t = (int64_t)blockIdx.x * kMlmBlock + threadIdx.x;
  const bool in = t < p.N;
  int64_t id = 0;
  uint32_t w0 = 0, w1 = 0;
  bool s = false;
  if (in) {
    id = p.ids[t];
    s = mlm_selected(p, key, t, id, w0, w1);
  }
  int total;
  const int rank = before + block_flag_prefix(s, smem, total);
  if (in) {
    const bool take = s && rank < cap;
    int64_t out = id;
    if (take) {
      const uint32_t a = w0 >> 16;
      if (a < kMlmMaskShare) out = p.mask_id;
      else if (a < kMlmRandShare) out = p.rand_lo + (int64_t)(((uint64_t)w1 * (uint64_t)(p.rand_hi - p.rand_lo)) >> 32);
      p.sel[rank] = t;
      p.tgt[rank] = id;
    }
    p.ids_out[t] = out;
    p.labels_out[t] = take ? id : -100;
    p.inv[t] = take ? rank : -1;
  }
  // the unused tail of the fixed-capacity buffers: row 0 gathered, label ignored
  for (int64_t r = (int64_t)n + (int64_t)blockIdx.x * kMlmBlock + threadIdx.x; r < cap; r += (int64_t)gridDim.x * kMlmBlock) {
    p.sel[r] = 0;
    p.tgt[r] = -100;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    p.counts[0] = n;
    p.counts[1] = all - n;
    p.n_valid[0] = (float)n;
  }
}

int mlm_mask_block() { return kMlmBlock; }
int mlm_mask_blocks(int64_t N) { return (int)((N + kMlmBlock - 1) / kMlmBlock); }

void launch_mlm_mask(MlmMaskParams p, bool use_step_seed, hipStream_t st) {
  p.dev_seed = use_step_seed ? g_dropout_dev_seed : nullptr;
  const int blocks = mlm_mask_blocks(p.N);
  if (blocks == 0) return;
  hipLaunchKernelGGL(mlm_count_kernel, dim3(blocks), dim3(kMlmBlock), 0, st, p);
  HSD_CHECK_LAUNCH();
  hipLaunchKernelGGL(mlm_write_kernel, dim3(blocks), dim3(kMlmBlock), 0, st, p);
  HSD_CHECK_LAUNCH();
}

// one 16-B vector (8 bf16) per thread; vecs = N * H / 8
__global__ __launch_bounds__(256) void mlm_scatter_rows_kernel(const bf16_t* __restrict__ dx, const int* __restrict__ inv,
                                                               bf16_t* __restrict__ dh, int64_t N, int H8,
                                                               int dx_rows) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N * H8) return;
  const int64_t t = i / H8;
  const int c = (int)(i - t * H8);
  const int r = inv[t];
  u32x4 v = {0u, 0u, 0u, 0u};
  if (r >= 0 && r < dx_rows) v = reinterpret_cast<const u32x4*>(dx)[(int64_t)r * H8 + c];
  reinterpret_cast<u32x4*>(dh)[i] = v;
}

void launch_mlm_scatter_rows(const bf16_t* dx, const int* inv, bf16_t* dh, int64_t N, int H, int dx_rows,
                             hipStream_t st) {
  const int H8 = H / 8;
  const int64_t vecs = N * H8;
  if (vecs == 0) return;
  const int64_t blocks = (vecs + 255) / 256;
  hipLaunchKernelGGL(mlm_scatter_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, st, dx, inv, dh, N, H8, dx_rows);
  HSD_CHECK_LAUNCH();
}

}  // namespace hsd
