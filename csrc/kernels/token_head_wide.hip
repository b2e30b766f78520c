// Fused token-classification head for 17 .. 64 classes: the semantics of token_head.hip (dropout, classifier, CE,
// accuracy in one forward and one backward kernel plus reducers), with a split of the work of its own. The 16-class
// kernels rest on C fitting ONE 16-wide MFMA tile (one accumulator quad per row tile, W for 16 classes in 33 KB of
// LDS, the dW accumulators of all H columns in 64 registers); at C = 64 the W image is 132 KB and the dW accumulators
// would be 256 registers per lane.
//
//   forward   d       = bf16(h · keep · 1/(1-p))      the hash dropout of ops/rng.py, element (row, col) of [R, H]
//             logits  = bf16(d·Wᵀ + b)                [R, C], 17 <= C <= 64
//             per valid row, from the rounded logits: logsumexp - logits[label], first-maximum argmax hit
//             per-block partial sums -> head_stats_kernel -> stats = {mean loss, hits, n_valid, loss sum}
//   backward  g       = (softmax(logits) - onehot(label)) · dloss / max(n_valid, 1)      0 on ignored rows
//             dh      = bf16((g·W) · keep · 1/(1-p))   every element written once, 16-byte stores
//             dW, db  : fp32 partial slabs [C][H] + [C], one per ROW block -> tokw_reduce_kernel adds them in a fixed
//                       order INTO the gradient buffers (+=). No atomics, no memset: two runs give the same bits.
//   label smoothing (kSmooth instantiations, eps a host constant): the formulas of token_head.hip's header over the C
//             real classes; eps = 0 launches the <false> forms.
//
// The class dimension is padded to ng = ceil(C / 16) groups of 16 (2 .. 4); the padding classes hold zeros in the W
// images and are masked out of every softmax, sum and store. Tile = 16 consecutive rows; lane l of a wave: r = l & 15
// (row of the tile), q = l >> 4; in a 32-column slice the lane owns the 8 columns q·8 .. +7 of its row (one 16-byte
// load, one 16-byte store). A loaded (and dropped) h fragment feeds the MFMAs of ALL class groups while it is in
// registers: h is read once per kernel.
//
// Forward: a FULL W image ([16·ng][H + 8] bf16, dynamic LDS, 16.6 KB at C = 17, H = 64 up to 132,096 B at C = 64,
// H = 1,024) at ONE block per CU instead of the narrow forward's three, paid back by the block's size: up to 768
// threads, 12 waves = 3 per SIMD (the kernel is held to 168 VGPRs for that; at 1,024 threads and 128 VGPRs it
// spills), each wave walking its own row tiles. That is the narrow forward's 3 waves per SIMD with one W image, and
// LDS is what bounds it: staging W by hidden-column ranges instead would keep partial logits of every tile alive.
// The grid is persistent, at most 256 blocks; a launch with fewer than 12·256 tiles takes 8- or 4-wave blocks so that
// the tiles still spread over the CUs.
// Per slice and class group one mfma_f32_16x16x32_bf16 (A = W [class r of the group][k = 8q + j] from LDS, B = d);
// the logits come out as lane (row r, classes 16·g + 4q .. +3), so the softmax statistics cross 4 lanes (xor 16, 32).
//
// Backward: a 2-D grid. blockIdx.y is a range of 256 hidden columns, blockIdx.x a persistent row block (grid stride
// over the row tiles). dh[:, cols] = g·W[:, cols], the rebuilt d[:, cols] and dW[:, cols] += gᵀ·d[:, cols] need only
// that range of h and W: h is still read once and dh written once overall, only the logits (<= 128 B per row against
// 2·H B of h) are re-read per range, the Wᵀ image is [256][64 + 4] bf16 = 34 KB and the dW accumulators of a wave are
// 2 slices x ng groups x 8 = 64 registers. Per tile and wave w (slices w and w + 4 of the range) the data path is the
// narrow kernel's: d through a per-wave LDS tile read back transposed (ds_read_b64_tr_b16) as B of dW += gᵀ·d, g
// through a [16][64 + 4] tile the same way (A), dh = Σ_groups Wᵀ-fragment x gᵀ chained through one accumulator
// (mfma_f32_16x16x16_bf16, K = the 16 classes of a group). The next tile's h is loaded before this one is processed;
// a tile whose rows are all ignored stores zeros and skips the rest. Block (x, y) writes columns y·256 .. of slab x
// (db: y = 0), so the slabs are complete without a memset. 512 blocks (2 per CU) in all: 512 / ranges row blocks.
//
// g is rounded to bf16 for the two backward products; db sums the fp32 g. All row-by-H offsets are 64-bit.
//
// hipcc -Rpass-analysis=kernel-resource-usage (gfx950, -O3, without the packed fp32 VALU forms; C and H are run-time
// values; profiles/token_head_wide/resource_usage.txt):
//   tokw_fwd_kernel<false>   159 VGPRs, scratch 0, occupancy 3 waves / SIMD, LDS 144 B static + the W image (dynamic)
//   tokw_fwd_kernel<true>    161 VGPRs, scratch 0, occupancy 3,              LDS 144 B static + the W image  (kSmooth)
//   tokw_bwd_kernel<false>   247 VGPRs, scratch 0, occupancy 2 waves / SIMD, LDS 48,640 B
//   tokw_bwd_kernel<true>    249 VGPRs, scratch 0, occupancy 2,              LDS 48,640 B                    (kSmooth)
//   tokw_bwd_kernel<false, true> (the given-gradient entry of crf_head_wide.hip): 256 VGPRs, scratch 0, occupancy 2,
//                            LDS 48,640 B (profiles/crf_wide/resource_usage.txt; the two above are unchanged by it)
//   tokw_reduce_kernel        12 VGPRs, scratch 0
// (no AGPRs in any of them)
#include "head_common.h"
#include "launchers.h"

namespace hsd {
namespace tokw {

constexpr int TR = 16;                 // rows per tile
constexpr int GMAX = 4;                // class groups of 16
constexpr int MAXH = 1024;
constexpr int FWD_MAX_BLOCKS = 256;    // one block per CU: the W image
constexpr int FWD_MAX_WAVES = 12;      // 768 threads: 3 waves per SIMD at <= 168 VGPRs
constexpr int FWD_BATCH = 8;           // 16-byte loads of h in flight per lane
constexpr int BWD_MAX_BLOCKS = 512;    // 2 blocks per CU over both grid dimensions
constexpr int CR = 256;                // hidden columns of one backward column range
constexpr int KS = CR / 32 / 4;        // 32-column slices per wave
constexpr int WROW_PAD = 8;            // forward W image: row stride H + 8 elements
constexpr int WT_STRIDE = 16 * GMAX + 4;  // backward Wᵀ image: 64 classes + 4 elements (136 B) per column
constexpr int G_STRIDE = 16 * GMAX + 4;   // per-wave g tile: 64 classes + 4 elements per row
constexpr int D_STRIDE = 40;           // per-wave d tile: 32 columns + 8 elements (80 B) per row

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

using head::keep8;
using head::pack8;
using head::unpack8;

// the LDS tiles of the backward are written and read by ONE wave: the LDS executes a wave's instructions in order,
// so only the compiler has to keep the order
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ------------------------------------------------------------------------------------------------ forward
template <bool kSmooth>
__global__ __launch_bounds__(768) void tokw_fwd_kernel(const bf16_t* __restrict__ h, const bf16_t* __restrict__ W,
                                                        const bf16_t* __restrict__ bias,
                                                        const int64_t* __restrict__ labels,
                                                        bf16_t* __restrict__ logits, float* __restrict__ partials,
                                                        int R, int H, int C, DropoutParams dp, float eps) {
  dp = resolve_seed(dp);
  extern __shared__ __attribute__((aligned(16))) bf16_t Wimg[];  // [16·ng][H + 8]
  __shared__ float red[FWD_MAX_WAVES][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int ng = (C + 15) >> 4;
  const int wstride = H + WROW_PAD;
  const int nch = H >> 3;
  for (int idx = threadIdx.x; idx < 16 * ng * nch; idx += blockDim.x) {
    const int c = idx / nch, ch = idx - c * nch;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (c < C) v = *reinterpret_cast<const u32x4*>(W + (int64_t)c * H + ch * 8);
    *reinterpret_cast<u32x4*>(Wimg + c * wstride + ch * 8) = v;
  }
  __syncthreads();

  const bool vec4 = (C & 3) == 0;  // a lane's 4 classes of a group are one aligned 8-byte store
  const int ntiles = (R + TR - 1) / TR;
  float loss_sum = 0.f, hits = 0.f, nvalid = 0.f;
  for (int tile = blockIdx.x * nwaves + wave; tile < ntiles; tile += gridDim.x * nwaves) {
    const int row = tile * TR + r;
    const bool rvalid = row < R;
    const uint32_t rw = dropout_row((uint32_t)row, dp);
    const bf16_t* hrow = h + (int64_t)row * H;
    f32x4 acc[GMAX];
#pragma unroll
    for (int g = 0; g < GMAX; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0; s0 * 32 < H; s0 += FWD_BATCH) {
      u32x4 raw[FWD_BATCH];
#pragma unroll
      for (int u = 0; u < FWD_BATCH; ++u) {
        const int h0 = (s0 + u) * 32 + q * 8;
        raw[u] = u32x4{0u, 0u, 0u, 0u};
        if (rvalid && h0 < H) raw[u] = *reinterpret_cast<const u32x4*>(hrow + h0);
      }
#pragma unroll
      for (int u = 0; u < FWD_BATCH; ++u) {
        const int h0 = (s0 + u) * 32 + q * 8;
        if ((s0 + u) * 32 < H) {  // wave-uniform
          u32x4 d = raw[u];       // zero where the lane is outside the matrix
          if (dp.enabled) {
            float v[8], kf[8];
            unpack8(raw[u], v);
            keep8(rw, h0, dp, kf);
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] *= kf[k];
            d = pack8(v);
          }
          // A = W [class r of group g][k], B = d [k][row]: D[class 16g + 4q + reg][row r]; d feeds every group
#pragma unroll
          for (int g = 0; g < GMAX; ++g) {
            if (g < ng) {  // kernel-uniform
              u32x4 wf = {0u, 0u, 0u, 0u};
              if (h0 < H) wf = *reinterpret_cast<const u32x4*>(Wimg + (16 * g + r) * wstride + h0);
              acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf),
                                                               __builtin_bit_cast(bf16x8, d), acc[g], 0, 0, 0);
            }
          }
        }
      }
    }
    // this lane: classes 16g + 4q .. +3 of row r, rounded to the bf16 values that are stored
    float lg[GMAX][4];
#pragma unroll
    for (int g = 0; g < GMAX; ++g) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {  // (the bias: 2-byte loads that hit L1 after the first tile)
        const int c = 16 * g + 4 * q + j;
        lg[g][j] = bf2f(f2bf(acc[g][j] + (c < C ? bf2f(bias[c]) : 0.f)));
      }
      if (g < ng && rvalid) {
        const int c0 = 16 * g + 4 * q;
        bf16_t* const out = logits + (int64_t)row * C + c0;
        if (vec4) {
          if (c0 < C) *reinterpret_cast<u32x2*>(out) = u32x2{pack_bf2(lg[g][0], lg[g][1]), pack_bf2(lg[g][2], lg[g][3])};
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (c0 + j < C) out[j] = f2bf(lg[g][j]);
        }
      }
    }
    if (labels != nullptr) {  // kernel-uniform
      const int64_t lab = rvalid ? labels[row] : -100;
      const bool valid = lab >= 0 && lab < C;
      float m = -INFINITY;
      int am = 0x7fffffff;
#pragma unroll
      for (int g = 0; g < GMAX; ++g)  // ascending classes within the lane: the first maximum, as torch.argmax
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (16 * g + 4 * q + j < C && lg[g][j] > m) { m = lg[g][j]; am = 16 * g + 4 * q + j; }
#pragma unroll
      for (int o = 16; o <= 32; o <<= 1) {
        const float om = __shfl_xor(m, o, 64);
        const int oa = __shfl_xor(am, o, 64);
        if (om > m || (om == m && oa < am)) { m = om; am = oa; }
      }
      float se = 0.f, picked = 0.f, zs = 0.f;  // zs (kSmooth): Σ lg over the row's real classes
#pragma unroll
      for (int g = 0; g < GMAX; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int c = 16 * g + 4 * q + j;
          if (c < C) {
            se += __expf(lg[g][j] - m);
            if constexpr (kSmooth) zs += lg[g][j];
          }
          if (c == lab) picked = lg[g][j];
        }
#pragma unroll
      for (int o = 16; o <= 32; o <<= 1) {
        se += __shfl_xor(se, o, 64);
        picked += __shfl_xor(picked, o, 64);
        if constexpr (kSmooth) zs += __shfl_xor(zs, o, 64);
      }
      if (q == 0 && valid) {
        if constexpr (kSmooth) loss_sum += __logf(se) + m - (1.0f - eps) * picked - eps / (float)C * zs;
        else loss_sum += __logf(se) + m - picked;
        hits += am == (int)lab ? 1.f : 0.f;
        nvalid += 1.f;
      }
    }
  }
  loss_sum = wave_sum(loss_sum);
  hits = wave_sum(hits);
  nvalid = wave_sum(nvalid);
  if (lane == 0) {
    red[wave][0] = loss_sum;
    red[wave][1] = hits;
    red[wave][2] = nvalid;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int k = threadIdx.x;
    float t = red[0][k];
    for (int w = 1; w < nwaves; ++w) t += red[w][k];  // wave order: the same bits every run
    partials[(int64_t)blockIdx.x * 4 + k] = t;
  }
}

// ------------------------------------------------------------------------------------------------ backward
// this wave's slices of one tile's h rows in the block's column range: slice k is columns c0 + (wave + 4k)·32 + q·8
// .. +7 of row `row`
__device__ __forceinline__ void load_tile(const bf16_t* __restrict__ h, int tile, int ntiles, int R, int H, int c0,
                                          int wave, int r, int q, u32x4 (&raw)[KS]) {
  const int row = tile * TR + r;
  const bool ok = tile < ntiles && row < R;
#pragma unroll
  for (int k = 0; k < KS; ++k) {
    const int h0 = c0 + (wave + 4 * k) * 32 + q * 8;
    raw[k] = u32x4{0u, 0u, 0u, 0u};
    if (ok && h0 < H) raw[k] = *reinterpret_cast<const u32x4*>(h + (int64_t)row * H + h0);
  }
}

// GIVEN = false: g from the logits and the labels. GIVEN = true (launch_token_head_wide_bwd_given: the CRF head of
// crf_head_wide.hip): the caller's per-row gradient table g0 [R][C] fp32, g[row][c] = g0[row][c] · dloss · gmul /
// max(cnt[c], 1); logits, labels and stats are not read, a row of zeros in g0 is an ignored row. Everything from g on
// is the same code.
template <bool kSmooth, bool GIVEN = false>
__global__ __launch_bounds__(256, 2) void tokw_bwd_kernel(const bf16_t* __restrict__ h, const bf16_t* __restrict__ W,
                                                          const bf16_t* __restrict__ logits,
                                                          const int64_t* __restrict__ labels,
                                                          const float* __restrict__ stats,
                                                          const float* __restrict__ dloss, bf16_t* __restrict__ dh,
                                                          float* __restrict__ part, int R, int H, int C, int write_dh,
                                                          DropoutParams dp, float eps,
                                                          const float* __restrict__ g0 = nullptr,
                                                          const float* __restrict__ cnt = nullptr, float gmul = 0.f) {
  static_assert(!(GIVEN && kSmooth), "a given gradient table is not smoothed");
  dp = resolve_seed(dp);
  __shared__ __attribute__((aligned(16))) bf16_t Wt[CR * WT_STRIDE];
  __shared__ __attribute__((aligned(16))) bf16_t Dst[4][TR * D_STRIDE];
  __shared__ __attribute__((aligned(16))) bf16_t Gst[4][TR * G_STRIDE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int ng = (C + 15) >> 4;
  const int c0 = blockIdx.y * CR;     // this block's hidden columns: c0 .. c0 + cw - 1
  const int cw = min(CR, H - c0);
  // Wᵀ image of the range: Wt[col - c0][class], zeros in the padding classes. One thread: 8 columns of a class PAIR
  // (two 16-byte loads, eight 4-byte LDS stores; the pair index runs fastest over the lanes)
  const int npair = 8 * ng, nch = cw >> 3;
  for (int idx = threadIdx.x; idx < npair * nch; idx += 256) {
    const int ch = idx / npair, cp = idx - ch * npair;
    u32x4 a = {0u, 0u, 0u, 0u}, b = {0u, 0u, 0u, 0u};
    if (2 * cp < C) a = *reinterpret_cast<const u32x4*>(W + (int64_t)(2 * cp) * H + c0 + ch * 8);
    if (2 * cp + 1 < C) b = *reinterpret_cast<const u32x4*>(W + (int64_t)(2 * cp + 1) * H + c0 + ch * 8);
    const uint32_t av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
    uint32_t* const dst = reinterpret_cast<uint32_t*>(Wt + (ch * 8) * WT_STRIDE + 2 * cp);
#pragma unroll
    for (int e = 0; e < 4; ++e) {  // columns 2e, 2e + 1: {class 2cp (low half), class 2cp + 1}
      dst[(2 * e) * (WT_STRIDE / 2)] = (av[e] & 0xFFFFu) | (bv[e] << 16);
      dst[(2 * e + 1) * (WT_STRIDE / 2)] = (av[e] >> 16) | (bv[e] & 0xFFFF0000u);
    }
  }
  __syncthreads();

  float scale = 0.f, cscale[GIVEN ? GMAX : 1][4];  // GIVEN: one factor per class 16g + 4q + j of this lane
  if constexpr (GIVEN) {
#pragma unroll
    for (int g = 0; g < GMAX; ++g)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = 16 * g + 4 * q + j;
        cscale[g][j] = c < C ? dloss[0] * gmul / fmaxf(cnt[c], 1.0f) : 0.f;
      }
  } else {
    scale = dloss[0] / fmaxf(stats[2], 1.0f);
  }
  const bool vec4 = (C & 3) == 0;
  // transposed-read addresses (ds_read_b64_tr_b16): lane 4a + p of a 16-lane group supplies row a, columns 4p .. 4p+3
  // of the group's 4-row block (rows 4q .. 4q+3 of the tile); lane i of the group receives column i of those rows
  const int ta = r >> 2, tp = r & 3;
  bf16_t* const dst = Dst[wave];
  bf16_t* const gst = Gst[wave];
  const bf16_t* const g_tr = gst + (4 * q + ta) * G_STRIDE + 4 * tp;
  const lds_bf16x4* const d_tr0 = (const lds_bf16x4*)(dst + (4 * q + ta) * D_STRIDE + 4 * tp);
  const lds_bf16x4* const d_tr1 = (const lds_bf16x4*)(dst + (4 * q + ta) * D_STRIDE + 16 + 4 * tp);

  f32x4 accw[KS][GMAX][2];  // dW: classes 16g + 4q + reg, column c0 + (wave + 4k)·32 + cb·16 + r
#pragma unroll
  for (int k = 0; k < KS; ++k)
#pragma unroll
    for (int g = 0; g < GMAX; ++g) {
      accw[k][g][0] = f32x4{0.f, 0.f, 0.f, 0.f};
      accw[k][g][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  float accb[GMAX][4];  // db: classes 16g + 4q + j, this lane's row of every tile
#pragma unroll
  for (int g = 0; g < GMAX; ++g)
#pragma unroll
    for (int j = 0; j < 4; ++j) accb[g][j] = 0.f;

  const int ntiles = (R + TR - 1) / TR;
  u32x4 cur[KS];
  load_tile(h, blockIdx.x, ntiles, R, H, c0, wave, r, q, cur);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    u32x4 nxt[KS];
    load_tile(h, tile + gridDim.x, ntiles, R, H, c0, wave, r, q, nxt);
    const int row = tile * TR + r;
    const bool rvalid = row < R;
    int64_t lab = -100;
    bool valid;
    float gr[GIVEN ? GMAX : 1][4];  // GIVEN: g0 of this lane's 4 classes per group of its row
    if constexpr (GIVEN) {
      valid = false;
#pragma unroll
      for (int g = 0; g < GMAX; ++g) {
        const int cg = 16 * g + 4 * q;
#pragma unroll
        for (int j = 0; j < 4; ++j) gr[g][j] = 0.f;
        if (g < ng && rvalid) {
          const float* const in = g0 + (int64_t)row * C + cg;
          if (vec4) {
            if (cg < C) {
              const f32x4 v = *reinterpret_cast<const f32x4*>(in);
              gr[g][0] = v.x; gr[g][1] = v.y; gr[g][2] = v.z; gr[g][3] = v.w;
            }
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (cg + j < C) gr[g][j] = in[j];
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) valid = valid || gr[g][j] != 0.f;
      }
    } else {
      lab = rvalid ? labels[row] : -100;
      valid = lab >= 0 && lab < C;
    }
    if (__ballot(valid) == 0ull) {
      // every row of the tile is ignored: zeros, nothing else (the branch is wave-uniform)
      if (write_dh) {
#pragma unroll
        for (int k = 0; k < KS; ++k) {
          const int h0 = c0 + (wave + 4 * k) * 32 + q * 8;
          if (rvalid && h0 < H) *reinterpret_cast<u32x4*>(dh + (int64_t)row * H + h0) = u32x4{0u, 0u, 0u, 0u};
        }
      }
    } else {
      // g of this lane's 4 classes per group of its row
      float e[GMAX][4], m = -INFINITY, inv = 0.f;
      if constexpr (!GIVEN) {
#pragma unroll
        for (int g = 0; g < GMAX; ++g) {
          const int cg = 16 * g + 4 * q;
#pragma unroll
          for (int j = 0; j < 4; ++j) e[g][j] = -INFINITY;
          if (g < ng && rvalid) {
            const bf16_t* const in = logits + (int64_t)row * C + cg;
            if (vec4) {
              if (cg < C) {
                const u32x2 v = *reinterpret_cast<const u32x2*>(in);
                e[g][0] = lo_bf(v.x); e[g][1] = hi_bf(v.x); e[g][2] = lo_bf(v.y); e[g][3] = hi_bf(v.y);
              }
            } else {
#pragma unroll
              for (int j = 0; j < 4; ++j)
                if (cg + j < C) e[g][j] = bf2f(in[j]);
            }
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) m = fmaxf(m, e[g][j]);
        }
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        if (!rvalid) m = 0.f;
        float se = 0.f;
#pragma unroll
        for (int g = 0; g < GMAX; ++g)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            e[g][j] = __expf(e[g][j] - m);  // exp(-inf) = 0 in the padding classes
            se += e[g][j];
          }
        se += __shfl_xor(se, 16, 64);
        se += __shfl_xor(se, 32, 64);
        inv = 1.0f / se;
      }
      bf16x4 gb[GMAX];  // B operand of dh: [k = class 16g + 4q + j][n = row r]
#pragma unroll
      for (int g = 0; g < GMAX; ++g) {
        float gv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int c = 16 * g + 4 * q + j;
          if constexpr (GIVEN) gv[j] = gr[g][j] * cscale[g][j];
          else if constexpr (kSmooth)
            gv[j] = valid && c < C ? (e[g][j] * inv - (c == (int)lab ? 1.0f - eps : 0.f) - eps / (float)C) * scale : 0.f;
          else gv[j] = valid && c < C ? (e[g][j] * inv - (c == (int)lab ? 1.f : 0.f)) * scale : 0.f;
          accb[g][j] += gv[j];
        }
        const u32x2 gpk = {pack_bf2(gv[0], gv[1]), pack_bf2(gv[2], gv[3])};
        gb[g] = __builtin_bit_cast(bf16x4, gpk);
        *reinterpret_cast<u32x2*>(gst + r * G_STRIDE + 16 * g + 4 * q) = gpk;
      }
      wave_lds_fence();
      bf16x4 ga[GMAX];  // A of dW: [m = class r of group g][k = row 4q + j]
#pragma unroll
      for (int g = 0; g < GMAX; ++g) ga[g] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)(g_tr + 16 * g));
      const uint32_t rw = dropout_row((uint32_t)row, dp);
#pragma unroll
      for (int k = 0; k < KS; ++k) {
        const int s = wave + 4 * k;  // slice of the range
        if (s * 32 < cw) {           // wave-uniform
          const int h0 = c0 + s * 32 + q * 8;
          const bool ok = rvalid && h0 < H;
          float kf[8] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
          if (dp.enabled) keep8(rw, h0, dp, kf);
          u32x4 d = cur[k];  // zero outside the matrix
          if (dp.enabled) {
            float v[8];
            unpack8(cur[k], v);
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] *= kf[i];
            d = pack8(v);
          }
          *reinterpret_cast<u32x4*>(dst + r * D_STRIDE + q * 8) = d;
          wave_lds_fence();
          // dW[class][col] += Σ_row g[row][class] · d[row][col]: B = d transposed, [k = row 4q + j][n = column]
          const bf16x4 db0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)d_tr0);
          const bf16x4 db1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)d_tr1);
#pragma unroll
          for (int g = 0; g < GMAX; ++g) {
            if (g < ng) {  // kernel-uniform
              accw[k][g][0] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(ga[g], db0, accw[k][g][0], 0, 0, 0);
              accw[k][g][1] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(ga[g], db1, accw[k][g][1], 0, 0, 0);
            }
          }
          wave_lds_fence();  // the next slice overwrites the d tile
          if (write_dh) {
            // dh[row][col] = Σ_class W[class][col] · g[row][class]: A = Wᵀ fragment [m][k = class 16g + 4q + j] with
            // output row m = 4a + b of MFMA t standing for column s·32 + a·8 + t·4 + b, so that a lane (output rows
            // 4q .. 4q+3) collects the 8 consecutive columns s·32 + q·8 .. +7 of its row from t = 0, 1; the class
            // groups chain through the accumulator
            float o[8];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
              const int col = s * 32 + (r >> 2) * 8 + t * 4 + (r & 3);  // of the range
              f32x4 od = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
              for (int g = 0; g < GMAX; ++g) {
                if (g < ng) {
                  u32x2 wa = {0u, 0u};
                  if (col < cw) wa = *reinterpret_cast<const u32x2*>(Wt + col * WT_STRIDE + 16 * g + 4 * q);
                  od = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(bf16x4, wa), gb[g], od, 0, 0, 0);
                }
              }
#pragma unroll
              for (int i = 0; i < 4; ++i) o[4 * t + i] = od[i] * kf[4 * t + i];
            }
            if (ok) *reinterpret_cast<u32x4*>(dh + (int64_t)row * H + h0) = pack8(o);
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < KS; ++k) cur[k] = nxt[k];
  }

  // this row block's partial slab, [C][H] then [C]: the columns of this block's range (db from the first range)
  float* const slab = part + (int64_t)blockIdx.x * ((int64_t)C * H + C);
#pragma unroll
  for (int k = 0; k < KS; ++k)
#pragma unroll
    for (int g = 0; g < GMAX; ++g)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
        const int col = c0 + (wave + 4 * k) * 32 + cb * 16 + r;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int c = 16 * g + 4 * q + i;
          if (c < C && col < H) slab[(int64_t)c * H + col] = accw[k][g][cb][i];
        }
      }
  if (blockIdx.y == 0 && wave == 0) {  // every wave holds the same g: one sums db over the tile rows (lanes r = 0 .. 15)
#pragma unroll
    for (int g = 0; g < GMAX; ++g)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float v = accb[g][j];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
        const int c = 16 * g + 4 * q + j;
        if (r == 0 && c < C) slab[(int64_t)C * H + c] = v;
      }
  }
}

// dW (then db) += the nblk partial slabs (the layout and the order of token_head.hip's tok_reduce_kernel, which is
// local to its file). RED_X outputs x RED_G groups of consecutive slabs per workgroup; a group's slabs are added in
// slab order and the group sums in group order: the same bits every run.
constexpr int RED_X = 16, RED_G = 16;
__global__ __launch_bounds__(256) void tokw_reduce_kernel(const float* __restrict__ part, int nblk, int n, int nw,
                                                          float* __restrict__ dW, float* __restrict__ db) {
  __shared__ float red[RED_G][RED_X];
  const int x = threadIdx.x % RED_X, grp = threadIdx.x / RED_X;
  const int e = blockIdx.x * RED_X + x;
  const int per = (nblk + RED_G - 1) / RED_G;
  const int b0 = grp * per, b1 = min(nblk, b0 + per);
  float s = 0.f;
  if (e < n)
    for (int b = b0; b < b1; ++b) s += part[(int64_t)b * n + e];
  red[grp][x] = s;
  __syncthreads();
  if (grp == 0 && e < n) {
    float t = red[0][x];
#pragma unroll
    for (int k = 1; k < RED_G; ++k) t += red[k][x];
    float* const dst = e < nw ? dW + e : db + (e - nw);
    *dst += t;
  }
}

static void launch_reduce(const float* part, int nblk, int H, int C, float* dW, float* db, hipStream_t st) {
  const int n = C * H + C;
  hipLaunchKernelGGL(tokw_reduce_kernel, dim3((n + RED_X - 1) / RED_X), dim3(RED_X * RED_G), 0, st, part, nblk, n,
                     C * H, dW, db);
  HSD_CHECK_LAUNCH();
}

// waves per forward block: the fewest of 4 / 8 / 12 with which the tiles fit FWD_MAX_BLOCKS blocks (12 beyond that)
static int fwd_waves(int ntiles) {
  for (int w = 4; w < FWD_MAX_WAVES; w += 4)
    if ((ntiles + w - 1) / w <= FWD_MAX_BLOCKS) return w;
  return FWD_MAX_WAVES;
}

}  // namespace tokw

int token_head_wide_fwd_blocks(int R) {
  const int ntiles = (R + tokw::TR - 1) / tokw::TR;
  const int w = tokw::fwd_waves(ntiles);
  return std::max(1, std::min((ntiles + w - 1) / w, tokw::FWD_MAX_BLOCKS));
}

int64_t token_head_wide_fwd_lds(int H, int C) {
  return (int64_t)16 * ((C + 15) / 16) * (H + tokw::WROW_PAD) * (int64_t)sizeof(bf16_t);
}

int token_head_wide_bwd_blocks(int R, int H) {
  const int ntiles = (R + tokw::TR - 1) / tokw::TR;
  const int ranges = (H + tokw::CR - 1) / tokw::CR;
  return std::max(1, std::min(ntiles, tokw::BWD_MAX_BLOCKS / ranges));
}

void launch_token_head_wide_fwd(const bf16_t* h, const bf16_t* W, const bf16_t* b, const int64_t* labels,
                                bf16_t* logits, float* partials, float* stats, int R, int H, int C, double p,
                                uint64_t seed, hipStream_t st, float label_smoothing) {
  const int nblk = token_head_wide_fwd_blocks(R);
  const int threads = 64 * tokw::fwd_waves((R + tokw::TR - 1) / tokw::TR);
  const size_t lds = (size_t)token_head_wide_fwd_lds(H, C);
  const DropoutParams dp = make_dropout(p, seed);
  const bool smooth = labels != nullptr && label_smoothing > 0.f;
  auto* const kern = smooth ? tokw::tokw_fwd_kernel<true> : tokw::tokw_fwd_kernel<false>;
  static bool raised[2] = {false, false};  // beyond the default 64 KB of dynamic LDS: once per instantiation
  if (!raised[smooth]) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)token_head_wide_fwd_lds(tokw::MAXH, 16 * tokw::GMAX));
    raised[smooth] = true;
  }
  hipLaunchKernelGGL(kern, dim3(nblk), dim3(threads), lds, st, h, W, b, labels, logits, partials, R, H, C, dp,
                     smooth ? label_smoothing : 0.f);
  HSD_CHECK_LAUNCH();
  if (labels != nullptr) launch_head_stats(partials, nblk, stats, st);
}

void launch_token_head_wide_bwd(const bf16_t* h, const bf16_t* W, const bf16_t* logits, const int64_t* labels,
                                const float* stats, const float* dloss, bf16_t* dh, float* part, float* dW, float* db,
                                int R, int H, int C, double p, uint64_t seed, hipStream_t st, float label_smoothing) {
  const int nblk = token_head_wide_bwd_blocks(R, H);
  const dim3 grid(nblk, (H + tokw::CR - 1) / tokw::CR);
  const DropoutParams dp = make_dropout(p, seed);
  if (label_smoothing > 0.f)
    hipLaunchKernelGGL(tokw::tokw_bwd_kernel<true>, grid, dim3(256), 0, st, h, W, logits, labels, stats, dloss, dh, part,
                       R, H, C, dh != nullptr ? 1 : 0, dp, label_smoothing);
  else
    hipLaunchKernelGGL(tokw::tokw_bwd_kernel<false>, grid, dim3(256), 0, st, h, W, logits, labels, stats, dloss, dh,
                       part, R, H, C, dh != nullptr ? 1 : 0, dp, 0.f);
  HSD_CHECK_LAUNCH();
  tokw::launch_reduce(part, nblk, H, C, dW, db, st);
}

void launch_token_head_wide_bwd_given(const bf16_t* h, const bf16_t* W, const float* g0, const float* cnt, float gmul,
                                      const float* dloss, bf16_t* dh, float* part, float* dW, float* db, int R, int H,
                                      int C, double p, uint64_t seed, hipStream_t st) {
  const int nblk = token_head_wide_bwd_blocks(R, H);
  const dim3 grid(nblk, (H + tokw::CR - 1) / tokw::CR);
  hipLaunchKernelGGL((tokw::tokw_bwd_kernel<false, true>), grid, dim3(256), 0, st, h, W, (const bf16_t*)nullptr,
                     (const int64_t*)nullptr, (const float*)nullptr, dloss, dh, part, R, H, C, dh != nullptr ? 1 : 0,
                     make_dropout(p, seed), 0.f, g0, cnt, gmul);
  HSD_CHECK_LAUNCH();
  tokw::launch_reduce(part, nblk, H, C, dW, db, st);
}

}  // namespace hsd
