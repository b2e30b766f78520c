// Linear-chain CRF head for 17 .. 64 tags: the definition, arguments and outputs of crf_head.hip (em [R][C] bf16, cu,
// labels / keep, theta = {trans, start, end}, pred, g0, per-sequence slabs, stats / cnt / dtheta), with a split of the
// work of its own. The narrow kernels hold all C x C tag pairs in ONE wave, four transition scores per lane; at C = 64
// that would be 64 scores per lane and 64 dependent exponentials per chain step.
//
// The class dimension is padded to NG = ceil(C / 16) groups of 16 (2 .. 4, a template parameter). Padding tags carry
// the large negative FINITE score NEG everywhere (never -inf: nothing can form inf - inf) and are clamped back to NEG
// after every step.
//
// Work split: ONE WORKGROUP OF NG WAVES per sequence. Lane j of EVERY wave is tag j (lanes >= C are padding); wave w owns
// the group 16w .. 16w+15 of the OTHER tag, and each lane keeps its 16 transition scores in registers for the whole
// sequence (forward: trans[16w+k][j], predecessors of j; marginals: trans[j][16w+k], successors of j). So the C x C
// pairs are spread over 64·NG lanes x 16 registers, and a chain step costs each lane 16 exponentials whatever C is.
//
// One chain step (forward): after the previous step every wave holds alpha[j] (and the Viterbi delta[j]) in lane j,
// so wave w reads its 16 inputs alpha[16w+k] with 16 v_readlane into SGPRs: uniform operands, no LDS, no bpermute.
// Per lane, over its 16 predecessors: the partial (max, Σ exp) and, in the same loop on the same sums, the partial
// Viterbi (max, first argmax). The NG partial records of a tag go through an LDS table [2][NG][64] of 16-byte records
// (8 KB) with ONE __syncthreads per step: step t writes buffer t & 1, every wave reads all NG records after the barrier,
// and buffer t & 1 is written again only at step t + 2, which lies behind the barrier of t + 1 that no wave passes
// before every wave has read step t. Every wave combines the records REDUNDANTLY in the fixed order w = 0 .. NG-1:
// all waves then hold the same bits (no broadcast needed), and a tie keeps the smaller tag. Everything is in log space
// (a scaled probability-space recursion would underflow to log 0 on tables with large negative forbidden
// transitions): alpha is stored centred by its maximum over the 64 lanes (four DPP row steps + the permlane16 /
// permlane32 swaps), logZ and the gold score are compensated sums.
//
// Uniform trip count: every wave derives the chain from the same labels (64-row chunks, one label per lane, ballot,
// scalar bit scan), so all waves of a workgroup execute the same number of barriers; no wave leaves early, and an
// empty chain runs zero steps in all of them.
//
// Staging: a chunk's emissions are its 64·C contiguous bf16 values (<= 8 KB), copied as they are (no re-layout: row
// r, tag j is element r·C + j); the waves split the loads. The next chunk is fetched into registers before the current
// one is consumed and committed to the other LDS buffer after it; the marginals kernel stages the stored alphas the
// same way. Nothing of O(sequence length) lives in LDS: any length runs.
//
// Back-pointers: u8 [R][16·NG] in the workspace (64 bytes per row do not fit the narrow kernel's registers-plus-
// v_readlane trick). The back-trace stages one chunk of them (<= 4 KB, one coalesced 16-byte load per thread, double
// buffered in the emissions' LDS) and wave 0 walks it with LDS reads: no dependent global load per step.
//
//   crfw_fwd_kernel<NG, GOLD>  alpha + Viterbi in one loop; wave 0 stores the centred alpha [R][16·NG] fp32 and
//            accumulates logZ - score(gold); wave 1 stores the back-pointers; back-trace; pred [R]; the record
//            {nll, chain rows, hits}. GOLD = false: decode only.
//   crfw_marg_kernel<NG>  the beta recursion backwards over the re-derived chain, each row normalised by its own
//            Z_t = lse_i(alpha_t[i] + beta_t[i]). The exponentials exp(x_k - m) of the beta step's partial sums are
//            kept and reused for the pair expectations: exp(alpha_t[i] + x_k - Z_t) = exp(x_k - m) · exp(alpha_t[i] + m
//            - Z_t), one more exponential per lane instead of 16 (both factors are <= 1: nothing overflows, and a
//            factor that underflows belongs to a pair marginal below 1e-38). Pair expectations minus gold counts
//            accumulate in 16 registers per lane laid out like the transitions; one slab [C·C + 2C] per sequence;
//            every element of g0 written once.
//   crfw_reduce_kernel  ceil(P / 256) workgroups of 1,024 threads: 256 elements x 4 ranges of consecutive slabs; a
//            thread adds its range into four independent sums (slab index mod 4, so four loads are in flight)
//            combined as (s0 + s1) + (s2 + s3), the four ranges are added in range order. Workgroup 0 also sums the
//            records -> stats, and N broadcast into cnt [64] (what launch_token_head_wide_bwd_given divides by).
//
// No atomics, no memset, one writer per output element: two runs give the same bits, and a padded and a packed form of
// the same batch give the same bits sequence by sequence.
//
// hipcc -Rpass-analysis=kernel-resource-usage (gfx950, -O3, without the packed fp32 VALU forms):
// profiles/crf_wide/resource_usage.txt (scratch 0 everywhere)
#include "common.h"
#include "launchers.h"

namespace hsd {
namespace crfw {

constexpr int CH = 64;         // rows per chunk: one label per lane
constexpr int CMAX = 64;       // tags, at most
constexpr float NEG = -1e30f;  // the score of a padding tag

__device__ __forceinline__ float dpp_row_mirror(float v) {  // lane l <- lane 15-l within each 16-lane row
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x140, 0xF, 0xF, false));
}
// max / sum over the 64 lanes: four DPP steps inside each 16-lane row, then the permlane16 / permlane32 swaps across the
// rows (each swap of v with itself returns both partners); every lane gets the result, the same bits in all of them
__device__ __forceinline__ float wmax(float v) {
  v = fmaxf(v, dpp_xor1(v));
  v = fmaxf(v, dpp_xor2(v));
  v = fmaxf(v, dpp_half_mirror(v));
  v = fmaxf(v, dpp_row_mirror(v));
  auto p = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return max_xor32(fmaxf(__uint_as_float(p[0]), __uint_as_float(p[1])));
}
__device__ __forceinline__ float wsum(float v) {
  v += dpp_xor1(v);
  v += dpp_xor2(v);
  v += dpp_half_mirror(v);
  v += dpp_row_mirror(v);
  auto p = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return sum_xor32(__uint_as_float(p[0]) + __uint_as_float(p[1]));
}
// lane `src` (wave-uniform) of v as a scalar
__device__ __forceinline__ float lane_of(float v, int src) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

// compensated (Kahan) running sum: logZ and the gold score grow with the chain, their difference is what is wanted
struct Kahan {
  float s = 0.f, c = 0.f;
  __device__ __forceinline__ void add(float v) {
#pragma clang fp reassociate(off)
    const float y = v - c;
    const float t = s + y;
    c = (t - s) - y;
    s = t;
  }
};

// the segment of sequence b, clamped to the buffer (nothing below indexes outside [0, R) whatever cu holds)
__device__ __forceinline__ void segment(const int* __restrict__ cu, int b, int R, int& start, int& stop) {
  start = min(max(cu[b], 0), R);
  stop = min(max(cu[b + 1], start), R);
}

// this lane's label of row `row` as an int: the tag on a chain row, -1 elsewhere
__device__ __forceinline__ int chain_label(const int64_t* __restrict__ labels, const int64_t* __restrict__ keep, int row,
                                           int stop, int C) {
  if (row >= stop) return -1;
  if (labels != nullptr) {
    const int64_t l = labels[row];
    return l >= 0 && l < C ? (int)l : -1;
  }
  return keep == nullptr || keep[row] != 0 ? 0 : -1;
}

// the chunk's emissions: element it·T + tid of its (rows in the sequence)·C contiguous bf16 values, T = 64·NG threads;
// 16 elements per thread cover 64·C for every C <= 16·NG
template <int NG>
__device__ __forceinline__ void fetch_em(const bf16_t* __restrict__ em, int r0, int stop, int C, bf16_t ev[16]) {
  const int lim = min(CH, stop - r0) * C;
#pragma unroll
  for (int it = 0; it < 16; ++it) {
    const int idx = it * (64 * NG) + (int)threadIdx.x;
    ev[it] = 0;
    if (idx < lim) ev[it] = em[(int64_t)r0 * C + idx];
  }
}
template <int NG>
__device__ __forceinline__ void commit_em(bf16_t* sE, const bf16_t ev[16]) {
#pragma unroll
  for (int it = 0; it < 16; ++it) sE[it * (64 * NG) + (int)threadIdx.x] = ev[it];  // < 16·64·NG <= CH·CMAX
}

template <int NG, bool GOLD>
__global__ __launch_bounds__(64 * NG) void crfw_fwd_kernel(const bf16_t* __restrict__ em, const int* __restrict__ cu,
                                                           const int64_t* __restrict__ labels,
                                                           const int64_t* __restrict__ keep,
                                                           const float* __restrict__ theta,
                                                           float* __restrict__ ws_alpha, uint8_t* __restrict__ ws_bp,
                                                           int* __restrict__ pred, float* __restrict__ rec, int R, int B,
                                                           int C) {
  constexpr int T = 64 * NG, CPW = 16 * NG;
  __shared__ __attribute__((aligned(16))) bf16_t sE[2][CH * CMAX];  // emissions; then the back-pointer chunks
  __shared__ __attribute__((aligned(16))) f32x4 sX[2][NG][64];       // {max, Σ exp, Viterbi max, its argmax}
  __shared__ float sT[GOLD ? CMAX * CMAX : 1];                       // trans [C][C], for the gold score
  __shared__ float sS[64], sEn[64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int start, stop;
  segment(cu, b, R, start, stop);
  const int nch = (stop - start + CH - 1) / CH;

  if (GOLD)
    for (int idx = tid; idx < C * C; idx += T) sT[idx] = theta[idx];
  if (tid < 64) {
    sS[tid] = tid < C ? theta[C * C + tid] : NEG;
    sEn[tid] = tid < C ? theta[C * C + C + tid] : NEG;
  }
  float tr[16];  // trans[16w+k][lane]: the predecessors of tag `lane` in this wave's group
#pragma unroll
  for (int k = 0; k < 16; ++k) tr[k] = lane < C && 16 * w + k < C ? theta[(16 * w + k) * C + lane] : NEG;
  const int jc = min(lane, C - 1);  // a padding lane reads a real tag's emission and is clamped afterwards

  float ah = NEG, dh = NEG;  // alpha / delta of tag `lane` (centred), the same bits in every wave
  int n = 0, yprev = 0;
  Kahan nll;

  bf16_t ev[16];
  int labv = -1, labn = -1;
  if (nch > 0) {
    labv = chain_label(labels, keep, start + lane, stop, C);
    fetch_em<NG>(em, start, stop, C, ev);
    commit_em<NG>(sE[0], ev);
  }
  __syncthreads();
  for (int c = 0; c < nch; ++c) {
    const int buf = c & 1, r0 = start + c * CH;
    if (c + 1 < nch) {  // the next chunk flies under this one's recursion
      labn = chain_label(labels, keep, r0 + CH + lane, stop, C);
      fetch_em<NG>(em, r0 + CH, stop, C, ev);
    }
    uint64_t mask = __ballot(labv >= 0);
    while (mask) {
      const int r = __ffsll((unsigned long long)mask) - 1;
      mask &= mask - 1;
      const int y = __builtin_amdgcn_readlane(labv, r);
      const int64_t row = r0 + r;
      const float ej = bf2f(sE[buf][r * C + jc]);
      float v, vd;
      int bi = 0;
      if (n == 0) {
        v = vd = sS[lane] + ej;
      } else {
        float x[16];
        float m = -INFINITY, best = -INFINITY;
        int bk = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          x[k] = lane_of(ah, 16 * w + k) + tr[k];
          m = fmaxf(m, x[k]);
          const float t = lane_of(dh, 16 * w + k) + tr[k];
          if (t > best) { best = t; bk = k; }  // strict: the first maximum
        }
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) s += __expf(x[k] - m);
        sX[n & 1][w][lane] = f32x4{m, s, best, __int_as_float(16 * w + bk)};
        __syncthreads();
        f32x4 q[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) q[g] = sX[n & 1][g][lane];
        float M = q[0].x;
#pragma unroll
        for (int g = 1; g < NG; ++g) M = fmaxf(M, q[g].x);
        float S = 0.f;
        best = q[0].z;
        bi = __float_as_int(q[0].w);
#pragma unroll
        for (int g = 0; g < NG; ++g) {  // group order: the same bits in every wave, a tie keeps the smaller tag
          S += q[g].y * __expf(q[g].x - M);
          if (g > 0 && q[g].z > best) { best = q[g].z; bi = __float_as_int(q[g].w); }
        }
        v = M + __logf(S) + ej;
        vd = best + ej;
      }
      v = lane < C ? v : NEG;
      vd = lane < C ? vd : NEG;
      // (the cross-lane reductions stay outside the selects: every lane must take part in them)
      const float cmax = wmax(v), dmax = wmax(vd);
      ah = lane < C ? v - cmax : NEG;
      dh = lane < C ? vd - dmax : NEG;
      if (GOLD && w == 0) {
        if (lane < CPW) ws_alpha[row * CPW + lane] = ah;
        const float tg = n == 0 ? sS[y] : sT[yprev * C + y];
        nll.add(cmax - tg - bf2f(sE[buf][r * C + y]));
      }
      if (w == 1 && lane < CPW) ws_bp[row * CPW + lane] = (uint8_t)bi;
      yprev = y;
      ++n;
    }
    if (c + 1 < nch) {
      labv = labn;
      commit_em<NG>(sE[buf ^ 1], ev);
    }
    __syncthreads();
  }

  // the last chain row: logZ's tail and the best final tag (first maximum)
  float nll_seq = 0.f;
  int cur = 0;
  if (n > 0) {
    if (GOLD) {
      const float fin = ah + sEn[lane];
      const float m = wmax(fin);
      nll_seq = nll.s + (m + __logf(wsum(__expf(fin - m))) - sEn[yprev]);
    }
    float bv = dh + sEn[lane];
    int bidx = lane;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bidx, o, 64);
      if (ov > bv || (ov == bv && oi < bidx)) { bv = ov; bidx = oi; }
    }
    cur = __builtin_amdgcn_readfirstlane(bidx) & 63;
  }

  // back-trace, last chunk first. A chunk's back-pointers are 64·CPW = 16·T bytes: one 16-byte load per thread (thread
  // tid: row r0 + tid / NG), double buffered in the LDS of the emissions (all waves are past the loop's last barrier);
  // wave 0 walks them.
  __threadfence();  // the back-pointer bytes wave 1 stored are read back by every wave
  __syncthreads();
  uint8_t* const sB = reinterpret_cast<uint8_t*>(&sE[0][0]);  // [2][CH·CPW] <= 8 KB of the 16 KB
  auto fetch_bp = [&](int r0) {
    u32x4 v = u32x4{0u, 0u, 0u, 0u};
    if (r0 + tid / NG < stop) v = *reinterpret_cast<const u32x4*>(ws_bp + (int64_t)r0 * CPW + 16 * tid);
    return v;
  };
  if (nch > 0)
    *reinterpret_cast<u32x4*>(sB + ((nch - 1) & 1) * (CH * CPW) + 16 * tid) = fetch_bp(start + (nch - 1) * CH);
  int hits = 0;
  for (int c = nch - 1; c >= 0; --c) {
    const int buf = c & 1, r0 = start + c * CH, row = r0 + lane;
    __syncthreads();
    u32x4 nx;
    if (c > 0) nx = fetch_bp(r0 - CH);
    if (w == 0) {
      const int lv = chain_label(labels, keep, row, stop, C);
      const uint8_t* const bp = sB + buf * (CH * CPW);
      int mine = -1;
      uint64_t mask = __ballot(lv >= 0);
      while (mask) {
        const int r = 63 - __clzll((unsigned long long)mask);
        mask &= ~(1ull << r);
        if (lane == r) mine = cur;
        cur = min(__builtin_amdgcn_readfirstlane((int)bp[r * CPW + cur]), CPW - 1);
      }
      if (row < stop) pred[row] = mine;
      if (GOLD) hits += __popcll(__ballot(lv >= 0 && mine == lv));
    }
    if (c > 0) *reinterpret_cast<u32x4*>(sB + (buf ^ 1) * (CH * CPW) + 16 * tid) = nx;
  }
  if (b == 0)  // the rows outside every sequence
    for (int row = tid; row < start; row += T) pred[row] = -1;
  if (b == B - 1)
    for (int row = stop + tid; row < R; row += T) pred[row] = -1;
  if (GOLD && tid == 0) *reinterpret_cast<f32x4*>(rec + 4 * (int64_t)b) = f32x4{nll_seq, (float)n, (float)hits, 0.f};
}

template <int NG>
__global__ __launch_bounds__(64 * NG) void crfw_marg_kernel(const bf16_t* __restrict__ em, const int* __restrict__ cu,
                                                            const int64_t* __restrict__ labels,
                                                            const float* __restrict__ theta,
                                                            const float* __restrict__ ws_alpha, float* __restrict__ g0,
                                                            float* __restrict__ slab, int R, int B, int C) {
  constexpr int T = 64 * NG, CPW = 16 * NG;
  __shared__ __attribute__((aligned(16))) bf16_t sE[2][CH * CMAX];
  __shared__ __attribute__((aligned(16))) float sA[2][CH * CPW];
  __shared__ __attribute__((aligned(8))) f32x2 sX[2][NG][64];  // {max, Σ exp}
  __shared__ float sEn[64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int start, stop;
  segment(cu, b, R, start, stop);
  const int nch = (stop - start + CH - 1) / CH;

  if (tid < 64) sEn[tid] = tid < C ? theta[C * C + C + tid] : NEG;
  float trT[16];  // trans[lane][16w+k]: the successors of tag `lane` in this wave's group
#pragma unroll
  for (int k = 0; k < 16; ++k) trT[k] = lane < C && 16 * w + k < C ? theta[lane * C + 16 * w + k] : NEG;
  const int ic = min(lane, C - 1), ia = min(lane, CPW - 1);

  float u = NEG;  // tag `lane`: em[t+1] + beta[t+1] - Z_{t+1}, the same bits in every wave
  float acc[16];  // Σ_t pair marginal (lane, 16w+k) - gold count
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.f;
  float dend = 0.f, g_last = 0.f;  // tag `lane`: marginal - onehot on the last / the most recent chain row
  int n = 0, ynext = 0;

  bf16_t ev[16];
  f32x4 av[4];
  int labv = -1, labn = -1;
  // chunk c's alphas: 64 rows x CPW floats are 4·T float4, four per thread (rows off the chain hold workspace junk that
  // is never used)
  auto fetch_alpha = [&](int r0) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int f = it * T + tid;
      av[it] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (r0 + f / (4 * NG) < stop) av[it] = *reinterpret_cast<const f32x4*>(ws_alpha + (int64_t)r0 * CPW + 4 * f);
    }
  };
  auto commit = [&](int buf) {
    commit_em<NG>(sE[buf], ev);
#pragma unroll
    for (int it = 0; it < 4; ++it) *reinterpret_cast<f32x4*>(&sA[buf][4 * (it * T + tid)]) = av[it];
  };
  if (nch > 0) {
    const int r0 = start + (nch - 1) * CH;
    labv = chain_label(labels, nullptr, r0 + lane, stop, C);
    fetch_em<NG>(em, r0, stop, C, ev);
    fetch_alpha(r0);
    commit((nch - 1) & 1);
  }
  __syncthreads();
  for (int c = nch - 1; c >= 0; --c) {
    const int buf = c & 1, r0 = start + c * CH;
    if (c > 0) {
      labn = chain_label(labels, nullptr, r0 - CH + lane, stop, C);
      fetch_em<NG>(em, r0 - CH, stop, C, ev);
      fetch_alpha(r0 - CH);
    }
    uint64_t mask = __ballot(labv >= 0);
    // exact zeros on the chunk's rows off the chain (every row of g0 has one writer)
    const int lim = min(CH, stop - r0) * C;
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int idx = it * T + tid;
      if (idx < lim && !((mask >> (idx / C)) & 1ull)) g0[(int64_t)r0 * C + idx] = 0.f;
    }
    while (mask) {
      const int r = 63 - __clzll((unsigned long long)mask);
      mask &= ~(1ull << r);
      const int y = __builtin_amdgcn_readlane(labv, r);
      const int64_t row = r0 + r;
      const float ei = bf2f(sE[buf][r * C + ic]);
      const float ah = lane < C ? sA[buf][r * CPW + ia] : NEG;
      float bcur, m = 0.f;
      float p[16];
      if (n == 0) {
        bcur = sEn[lane];
      } else {
        float x[16];
        m = -INFINITY;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          x[k] = trT[k] + lane_of(u, 16 * w + k);
          m = fmaxf(m, x[k]);
        }
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          p[k] = __expf(x[k] - m);
          s += p[k];
        }
        sX[n & 1][w][lane] = f32x2{m, s};
        __syncthreads();
        f32x2 q[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) q[g] = sX[n & 1][g][lane];
        float M = q[0].x;
#pragma unroll
        for (int g = 1; g < NG; ++g) M = fmaxf(M, q[g].x);
        float S = 0.f;
#pragma unroll
        for (int g = 0; g < NG; ++g) S += q[g].y * __expf(q[g].x - M);
        bcur = lane < C ? M + __logf(S) : NEG;
      }
      const float la = ah + bcur;
      const float zm = wmax(la);
      const float z = zm + __logf(wsum(__expf(la - zm)));
      const float g = __expf(la - z) - (lane == y ? 1.f : 0.f);
      if (n == 0) {
        dend = g;
      } else {
        const float sc = __expf(ah + m - z);  // exp(alpha + x_k - Z) = exp(x_k - m) · sc
        const int kg = lane == y ? ynext - 16 * w : -1;
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[k] += p[k] * sc - (k == kg ? 1.f : 0.f);
      }
      if (w == 0 && lane < C) g0[row * C + lane] = g;
      u = lane < C ? ei + (bcur - z) : NEG;
      g_last = g;
      ynext = y;
      ++n;
    }
    if (c > 0) {
      labv = labn;
      commit(buf ^ 1);
    }
    __syncthreads();
  }
  if (b == 0)
    for (int64_t e = tid; e < (int64_t)start * C; e += T) g0[e] = 0.f;
  if (b == B - 1)
    for (int64_t e = (int64_t)stop * C + tid; e < (int64_t)R * C; e += T) g0[e] = 0.f;

  float* const sl = slab + (int64_t)b * (C * C + 2 * C);
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (lane < C && 16 * w + k < C) sl[lane * C + 16 * w + k] = acc[k];
  if (w == 0 && lane < C) {
    sl[C * C + lane] = n > 0 ? g_last : 0.f;  // the walk ends on the first chain row
    sl[C * C + C + lane] = dend;
  }
}

// Σ over the sequences in a fixed order. Thread (x, grp) of workgroup k: element k·256 + x, the grp-th quarter of the
// slabs.
constexpr int RED_X = 256, RED_G = 4;
__global__ __launch_bounds__(RED_X * RED_G) void crfw_reduce_kernel(const float* __restrict__ rec,
                                                                    const float* __restrict__ slab, int B, int P,
                                                                    float* __restrict__ stats, float* __restrict__ cnt,
                                                                    float* __restrict__ dtheta) {
  __shared__ float red[3][RED_X * RED_G];
  const int t = threadIdx.x;
  if (slab != nullptr) {
    const int x = t % RED_X, grp = t / RED_X, e = blockIdx.x * RED_X + x;
    const int per = (B + RED_G - 1) / RED_G;
    const int b0 = grp * per, b1 = min(B, b0 + per);
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    if (e < P) {
      int bb = b0;
      for (; bb + 4 <= b1; bb += 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] += slab[(int64_t)(bb + i) * P + e];
      }
      for (int i = 0; bb + i < b1; ++i) s[i] += slab[(int64_t)(bb + i) * P + e];
    }
    red[0][t] = (s[0] + s[1]) + (s[2] + s[3]);
    __syncthreads();
    if (grp == 0 && e < P) {
      float v = red[0][x];
#pragma unroll
      for (int k = 1; k < RED_G; ++k) v += red[0][k * RED_X + x];
      dtheta[e] = v;
    }
    __syncthreads();
  }
  if (blockIdx.x != 0) return;
  // the records: thread t takes sequences t, t + 1024, ... in increasing order, then a fixed tree
  float s[3] = {0.f, 0.f, 0.f};
  for (int b = t; b < B; b += RED_X * RED_G) {
    const f32x4 r = *reinterpret_cast<const f32x4*>(rec + 4 * (int64_t)b);
    s[0] += r.x;
    s[1] += r.y;
    s[2] += r.z;
  }
#pragma unroll
  for (int f = 0; f < 3; ++f) red[f][t] = s[f];
  __syncthreads();
  for (int o = RED_X * RED_G / 2; o > 0; o >>= 1) {
    if (t < o) {
#pragma unroll
      for (int f = 0; f < 3; ++f) red[f][t] += red[f][t + o];
    }
    __syncthreads();
  }
  const float lsum = red[0][0], nrows = red[1][0], hits = red[2][0];
  if (t < CMAX) cnt[t] = nrows;
  if (t == 0) {
    stats[0] = lsum / fmaxf(nrows, 1.0f);
    stats[1] = hits;
    stats[2] = nrows;
    stats[3] = lsum;
  }
}

template <int NG>
static void launch_fwd(const bf16_t* em, const int* cu, const int64_t* labels, const int64_t* keep, const float* theta,
                       float* ws_alpha, uint8_t* ws_bp, int* pred, float* rec, int R, int B, int C, hipStream_t st) {
  if (labels != nullptr)
    hipLaunchKernelGGL((crfw_fwd_kernel<NG, true>), dim3(B), dim3(64 * NG), 0, st, em, cu, labels, keep, theta, ws_alpha,
                       ws_bp, pred, rec, R, B, C);
  else
    hipLaunchKernelGGL((crfw_fwd_kernel<NG, false>), dim3(B), dim3(64 * NG), 0, st, em, cu, labels, keep, theta,
                       ws_alpha, ws_bp, pred, rec, R, B, C);
}

}  // namespace crfw

void launch_crf_wide_forward(const bf16_t* em, const int* cu, const int64_t* labels, const int64_t* keep,
                             const float* theta, float* ws_alpha, uint8_t* ws_bp, int* pred, float* rec, int R, int B,
                             int C, hipStream_t st) {
  const int ng = (C + 15) / 16;
  if (ng == 2) crfw::launch_fwd<2>(em, cu, labels, keep, theta, ws_alpha, ws_bp, pred, rec, R, B, C, st);
  else if (ng == 3) crfw::launch_fwd<3>(em, cu, labels, keep, theta, ws_alpha, ws_bp, pred, rec, R, B, C, st);
  else crfw::launch_fwd<4>(em, cu, labels, keep, theta, ws_alpha, ws_bp, pred, rec, R, B, C, st);
  HSD_CHECK_LAUNCH();
}

void launch_crf_wide_marginals(const bf16_t* em, const int* cu, const int64_t* labels, const float* theta,
                               const float* ws_alpha, float* g0, float* slab, int R, int B, int C, hipStream_t st) {
  const int ng = (C + 15) / 16;
  auto* const kern = ng == 2 ? crfw::crfw_marg_kernel<2> : ng == 3 ? crfw::crfw_marg_kernel<3> : crfw::crfw_marg_kernel<4>;
  hipLaunchKernelGGL(kern, dim3(B), dim3(64 * ng), 0, st, em, cu, labels, theta, ws_alpha, g0, slab, R, B, C);
  HSD_CHECK_LAUNCH();
}

void launch_crf_wide_reduce(const float* rec, const float* slab, int B, int C, float* stats, float* cnt, float* dtheta,
                            hipStream_t st) {
  const int P = C * C + 2 * C;
  const int grid = slab != nullptr ? (P + crfw::RED_X - 1) / crfw::RED_X : 1;  // without slabs: the records alone
  hipLaunchKernelGGL(crfw::crfw_reduce_kernel, dim3(grid), dim3(crfw::RED_X * crfw::RED_G), 0, st, rec, slab, B, P,
                     stats, cnt, dtheta);
  HSD_CHECK_LAUNCH();
}

}  // namespace hsd
