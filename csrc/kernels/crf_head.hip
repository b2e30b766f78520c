// Linear-chain CRF head of --task token-classification --crf true (BERT-CRF): the sequence log-likelihood, its
// gradients and the Viterbi path over the per-token scores of token_head.hip's classifier pass.
//
//   em [R][C] bf16     the emissions (tok_fwd_kernel in its logits-only mode), 2 <= C <= 16
//   cu int32 [B+1]     sequence b = rows cu[b] .. cu[b+1]-1 (padded batches: arange(B+1)·S)
//   labels int64 [R]   the CHAIN of a sequence = its rows with 0 <= label < C, in order; every other row is stepped
//                      over. Without labels (decode only) the chain is the rows with keep[row] != 0 (all rows if null).
//   theta fp32         {trans [C][C] (trans[i][j]: tag i followed by tag j), start [C], end [C]}, one packed vector
//
// Work split: the recursion is sequential along the chain and parallel only over the C x C tag pairs, so ONE WAVE
// (a 64-thread workgroup) owns one sequence. The lanes form a 16 x 4 grid: lane = 16 q + j holds tag j and the quarter
// q of the OTHER tag (tags 4q .. 4q+3); its four transition scores live in registers for the whole sequence
// (forward: trans[4q+k][j], predecessors of j; backward: trans[j][4q+k], successors of j). Tags >= C carry the large
// negative FINITE score NEG everywhere (never -inf: nothing can form inf - inf), and are clamped back to NEG after
// every step so the padding cannot drift.
//
// One chain step (forward): x_k = alpha[4q+k] + trans[4q+k][j]; max and Σ exp over k in registers, then across q, i.e.
// across the four 16-lane rows, on the gfx950 permlane16 / permlane32 swaps (no LDS traffic); the new alpha[j] then sits
// in lane j of every row and is re-centred by its row maximum (four DPP steps), so the stored alpha is <= 0 with maximum
// 0 and the sequence's log-partition is carried separately as a compensated sum of the per-step maxima. The Viterbi
// delta rides in the same loop on (max, first argmax) pairs with the same exchanges and shares the loads.
//
// The hand-off (the step's critical path): lane (j, q) next needs alpha[4q .. 4q+3], which sit in lanes 4q .. 4q+3 of its
// own row. It is done with ds_bpermute (four __shfl per recursion). Why not the alternatives: DPP on gfx9 has no
// row_share / arbitrary in-row broadcast (only quad permutes, shifts, rotates and mirrors), so "lane 4q+k of my row"
// is not one DPP op; an LDS round trip is a write, a wait, and four reads with a second wait, where the four
// bpermutes are issued back to back, use no LDS allocation and retire under ONE lgkmcnt wait.
//
// Rows are walked in 64-row chunks: one lane loads one label, a wave ballot gives the chunk's chain rows and the wave
// iterates over the set bits (scalar bit scans). The next chunk's emissions (and, in the backward pass, alphas) are
// fetched into registers before the current chunk is consumed and committed to the other LDS buffer after it, so the
// global loads fly under the recursion. Nothing of O(sequence length) lives in LDS: any length runs.
//
//   crf_fwd_kernel<GOLD>  alpha + Viterbi delta in one loop; stores the centred alpha [R][16] fp32 and the
//            back-pointers [R][16] u8 at chain rows; accumulates logZ - score(gold) (compensated); back-traces on the
//            device from the last chain row (the chunk's back-pointer rows sit in registers, one lane per row, and are
//            read with v_readlane: no dependent memory load per step); writes pred [R] (int32 tag, -1 off the chain)
//            and the record {nll, chain rows, hits}. GOLD = false: decode only (no alpha store, no record).
//   crf_marg_kernel   the beta recursion backwards over the same chain, RE-DERIVED from the labels chunk by chunk in
//            reverse (no compacted index: nothing else to store or to keep in step with kernel 1). Each row's marginal
//            is normalised by its own log-sum-exp Z_t = lse_i(alpha_t[i] + beta_t[i]), which is also the normaliser of
//            the pair expectations of the step (t, t+1): no drift with the chain length and logZ is never subtracted
//            from large numbers. Writes every row of g0 [R][C] once (marginal - onehot; exact zeros off the chain and
//            on the rows outside every sequence); accumulates the pair expectations minus the gold counts in
//            registers laid out like the transitions; writes the sequence's slab [C·C + 2C] = {dtrans, dstart, dend}.
//   crf_reduce_kernel one workgroup: records and slabs summed over the sequences in a fixed order ->
//            stats {mean loss, hits, N, loss sum}, N broadcast into cnt [16] (what launch_token_head_bwd_given divides
//            by) and the UNSCALED parameter gradients dtheta (the op's backward scales by dloss / max(N, 1)).
//
// No atomics, no memset, one writer per output element: two runs give the same bits, and a padded and a packed form of
// the same batch give the same bits (a sequence's result depends on its chain alone).
//
// hipcc -Rpass-analysis=kernel-resource-usage (gfx950, -O3): profiles/crf/resource_usage.txt (scratch 0 everywhere)
#include "common.h"
#include "launchers.h"

namespace hsd {
namespace crf {

constexpr int CP = 16;        // tags, padded
constexpr int CH = 64;        // rows per chunk: one label per lane
constexpr float NEG = -1e30f;  // the score of a padding tag

__device__ __forceinline__ float dpp_row_mirror(float v) {  // lane l <- lane 15-l within each 16-lane row
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x140, 0xF, 0xF, false));
}
// max / sum over each 16-lane row; every lane gets its row's result, and the same bits in all 16 lanes (both partners of
// an exchange compute the same commutative operation)
__device__ __forceinline__ float row_max(float v) {
  v = fmaxf(v, dpp_xor1(v));
  v = fmaxf(v, dpp_xor2(v));
  v = fmaxf(v, dpp_half_mirror(v));
  return fmaxf(v, dpp_row_mirror(v));
}
__device__ __forceinline__ float row_sum(float v) {
  v += dpp_xor1(v);
  v += dpp_xor2(v);
  v += dpp_half_mirror(v);
  return v + dpp_row_mirror(v);
}
// reductions across the four rows (lane l with l^16, then l^32): each swap of v with itself returns in every lane the
// pair {even row's value, odd row's value} (permlane16) / {lower half's, upper half's} (permlane32)
__device__ __forceinline__ float rows_max(float v) {
  auto p = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = fmaxf(__uint_as_float(p[0]), __uint_as_float(p[1]));
  return max_xor32(v);
}
__device__ __forceinline__ float rows_sum(float v) {
  auto p = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = __uint_as_float(p[0]) + __uint_as_float(p[1]);
  return sum_xor32(v);
}
// (max, first argmax) across the four rows: element 0 of each swap belongs to the row / half with the smaller tags, so a
// tie keeps it
__device__ __forceinline__ void rows_argmax(float& v, int& idx) {
  auto pv = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  auto pi = __builtin_amdgcn_permlane16_swap((uint32_t)idx, (uint32_t)idx, false, false);
  bool hi = __uint_as_float(pv[1]) > __uint_as_float(pv[0]);
  v = __uint_as_float(hi ? pv[1] : pv[0]);
  idx = (int)(hi ? pi[1] : pi[0]);
  pv = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  pi = __builtin_amdgcn_permlane32_swap((uint32_t)idx, (uint32_t)idx, false, false);
  hi = __uint_as_float(pv[1]) > __uint_as_float(pv[0]);
  v = __uint_as_float(hi ? pv[1] : pv[0]);
  idx = (int)(hi ? pi[1] : pi[0]);
}
// the hand-off: lane (j, q) <- the values of tags 4q .. 4q+3 (lanes 4q+k; every row holds the same 16 values)
__device__ __forceinline__ void hand_off(float v, int q, float out[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) out[k] = __shfl(v, 4 * q + k, 64);
}
__device__ __forceinline__ float max4(const float x[4]) { return fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])); }

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

// trans / start / end of theta as padded LDS tables (NEG in the padding)
__device__ __forceinline__ void load_theta(const float* __restrict__ theta, int C, float* sT, float* sS, float* sEn) {
  const int lane = threadIdx.x;
  for (int idx = lane; idx < CP * CP; idx += 64) {
    const int i = idx >> 4, j = idx & 15;
    sT[idx] = i < C && j < C ? theta[i * C + j] : NEG;
  }
  if (lane < CP) {
    sS[lane] = lane < C ? theta[C * C + lane] : NEG;
    sEn[lane] = lane < C ? theta[C * C + C + lane] : NEG;
  }
}

// this lane's label of chunk row r0 + lane as an int: the tag on a chain row, -1 elsewhere
__device__ __forceinline__ int chain_label(const int64_t* __restrict__ labels, const int64_t* __restrict__ keep, int row,
                                           int stop, int C) {
  if (row >= stop) return -1;
  if (labels != nullptr) {
    const int64_t l = labels[row];
    return l >= 0 && l < C ? (int)l : -1;
  }
  return keep == nullptr || keep[row] != 0 ? 0 : -1;
}

// the chunk's emissions: element it·64 + lane of its 64·C contiguous bf16 values (coalesced), as raw words
__device__ __forceinline__ void fetch_em(const bf16_t* __restrict__ em, int r0, int stop, int C, bf16_t ev[CP]) {
  const int lane = threadIdx.x;
#pragma unroll
  for (int it = 0; it < CP; ++it) {
    ev[it] = 0;
    const int idx = it * 64 + lane;
    if (it < C && r0 + idx / C < stop) ev[it] = em[(int64_t)r0 * C + idx];
  }
}
__device__ __forceinline__ void commit_em(float* sE, int C, const bf16_t ev[CP]) {
  const int lane = threadIdx.x;
#pragma unroll
  for (int it = 0; it < CP; ++it) {
    const int idx = it * 64 + lane, rr = idx / C;
    if (it < C) sE[rr * CP + (idx - rr * C)] = bf2f(ev[it]);
  }
}

template <bool GOLD>
__global__ __launch_bounds__(64) void crf_fwd_kernel(const bf16_t* __restrict__ em, const int* __restrict__ cu,
                                                     const int64_t* __restrict__ labels,
                                                     const int64_t* __restrict__ keep, const float* __restrict__ theta,
                                                     float* __restrict__ ws_alpha, uint8_t* __restrict__ ws_bp,
                                                     int* __restrict__ pred, float* __restrict__ rec, int R, int B,
                                                     int C) {
  __shared__ float sE[2][CH * CP];
  __shared__ int sL[2][CH];
  __shared__ float sT[CP * CP], sS[CP], sEn[CP];
  const int b = blockIdx.x, lane = threadIdx.x, j = lane & 15, q = lane >> 4;
  int start, stop;
  segment(cu, b, R, start, stop);
  const int nch = (stop - start + CH - 1) / CH;

  load_theta(theta, C, sT, sS, sEn);
  for (int idx = lane; idx < 2 * CH * CP; idx += 64) (&sE[0][0])[idx] = NEG;  // the padding tags' columns stay NEG
  __syncthreads();
  float tr[4];  // trans[4q+k][j]: the predecessors of tag j
#pragma unroll
  for (int k = 0; k < 4; ++k) tr[k] = sT[(4 * q + k) * CP + j];

  float a[4], dl[4];        // alpha / delta of tags 4q+k (centred)
  float ah = NEG, dh = NEG;  // ... of tag j
  int n = 0, yprev = 0;
  Kahan nll;

  bf16_t ev[CP];
  int lab = -1;
  if (nch > 0) {
    lab = chain_label(labels, keep, start + lane, stop, C);
    fetch_em(em, start, stop, C, ev);
    sL[0][lane] = lab;
    commit_em(sE[0], C, ev);
  }
  __syncthreads();
  for (int c = 0; c < nch; ++c) {
    const int buf = c & 1, r0 = start + c * CH;
    if (c + 1 < nch) {  // the next chunk flies under this one's recursion
      lab = chain_label(labels, keep, r0 + CH + lane, stop, C);
      fetch_em(em, r0 + CH, stop, C, ev);
    }
    const int labv = sL[buf][lane];
    uint64_t mask = __ballot(labv >= 0);
    while (mask) {
      const int r = __ffsll((unsigned long long)mask) - 1;
      mask &= mask - 1;
      const int y = __builtin_amdgcn_readlane(labv, r);
      const int64_t row = r0 + r;
      const float ej = sE[buf][r * CP + j];
      float v, vd, tg;
      int bi = 0;
      if (n == 0) {
        v = vd = sS[j] + ej;
        tg = sS[y];
      } else {
        float x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = a[k] + tr[k];
        const float m = rows_max(max4(x));
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) s += __expf(x[k] - m);
        v = m + __logf(rows_sum(s)) + ej;
        float best = dl[0] + tr[0];
        bi = 4 * q;
#pragma unroll
        for (int k = 1; k < 4; ++k) {
          const float t = dl[k] + tr[k];
          if (t > best) { best = t; bi = 4 * q + k; }
        }
        rows_argmax(best, bi);
        vd = best + ej;
        tg = sT[yprev * CP + y];
      }
      v = j < C ? v : NEG;
      vd = j < C ? vd : NEG;
      // (the cross-lane reductions stay outside the selects: every lane of the row must take part in them)
      const float cmax = row_max(v), dmax = row_max(vd);
      ah = j < C ? v - cmax : NEG;
      dh = j < C ? vd - dmax : NEG;
      if (q == 0) {
        if (GOLD) ws_alpha[row * CP + j] = ah;
        ws_bp[row * CP + j] = (uint8_t)bi;
      }
      hand_off(ah, q, a);
      hand_off(dh, q, dl);
      if (GOLD) nll.add(cmax - tg - sE[buf][r * CP + y]);
      yprev = y;
      ++n;
    }
    if (c + 1 < nch) {
      sL[buf ^ 1][lane] = lab;
      commit_em(sE[buf ^ 1], C, ev);
    }
    __syncthreads();
  }

  // the last chain row: logZ's tail and the best final tag (first maximum)
  float nll_seq = 0.f;
  int cur = 0;
  if (n > 0) {
    if (GOLD) {
      const float fin = ah + sEn[j];
      const float m = row_max(fin);
      nll_seq = nll.s + (m + __logf(row_sum(__expf(fin - m))) - sEn[yprev]);
    }
    float bv = dh + sEn[j];
    int bidx = j;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bidx, o, 64);
      if (ov > bv || (ov == bv && oi < bidx)) { bv = ov; bidx = oi; }
    }
    cur = __builtin_amdgcn_readfirstlane(bidx) & 15;
  }

  // back-trace, last chunk first: lane l holds the 16 back-pointers of row r0 + l
  __threadfence();  // the back-pointer bytes this wave stored are read back below
  int hits = 0;
  for (int c = nch - 1; c >= 0; --c) {
    const int r0 = start + c * CH, row = r0 + lane;
    const int labv = chain_label(labels, keep, row, stop, C);
    u32x4 bp = u32x4{0u, 0u, 0u, 0u};
    if (labv >= 0) bp = *reinterpret_cast<const u32x4*>(ws_bp + (int64_t)row * CP);
    int mine = -1;
    uint64_t mask = __ballot(labv >= 0);
    while (mask) {
      const int r = 63 - __clzll((unsigned long long)mask);
      mask &= ~(1ull << r);
      const int cw = cur >> 2;
      const uint32_t w = cw == 0 ? bp.x : cw == 1 ? bp.y : cw == 2 ? bp.z : bp.w;
      const uint32_t wv = (uint32_t)__builtin_amdgcn_readlane((int)w, r);
      if (lane == r) mine = cur;
      cur = (wv >> (8 * (cur & 3))) & 15;
    }
    if (row < stop) pred[row] = mine;
    if (GOLD) hits += __popcll(__ballot(labv >= 0 && mine == labv));
  }
  if (b == 0)  // the rows outside every sequence
    for (int row = lane; row < start; row += 64) pred[row] = -1;
  if (b == B - 1)
    for (int row = stop + lane; row < R; row += 64) pred[row] = -1;
  if (GOLD && lane == 0)
    *reinterpret_cast<f32x4*>(rec + 4 * (int64_t)b) = f32x4{nll_seq, (float)n, (float)hits, 0.f};
}

__global__ __launch_bounds__(64) void crf_marg_kernel(const bf16_t* __restrict__ em, const int* __restrict__ cu,
                                                      const int64_t* __restrict__ labels,
                                                      const float* __restrict__ theta,
                                                      const float* __restrict__ ws_alpha, float* __restrict__ g0,
                                                      float* __restrict__ slab, int R, int B, int C) {
  __shared__ float sE[2][CH * CP];
  __shared__ __attribute__((aligned(16))) float sA[2][CH * CP];
  __shared__ int sL[2][CH];
  __shared__ float sT[CP * CP], sS[CP], sEn[CP];
  const int b = blockIdx.x, lane = threadIdx.x, i = lane & 15, q = lane >> 4;
  int start, stop;
  segment(cu, b, R, start, stop);
  const int nch = (stop - start + CH - 1) / CH;

  load_theta(theta, C, sT, sS, sEn);
  for (int idx = lane; idx < 2 * CH * CP; idx += 64) (&sE[0][0])[idx] = NEG;
  __syncthreads();
  float trT[4];  // trans[i][4q+k]: the successors of tag i
#pragma unroll
  for (int k = 0; k < 4; ++k) trT[k] = sT[i * CP + 4 * q + k];

  float x[4] = {NEG, NEG, NEG, NEG};   // trans[i][j] + em[t+1][j] + beta[t+1][j], j = 4q+k
  float acc[4] = {0.f, 0.f, 0.f, 0.f};  // Σ_t pair marginal (i, 4q+k) - gold count
  float dend = 0.f, g_last = 0.f;       // tag i: marginal - onehot on the last / the most recent chain row
  int n = 0, ynext = 0;

  bf16_t ev[CP];
  f32x4 av[4];
  int lab = -1;
  // chunk c's alphas: the 64 rows x 16 floats are 256 float4, four per lane (rows off the chain hold workspace junk that
  // is never used)
  auto fetch_alpha = [&](int r0) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int f = it * 64 + lane;
      av[it] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (r0 + (f >> 2) < stop) av[it] = *reinterpret_cast<const f32x4*>(ws_alpha + (int64_t)r0 * CP + 4 * f);
    }
  };
  auto commit = [&](int buf) {
    sL[buf][lane] = lab;
    commit_em(sE[buf], C, ev);
#pragma unroll
    for (int it = 0; it < 4; ++it) *reinterpret_cast<f32x4*>(&sA[buf][4 * (it * 64 + lane)]) = av[it];
  };
  if (nch > 0) {
    const int r0 = start + (nch - 1) * CH;
    lab = chain_label(labels, nullptr, r0 + lane, stop, C);
    fetch_em(em, r0, stop, C, ev);
    fetch_alpha(r0);
    commit((nch - 1) & 1);
  }
  __syncthreads();
  for (int c = nch - 1; c >= 0; --c) {
    const int buf = c & 1, r0 = start + c * CH;
    if (c > 0) {
      lab = chain_label(labels, nullptr, r0 - CH + lane, stop, C);
      fetch_em(em, r0 - CH, stop, C, ev);
      fetch_alpha(r0 - CH);
    }
    const int labv = sL[buf][lane];
    uint64_t mask = __ballot(labv >= 0);
    // exact zeros on the chunk's rows off the chain (every row of g0 has one writer)
#pragma unroll
    for (int it = 0; it < CP; ++it) {
      const int idx = it * 64 + lane, rr = idx / C;
      if (it < C && r0 + rr < stop && !((mask >> rr) & 1ull)) g0[(int64_t)r0 * C + idx] = 0.f;
    }
    while (mask) {
      const int r = 63 - __clzll((unsigned long long)mask);
      mask &= ~(1ull << r);
      const int y = __builtin_amdgcn_readlane(labv, r);
      const int64_t row = r0 + r;
      const float ei = sE[buf][r * CP + i], ah = sA[buf][r * CP + i];
      float bcur;
      if (n == 0) {
        bcur = sEn[i];
      } else {
        const float m = rows_max(max4(x));
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) s += __expf(x[k] - m);
        const float lse = m + __logf(rows_sum(s));
        bcur = i < C ? lse : NEG;
      }
      const float la = ah + bcur;
      const float zm = row_max(la);
      const float z = zm + __logf(row_sum(__expf(la - zm)));
      const float g = __expf(la - z) - (i == y ? 1.f : 0.f);
      if (n == 0) {
        dend = g;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          acc[k] += __expf(ah + x[k] - z) - (i == y && 4 * q + k == ynext ? 1.f : 0.f);
      }
      if (q == 0 && i < C) g0[row * C + i] = g;
      const float u = i < C ? ei + (bcur - z) : NEG;
      float uk[4];
      hand_off(u, q, uk);
#pragma unroll
      for (int k = 0; k < 4; ++k) x[k] = trT[k] + uk[k];
      g_last = g;
      ynext = y;
      ++n;
    }
    if (c > 0) commit(buf ^ 1);
    __syncthreads();
  }
  if (b == 0)
    for (int64_t e = lane; e < (int64_t)start * C; e += 64) g0[e] = 0.f;
  if (b == B - 1)
    for (int64_t e = (int64_t)stop * C + lane; e < (int64_t)R * C; e += 64) g0[e] = 0.f;

  float* const sl = slab + (int64_t)b * (C * C + 2 * C);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (i < C && 4 * q + k < C) sl[i * C + 4 * q + k] = acc[k];
  if (q == 0 && i < C) {
    sl[C * C + i] = n > 0 ? g_last : 0.f;  // the walk ends on the first chain row
    sl[C * C + C + i] = dend;
  }
}

// Σ over the sequences in a fixed order: thread t takes sequences t, t+256, ... in increasing order, then a fixed tree
__global__ __launch_bounds__(256) void crf_reduce_kernel(const float* __restrict__ rec, const float* __restrict__ slab,
                                                         int B, int P, float* __restrict__ stats,
                                                         float* __restrict__ cnt, float* __restrict__ dtheta) {
  __shared__ float red[3][256];
  const int t = threadIdx.x;
  float s[3] = {0.f, 0.f, 0.f};
  for (int b = t; b < B; b += 256) {
    const f32x4 r = *reinterpret_cast<const f32x4*>(rec + 4 * (int64_t)b);
    s[0] += r.x;
    s[1] += r.y;
    s[2] += r.z;
  }
#pragma unroll
  for (int f = 0; f < 3; ++f) red[f][t] = s[f];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
#pragma unroll
      for (int f = 0; f < 3; ++f) red[f][t] += red[f][t + o];
    }
    __syncthreads();
  }
  const float lsum = red[0][0], nrows = red[1][0], hits = red[2][0];
  if (t < CP) cnt[t] = nrows;
  if (t == 0) {
    stats[0] = lsum / fmaxf(nrows, 1.0f);
    stats[1] = hits;
    stats[2] = nrows;
    stats[3] = lsum;
  }
  if (slab != nullptr) {
    for (int p = t; p < P; p += 256) {
      float v = 0.f;
      for (int b = 0; b < B; ++b) v += slab[(int64_t)b * P + p];
      dtheta[p] = v;
    }
  }
}

}  // namespace crf

void launch_crf_forward(const bf16_t* em, const int* cu, const int64_t* labels, const int64_t* keep, const float* theta,
                        float* ws_alpha, uint8_t* ws_bp, int* pred, float* rec, int R, int B, int C, hipStream_t st) {
  if (labels != nullptr)
    hipLaunchKernelGGL(crf::crf_fwd_kernel<true>, dim3(B), dim3(64), 0, st, em, cu, labels, keep, theta, ws_alpha, ws_bp,
                       pred, rec, R, B, C);
  else
    hipLaunchKernelGGL(crf::crf_fwd_kernel<false>, dim3(B), dim3(64), 0, st, em, cu, labels, keep, theta, ws_alpha,
                       ws_bp, pred, rec, R, B, C);
  HSD_CHECK_LAUNCH();
}

void launch_crf_marginals(const bf16_t* em, const int* cu, const int64_t* labels, const float* theta,
                          const float* ws_alpha, float* g0, float* slab, int R, int B, int C, hipStream_t st) {
  hipLaunchKernelGGL(crf::crf_marg_kernel, dim3(B), dim3(64), 0, st, em, cu, labels, theta, ws_alpha, g0, slab, R, B, C);
  HSD_CHECK_LAUNCH();
}

void launch_crf_reduce(const float* rec, const float* slab, int B, int C, float* stats, float* cnt, float* dtheta,
                       hipStream_t st) {
  hipLaunchKernelGGL(crf::crf_reduce_kernel, dim3(1), dim3(256), 0, st, rec, slab, B, C * C + 2 * C, stats, cnt, dtheta);
  HSD_CHECK_LAUNCH();
}

}  // namespace hsd
