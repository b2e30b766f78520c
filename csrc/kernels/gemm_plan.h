// Host-side launch policy of the MFMA GEMMs (gemm2.hip bf16, gemm8 fp8): which kernel runs for a shape, on which tile,
// with how many K-splits and how much slab workspace. One planning function per entry point returns a GemmPlan; the
// launchers (gemm2.hip) execute it and the bindings size their workspaces from it. Pure functions: no HIP includes, no
// device query (the CU count is an argument), so the policy is testable on a machine without a GPU (_C.gemm_plan,
// tests/test_gemm_plan.py).
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "knobs.h"

#ifdef __HIP__
#define HSD_PLAN_HD __attribute__((host)) __attribute__((device))
#else
#define HSD_PLAN_HD
#endif

namespace hsd {

// E2_BIAS_GELU_D: C = gelu'(y), C2 = gelu(y) (y = acc + bias) — the FFN1 forward keeps the GELU DERIVATIVE
// for backward, so the FFN2 dgrad epilogue is a plain product (E2_MUL: C = bf16(acc) * aux) instead of
// re-evaluating erf/exp per element.
// E2_STORE_RDOT: C = bf16(acc), plus the attention backward's delta rows rd[(b·heads + h)·S + s] = Σ_{64 columns of head h}
// C·aux over row m = b·S + s (aux = the attention output O, heads = N / 64): the out-projection dgrad writes dO AND the
// row dots the streaming attention backward would otherwise recompute in a separate pass (re-reading dO and O)
enum Epi2 : int { E2_STORE = 0, E2_BIAS = 1, E2_BIAS_GELU = 2, E2_BIAS_DROP_RES = 3, E2_RES = 4, E2_DGELU = 5,
                  E2_F32_ATOMIC = 6, E2_F32_SLAB = 7, E2_BIAS_GELU_D = 8, E2_MUL = 9, E2_STORE_RDOT = 10 };

HSD_PLAN_HD constexpr bool epi_bias(int e) { return e == E2_BIAS || e == E2_BIAS_GELU || e == E2_BIAS_DROP_RES || e == E2_BIAS_GELU_D; }
HSD_PLAN_HD constexpr bool epi_aux(int e) {
  return e == E2_BIAS_DROP_RES || e == E2_RES || e == E2_DGELU || e == E2_MUL || e == E2_STORE_RDOT;
}
HSD_PLAN_HD constexpr bool epi_two_out(int e) { return e == E2_BIAS_GELU || e == E2_BIAS_GELU_D; }
HSD_PLAN_HD constexpr bool epi_bf16_out(int e) {
  return e <= E2_DGELU || e == E2_BIAS_GELU_D || e == E2_MUL || e == E2_STORE_RDOT;
}
// fused bias-gradient column sums (dbias): 8 columns per lane, BN 256 only
constexpr bool epi_fused_dbias(int e) { return e == E2_DGELU || e == E2_MUL; }
// fp8 output copies: the FFN epilogues whose outputs feed the next fp8 GEMM (GELU -> FFN2 forward, GELU'
// product -> FFN1 dgrad)
constexpr bool epi_q8_copy(int e) { return e == E2_BIAS_GELU_D || e == E2_BIAS_GELU || e == E2_MUL || e == E2_DGELU; }

// every bf16-output epilogue, for the launch switches: X(E) per epilogue
#define HSD_BF16_EPIS(X)                                                                                          \
  X(E2_STORE) X(E2_BIAS) X(E2_BIAS_GELU) X(E2_BIAS_DROP_RES) X(E2_RES) X(E2_DGELU) X(E2_BIAS_GELU_D) X(E2_MUL) \
  X(E2_STORE_RDOT)

enum GemmKernel : int {
  GK_NONE = 0,  // unsupported
  GK_G2,        // gemm2_kernel<LA, LB, EPI, BN, SYNC, SEG>: 256-row tiles, one tile (x K-split) per workgroup
  GK_G2PK,      // gemm2pk_kernel<EPI, BN>: persistent NT
  GK_G2S,       // gemm2s_kernel<LA, LB, EPI, NSTG, KW, SEG>: 128 x 128 tiles
  GK_G8PK,      // gemm8pk_kernel<EPI, BN, FA, 0, Q8>: persistent fp8 NT
  GK_G8TT,      // gemm8tt_kernel<FA, 0>: fp8 weight gradient
};

// how the main kernel's result reaches C
enum GemmLanding : int {
  GL_STORE = 0,     // the kernel writes C
  GL_ACCUM,         // the kernel adds into C in place (every element has one owner)
  GL_ATOMIC,        // fp32 atomics into C
  GL_SLABS_ASSIGN,  // fp32 slabs in the workspace, then slab_reduce_kernel: C = Σ slabs
  GL_SLABS_ADD,     // ... C += Σ slabs
  GL_SLABS_EPI,     // ... then splitk_epi_kernel<out_epi>: C = epilogue(Σ slabs)
};

struct GemmPlan {
  int kernel = GK_NONE;
  // template choices of the main kernel (those its family has)
  int la = 0, lb = 0, epi = 0, bn = 256, sync = 4, nstg = 2, kw = 1, fa = 0;
  bool seg = false, q8 = false;
  // G2Params fields and the launch
  int kps = 0;     // K elements per split
  int splits = 1;  // slabs actually launched
  int tiles_n = 0, ntiles = 0, grid = 0, wg = 512;
  int landing = GL_STORE;
  bool accum_flag = false;  // G2Params::accum_direct
  int out_epi = 0;          // GL_SLABS_EPI: the epilogue pass
  int M = 0, N = 0;         // the reduce / epilogue pass's shape
  int64_t ws_numel = 0;     // fp32 workspace elements (0: none)

  bool supported() const { return kernel != GK_NONE; }
  bool slabs() const { return landing >= GL_SLABS_ASSIGN; }
};

namespace plan {

constexpr int kBM = 256, kBK = 64, kSBM = 128, kSBN = 128;  // g2::BM / BK / SBM / SBN

struct KSplit {
  int kps, real;
};
// `splits` requested over K in K-tiles of `bk`: the K elements per split and the number of splits actually launched
inline KSplit k_split(int K, int splits, int bk = kBK) {
  if (splits < 1) splits = 1;
  int kps = (K + splits - 1) / splits;
  kps = (kps + bk - 1) / bk * bk;
  return KSplit{kps, (K + kps - 1) / kps};
}

// Main-loop schedule (interleaved rounds in one process, random operands, T = 131072 tokens): the staggered 4-phase
// form (SYNC 4) is the fastest on both layouts. NT (forward / dgrad): +5-10 % over one-barrier-per-K-tile SYNC 1 on
// every BERT shape (tools/gemm_probe.py, profiles/gemm_probe_r1_sync.json). TT (weight gradients), once its LDS-DMA
// stopped draining every K-tile (dma_lds_asm): 1,018-1,134 TFLOP/s vs 920-1,065 for SYNC 7 and 979-1,074 for SYNC 0
// on the four bert-base weights (tools/tt_probe.py, profiles/tt_probe_r3_sync_splits.json). HSD_G2_SYNC overrides
// for A/B runs; the bf16 epilogue stores are non-temporal (st16nt).
inline int g2_sync_mode() {
  const int e = HSD_KNOB("HSD_G2_SYNC", kKnobUnset);
  const int m = e != kKnobUnset ? e : 4;
  return (m == 1 || m == 2 || m == 4 || m == 5 || m == 6 || m == 7) ? m : 0;  // any other value: SYNC 0
}

// Persistent NT kernel (gemm2pk_kernel): for grids of more than one round of workgroups (a one-round grid has no tile
// seam to hide). Measured on the bert-base B=1024 NT GEMMs (tools/env_ab_gemm.py, profiles/persist_ab_r3.log): 1-6 %
// faster on every one, bit-identical outputs; the headline step 80.8 -> 79.3 ms. HSD_G2_PERSIST=0 turns it off.
inline bool g2_persist(int tiles, int cus) {
  if (!HSD_KNOB("HSD_G2_PERSIST", 1)) return false;
  return tiles > (cus & ~7);
}

// Tile width for a bf16-output NT GEMM: minimise (rounds of 256 CUs) x (per-tile cost ∝ BN + c).
inline int gemm2_pick_bn(int M, int N) {
  const int tm = (M + 255) / 256;
  int best = 0;
  double best_cost = 1e30;
  for (int bn : {256, 192}) {
    if (N % bn) continue;
    const int blocks = tm * (N / bn);
    const int rounds = (blocks + 255) / 256;
    const double cost = rounds * (bn + 64.0);
    if (cost < best_cost) { best_cost = cost; best = bn; }
  }
  return best;
}

// gemm2s (128 x 128 tiles) for NT grids that 256 x 256 tiles leave mostly idle. HSD_G2_SMALL=0 disables,
// =1 forces it for every shape it supports.
inline bool gemm2s_use(int M, int N, int K) {
  if (N % kSBN != 0 || K % 64 != 0) return false;
  const int e = HSD_KNOB("HSD_G2_SMALL", kKnobUnset);
  if (e != kKnobUnset) return e != 0;
  // long K (>= 16,384: the MLM head's dgrad over the ~50k-word table): the 256 x 256 kernel with K-splits filling the
  // CUs beats 128 x 128 tiles at one split -- 4,928 x 1,024 x 50,432: 446 us at 3 splits vs 770 us
  // (tools/mlm_dgrad_probe.py, profiles/mlm_dgrad_probe_r4.jsonl)
  if (K >= 16384) return false;
  const int tiles = ((M + 255) / 256) * ((N + 255) / 256);
  return tiles * 2 <= 256;
}

// K-splits for a bf16-output NT GEMM. A 256 x 256 tile grid that leaves more than half of the 256 CUs idle
// (the reference's own per-rank batch: bert-large, B = 8, S = 512 -> M = 4096: 64 tiles on the H-wide GEMMs)
// is split over K into fp32 slabs plus one reduce-and-epilogue pass, keeping >= 8 K-tiles per split.
// HSD_G2_SPLITK=0 disables, =n forces n.
inline int gemm2_nt_splits(int M, int N, int K) {
  const int e = HSD_KNOB("HSD_G2_SPLITK", kKnobUnset);
  const int kt = K / 64;
  if (e != kKnobUnset) return std::max(1, std::min(e, kt));
  if (gemm2s_use(M, N, K)) {
    // 128 x 128 tiles: split only grids that leave more than half of the CUs idle (serving batches: B = 1 has 6-24
    // tiles, each a latency-bound chain of 12-48 K-steps), >= 2 K-tiles per split
    const int tiles = ((M + 127) / 128) * (N / 128);
    if (tiles * 2 > 256) return 1;
    int s = 256 / tiles;
    while (s > 1 && kt / s < 2) --s;
    return s;
  }
  const int tiles = ((M + 255) / 256) * ((N + 255) / 256);
  if (tiles * 2 > 256) return 1;
  int s = 256 / tiles;
  while (s > 1 && kt / s < 8) --s;
  return s;
}

// Weight-gradient plan: 256 x 256 tiles (gemm2, split-K slabs) or 128 x 128 tiles (gemm2s TT), and the K-split
// count, by a cost model fitted to tools/wgrad_ab.py on MI355X (24 BERT shapes x T = 4096 / 8192 / 16384; it
// picks the faster path on all 24, profiles/wgrad_ab_r2.json): us = rounds x (a·K-tiles per split + b) + c·MB of
// slab / C traffic, rounds = ceil(workgroups / 256) (one workgroup per CU on both). HSD_G2_SMALL_TT=0 / 1 forces
// the tile size (the split count is still chosen by the model); >= 2 K-tiles per split.
struct WgradPlan {
  bool small;
  int splits;
};

inline double wgrad_cost(int M, int N, int K, int s, bool small) {
  const int tile = small ? 128 : 256;
  const double tiles = (double)((M + tile - 1) / tile) * ((N + tile - 1) / tile);
  const int kt_all = K / 64;
  const int kt = (kt_all + s - 1) / s;
  const int real = (kt_all + kt - 1) / kt;
  const double rounds = std::ceil(tiles * real / 256.0);
  const double mb = ((real > 1 ? 8.0 * real : 0.0) + 8.0) * M * N / 1e6;
  return small ? rounds * (0.658 * kt + 5.02) + 0.176 * mb : rounds * (1.637 * kt + 15.9) + 0.0847 * mb;
}

inline WgradPlan wgrad_plan(int M, int N, int K) {
  const int force = HSD_KNOB("HSD_G2_SMALL_TT", -1);
  const bool can_small = N % kSBN == 0 && M % 8 == 0 && K % 64 == 0 && force != 0;
  const bool can_big = N % 256 == 0 && force != 1;
  // small steps (<= 8,192 tokens), whose weight gradients run on the side stream under the backward: the fewest K-splits
  // of the 128 x 128 kernel that still give 384 workgroups, so a weight gradient takes no more CUs and slab traffic
  // than it needs beside the critical path (the latency cost model below minimises its own time instead). Measured
  // (profiles/wgrad_min_grid_ab_r4.log): bert-large S=512 B=8 504-505 -> 524-526 seq/s, bert-base B=64 +1.8 % at a
  // 192-workgroup target; re-swept in round 6 with the optimizer slices behind the weight-gradient forks
  // (profiles/r6/bl8_knob_sweep_r6.log, profiles/r6/wgrad_min_grid_small_steps_r6.log): 384 is +1.2-1.4 % at
  // bert-large B = 8 (552.6-554.2 vs 546.4-547.7) and ahead at bert-base B = 32 too; 256, 512 and 768 are 2 % slower.
  // Both are 4,096-token steps: below that (the graph-replayed small batches) the measured 192 stays.
  // HSD_WGRAD_MIN_GRID sets the workgroup target (0 = the cost model at every size).
  const int grid_knob = HSD_KNOB("HSD_WGRAD_MIN_GRID", kKnobUnset);
  const int min_grid = grid_knob != kKnobUnset ? grid_knob : (K <= 8192 ? (K >= 4096 ? 384 : 192) : 0);
  if (min_grid > 0 && can_small) {
    const int tiles = ((M + 127) / 128) * ((N + 127) / 128);
    int sp = 1;
    while (tiles * sp < min_grid && sp < 32 && (K / 64) / (sp + 1) >= 2) ++sp;
    return WgradPlan{true, sp};
  }
  const int min_kt = 2;
  const int kt_all = K / 64;
  WgradPlan best{can_small && !can_big, 1};
  double best_cost = 1e30;
  for (int small = 0; small < 2; ++small) {
    if (small ? !can_small : !can_big) continue;
    for (int sp = 1; sp <= 32 && (sp == 1 || kt_all / sp >= min_kt); ++sp) {
      const double c = wgrad_cost(M, N, K, sp, small);
      if (c < best_cost) { best_cost = c; best = WgradPlan{small != 0, sp}; }
    }
  }
  return best;
}

// LDS stages of gemm2s: 2 -> two workgroups per CU, 3 -> one with a deeper DMA prefetch. A grid that fits one
// workgroup per CU takes 3 stages, a larger one 2 (tools/nt_ab.py, profiles/nt_ab_r2.jsonl: at T = 8192 the 384-tile
// bert-base GEMMs run 19-49 us at 2 stages vs 26-68 us at 3; at <= 256 tiles 3 stages are equal or up to 5 % faster).
// HSD_G2S_STAGES (2-4) overrides.
inline int g2s_stages(int grid) {
  const int e = HSD_KNOB("HSD_G2S_STAGES", kKnobUnset);
  const int v = e != kKnobUnset ? e : (grid <= 256 ? 3 : 2);
  return v < 2 ? 2 : (v > 4 ? 4 : v);
}

// gemm2s workgroup for grids of one workgroup per CU (3 stages): 8 waves with the in-workgroup K-split (2 waves per
// SIMD, default) or 4 (one per SIMD). Measured end to end (profiles/g2s_kw2_ab_r4.log, interleaved x2): bert-large
// S = 512 B = 8 488 -> 500-502 seq/s, bert-base B = 32 5,581-5,666 -> 5,723-5,734. HSD_G2S_KW = 1 / 2 overrides.
inline int g2s_kw(int grid) {
  const int e = HSD_KNOB("HSD_G2S_KW", kKnobUnset);
  if (e != kKnobUnset) return e == 2 ? 2 : 1;
  (void)grid;
  return 2;
}

// K-splits of the fp32-output NT GEMM (the fp32 step's split-product forward / dgrad): a 256 x 256 grid of at most
// half the CUs (bert-large B = 8: M = 4,096 tokens, N = 1,024 -> 64 workgroups on 256 CUs) is split over K until it
// fills the chip, keeping >= 8 K-tiles per split. HSD_F32NT_SPLITS: 1 = off, n = force n.
inline int gemm2_f32nt_splits(int M, int N, int K, int cus) {
  const int force = HSD_KNOB("HSD_F32NT_SPLITS", 0);
  if (force > 0) return std::max(1, std::min(force, K / 64));
  const int tiles = ((M + 255) / 256) * ((N + 255) / 256);
  if (2 * tiles > cus) return 1;
  return std::max(1, std::min(cus / tiles, K / (64 * 8)));
}

// the fp32 forward / dgrad on 128 x 128 tiles (gemm2s, one K-split) for grids that 256 x 256 tiles leave mostly idle
// (gemm2s_use) and K < 6,144, instead of 256 x 256 tiles split over K into slabs plus a reduce pass. bert-large T = 4,096
// (tools/seg_vs_cat.py, profiles/r6/seg_vs_cat_r6e.log): N 1,024 at K 3 x 1,024: 32.4 / 34.8 us (fwd / dgrad) vs 44.4 /
// 45.2 on slabs; at K 3 x 3,072 and 3 x 4,096 the slabs win (81.6 vs 91.2, 96.6 vs 111.8, 99.3 vs 124.5 us).
// HSD_SEG_NT_SMALL=0: always the slabs.
inline bool seg_nt_small(int M, int N, int K) {
  return HSD_KNOB("HSD_SEG_NT_SMALL", 1) && K < 6144 && gemm2s_use(M, N, K);
}

// K-splits of the fp8 weight gradient: wgrad_plan's cost model for the 256-tile kernel with one fp8 K-tile (128 tokens:
// the bytes and MFMA cycles of one bf16 K-tile of 64) per bf16 K-tile
inline int gemm8_wgrad_splits(int M, int N, int T) {
  const int kt_all = T / 128;
  int best = 1;
  double best_cost = 1e30;
  for (int sp = 1; sp <= 32 && (sp == 1 || kt_all / sp >= 2); ++sp) {
    const double c = wgrad_cost(M, N, T / 2, sp, false);
    if (c < best_cost) { best_cost = c; best = sp; }
  }
  return best;
}

// ---- plan builders ----------------------------------------------------------------------------------------------------
// 256-row tiles, one tile x K-split per workgroup (gemm2_kernel)
inline void use_g2(GemmPlan& pl, int M, int N, int K, int bn, int splits) {
  const KSplit ks = k_split(K, splits);
  pl.kernel = GK_G2;
  pl.bn = bn;
  pl.sync = pl.seg ? 4 : g2_sync_mode();
  pl.kps = ks.kps;
  pl.splits = ks.real;
  pl.tiles_n = (N + bn - 1) / bn;
  pl.ntiles = ((M + kBM - 1) / kBM) * pl.tiles_n;
  pl.grid = pl.ntiles * ks.real;
  pl.wg = 512;
}

// 128 x 128 tiles (gemm2s_kernel): stages and waves by the grid
inline void use_g2s(GemmPlan& pl, int M, int N, int K, int splits) {
  const KSplit ks = splits <= 1 ? KSplit{K, 1} : k_split(K, splits);
  pl.kernel = GK_G2S;
  pl.kps = ks.kps;
  pl.splits = ks.real;
  pl.tiles_n = N / kSBN;
  pl.ntiles = ((M + kSBM - 1) / kSBM) * pl.tiles_n;
  pl.grid = pl.ntiles * ks.real;
  const int ns = g2s_stages(pl.grid);
  if (ns == 2) { pl.nstg = 2; pl.kw = 1; }
  else if (pl.seg || (ns == 3 && g2s_kw(pl.grid) == 2)) { pl.nstg = 3; pl.kw = 2; }
  else { pl.nstg = ns; pl.kw = 1; }
  pl.wg = 256 * pl.kw;
}

// persistent NT kernels (gemm2pk / gemm8pk): one workgroup per CU over a tile queue
inline void use_pk(GemmPlan& pl, int kernel, int M, int N, int K, int bn, int cus) {
  pl.kernel = kernel;
  pl.bn = bn;
  pl.kps = K;
  pl.splits = 1;
  pl.tiles_n = (N + bn - 1) / bn;
  pl.ntiles = ((M + kBM - 1) / kBM) * pl.tiles_n;
  pl.grid = std::min(pl.ntiles, cus & ~7);
  pl.wg = 512;
}

inline void use_slabs(GemmPlan& pl, int landing, int M, int N) {
  pl.landing = landing;
  pl.ws_numel = (int64_t)pl.splits * M * N;
}

// Tile width of a one-pass bf16-output NT GEMM: E2_STORE_RDOT has 64-column wave tiles (one head per 8-lane group) and
// the fused column sums 8 columns per lane, both BN 256 only; k-strided B images are 256 wide
inline int nt_bn(int lb, int epi, int M, int N, bool dbias) {
  return (lb == 1 || epi == E2_STORE_RDOT || dbias) ? 256 : gemm2_pick_bn(M, N);
}

// ---- entry points -----------------------------------------------------------------------------------------------------
// launch_gemm2: NT (0,0) / (0,1) with a bf16 epilogue (B k-contiguous, or k-strided: the dgrad reading W[N_out][K_in]
// directly, no Wᵀ copy), the fp32-output NT (la 0, E2_F32_SLAB) and the TT weight gradient (1,1; E2_F32_SLAB /
// E2_F32_ATOMIC, C += ...). splits <= 0: automatic. c_vec4: C's leading dimension is a multiple of 4 (TT in place).
inline GemmPlan plan_gemm2(int la, int lb, int epi, int M, int N, int K, int splits, bool dbias, int cus,
                           bool c_vec4 = true) {
  GemmPlan pl;
  pl.la = la; pl.lb = lb; pl.epi = epi; pl.M = M; pl.N = N;
  if (K % 64 || M < 1 || N % 8 || K < 64) return pl;
  if (epi == E2_STORE_RDOT && (la != 0 || N % 256)) return pl;
  if (dbias && (la != 0 || !epi_fused_dbias(epi) || N % 256)) return pl;
  if (la == 0 && epi == E2_F32_SLAB) {
    // fp32 output [M][N] (ldc == N): the split-product GEMMs of the fp32 step (fp32.hip, ops/hip32.py). More than one
    // split (grids that would leave most CUs idle): K-split fp32 slabs in the workspace, then C = Σ slabs
    if (N % 256 || (lb != 0 && lb != 1)) return pl;
    if (splits <= 0) splits = gemm2_f32nt_splits(M, N, K, cus);
    use_g2(pl, M, N, K, 256, splits);
    if (splits > 1) use_slabs(pl, GL_SLABS_ASSIGN, M, N);
    return pl;
  }
  if (la == 0 && (lb == 0 || lb == 1)) {
    // 128 x 128 tiles for grids the 256 x 256 kernel leaves mostly idle, split-K slabs + one reduce-and-epilogue pass
    // for the smallest grids
    if (!epi_bf16_out(epi)) return pl;
    const bool small = gemm2s_use(M, N, K);
    if (lb == 0 ? gemm2_pick_bn(M, N) == 0 : !(N % 256 == 0 || small)) return pl;
    if (splits <= 0) splits = gemm2_nt_splits(M, N, K);
    if (splits > 1) {
      pl.epi = E2_F32_SLAB;
      pl.out_epi = epi;
      if (small) use_g2s(pl, M, N, K, splits);
      else use_g2(pl, M, N, K, 256, splits);
      use_slabs(pl, GL_SLABS_EPI, M, N);
    } else if (small) {
      use_g2s(pl, M, N, K, 1);
    } else {
      const int bn = nt_bn(lb, epi, M, N, dbias);
      if (lb == 0 && g2_persist((M + 255) / 256 * (N / bn), cus)) use_pk(pl, GK_G2PK, M, N, K, bn, cus);
      else use_g2(pl, M, N, K, bn, 1);
    }
    return pl;
  }
  if (la == 1 && lb == 1) {
    if ((epi != E2_F32_ATOMIC && epi != E2_F32_SLAB) || M % 8) return pl;
    const WgradPlan wp = wgrad_plan(M, N, K);
    const bool small = epi == E2_F32_SLAB && wp.small;
    if (N % 256 && !small) return pl;
    if (splits <= 0) splits = wp.splits;
    if (small) {
      // one split: the kernel accumulates into C (unique owner per element)
      use_g2s(pl, M, N, K, splits);
      if (pl.splits > 1) use_slabs(pl, GL_SLABS_ADD, M, N);
      else pl.landing = GL_ACCUM;
    } else if (epi == E2_F32_SLAB && splits > 1) {
      use_g2(pl, M, N, K, 256, splits);
      use_slabs(pl, GL_SLABS_ADD, M, N);
    } else if (epi == E2_F32_SLAB && c_vec4 && !HSD_KNOB("HSD_G2_TT_ATOMIC", 0)) {
      // one K-split: every output element has one owner -> C += acc in place instead of fp32 atomics (the tied MLM
      // decoder weight gradient: Vp x H = 51.6 M atomics per roberta-large step; HSD_G2_TT_ATOMIC=1 = the old path)
      use_g2(pl, M, N, K, 256, 1);
      pl.landing = GL_ACCUM;
      pl.accum_flag = true;
    } else {
      pl.epi = E2_F32_ATOMIC;
      use_g2(pl, M, N, K, 256, splits);
      pl.landing = GL_ATOMIC;
    }
    return pl;
  }
  return pl;
}

// launch_gemm2_seg: segmented-K fp32-output GEMMs, K = 3 · Kseg. la = 0, lb = 0 / 1: the NT forward / dgrad (C written,
// or C += with `accumulate`; split-K slabs + one reduce for small grids, gemm2_f32nt_splits), la = lb = 1: the TT weight
// gradient (C += ..., wgrad_plan's tile size and K-splits).
inline GemmPlan plan_gemm2_seg(int la, int lb, int M, int N, int Kseg, bool accumulate, int cus) {
  GemmPlan pl;
  pl.la = la; pl.lb = lb; pl.epi = E2_F32_SLAB; pl.M = M; pl.N = N;
  pl.seg = true;
  const int K = 3 * Kseg;
  if (Kseg % 64 || Kseg <= 0 || M < 1 || N % 8) return pl;
  if (la == 0 && (lb == 0 || lb == 1)) {
    if (N % 256) return pl;
    if (seg_nt_small(M, N, K)) {
      // 128 x 128 tiles, one K-split: the grid fills the CUs without slabs or a reduce pass; each output element has
      // one owner (written, or C += acc with `accumulate`)
      use_g2s(pl, M, N, K, 1);
      pl.landing = accumulate ? GL_ACCUM : GL_STORE;
      pl.accum_flag = accumulate;
      return pl;
    }
    const int sp = gemm2_f32nt_splits(M, N, K, cus);
    use_g2(pl, M, N, K, 256, sp);
    if (sp > 1) {
      use_slabs(pl, accumulate ? GL_SLABS_ADD : GL_SLABS_ASSIGN, M, N);
    } else {
      pl.landing = accumulate ? GL_ACCUM : GL_STORE;  // one split: each element has one owner (C += acc in place)
      pl.accum_flag = accumulate;
    }
    return pl;
  }
  if (la == 1 && lb == 1) {
    const WgradPlan wp = wgrad_plan(M, N, K);
    if (M % 8 || (N % 256 && !wp.small)) return pl;
    if (wp.small) use_g2s(pl, M, N, K, wp.splits);  // one split: the kernel accumulates into C
    else use_g2(pl, M, N, K, 256, wp.splits);
    if (pl.splits > 1) {
      use_slabs(pl, GL_SLABS_ADD, M, N);
    } else {
      pl.landing = GL_ACCUM;
      pl.accum_flag = !wp.small;
    }
    return pl;
  }
  return pl;
}

// launch_gemm8: fp8 NT on the persistent kernel, bf16 epilogues. K in fp8 elements (bytes), K % 128 == 0; fa: A format
// (0 e4m3, 1 e5m2); q8: the epilogue also writes the output's fp8 copy.
inline GemmPlan plan_gemm8(int epi, int M, int N, int K, int fa, bool dbias, bool q8, int cus) {
  GemmPlan pl;
  pl.epi = epi; pl.fa = fa; pl.q8 = q8; pl.M = M; pl.N = N;
  if (epi == E2_STORE_RDOT && N % 256) return pl;  // 256-wide tiles: one 64-column head per 8-lane group
  if (K % 128 || K < 128 || M < 1 || N % 8 || !epi_bf16_out(epi) || gemm2_pick_bn(M, N) == 0) return pl;
  if (dbias && (!epi_fused_dbias(epi) || N % 256)) return pl;
  if (q8 && !epi_q8_copy(epi)) return pl;
  if (fa != 0 && fa != 1) return pl;
  use_pk(pl, GK_G8PK, M, N, K / 2, nt_bn(0, epi, M, N, dbias), cus);  // a K-tile of 128 fp8 values = 64 bf16 words
  return pl;
}

// launch_gemm8_wgrad: the fp8 TT weight gradient, T tokens in splits of a multiple of 128; the workspace holds one
// [M][N] fp32 slab per split launched, summed into C by slab_reduce_kernel. splits <= 0: automatic.
inline GemmPlan plan_gemm8_wgrad(int M, int N, int T, int splits, int fdy) {
  GemmPlan pl;
  pl.la = 1; pl.lb = 1; pl.epi = E2_F32_SLAB; pl.fa = fdy; pl.M = M; pl.N = N;
  if (M % 256 || N % 256 || T % 128 || T < 128 || M < 256 || N < 256 || (fdy != 0 && fdy != 1)) return pl;
  if (splits <= 0) splits = gemm8_wgrad_splits(M, N, T);
  const KSplit ks = k_split(T, splits, 128);
  pl.kernel = GK_G8TT;
  pl.kps = ks.kps;
  pl.splits = ks.real;
  pl.tiles_n = N / 256;
  pl.ntiles = (M / 256) * pl.tiles_n;
  pl.grid = pl.ntiles * ks.real;
  pl.wg = 512;
  use_slabs(pl, GL_SLABS_ADD, M, N);
  return pl;
}

// ---- the kernels a plan enqueues, in order (_C.gemm_plan; compared with kernel traces) -----------------------------
struct GridDim {
  int x, y;
};
inline int slab_reduce_blocks(int M, int N) {
  const int64_t n4 = (int64_t)M * N / 4;
  return (int)std::min<int64_t>((n4 + 255) / 256, 2048);
}
// splitk_epi_kernel: 64 columns x `rpb` rows per block
inline GridDim splitk_epi_grid(int M, int N, int* rpb_out) {
  const int gx = (N + 63) / 64;
  const int gy_want = std::max(1, 2048 / gx);
  int rpb = (M + gy_want - 1) / gy_want;
  rpb = (rpb + 31) / 32 * 32;
  *rpb_out = rpb;
  return GridDim{gx, (M + rpb - 1) / rpb};
}

struct PlannedLaunch {
  std::string kernel;
  std::vector<int> targs;
  int grid, wg;
};

inline std::vector<PlannedLaunch> plan_launches(const GemmPlan& pl) {
  std::vector<PlannedLaunch> out;
  switch (pl.kernel) {
    case GK_G2: out.push_back({"gemm2_kernel", {pl.la, pl.lb, pl.epi, pl.bn, pl.sync, pl.seg}, pl.grid, pl.wg}); break;
    case GK_G2PK: out.push_back({"gemm2pk_kernel", {pl.epi, pl.bn}, pl.grid, pl.wg}); break;
    case GK_G2S:
      out.push_back({"gemm2s_kernel", {pl.la, pl.lb, pl.epi, pl.nstg, pl.kw, pl.seg}, pl.grid, pl.wg});
      break;
    case GK_G8PK: out.push_back({"gemm8pk_kernel", {pl.epi, pl.bn, pl.fa, 0, pl.q8}, pl.grid, pl.wg}); break;
    case GK_G8TT: out.push_back({"gemm8tt_kernel", {pl.fa, 0}, pl.grid, pl.wg}); break;
    default: return out;
  }
  if (pl.landing == GL_SLABS_ASSIGN || pl.landing == GL_SLABS_ADD) {
    out.push_back({"slab_reduce_kernel", {}, slab_reduce_blocks(pl.M, pl.N), 256});
  } else if (pl.landing == GL_SLABS_EPI) {
    int rpb;
    const GridDim g = splitk_epi_grid(pl.M, pl.N, &rpb);
    out.push_back({"splitk_epi_kernel", {pl.out_epi}, g.x * g.y, 256});
  }
  return out;
}

}  // namespace plan
}  // namespace hsd
