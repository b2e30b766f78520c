// Host-side launch functions of the gfx950 kernels (implemented in csrc/kernels/*.hip).
// Every launcher is stream-ordered and allocation-free, so callers may capture it into a hipGraph.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm_plan.h"

namespace hsd {
typedef uint16_t bf16_t;
struct DropoutParams;

// adam.hip
void launch_adam(float* p, float* m, float* v, void* g, bool grad_bf16, bf16_t* out_bf16,
                 const uint8_t* decay, int64_t n, float step, float eps, float b1, float b2, float gscale,
                 float lr_wd, const float* coef, hipStream_t stream,
                 bf16_t* out_lo = nullptr, bool zero_grad = false, const float* clip = nullptr,
                 const float* lr_mul = nullptr,  // fp32 [n / 64]: learning-rate multiplier per 64-element block
                 // fp32 [n]: the weight average, ema += ema_w·(p_new - ema) in the same pass (coef[4] replaces ema_w;
                 // coef is then fp32 [8])
                 float* ema = nullptr, float ema_w = 0.0f);

// gradnorm.hip: global-norm gradient clipping. grad_sumsq writes grad_sumsq_blocks(n, bf16) fp32 partials (one per
// block, no atomics) for n gradients (a multiple of 64, 16-B aligned); finalize turns `nparts` partials into
// out[0] = norm = sqrt(sum) * gscale (gscale from coef[2] when coef is given) and out[1] = max_norm / norm if
// norm > max_norm else 1.
int grad_sumsq_blocks(int64_t n, bool grad_bf16);
void launch_grad_sumsq(const void* g, bool grad_bf16, int64_t n, float* partials, hipStream_t stream);
void launch_grad_clip_finalize(const float* partials, int64_t nparts, float gscale, const float* coef, float max_norm,
                               float* out, hipStream_t stream);

// lamb.hip: fused LAMB (TF Addons' math) on segments [seg0, seg0 + nsegs) of the flat store = tiles
// [tile0, tile0 + ntiles) of the host-built tables tiles [*, 3] = (start, length, segment) and segs [*, 3] = (first
// tile, tiles, adapt / decay flag); a tile is at most lamb_tile() elements and never straddles two segments. Three
// launches: moments + per-tile (Σw², Σu²) into partials[2 tile ...], per-segment (r, Σw², Σu²) into ratio[3 seg ...],
// then the weight update (with the bf16 copy, or the hi / lo halves). coef: fp32 [8] on the device (lr, 1/(1-b1ᵗ),
// 1/(1-b2ᵗ), eps, grad_scale, wd, ema_w, -) overriding the scalars; clip: fp32 [1] multiplied into grad_scale; lr_mul:
// fp32 [segments], each segment's learning-rate multiplier (indexed by global segment id; the weight update only);
// ema: fp32, laid out as p, the weight average ema += ema_w·(p_new - ema) written by the weight update.
int lamb_tile();
void launch_lamb(float* p, float* m, float* v, void* g, bool grad_bf16, bf16_t* out_bf16, bf16_t* out_lo,
                 const int64_t* tiles, const int64_t* segs, int64_t tile0, int64_t ntiles, int64_t seg0, int64_t nsegs,
                 float* partials, float* ratio, float lr, float ibc1, float ibc2, float eps, float b1, float b2,
                 float gscale, float wd, const float* coef, const float* clip, bool zero_grad, hipStream_t stream,
                 const float* lr_mul = nullptr, float* ema = nullptr, float ema_w = 0.0f);

}  // namespace hsd

namespace hsd {
// layernorm.hip
void launch_ln_fwd(const bf16_t* y, const bf16_t* res, const bf16_t* gamma, const bf16_t* beta, bf16_t* z,
                   bf16_t* out, float* mean, float* rstd, int rows, int H, float eps, double p, uint64_t seed,
                   hipStream_t st, uint32_t row_mul = 1);
void launch_ln_fwd_q8(const bf16_t* y, const bf16_t* gamma, const bf16_t* beta, bf16_t* out, float* mean, float* rstd,
                      int rows, int H, float eps, uint8_t* q8, const float* amax_in, float* sinv, float* amax_track,
                      hipStream_t st);
void launch_ln_bwd_q8(const bf16_t* dout, const bf16_t* z, const float* mean, const float* rstd, const bf16_t* gamma,
                      bf16_t* dz, bf16_t* dy, const bf16_t* dres_add, float* dgamma, float* dbeta, float* dbias,
                      int rows, int H, double p, uint64_t seed, uint8_t* q8, const float* amax_in, float* sinv,
                      float* amax_track, int qfmt, hipStream_t st, bool q8_only = false);
void launch_ln_bwd(const bf16_t* dout, const bf16_t* z, const float* mean, const float* rstd, const bf16_t* gamma,
                   bf16_t* dz, bf16_t* dy, const bf16_t* dres_add, float* dgamma, float* dbeta, float* dbias,
                   int rows, int H, double p, uint64_t seed, hipStream_t st, uint32_t row_mul = 1);
// embedding.hip
void launch_embed_fwd(const int64_t* ids, const int64_t* pos_ids, const int64_t* type_ids, const bf16_t* word,
                      const bf16_t* pos, const bf16_t* type, const bf16_t* gamma, const bf16_t* beta, bf16_t* out,
                      float* mean, float* rstd, int rows, int H, float eps, double p, uint64_t seed, hipStream_t st,
                      uint8_t* q8 = nullptr, const float* amax_in = nullptr, float* sinv = nullptr,
                      float* amax_track = nullptr);  // q8: the output's fp8 copy (as launch_ln_fwd_q8)
void launch_embed_bwd(const bf16_t* dout, const int64_t* ids, const int64_t* pos_ids, const int64_t* type_ids,
                      const bf16_t* word, const bf16_t* pos, const bf16_t* type, const bf16_t* gamma,
                      const float* mean, const float* rstd, float* gword, float* gpos, float* gtype, float* ggamma,
                      float* gbeta, int B, int S, int H, int pos_is_arange, double p, uint64_t seed, hipStream_t st);
// elementwise.hip
void launch_gelu_fwd(const bf16_t* y, bf16_t* g, int64_t n, hipStream_t st);
void launch_gelu_bwd_colsum(const bf16_t* dg, const bf16_t* y, bf16_t* da, float* dbias, int rows, int N,
                            hipStream_t st);
void launch_colsum(const bf16_t* x, float* dbias, int rows, int N, hipStream_t st);
// the 32 mask bits of column pair cp of row `row` of a dropout site with 64-bit `seed` (common.h), on the host
uint32_t dropout_pair_bits_host(uint64_t seed, uint32_t row, uint32_t cp);
// row_mul: row r of x is row r * row_mul of the dropout site (common.h DropoutParams)
void launch_dropout(const bf16_t* x, bf16_t* out, int64_t n, int W, double p, uint64_t seed, hipStream_t st,
                    uint32_t row_mul = 1);
// dst[b * S][:] += src[b][:] (bf16, H % 8 == 0): the first-token rows' residual gradient into a [B * S, H] buffer
void launch_add_rows_strided(bf16_t* dst, const bf16_t* src, int B, int S, int H, hipStream_t st);
void launch_mask_bias(const void* mask, bool i64, float* out, int64_t n, hipStream_t st);
// C[N][K] (fp32, ldc) += dy[T][N]ᵀ · x[T][K] for small T (K % 4 == 0)
void launch_small_wgrad(const bf16_t* dy, int64_t ldy, const bf16_t* x, int64_t ldx, float* C, int64_t ldc, int T,
                        int N, int K, hipStream_t st);
// xent.hip: fused softmax cross-entropy (+ gradient, + argmax-correct count); stats = {Σloss, correct}.
// label_smoothing eps in [0, 1): target (1-eps)·onehot + eps/V over the V real classes (0: the plain CE's own code)
void launch_xent(const void* logits, bool bf16, const int64_t* labels, void* dlogits, float* stats,
                 const float* n_valid, int rows, int V, int64_t ld, hipStream_t st, float label_smoothing = 0.0f);
// mlm_mask.hip: dynamic MLM masking with ordered compaction into fixed-capacity buffers (ops/rng.py "MLM mask").
// ids / attention_mask (optional) / labels_in (optional): int64 [N]; ids_out, labels_out: int64 [N]; sel, tgt: int64
// [cap]; inv: int32 [N]; counts: int32 [2] = {n, dropped}; n_valid: fp32 [1]; ws: int32 [mlm_mask_blocks(N)].
struct MlmMaskParams {
  const int64_t* ids;
  const int64_t* attention_mask;
  const int64_t* labels_in;
  int64_t* ids_out;
  int64_t* labels_out;
  int64_t* sel;
  int64_t* tgt;
  int* inv;
  int* counts;
  float* n_valid;
  int* ws;
  int64_t N;
  int cap;
  uint32_t seed_lo, seed_hi;
  uint32_t thr;  // select iff the low 16 bits of w0 < thr
  int64_t mask_id, rand_lo, rand_hi;
  int64_t special[8];
  int n_special;
  const uint32_t* dev_seed;  // set by the launcher
};
int mlm_mask_block();
int mlm_mask_blocks(int64_t N);
// use_step_seed: XOR the process-wide device step seed (set_dropout_dev_seed) into the mask seed, as dropout does
void launch_mlm_mask(MlmMaskParams p, bool use_step_seed, hipStream_t st);
// dh[t][:] = inv[t] >= 0 ? dx[inv[t]][:] : 0   (bf16 [N, H], H % 8 == 0, dx [dx_rows, H]); every row written once
void launch_mlm_scatter_rows(const bf16_t* dx, const int* inv, bf16_t* dh, int64_t N, int H, int dx_rows,
                             hipStream_t st);
// gradient wire casts (comm_engine 16-bit compression): to16: dst16 = src32 * scale; else dst32 = src16 * scale.
// half: fp16, else bf16. n % 4 == 0, 16-B aligned fp32 side.
void launch_wire_cast(const void* src, void* dst, int64_t n, bool to16, bool half, float scale, hipStream_t st);
// desc: int64 [n][5] = {src, dst, rows, cols, first_tile}; rows, cols multiples of 4
void launch_transpose_many(const int64_t* desc, int n, int total_tiles, hipStream_t st);
// head_stats.hip: partials fp32 [nblk][4] = per-block {loss sum, hits, n_valid} of a classification head's forward ->
// stats fp32 [4] = {mean loss, hits, n_valid, loss sum} (one workgroup)
void launch_head_stats(const float* partials, int nblk, float* stats, hipStream_t st);
// cls_head.hip: fused sequence-classification head after the dense GEMM (act, dropout, classifier, CE, accuracy)
int cls_head_blocks(int R);
void launch_cls_head_fwd(const bf16_t* pre, int64_t ld_pre, const bf16_t* W2, const bf16_t* b2, const int64_t* labels,
                         bf16_t* t_out, bf16_t* logits, float* partials, float* stats, int R, int H, int C, int act,
                         double p, uint64_t seed, hipStream_t st);
void launch_cls_head_bwd(const bf16_t* t_in, const bf16_t* W2, const bf16_t* logits, const int64_t* labels,
                         const float* stats, const float* dloss, bf16_t* dpre, float* dW2, float* db2, int R, int H,
                         int C, int act, double p, uint64_t seed, hipStream_t st);
// seq_head.hip: the same place in the sequence-classification model for 1 <= C <= 64 and three losses. mode 0: CE,
// labels lab_i int64 [R]; 1: BCE-with-logits, 2: MSE, labels lab_f fp32 [R][C] (a row whose first label is NaN is
// ignored). The backward writes g fp32 [R][C] and seq_head_splits(R) slabs of seq_head_slab(H, C) floats, and adds
// them into dW2 / db2 in split order (no atomics).
int seq_head_blocks(int R);
int seq_head_splits(int R);
int64_t seq_head_slab(int H, int C);
void launch_seq_head_fwd(const bf16_t* pre, int64_t ld_pre, const bf16_t* W2, const bf16_t* b2, const int64_t* lab_i,
                         const float* lab_f, bf16_t* t_out, bf16_t* logits, float* partials, float* stats, int R, int H,
                         int C, int mode, float tol, int act, double p, uint64_t seed, hipStream_t st,
                         float label_smoothing = 0.0f);
void launch_seq_head_bwd(const bf16_t* t_in, const bf16_t* W2, const bf16_t* logits, const int64_t* lab_i,
                         const float* lab_f, const float* stats, const float* dloss, bf16_t* dpre, float* g, float* slab,
                         float* dW2, float* db2, int R, int H, int C, int mode, int act, double p, uint64_t seed,
                         hipStream_t st, float label_smoothing = 0.0f);
// label_smoothing (CE mode of seq_head, token_head with labels): eps in [0, 1), target (1-eps)·onehot + eps/C. It is a
// host constant of the launch; 0 launches the unsmoothed template instantiations.
// token_head.hip: fused token-classification head over every row (dropout, classifier, CE, accuracy); H % 8 == 0,
// H <= 1024, 2 <= C <= 16. labels may be null (logits only: stats untouched). The backward writes
// token_head_bwd_blocks(R) fp32 partial slabs of C·H + C into `part` and adds them into dW / db; dh may be null.
int token_head_fwd_blocks(int R);
int token_head_bwd_blocks(int R);
void launch_token_head_fwd(const bf16_t* h, const bf16_t* W, const bf16_t* b, const int64_t* labels, bf16_t* logits,
                           float* partials, float* stats, int R, int H, int C, double p, uint64_t seed,
                           hipStream_t st, float label_smoothing = 0.0f);
void launch_token_head_bwd(const bf16_t* h, const bf16_t* W, const bf16_t* logits, const int64_t* labels,
                           const float* stats, const float* dloss, bf16_t* dh, float* part, float* dW, float* db,
                           int R, int H, int C, double p, uint64_t seed, hipStream_t st,
                           float label_smoothing = 0.0f);
// the same backward from a GIVEN per-row gradient table g0 [R][C] fp32 (zero rows are ignored rows):
// g[row][c] = g0[row][c] · dloss · gmul / max(cnt[c], 1), cnt fp32 [C] on the device
void launch_token_head_bwd_given(const bf16_t* h, const bf16_t* W, const float* g0, const float* cnt, float gmul,
                                 const float* dloss, bf16_t* dh, float* part, float* dW, float* db, int R, int H,
                                 int C, double p, uint64_t seed, hipStream_t st);
// qa_head.hip: span-extraction loss of --task question-answering on logits [R][2] bf16. One workgroup per sequence
// (rows cu[b] .. cu[b+1]-1, at most 1,024; mask int64 [R] optional), then the stats reducer. pos int64 [B][2] may be
// null (pred only: rec, g0 and stats untouched). rec fp32 [B][8], pred int32 [B][2], g0 fp32 [R][2], stats fp32 [8].
void launch_span_ce(const bf16_t* logits, const int* cu, const int64_t* mask, const int64_t* pos, int max_answer_length,
                    float* rec, int* pred, float* g0, float* stats, int R, int B, hipStream_t st);
// attention.hip
bool attn_streaming(int S);
// kmask (optional, streaming S > 128 kernels: attn_keep_mask_supported): the forward writes its dropout keep bits
// ([B*heads][S/32][S] u32, attentionS.hip header), the backward reads them instead of re-hashing every (query, key) pair
bool attn_keep_mask_supported(int S);
int64_t attn_keep_mask_numel(int B, int S, int heads);
void launch_attn_fwd(const bf16_t* qkv, const float* mask, bf16_t* out, float* lse2, int B, int S, int heads,
                     double p, uint64_t seed, hipStream_t st, uint32_t* kmask = nullptr);
// attentionS.hip fp8 variants (S > 128 streaming kernels only: attn_streaming(S) && S > 128)
void launch_attnS_fwd_q8(const bf16_t* qkv, const float* mask, bf16_t* out, float* lse2, int B, int S, int heads,
                         double p, uint64_t seed, uint8_t* q8, const float* amax_in, float* sinv, float* amax_track,
                         hipStream_t st, uint32_t* kmask = nullptr);
void launch_attnS_bwd_q8(const bf16_t* qkv, const float* mask, const bf16_t* o, const bf16_t* dout, const float* lse2,
                         bf16_t* dqkv, float* delta_ws, float* dbias, int B, int S, int heads, double p, uint64_t seed,
                         uint8_t* q8, const float* amax_in, float* sinv, float* amax_track, int qfmt, hipStream_t st,
                         const uint32_t* kmask = nullptr, bool delta_ready = false, bool q8_only = false);
// dbias (optional): fp32 [3H] += column sums of dqkv (the fused QKV bias gradient)
void launch_attn_bwd(const bf16_t* qkv, const float* mask, const bf16_t* o, const bf16_t* dout, const float* lse2,
                     bf16_t* dqkv, float* dq_acc, float* dbias, int B, int S, int heads, double p, uint64_t seed,
                     hipStream_t st, const uint32_t* kmask = nullptr, bool delta_ready = false);
// attention_cls.hip: attention of query row 0 only (the first token of each sequence; head_dim 64, even S <= 4096).
// Forward: out [B, H], lse2 [B * heads]. Backward: the full dqkv [B * S, 3H] (dK / dV of every key, dQ of row 0, zeros
// in every other dQ row) and, with dbias, fp32 [3H] += its column sums. Dropout rows are the full kernels' rows.
bool attn_cls_supported(int S, int head_dim);
void launch_attn_cls_fwd(const bf16_t* qkv, const float* mask, bf16_t* out, float* lse2, int B, int S, int heads,
                         double p, uint64_t seed, hipStream_t st);
void launch_attn_cls_bwd(const bf16_t* qkv, const float* mask, const bf16_t* dctx, const float* lse2, bf16_t* dqkv,
                         float* dbias, int B, int S, int heads, double p, uint64_t seed, hipStream_t st);
// attention_varlen.hip: padding-free attention over a packed qkv [T, 3H]; sequence b is rows cu_seqlens[b] ..
// cu_seqlens[b+1]-1 (device int32 [B+1]), rows from cu_seqlens[B] on are dead (written as zeros); lse2 is [heads, T].
// The backward writes every dqkv element once (no atomics) and adds the column sums of dqkv into dbias when given.
void launch_attn_varlen_fwd(const bf16_t* qkv, const int* cu_seqlens, bf16_t* out, float* lse2, int T, int B,
                            int max_seqlen, int heads, double p, uint64_t seed, hipStream_t st);
void launch_attn_varlen_bwd(const bf16_t* qkv, const int* cu_seqlens, const bf16_t* o, const bf16_t* dout,
                            const float* lse2, bf16_t* dqkv, float* dbias, int T, int B, int max_seqlen, int heads,
                            double p, uint64_t seed, hipStream_t st);
}  // namespace hsd

namespace hsd {
// gemm.hip — la: 0 A[M][K], 1 A[K][M];  lb: 0 B[N][K], 1 B[K][N];  epi: see gemm.hip Epi
void launch_gemm(int la, int lb, int epi, const bf16_t* A, int64_t lda, const bf16_t* B, int64_t ldb, int M, int N,
                 int K, void* C, int64_t ldc, const bf16_t* bias, const bf16_t* aux, int64_t ldaux, bf16_t* C2,
                 double p_drop, uint64_t seed, int splits, hipStream_t st, uint32_t row_mul = 1);
// device step seed for dropout (common.h g_dropout_dev_seed); nullptr = off
void set_dropout_dev_seed(const uint32_t* p);
// HSD_* knobs are cached per generation (common.h HSD_KNOB); this re-reads them at their next use
void refresh_env_knobs();
// fp32.hip: the fp32 (reference precision) step -- split-product operands for the bf16 MFMA GEMMs, fp32 epilogues,
// LayerNorm, embeddings, streaming attention, classification head (ops/hip32.py)
void launch_split3(const float* x, bf16_t* out, int64_t R, int64_t C, int pat, bool rows, hipStream_t st,
                   bf16_t* out2 = nullptr, int pat2 = 0);
void launch_epi32(float* y, const float* bias, const float* aux, float* out, int64_t M, int N, int kind, double p,
                  uint64_t seed, hipStream_t st, bf16_t* hi = nullptr, bf16_t* lo = nullptr);
void launch_dropout32(const float* x, float* out, int64_t n, int W, double p, uint64_t seed, hipStream_t st,
                      bf16_t* hi = nullptr, bf16_t* lo = nullptr);
void launch_colsum32(const float* x, float* dbias, int M, int N, hipStream_t st);
void launch_ln32_fwd(const float* x, const float* g, const float* b, float* out, float* mean, float* rstd, int R,
                     int H, float eps, hipStream_t st, bf16_t* hi = nullptr, bf16_t* lo = nullptr);
void launch_ln32_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* g, float* dx,
                     float* dg, float* db, int R, int H, hipStream_t st);
void launch_embed32_gather(const int64_t* ids, const int64_t* pids, const int64_t* tids, const float* word,
                           const float* pos, const float* type, float* x, int R, int H, hipStream_t st);
void launch_embed32_scatter(const float* dx, const int64_t* ids, const int64_t* pids, const int64_t* tids,
                            float* gword, float* gpos, float* gtype, int R, int H, hipStream_t st);
void launch_attn32_fwd(const float* qkv, const float* mask, float* out, float* lse, int B, int S, int heads, double p,
                       uint64_t seed, hipStream_t st);
void launch_attn32_bwd(const float* qkv, const float* mask, const float* o, const float* dout, const float* lse,
                       float* dqkv, float* delta, int B, int S, int heads, double p, uint64_t seed, hipStream_t st);
void launch_attn32_delta(const float* o, const float* dout, float* delta, int B, int S, int heads, hipStream_t st);
// fp32 attention on split bf16 MFMA products (attention32m.hip)
bool attn32m_supported(int S, int head_dim);
void launch_split2(const float* x, bf16_t* hi, bf16_t* lo, int64_t n, hipStream_t st);
void launch_attn32m_fwd(const bf16_t* qkv_hi, const bf16_t* qkv_lo, const float* mask, float* out, float* lse2, int B,
                        int S, int heads, double p, uint64_t seed, hipStream_t st);
void launch_attn32m_bwd(const bf16_t* qkv_hi, const bf16_t* qkv_lo, const bf16_t* do_hi, const bf16_t* do_lo,
                        const float* mask, const float* lse2, const float* delta, float* dqkv, int B, int S, int heads,
                        double p, uint64_t seed, hipStream_t st);
void launch_cls32_fwd(const float* pre, const float* W2, const float* b2, const int64_t* labels, float* t_out,
                      float* logits, float* stats, int R, int H, int C, int act, double p, uint64_t seed,
                      hipStream_t st);
void launch_cls32_bwd(const float* pre, const float* t_in, const float* W2, const float* logits,
                      const int64_t* labels, const float* dloss, float* dpre, float* dW2, float* db2, int R, int H,
                      int C, int act, double p, uint64_t seed, hipStream_t st);
// contention emulation: `blocks` workgroups holding one whole CU each (160 KiB LDS) for `usec` us
void launch_cu_hog(int blocks, double usec, hipStream_t st);

// fp8.hip
void launch_fp8_quant(const bf16_t* x, int64_t n, float* amax, uint8_t* q, float* sinv, int fmt, bool compute_amax,
                      float* amax_track, hipStream_t st);
void launch_fp8_quant_many(const int64_t* amax_desc, int n_amax, int amax_blocks, const int64_t* quant_desc,
                           int n_quant, int quant_blocks_total, float* amax, float* sinv, int fmt, hipStream_t st);
int fp8_elems_per_block();
void attn_set_force_generic(bool on);  // tests: every S on the tiled generic attention kernels
void attn128_set_diag(void* p);  // diagnostic phase stamps of the S=128 attention backward ([B*heads][8] u64)

// ---- MFMA GEMMs (gemm2.hip, gemm8.hip). The launch policy is gemm_plan.h: the *_supported / *_splits / *_ws_numel
// functions are thin reads of a plan; a launcher given `planned` runs that plan instead of planning again. -----------
int gemm_num_cus();  // CUs of the current device (256 without one)
void gemm2_set_diag(void* p);  // diagnostic timestamps of the persistent NT kernel ([grid][64][4] u64), nullptr = off
// gemm2.hip — 256-row-tile 8-phase MFMA GEMM: (0,0) / (0,1) NT bf16 out with the bf16 epilogues; (0,x) epi 7: fp32 NT
// out; (1,1) TT fp32 out (epi 6 = atomics, 7 = in place, or split-K slabs in `ws` + reduce into C)
void launch_gemm2(int la, int lb, int epi, const bf16_t* A, int64_t lda, const bf16_t* B, int64_t ldb, int M, int N,
                  int K, void* C, int64_t ldc, const bf16_t* bias, const bf16_t* aux, int64_t ldaux, bf16_t* C2,
                  double p_drop, uint64_t seed, int splits, float* ws, float* dbias, hipStream_t st,
                  float* rd = nullptr, int rd_seq = 0, const GemmPlan* planned = nullptr, uint32_t row_mul = 1);
bool gemm2_supported(int la, int lb, int epi, int M, int N, int K);
int gemm2_wgrad_splits(int M, int N, int K);
int gemm2_nt_splits(int M, int N, int K);
int gemm2_f32nt_splits(int M, int N, int K);
// segmented-K fp32-output GEMMs over bf16 hi / lo operand halves (the fp32 step's split products)
bool gemm2_seg_supported(int la, int lb, int M, int N, int Kseg);
int64_t gemm2_seg_ws_numel(int la, int lb, int M, int N, int Kseg);
void launch_gemm2_seg(int la, int lb, const bf16_t* const A[3], int64_t lda, const bf16_t* const B[3], int64_t ldb,
                      int M, int N, int Kseg, float* C, int64_t ldc, float* ws, hipStream_t st, bool accumulate = false);
// fp8 NT (gemm8.hip; gemm2.hip gemm8pk_kernel)
bool gemm8_supported(int epi, int M, int N, int K);
void launch_gemm8(int epi, const uint8_t* A, int64_t lda, int fa, const float* sa, const uint8_t* B, int64_t ldb,
                  int fb, const float* sb, int M, int N, int K, bf16_t* C, int64_t ldc, const bf16_t* bias,
                  const bf16_t* aux, int64_t ldaux, bf16_t* C2, double p_drop, uint64_t seed, float* dbias,
                  hipStream_t st, uint8_t* q8 = nullptr, const float* q8_amax = nullptr, float* q8_sinv = nullptr,
                  float* q8_track = nullptr, int q8_fmt = 0, float* rd = nullptr, int rd_seq = 0,
                  int q8_only = 0, const GemmPlan* planned = nullptr);
// fp8 TT weight gradient (gemm2.hip gemm8tt_kernel + slab_reduce): C[M][N] (fp32) += sdy·sx · dY8ᵀ · X8
bool gemm8_wgrad_supported(int M, int N, int T);
int gemm8_wgrad_splits(int M, int N, int T);
int64_t gemm8_wgrad_ws_numel(int M, int N, int T, int splits);
void launch_gemm8_wgrad(const uint8_t* dy, int64_t ldd, int fdy, const float* sdy, const uint8_t* x, int64_t ldx,
                        int fx, const float* sx, int M, int N, int T, float* C, int64_t ldc, int splits, float* ws,
                        hipStream_t st);
}  // namespace hsd
