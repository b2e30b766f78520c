"""Op dispatch: one API, two implementations.

* CUDA (=HIP on ROCm) tensors -> hand-written gfx950 kernels in ``csrc/kernels`` via
  :mod:`.hip` (custom autograd Functions). If the compiled extension is missing on a GPU box this
  raises — there is no silent eager fallback.
* fp32 GPU tensors (``--dtype fp32``, the reference's own precision) -> :mod:`.hip32` (fp32 kernels in
  ``csrc/kernels/fp32.hip`` + split-product MFMA GEMMs).
* CPU tensors -> :mod:`.reference` (plain torch; also the numerics oracle for the kernel tests).

``HSD_OPS=torch`` forces the reference path on GPU (only for A/B measurements of the kernels); ``HSD_FP32_OPS=torch``
does so for fp32 tensors only. ``HSD_CLS_ROWS_ONLY=0`` keeps the last encoder layer of a sequence-classification
model on all rows (:func:`attn_block_cls`; tests and same-process A/Bs). ``HSD_TOKEN_HEAD=composed`` runs the
token-classification head (:func:`token_head`) as composed ops instead of its fused kernels (A/B measurements);
``HSD_QA_HEAD=composed`` does the same for the question-answering head (:func:`qa_head`), ``HSD_SEQ_HEAD=composed``
for the sequence-level head of ``--problem_type`` (:func:`cls_head` beyond single-label heads of at most 4 classes).

``label_smoothing`` (``--label_smoothing_factor``; :func:`cross_entropy`, :func:`cls_head`, :func:`token_head`,
:func:`mlm_head`, :func:`mlm_head_fixed`): ε in [0, 1), the target of every CE row becomes ``(1-ε)·onehot + ε/C`` over
the C real classes (definition: ``reference.cross_entropy``). On the HIP path ε is a host constant of the launch that
selects the kernels' smoothed template instantiations; ε = 0 dispatches exactly as a call without the keyword.
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from . import reference as _ref

_FORCE_TORCH = os.environ.get("HSD_OPS", "").lower() == "torch"
_FP32_TORCH = os.environ.get("HSD_FP32_OPS", "").lower() == "torch"
# the last encoder layer of a sequence-classification model on its first-token rows only (attn_block_cls)
CLS_ROWS_ONLY = os.environ.get("HSD_CLS_ROWS_ONLY", "1").strip().lower() not in ("0", "off", "false")
# HSD_TOKEN_HEAD=composed: the token-classification head as dropout -> linear -> cross_entropy instead of the fused
# kernels of csrc/kernels/token_head.hip (A/B measurements)
TOKEN_HEAD_FUSED = os.environ.get("HSD_TOKEN_HEAD", "fused").strip().lower() != "composed"
# HSD_QA_HEAD=composed: the question-answering head as dropout -> linear -> masked span cross-entropy in torch instead
# of the fused kernels of csrc/kernels/qa_head.hip (A/B measurements)
QA_HEAD_FUSED = os.environ.get("HSD_QA_HEAD", "fused").strip().lower() != "composed"
# HSD_SEQ_HEAD=composed: the sequence-level head of --problem_type (and of single-label heads with 5..64 classes) as
# composed ops + reference.seq_loss instead of the fused kernels of csrc/kernels/seq_head.hip (A/B measurements)
SEQ_HEAD_FUSED = os.environ.get("HSD_SEQ_HEAD", "fused").strip().lower() != "composed"


def _hip(x: torch.Tensor) -> bool:
    # bf16 / fp8 steps: the HIP kernels of ops/hip.py
    return x.is_cuda and not _FORCE_TORCH and x.dtype != torch.float32


def _hip32(x: torch.Tensor) -> bool:
    # fp32 steps (``--dtype fp32``, the reference's own precision: scripts/train.py:113-123 has no mixed-precision
    # policy): the fp32 kernels of ops/hip32.py
    return x.is_cuda and not _FORCE_TORCH and not _FP32_TORCH and x.dtype == torch.float32


def _hipmod():
    from . import hip  # noqa: WPS433 (lazy: imports the compiled extension)

    return hip


def _hip32mod():
    from . import hip32  # noqa: WPS433

    return hip32


def key_mask_bias(attention_mask: Optional[torch.Tensor]):
    if attention_mask is not None and attention_mask.is_cuda and not _FORCE_TORCH and \
            attention_mask.dtype in (torch.int64, torch.int32):
        return _hipmod().key_mask_bias(attention_mask)
    return _ref.key_mask_bias(attention_mask)


def dropout(x: torch.Tensor, p: float, seed: int):
    if p <= 0.0:
        return x
    if _hip(x):
        return _hipmod().dropout(x, p, seed)
    if _hip32(x):
        return _hip32mod().dropout(x, p, seed)
    return _ref.dropout(x, p, seed, True)


def embed_ln(input_ids, position_ids, token_type_ids, word_w, pos_w, type_w, ln_w, ln_b, eps, p, seed,
             pos_is_arange=False, q8_for=None):
    if _hip(word_w):
        return _hipmod().embed_ln(input_ids, position_ids, token_type_ids, word_w, pos_w, type_w, ln_w, ln_b,
                                  eps, p, seed, pos_is_arange, q8_for)
    if _hip32(word_w) and word_w.shape[1] % 4 == 0 and word_w.shape[1] <= 1024:
        return _hip32mod().embed_ln(input_ids, position_ids, token_type_ids, word_w, pos_w, type_w, ln_w, ln_b,
                                    eps, p, seed)
    return _ref.embed_ln(input_ids, position_ids, token_type_ids, word_w, pos_w, type_w, ln_w, ln_b, eps, p, seed,
                         p > 0)


def linear(x, w, b):
    if _hip(x):
        return _hipmod().linear(x, w, b)
    if _hip32(x):
        return _hip32mod().linear(x, w, b)
    return _ref.linear(x, w, b)


def linear_gelu(x, w, b):
    if _hip(x):
        return _hipmod().linear_gelu(x, w, b)
    if _hip32(x):
        return _hip32mod().linear_gelu(x, w, b)
    return _ref.linear_gelu(x, w, b)


def layer_norm(x, w, b, eps):
    if _hip(x):
        return _hipmod().layer_norm(x, w, b, eps)
    if _hip32(x) and x.shape[-1] % 4 == 0 and x.shape[-1] <= 1024:
        return _hip32mod().layer_norm(x, w, b, eps)
    return _ref.layer_norm(x, w, b, eps)


def dense_residual_ln(x, w, b, residual, ln_w, ln_b, eps, p, seed, row_mul=1):
    """``LN(dropout(x Wᵀ + b) + residual)`` — the post-LN block tail. ``row_mul``: row r is row ``r * row_mul`` of the
    dropout site (ops/rng.py keep_mask)."""
    if _hip(x):
        return _hipmod().dense_residual_ln(x, w, b, residual, ln_w, ln_b, eps, p, seed, row_mul)
    if row_mul == 1 and _hip32(x) and w.shape[0] % 4 == 0 and w.shape[0] <= 1024:
        return _hip32mod().dense_residual_ln(x, w, b, residual, ln_w, ln_b, eps, p, seed)
    return _ref.layer_norm(_ref.linear_dropout_residual(x, w, b, residual, p, seed, p > 0, row_mul), ln_w, ln_b, eps)


def attn_block_cls_ok(h, qkv_w, batch, seq, heads) -> bool:
    """Whether :func:`attn_block_cls` takes these tensors (``models.bert.Encoder`` asks before it prunes the last
    layer): an even S, and either the reference ops (CPU tensors, ``HSD_OPS=torch``) or the bf16 HIP ops with fp8 off
    (``ops/hip.py attn_block_cls_ok``). fp32 GPU tensors keep the full layer."""
    if seq % 2:
        return False
    if not h.is_cuda or _FORCE_TORCH:
        return True
    return _hip(h) and _hipmod().attn_block_cls_ok(h, qkv_w, batch, seq, heads)


def attn_block_cls(h, qkv_w, qkv_b, out_w, out_b, ln_w, ln_b, eps, mask_bias, batch, seq, heads, p_attn, seed_attn,
                   p_hidden, seed_hidden):
    """:func:`attn_block` for the first-token row of each sequence only: ``h [B·S, H]`` -> ``[B, H]``, the rows
    ``b·S`` of what :func:`attn_block` returns (same function, same dropout bits; bf16 / fp32 rounding differs). The
    last encoder layer of a sequence-classification model: its head reads nothing else. K and V are computed at
    every position, everything after the scores for one query per sequence; the hidden dropout draws row ``b·S`` of
    the ``[B·S, H]`` site (``row_mul = seq``)."""
    if _hip(h):
        return _hipmod().attn_block_cls(h, qkv_w, qkv_b, out_w, out_b, ln_w, ln_b, eps, mask_bias, batch, seq, heads,
                                        p_attn, seed_attn, p_hidden, seed_hidden)
    qkv = _ref.linear(h.reshape(batch * seq, -1), qkv_w, qkv_b)
    ctx0 = _ref.attention_cls(qkv, mask_bias, batch, seq, heads, p_attn, seed_attn, p_attn > 0)
    x0 = h.reshape(batch, seq, -1)[:, 0]
    z = _ref.linear_dropout_residual(ctx0, out_w, out_b, x0, p_hidden, seed_hidden, p_hidden > 0, seq)
    return _ref.layer_norm(z, ln_w, ln_b, eps)


def attn_block(h, qkv_w, qkv_b, out_w, out_b, ln_w, ln_b, eps, mask_bias, batch, seq, heads, p_attn, seed_attn,
               p_hidden, seed_hidden, q8_next=None, *, cu_seqlens=None, max_seqlen=0):
    """Self-attention sub-block: ``LN(dropout(attn(h Wqkvᵀ + b) Woᵀ + bo) + h)``. ``q8_next``: the weight of the
    GEMM that consumes the output (HIP fp8 path: the LayerNorm writes its fp8 input copy).

    ``cu_seqlens`` (with ``max_seqlen``): ``h`` is a packed ``[T, H]`` buffer (data/packing.py) and the block is the
    three-op composition below around ``attention_varlen``; ``mask_bias`` / ``batch`` / ``seq`` are not read."""
    if cu_seqlens is not None:
        if mask_bias is not None:
            raise ValueError("attn_block: a packed batch (cu_seqlens) takes no attention mask")
        qkv = linear(h, qkv_w, qkv_b)
        ctx = attention_varlen(qkv, cu_seqlens, max_seqlen, heads, p_attn, seed_attn)
        return dense_residual_ln(ctx, out_w, out_b, h, ln_w, ln_b, eps, p_hidden, seed_hidden)
    if _hip(h) and h.dtype == torch.bfloat16 and qkv_w.shape[0] == 3 * heads * 64 and seq % 2 == 0:
        # (an odd sequence length: the three ops below, with the reference attention -- ops/hip.py attention_ok)
        return _hipmod().attn_block(h, qkv_w, qkv_b, out_w, out_b, ln_w, ln_b, eps, mask_bias, batch, seq, heads,
                                    p_attn, seed_attn, p_hidden, seed_hidden, q8_next)
    if _hip32(h) and _hip32mod().attn_block_ok(h, qkv_w, seq, heads):
        return _hip32mod().attn_block(h, qkv_w, qkv_b, out_w, out_b, ln_w, ln_b, eps, mask_bias, batch, seq, heads,
                                      p_attn, seed_attn, p_hidden, seed_hidden)
    qkv = linear(h, qkv_w, qkv_b)
    ctx = attention(qkv, mask_bias, batch, seq, heads, p_attn, seed_attn)
    return dense_residual_ln(ctx, out_w, out_b, h, ln_w, ln_b, eps, p_hidden, seed_hidden)


def ffn_block(h, w1, b1, w2, b2, ln_w, ln_b, eps, p, seed, q8_next=None, drop_row_mul=1):
    """Feed-forward sub-block: ``LN(dropout(gelu(h W1ᵀ + b1) W2ᵀ + b2) + h)``. ``drop_row_mul``: row r of ``h`` is row
    ``r * drop_row_mul`` of the dropout site (the first-token rows after :func:`attn_block_cls`)."""
    if _hip(h) and h.dtype == torch.bfloat16:
        return _hipmod().ffn_block(h, w1, b1, w2, b2, ln_w, ln_b, eps, p, seed, q8_next, drop_row_mul)
    if drop_row_mul == 1 and _hip32(h) and _hip32mod().ffn_block_ok(h, w1):
        return _hip32mod().ffn_block(h, w1, b1, w2, b2, ln_w, ln_b, eps, p, seed)
    a = linear_gelu(h, w1, b1)
    return dense_residual_ln(a, w2, b2, h, ln_w, ln_b, eps, p, seed, drop_row_mul)


def attention(qkv, mask_bias, batch, seq, heads, p, seed):
    if _hip(qkv):
        return _hipmod().attention(qkv, mask_bias, batch, seq, heads, p, seed)
    if _hip32(qkv):
        return _hip32mod().attention(qkv, mask_bias, batch, seq, heads, p, seed)
    return _ref.attention(qkv, mask_bias, batch, seq, heads, p, seed, p > 0)


def attention_varlen(qkv, cu_seqlens, max_seqlen, heads, p, seed):
    """Attention over packed sequences (``--pack_sequences``): bf16 GPU tensors run the varlen HIP kernels,
    everything else the reference op."""
    if _hip(qkv) and qkv.dtype == torch.bfloat16:
        return _hipmod().attention_varlen(qkv, cu_seqlens, max_seqlen, heads, p, seed)
    return _ref.attention_varlen(qkv, cu_seqlens, max_seqlen, heads, p, seed, p > 0)


def hip_active(device) -> bool:
    """True when tensors on ``device`` run the HIP kernels (not the reference ops)."""
    return torch.device(device).type == "cuda" and not _FORCE_TORCH


def set_fp8(on: bool, grad_fmt: str = "e4m3") -> None:
    """Route the encoder's forward / dgrad GEMMs through the fp8 kernel (weights need fp8 copies:
    ``FlatParamStore(..., fp8=True)``)."""
    _hipmod().set_fp8(on, grad_fmt)


def join_side_streams() -> None:
    """Order the current stream after the wgrad side stream (no-op on CPU / reference ops)."""
    if torch.cuda.is_available() and not _FORCE_TORCH:
        _hipmod().join_side_streams()


def _with_stats(loss, stats, pred=None):
    """The attribute protocol of the fused heads: ``loss._hsd_stats`` = the head's device stats (the metric meter folds
    them lazily) with the argmax hits on ``loss._hsd_correct``, or, for a span head, its best spans on
    ``loss._hsd_pred``."""
    loss._hsd_stats = stats
    if pred is None:
        loss._hsd_correct = stats[1]
    else:
        loss._hsd_pred = pred
    return loss


def _smoothing(label_smoothing) -> float:
    eps = float(label_smoothing)
    if not 0.0 <= eps < 1.0:  # NaN fails both comparisons
        raise ValueError(f"label_smoothing {label_smoothing!r}: 0 <= label_smoothing < 1")
    return eps


def _sum_ce(logits, tgt, n=None, label_smoothing: float = 0.0):
    """Composed CE: ``Σ CE / max(n, 1)`` over the rows whose target is not -100, carrying {mean loss, hits, n, loss
    sum}. ``n``: the number of such rows as a device fp32 scalar (counted here when not given). ``label_smoothing``:
    the smoothed CE of ``reference.cross_entropy``."""
    lsum = torch.nn.functional.cross_entropy(logits.float(), tgt, ignore_index=-100, reduction="sum",
                                             label_smoothing=float(label_smoothing))
    with torch.no_grad():
        ok = tgt.ne(-100)
        if n is None:
            n = ok.sum().to(torch.float32)
        hits = ((logits.argmax(dim=-1) == tgt) & ok).sum().to(torch.float32)
    loss = lsum / n.clamp(min=1.0)
    with torch.no_grad():
        stats = torch.stack([loss.detach().float(), hits, n, lsum.detach().float()])
    return _with_stats(loss, stats)


def cross_entropy(logits, labels, label_smoothing: float = 0.0):
    """Mean CE over non-ignored labels. On the HIP path the fused kernel also counts argmax hits; the count
    rides on the loss tensor (``loss._hsd_correct``) so metrics need no second pass over the logits.

    ``label_smoothing`` ε > 0: the smoothed CE, on the smoothed instantiation of the same kernel; fp32 GPU logits (the
    composed fp32 heads) take that kernel too (``xent_kernel<false, true>``)."""
    eps = _smoothing(label_smoothing)
    if _hip(logits) or (eps > 0.0 and _hip32(logits) and logits.dim() == 2):
        loss, correct = _hipmod().cross_entropy(logits, labels, eps)
        loss._hsd_correct = correct
        return loss
    return _ref.cross_entropy(logits, labels, eps)


def cls_head(h, w1, b1, w2, b2, labels, act: str, p_in: float, seed_in: int, p: float, seed: int, *,
             problem_type: Optional[str] = None, tol: float = 0.5, label_smoothing: float = 0.0):
    """Classification head on the first token of ``h`` [B, S, H] (+ the loss when ``labels`` is given). ``S`` is 1 when
    the encoder already pruned its last layer to the first-token rows (``Encoder.forward(first_token_only=True)``).

    Returns ``logits`` without labels, else ``(loss, logits)`` with the argmax-hit count on ``loss._hsd_correct``
    and the fused {mean loss, hits, rows, loss sum} on ``loss._hsd_stats`` (HIP path). On GPUs the dense layer runs on gemm2 and everything after it (activation, dropout, classifier, CE,
    accuracy) in one fused kernel per direction (csrc/kernels/cls_head.hip); the first-token rows are read in place
    (no gather copy) and their gradient is written straight into the zeroed ``dh`` rows.

    ``problem_type`` (HF ``config.problem_type``; ``None`` = single-label): ``"multi_label_classification"`` and
    ``"regression"`` take fp32 labels ``[B, C]`` (a row whose first label is NaN is ignored) and return the loss of
    ``reference.seq_loss`` with its {mean loss, hits, n, loss sum} on ``loss._hsd_stats`` on every path; ``tol`` is
    the regression hit tolerance. bf16 GPU tensors within ``hip.seq_head_ok`` (H % 8 == 0, H <= 1024, C <= 64) run
    csrc/kernels/seq_head.hip for both and for single-label heads of 5..64 classes, unless ``HSD_SEQ_HEAD=composed``;
    everything else runs the composed ops with the same seeds and so the same masks.

    ``label_smoothing`` ε > 0 (single-label only; the other two types refuse it): the smoothed CE. cls_head.hip and the
    fp32 fused tail have no smoothed form, so single-label bf16 heads of 1..64 classes all run seq_head.hip's smoothed
    instantiations and fp32 GPU heads the composed ops with :func:`cross_entropy` on the smoothed CE kernel. With
    ε = 0 the dispatch is the one above."""
    if problem_type not in (None,) + _ref.PROBLEM_TYPES:
        raise ValueError(f"problem_type {problem_type!r}: one of {_ref.PROBLEM_TYPES} or None")
    single = problem_type in (None, "single_label_classification")
    eps = _smoothing(label_smoothing)
    if eps > 0.0 and not single:
        raise ValueError(f"label_smoothing is for single-label classification, not problem_type {problem_type!r}")
    mod = _hipmod() if _hip(h) else _hip32mod() if _hip32(h) else None
    if eps == 0.0 and single and mod is not None and labels is not None and mod.cls_head_ok(h, w1, w2):
        loss, logits, stats = mod.cls_head(h, w1, b1, w2, b2, labels, act, p_in, seed_in, p, seed)
        return _with_stats(loss, stats), logits
    if _hip(h) and SEQ_HEAD_FUSED and labels is not None and _hipmod().seq_head_ok(h, w1, w2):
        loss, logits, stats = _hipmod().seq_head(h, w1, b1, w2, b2, labels, act, p_in, seed_in, p, seed,
                                                 problem_type, tol, eps)
        return _with_stats(loss, stats), logits
    x = h[:, 0].contiguous()
    if _hip(h) or _hip32(h):
        x = dropout(x, p_in, seed_in)
        y = linear(x, w1, b1)
        y = torch.tanh(y) if act == "tanh" else torch.relu(y)
        y = dropout(y, p, seed)
        C = w2.shape[0]
        if _hip32(h) and C % 4:
            # the fp32 GEMM epilogue takes whole groups of 4 columns (smoothed heads come here with any C): classes of
            # zeros pad the classifier and their logits are cut off again, so they reach neither loss nor gradient
            pad = 4 - C % 4
            logits = linear(y, torch.cat([w2, w2.new_zeros(pad, w2.shape[1])]), torch.cat([b2, b2.new_zeros(pad)]))
            logits = logits[:, :C].contiguous()
        else:
            logits = linear(y, w2, b2)
    else:
        logits = _ref.cls_head(x, w1, b1, w2, b2, act, p_in, seed_in, p, seed, True)
    if labels is None:
        return logits
    if single and problem_type is None:
        return cross_entropy(logits, labels, eps), logits
    loss, stats = _ref.seq_loss(logits, labels, problem_type, tol, eps)
    return _with_stats(loss, stats), logits


def token_head(h2d, w, b, labels, p: float, seed: int, label_smoothing: float = 0.0):
    """Token-classification head on every row of ``h2d`` [R, H]: ``logits = dropout(h) Wᵀ + b`` [R, C] and, with
    ``labels`` [R], the CE over the rows whose label is not -100 divided by ``max(n_valid, 1)`` (0 when every row is
    ignored). Returns ``logits`` without labels, else ``(loss, logits)`` with the fused {mean loss, hits, n_valid,
    loss sum} on ``loss._hsd_stats`` and the hits on ``loss._hsd_correct`` (every path: nothing reads a device value
    on the host).

    bf16 GPU tensors within ``hip.token_head_ok`` (H % 8 == 0, H <= 1024, 2 <= C <= 16) run the fused kernels of
    csrc/kernels/token_head.hip, unless ``HSD_TOKEN_HEAD=composed``. Everything else (CPU tensors, fp32 GPU tensors,
    ``HSD_OPS=torch``, other shapes) runs the composed ``dropout -> linear -> cross_entropy`` with the same seed and
    so the same mask; the all-torch form of it is ``reference.token_head``, the kernels' oracle.

    ``label_smoothing`` ε > 0: the smoothed CE on every path (the fused kernels' smoothed instantiations, ``_sum_ce``,
    ``reference.token_head``)."""
    eps = _smoothing(label_smoothing)
    lab = labels.reshape(-1) if labels is not None else None
    needs_grad = torch.is_grad_enabled() and (h2d.requires_grad or w.requires_grad or b.requires_grad)
    if _hip(h2d) and TOKEN_HEAD_FUSED and _hipmod().token_head_ok(h2d, w) and not (lab is None and needs_grad):
        if lab is None:  # inference: the fused forward alone (differentiable logits take the composed ops below)
            return _hipmod().token_head_logits(h2d, w, b, p, seed)
        loss, logits, stats = _hipmod().token_head(h2d, w, b, lab, p, seed, eps)
        return _with_stats(loss, stats), logits
    if _hip(h2d) or (_hip32(h2d) and w.shape[0] % 4 == 0):  # (the fp32 GEMM epilogue takes whole groups of 4 columns)
        logits = linear(dropout(h2d, p, seed), w, b)
        return logits if lab is None else (_sum_ce(logits, lab.long(), None, eps), logits)
    out = _ref.token_head(h2d, w, b, lab, p, seed, True, eps)
    if lab is None:
        return out
    loss, logits, stats = out
    return _with_stats(loss, stats), logits


def qa_head(h2d, w, b, positions, cu, row_mask, p: float, seed: int, max_answer_length: int = 30, max_seqlen=None):
    """Question-answering (span extraction) head on every row of ``h2d`` [R, H]: ``logits = dropout(h) Wᵀ + b``
    [R, 2] (start, end) and the span loss over the sequences ``cu[b] .. cu[b+1]-1`` of the flat buffer, with
    ``row_mask`` [R] taking rows out (padded batches: ``cu = arange(B+1)·S`` and the flat attention mask; packed ones:
    ``cu_seqlens``, no mask). ``positions`` [B, 2] (start, end) count from the sequence's first row; the definition of
    the loss, of an ignored position and of the best span is ``reference.span_loss`` / ``span_best``.

    With ``positions`` returns ``(loss, logits)`` with the fp32 [8] {loss, hits, n, loss·n, n_start, n_end, start hits,
    end hits} on ``loss._hsd_stats`` and the best spans (int32 [B, 2]) on ``loss._hsd_pred``; without them
    ``(logits, pred)``. ``max_seqlen``: the longest sequence as a host int, if the caller knows it.

    bf16 GPU tensors within ``hip.qa_head_ok`` (H % 8 == 0, H <= 1024, sequences of at most 1,024 rows) run the fused
    kernels of csrc/kernels/qa_head.hip and token_head.hip, unless ``HSD_QA_HEAD=composed``. Everything else (CPU
    tensors, fp32 GPU tensors, ``HSD_OPS=torch``, other shapes) runs the composed ops with the same seed and so the
    same mask; the all-torch form is ``reference.qa_head``, the kernels' oracle."""
    needs_grad = torch.is_grad_enabled() and (h2d.requires_grad or w.requires_grad or b.requires_grad)
    if _hip(h2d) and QA_HEAD_FUSED and _hipmod().qa_head_ok(h2d, w, cu, max_seqlen) \
            and not (positions is None and needs_grad):
        if positions is None:
            return _hipmod().qa_head_logits(h2d, w, b, cu, row_mask, p, seed, max_answer_length)
        loss, logits, stats, pred = _hipmod().qa_head(h2d, w, b, positions, cu, row_mask, p, seed, max_answer_length)
    elif _hip(h2d):
        logits = linear(dropout(h2d, p, seed), w, b)
        if positions is None:
            return logits, _ref.span_best(logits, cu, row_mask, max_answer_length, max_seqlen)
        loss, stats, pred = _ref.span_loss(logits, positions, cu, row_mask, max_answer_length, max_seqlen)
    else:
        out = _ref.qa_head(h2d, w, b, positions, cu, row_mask, p, seed, max_answer_length, True, max_seqlen)
        if positions is None:
            return out
        loss, logits, stats, pred = out
    return _with_stats(loss, stats, pred), logits


def mlm_head(h2d, labels, w1, b1, ln_w, ln_b, eps, wemb, bias, vocab, label_smoothing: float = 0.0):
    """Masked-LM head (RoBERTa) on the masked rows of ``h2d`` -> (loss, logits over the real vocabulary).

    GPU: every GEMM on gemm2 (dense + GELU epilogue, LN kernel, the tied decoder over the 256-padded vocabulary, its
    dgrad reading the embedding table directly and the embedding-table weight gradient), the chunked-vocabulary CE
    kernel; the argmax-hit count rides on ``loss._hsd_correct``. ``label_smoothing``: the smoothed CE over the
    ``vocab`` real classes; the padding columns of the decoder keep an exactly zero gradient."""
    ls = _smoothing(label_smoothing)
    if _hip(h2d) and h2d.dtype == torch.bfloat16 and _hipmod().mlm_head_ok(h2d, w1, wemb):
        loss, logits, correct = _hipmod().mlm_head(h2d, labels, w1, b1, ln_w, ln_b, eps, wemb, bias, vocab, ls)
        loss._hsd_correct = correct
        return loss, logits
    if _hip(h2d):
        sel = labels.ne(-100).nonzero(as_tuple=True)[0]
        x = h2d.index_select(0, sel)
        x = layer_norm(linear_gelu(x, w1, b1), ln_w, ln_b, eps)
        logits = linear(x, wemb[:vocab], bias[:vocab])
        return cross_entropy(logits, labels.index_select(0, sel), ls), logits
    return _ref.mlm_head(h2d, labels, w1, b1, ln_w, ln_b, eps, wemb, bias, vocab, ls)


def mlm_mask(input_ids, attention_mask, labels_in, seed, p, mask_id, special_ids, rand_range, cap=None,
             use_step_seed=True):
    """Dynamic MLM masking (``--mlm_masking dynamic``; definition: ops/rng.py "MLM mask"): a fresh 80 / 10 / 10 draw
    over the maskable tokens of the flat id buffer, compacted in order into fixed-capacity buffers. Returns an
    :class:`ops.rng.MlmMask` (``input_ids``, ``labels``, ``sel``, ``tgt``, ``inv``, ``counts``, ``n_valid``, ``cap``).

    GPU tensors: the HIP kernels (two launches, no host sync; ``use_step_seed`` folds the device step seed of a
    graph-enabled trainer in, as the dropout kernels do). CPU tensors, and ``HSD_OPS=torch``: the torch reference."""
    if input_ids.is_cuda and not _FORCE_TORCH:
        return _hipmod().mlm_mask(input_ids, attention_mask, labels_in, seed, p, mask_id, special_ids, rand_range,
                                  cap, use_step_seed)
    from .rng import mlm_mask_reference

    return mlm_mask_reference(input_ids, attention_mask, labels_in, seed, p, mask_id, special_ids, rand_range, cap)


def mlm_head_fixed(h2d, mask, w1, b1, ln_w, ln_b, eps, wemb, bias, vocab, label_smoothing: float = 0.0):
    """Masked-LM head on the fixed-capacity rows of an :func:`mlm_mask` result -> (loss, logits [cap, vocab]).

    The loss is ``Σ CE / max(n, 1)`` computed on the device (0 when nothing was selected) and carries the fused
    {mean loss, hits, rows, loss sum} on ``loss._hsd_stats`` / the hits on ``loss._hsd_correct``: nothing in here reads a
    device value on the host. GPU bf16 tensors that :func:`hip.mlm_head_ok` accepts run the HIP head (the static
    head's kernels on ``cap`` rows, a row-scatter kernel for the hidden-state gradient); everything else the same
    ``(sel, tgt)`` through the composed ops. ``label_smoothing`` as in :func:`mlm_head`."""
    ls = _smoothing(label_smoothing)
    sel, tgt, n_valid = mask.sel, mask.tgt, mask.n_valid
    if _hip(h2d) and h2d.dtype == torch.bfloat16 and _hipmod().mlm_head_ok(h2d, w1, wemb):
        loss, logits, stats = _hipmod().mlm_head_fixed(h2d, sel, tgt, mask.inv, n_valid, w1, b1, ln_w, ln_b, eps, wemb,
                                                       bias, vocab, ls)
        return _with_stats(loss, stats), logits
    x = h2d.index_select(0, sel)
    if _hip(h2d) or _hip32(h2d):
        x = layer_norm(linear_gelu(x, w1, b1), ln_w, ln_b, eps)
        logits = linear(x, wemb[:vocab], bias[:vocab])
    else:
        x = _ref.layer_norm(_ref.linear_gelu(x, w1, b1), ln_w, ln_b, eps)
        logits = torch.nn.functional.linear(x, wemb[:vocab], bias[:vocab])
    return _sum_ce(logits, tgt, n_valid[0], ls), logits


def accuracy_count(logits, labels):
    return _ref.accuracy_count(logits, labels)
