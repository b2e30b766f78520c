"""Plain-PyTorch reference implementations of every fused op.

These are (a) the CPU execution path (tests, gloo plumbing runs) and (b) the numerics oracle the
HIP kernels are tested against. Math follows HF PyTorch BERT
([dep: transformers/models/bert/modeling_bert.py]) which is what the reference's TF model computes
(``scripts/train.py:117``): post-LN residual blocks, exact-erf GELU, additive key-padding mask.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as F

from .rng import keep_mask


def dropout(x: torch.Tensor, p: float, seed: int, training: bool = True, row_mul: int = 1) -> torch.Tensor:
    if not training or p <= 0.0:
        return x
    m = keep_mask(seed, x.shape, p, device=x.device, row_mul=row_mul)
    return x * m.to(x.dtype) * (1.0 / (1.0 - p))


def embed_ln(input_ids, position_ids, token_type_ids, word_w, pos_w, type_w, ln_w, ln_b,
             eps: float, p: float, seed: int, training: bool) -> torch.Tensor:
    """``dropout(LN(word[ids] + pos[pos_ids] + type[tt]))`` (modeling_bert.py BertEmbeddings)."""
    h = F.embedding(input_ids, word_w) + F.embedding(position_ids, pos_w)
    if type_w is not None:
        h = h + F.embedding(token_type_ids, type_w)
    h = F.layer_norm(h.float(), (h.shape[-1],), ln_w.float(), ln_b.float(), eps).to(word_w.dtype)
    return dropout(h, p, seed, training)


def linear(x, w, b):
    return F.linear(x, w, b)


def gelu(x):
    return F.gelu(x.float(), approximate="none").to(x.dtype)


def linear_gelu(x, w, b):
    return gelu(F.linear(x, w, b))


def linear_dropout_residual(x, w, b, residual, p: float, seed: int, training: bool, row_mul: int = 1):
    """``dropout(x Wᵀ + b) + residual`` rounded ONCE to the output dtype (fp32 product and sum), as the HIP epilogues
    compute it (gemm_common.h / gemm.hip: bf16(fma(y, keep · scale, residual)) with y = bf16(x Wᵀ + b))."""
    y = F.linear(x, w, b)
    if not training or p <= 0.0:
        return y + residual
    k = keep_mask(seed, y.shape, p, device=y.device, row_mul=row_mul).to(torch.float32) * (1.0 / (1.0 - p))
    return torch.addcmul(residual.float(), y.float(), k).to(y.dtype)


def layer_norm(x, w, b, eps: float):
    return F.layer_norm(x.float(), (x.shape[-1],), w.float(), b.float(), eps).to(x.dtype)


def key_mask_bias(attention_mask: Optional[torch.Tensor], dtype=torch.float32) -> Optional[torch.Tensor]:
    """[B,S] 0/1 mask -> additive fp32 bias [B,S] (0 keep, -inf-like mask)."""
    if attention_mask is None:
        return None
    return (1.0 - attention_mask.to(torch.float32)) * torch.finfo(torch.float32).min


def attention(qkv: torch.Tensor, mask_bias: Optional[torch.Tensor], batch: int, seq: int, heads: int,
              p: float, seed: int, training: bool) -> torch.Tensor:
    """Self-attention over a packed ``[B*S, 3H]`` QKV tensor -> ``[B*S, H]`` context.

    Dropout on the probabilities: row ``(b*heads + h)*S + i``, column ``j`` of the site's [rows, S] view (ops/rng.py).
    """
    H3 = qkv.shape[-1]
    H = H3 // 3
    d = H // heads
    x = qkv.view(batch, seq, 3, heads, d).permute(2, 0, 3, 1, 4).float()  # [3,B,h,S,d]
    q, k, v = x[0], x[1], x[2]
    s = torch.matmul(q, k.transpose(-1, -2)) * (1.0 / math.sqrt(d))
    if mask_bias is not None:
        s = s + mask_bias.view(batch, 1, 1, seq).float()
    pr = torch.softmax(s, dim=-1)
    pr = dropout(pr, p, seed, training)
    o = torch.matmul(pr, v)  # [B,h,S,d]
    return o.permute(0, 2, 1, 3).reshape(batch * seq, H).to(qkv.dtype)


def attention_cls(qkv: torch.Tensor, mask_bias: Optional[torch.Tensor], batch: int, seq: int, heads: int,
                  p: float, seed: int, training: bool) -> torch.Tensor:
    """:func:`attention` for the first query row of each sequence only: ``[B*S, 3H]`` -> ``[B, H]``. The same op
    sequence on one query, and the dropout bits :func:`attention` draws for that row: row ``(b*heads + h)*S``."""
    H3 = qkv.shape[-1]
    H = H3 // 3
    d = H // heads
    x = qkv.view(batch, seq, 3, heads, d).permute(2, 0, 3, 1, 4).float()  # [3,B,h,S,d]
    q, k, v = x[0][:, :, :1], x[1], x[2]
    s = torch.matmul(q, k.transpose(-1, -2)) * (1.0 / math.sqrt(d))  # [B,h,1,S]
    if mask_bias is not None:
        s = s + mask_bias.view(batch, 1, 1, seq).float()
    pr = torch.softmax(s, dim=-1)
    pr = dropout(pr, p, seed, training, row_mul=seq)
    o = torch.matmul(pr, v)  # [B,h,1,d]
    return o.permute(0, 2, 1, 3).reshape(batch, H).to(qkv.dtype)


def attention_varlen(qkv: torch.Tensor, cu_seqlens: torch.Tensor, max_seqlen: int, heads: int, p: float, seed: int,
                     training: bool) -> torch.Tensor:
    """Self-attention over packed sequences: ``qkv [T, 3H]`` with sequence ``b`` in rows ``cu_seqlens[b] ..
    cu_seqlens[b+1]-1`` (data/packing.py) -> ``[T, H]`` context. A query sees the keys of its own sequence only; the
    dead rows (from ``cu_seqlens[-1]`` on) come back as zeros.

    Dropout on the probabilities: head ``h``, packed row ``t``, key ``j`` within the sequence is row ``h*T + t``,
    column ``j`` of the site (ops/rng.py)."""
    T, H3 = qkv.shape
    H = H3 // 3
    d = H // heads
    cu = [int(c) for c in cu_seqlens.tolist()]
    keep = None
    if training and p > 0.0:
        keep = keep_mask(seed, (heads * T, int(max_seqlen)), p, device=qkv.device).view(heads, T, int(max_seqlen))
    outs = []
    for b in range(len(cu) - 1):
        s0, s1 = cu[b], cu[b + 1]
        L = s1 - s0
        # the same op sequence as ``attention`` on a batch of one sequence of length L (bit-identical without dropout)
        x = qkv[s0:s1].view(1, L, 3, heads, d).permute(2, 0, 3, 1, 4).float()  # [3,1,h,L,d]
        s = torch.matmul(x[0], x[1].transpose(-1, -2)) * (1.0 / math.sqrt(d))
        pr = torch.softmax(s, dim=-1)
        if keep is not None:
            pr = pr * keep[:, s0:s1, :L].unsqueeze(0).to(pr.dtype) * (1.0 / (1.0 - p))
        o = torch.matmul(pr, x[2])  # [1,h,L,d]
        outs.append(o.permute(0, 2, 1, 3).reshape(L, H).to(qkv.dtype))
    if cu[-1] < T:
        outs.append(qkv.new_zeros((T - cu[-1], H)))
    return torch.cat(outs, dim=0)


def cross_entropy(logits: torch.Tensor, labels: torch.Tensor, label_smoothing: float = 0.0) -> torch.Tensor:
    """SparseCategoricalCrossentropy(from_logits=True), SUM_OVER_BATCH_SIZE (``scripts/train.py:118``).

    ``label_smoothing`` ε in [0, 1) (HF ``LabelSmoother``, Keras ``label_smoothing=``): the target of a row is
    ``(1-ε)·onehot + ε/C`` over the C classes, so its term is ``lse - (1-ε)·z[y] - (ε/C)·Σ_c z[c]`` and its gradient
    ``softmax(z) - (1-ε)·onehot - ε/C``; ignored rows add nothing. Every CE in this module takes it the same way."""
    return F.cross_entropy(logits.float(), labels.long(), label_smoothing=float(label_smoothing))


def accuracy_count(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    return (logits.argmax(dim=-1) == labels.long()).sum()


def cls_head(x, w1, b1, w2, b2, act: str, p_in: float, seed_in: int, p: float, seed: int, training: bool):
    """Sequence-classification head on the first-token rows ``x`` [B, H] -> logits [B, C]:
    ``W2·dropout(act(W1·dropout_in(x) + b1)) + b2`` (HF BertPooler + classifier, RobertaClassificationHead,
    DistilBERT pre_classifier; act = "tanh" | "relu")."""
    x = dropout(x, p_in, seed_in, training)
    h = F.linear(x, w1, b1)
    h = torch.tanh(h) if act == "tanh" else torch.relu(h)
    h = dropout(h, p, seed, training)
    return F.linear(h, w2, b2)


PROBLEM_TYPES = ("single_label_classification", "multi_label_classification", "regression")


def seq_loss(logits, labels, problem_type: Optional[str] = None, tol: float = 0.5, label_smoothing: float = 0.0):
    """Loss and metric of the sequence-level head on ``logits`` [B, C] (HF ``*ForSequenceClassification`` with
    ``config.problem_type``) -> ``(loss, stats)``, ``stats`` = fp32 {mean loss, hits, n, loss sum}.

    * ``None`` / ``"single_label_classification"``: labels int [B]; CE over the rows whose label is not -100
      (``label_smoothing`` as in :func:`cross_entropy`; the other two types refuse a non-zero one);
      hits = first-maximum argmax == label.
    * ``"multi_label_classification"``: labels float [B, C] in [0, 1]; per element
      ``max(z,0) - z·y + log1p(exp(-|z|))`` (``BCEWithLogitsLoss``); hits = rows with ``(z > 0) == (y > 0.5)`` for
      every label (subset accuracy).
    * ``"regression"``: labels float [B, C] ([B] when C = 1); per element ``(z - y)²`` (``MSELoss``); hits = rows with
      ``|z - y| <= tol`` for every target.

    A float-label row whose FIRST label is NaN is ignored. ``n`` counts the other rows; the float losses are
    ``Σ_valid rows Σ_c term / (max(n, 1)·C)``: 0, not NaN, with zero gradients, when every row is ignored."""
    z = logits.float()
    if label_smoothing and problem_type not in (None, "single_label_classification"):
        raise ValueError(f"label_smoothing is for single-label classification, not problem_type {problem_type!r}")
    if problem_type in (None, "single_label_classification"):
        lab = labels.reshape(-1).long()
        lsum = F.cross_entropy(z, lab, ignore_index=-100, reduction="sum", label_smoothing=float(label_smoothing))
        with torch.no_grad():
            ok = lab.ne(-100)
            hits = ((z.argmax(dim=-1) == lab) & ok).sum().to(torch.float32)
    elif problem_type in ("multi_label_classification", "regression"):
        C = z.shape[-1]
        y = labels.to(torch.float32).reshape(z.shape[0], C)
        ok = ~torch.isnan(y[:, 0])
        y = torch.where(ok.unsqueeze(1), y, torch.zeros_like(y))  # no NaN reaches the graph of an ignored row
        if problem_type == "regression":
            term = (z - y) ** 2
            with torch.no_grad():
                good = ((z - y).abs() <= tol).all(dim=-1)
        else:
            term = z.clamp(min=0) - z * y + torch.log1p(torch.exp(-z.abs()))
            with torch.no_grad():
                good = ((z > 0) == (y > 0.5)).all(dim=-1)
        lsum = (term * ok.unsqueeze(1).to(term.dtype)).sum() / C
        with torch.no_grad():
            hits = (good & ok).sum().to(torch.float32)
    else:
        raise ValueError(f"problem_type {problem_type!r}: one of {PROBLEM_TYPES} or None")
    with torch.no_grad():
        n = ok.sum().to(torch.float32)
    loss = lsum / n.clamp(min=1.0)
    with torch.no_grad():
        stats = torch.stack([loss.detach().float(), hits, n, lsum.detach().float()])
    return loss, stats


def token_head(h2d, w, b, labels, p: float, seed: int, training: bool = True, label_smoothing: float = 0.0):
    """Token-classification head on every row of ``h2d`` [R, H] (HF ``*ForTokenClassification``):
    ``logits = dropout(h) Wᵀ + b`` [R, C]; the dropout site is the flat ``[R, H]`` buffer. With ``labels`` [R]
    returns ``(loss, logits, stats)``: ``loss`` = CE summed over the rows whose label is not -100, divided by
    ``max(n_valid, 1)`` (0, not NaN, when every row is ignored), and ``stats`` = fp32 {mean loss, first-maximum argmax
    hits, n_valid, loss sum}. ``label_smoothing`` as in :func:`cross_entropy`. Without labels: the logits."""
    logits = F.linear(dropout(h2d, p, seed, training), w, b)
    if labels is None:
        return logits
    lab = labels.reshape(-1).long()
    lsum = F.cross_entropy(logits.float(), lab, ignore_index=-100, reduction="sum",
                           label_smoothing=float(label_smoothing))
    with torch.no_grad():
        ok = lab.ne(-100)
        n = ok.sum().to(torch.float32)
        hits = ((logits.argmax(dim=-1) == lab) & ok).sum().to(torch.float32)
    loss = lsum / n.clamp(min=1.0)
    with torch.no_grad():
        stats = torch.stack([loss.detach().float(), hits, n, lsum.detach().float()])
    return loss, logits, stats


def span_segments(cu, rows: int, row_mask=None):
    """Rows of a flat ``[rows]`` buffer -> (sequence index ``seg`` [rows] with ``B`` on the dead rows past ``cu[B]``,
    index within the sequence ``rel`` [rows], ``real`` [rows] bool: in a sequence and not masked). No host read."""
    cu = cu.long()
    B = cu.numel() - 1
    r = torch.arange(rows, device=cu.device)
    seg = torch.searchsorted(cu[1:].contiguous(), r, right=True)
    real = (seg < B) & (r >= cu[0])
    if row_mask is not None:
        real = real & row_mask.reshape(-1).ne(0)
    rel = r - cu[seg.clamp(max=B - 1)]
    return seg, rel, real


def span_best(logits, cu, row_mask, max_answer_length: int, max_seqlen: Optional[int] = None):
    """Best span of every sequence: ``pred [B, 2]`` int32 = the first maximum, in ``(s, e)`` lexicographic order, of
    ``start[s] + end[e]`` (ONE fp32 add of the logits as stored) over the real rows with
    ``s <= e <= s + max_answer_length - 1``; ``(0, 0)`` for a sequence without a real row. ``max_seqlen``: the longest
    sequence as a host int (read from ``cu`` when it is not given)."""
    R = logits.shape[0]
    B = cu.numel() - 1
    seg, rel, real = span_segments(cu, R, row_mask)
    if max_seqlen is None:
        max_seqlen = int((cu[1:] - cu[:-1]).max())
    L = max(1, int(max_seqlen))
    ok = real & (rel < L)
    slot = torch.where(ok, seg * L + rel, torch.full_like(seg, B * L))  # one spare slot takes every other row
    x = logits.detach().float()
    pad = torch.full(((B + 1) * L,), float("-inf"), dtype=torch.float32, device=x.device)
    st = pad.scatter(0, slot, torch.where(ok, x[:, 0], pad[:1]))[:B * L].view(B, L)
    en = pad.scatter(0, slot, torch.where(ok, x[:, 1], pad[:1]))[:B * L].view(B, L)
    i = torch.arange(L, device=x.device)
    band = (i[None, :] >= i[:, None]) & (i[None, :] - i[:, None] < max(1, int(max_answer_length)))
    out = []
    step = max(1, (1 << 24) // (L * L))
    for b0 in range(0, B, step):
        sc = st[b0:b0 + step, :, None] + en[b0:b0 + step, None, :]
        sc = sc.masked_fill(~band, float("-inf"))
        k = sc.view(sc.shape[0], -1).argmax(dim=1)  # the first maximum
        out.append(torch.stack([k // L, k % L], dim=1))
    return torch.cat(out).to(torch.int32)


def span_loss(logits, positions, cu, row_mask, max_answer_length: int, max_seqlen: Optional[int] = None):
    """Span-extraction loss of ``logits [R, 2]`` (column 0 = start, column 1 = end) over the sequences
    ``cu[b] .. cu[b+1]-1`` of the flat buffer, ``row_mask [R]`` taking rows out (the padded layout:
    ``cu = arange(B+1)·S`` plus the flat attention mask). ``positions [B, 2]`` are relative to the sequence's first
    row; one is ignored when it is ``< 0``, ``>= len`` or on a masked row. For column c sequence b contributes
    ``lse_c(b) - logit[pos_c(b), c]`` with the logsumexp over the REAL rows of b;
    ``loss = ½ (Σ start terms / max(n_start, 1) + Σ end terms / max(n_end, 1))``, 0 when everything is ignored.

    Returns ``(loss, stats, pred)``: ``stats`` fp32 [8] = {loss, hits, n, loss·n, n_start, n_end, start hits, end hits}
    (hits: both labels valid and equal to the best span; n: both labels valid), ``pred`` from :func:`span_best`."""
    R = logits.shape[0]
    B = cu.numel() - 1
    cul = cu.long()
    seg, rel, real = span_segments(cu, R, row_mask)
    x = logits.float()
    ninf = torch.full((), float("-inf"), dtype=torch.float32, device=x.device)
    xm = torch.where(real[:, None], x, ninf)
    idx = seg[:, None].expand(-1, 2)
    m = torch.full((B + 1, 2), float("-inf"), dtype=torch.float32, device=x.device)
    m = m.scatter_reduce(0, idx, xm.detach(), "amax", include_self=True)
    z = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.where(real[:, None], torch.exp(xm - z[seg]), torch.zeros_like(x))
    se = torch.zeros((B + 1, 2), dtype=torch.float32, device=x.device).index_add(0, seg, e)
    lse = (z + torch.log(se.clamp_min(1e-30)))[:B]
    pos = positions.reshape(B, 2).long()
    length = (cul[1:] - cul[:-1])[:, None]
    inside = (pos >= 0) & (pos < length)
    row = (cul[:-1, None] + torch.where(inside, pos, torch.zeros_like(pos))).clamp(0, R - 1)
    valid = inside & real[row] & (seg[row] == torch.arange(B, device=x.device)[:, None])
    tgt = torch.gather(x, 0, row)  # [B, 2]: column c of row[:, c]
    terms = torch.where(valid, lse - tgt, torch.zeros_like(tgt))
    nc = valid.sum(0).to(torch.float32)
    loss = 0.5 * (terms.sum(0) / nc.clamp(min=1.0)).sum()
    with torch.no_grad():
        pred = span_best(logits, cu, row_mask, max_answer_length, max_seqlen)
        eq = (pred.long() == pos) & valid
        both = valid.all(dim=1)
        n = both.sum().to(torch.float32)
        hits = (eq.all(dim=1) & both).sum().to(torch.float32)
        lv = loss.detach().float()
        stats = torch.stack([lv, hits, n, lv * n, nc[0], nc[1], eq[:, 0].sum().float(), eq[:, 1].sum().float()])
    return loss, stats, pred


def qa_head(h2d, w, b, positions, cu, row_mask, p: float, seed: int, max_answer_length: int = 30,
            training: bool = True, max_seqlen: Optional[int] = None):
    """Question-answering head on every row of ``h2d`` [R, H] (HF ``*ForQuestionAnswering``):
    ``logits = dropout(h) Wᵀ + b`` [R, 2], the dropout site being the flat ``[R, H]`` buffer, then :func:`span_loss`.
    With ``positions`` returns ``(loss, logits, stats, pred)``, without ``(logits, pred)``. Unlike HF the softmax runs
    over the real rows only (docs/PARITY.md)."""
    logits = F.linear(dropout(h2d, p, seed, training), w, b)
    if positions is None:
        return logits, span_best(logits, cu, row_mask, max_answer_length, max_seqlen)
    loss, stats, pred = span_loss(logits, positions, cu, row_mask, max_answer_length, max_seqlen)
    return loss, logits, stats, pred


def mlm_head(h2d, labels, w1, b1, ln_w, ln_b, eps: float, wemb, bias, vocab: int, label_smoothing: float = 0.0):
    """RoBERTa LM head on the masked positions (labels != -100) of ``h2d`` [T, H]: ``LN(gelu(x W1ᵀ + b1))`` ->
    tied decoder (``wemb[:vocab]``, ``bias[:vocab]``) -> mean CE (``label_smoothing`` as in :func:`cross_entropy`,
    over the ``vocab`` real classes). Returns (loss, logits [n_masked, vocab])."""
    sel = labels.ne(-100).nonzero(as_tuple=True)[0]
    x = h2d.index_select(0, sel)
    x = layer_norm(linear_gelu(x, w1, b1), ln_w, ln_b, eps)
    logits = F.linear(x, wemb[:vocab], bias[:vocab])
    return cross_entropy(logits, labels.index_select(0, sel), label_smoothing), logits
