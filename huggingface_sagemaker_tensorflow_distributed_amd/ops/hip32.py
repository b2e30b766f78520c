"""The fp32 step on hand-written gfx950 kernels: the reference's own precision.

The reference trains in plain fp32 (``/root/reference/scripts/train.py:113-123`` compiles a Keras model with no
mixed-precision policy). ``--dtype fp32`` on a GPU runs every op here (VERDICT r3 'missing 2'); nothing falls back
to ATen GEMMs / softmax / bmm on the supported shapes (BERT-family encoders, head dim 64, even S, widths that are
multiples of 256):

* GEMMs: the bf16 MFMA kernels (``csrc/kernels/gemm2.hip``) on 3-term split products. ``x = hi + lo`` with
  ``hi = bf16(x)``, ``lo = bf16(x - hi)`` (``|x - hi - lo| <= 2^-17 |x|``), and ``x·wᵀ ≈ xh·whᵀ + xh·wlᵀ + xl·whᵀ``
  (the dropped ``xl·wlᵀ`` is ``<= 2^-16`` of each product), summed in fp32 by ONE GEMM over a segmented K
  (``gemm2_seg``: K-tiles of segment s read the s-th (A, B) pair of hi / lo halves as they are stored, so the operands
  are never copied into three-block concatenations). Forward and dgrad are NT with fp32 output, the weight gradient is
  the TT kernel accumulating into the fp32 ``main_grad`` with the segments along the tokens. Relative error per output
  ~1e-5 of Σ|products| (vs ~4e-3 for one bf16 product).
* Splits: weights are split ONCE per optimizer step -- the fused Adam writes each updated weight's hi / lo halves
  (``FlatParamStore`` fp32 split buffers, ``p._hsd_split``); an activation is split once in the forward and its halves
  saved for the weight gradient; an incoming gradient is split once for both of its GEMMs.
* bias / GELU / dropout + residual epilogues, LayerNorm, embeddings, streaming attention (online softmax, exact fp32
  FMAs) and the classification head: ``csrc/kernels/fp32.hip``.

Dropout sites use the reference ops' element indexing and hash (``ops/rng.py``), so a GPU fp32 step draws the CPU
reference's masks bit for bit (``tests/test_gpu_fp32.py``).
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from . import hip
from .hip import _Grad, _s64

_C = hip._C
PAT_A = 0b100  # blocks [hi | hi | lo]
PAT_B = 0b010  # blocks [hi | lo | hi]
_ACT = {"tanh": 0, "relu": 1}


def _split(x: torch.Tensor, pat: int, rows: bool = False, pad_rows: int = 0) -> torch.Tensor:
    """bf16 split concatenation of fp32 ``x`` [R, C]: [R, 3C] (blocks along K = columns) or [3R', C] (blocks stacked
    along K = rows; R' = R rounded up to ``pad_rows`` with zero rows, which add nothing to the product)."""
    x = x.contiguous()
    if rows and pad_rows and x.shape[0] % pad_rows:
        r = -(-x.shape[0] // pad_rows) * pad_rows
        xp = torch.zeros((r, x.shape[1]), dtype=x.dtype, device=x.device)
        xp[: x.shape[0]] = x
        x = xp
    R, C = x.shape
    out = torch.empty((3 * R, C) if rows else (R, 3 * C), dtype=torch.bfloat16, device=x.device)
    _C.split3(x, out, pat, rows)
    return out


# A linear layer's incoming gradient is split ONCE into both layouts its backward needs (column blocks for the dgrad,
# row blocks for the weight gradient): one read of dy and one launch instead of two (profiles/fp32_dual_split_ab_r5.log)


def _grad_seg_ok(T: int, N: int, K: int, need_dgrad: bool) -> bool:
    """A [T, N] gradient of a layer with weight [N, K] goes to the segmented GEMMs (weight gradient, and dgrad)."""
    return N % 4 == 0 and _seg_ok(1, 1, N, K, T) and (not need_dgrad or _seg_ok(0, 1, T, K, N))


def _split_grad(dy: torch.Tensor, need_dgrad: bool, w: Optional[torch.Tensor] = None, halves=None):
    """``dy``'s split for both of its GEMMs: ((hi, lo), (hi, lo)) when the segmented GEMMs take the layer's shapes
    (``w`` given; ``halves``: dy's (hi, lo) written by its producer), else (column-block split for :func:`mm_dgrad` or
    None, row-block split for :func:`wgrad_` or None)."""
    if w is not None and dy.dim() == 2 and dy.shape[1] % 4 == 0:
        T, N = dy.shape
        if _grad_seg_ok(T, N, w.shape[1], need_dgrad):
            hl = halves if halves is not None else _split2(dy.contiguous())
            return (hl if need_dgrad else None), hl
    if not (need_dgrad and dy.dim() == 2 and dy.shape[0] % 64 == 0 and dy.shape[1] % 4 == 0):
        return None, None
    dy = dy.contiguous()
    R, C = dy.shape
    cols = torch.empty((R, 3 * C), dtype=torch.bfloat16, device=dy.device)
    rows = torch.empty((3 * R, C), dtype=torch.bfloat16, device=dy.device)
    _C.split3_dual(dy, cols, PAT_A, rows, PAT_A)
    return cols, rows


def _split2(x: torch.Tensor):
    hi = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    lo = torch.empty_like(hi)
    _C.split2(x, hi, lo)
    return hi, lo


def _halves_like(x: torch.Tensor):
    return torch.empty(x.shape, dtype=torch.bfloat16, device=x.device), torch.empty(x.shape, dtype=torch.bfloat16,
                                                                                    device=x.device)


# A block's output (its LayerNorm's, or the embeddings') feeds the next block's first GEMM: the producing kernel writes
# its bf16 halves as well (ln32_fwd / dropout32 hi / lo) and leaves them here; the next block takes them instead of a
# split2 pass over its input. (tensor, version, hi, lo): the tensor reference keeps the storage from being reused, and
# the halves are taken only for that storage, unmodified (same data pointer, numel and version counter).
_next_halves = None


def _publish_halves(t: torch.Tensor, hi: torch.Tensor, lo: torch.Tensor) -> None:
    global _next_halves
    _next_halves = (t, t._version, hi, lo)


def _take_halves(x2: torch.Tensor):
    global _next_halves
    c = _next_halves
    if c is None:
        return None
    t, ver, hi, lo = c
    if (x2.data_ptr() == t.data_ptr() and x2.numel() == t.numel() and x2._version == ver and x2.is_contiguous()
            and t.is_contiguous()):
        _next_halves = None
        return hi.view(x2.shape), lo.view(x2.shape)
    return None


def _halves_wanted(rows: int, H: int) -> bool:
    """Whether a block output [rows, H] is worth splitting in its producer (the next block's segmented GEMMs read it)."""
    return rows % 64 == 0 and H % 64 == 0 and H % 256 == 0


def weight_split(w: torch.Tensor):
    """(hi, lo) of weight ``w``: the halves the optimizer step wrote (``FlatParamStore`` split buffers) while they are
    current, else split here. Current = no in-place change since the store last wrote them: the store's master buffer
    and the parameter itself carry the versions recorded at that refresh (the fused Adam writes master and halves in
    one kernel, so an optimizer step keeps them current)."""
    sp = getattr(w, "_hsd_split", None)
    if sp is not None:
        hi, lo, store, ver = sp
        if store.splits_current() and w._version == ver:
            return hi, lo
    return _split2(w.contiguous())


def _seg_ok(la: int, lb: int, M: int, N: int, Kseg: int) -> bool:
    return Kseg % 64 == 0 and _C.gemm2_seg_supported(la, lb, M, N, Kseg)


def _nt_ok(M: int, N: int, K: int) -> bool:
    return N % 256 == 0 and (3 * K) % 64 == 0 and K % 4 == 0 and _C.gemm2_supported(0, 0, hip.EPI_F32_SLAB, M, N, 3 * K)


def mm_nt(x: torch.Tensor, w: torch.Tensor, xs=None) -> torch.Tensor:
    """x [M, K] · w [N, K]ᵀ -> [M, N] fp32 (split-product MFMA GEMM). ``xs``: x's (hi, lo), already made."""
    M, K = x.shape
    N = w.shape[0]
    if _seg_ok(0, 0, M, N, K):
        xh, xl = xs if xs is not None else _split2(x)
        wh, wl = weight_split(w)
        y = torch.empty((M, N), dtype=torch.float32, device=x.device)
        _C.gemm2_seg([xh, xh, xl], [wh, wl, wh], y, 0, 0)
        return y
    if not _nt_ok(M, N, K):
        return x @ w.t()  # odd widths only (not on the BERT-family shapes)
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    _C.gemm2_f32nt(_split(x, PAT_A), _split(w, PAT_B), y, 0)
    return y


def mm_dgrad(dy: torch.Tensor, w: torch.Tensor, dys: Optional[torch.Tensor] = None,
             acc: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dy [M, N] · w [N, K] -> [M, K] fp32: NT with W read k-strided (layout (0, 1)), the split blocks of W stacked
    along its rows (= the product's K). ``dys``: dy's split, already made (:func:`_split_grad`). ``acc`` (fp32 [M, K],
    segmented GEMM only): the product is added to it in place and it is returned (a residual gradient + the dgrad
    in one pass: the fused fp32 blocks below)."""
    M, N = dy.shape
    K = w.shape[1]
    if isinstance(dys, tuple) or (dys is None and _seg_ok(0, 1, M, K, N)):
        dh, dl = dys if dys is not None else _split2(dy.contiguous())
        wh, wl = weight_split(w)
        dx = acc if acc is not None else torch.empty((M, K), dtype=torch.float32, device=dy.device)
        _C.gemm2_seg([dh, dh, dl], [wh, wl, wh], dx, 0, 1, acc is not None)
        return dx
    if acc is not None:
        return acc.add_(mm_dgrad(dy, w, dys))
    if not (K % 256 == 0 and (3 * N) % 64 == 0 and N % 4 == 0 and _C.gemm2_supported(0, 1, hip.EPI_F32_SLAB, M, K, 3 * N)):
        return dy @ w
    dx = torch.empty((M, K), dtype=torch.float32, device=dy.device)
    _C.gemm2_f32nt(dys if dys is not None else _split(dy, PAT_A), _split(w, PAT_B, rows=True), dx, 1)
    return dx


def wgrad_(g: _Grad, dy: torch.Tensor, x: torch.Tensor, dys=None, xs=None) -> None:
    """g.buf [N, K] += dyᵀ [N, T] · x [T, K] in fp32 (TT kernel, split blocks stacked along the tokens, padded to
    64-token K-tiles). ``dys``: dy's split made by :func:`_split_grad` -- (hi, lo) on the segmented GEMM, else the
    row-block split (T % 64 == 0); ``xs``: x's (hi, lo) saved by the forward."""
    N, K, T = dy.shape[1], (x if x is not None else xs[0]).shape[1], dy.shape[0]
    if xs is not None or isinstance(dys, tuple) or (dys is None and _seg_ok(1, 1, N, K, T)):
        # (xs is only made where this segmented GEMM takes the shape: _x_split)
        dh, dl = dys if isinstance(dys, tuple) else _split2(dy.contiguous())
        xh, xl = xs if xs is not None else _split2(x.contiguous())
        _C.gemm2_seg([dh, dh, dl], [xh, xl, xh], g.buf, 1, 1)
        return
    Tp = -(-T // 64) * 64
    if not (N % 8 == 0 and K % 256 == 0 and N % 4 == 0 and K % 4 == 0 and hip._tt_ok(N, K, 3 * Tp)):
        g.buf.add_(dy.t() @ x)
        return
    a = dys if dys is not None else _split(dy, PAT_A, rows=True, pad_rows=64)
    b = _split(x, PAT_B, rows=True, pad_rows=64)
    _, sp, ws = _C.gemm2_wgrad_plan(N, K, 3 * Tp)
    _C.gemm2(a, b, g.buf, 1, 1, hip.EPI_F32_SLAB, None, None, None, 0.0, 0, sp, hip._workspace(ws, dy.device), None)


def _colsum_(g: _Grad, x: torch.Tensor) -> None:
    _C.colsum32(x.contiguous(), g.buf)


# ------------------------------------------------------------------------------------------ linear layers
def _x_split(x2: torch.Tensor, w: torch.Tensor):
    """x's (hi, lo) when the segmented GEMMs take the layer (forward NT and the weight gradient reuse them), else None."""
    M, K = x2.shape
    if _seg_ok(0, 0, M, w.shape[0], K) and _seg_ok(1, 1, w.shape[0], K, M):
        hl = _take_halves(x2)
        return hl if hl is not None else _split2(x2)
    return None


def _save_x(ctx, x2, xs, *rest):
    """Keep x's halves for the weight gradient instead of x itself (the same bytes, no re-split in backward)."""
    if xs is not None:
        ctx.save_for_backward(xs[0], xs[1], *rest)
        ctx.x_split = True
    else:
        ctx.save_for_backward(x2, *rest)
        ctx.x_split = False


def _saved_x(ctx):
    """(x2 or None, xs or None, *rest) from :func:`_save_x`."""
    t = ctx.saved_tensors
    if ctx.x_split:
        return (None, (t[0], t[1])) + tuple(t[2:])
    return (t[0], None) + tuple(t[1:])


class _Linear32(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        xs = _x_split(x2, w)
        y = mm_nt(x2, w, xs)
        _C.epi32(y, b, None, y, 0, 0.0, 0)
        _save_x(ctx, x2, xs, w, b)
        ctx.xshape = x.shape
        return y.view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, xs, w, b = _saved_x(ctx)
        dy2 = dy.reshape(-1, w.shape[0]).contiguous()
        sc, sr = _split_grad(dy2, ctx.needs_input_grad[0], w)
        dx = mm_dgrad(dy2, w, sc).view(ctx.xshape) if ctx.needs_input_grad[0] else None
        gw, gb = _Grad(w), _Grad(b)
        wgrad_(gw, dy2, x2, sr, xs)
        _colsum_(gb, dy2)
        return dx, gw.done(), gb.done()


def linear(x, w, b):
    return _Linear32.apply(x, w, b)


class _LinearGelu32(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        xs = _x_split(x2, w)
        y = mm_nt(x2, w, xs)  # becomes the pre-activation (bias added in place)
        g = torch.empty_like(y)
        _C.epi32(y, b, None, g, 1, 0.0, 0)
        _save_x(ctx, x2, xs, w, b, y)
        ctx.xshape = x.shape
        return g.view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dg):
        x2, xs, w, b, y = _saved_x(ctx)
        da = torch.empty_like(y)
        _C.epi32(dg.reshape(y.shape).contiguous(), None, y, da, 4, 0.0, 0)
        gw, gb = _Grad(w), _Grad(b)
        _colsum_(gb, da)
        sc, sr = _split_grad(da, ctx.needs_input_grad[0], w)
        dx = mm_dgrad(da, w, sc).view(ctx.xshape) if ctx.needs_input_grad[0] else None
        wgrad_(gw, da, x2, sr, xs)
        return dx, gw.done(), gb.done()


def linear_gelu(x, w, b):
    return _LinearGelu32.apply(x, w, b)


class _DenseResidualLN32(torch.autograd.Function):
    """LN(dropout(x Wᵀ + b) + residual)."""

    @staticmethod
    def forward(ctx, x, w, b, res, ln_w, ln_b, eps, p, seed):
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        xs = _x_split(x2, w)
        y = mm_nt(x2, w, xs)
        rows, H = y.shape
        z = torch.empty_like(y)
        _C.epi32(y, b, res.reshape(rows, H).contiguous(), z, 2, float(p), _s64(seed))
        out = torch.empty_like(z)
        mean = torch.empty(rows, dtype=torch.float32, device=y.device)
        rstd = torch.empty_like(mean)
        _C.ln32_fwd(z, ln_w, ln_b, out, mean, rstd, float(eps))
        _save_x(ctx, x2, xs, w, b, z, mean, rstd, ln_w, ln_b)
        ctx.p, ctx.seed, ctx.xshape = float(p), seed, x.shape
        return out.view(res.shape)

    @staticmethod
    def backward(ctx, dout):
        x2, xs, w, b, z, mean, rstd, ln_w, ln_b = _saved_x(ctx)
        gw, gb, gg, gbe = _Grad(w), _Grad(b), _Grad(ln_w), _Grad(ln_b)
        dz = torch.empty_like(z)
        _C.ln32_bwd(dout.reshape(z.shape).contiguous(), z, mean, rstd, ln_w, dz, gg.buf, gbe.buf)
        dy = dz
        if ctx.p > 0:
            dy = torch.empty_like(dz)
            _C.dropout32(dz, dy, ctx.p, _s64(ctx.seed))
        _colsum_(gb, dy)
        sc, sr = _split_grad(dy, ctx.needs_input_grad[0], w)
        dx = mm_dgrad(dy, w, sc).view(ctx.xshape) if ctx.needs_input_grad[0] else None
        wgrad_(gw, dy, x2, sr, xs)
        return dx, gw.done(), gb.done(), dz.view(dout.shape), gg.done(), gbe.done(), None, None, None


def dense_residual_ln(x, w, b, residual, ln_w, ln_b, eps, p, seed):
    return _DenseResidualLN32.apply(x, w, b, residual, ln_w, ln_b, eps, p, seed)


class _LayerNorm32(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, eps):
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        rows = x2.shape[0]
        out = torch.empty_like(x2)
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        _C.ln32_fwd(x2, w, b, out, mean, rstd, float(eps))
        ctx.save_for_backward(x2, mean, rstd, w, b)
        return out.view(x.shape)

    @staticmethod
    def backward(ctx, dout):
        x2, mean, rstd, w, b = ctx.saved_tensors
        gg, gbe = _Grad(w), _Grad(b)
        dx = torch.empty_like(x2)
        _C.ln32_bwd(dout.reshape(x2.shape).contiguous(), x2, mean, rstd, w, dx, gg.buf, gbe.buf)
        return dx.view(dout.shape), gg.done(), gbe.done(), None


def layer_norm(x, w, b, eps):
    return _LayerNorm32.apply(x, w, b, eps)


class _Dropout32(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed):
        xc = x.contiguous()
        out = torch.empty_like(xc)
        _C.dropout32(xc, out, float(p), _s64(seed))
        ctx.p, ctx.seed = float(p), seed
        return out

    @staticmethod
    def backward(ctx, dout):
        dx = torch.empty_like(dout)
        _C.dropout32(dout.contiguous(), dx, ctx.p, _s64(ctx.seed))
        return dx, None, None


def dropout(x, p, seed):
    if p <= 0.0:
        return x
    if x.dim() == 0 or x.shape[-1] % 4:
        from .reference import dropout as ref

        return ref(x, p, seed, True)
    return _Dropout32.apply(x, p, seed)


# ------------------------------------------------------------------------------------------ embeddings
class _EmbedLN32(torch.autograd.Function):
    """dropout(LN(word[ids] + pos[pos_ids] (+ type[type_ids])))."""

    @staticmethod
    def forward(ctx, ids, pos_ids, type_ids, word, pos, typ, ln_w, ln_b, eps, p, seed):
        B, S = ids.shape
        H = word.shape[1]
        ids_c = ids.contiguous().long()
        pos_c = pos_ids.expand(B, S).contiguous().long()
        tt_c = type_ids.expand(B, S).contiguous().long() if (typ is not None and type_ids is not None) else None
        x = torch.empty((B * S, H), dtype=torch.float32, device=word.device)
        _C.embed32_gather(ids_c, pos_c, tt_c, word, pos, typ, x)
        out = torch.empty_like(x)
        mean = torch.empty(B * S, dtype=torch.float32, device=word.device)
        rstd = torch.empty_like(mean)
        hl = _halves_like(out) if _halves_wanted(B * S, H) else None
        if p > 0:
            _C.ln32_fwd(x, ln_w, ln_b, out, mean, rstd, float(eps))
            _C.dropout32(out, out, float(p), _s64(seed), *(hl or (None, None)))
        else:
            _C.ln32_fwd(x, ln_w, ln_b, out, mean, rstd, float(eps), *(hl or (None, None)))
        if hl is not None:
            _publish_halves(out, *hl)
        ctx.save_for_backward(ids_c, pos_c, tt_c if tt_c is not None else ids_c, x, mean, rstd, ln_w)
        ctx.tensors = (word, pos, typ, ln_b)
        ctx.has_tt = tt_c is not None
        ctx.p, ctx.seed = float(p), seed
        return out.view(B, S, H)

    @staticmethod
    def backward(ctx, dout):
        ids, pos_ids, tt, x, mean, rstd, ln_w = ctx.saved_tensors
        word, pos, typ, ln_b = ctx.tensors
        d = dout.reshape(x.shape).contiguous()
        if ctx.p > 0:
            dd = torch.empty_like(d)
            _C.dropout32(d, dd, ctx.p, _s64(ctx.seed))
            d = dd
        gg, gbe = _Grad(ln_w), _Grad(ln_b)
        dx = torch.empty_like(x)
        _C.ln32_bwd(d, x, mean, rstd, ln_w, dx, gg.buf, gbe.buf)
        gwd, gp = _Grad(word), _Grad(pos)
        gt = _Grad(typ) if typ is not None else None
        _C.embed32_scatter(dx, ids, pos_ids, tt if ctx.has_tt else None, gwd.buf, gp.buf, gt.buf if gt else None)
        return (None, None, None, gwd.done(), gp.done(), gt.done() if gt else None, gg.done(), gbe.done(),
                None, None, None)


def embed_ln(input_ids, position_ids, token_type_ids, word_w, pos_w, type_w, ln_w, ln_b, eps, p, seed):
    if type_w is not None and token_type_ids is None:
        token_type_ids = torch.zeros_like(input_ids)
    return _EmbedLN32.apply(input_ids, position_ids, token_type_ids, word_w, pos_w, type_w, ln_w, ln_b, eps, p, seed)


# ------------------------------------------------------------------------------------------ attention
class _Attention32(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, mask_bias, B, S, heads, p, seed):
        qkv = qkv.contiguous()
        H = qkv.shape[-1] // 3
        out = torch.empty((B * S, H), dtype=torch.float32, device=qkv.device)
        lse = torch.empty(B * heads * S, dtype=torch.float32, device=qkv.device)
        mb = mask_bias.contiguous().float() if mask_bias is not None else None
        _C.attn32_fwd(qkv, mb, out, lse, B, S, heads, float(p), _s64(seed))
        ctx.save_for_backward(qkv, out, lse, mb if mb is not None else lse)
        ctx.has_mask = mb is not None
        ctx.cfg = (B, S, heads, float(p), seed)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse, mb = ctx.saved_tensors
        B, S, heads, p, seed = ctx.cfg
        dqkv = torch.empty_like(qkv)
        delta = torch.empty(B * heads * S, dtype=torch.float32, device=qkv.device)
        _C.attn32_bwd(qkv, mb if ctx.has_mask else None, out, dout.contiguous(), lse, dqkv, delta, B, S, heads, p,
                      _s64(seed))
        return dqkv, None, None, None, None, None, None


class _Attention32M(torch.autograd.Function):
    """fp32 attention on the bf16 matrix cores (attention32m.hip): qkv and dout carried as hi + lo bf16 pairs, every
    product the three-term split product, softmax / dropout / accumulation fp32. S a multiple of 128 up to 1024."""

    @staticmethod
    def forward(ctx, qkv, mask_bias, B, S, heads, p, seed):
        qkv = qkv.contiguous()
        H = qkv.shape[-1] // 3
        qh, ql = _split2(qkv)
        out = torch.empty((B * S, H), dtype=torch.float32, device=qkv.device)
        lse = torch.empty(B * heads * S, dtype=torch.float32, device=qkv.device)
        mb = mask_bias.contiguous().float() if mask_bias is not None else None
        _C.attn32m_fwd(qh, ql, mb, out, lse, B, S, heads, float(p), _s64(seed))
        ctx.save_for_backward(qh, ql, out, lse, mb if mb is not None else lse)
        ctx.has_mask = mb is not None
        ctx.cfg = (B, S, heads, float(p), seed)
        return out

    @staticmethod
    def backward(ctx, dout):
        qh, ql, out, lse, mb = ctx.saved_tensors
        B, S, heads, p, seed = ctx.cfg
        dout = dout.contiguous()
        dh, dl = _split2(dout)
        dqkv = torch.empty(qh.shape, dtype=torch.float32, device=qh.device)
        delta = torch.empty(B * heads * S, dtype=torch.float32, device=qh.device)
        _C.attn32m_bwd(qh, ql, dh, dl, mb if ctx.has_mask else None, out, dout, lse, dqkv, delta, B, S, heads, p,
                       _s64(seed))
        return dqkv, None, None, None, None, None, None


# the split-product MFMA attention wherever it takes the sequence length; the vector-ALU fp32 kernels (exact fp32 FMAs)
# serve the rest. Module attribute, not an env knob: tests/test_gpu_fp32.py flips it to cover the fallback.
_ATTN32M = True


def attention_ok(qkv, seq, heads) -> bool:
    return qkv.shape[-1] == 3 * heads * 64 and seq % 2 == 0


def attention(qkv, mask_bias, batch, seq, heads, p, seed):
    if not attention_ok(qkv, seq, heads):
        from .reference import attention as ref

        return ref(qkv, mask_bias, batch, seq, heads, p, seed, p > 0)
    if _ATTN32M and _C.attn32m_supported(seq):
        return _Attention32M.apply(qkv, mask_bias, batch, seq, heads, p, seed)
    return _Attention32.apply(qkv, mask_bias, batch, seq, heads, p, seed)


# ------------------------------------------------------------------------------------------ fused encoder blocks
# The post-LN residual of a block, LN(dropout(f(h) Wᵀ + b) + h), gives h two consumers; as separate autograd ops
# the two gradients of h are summed by an ATen add (2 per layer, ~0.5 ms of a bert-large B = 8 step). The fused
# blocks add the block's first dgrad straight into the residual gradient the LayerNorm backward produced
# (mm_dgrad(acc=)): the segmented GEMM accumulates in place, one pass. Every kernel is the unfused ops' kernel, in the
# same order, and the residual add is the same single fp32 add: outputs and gradients match the unfused ops bit for bit
# (tests/test_gpu_fp32.py::test_fused_fp32_blocks_match_unfused_ops).
def _ln_tail_bwd(dout, z, mean, rstd, ln_w, ln_b, p, seed, gb, w):
    """LN backward of the block tail: (dz = the residual gradient, dy = the GEMM-output gradient, dy's (hi, lo) for the
    segmented GEMMs of the block's last linear (weight ``w``) or None), with the LN and the GEMM bias gradients
    accumulated. The dropout pass writes dy's halves (no split2 pass)."""
    gg, gbe = _Grad(ln_w), _Grad(ln_b)
    dz = torch.empty_like(z)
    _C.ln32_bwd(dout.reshape(z.shape).contiguous(), z, mean, rstd, ln_w, dz, gg.buf, gbe.buf)
    dy, dys = dz, None
    if p > 0:
        dy = torch.empty_like(dz)
        dys = _halves_like(dz) if _grad_seg_ok(dz.shape[0], dz.shape[1], w.shape[1], True) else None
        _C.dropout32(dz, dy, p, _s64(seed), *(dys or (None, None)))
    _colsum_(gb, dy)
    return dz, dy, dys, gg, gbe


def _ln_tail_fwd(y, b, res2d, ln_w, ln_b, eps, p, seed):
    """dropout(y + b) + res -> LayerNorm; the output's halves go to the next block (_publish_halves)."""
    rows, H = y.shape
    z = torch.empty_like(y)
    _C.epi32(y, b, res2d, z, 2, float(p), _s64(seed))
    out = torch.empty_like(z)
    mean = torch.empty(rows, dtype=torch.float32, device=y.device)
    rstd = torch.empty_like(mean)
    hl = _halves_like(out) if _halves_wanted(rows, H) else None
    _C.ln32_fwd(z, ln_w, ln_b, out, mean, rstd, float(eps), *(hl or (None, None)))
    if hl is not None:
        _publish_halves(out, *hl)
    return z, out, mean, rstd


class _AttnBlock32(torch.autograd.Function):
    """LN(dropout(attn(h Wqkvᵀ + bqkv) Woᵀ + bo) + h): QKV split-product GEMM, the split-product MFMA attention
    (attention32m.hip), out-projection, dropout + residual, LayerNorm."""

    @staticmethod
    def forward(ctx, h, qkv_w, qkv_b, out_w, out_b, ln_w, ln_b, eps, mask_bias, B, S, heads, p_a, seed_a, p_h, seed_h):
        h2d = h.reshape(-1, h.shape[-1]).contiguous()
        hs = _x_split(h2d, qkv_w)
        qkv = mm_nt(h2d, qkv_w, hs)
        qh, ql = _halves_like(qkv)
        _C.epi32(qkv, qkv_b, None, None, 0, 0.0, 0, qh, ql)  # qkv + bias -> its halves only (the fp32 sum is unused)
        del qkv
        H = out_w.shape[1]
        att = torch.empty((h2d.shape[0], H), dtype=torch.float32, device=h.device)
        lse = torch.empty(B * heads * S, dtype=torch.float32, device=h.device)
        mb = mask_bias.contiguous().float() if mask_bias is not None else None
        _C.attn32m_fwd(qh, ql, mb, att, lse, B, S, heads, float(p_a), _s64(seed_a))
        as_ = _x_split(att, out_w)
        y = mm_nt(att, out_w, as_)
        z, out, mean, rstd = _ln_tail_fwd(y, out_b, h2d, ln_w, ln_b, eps, p_h, seed_h)
        ctx.save_for_backward(*(hs if hs is not None else (h2d,)), qkv_w, qkv_b, qh, ql, att, lse,
                              mb if mb is not None else lse, *(as_ if as_ is not None else ()), out_w, out_b, z, mean,
                              rstd, ln_w, ln_b)
        ctx.cfg = (B, S, heads, float(p_a), seed_a, float(p_h), seed_h, mb is not None, hs is not None,
                   as_ is not None)
        return out.view(h.shape)

    @staticmethod
    def backward(ctx, dout):
        B, S, heads, p_a, seed_a, p_h, seed_h, has_mask, h_split, a_split = ctx.cfg
        t = list(ctx.saved_tensors)
        hs = (t.pop(0), t.pop(0)) if h_split else None
        h2d = None if h_split else t.pop(0)
        qkv_w, qkv_b, qh, ql, att, lse, mb = t[:7]
        t = t[7:]
        as_ = (t.pop(0), t.pop(0)) if a_split else None
        out_w, out_b, z, mean, rstd, ln_w, ln_b = t
        g_ow, g_ob, g_qw, g_qb = _Grad(out_w), _Grad(out_b), _Grad(qkv_w), _Grad(qkv_b)
        dz, dy, dys, gg, gbe = _ln_tail_bwd(dout, z, mean, rstd, ln_w, ln_b, p_h, seed_h, g_ob, out_w)
        sc, sr = _split_grad(dy, True, out_w, dys)
        datt = mm_dgrad(dy, out_w, sc)
        wgrad_(g_ow, dy, None if a_split else att, sr, as_)
        dh_, dl_ = _split2(datt)
        dqkv = torch.empty(qh.shape, dtype=torch.float32, device=qh.device)
        delta = torch.empty(B * heads * S, dtype=torch.float32, device=qh.device)
        _C.attn32m_bwd(qh, ql, dh_, dl_, mb if has_mask else None, att, datt, lse, dqkv, delta, B, S, heads, p_a,
                       _s64(seed_a))
        _colsum_(g_qb, dqkv)
        sc, sr = _split_grad(dqkv, ctx.needs_input_grad[0], qkv_w)
        dh = mm_dgrad(dqkv, qkv_w, sc, acc=dz) if ctx.needs_input_grad[0] else None
        wgrad_(g_qw, dqkv, h2d, sr, hs)
        return (dh.view(dout.shape) if dh is not None else None, g_qw.done(), g_qb.done(), g_ow.done(), g_ob.done(),
                gg.done(), gbe.done(), None, None, None, None, None, None, None, None, None)


class _FFNBlock32(torch.autograd.Function):
    """LN(dropout(gelu(h W1ᵀ + b1) W2ᵀ + b2) + h)."""

    @staticmethod
    def forward(ctx, h, w1, b1, w2, b2, ln_w, ln_b, eps, p, seed):
        h2d = h.reshape(-1, h.shape[-1]).contiguous()
        hs = _x_split(h2d, w1)
        pre = mm_nt(h2d, w1, hs)  # becomes the pre-activation (bias added in place)
        T, I = pre.shape
        if _seg_ok(0, 0, T, w2.shape[0], I) and _seg_ok(1, 1, w2.shape[0], I, T):
            # GELU output as its halves only: the FFN2 forward and weight gradient read nothing else
            g, gs = None, _halves_like(pre)
            _C.epi32(pre, b1, None, None, 1, 0.0, 0, *gs)
        else:
            g, gs = torch.empty_like(pre), None
            _C.epi32(pre, b1, None, g, 1, 0.0, 0)
        y = mm_nt(g if g is not None else pre, w2, gs)  # (with gs, mm_nt reads only the shape of its first argument)
        z, out, mean, rstd = _ln_tail_fwd(y, b2, h2d, ln_w, ln_b, eps, p, seed)
        ctx.save_for_backward(*(hs if hs is not None else (h2d,)), w1, b1, pre, *(gs if gs is not None else (g,)), w2,
                              b2, z, mean, rstd, ln_w, ln_b)
        ctx.cfg = (float(p), seed, hs is not None, gs is not None)
        return out.view(h.shape)

    @staticmethod
    def backward(ctx, dout):
        p, seed, h_split, g_split = ctx.cfg
        t = list(ctx.saved_tensors)
        hs = (t.pop(0), t.pop(0)) if h_split else None
        h2d = None if h_split else t.pop(0)
        w1, b1, pre = t[:3]
        t = t[3:]
        gs = (t.pop(0), t.pop(0)) if g_split else None
        g = None if g_split else t.pop(0)
        w2, b2, z, mean, rstd, ln_w, ln_b = t
        g_w1, g_b1, g_w2, g_b2 = _Grad(w1), _Grad(b1), _Grad(w2), _Grad(b2)
        dz, dy, dys, gg, gbe = _ln_tail_bwd(dout, z, mean, rstd, ln_w, ln_b, p, seed, g_b2, w2)
        sc, sr = _split_grad(dy, True, w2, dys)
        dg = mm_dgrad(dy, w2, sc)
        wgrad_(g_w2, dy, g, sr, gs)
        da = torch.empty_like(pre)
        das = _halves_like(da) if _grad_seg_ok(da.shape[0], da.shape[1], w1.shape[1], ctx.needs_input_grad[0]) else None
        _C.epi32(dg, None, pre, da, 4, 0.0, 0, *(das or (None, None)))
        _colsum_(g_b1, da)
        sc, sr = _split_grad(da, ctx.needs_input_grad[0], w1, das)
        dh = mm_dgrad(da, w1, sc, acc=dz) if ctx.needs_input_grad[0] else None
        wgrad_(g_w1, da, h2d, sr, hs)
        return (dh.view(dout.shape) if dh is not None else None, g_w1.done(), g_b1.done(), g_w2.done(), g_b2.done(),
                gg.done(), gbe.done(), None, None, None)


def _blocks_ok(h, H: int, inner: int) -> bool:
    """The fused blocks' segmented GEMMs and fp32 LayerNorm take these shapes (else the unfused ops run)."""
    T = h.numel() // H
    return (H % 4 == 0 and H <= 1024 and T % 64 == 0 and _seg_ok(0, 0, T, inner, H) and _seg_ok(0, 1, T, H, inner)
            and _seg_ok(0, 0, T, H, inner) and _seg_ok(0, 1, T, inner, H))


def attn_block_ok(h, qkv_w, S: int, heads: int) -> bool:
    H = h.shape[-1]
    return (qkv_w.shape[0] == 3 * heads * 64 and _ATTN32M and _C.attn32m_supported(S) and _blocks_ok(h, H, 3 * H)
            and _seg_ok(1, 1, 3 * H, H, h.numel() // H) and _seg_ok(1, 1, H, H, h.numel() // H))


def ffn_block_ok(h, w1) -> bool:
    H, inner = h.shape[-1], w1.shape[0]
    T = h.numel() // H
    return _blocks_ok(h, H, inner) and _seg_ok(1, 1, inner, H, T) and _seg_ok(1, 1, H, inner, T)


def attn_block(h, qkv_w, qkv_b, out_w, out_b, ln_w, ln_b, eps, mask_bias, B, S, heads, p_a, seed_a, p_h, seed_h):
    return _AttnBlock32.apply(h, qkv_w, qkv_b, out_w, out_b, ln_w, ln_b, eps, mask_bias, B, S, heads, p_a, seed_a,
                              p_h, seed_h)


def ffn_block(h, w1, b1, w2, b2, ln_w, ln_b, eps, p, seed):
    return _FFNBlock32.apply(h, w1, b1, w2, b2, ln_w, ln_b, eps, p, seed)


# ------------------------------------------------------------------------------------------ classification head
class _ClsTail32(torch.autograd.Function):
    """pre [B, H] -> act -> dropout -> classifier -> CE + accuracy (fp32.hip cls32_*)."""

    @staticmethod
    def forward(ctx, pre, w2, b2, labels, act, p, seed):
        R, H = pre.shape
        C = w2.shape[0]
        t = torch.empty_like(pre)
        logits = torch.empty((R, C), dtype=torch.float32, device=pre.device)
        sums = torch.zeros(2, dtype=torch.float32, device=pre.device)
        lab = labels.contiguous().long()
        _C.cls32_fwd(pre, w2, b2, lab, t, logits, sums, _ACT[act], float(p), _s64(seed))
        stats = torch.stack([sums[0] / R, sums[1], torch.full_like(sums[0], float(R)), sums[0]])
        ctx.save_for_backward(pre, t, w2, b2, logits, lab)
        ctx.cfg = (act, float(p), seed)
        ctx.mark_non_differentiable(logits, stats)
        ctx.set_materialize_grads(False)
        return stats[0], logits, stats

    @staticmethod
    def backward(ctx, dloss, _dlogits, _dstats):
        pre, t, w2, b2, logits, lab = ctx.saved_tensors
        act, p, seed = ctx.cfg
        if dloss is None:
            dloss = torch.zeros((), dtype=torch.float32, device=pre.device)
        gw2, gb2 = _Grad(w2), _Grad(b2)
        dpre = torch.empty_like(pre)
        _C.cls32_bwd(pre, t, w2, logits, lab, dloss.reshape(1).float().contiguous(), dpre, gw2.buf, gb2.buf,
                     _ACT[act], p, _s64(seed))
        return dpre, gw2.done(), gb2.done(), None, None, None, None


def cls_head_ok(h, w1, w2) -> bool:
    H = h.shape[-1]
    return h.dim() == 3 and H % 4 == 0 and 1 <= w2.shape[0] <= 8 and w1.shape[0] == H


def cls_head(h, w1, b1, w2, b2, labels, act, p_in, seed_in, p, seed):
    """(loss, logits, stats): first-token rows -> dropout -> dense (split-product GEMM) -> fused fp32 tail; stats =
    fp32 {mean loss, argmax hits, rows scored, loss sum} as on the bf16 path."""
    x = h[:, 0].contiguous()
    x = dropout(x, p_in, seed_in)
    pre = linear(x, w1, b1)
    return _ClsTail32.apply(pre, w2, b2, labels, act, p, seed)
