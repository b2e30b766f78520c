"""The row-wise and elementwise HIP kernels at their edge shapes (embedding, LayerNorm, column sums, GELU, dropout,
small-batch weight gradient, cross-entropy, classification head, Adam) vs fp64 (or ops/reference.py fp32) references
computed from the same bf16-rounded inputs.

Every case names the branch of the launcher its shape was chosen to reach and, where the branch depends on launch
geometry, recomputes that geometry with the launcher's own formula and asserts the property it relies on: a retune of
the launcher then fails here instead of silently losing the coverage.

Tolerances are the project's own for the op (tests/test_gpu_ops.py) or derived in place:

* fp32 summation of n terms in any grouping: |err| <= (n - 1) * 2^-24 * sum|terms| (first order). bf16 values and
  products of two bf16 values are exact in fp32, so the column sums and the small weight gradient are such sums. The
  accumulate-into targets start at 0.5 * sum|terms| (random sign): with that start value as one more term the error
  stays below n * 2^-24 * 1.5 * sum|terms| < n * 2^-23 * sum|terms|, the bound used below.
* GELU: the kernels' erf is Abramowitz & Stegun 7.1.26, |err| <= 1.5e-7 (csrc/kernels/common.h): one bf16 ulp of the
  reference for the output rounding plus 1e-7 |x| (forward: 0.5 |x| * erf error) or 2e-7 |dg| max(1, |y|) (derivative).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from huggingface_sagemaker_tensorflow_distributed_amd.ops import reference as ref  # noqa: E402
from huggingface_sagemaker_tensorflow_distributed_amd.ops.rng import keep_mask  # noqa: E402


def _hip():
    from huggingface_sagemaker_tensorflow_distributed_amd.ops import hip

    return hip


def _close(a, b, atol, rtol, what=""):
    """At most 0.1 % of the elements beyond tolerance (bf16 rounding flips), and NONE beyond 4x the tolerance."""
    a = a.float()
    b = b.float()
    err = (a - b).abs()
    # atol is relative to the tensor's scale (bf16 outputs of long reductions), rtol per element
    tol = atol * b.abs().max().clamp_min(1e-6) + rtol * b.abs()
    bad = (err > tol).float().mean().item()
    worst = (err / tol).max().item()
    assert bad <= 1e-3, f"{what}: {bad*100:.3f}% elements out of tol, max err {err.max().item():.4g}"
    assert worst <= 4.0, f"{what}: an element is {worst:.2f}x beyond tolerance (max err {err.max().item():.4g})"


def _bf16_ulp(r):
    """Spacing of bf16 (8 significant bits) at the magnitude of ``r``: 2^(floor(log2 |r|) - 7), at least 2^-133."""
    e = (r.float().abs().view(torch.int32) & 0x7F800000).view(torch.float32)  # 2^floor(log2 |r|), 0 below 2^-126
    return (e.double() * 2.0 ** -7).clamp_min(2.0 ** -133)


def _within(a, r, bound, what):
    """|a - r| <= bound element-wise (fp64), no exceptions."""
    err = (a.double() - r).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    bad = int((err > bound).sum().item())
    assert bad == 0, f"{what}: {bad} elements beyond the bound, worst err / bound = {ratio:.3f}"


def _start_value(absum, gen_seed):
    """Non-zero start of an accumulate-into target: 0.5 * sum|terms| with a random sign (module docstring)."""
    g = torch.Generator(device=absum.device).manual_seed(gen_seed)
    sign = torch.randint(0, 2, absum.shape, device=absum.device, generator=g).double() * 2 - 1
    return (0.5 * absum * sign).float()


# ------------------------------------------------------------------------------------------------ 1. embedding
def _embed_bwd_geometry(B, S, H):
    """(kernel, chunks, bpc, rows of the last chunk): the arithmetic of launch_embed_bwd (csrc/kernels/embedding.hip)."""
    vec = H % 8 == 0 and H <= 1024
    target = 512 if vec else 2048
    chunks = max(1, min(B, (target + S - 1) // S))
    bpc = (B + chunks - 1) // chunks
    chunks = (B + bpc - 1) // bpc
    if vec:
        kern = "bwd16<1,8>" if H <= 512 else ("bwd16<2,12>" if H <= 768 else "bwd16<2,16>")
    else:
        ne = (H + 63) // 64
        kern = "bwd<%d>" % (1 if ne <= 1 else 2 if ne <= 2 else 12 if ne <= 12 else 16)
    return kern, chunks, bpc, B - (chunks - 1) * bpc


def _embed_case(gpu, B, S, H, p, arange, type_rows, ids=None, pos=None, pos_rows=None, V=1000):
    hip = _hip()
    torch.manual_seed(B * 1000 + S * 10 + H)
    if ids is None:
        ids = torch.randint(0, V, (B, S), device=gpu)
    if pos is None:
        # RoBERTa-style position ids (padding_idx + 1 + arange, per-token gradient atomics) when not arange
        pos = torch.arange(S, device=gpu).unsqueeze(0).expand(B, S) + (0 if arange else 2)
    pos = pos.contiguous()
    pos_rows = pos_rows or S + 2
    tt = torch.randint(0, type_rows, (B, S), device=gpu) if type_rows else None
    word = (torch.randn(V, H, device=gpu) * 0.02).bfloat16().requires_grad_()
    pw = (torch.randn(pos_rows, H, device=gpu) * 0.02).bfloat16().requires_grad_()
    tw = (torch.randn(type_rows, H, device=gpu) * 0.02).bfloat16().requires_grad_() if type_rows else None
    g = (1 + 0.1 * torch.randn(H, device=gpu)).bfloat16().requires_grad_()
    be = (0.1 * torch.randn(H, device=gpu)).bfloat16().requires_grad_()
    out = hip.embed_ln(ids, pos, tt, word, pw, tw, g, be, 1e-12, p, 99, arange)
    f = lambda t: t.detach().float().requires_grad_() if t is not None else None  # noqa: E731
    word32, pw32, tw32, g32, be32 = f(word), f(pw), f(tw), f(g), f(be)
    r = ref.embed_ln(ids, pos, tt, word32, pw32, tw32, g32, be32, 1e-12, 0.0, 0, False)
    if p > 0:
        # kernel applies dropout to the bf16-rounded LN output
        r = r.bfloat16().float() * keep_mask(99, r.shape, p, device=gpu).float() / (1 - p)
    _close(out, r, 3e-2, 2e-2, "fwd")
    d = torch.randn_like(out)
    out.backward(d)
    r.backward(d.float())
    _close(word.grad, word32.grad, 1e-2, 5e-2, "dword")
    _close(pw.grad, pw32.grad, 1e-1, 5e-2, "dpos")
    if type_rows:
        _close(tw.grad, tw32.grad, 5e-1, 5e-2, "dtype")
    _close(g.grad, g32.grad, 2e-1, 5e-2, "dgamma")
    _close(be.grad, be32.grad, 2e-1, 5e-2, "dbeta")


# (p, pos_is_arange, rows of the type table: ids 0..3, or no table)
_EMB_A = (0.1, True, 4)
_EMB_B = (0.0, False, 0)
_EMB_C = (0.1, False, 4)

_EMBED_WIDTHS = [
    (64, "bwd16<1,8>", _EMB_A),      # one partial 16-B chunk (8 of 64 lanes), NE = 8 with e < H only for i = 0
    (64, "bwd16<1,8>", _EMB_C),      # same, per-token position atomics and type rows 1..3 by atomics
    (512, "bwd16<1,8>", _EMB_A),     # the widest <1,8>: every lane of the single chunk
    (512, "bwd16<1,8>", _EMB_B),     # same, no type table, non-arange positions
    (520, "bwd16<2,12>", _EMB_A),    # first width of <2,12>: second chunk holds one lane
    (520, "bwd16<2,12>", _EMB_B),
    (768, "bwd16<2,12>", _EMB_A),    # the model's width, here with a 4-wave block and a short last chunk
    (768, "bwd16<2,12>", _EMB_C),
    (776, "bwd16<2,16>", _EMB_A),    # first width of <2,16>
    (776, "bwd16<2,16>", _EMB_C),
    (1016, "bwd16<2,16>", _EMB_A),   # partial second chunk (63 of 64 lanes), forward NCH = 4 with a partial last chunk
    (1016, "bwd16<2,16>", _EMB_B),
    (1024, "bwd16<2,16>", _EMB_A),   # bert-large: both chunks full
    (1024, "bwd16<2,16>", _EMB_B),
]


@pytest.mark.parametrize("H,kernel,cfg", _EMBED_WIDTHS)
def test_embed_ln_16B_rows_loop_and_short_chunk(gpu, H, kernel, cfg):
    """16-B backward with bpc = 6 rows per block (waves 0 and 1 take two rows: the b += 4 loop; waves 1-3 hold
    non-zero partials for the 4-wave LDS reduction) and a 3-row last chunk (wave 3 idle there)."""
    B, S = 45, 64
    kern, chunks, bpc, last = _embed_bwd_geometry(B, S, H)
    assert kern == kernel, kern
    assert (chunks, bpc, last) == (8, 6, 3)
    assert bpc >= 5 and B % bpc not in (0, 4)
    _embed_case(gpu, B, S, H, *cfg)


@pytest.mark.parametrize("H,kernel,cfg", [
    (100, "bwd<2>", _EMB_A),  # H % 8 != 0: scalar backward, NE = 2 with a partial second element; forward nq = 25 < 64
    (100, "bwd<2>", _EMB_C),  # same with per-token position atomics and type rows above 0
    (100, "bwd<2>", _EMB_B),  # same without a type table
    (36, "bwd<1>", _EMB_A),   # scalar backward NE = 1, 36 of 64 lanes
    (36, "bwd<1>", _EMB_B),
    (260, "bwd<12>", _EMB_C),  # the scalar kernel's NE = 12 (128 < H <= 768): 5 elements per lane in use, the fifth partial
    (772, "bwd<16>", _EMB_A),  # its NE = 16 (the block's whole 64 KiB of LDS), 13 elements per lane, the last partial
])
def test_embed_ln_scalar_rows_loop_and_short_chunk(gpu, H, kernel, cfg):
    """Scalar backward (target 2048 blocks) with bpc = 7 (waves 0-2 take two rows) and a 2-row last chunk."""
    B, S = 198, 64
    kern, chunks, bpc, last = _embed_bwd_geometry(B, S, H)
    assert kern == kernel, kern
    assert bpc >= 5 and B % bpc not in (0, 4) and last == B % bpc, (chunks, bpc, last)
    _embed_case(gpu, B, S, H, *cfg)


@pytest.mark.parametrize("B,S", [
    (1, 5),  # one batch row: bpc = 1, waves 1-3 of every block idle, forward's last block holds one row
    (3, 1),  # one position: a single column of blocks, 3 forward rows in one block
])
@pytest.mark.parametrize("H,kernel,cfg", [
    (64, "bwd16<1,8>", _EMB_C),
    (768, "bwd16<2,12>", _EMB_A),
    (1024, "bwd16<2,16>", _EMB_B),
    (100, "bwd<2>", _EMB_C),
])
def test_embed_ln_tiny(gpu, B, S, H, kernel, cfg):
    kern, chunks, bpc, last = _embed_bwd_geometry(B, S, H)
    assert kern == kernel and bpc == 1 and chunks == B, (kern, chunks, bpc)
    _embed_case(gpu, B, S, H, *cfg)


@pytest.mark.parametrize("H,kernel", [(768, "bwd16<2,12>"), (100, "bwd<2>")])
def test_embed_ln_all_tokens_same_id(gpu, H, kernel):
    """Every token carries id 7: all B * S word-gradient atomics land on one row (the other rows stay exactly 0)."""
    B, S = 45, 64
    assert _embed_bwd_geometry(B, S, H)[0] == kernel
    ids = torch.full((B, S), 7, device=gpu, dtype=torch.long)
    _embed_case(gpu, B, S, H, 0.1, True, 4, ids=ids)


@pytest.mark.parametrize("H,kernel", [(768, "bwd16<2,12>"), (100, "bwd<2>")])
def test_embed_ln_shared_padding_position(gpu, H, kernel):
    """RoBERTa positions: real tokens 2 + arange, every padded token position row 1 (padding_idx): the non-arange
    atomics with about half of all tokens on one position row."""
    B, S = 45, 64
    assert _embed_bwd_geometry(B, S, H)[0] == kernel
    torch.manual_seed(77)
    lens = torch.randint(1, S + 1, (B,), device=gpu)
    real = torch.arange(S, device=gpu)[None, :] < lens[:, None]
    pos = torch.where(real, torch.arange(S, device=gpu)[None, :] + 2, torch.ones((), dtype=torch.long, device=gpu))
    _embed_case(gpu, B, S, H, 0.1, False, 4, pos=pos)


def test_embed_bwd_binding_rejects_bad_widths(gpu):
    """embed_bwd's binding refuses what the launcher has no kernel for, before any launch."""
    C_ = _hip()._C
    B, S = 2, 4

    def call(H, mean_n=None, gamma_n=None):
        z = lambda *s, dt=torch.float32: torch.zeros(*s, device=gpu, dtype=dt)  # noqa: E731
        bf = torch.bfloat16
        ids = torch.zeros(B, S, device=gpu, dtype=torch.long)
        C_.embed_bwd(z(B * S, H, dt=bf), ids, ids, None, z(10, H, dt=bf), z(S, H, dt=bf), None,
                     z(gamma_n or H, dt=bf), z(mean_n or B * S), z(mean_n or B * S), z(10, H), z(S, H), None, z(H),
                     z(H), B, S, True, 0.0, 0)

    call(64)  # the accepted form of the same call
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        call(1032)  # above every instantiation (the launcher would abort)
    with pytest.raises(RuntimeError):
        call(66)  # not a multiple of 4
    with pytest.raises(RuntimeError):
        call(64, mean_n=B * S - 1)  # mean / rstd shorter than the token count
    with pytest.raises(RuntimeError):
        call(64, gamma_n=32)  # gamma narrower than the tables


# ------------------------------------------------------------------------------------------------ 2. LayerNorm
def _ln_ref64(z, gamma, beta, eps):
    z64 = z.double()
    mean = z64.mean(-1)
    var = z64.var(-1, unbiased=False)
    rstd = (var + eps).rsqrt()
    xh = (z64 - mean[:, None]) * rstd[:, None]
    return xh * gamma.double() + beta.double(), mean, rstd, xh


def _ln_inputs(gpu, rows, H, seed):
    torch.manual_seed(seed)
    y = torch.randn(rows, H, device=gpu).bfloat16()
    res = torch.randn(rows, H, device=gpu).bfloat16()
    g = (1 + 0.1 * torch.randn(H, device=gpu)).bfloat16()
    b = (0.1 * torch.randn(H, device=gpu)).bfloat16()
    return y, res, g, b


def _ln_fwd(gpu, y, res, g, b, want_z, p, seed, eps=1e-12):
    C_ = _hip()._C
    rows, H = y.shape
    # poisoned outputs: a row or column the kernel skips shows up as NaN
    out = torch.full_like(y, float("nan"))
    z = torch.full_like(y, float("nan")) if want_z else None
    mean = torch.full((rows,), float("nan"), device=gpu)
    rstd = torch.full((rows,), float("nan"), device=gpu)
    C_.ln_fwd(y, res, g, b, z, out, mean, rstd, eps, p, seed)
    return out, z, mean, rstd


def _check_ln_fwd(gpu, y, res, g, b, want_z, p, seed, what):
    """Forward vs fp64: z within one bf16 ulp of dropout(y) + res, out vs the fp64 LayerNorm of the stored bf16 z."""
    rows, H = y.shape
    out, z, mean, rstd = _ln_fwd(gpu, y, res, g, b, want_z, p, seed)
    z64 = y.double()
    if p > 0:
        # the kernel multiplies by the fp32 scale 1 / (1 - p)
        z64 = z64 * keep_mask(seed, y.shape, p, device=gpu).double() * float(torch.tensor(1.0 / (1.0 - p)).float())
    mag = z64.abs()
    if res is not None:
        z64 = z64 + res.double()
        mag = mag + res.double().abs()
    if want_z:
        # one bf16 rounding of a value built from an fp32 product and an fp32 sum (2^-24 of the operands each)
        _within(z, z64, _bf16_ulp(z64) + 2.0 ** -23 * mag, what + " z")
        zs = z
    else:
        zs = z64.bfloat16()
        if p == 0 and res is None:
            assert torch.equal(zs, y)
    o64, m64, r64, _ = _ln_ref64(zs, g, b, 1e-12)
    _close(out, o64, 3e-2, 2e-2, what + " out")
    # fp32 two-pass statistics: a lane adds at most 32 values, the wave reduction 6 more levels, so each sum carries
    # at most 38 roundings: 38 * 2^-24 = 2.3e-6 of the row's scale on the mean, the same (relative) on the variance
    # and half of it on rstd, plus the division and the rsqrt (a few 2^-24 each): 1e-5 leaves 4x
    scale = zs.double().abs().amax(-1).clamp_min(1e-30)
    _within(mean, m64, 1e-5 * scale, what + " mean")
    _within(rstd, r64, 1e-5 * r64, what + " rstd")
    return out, zs, mean, rstd


def _ln_bwd_ref64(dout, z, g, dres_add, p, seed):
    _, _, rstd, xh = _ln_ref64(z, g, g, 1e-12)
    d64 = dout.double()
    gg = d64 * g.double()
    dz = rstd[:, None] * (gg - gg.mean(-1, keepdim=True) - xh * (gg * xh).mean(-1, keepdim=True))
    if dres_add is not None:
        dz = dz + dres_add.double()
    dy = dz
    if p > 0:
        dy = dz * keep_mask(seed, z.shape, p, device=z.device).double() * float(torch.tensor(1.0 / (1.0 - p)).float())
    return dz, dy, (d64 * xh).sum(0), d64.sum(0)


def _colsum_bound(x):
    """rows * 2^-23 * sum_r |x[r, c]| per column (module docstring)."""
    x64 = x.double()
    return x64.sum(0), x.shape[0] * 2.0 ** -23 * x64.abs().sum(0)


def _check_ln_bwd(gpu, z, mean, rstd, g, combo, p, seed, col_tol, what):
    """ln_bwd with the argument combination ``combo`` = (dz?, dres_add?, dbias?) vs fp64; dy always given."""
    C_ = _hip()._C
    rows, H = z.shape
    has_dz, has_dres, has_dbias = combo
    torch.manual_seed(seed & 0xFFFF)
    dout = torch.randn(rows, H, device=gpu).bfloat16()
    dres = torch.randn(rows, H, device=gpu).bfloat16() if has_dres else None
    dz = torch.full_like(z, float("nan")) if has_dz else None
    dy = torch.full_like(z, float("nan"))
    # dgamma / dbeta accumulate: start from a known non-zero value
    dg0 = torch.randn(H, device=gpu)
    db0 = torch.randn(H, device=gpu)
    dgamma, dbeta = dg0.clone(), db0.clone()
    dbias = torch.zeros(H, device=gpu) if has_dbias else None
    C_.ln_bwd(dout, z, mean, rstd, g, dz, dy, dres, dgamma, dbeta, dbias, p, seed)
    dz64, dy64, dg64, db64 = _ln_bwd_ref64(dout, z, g, dres, p, seed)
    _close(dy, dy64, 5e-2, 5e-2, what + " dy")
    if has_dz:
        _close(dz, dz64, 5e-2, 5e-2, what + " dz")
    _close(dgamma.double() - dg0.double(), dg64, col_tol, 2e-2, what + " dgamma")
    _close(dbeta.double() - db0.double(), db64, col_tol, 2e-2, what + " dbeta")
    if has_dbias:
        s, bound = _colsum_bound(dy)
        _within(dbias, s, bound, what + " dbias")


_LN_ROWS = [
    1,     # fewer rows than either kernel's rows per wave (forward 2, backward 4): a lone row, no prefetch
    2,     # the forward's pair exactly, half a backward wave
    3,     # forward: second wave holds one row; backward: r + 2 < r1 prefetch then an odd stop
    5,     # backward: a full wave of 4 and a wave with one row
    7,     # backward: second wave stops after 3 rows
    4099,  # many blocks, row count no multiple of rows per wave x 4 waves
]


@pytest.mark.parametrize("H", [
    4,     # one lane of one 8-B chunk; H % 8 != 0: generic forward
    8,     # one lane of one 16-B chunk: plain 16-B forward NC8 = 1
    100,   # H % 8 != 0, nq = 25 < 64: partial single chunk
    252,   # H % 8 != 0, nq = 63: one lane short of a full chunk
    260,   # H % 8 != 0, nq = 65: NCH = 2 with one lane in the second chunk
    312,   # 16-B forward NC8 = 1 with 39 lanes; 8-B NCH = 2 with a partial second chunk
    384,   # 16-B forward NC8 = 1, 48 lanes
    512,   # last width of NC8 = 1 (all 64 lanes), NCH = 2 full
    520,   # first width of NC8 = 2 (one lane in the second chunk), NCH = 3 partial
    772,   # H % 8 != 0 above 768: generic forward NCH = 4 with one lane in the fourth chunk
    1016,  # NC8 = 2 with 63 lanes in the second chunk, NCH = 4 partial
    1024,  # the widest backward: NC8 = 2 and NCH = 4 full
])
def test_layer_norm_widths_and_rows(gpu, H):
    """Forward (plain: 16-B kernel when H % 8 == 0, else the generic one; and dropout + residual + z: generic) and the
    backward of hip.layer_norm (dy only) at every row count of _LN_ROWS."""
    plain16 = H % 8 == 0 and H <= 1024  # ln_fwd_t's condition for the 16-B kernel (with no res / z / dropout)
    assert plain16 == (H in (8, 312, 384, 512, 520, 1016, 1024))
    for rows in _LN_ROWS:
        what = f"H={H} rows={rows}"
        y, res, g, b = _ln_inputs(gpu, rows, H, 100 + rows)
        _, zs, mean, rstd = _check_ln_fwd(gpu, y, None, g, b, False, 0.0, 0, what + " plain")
        _check_ln_bwd(gpu, zs, mean, rstd, g, (False, False, False), 0.0, 0, 2e-1, what + " plain bwd")
        _check_ln_fwd(gpu, y, res, g, b, True, 0.1, 4321, what + " drop+res")


def test_layer_norm_odd_rows_per_wave(gpu):
    """9001 rows at H = 64: the backward's rows per wave is 5 (odd, above the floor of 4: the pair pipeline ends on a
    lone third pair) and the last wave holds one row."""
    rows, H = 9001, 64
    rpw = max(4, (rows + 2047) // 2048)  # ln_bwd_t
    waves = (rows + rpw - 1) // rpw
    assert rpw == 5 and rows - (waves - 1) * rpw == 1 and waves % 4 == 1
    y, res, g, b = _ln_inputs(gpu, rows, H, 9)
    _, zs, mean, rstd = _check_ln_fwd(gpu, y, None, g, b, False, 0.0, 0, "plain")
    _check_ln_bwd(gpu, zs, mean, rstd, g, (False, False, False), 0.0, 0, 2e-1, "plain bwd")
    _, zs, mean, rstd = _check_ln_fwd(gpu, y, res, g, b, True, 0.1, 55, "drop+res")
    _check_ln_bwd(gpu, zs, mean, rstd, g, (True, False, True), 0.1, 55, 1e-1, "bwd")


@pytest.mark.parametrize("combo", [
    (True, False, True),    # (dz, dy, dbias): dense_residual_ln with dropout
    (False, False, True),   # (None, dy, dbias): dense_residual_ln without dropout
    (False, False, False),  # (None, dy, None): hip.layer_norm
    (True, True, True),     # (dz, dy, dres_add, dbias): the residual gradient added in the same pass
])
@pytest.mark.parametrize("H", [
    520,  # H % 8 == 0, NCH = 3 with a 2-lane third chunk
    772,  # H % 8 != 0, NCH = 4 with a 1-lane fourth chunk
])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_layer_norm_bwd_argument_combinations(gpu, combo, H, p):
    """37 rows: 10 waves of 4 rows (the last with one row), the third block with two idle waves in the LDS reduction."""
    rows = 37
    rpw = max(4, (rows + 2047) // 2048)
    waves = (rows + rpw - 1) // rpw
    assert rpw == 4 and waves % 4 == 2 and rows % rpw == 1
    y, res, g, b = _ln_inputs(gpu, rows, H, 31)
    _, zs, mean, rstd = _check_ln_fwd(gpu, y, res, g, b, True, p, 777, "fwd")
    _check_ln_bwd(gpu, zs, mean, rstd, g, combo, p, 777, 1e-1, f"combo={combo}")


@pytest.mark.parametrize("H", [
    1028,  # first width of ln_fwd_t<8>: one lane in the fifth chunk
    1536,  # NCH = 8 with six full chunks
    2048,  # the widest forward: all eight chunks
])
@pytest.mark.parametrize("with_res", [False, True])
def test_layer_norm_forward_only_widths(gpu, H, with_res):
    """1024 < H <= 2048 has a forward only (the backward binding stops at 1024 and is not called here)."""
    assert (H // 4 + 63) // 64 > 4
    y, res, g, b = _ln_inputs(gpu, 9, H, 12)
    _check_ln_fwd(gpu, y, res if with_res else None, g, b, with_res, 0.1 if with_res else 0.0, 99, f"H={H}")


@pytest.mark.parametrize("H,plain", [
    (768, True),   # plain 16-B forward
    (100, False),  # generic forward (H % 8 != 0)
])
def test_layer_norm_constant_rows(gpu, H, plain):
    """Rows of one repeated value have zero variance: out == beta exactly and nothing is NaN. The values (1.5, -2.25,
    0) keep every fp32 partial sum exact, so the mean is the value itself and x - mean is exactly 0."""
    rows = 6
    vals = torch.tensor([1.5, -2.25, 0.0, 1.5, -2.25, 0.0], device=gpu)
    y = vals[:, None].expand(rows, H).contiguous().bfloat16()
    _, _, g, b = _ln_inputs(gpu, rows, H, 3)
    assert plain == (H % 8 == 0)
    out, _, mean, rstd = _ln_fwd(gpu, y, None, g, b, False, 0.0, 0)
    assert not bool(torch.isnan(out.float()).any() | torch.isnan(mean).any() | torch.isnan(rstd).any())
    assert torch.equal(mean, vals)
    assert torch.equal(out, b[None, :].expand(rows, H))


# ------------------------------------------------------------------------------------------------ 3. direct tests
def _colsum_geometry(rows, N):
    """(column blocks, rows per block, row blocks): colsum_launch (csrc/kernels/elementwise.hip)."""
    gx = (N + 511) // 512
    want_y = max(1, 2048 // gx)
    rpb = max(16, (rows + want_y - 1) // want_y)
    rpb = (rpb + 15) // 16 * 16
    return gx, rpb, (rows + rpb - 1) // rpb


_COLSUM_ROWS = [
    1,   # one row: row groups 1-3 add zeros in the LDS reduction
    3,   # fewer rows than row groups
    15,  # one short of the 16 rows a block holds in flight
    16,  # exactly one trip with all 4 loads of every row group
    17,  # a second row block with a single row
    65,  # five row blocks, the last with one row
]


@pytest.mark.parametrize("N", [
    8,     # one active column chunk of 64
    504,   # one column block, last chunk idle
    512,   # exactly one column block
    520,   # a second column block with one active chunk
    3072,  # six column blocks (the FFN bias)
])
def test_colsum(gpu, N):
    C_ = _hip()._C
    for rows in _COLSUM_ROWS:
        gx, rpb, gy = _colsum_geometry(rows, N)
        assert gx == (N + 511) // 512 and rpb == 16 and gy == (rows + 15) // 16
        torch.manual_seed(rows * 7 + N)
        x = torch.randn(rows, N, device=gpu).bfloat16()
        s, bound = _colsum_bound(x)
        d0 = _start_value(x.double().abs().sum(0), rows + N)  # the kernel accumulates
        dbias = d0.clone()
        C_.colsum(x, dbias)
        _within(dbias, s + d0.double(), bound, f"colsum rows={rows} N={N}")


def test_colsum_two_trips_of_the_row_loop(gpu):
    """(40003, 8): more rows than 2048 blocks x 16, so rows per block is 32 and every row group loops twice."""
    C_ = _hip()._C
    rows, N = 40003, 8
    gx, rpb, gy = _colsum_geometry(rows, N)
    assert rpb == 32 and rpb > 16 and gy == 1251 and rows % rpb == 3
    torch.manual_seed(40003)
    x = torch.randn(rows, N, device=gpu).bfloat16()
    s, bound = _colsum_bound(x)
    d0 = _start_value(x.double().abs().sum(0), 1)
    dbias = d0.clone()
    C_.colsum(x, dbias)
    _within(dbias, s + d0.double(), bound, "colsum (40003, 8)")


def _all_bf16_upto40(gpu):
    """Every finite bf16 value with |x| <= 40 (33,858 of them), padded with zeros to 51 x 664 (a multiple of 8)."""
    v = torch.arange(-(1 << 15), 1 << 15, device=gpu, dtype=torch.int16).view(torch.bfloat16)  # every bit pattern
    v = v[torch.isfinite(v.float()) & (v.float().abs() <= 40)]
    assert v.numel() == 33858
    out = torch.zeros(51 * 664, device=gpu, dtype=torch.bfloat16)
    out[:v.numel()] = v
    return out.view(51, 664)


def _gelu64(x):
    x = x.double()
    # 0.5 x (1 + erf(x / sqrt 2)), with 1 + erf(t) written as erfc(-t): no cancellation for very negative x
    return 0.5 * x * torch.erfc(-x / math.sqrt(2.0))


def _gelu_grad64(y):
    y = y.double()
    return 0.5 * torch.erfc(-y / math.sqrt(2.0)) + y * torch.exp(-0.5 * y * y) / math.sqrt(2.0 * math.pi)


def test_gelu_fwd_every_bf16_value(gpu):
    """gelu_fwd over every finite bf16 input up to |x| = 40 vs fp64: one bf16 ulp + 1e-7 |x| (A&S erf error)."""
    C_ = _hip()._C
    x = _all_bf16_upto40(gpu)
    g = torch.full_like(x, float("nan"))
    C_.gelu_fwd(x, g)
    r = _gelu64(x)
    _within(g, r, _bf16_ulp(r) + 1e-7 * x.double().abs(), "gelu_fwd")


@pytest.mark.parametrize("random_dg", [False, True])
def test_gelu_bwd_colsum_every_bf16_value(gpu, random_dg):
    """gelu_bwd_colsum over the same exhaustive y as (51, 664): two column blocks (the second 152 columns wide), four
    row blocks of 16 (the last with 3 rows). da vs fp64 dg gelu'(y); dbias = column sums of the da it wrote."""
    C_ = _hip()._C
    y = _all_bf16_upto40(gpu)
    rows, N = y.shape
    gx, rpb, gy = _colsum_geometry(rows, N)
    assert (gx, rpb, gy) == (2, 16, 4) and rows % rpb == 3
    torch.manual_seed(5)
    dg = torch.randn(rows, N, device=gpu).bfloat16() if random_dg else torch.ones_like(y)
    r = dg.double() * _gelu_grad64(y)
    bound = _bf16_ulp(r) + 2e-7 * dg.double().abs() * y.double().abs().clamp_min(1.0)
    # without a bias gradient
    da0 = torch.full_like(y, float("nan"))
    C_.gelu_bwd_colsum(dg, y, da0, None)
    _within(da0, r, bound, "da (dbias=None)")
    # with one, accumulated onto a non-zero start
    s, cbound = _colsum_bound(da0)
    d0 = _start_value(da0.double().abs().sum(0), 11)
    dbias = d0.clone()
    da = torch.full_like(y, float("nan"))
    C_.gelu_bwd_colsum(dg, y, da, dbias)
    assert torch.equal(da, da0)
    _within(dbias, s + d0.double(), cbound, "dbias")


@pytest.mark.parametrize("T", [
    1,   # a single token: one fma per element
    8,   # the reference's own batch
    63,  # the largest count below one 64-token K-tile
])
def test_small_wgrad(gpu, T):
    """C += dyᵀ x with row-strided dy / x (the [CLS]-row views of ops/hip.py) and a non-zero, row-strided C."""
    C_ = _hip()._C
    for N in (2, 3, 768):          # 2 / 3: the classifier's rows; 768: n * (K / 4) passes one block
        for K in (4, 100, 768):    # 4: one thread per row of C; 100: K / 4 = 25 no multiple of a wave; 768: the model's
            torch.manual_seed(T * 100000 + N * 1000 + K)
            dyb = torch.randn(T, N + 5, device=gpu).bfloat16()
            xb = torch.randn(T, 3 * K, device=gpu).bfloat16()
            dy, x = dyb[:, :N], xb[:, :K]
            prod = dy.double().t() @ x.double()
            absum = dy.double().abs().t() @ x.double().abs()
            cb = torch.randn(N, K + 4, device=gpu)
            cb[:, :K] = _start_value(absum, N + K)
            cb0 = cb.clone()
            Cv = cb[:, :K]
            assert (dy.stride(0), x.stride(0), Cv.stride(0)) == (N + 5, 3 * K, K + 4)  # none is dense
            C_.small_wgrad(dy, x, Cv)
            _within(Cv, prod + cb0[:, :K].double(), T * 2.0 ** -23 * absum, f"small_wgrad T={T} N={N} K={K}")
            assert torch.equal(cb[:, K:], cb0[:, K:])  # the columns beyond K untouched


@pytest.mark.parametrize("shape,inplace", [
    ((37, 100), False),    # odd rows, width no multiple of 8: 4-element vectors with row changes inside a wave
    ((5, 4), False),       # one vector per row
    ((1100, 2052), False),  # 564,300 vectors: beyond the 2048-block cap, a second grid-stride trip
    ((37, 100), True),     # in place (out is x), as cls_head's dgrad does
])
def test_dropout_bit_equal_reference(gpu, shape, inplace):
    C_ = _hip()._C
    n4 = shape[0] * shape[1] // 4
    blocks = min(2048, (n4 + 255) // 256)  # grid_for
    assert (n4 > blocks * 256) == (shape == (1100, 2052))
    torch.manual_seed(shape[0])
    x = torch.randn(*shape, device=gpu).bfloat16()
    seed = 0x1234ABCD5678
    want = ref.dropout(x, 0.1, seed, True)
    assert 0.85 < (want != 0).float().mean().item() < 0.95
    if inplace:
        out = x.clone()
        C_.dropout(out, out, 0.1, seed)
    else:
        out = torch.full_like(x, float("nan"))
        C_.dropout(x, out, 0.1, seed)
    assert torch.equal(out, want)


# ------------------------------------------------------------------------------------------------ 4. cross-entropy
def _xent_geometry(ld, V, dtype):
    """(vector path?, end of the 4-in-flight loop, end of the single-load loop = Vv) of xent_kernel's first pass."""
    VEC = 8 if dtype == torch.bfloat16 else 4
    vec = ld % VEC == 0
    Vv = V - V % VEC if vec else 0
    span = 4 * 64 * VEC
    j = 0
    while j + 3 * 64 * VEC < Vv:  # lane 0's trips
        j += span
    return vec, j, Vv


def _check_xent(gpu, logits, labels, V=0):
    """hip.cross_entropy (V == 0) or _C.xent on a padded row (V < ld) vs torch on the fp32 copy of the V real columns."""
    hip = _hip()
    dtype = logits.dtype
    R, ld = logits.shape
    if V:
        stats = torch.zeros(2, device=gpu)
        n_valid = labels.ne(-100).sum().float().reshape(1)
        dl = torch.full_like(logits, float("nan"))
        hip._C.xent(logits, labels, dl, stats, n_valid, V)
        loss, correct = stats[0] / n_valid.clamp(min=1.0), stats[1]
    else:
        V = ld
        lg = logits.clone().requires_grad_()
        loss, correct = hip.cross_entropy(lg, labels)
        loss.backward()
        dl = lg.grad
    l32 = logits[:, :V].detach().float().requires_grad_()
    want = torch.nn.functional.cross_entropy(l32, labels, ignore_index=-100)
    want.backward()
    assert abs(loss.item() - want.item()) < 1e-3 * max(1.0, abs(want.item())), (loss.item(), want.item())
    _close(dl[:, :V], l32.grad, 2e-2 if dtype == torch.bfloat16 else 1e-5, 1e-3, "dlogits")
    if V < ld:
        assert torch.count_nonzero(dl[:, V:]) == 0  # exact zeros on the padding
    keep = labels.ne(-100)
    assert int(correct.item()) == int((l32.argmax(-1) == labels)[keep].sum().item())


def _xent_labels(gpu, R, V):
    labels = torch.randint(0, V, (R,), device=gpu)
    if R > 2:
        labels[::5] = -100
    return labels


@pytest.mark.parametrize("R,V,dtype", [
    (5, 4, torch.float32),      # one 16-B load in lane 0 only; a second block with one row
    (3, 8, torch.float32),      # two lanes
    (9, 764, torch.float32),    # single-load loop only: 191 vectors, three trips, the last with 63 lanes
    (7, 768, torch.float32),    # 3 x 256 elements: still one short of a 4-in-flight trip
    (6, 1540, torch.float32),   # one 4-in-flight trip for every lane, then a remainder trip of 129 vectors
    (2, 4100, torch.float32),   # four 4-in-flight trips, then a single vector in lane 0
    (5, 8, torch.bfloat16),     # one 16-B load in lane 0 only
    (9, 1528, torch.bfloat16),  # single-load loop only: 191 vectors
    (7, 1536, torch.bfloat16),  # 3 x 512 elements: one short of a 4-in-flight trip
    (6, 1544, torch.bfloat16),  # first size past it: lane 0 alone takes the 4-in-flight trip
    (3, 8200, torch.bfloat16),  # four 4-in-flight trips, then a single vector in lane 0
    (1, 1544, torch.bfloat16),  # R = 1: the binding takes ld from the width, waves 1-3 of the block exit
    (1, 764, torch.float32),    # R = 1, fp32
])
def test_cross_entropy_16B_paths(gpu, R, V, dtype):
    vec, j4, Vv = _xent_geometry(V, V, dtype)
    assert vec and Vv == V
    assert (j4 > 0) == (V in (1540, 4100, 1544, 8200)), j4
    torch.manual_seed(R * 10000 + V)
    logits = (torch.randn(R, V, device=gpu) * 3).to(dtype)
    _check_xent(gpu, logits, _xent_labels(gpu, R, V))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cross_entropy_padded_rows(gpu, dtype):
    """V = 1003 scored columns in rows of 1008: the vector loops end at Vv (1000 for both types), the scalar tail
    takes Vv..V, and the padding (+50, far above every logit) enters neither the loss nor the argmax."""
    R, V, ld = 11, 1003, 1008
    vec, _, Vv = _xent_geometry(ld, V, dtype)
    assert vec and Vv == 1000 and Vv < V < ld
    torch.manual_seed(1003)
    logits = (torch.randn(R, ld, device=gpu) * 3).to(dtype)
    logits[:, V:] = 50.0
    _check_xent(gpu, logits, _xent_labels(gpu, R, V), V=V)


@pytest.mark.parametrize("dtype,padded", [(torch.float32, True), (torch.bfloat16, True), (torch.bfloat16, False),
                                          (torch.float32, False)])
def test_cross_entropy_tied_maxima(gpu, dtype, padded):
    """Integer logits on levels 0..3 with one to three copies of the top level 4 per row, at random columns: tied
    maxima in different lanes, different trips and (padded rows) the scalar tail. The count must follow torch's
    first-index argmax, so every label is the first maximum and every row must count."""
    R = 48
    V, ld = (1003, 1008) if padded else (2056, 2056)  # 2056: 4-in-flight trips in every lane + an 8-column remainder
    VEC = 8 if dtype == torch.bfloat16 else 4
    vec, _, Vv = _xent_geometry(ld, V, dtype)
    assert vec and (Vv < V) == padded
    torch.manual_seed(48)
    logits = torch.randint(0, 4, (R, ld), device=gpu).float()
    for r in range(R):
        k = 1 + r % 3
        cols = torch.randint(0, V, (k,), device=gpu)
        if padded and r % 4 == 0:
            cols = torch.randint(Vv, V, (k,), device=gpu)  # maxima in the scalar tail only
        if padded and r % 4 == 1:
            cols[0] = V - 1  # one in the tail, the others (if any) in the vector part
        logits[r, cols] = 4.0
    if padded:
        logits[:, V:] = 50.0
    logits = logits.to(dtype)
    labels = logits[:, :V].float().argmax(-1)
    assert len(set(((labels // VEC) % 64).tolist())) > 8  # the first maxima sit in many different lanes
    _check_xent(gpu, logits, labels, V=V if padded else 0)
    # and a label on a later copy of the maximum must not count
    later = torch.tensor([int((logits[r, :V] == 4).nonzero()[-1]) for r in range(R)], device=gpu)
    multi = later != labels
    assert int(multi.sum()) >= R // 2
    _check_xent(gpu, logits, later, V=V if padded else 0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cross_entropy_all_rows_ignored(gpu, dtype):
    """Every label -100: the project's convention is loss 0, gradient 0, count 0 (torch returns NaN here)."""
    hip = _hip()
    torch.manual_seed(1)
    logits = (torch.randn(6, 1544, device=gpu) * 3).to(dtype).requires_grad_()
    labels = torch.full((6,), -100, device=gpu, dtype=torch.long)
    loss, correct = hip.cross_entropy(logits, labels)
    loss.backward()
    assert loss.item() == 0.0 and correct.item() == 0.0
    assert torch.count_nonzero(logits.grad) == 0


def test_cross_entropy_minus_inf_first_fp32(gpu):
    """One fp32 row of 130 columns (ld % 4 != 0: the scalar loop) whose first element is -inf: lane 0's running
    maximum is -inf when it is first rescaled. torch's loss is finite.

    Before the guard in xent.hip (no rescale while the maximum is -inf) this row gave loss NaN and an all-NaN
    gradient: m - nm = -inf - (-inf)."""
    vec, _, _ = _xent_geometry(130, 130, torch.float32)
    assert not vec
    torch.manual_seed(130)
    logits = torch.randn(1, 130, device=gpu) * 3
    logits[0, 0] = float("-inf")
    _check_xent(gpu, logits, torch.tensor([17], device=gpu))


def test_cross_entropy_minus_inf_first_vector_bf16(gpu):
    """One bf16 row whose first 8 columns (lane 0's first 16-B load) are all -inf, in front of a second row without
    any. Same fault as the fp32 case, in the vector path's update."""
    V = 1544
    vec, j4, _ = _xent_geometry(V, V, torch.bfloat16)
    assert vec and j4 > 0
    torch.manual_seed(1544)
    logits = (torch.randn(2, V, device=gpu) * 3).bfloat16()
    logits[0, :8] = float("-inf")
    _check_xent(gpu, logits, torch.tensor([100, 3], device=gpu))


# ------------------------------------------------------------------------------------------------ 5. classification head
def _cls_case(gpu, R, C, H, act, p, labels=None):
    from huggingface_sagemaker_tensorflow_distributed_amd import ops

    torch.manual_seed(17 + R + C + H)
    S = 16
    mk = lambda *s, sc=0.05: (torch.randn(*s, device=gpu) * sc).bfloat16().requires_grad_()  # noqa: E731
    h = torch.randn(R, S, H, device=gpu).bfloat16().requires_grad_()
    # keep the pre-activation's scale independent of H (the existing test's 0.05 is sized for H >= 768)
    w1, b1, w2, b2 = mk(H, H, sc=1.0 / math.sqrt(H)), mk(H, sc=0.5), mk(C, H, sc=0.5), mk(C, sc=0.5)
    if labels is None:
        labels = torch.randint(0, C, (R,), device=gpu)
        if R > 1:
            labels[1] = -100  # an ignored row (eval-shard padding)
    p_in = p if act == "tanh" else 0.0  # RoBERTa's head drops its input too
    params = [h, w1, b1, w2, b2]
    loss, logits = ops.cls_head(h, w1, b1, w2, b2, labels, act, p_in, 21, p, 22)
    assert getattr(loss, "_hsd_stats", None) is not None, "the fused HIP head did not run"
    loss.backward()
    g_hip = [t.grad.float() for t in params]
    f = [t.detach().float().requires_grad_() for t in params]
    lg_ref = ref.cls_head(f[0][:, 0], f[1], f[2], f[3], f[4], act, p_in, 21, p, 22, True)
    return loss, logits, g_hip, f, lg_ref, labels


@pytest.mark.parametrize("C", [1, 4])  # the smallest and the largest class count the binding accepts
@pytest.mark.parametrize("R", [
    1,   # one row: waves 1-3 idle, the wave's 4-row loop breaks after the first
    5,   # wave 1 breaks after one row
    17,  # a second block with one row
    33,  # a third block with one row: three partials in the stats reduction
])
@pytest.mark.parametrize("H", [
    8,    # one lane of one 16-B chunk
    64,   # 8 lanes
    520,  # a second chunk with one lane
])
def test_cls_head_edges(gpu, C, R, H):
    assert R % 4 != 0  # a wave's 4-row loop breaks early
    for act, p in (("tanh", 0.0), ("tanh", 0.1), ("relu", 0.0), ("relu", 0.1)):
        what = f"act={act} p={p}"
        loss, logits, g_hip, f, lg_ref, labels = _cls_case(gpu, R, C, H, act, p)
        valid = labels.ne(-100)
        assert bool(valid.any())
        loss_ref = torch.nn.functional.cross_entropy(lg_ref, labels, ignore_index=-100)
        loss_ref.backward()
        assert abs(loss.item() - loss_ref.item()) < 2e-2 * max(1.0, abs(loss_ref.item())), (what, loss.item(), loss_ref.item())
        _close(logits, lg_ref, 3e-2, 3e-2, what + " logits")
        hits = (lg_ref.argmax(-1) == labels)[valid].sum().item()
        assert abs(loss._hsd_stats[1].item() - hits) <= 1 and loss._hsd_stats[2].item() == valid.sum().item()
        for n, a, b in zip(["h", "w1", "b1", "w2", "b2"], g_hip, [t.grad for t in f]):
            rel = (a - b).norm() / (b.norm() + 1e-6)
            assert rel < 4e-2, f"{what} {n}: rel err {rel:.3g}"
            # element-wise on the gradients derived from dpre (bf16 like the dense layers' dx / dw elsewhere in the
            # suite: 5e-2 of the tensor's scale + 5e-2 per element), where 0.1 % is at least one element
            if n == "h":
                a, b = a[:, 0], b[:, 0]  # the rows that carry gradient
            if n in ("h", "w1", "b1") and a.numel() >= 1000:
                _close(a, b, 5e-2, 5e-2, f"{what} d{n}")
        assert torch.count_nonzero(g_hip[0][:, 1:]) == 0  # only the first-token rows receive gradient


@pytest.mark.parametrize("act", ["tanh", "relu"])
def test_cls_head_all_rows_ignored(gpu, act):
    """Every label -100: loss 0, all five gradients exactly zero, no row scored."""
    R, C, H = 5, 4, 64
    labels = torch.full((R,), -100, device=gpu, dtype=torch.long)
    loss, logits, g_hip, f, lg_ref, _ = _cls_case(gpu, R, C, H, act, 0.1, labels=labels)
    assert loss.item() == 0.0
    assert loss._hsd_stats[2].item() == 0
    _close(logits, lg_ref, 3e-2, 3e-2, "logits")
    for n, a in zip(["h", "w1", "b1", "w2", "b2"], g_hip):
        assert torch.count_nonzero(a) == 0, n


# ------------------------------------------------------------------------------------------------ 6. Adam
@pytest.mark.parametrize("n", [
    64,          # a single partial wave: 16 of 256 threads, the second chunk of the pair beyond n4 for all of them
    64 * 3,      # 48 threads
    64 * 70001,  # 4,480,064: past 2048 blocks x 256 threads x 2 chunks, so a second grid-stride trip that ends
                 # inside the unrolled pair (the i >= n4 break)
])
@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("variant", [
    "host",  # host scalars, bf16 copy written
    "coef",  # device scalars (the host ones are garbage), no bf16 copy
])
def test_adam_edges(gpu, n, gdt, variant):
    hip = _hip()
    n4 = n // 4
    blocks = min(2048, (n4 + 255) // 256)  # launch_adam
    trips = -(-n4 // (blocks * 256 * 2))
    assert trips == (2 if n == 64 * 70001 else 1)
    if trips == 2:
        left = n4 - blocks * 256 * 2
        assert 0 < left < blocks * 256  # the second trip's first chunks end before the stride: its second chunks break
    torch.manual_seed(n % 1000 + (1 if variant == "host" else 2))
    pad = 128  # 64-aligned slices of larger buffers
    N = n + 2 * pad
    sl = slice(pad, pad + n)
    P = torch.randn(N, device=gpu)
    M = torch.randn(N, device=gpu).abs() * 0.1
    Vb = torch.randn(N, device=gpu).abs() * 0.1
    G = torch.randn(N, device=gpu).to(gdt)
    O = torch.randn(N, device=gpu).bfloat16()
    P0, M0, V0, G0, O0 = (t.clone() for t in (P, M, Vb, G, O))
    step, eps, b1, b2, gs, lr_wd = 1e-3, 1e-7, 0.9, 0.999, 0.5, 1e-2
    decay = (torch.rand(n // 64, device=gpu) < 0.5).to(torch.uint8)  # one flag per 64 elements of the slice
    decay[0] = 1
    if variant == "host":
        hip.adam_step(P[sl], M[sl], Vb[sl], G[sl], O[sl], decay, step, eps, b1, b2, gs, lr_wd)
    else:
        coef = torch.tensor([step, eps, gs, lr_wd], device=gpu, dtype=torch.float32)
        hip.adam_step(P[sl], M[sl], Vb[sl], G[sl], None, decay, 123.0, 456.0, b1, b2, 789.0, 0.5, coef=coef)
    torch.cuda.synchronize()
    # fp64 replay from the values the kernel received: the scalars rounded to fp32 (1 - b is exact in fp32)
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))  # noqa: E731
    step_, eps_, b1_, b2_, gs_, wd_ = f32(step), f32(eps), f32(b1), f32(b2), f32(gs), f32(lr_wd)
    gg = G0[sl].double() * gs_
    mr = b1_ * M0[sl].double() + (1 - b1_) * gg
    vr = b2_ * V0[sl].double() + (1 - b2_) * gg * gg
    wdf = torch.ones(n, device=gpu, dtype=torch.float64)
    wdf[decay.repeat_interleave(64).bool()] = f32(1.0 - wd_)
    pr = P0[sl].double() * wdf - step_ * mr / (vr.sqrt() + eps_)
    torch.testing.assert_close(P[sl].double(), pr, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(M[sl].double(), mr, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(Vb[sl].double(), vr, rtol=1e-5, atol=1e-6)
    if variant == "host":
        assert torch.equal(O[sl], P[sl].bfloat16())  # the bf16 copy is the updated weight rounded once
    else:
        assert torch.equal(O, O0)
    assert torch.equal(G, G0)  # zero_grad off: the gradient is only read
    for name, t, t0 in (("p", P, P0), ("m", M, M0), ("v", Vb, V0), ("out", O, O0)):
        assert torch.equal(t[:pad], t0[:pad]) and torch.equal(t[pad + n:], t0[pad + n:]), f"{name}: outside the slice"
