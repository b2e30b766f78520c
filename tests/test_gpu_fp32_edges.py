"""The fp32 step kernels (csrc/kernels/fp32.hip, split2 of attention32m.hip) at their edge shapes, through the `_C`
bindings, against fp64 references computed from the same fp32 inputs -- or the exact fp32 expression where the result
is determined bit for bit (the splits, the bias / residual epilogues, dropout, the embedding gather).

Every case names the branch its shape was chosen to reach; where that depends on launch geometry the test recomputes the
geometry with the launcher's formula (tests/fp32_edge_cases.py) and asserts the property it relies on, so a retune of a
launcher fails here instead of silently losing the coverage. Every output is a contiguous, 16-byte-aligned slice of a
larger allocation (fp32_edge_cases.Guard): NaN-filled for pure outputs, which must hold no NaN afterwards, a known
value around accumulate-into targets; the guard elements must come back unchanged. The shared case tables and
references are pinned on the CPU by tests/test_fp32_edge_references.py.

Tolerances. U = 2^-24. Each fp32 operation contributes a relative U; a sum of n terms in any grouping is bounded by
(n - 1) U sum|terms|; accumulation by atomics is one more grouping, and a non-zero start value one more term. A fused
multiply-add only removes a rounding, so the bounds hold whether or not the compiler contracts. Every comparison is per
element with no exceptions (`_within`). The bounds are derived next to the reference they belong to
(fp32_edge_cases.ln_fwd_ref, ln_bwd_ref, attn_fwd_bounds, attn_bwd_bounds) or in the docstring of the test.

Device math calls (erff, expf, tanhf, rsqrtf, exp2f, __log2f, logf): the local ROCm documentation ships no accuracy
table, so each allowance is measured: the same expression is evaluated in fp32 on
the host and compared with fp64 on the test family's own inputs (never with the kernel), in units that follow the
expression's error structure (fp32_edge_cases.*_unit); the kernel is allowed MATH_MARGIN = 8 times the host's worst
ratio, because device and host libm may differ by a few ulp each and nobody has measured that here. The ratio is
recomputed on every run (the inputs are seeded on the CPU); the value seen when the test was written stands in the
docstring of the test that uses it.
"""
import math

import pytest
import torch

import fp32_edge_cases as F
from fp32_edge_cases import Guard, U

pytestmark = pytest.mark.gpu

from huggingface_sagemaker_tensorflow_distributed_amd.ops import reference as ref  # noqa: E402
from huggingface_sagemaker_tensorflow_distributed_amd.ops.rng import keep_mask  # noqa: E402

BF = torch.bfloat16
F32 = torch.float32


@pytest.fixture
def C_(gpu):
    from huggingface_sagemaker_tensorflow_distributed_amd.ops import hip32

    return hip32._C


def _sync():
    """Wait for the kernels (tests/test_fp32_edge_references.py runs these checks on the CPU against an fp32 torch
    emulation of every binding: nothing to wait for there)."""
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def _within(a, r, bound, what):
    """|a - r| <= bound element-wise (fp64), no exceptions."""
    err = (a.double() - r).abs()
    bound = bound.expand_as(err)
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    bad = int((err > bound).sum().item())
    print(f"{what}: worst err / bound = {ratio:.4f}")
    assert bad == 0, f"{what}: {bad} elements beyond the bound, worst err / bound = {ratio:.3f}"


def _start_value(absum, gen_seed):
    """Non-zero start of an accumulate-into target: 0.5 * sum|terms| with a random sign: with the start as one more term
    n terms stay below n * 2^-24 * 1.5 * sum|terms| < n * 2^-23 * sum|terms|."""
    g = torch.Generator(device="cpu").manual_seed(gen_seed)
    sign = (torch.randint(0, 2, absum.shape, generator=g).double() * 2 - 1).to(absum.device)
    return (0.5 * absum * sign).float()


def _cpu_randn(shape, seed, device, scale=1.0, shift=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + shift).to(device)


def _cpu_rand(shape, seed, device):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.rand(shape, generator=g).to(device)


def _halves(shape, gpu):
    return Guard(shape, BF, gpu), Guard(shape, BF, gpu)


def _check_halves(hi, lo, out, what):
    rh, rl = F.split_halves(out)
    assert F.same_bits(hi.check(what + " hi"), rh), what + ": hi != bf16(out)"
    assert F.same_bits(lo.check(what + " lo"), rl), what + ": lo != bf16(out - hi)"


# ------------------------------------------------------------------------------------------------ 1. splits
def _split3_case(C_, gpu, x, pat, rows):
    R, C = x.shape
    out = Guard((3 * R, C) if rows else (R, 3 * C), BF, gpu)
    C_.split3(x, out.t, pat, rows)
    _sync()
    assert F.same_bits(out.check(f"split3 pat {pat} rows {rows}"), F.split3_ref(x, pat, rows)), (pat, rows)


def _split3_dual_case(C_, gpu, x, pat_cols, pat_rows):
    R, C = x.shape
    cols, rows = Guard((R, 3 * C), BF, gpu), Guard((3 * R, C), BF, gpu)
    C_.split3_dual(x, cols.t, pat_cols, rows.t, pat_rows)
    _sync()
    assert F.same_bits(cols.check("split3_dual cols"), F.split3_ref(x, pat_cols, False))
    assert F.same_bits(rows.check("split3_dual rows"), F.split3_ref(x, pat_rows, True))


@pytest.mark.parametrize("C", [40, 12])
def test_split3_every_pattern_bit_exact(C_, gpu, C):
    """Every block pattern 0..7 in both layouts at (3, C): block b takes bit b of `pat` (a reversed bit order swaps
    patterns 1 and 4, 3 and 6), V = 8 (C = 40) and V = 4 (C = 12). Inputs span 2^-100 .. 2^100 with +-0; subnormal
    results are outside the contract and the inputs keep away from them (fp32_edge_cases.wide_range_input)."""
    assert F.split3_geometry(3, C)[0] == (8 if C == 40 else 4)
    x = F.wide_range_input((3, C), 11 + C, gpu)
    for pat in range(8):
        for rows in (False, True):
            _split3_case(C_, gpu, x, pat, rows)
    for pat in range(8):
        _split3_dual_case(C_, gpu, x, pat, 7 - pat)


@pytest.mark.parametrize("R,C,why", F.SPLIT_SMALL)
def test_split3_small_shapes(C_, gpu, R, C, why):
    V, cvn, groups, stride = F.split3_geometry(R, C)
    assert V == (8 if C % 8 == 0 else 4) and groups < 256  # one partly filled block
    x = F.wide_range_input((R, C), 100 * R + C, gpu)
    _split3_case(C_, gpu, x, 0b100, False)
    _split3_case(C_, gpu, x, 0b010, True)
    _split3_dual_case(C_, gpu, x, 0b100, 0b011)


@pytest.mark.parametrize("R,C,why", F.SPLIT_SECOND_TRIP + [F.SPLIT_WIDE_ROW])
def test_split3_second_grid_stride_trip(C_, gpu, R, C, why):
    """More groups than the 2048 x 256 threads of the grid: the second trip of the loop, the only place where the
    incremental (row, column) advance runs, with a stride that is no multiple of the row's groups (the wrap) or, for
    the wide row, smaller than one row (sr == 0)."""
    V, cvn, groups, stride = F.split3_geometry(R, C)
    assert stride == 2048 * 256 and groups > stride and stride % cvn != 0
    if R == 2:
        assert stride < cvn and groups > 2 * stride  # sr == 0, a third trip
    else:
        assert stride // cvn > 0 and (stride % cvn) * 2 >= cvn  # some thread wraps on its first advance
    x = F.wide_range_input((R, C), R + C, gpu)
    _split3_case(C_, gpu, x, 0b100, False)
    _split3_dual_case(C_, gpu, x, 0b001, 0b110)


@pytest.mark.parametrize("n", [4, 4 * 300, F.SPLIT2_N])
def test_split2_bit_exact_with_tail_past_the_block_cap(C_, gpu, n):
    """split2: one group; two blocks, the second partly filled; and 4096 x 256 + 37 groups, 37 threads of which make a
    second trip past launch_split2's cap of 4096 blocks."""
    groups, stride = F.split2_geometry(n)
    if n == F.SPLIT2_N:
        assert stride == 4096 * 256 and groups - stride == 37
    else:
        assert groups <= stride and (groups == 1 or (groups > 256 and groups % 256))
    x = F.wide_range_input((n,), n % 1000, gpu)
    hi, lo = _halves((n,), gpu)
    C_.split2(x, hi.t, lo.t)
    _sync()
    _check_halves(hi, lo, x, "split2")


# ------------------------------------------------------------------------------------------------ 2. epi32
def _epi_inputs(M, N, seed, gpu):
    """y with 0.5 <= |y| < 1.5 and |bias| <= 0.25, so |y + bias| >= 0.25: a kept dropout element never equals its
    residual."""
    y = (_cpu_rand((M, N), seed, gpu) + 0.5) * (torch.randint(0, 2, (M, N), generator=torch.Generator().manual_seed(
        seed + 1)).float() * 2 - 1).to(gpu)
    bias = (_cpu_rand((N,), seed + 2, gpu) - 0.5) * 0.5
    res = _cpu_randn((M, N), seed + 3, gpu)
    return y, bias, res


def _gelu_inputs(M, N, seed, gpu):
    """Pre-activations y + bias spread over [-12, 12], with exact zeros (y = -bias) and the ends +-12."""
    y = _cpu_rand((M, N), seed, gpu) * 24 - 12
    bias = (_cpu_rand((N,), seed + 2, gpu) - 0.5) * 0.5
    bias[0] = 0.0
    yf = y.view(-1)
    yf[0] = 0.0
    yf[1] = -bias[1 % N]
    yf[2] = 12.0
    yf[3] = -12.0
    return y.contiguous(), bias


def _epi_run(C_, gpu, kind, y, bias, aux, p, seed, want_out, want_halves):
    """One epi32 call inside guards -> (y after the call, out or None, hi, lo guards or None)."""
    yg = Guard(y.shape, F32, gpu, init=y)
    out = Guard(y.shape, F32, gpu) if want_out else None
    hi, lo = _halves(y.shape, gpu) if want_halves else (None, None)
    C_.epi32(yg.t, bias, aux, out.t if out else None, kind, p, seed, hi.t if hi else None, lo.t if lo else None)
    _sync()
    what = f"epi32 kind {kind} {tuple(y.shape)}"
    yg.check(what + " y")
    return yg.t, (out.check(what + " out") if out else None), hi, lo


def _epi_variants(C_, gpu, kind, y, bias, aux, p, seed, check):
    """out only; out + halves; for kinds 0 / 1 halves only (compared with the twin call's out)."""
    ya, out, _, _ = _epi_run(C_, gpu, kind, y, bias, aux, p, seed, True, False)
    check(ya, out)
    ya2, out2, hi, lo = _epi_run(C_, gpu, kind, y, bias, aux, p, seed, True, True)
    assert F.same_bits(out2, out) and F.same_bits(ya2, ya)
    _check_halves(hi, lo, out2, f"epi32 kind {kind}")
    if kind <= 1:
        ya3, _, hi, lo = _epi_run(C_, gpu, kind, y, bias, aux, p, seed, False, True)
        assert F.same_bits(ya3, ya)
        _check_halves(hi, lo, out, f"epi32 kind {kind} without out")


@pytest.mark.parametrize("M,N", F.EPI_SHAPES)
def test_epi32_bias_residual_kinds_bit_exact(C_, gpu, M, N):
    """Kind 0 = y + bias, kind 3 = y + aux, kind 2 at p = 0 = (y + bias) + res: single fp32 additions, bit exact.
    (1, 4): one group; (3, 12): N4 = 3, rows of three groups; (5, 260): N4 = 65, two blocks."""
    y, bias, res = _epi_inputs(M, N, 7 * M + N, gpu)

    def exact(want, y_kept=True):
        def check(ya, out):
            assert F.same_bits(out, want)
            assert F.same_bits(ya, y)  # kinds 0, 2, 3 leave y alone
        return check

    _epi_variants(C_, gpu, 0, y, bias, None, 0.0, 0, exact(y + bias))
    _epi_variants(C_, gpu, 0, y, None, None, 0.0, 0, exact(y))
    _epi_variants(C_, gpu, 3, y, None, res, 0.0, 0, exact(y + res))
    _epi_variants(C_, gpu, 2, y, bias, res, 0.0, 5, exact((y + bias) + res))


def _check_dropres(out, y, bias, res, p, seed):
    """Kind 2 at p > 0: out != res exactly where ops/rng.keep_mask keeps (|y + bias| >= 0.25 there), out == res bit for
    bit where it drops, and kept values within 2^-23 (|v s| + |res|) of v s + res (v = fp32(y + bias), s = fp32(1 /
    (1 - p))): two roundings of U each, one if the compiler contracts the multiply-add."""
    keep = keep_mask(seed, tuple(y.shape), p, device=y.device)
    v = (y + bias).double()
    s = float(torch.tensor(1.0 / (1.0 - p), dtype=F32))
    assert bool(((out != res) == keep).all()), "dropout zero pattern != keep_mask"
    assert F.same_bits(out[~keep], res[~keep])
    want = v * s + res.double()
    bound = 2.0 ** -23 * ((v * s).abs() + res.double().abs())
    _within(out[keep], want[keep], bound[keep], "epi32 kind 2 kept values")


@pytest.mark.parametrize("M,N", F.EPI_SHAPES)
def test_epi32_dropout_residual_matches_keep_mask(C_, gpu, M, N):
    y, bias, res = _epi_inputs(M, N, 9 * M + N, gpu)
    _epi_variants(C_, gpu, 2, y, bias, res, 0.1, 4242, lambda ya, out: (_check_dropres(out, y, bias, res, 0.1, 4242),
                                                                         F.same_bits(ya, y)))


def _gelu_family(gpu):
    return [(M, N) + _gelu_inputs(M, N, 31 * M + N, gpu) for M, N in F.EPI_SHAPES]


def test_epi32_gelu_forward_against_fp64(C_, gpu):
    """Kind 1 writes the pre-activation v = y + bias back bit exact and out = 0.5 v (1 + erff(v / sqrt 2)): within
    8 x r x gelu_unit of fp64, gelu_unit = U (|v| + |gelu(v)|) (the roundings of erff and of 1 + erf are absolute,
    0.5 |v| U each). r = worst host-fp32 / unit ratio over the three shapes' inputs (|v| up to 12, exact zeros, where
    the unit and so the bound is 0): measured 0.80 when written, so the kernel is allowed 6.4 units."""
    fam = _gelu_family(gpu)
    r = max(F.host_ratio(F.gelu32_host(y + b), F.gelu64(y + b), F.gelu_unit(y + b)) for _, _, y, b in fam)
    print(f"gelu forward: host ratio r = {r:.4f}")
    assert 0.05 < r < 4.0  # a host evaluation this far off would not be a measure of rounding
    for M, N, y, b in fam:
        v = y + b
        assert bool((v == 0).any()) and float(v.abs().max()) >= 11.5

        def check(ya, out):
            assert F.same_bits(ya, v)
            _within(out, F.gelu64(v), F.MATH_MARGIN * r * F.gelu_unit(v), f"gelu {M}x{N}")
            assert bool((out[v == 0] == 0).all())
        _epi_variants(C_, gpu, 1, y, b, None, 0.0, 0, check)


def test_epi32_gelu_backward_against_fp64(C_, gpu):
    """Kind 4: out = y (Phi(x) + x phi(x)) with x = aux the saved pre-activation: within 8 x r x dgelu_unit of fp64,
    dgelu_unit = U |y| (1 + |gelu'(x)|). r measured 1.14 when written (9.1 units allowed)."""
    fam = [(M, N, _cpu_randn((M, N), 5 * M + N, gpu), _gelu_inputs(M, N, 77 * M + N, gpu)[0]) for M, N in F.EPI_SHAPES]
    r = max(F.host_ratio(F.dgelu32_host(y, x), y.double() * F.dgelu64(x), F.dgelu_unit(y, x)) for _, _, y, x in fam)
    print(f"gelu backward: host ratio r = {r:.4f}")
    assert 0.05 < r < 4.0
    for M, N, y, x in fam:
        assert bool((x == 0).any()) and float(x.abs().max()) >= 11.5

        def check(ya, out):
            assert F.same_bits(ya, y)
            _within(out, y.double() * F.dgelu64(x), F.MATH_MARGIN * r * F.dgelu_unit(y, x), f"gelu' {M}x{N}")
        _epi_variants(C_, gpu, 4, y, None, x, 0.0, 0, check)


def test_epi32_second_grid_stride_trip(C_, gpu):
    """(180000, 12): 540000 groups on 2048 x 256 threads with N4 = 3 and stride % 3 = 2: on the second trip a wrong
    column wrap moves the bias column (kind 0) and the dropout row (kind 2, p = 0.1)."""
    M, N = F.EW_SECOND_TRIP
    N4, groups, stride = F.ew4_geometry(M, N)
    assert stride == 2048 * 256 and groups > stride and stride % N4 == 2 and stride // N4 > 0
    y, bias, res = _epi_inputs(M, N, 3, gpu)
    ya, out, hi, lo = _epi_run(C_, gpu, 0, y, bias, None, 0.0, 0, True, True)
    assert F.same_bits(out, y + bias) and F.same_bits(ya, y)
    _check_halves(hi, lo, out, "epi32 kind 0 second trip")
    ya, out, hi, lo = _epi_run(C_, gpu, 2, y, bias, res, 0.1, 99, True, True)
    _check_dropres(out, y, bias, res, 0.1, 99)
    _check_halves(hi, lo, out, "epi32 kind 2 second trip")
    ya, out, _, _ = _epi_run(C_, gpu, 2, y, bias, res, 0.0, 99, True, False)
    assert F.same_bits(out, (y + bias) + res)


# ------------------------------------------------------------------------------------------------ 3. dropout32
@pytest.mark.parametrize("shape", F.DROPOUT_SHAPES + [F.EW_SECOND_TRIP])
def test_dropout32_equals_reference_bit_for_bit(C_, gpu, shape):
    """out == ops/reference.dropout(x) bit for bit: the reference multiplies by the mask and then by fp32(1 / (1 - p)),
    the kernel by keep ? fp32(1 / (1 - p)) : 0 -- one rounding either way, the same one (no division in either). The
    mask row is the flattened leading dimensions ((2, 3, 20): 6 rows of 20). Out of place, in place, with halves."""
    rows = 1
    for d in shape[:-1]:
        rows *= d
    W4, groups, stride = F.ew4_geometry(rows, shape[-1])
    if tuple(shape) == F.EW_SECOND_TRIP:
        assert groups > stride and stride % W4 == 2
    else:
        assert groups < 256
    x = _cpu_randn(shape, sum(shape), gpu)
    want = ref.dropout(x, 0.1, 777)
    assert bool((want == 0).any()) or x.numel() <= 4
    out = Guard(shape, F32, gpu)
    C_.dropout32(x, out.t, 0.1, 777, None, None)
    _sync()
    assert F.same_bits(out.check("dropout32"), want)
    io = Guard(shape, F32, gpu, init=x)
    hi, lo = _halves(shape, gpu)
    C_.dropout32(io.t, io.t, 0.1, 777, hi.t, lo.t)
    _sync()
    assert F.same_bits(io.check("dropout32 in place"), want)
    _check_halves(hi, lo, want, "dropout32")


# ------------------------------------------------------------------------------------------------ 4. colsum32
def _colsum_case(C_, gpu, M, N):
    x = _cpu_randn((M, N), 1000 * M + N, gpu)
    absum = x.double().abs().sum(0)
    start = _start_value(absum, M + N)
    d = Guard((N,), F32, gpu, init=start)
    C_.colsum32(x, d.t)
    _sync()
    _within(d.check("colsum32"), start.double() + x.double().sum(0), M * 2.0 ** -23 * absum, f"colsum32 {M}x{N}")


@pytest.mark.parametrize("N", F.COLSUM_VECTOR_N)
@pytest.mark.parametrize("M", F.COLSUM_VECTOR_M + F.COLSUM_LONG_M)
def test_colsum32_vector_path(C_, gpu, M, N):
    """16-byte path (N % 4 == 0), dbias += column sums from a non-zero start: |err| <= M 2^-23 sum|x| (M terms and the
    start in any grouping, `_start_value`). N = 4: one lane; N = 260: the second block column has one active lane.
    M = 1 .. 17: the unrolled loop's `r + 12 < r1` boundary in each of the four row groups; 255 / 256 / 257: the grid's
    y going from 1 to 2 (129 + 128 rows); 4097: 17 blocks of exactly 241 rows (odd, so every row group ends in the
    tail loop); 4100: 17 blocks of 242 rows, the last one short (228)."""
    path, gx, gy, rpb = F.colsum32_geometry(M, N)
    assert path == "vector" and gx == (1 if N == 4 else 2) and (N - 1) // 4 % 64 == 0
    if M <= 256:
        assert (gy, rpb) == (1, M)
    elif M == 257:
        assert (gy, rpb) == (2, 129)
    elif M == 4097:
        assert (gy, rpb) == (17, 241) and gy * rpb == M
    else:
        assert (gy, rpb) == (17, 242) and M - (gy - 1) * rpb == 228
    _colsum_case(C_, gpu, M, N)


@pytest.mark.parametrize("N", F.COLSUM_SCALAR_N)
@pytest.mark.parametrize("M", F.COLSUM_SCALAR_M)
def test_colsum32_scalar_path(C_, gpu, M, N):
    """Scalar path (N % 4 != 0), 64 columns per block: N = 1, 63 (one partly filled block), 65 and 130 (a last block
    with 1 and 2 columns). The launcher asks for up to 1024 block rows, so every M here runs one row per block (three of
    the four row groups idle), except M = 1000 at N = 130 (three block columns: 682 block rows at the most, two rows
    per block)."""
    path, gx, gy, rpb = F.colsum32_geometry(M, N)
    assert path == "scalar" and gx == F.ceil_div(N, 64)
    assert (rpb, gy) == ((2, 500) if (M, N) == (1000, 130) else (1, M))
    _colsum_case(C_, gpu, M, N)


# ------------------------------------------------------------------------------------------------ 5. LayerNorm
def _ln_rows(kind, R, H, seed, gpu):
    if kind == "randn":
        return _cpu_randn((R, H), seed, gpu)
    return _cpu_randn((R, H), seed, gpu, shift=1000.0)  # mean 1000, standard deviation 1


def _ln_params(H, gpu):
    return _cpu_randn((H,), H, gpu, 0.1, 1.0), _cpu_randn((H,), H + 1, gpu, 0.1)


def _ln_family(gpu):
    return [(kind, R, H, _ln_rows(kind, R, H, 13 * H + R, gpu)) for H in F.LN_H for R in F.LN_R
            for kind in ("randn", "mean1000")]


def _rsqrt_ratio(fam, eps):
    """Host fp32 rsqrt against fp64 at the family's own fp32(var + eps) values, in units of U rstd."""
    v = torch.cat([F.ln_fwd_ref(x, x[0], x[0], eps)[2].pow(-2).float().cpu() for _, _, _, x in fam])
    return F.host_ratio(v.rsqrt(), v.double().rsqrt(), U * v.double().rsqrt())


def _ln_fwd_case(C_, gpu, x, g, b, eps, a_rsqrt, what, halves=True):
    R, H = x.shape
    out, mean, rstd = Guard((R, H), F32, gpu), Guard((R,), F32, gpu), Guard((R,), F32, gpu)
    hi, lo = _halves((R, H), gpu) if halves else (None, None)
    C_.ln32_fwd(x, g, b, out.t, mean.t, rstd.t, eps, hi.t if hi else None, lo.t if lo else None)
    _sync()
    ro, rm, rr, bd = F.ln_fwd_ref(x, g, b, eps)
    br = bd["rstd"] + a_rsqrt * U * rr
    _within(mean.check(what + " mean"), rm, bd["mean"], what + " mean")
    _within(rstd.check(what + " rstd"), rr, br, what + " rstd")
    _within(out.check(what + " out"), ro, F.ln_out_bound(ro, rr, br, bd["d"], bd["D"], g), what + " out")
    if halves:
        _check_halves(hi, lo, out.t, what)


@pytest.mark.parametrize("H", F.LN_H)
def test_ln32_fwd_widths_and_offset_rows(C_, gpu, H):
    """NJ = 1 (H <= 256), 2 (<= 512) and 4, each with a partial last chunk (4, 252, 260, 516, 1020; at 516 NJ = 4 runs
    with one chunk empty), R = 1, 3, 5 (blocks of four waves with idle waves). Rows of unit variance around 0 and
    around 1000: a one-pass variance E[x^2] - mean^2 loses the latter (x^2 ~ 1e6 carries an ulp of 0.06) while the
    two-pass bound of fp32_edge_cases.ln_fwd_ref stays below 1 % of the variance at H = 4. mean, rstd and out are each
    checked, the halves equal the split of out. rsqrtf: 8 x r x U rstd on top, r = host rsqrt ratio over the family's
    var + eps values, measured 1.36 when written (10.9 units, against bounds of tens to hundreds of units)."""
    assert F.ln32_nj(H) == (1 if H <= 256 else 2 if H <= 512 else 4)
    fam = _ln_family(gpu)
    r = _rsqrt_ratio(fam, 1e-5)
    print(f"ln32 rsqrt: host ratio r = {r:.4f}")
    assert 0.05 < r < 4.0
    g, b = _ln_params(H, gpu)
    for kind, R, h, x in fam:
        if h == H:
            _ln_fwd_case(C_, gpu, x, g, b, 1e-5, F.MATH_MARGIN * r, f"ln32_fwd {kind} {R}x{H}")


@pytest.mark.parametrize("H", [4, 260, 1024])
def test_ln32_fwd_constant_rows(C_, gpu, H):
    """Rows of one small integer value with eps = 1e-12: every partial sum is an exact integer below 2^24 and the
    division returns the value, so mean is exact, every difference is 0, out == beta bit for bit and rstd =
    rsqrtf(fp32(1e-12)) within the rsqrt allowance: 8 x r x U rstd with r the host ratio over the LayerNorm family's
    var + eps values and this one (a single value says nothing about a worst case: 0.03 here), measured 1.36
    (10.9 U allowed)."""
    R = 3
    x = torch.tensor([-3.0, 2.0, 5.0], device=gpu)[:, None].expand(R, H).contiguous()
    g, b = _ln_params(H, gpu)
    out, mean, rstd = Guard((R, H), F32, gpu), Guard((R,), F32, gpu), Guard((R,), F32, gpu)
    C_.ln32_fwd(x, g, b, out.t, mean.t, rstd.t, 1e-12, None, None)
    _sync()
    assert F.same_bits(mean.check("mean"), x[:, 0].contiguous())
    assert F.same_bits(out.check("out"), b[None, :].expand(R, H).contiguous())
    e32 = torch.full((R,), 1e-12, dtype=F32)
    want = e32.double().rsqrt()
    r = max(F.host_ratio(e32.rsqrt(), want, U * want), _rsqrt_ratio(_ln_family(gpu), 1e-5))
    print(f"ln32 rsqrt at eps: host ratio r = {r:.4f}")
    assert 0.05 < r < 4.0
    _within(rstd.check("rstd"), want.to(gpu), (F.MATH_MARGIN * r * U * want).to(gpu), "ln32_fwd constant rows rstd")


def _ln_bwd_case(C_, gpu, R, H, alias, what):
    x = _cpu_randn((R, H), 3 * R + H, gpu, 1.5, 0.5)
    dy = _cpu_randn((R, H), 5 * R + H, gpu)
    g, b = _ln_params(H, gpu)
    _, m64, r64, _ = F.ln_fwd_ref(x, g, b, 1e-5)
    mean, rstd = m64.float(), r64.float()
    rdx, tg, tb, bdx = F.ln_bwd_ref(dy, x, mean, rstd, g)
    ag, ab = tg.abs().sum(0), tb.abs().sum(0)
    sg, sb = _start_value(ag, R + H), _start_value(ab, R + H + 1)
    dg, db = Guard((H,), F32, gpu, init=sg), Guard((H,), F32, gpu, init=sb)
    if alias:
        dx = Guard((R, H), F32, gpu, init=dy)
        C_.ln32_bwd(dx.t, x, mean, rstd, g, dx.t, dg.t, db.t)
    else:
        dx = Guard((R, H), F32, gpu)
        C_.ln32_bwd(dy, x, mean, rstd, g, dx.t, dg.t, db.t)
    _sync()
    _within(dx.check(what + " dx"), rdx, bdx, what + " dx")
    _within(dg.check(what + " dgamma"), sg.double() + tg.sum(0), (R + 3) * 2.0 ** -23 * ag, what + " dgamma")
    _within(db.check(what + " dbeta"), sb.double() + tb.sum(0), R * 2.0 ** -23 * ab, what + " dbeta")


@pytest.mark.parametrize("H", F.LN_H)
def test_ln32_bwd_widths(C_, gpu, H):
    """The backward at every width of the forward test, R = 1, 3, 5 (one row per wave, one block), dgamma / dbeta
    accumulating into a non-zero start: R terms (dgamma's carry 3 U each: xhat's two roundings and the product) and the
    start, summed per lane, over the block's four waves in LDS and by atomics: (R + 3) 2^-23 sum|dy xhat| and
    R 2^-23 sum|dy| with `_start_value`. dx against fp32_edge_cases.ln_bwd_ref. Once per width with dx aliasing dy."""
    for R in F.LN_R:
        rpw, waves, launched = F.ln32_bwd_geometry(R)
        assert rpw == 1 and waves == R and launched - waves == (4 - R % 4) % 4
        _ln_bwd_case(C_, gpu, R, H, R == 3, f"ln32_bwd {R}x{H}")


@pytest.mark.parametrize("R,H", F.LN_BWD_LONG)
def test_ln32_bwd_several_rows_per_wave(C_, gpu, R, H):
    """R = 1025: two rows per wave, the last wave has one row and three waves of the last block have none (they must
    add zeros); R = 2049: three rows per wave, 683 waves, one idle wave."""
    rpw, waves, launched = F.ln32_bwd_geometry(R)
    if R == 1025:
        assert (rpw, waves, launched) == (2, 513, 516) and R - (waves - 1) * rpw == 1
    else:
        assert (rpw, waves, launched) == (3, 683, 684) and R - (waves - 1) * rpw == 3
    _ln_bwd_case(C_, gpu, R, H, False, f"ln32_bwd {R}x{H}")


# ------------------------------------------------------------------------------------------------ 6. embeddings
def _ids(n, hi, seed, gpu):
    return torch.randint(0, hi, (n,), generator=torch.Generator().manual_seed(seed)).to(gpu)


@pytest.mark.parametrize("R", F.EMBED_R)
@pytest.mark.parametrize("H", F.GATHER_H)
def test_embed32_gather_bit_exact(C_, gpu, H, R):
    """x = (word[ids] + pos[pids]) + type[tids] in fp32, bit exact. H = 4: one lane; 260: a second trip of the 256-column
    loop with one lane; 772 and 1028: four and five trips, the last partial (any H % 4 == 0 is legal here). R = 1 and 5
    (a second block with one row). Without a type table, with one, and with a table but no ids (row 0)."""
    V, P, T = 11, 7, 3
    word, pos, typ = _cpu_randn((V, H), H, gpu), _cpu_randn((P, H), H + 1, gpu), _cpu_randn((T, H), H + 2, gpu)
    ids, pids, tids = _ids(R, V, R, gpu), _ids(R, P, R + 1, gpu), _ids(R, T, R + 2, gpu)
    if R == 5:
        tids[0] = 2
    for tt, tab, want in ((None, None, word[ids] + pos[pids]),
                          (tids, typ, (word[ids] + pos[pids]) + typ[tids]),
                          (None, typ, (word[ids] + pos[pids]) + typ[0])):
        x = Guard((R, H), F32, gpu)
        C_.embed32_gather(ids, pids, tt, word, pos, tab, x.t)
        _sync()
        assert F.same_bits(x.check("embed32_gather"), want)


def _scatter_case(C_, gpu, R, H, ids, pids, tids, use_pos, use_type, what):
    V, P, T = 11, 7, 3
    dx = _cpu_randn((R, H), 17 * R + H, gpu)
    tables = []
    for rows, idx, used, seed in ((V, ids, True, 1), (P, pids, use_pos, 2), (T, tids, use_type, 3)):
        start = _cpu_randn((rows, H), seed + H, gpu)
        tables.append((Guard((rows, H), F32, gpu, init=start), start, idx, used))
    C_.embed32_scatter(dx, ids, pids, tids if use_type else None, tables[0][0].t, tables[1][0].t if use_pos else None,
                       tables[2][0].t if use_type else None)
    _sync()
    for (gd, start, idx, used), name in zip(tables, ("gword", "gpos", "gtype")):
        got = gd.check(f"{what} {name}")
        if not used:
            assert F.same_bits(got, start)
            continue
        want = start.double().index_add(0, idx, dx.double())
        mag = start.double().abs().index_add(0, idx, dx.double().abs())
        n = torch.zeros(start.shape[0], dtype=torch.float64, device=gpu).index_add(0, idx, torch.ones(R, dtype=torch.float64, device=gpu))
        _within(got, want, n[:, None] * U * mag, f"{what} {name}")
        assert F.same_bits(got[n == 0], start[n == 0]), f"{what} {name}: an untouched row changed"


@pytest.mark.parametrize("H", F.SCATTER_H)
def test_embed32_scatter_into_nonzero_gradients(C_, gpu, H):
    """Table gradients by fp32 atomics into non-zero tables: a row hit n times sums n terms onto its start value,
    |err| <= n U (sum|terms| + |start|); rows no token names keep their bits. H = 1 and 63: part of one 64-lane trip;
    65: a second trip with one lane; 768: twelve trips (any H is legal here). R = 1 and 5; every token the same id; all
    rows on one position row; no position table; no type table; a type table without ids (row 0)."""
    V, P, T = 11, 7, 3
    for R in F.EMBED_R:
        ids, pids, tids = _ids(R, V, R, gpu), _ids(R, P, R + 1, gpu), _ids(R, T, R + 2, gpu)
        _scatter_case(C_, gpu, R, H, ids, pids, tids, True, True, f"scatter {R}x{H}")
    R = 5
    ids, pids, tids = _ids(R, V, 4, gpu), _ids(R, P, 5, gpu), _ids(R, T, 6, gpu)
    same = torch.full((R,), 7, dtype=torch.long, device=gpu)
    _scatter_case(C_, gpu, R, H, same, pids, tids, True, True, "scatter same id")
    _scatter_case(C_, gpu, R, H, ids, torch.full_like(pids, 1), tids, True, True, "scatter one position row")
    _scatter_case(C_, gpu, R, H, ids, pids, tids, False, True, "scatter without gpos")
    _scatter_case(C_, gpu, R, H, ids, pids, tids, True, False, "scatter without gtype")
    # a type table without ids: every token on row 0
    dx = _cpu_randn((R, H), H, gpu)
    start = _cpu_randn((T, H), H + 9, gpu)
    gw, gt = Guard((V, H), F32, gpu, init=torch.zeros(V, H)), Guard((T, H), F32, gpu, init=start)
    C_.embed32_scatter(dx, ids, pids, None, gw.t, None, gt.t)
    _sync()
    want = start.double()
    want[0] += dx.double().sum(0)
    mag = start.double().abs()
    mag[0] += dx.double().abs().sum(0)
    _within(gt.check("gtype row 0"), want, R * U * mag, "scatter type row 0")
    assert F.same_bits(gt.t[1:], start[1:])


# ------------------------------------------------------------------------------------------------ 7. cls head
def _cls_inputs(R, H, C, seed, gpu):
    """|pre| in [0.1, 2.1): no activation output is 0, so t_out's zero pattern is the dropout mask's (and relu's)."""
    pre = (_cpu_rand((R, H), seed, gpu) * 2 + 0.1) * (torch.randint(0, 2, (R, H), generator=torch.Generator().manual_seed(
        seed + 1)).float() * 2 - 1).to(gpu)
    W2 = _cpu_randn((C, H), seed + 2, gpu, 1.0 / math.sqrt(H))
    b2 = _cpu_randn((C,), seed + 3, gpu, 0.5)
    labels = _ids(R, C, seed + 4, gpu)
    return pre, W2, b2, labels


def _cls_family(gpu):
    return [(C, H, R, _cls_inputs(R, H, C, 1000 * C + 10 * H + R, gpu)) for C in F.CLS_C for H in F.CLS_H
            for R in F.CLS_R]


def _cls_ratios(gpu):
    """Host ratios over the whole family's inputs: tanh (unit U |tanh|), the per-row cross-entropy (ce_unit) and
    (softmax - onehot) g (dlogits_unit), the latter two at the fp32-rounded reference logits of the p = 0 tanh head."""
    fam = _cls_family(gpu)
    pre = torch.cat([i[0].reshape(-1) for _, _, _, i in fam])
    r_tanh = F.host_ratio(torch.tanh(pre.cpu()), torch.tanh(pre.double()), U * torch.tanh(pre.double()).abs())
    r_ce = r_dl = 0.0
    for C, H, R, (pre, W2, b2, labels) in fam:
        _, lg = F.cls_forward64(pre.double(), W2.double(), b2.double(), 0, 1.0, 1.0)
        lg32 = lg.float()
        r_ce = max(r_ce, F.host_ratio(F.ce_rows32_host(lg32, labels), F.ce_rows64(lg32.double(), labels),
                                      F.ce_unit(lg32, labels)))
        dl = torch.tensor([0.7], dtype=F32)
        g64 = float(dl.double()) / R
        r_dl = max(r_dl, F.host_ratio(F.dlogits32_host(lg32, labels, dl, R), F.dlogits64(lg32, labels, g64)[0],
                                      F.dlogits_unit(lg32, labels, g64)))
    return r_tanh, r_ce, r_dl


def _cls_case(C_, gpu, pre, W2, b2, labels, act, p, seed, ratios, what):
    a_tanh, a_ce, a_dl = (F.MATH_MARGIN * r for r in ratios)
    R, H = pre.shape
    C = W2.shape[0]
    s32 = float(torch.tensor(1.0 / (1.0 - p), dtype=F32)) if p > 0 else 1.0
    keep = keep_mask(seed, (R, H), p, device=gpu) if p > 0 else torch.ones(R, H, dtype=torch.bool, device=gpu)
    pre64 = pre.double().requires_grad_()
    W64, b64 = W2.double().requires_grad_(), b2.double().requires_grad_()
    t64, lg64 = F.cls_forward64(pre64, W64, b64, act, keep.double(), s32)
    t64d, lg64d = t64.detach(), lg64.detach()
    # ---- forward
    s0, s1 = 2.5, 3.0
    t_out, logits = Guard((R, H), F32, gpu), Guard((R, C), F32, gpu)
    stats = Guard((4,), F32, gpu, init=torch.tensor([s0, s1, -1.0, -2.0]))
    C_.cls32_fwd(pre, W2, b2, labels, t_out.t, logits.t, stats.t, act, p, seed)
    _sync()
    t_k = t_out.check(what + " t_out")
    if act == 0:
        assert bool(((t_k != 0) == keep).all()), what + ": t_out's zero pattern != keep_mask"
        bt = (a_tanh + 1) * U * t64d.abs()
        _within(t_k, t64d, bt, what + " t_out")
    else:
        assert bool(((t_k != 0) == (keep & (pre > 0))).all()), what + ": t_out's zero pattern"
        assert F.same_bits(t_k, torch.relu(pre) * (keep.float() * s32))  # one fp32 product
        bt = U * t64d.abs()
    blg = (bt @ W2.double().abs().t() + (H + 2) * U * (t64d.abs() @ W2.double().abs().t() + b2.double().abs())) * F.SECOND
    _within(logits.check(what + " logits"), lg64d, blg, what + " logits")
    ce = F.ce_rows64(lg64d, labels)
    bce = 2 * blg.max(1).values + a_ce * F.ce_unit(lg64d, labels)
    bs0 = bce.sum() + R * U * (ce.abs().sum() + s0)
    st = stats.check(what + " stats")
    _within(st[:1], (s0 + ce.sum()).reshape(1), bs0.reshape(1), what + " stats[0]")
    top = lg64d.topk(min(2, C), 1).values
    if C > 1:
        assert bool((top[:, 0] - top[:, 1] > 2 * blg.max(1).values).all())  # the argmax is decided
    hits = float((lg64d.argmax(1) == labels).sum())
    assert float(st[1]) == s1 + hits and float(st[2]) == -1.0 and float(st[3]) == -2.0
    # ---- backward, from fp32 inputs t and logits (the reference values rounded): the fp64 graph carries the same
    # values (straight-through) so that autograd differentiates what the kernel is given
    t_in, lg_in = t64d.float(), lg64d.float()
    dloss = torch.tensor([0.7], dtype=F32, device=gpu)
    t_st = t64 + (t_in.double() - t64d)
    lg_st = t_st @ W64.t() + b64
    lg_st = lg_st + (lg_in.double() - lg_st.detach())
    loss = F.ce_rows64(lg_st, labels).mean()
    loss.backward(dloss.double()[0])
    sW, sb = _cpu_randn((C, H), seed % 97, gpu), _cpu_randn((C,), seed % 89, gpu)
    dpre, dW2, db2 = Guard((R, H), F32, gpu), Guard((C, H), F32, gpu, init=sW), Guard((C,), F32, gpu, init=sb)
    C_.cls32_bwd(pre, t_in, W2, lg_in, labels, dloss, dpre.t, dW2.t, db2.t, act, p, seed)
    _sync()
    g64 = float(dloss.double()) / R
    dl, _ = F.dlogits64(lg_in, labels, g64)
    bdl = a_dl * F.dlogits_unit(lg_in, labels, g64)
    _within(db2.check(what + " db2"), sb.double() + b64.grad, bdl.sum(0) + R * U * (dl.abs().sum(0) + sb.double().abs()),
            what + " db2")
    tin = t_in.double().abs()
    bW = bdl.t() @ tin + U * (dl.abs().t() @ tin) + R * U * (dl.abs().t() @ tin + sW.double().abs())
    _within(dW2.check(what + " dW2"), sW.double() + W64.grad, bW * F.SECOND, what + " dW2")
    Wa = W2.double().abs()
    dt = dl @ W2.double()
    bdt = bdl @ Wa + (C + 1) * U * (dl.abs() @ Wa)
    if act == 0:
        th = torch.tanh(pre.double())
        da = 1 - th * th
        bda = 2 * th.abs() * a_tanh * U * th.abs() + U * th * th + U * da.abs()
    else:
        da, bda = (pre > 0).double(), torch.zeros_like(dt)
    kf = keep.double() * s32
    want = dt * kf * da
    bdpre = (kf * (da.abs() * bdt + dt.abs() * bda + bdt * bda) + 2 * U * want.abs()) * F.SECOND
    _within(dpre.check(what + " dpre"), pre64.grad, bdpre, what + " dpre")
    assert float((want - pre64.grad).abs().max()) <= 1e-12 * float(want.abs().max() + 1e-300)


@pytest.mark.parametrize("H", F.CLS_H)
@pytest.mark.parametrize("C", F.CLS_C)
def test_cls32_head_forward_and_backward(C_, gpu, C, H):
    """C = 1, 2, 8 classes (the register arrays' ends), H = 2 (one lane), 126 (63 lanes), 128, 130 (a second trip with
    one lane) and 768, R = 1 and 5 rows, tanh and relu, p = 0 and 0.1. t_out against the keep mask (tanh within (8 r + 1)
    U, relu bit exact), logits within sum_h bt |W2| + (H + 2) U (sum|t W2| + |b2|), stats[0:2] accumulating into
    (2.5, 3.0) -- the loss sum within the rows' bounds (2 max blg + 8 r ce_unit each) plus R U (sum|ce| + 2.5), the
    hit count exact -- dloss = 0.7, dW2 / db2 accumulating into non-zero starts, dpre / dW2 / db2 against fp64
    autograd. Host ratios over the whole family's inputs, measured when written: tanh 1.04 (U |tanh|), cross-entropy
    0.35 (ce_unit), (softmax - onehot) g 1.11 (dlogits_unit): 8.3, 2.8 and 8.9 units allowed."""
    ratios = _cls_ratios(gpu)
    print("cls32: host ratios tanh %.4f ce %.4f dlogits %.4f" % ratios)
    assert all(0.02 < r < 4.0 for r in ratios)
    for C2, H2, R, (pre, W2, b2, labels) in _cls_family(gpu):
        if (C2, H2) != (C, H):
            continue
        for act in (0, 1):
            for p in (0.0, 0.1):
                _cls_case(C_, gpu, pre, W2, b2, labels, act, p, 31337 + H + R, ratios, f"cls32 C{C} H{H} R{R} act{act} p{p}")


@pytest.mark.parametrize("C,a,b", [(2, 0, 1), (8, 2, 5)])
def test_cls32_first_of_two_equal_maxima_wins(C_, gpu, C, a, b):
    """Classes a < b share one weight row and one bias (10 above the rest), so their logits are equal and maximal in
    every row: the accuracy count must take the first index, as torch.argmax does. Labels a, b, a, a, other: three
    hits for the first index, one for the last."""
    R, H = 5, 130
    pre, W2, b2, _ = _cls_inputs(R, H, C, 5, gpu)
    W2[b] = W2[a]
    b2[a] = b2[b] = 10.0
    labels = torch.tensor([a, b, a, a, (b + 1) % C], device=gpu)
    t_out, logits = Guard((R, H), F32, gpu), Guard((R, C), F32, gpu)
    stats = Guard((2,), F32, gpu, init=torch.tensor([0.0, 1.0]))
    C_.cls32_fwd(pre, W2, b2, labels, t_out.t, logits.t, stats.t, 0, 0.0, 0)
    _sync()
    lg = logits.check("logits")
    assert bool((lg[:, a] == lg[:, b]).all()) and bool((lg.argmax(1) == a).all())
    assert float(stats.check("stats")[1]) == 1.0 + float((labels == a).sum())


# ------------------------------------------------------------------------------------------------ 8. attention
def _attn_inputs(S, gpu):
    B, heads = F.ATTN_B, F.ATTN_HEADS
    qkv = _cpu_randn((B * S, 3 * heads * 64), S, gpu)
    dout = _cpu_randn((B * S, heads * 64), S + 1, gpu)
    return qkv, dout


def _attn_ratios(gpu):
    """Host ratios of exp2 (at the family's own s - max arguments, unit U 2^x) and log2 (at the row sums l in [1, S],
    unit U max(1, |log2 l|))."""
    r_exp = r_log = 0.0
    for S in F.ATTN_S:
        qkv, _ = _attn_inputs(S, gpu)
        _, _, pc = F.attention64(qkv, None, F.ATTN_B, S, F.ATTN_HEADS, 0.0, 0, keep_mask)
        s2 = pc["s"] * F.LOG2E
        arg = (s2 - s2.max(-1, keepdim=True).values).float().cpu()
        r_exp = max(r_exp, F.host_ratio(torch.exp2(arg), torch.exp2(arg.double()), U * torch.exp2(arg.double())))
        l = torch.exp2(arg.double()).sum(-1).float()
        r_log = max(r_log, F.host_ratio(torch.log2(l), torch.log2(l.double()), U * torch.log2(l.double()).abs().clamp_min(1.0)))
    return r_exp, r_log


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("mask_kind", F.ATTN_MASKS)
@pytest.mark.parametrize("S", F.ATTN_S)
def test_attn32_vector_kernels_against_fp64(C_, gpu, S, mask_kind, p):
    """attn32_fwd / attn32_bwd at lengths the MFMA path rejects: S = 2 (one key pair of one tile), 34 (a partial second
    key tile), 62 (a partial query block), 66 (two query blocks, the second with two queries); B = 2, heads = 3; no
    mask, the last keys of sequence 1 masked, sequence 1 fully masked (uniform probabilities, lse <= -1e30), a finite
    bias of -2.5 on every third key of sequence 0 (the only case where the bias' log2(e) factor shows). out, lse and
    dqkv per element against a plain fp64 softmax attention (fp32_edge_cases.attention64, autograd for the backward)
    with the keep mask of ops/rng.py; bounds: fp32_edge_cases.attn_fwd_bounds / attn_bwd_bounds. dK and dV of masked
    keys are exactly 0. Host ratios measured when written: exp2 1.11 (U 2^x), log2 1.00 (U max(1, |log2 l|)): 8.9 and
    8.0 units allowed."""
    assert S % 128 != 0  # attn32m_supported: multiples of 128 only
    B, heads = F.ATTN_B, F.ATTN_HEADS
    H = heads * 64
    r_exp, r_log = _attn_ratios(gpu)
    print(f"attn32: host ratios exp2 {r_exp:.4f} log2 {r_log:.4f}")
    assert 0.05 < r_exp < 4.0 and 0.05 < r_log < 4.0
    a_exp, a_log = F.MATH_MARGIN * r_exp, F.MATH_MARGIN * r_log
    qkv, dout = _attn_inputs(S, gpu)
    mask, kept = F.attn_masks(mask_kind, B, S, gpu)
    seed = 2024 + S
    q64 = qkv.double().requires_grad_()
    out64, lse64, pc = F.attention64(q64, mask, B, S, heads, p, seed, keep_mask)
    pcd = {k: v.detach() for k, v in pc.items()}
    bo, blse, full = F.attn_fwd_bounds(pcd, mask, kept, B, S, heads, a_exp, a_log)
    out, lse = Guard((B * S, H), F32, gpu), Guard((B * heads * S,), F32, gpu)
    C_.attn32_fwd(qkv, mask, out.t, lse.t, B, S, heads, p, seed)
    _sync()
    what = f"attn32 S{S} {mask_kind} p{p}"
    _within(out.check(what + " out"), out64.detach(), bo, what + " out")
    full_rows = full.view(B, 1, 1).expand(B, heads, S).reshape(-1)
    lk = lse.check(what + " lse")
    assert bool((lk[full_rows] <= -1e30).all())
    _within(lk[~full_rows], lse64.detach()[~full_rows], blse[~full_rows], what + " lse")
    # ---- backward from the fp32-rounded reference o and lse (-1e30 where every key is masked, as the forward writes)
    o_in = out64.detach().float()
    lse_in = torch.where(full_rows, torch.full_like(lk, -1e30), lse64.detach().float())
    out64.backward(dout.double())
    dqkv, delta = Guard((B * S, 3 * H), F32, gpu), Guard((B * heads * S,), F32, gpu)
    C_.attn32_bwd(qkv, mask, o_in, dout, lse_in, dqkv.t, delta.t, B, S, heads, p, seed)
    _sync()
    delta.check(what + " delta")
    bd = F.attn_bwd_bounds(pcd, mask, kept, dout, lse_in, B, S, heads, a_exp)
    got = dqkv.check(what + " dqkv")
    _within(got, q64.grad, bd, what + " dqkv")
    if mask_kind == "tail":
        dead = (~kept).view(B * S)
        assert bool(dead.any()) and bool((got[dead][:, H:] == 0).all()), "dK / dV of masked keys must be exactly 0"


# ------------------------------------------------------------------------------------------------ bindings
def _z(gpu, *s, dt=F32):
    return torch.zeros(*s, device=gpu, dtype=dt)


def test_cls32_bwd_binding_rejects_what_the_launcher_aborts_on(C_, gpu):
    R, H, C = 3, 6, 2

    def call(H=H, labels=None, t=None, logits=None, dloss=None, W2=None):
        lab = _z(gpu, R, dt=torch.long) if labels is None else labels
        C_.cls32_bwd(_z(gpu, R, H), _z(gpu, R, H) if t is None else t, _z(gpu, C, H) if W2 is None else W2,
                     _z(gpu, R, C) if logits is None else logits, lab, _z(gpu, 1) if dloss is None else dloss,
                     _z(gpu, R, H), _z(gpu, C, H) if W2 is None else torch.zeros_like(W2), _z(gpu, C), 0, 0.0, 0)

    call()
    _sync()
    for bad in (dict(H=5),                                    # odd H: launch_cls32_bwd aborts
                dict(labels=_z(gpu, R, dt=torch.int32)),      # labels dtype
                dict(labels=_z(gpu, R - 1, dt=torch.long)),   # labels numel: an unchecked index
                dict(labels=_z(gpu, 2 * R, dt=torch.long)[::2]),  # labels not contiguous
                dict(labels=torch.zeros(R, dtype=torch.long)),    # labels on the host
                dict(t=_z(gpu, R, H - 2)), dict(logits=_z(gpu, R, C + 1)), dict(logits=_z(gpu, R - 1, C)),
                dict(dloss=_z(gpu, 0)), dict(W2=_z(gpu, 9, H))):  # more than 8 classes
        with pytest.raises(RuntimeError):
            call(**bad)


def test_attn32_bwd_binding_rejects_odd_lengths_and_wrong_widths(C_, gpu):
    def call(B=1, S=4, heads=1, qkv_w=None, lse_n=None):
        H = heads * 64
        w = 3 * H if qkv_w is None else qkv_w
        C_.attn32_bwd(_z(gpu, B * S, w), None, _z(gpu, B * S, H), _z(gpu, B * S, H),
                      _z(gpu, B * heads * S if lse_n is None else lse_n), _z(gpu, B * S, w), _z(gpu, B * heads * S), B, S,
                      heads, 0.0, 0)

    call()
    _sync()
    for bad in (dict(S=3), dict(qkv_w=2 * 64), dict(qkv_w=4 * 64), dict(lse_n=3), dict(S=0)):
        with pytest.raises(RuntimeError):
            call(**bad)
    with pytest.raises(RuntimeError):  # the forward's twin check
        C_.attn32_fwd(_z(gpu, 3, 192), None, _z(gpu, 3, 64), _z(gpu, 3), 1, 3, 1, 0.0, 0)


def test_ln32_bwd_binding_rejects_short_statistics(C_, gpu):
    R, H = 3, 8

    def call(mean_n=R, rstd_n=R, g_n=H, H=H):
        C_.ln32_bwd(_z(gpu, R, H), _z(gpu, R, H), _z(gpu, mean_n), _z(gpu, rstd_n), _z(gpu, g_n), _z(gpu, R, H), _z(gpu, H),
                    _z(gpu, H))

    call()
    _sync()
    for bad in (dict(rstd_n=R - 1), dict(mean_n=R - 1), dict(g_n=H - 4), dict(H=6), dict(H=1028)):
        with pytest.raises(RuntimeError):
            call(**bad)


def test_embed32_scatter_binding_rejects_mismatched_ids_and_tables(C_, gpu):
    R, H = 3, 5
    ids = _z(gpu, R, dt=torch.long)

    def call(pids=ids, tids=ids, gpos_w=H, gtype_w=H, ids_=ids):
        C_.embed32_scatter(_z(gpu, R, H), ids_, pids, tids, _z(gpu, 4, H), _z(gpu, 4, gpos_w), _z(gpu, 2, gtype_w))

    call()
    _sync()
    for bad in (dict(pids=_z(gpu, R - 1, dt=torch.long)), dict(tids=_z(gpu, R, dt=torch.int32)),
                dict(tids=_z(gpu, R - 1, dt=torch.long)), dict(gpos_w=H - 1), dict(gtype_w=H + 1),
                dict(ids_=_z(gpu, 2 * R, dt=torch.long)[::2]), dict(pids=_z(gpu, 2 * R, dt=torch.long)[::2]),
                dict(tids=torch.zeros(R, dtype=torch.long))):
        with pytest.raises(RuntimeError):
            call(**bad)


def test_embed32_gather_binding_rejects_a_narrow_type_table(C_, gpu):
    R, H = 3, 8
    ids = _z(gpu, R, dt=torch.long)

    def call(type_w=H, tids=ids, H=H):
        C_.embed32_gather(ids, ids, tids, _z(gpu, 4, H), _z(gpu, 4, H), _z(gpu, 2, type_w), _z(gpu, R, H))

    call()
    _sync()
    for bad in (dict(type_w=H - 4), dict(type_w=H + 4), dict(tids=_z(gpu, R - 1, dt=torch.long)), dict(H=6, type_w=6)):
        with pytest.raises(RuntimeError):
            call(**bad)
