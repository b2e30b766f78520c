"""The case tables, fp64 references and fp32 bounds of tests/test_gpu_fp32_edges.py, pinned without a GPU, so that an
error in a reference or a bound cannot hollow out the GPU tests:

* the launch geometry of every table row has the property the row is there for (tests/fp32_edge_cases.py);
* every fp64 reference agrees with ops/reference.py, torch.nn.functional or fp32 autograd at the same edge shapes;
* the GPU file's own checks (guards, bit-exact expectations, per-element bounds, the math-call allowances measured on
  the host) run here against `Emu`, an emulation of each `_C` binding in plain fp32 torch -- ops/reference.py where it
  has the op, torch.nn.functional and fp32 autograd elsewhere. An fp32 evaluation in some other grouping must sit
  inside every bound; and each check must fail for a deliberately wrong emulation (wrong bit order, one-pass variance,
  last-index argmax, a dropped log2(e), a missing row wrap): the mutation list of the GPU tests, rehearsed on the CPU.
"""
import math

import pytest
import torch
import torch.nn.functional as TF

import fp32_edge_cases as F
import test_gpu_fp32_edges as G
from huggingface_sagemaker_tensorflow_distributed_amd.ops import reference as ref
from huggingface_sagemaker_tensorflow_distributed_amd.ops.rng import keep_mask

CPU = torch.device("cpu")


# ------------------------------------------------------------------------------------------------ geometry
def test_split_tables_reach_the_second_trip_and_the_wrap():
    assert {F.split3_geometry(R, C)[0] for R, C, _ in F.SPLIT_SMALL} == {4, 8}
    assert {(R, C) for R, C, _ in F.SPLIT_SMALL} >= {(r, c) for r in (1, 3) for c in (8, 40, 4, 12)}
    for R, C, _ in F.SPLIT_SMALL:
        assert F.split3_geometry(R, C)[2] <= 256
    for R, C, _ in F.SPLIT_SECOND_TRIP:
        V, cvn, groups, stride = F.split3_geometry(R, C)
        assert groups > 2048 * 256 == stride and stride % cvn != 0 and stride // cvn > 0
        assert R * C <= 5.5e6  # about 5 M floats at the most
    assert {F.split3_geometry(R, C)[0] for R, C, _ in F.SPLIT_SECOND_TRIP} == {4, 8}
    R, C, _ = F.SPLIT_WIDE_ROW
    V, cvn, groups, stride = F.split3_geometry(R, C)
    assert V == 8 and cvn > stride and groups > 2 * stride
    groups, stride = F.split2_geometry(F.SPLIT2_N)
    assert stride == 4096 * 256 and groups == stride + 37
    W4, groups, stride = F.ew4_geometry(*F.EW_SECOND_TRIP)
    assert groups > 2048 * 256 == stride and stride % W4 != 0
    for shape in F.EPI_SHAPES:
        assert F.ew4_geometry(*shape)[1] in (1, 9, 325)


def _colsum_vector_trips(M):
    """(unrolled, tail) loop trips of each of the four row groups of colsum32_kernel's first block."""
    _, _, _, rpb = F.colsum32_geometry(M, 4)
    r1 = min(M, rpb)
    trips = []
    for rg in range(4):
        r, un, tail = rg, 0, 0
        while r + 12 < r1:
            un, r = un + 1, r + 16
        while r < r1:
            tail, r = tail + 1, r + 4
        trips.append((un, tail))
    return trips


def test_colsum_tables_cover_the_unrolled_loop_boundary_and_both_paths():
    t = {M: _colsum_vector_trips(M) for M in F.COLSUM_VECTOR_M}
    assert t[1] == [(0, 1), (0, 0), (0, 0), (0, 0)] and t[3][3] == (0, 0)
    assert t[13] == [(1, 0), (0, 3), (0, 3), (0, 3)]  # r + 12 == r1 - 1 in group 0, == r1 in group 1
    assert t[16] == [(1, 0)] * 4 and t[17] == [(1, 1), (1, 0), (1, 0), (1, 0)]
    assert [F.colsum32_geometry(M, 4)[2] for M in (255, 256, 257)] == [1, 1, 2]
    for N in F.COLSUM_VECTOR_N:
        assert F.colsum32_geometry(16, N)[0] == "vector"
    assert F.colsum32_geometry(4097, 260)[2:] == (17, 241) and F.colsum32_geometry(4100, 260)[2:] == (17, 242)
    assert 4100 - 16 * 242 == 228 < 242
    for N in F.COLSUM_SCALAR_N:
        for M in F.COLSUM_SCALAR_M:
            path, gx, gy, rpb = F.colsum32_geometry(M, N)
            assert path == "scalar" and gx == F.ceil_div(N, 64) and gy * rpb >= M
    assert {N % 64 for N in F.COLSUM_SCALAR_N} == {1, 63, 2}


def test_layernorm_tables_cover_every_chunk_count_with_a_partial_chunk():
    by_nj = {}
    for H in F.LN_H:
        assert H % 4 == 0 and H <= 1024
        by_nj.setdefault(F.ln32_nj(H), []).append(H)
    assert set(by_nj) == {1, 2, 4}
    for nj, hs in by_nj.items():
        assert any(h % 256 for h in hs) and any(h == 256 * nj for h in hs)
    assert F.ln32_nj(516) == 4 and F.ceil_div(516, 256) == 3  # NJ = 4 with one chunk empty
    assert F.ln32_bwd_geometry(1025) == (2, 513, 516) and F.ln32_bwd_geometry(2049) == (3, 683, 684)
    assert all(F.ln32_bwd_geometry(R)[0] == 1 for R in F.LN_R)
    assert all(H % 2 == 0 for H in F.CLS_H) and max(F.CLS_C) == 8
    assert all(S % 2 == 0 and S % 128 for S in F.ATTN_S)
    assert {S <= 32 for S in F.ATTN_S} == {True, False} and {S <= 64 for S in F.ATTN_S} == {True, False}


# ------------------------------------------------------------------------------------------------ references
def test_wide_range_input_keeps_clear_of_subnormals():
    x = F.wide_range_input((3000,), 1, CPU)
    nz = x[x != 0].abs()
    assert float(nz.min()) >= 2.0 ** -100 and float(nz.max()) < 2.0 ** 101
    assert bool((x == 0).any()) and bool((F.bits(x) == -2 ** 31).any())  # +0 and -0
    hi, lo = F.split_halves(x)
    l = (x - hi.float())
    assert float(l[l != 0].abs().min()) >= 2.0 ** -126  # normal numbers
    assert bool(((hi.double() + lo.double() - x.double()).abs() <= 2.0 ** -16 * x.double().abs()).all())
    big = F.wide_range_input((3, (1 << 20) + 5), 2, CPU)
    assert big.shape == (3, (1 << 20) + 5) and not F.same_bits(big[0, :1000].contiguous(), big[1, :1000].contiguous())


def test_split3_reference_layouts():
    x = F.wide_range_input((2, 4), 3, CPU)
    hi, lo = F.split_halves(x)
    assert F.same_bits(F.split3_ref(x, 0b001, False), torch.cat([lo, hi, hi], 1))
    assert F.same_bits(F.split3_ref(x, 0b100, False), torch.cat([hi, hi, lo], 1))
    assert F.same_bits(F.split3_ref(x, 0b110, True), torch.cat([hi, lo, lo], 0))


def test_gelu_references_match_torch():
    x = torch.linspace(-12, 12, 4001, dtype=torch.float64).requires_grad_()
    y = TF.gelu(x)
    y.sum().backward()
    assert float((F.gelu64(x.detach()) - y.detach()).abs().max()) < 1e-14
    assert float((F.dgelu64(x.detach()) - x.grad).abs().max()) < 1e-14
    x32 = x.detach().float()
    assert float((ref.gelu(x32).double() - F.gelu64(x32)).abs().max()) < 1e-6


@pytest.mark.parametrize("H", [4, 516, 1024])
def test_layernorm_references_match_torch(H):
    x = G._ln_rows("mean1000", 5, H, 1, CPU)
    g, b = G._ln_params(H, CPU)
    out, mean, rstd, _ = F.ln_fwd_ref(x, g, b, 1e-5)
    x64 = x.double().requires_grad_()
    g64, b64 = g.double().requires_grad_(), b.double().requires_grad_()
    want = TF.layer_norm(x64, (H,), g64, b64, 1e-5)
    assert float((out - want.detach()).abs().max()) < 1e-9
    dy = G._cpu_randn((5, H), 2, CPU)
    want.backward(dy.double())
    dx, tg, tb, _ = F.ln_bwd_ref(dy, x, mean, rstd, g)  # fp64 statistics passed straight through
    assert float((dx - x64.grad).abs().max()) < 1e-8
    assert float((tg.sum(0) - g64.grad).abs().max()) < 1e-8 and float((tb.sum(0) - b64.grad).abs().max()) < 1e-12


@pytest.mark.parametrize("mask_kind", F.ATTN_MASKS)
@pytest.mark.parametrize("S", F.ATTN_S)
def test_attention64_matches_the_fp32_reference_op(S, mask_kind):
    B, heads = F.ATTN_B, F.ATTN_HEADS
    qkv, _ = G._attn_inputs(S, CPU)
    mask, kept = F.attn_masks(mask_kind, B, S, CPU)
    assert bool(kept[0].all()) and (mask_kind != "tail" or (bool(kept[1].any()) and not bool(kept[1].all())))
    for p in (0.0, 0.1):
        out, lse2, _ = F.attention64(qkv, mask, B, S, heads, p, 5, keep_mask)
        want = ref.attention(qkv, mask, B, S, heads, p, 5, True)
        assert float((out - want.double()).abs().max()) < 2e-5
    x = qkv.view(B, S, 3, heads, 64).permute(2, 0, 3, 1, 4).double()
    s = torch.matmul(x[0], x[1].transpose(-1, -2)) / 8.0
    if mask is not None:
        s = s + mask.double().view(B, 1, 1, S)
    assert float((lse2.view(B, heads, S) - torch.log2(torch.exp2((s - s.max(-1, keepdim=True).values) * F.LOG2E).sum(-1))
                  - s.max(-1).values * F.LOG2E).abs().max()) < 1e-9 * max(1.0, float(lse2.abs().max()))


def test_cls_references_match_the_reference_head():
    R, H, C = 5, 130, 8
    pre, W2, b2, labels = G._cls_inputs(R, H, C, 3, CPU)
    keep = keep_mask(9, (R, H), 0.1, device=CPU)
    s32 = float(torch.tensor(1.0 / 0.9, dtype=torch.float32))
    for act, fn in ((0, torch.tanh), (1, torch.relu)):
        t, lg = F.cls_forward64(pre.double(), W2.double(), b2.double(), act, keep.double(), s32)
        want = TF.linear(ref.dropout(fn(pre), 0.1, 9), W2, b2)
        assert float((lg - want.double()).abs().max()) < 1e-5
    assert float((F.ce_rows64(lg, labels).mean() - ref.cross_entropy(lg.float(), labels).double()).abs()) < 1e-6
    assert float((F.ce_rows32_host(lg.float(), labels).double() - F.ce_rows64(lg, labels)).abs().max()) < 1e-5
    lg_ = lg.clone().requires_grad_()
    (F.ce_rows64(lg_, labels).mean() * 0.7).backward()
    assert float((F.dlogits64(lg, labels, 0.7 / R)[0] - lg_.grad).abs().max()) < 1e-14
    assert float((F.dlogits32_host(lg.float(), labels, torch.tensor([0.7]), R).double() - lg_.grad).abs().max()) < 1e-6


# ------------------------------------------------------------------------------------------------ the emulation
def _opt(t):
    return None if t is None else t


class Emu:
    """Every `_C` binding the GPU file calls, in plain fp32 torch on the CPU. `wrong` names one deliberate error."""

    def __init__(self, wrong=None):
        self.wrong = wrong

    # splits
    def split3(self, x, out, pat, rows):
        if self.wrong == "bit_order":
            pat = ((pat & 1) << 2) | (pat & 2) | ((pat >> 2) & 1)
        out.copy_(F.split3_ref(x, pat, rows))

    def split3_dual(self, x, oc, pc, orr, pr):
        self.split3(x, oc, pc, False)
        self.split3(x, orr, pr, True)

    def split2(self, x, hi, lo):
        h, l = F.split_halves(x)
        hi.copy_(h)
        lo.copy_(l)

    def _put_halves(self, v, hi, lo):
        if hi is not None:
            h, l = F.split_halves(v)
            hi.copy_(h.view(hi.shape))
            lo.copy_(l.view(lo.shape))

    # element passes
    def _rows_wrong(self, shape, p, seed):
        """The keep mask a missing `++row` at the column wrap would draw: exact for the first trip of the grid."""
        keep = keep_mask(seed, shape, p, device=CPU)
        W = shape[-1]
        rows = keep.numel() // W
        W4, groups, stride = F.ew4_geometry(rows, W)
        if self.wrong != "row_wrap" or groups <= stride:
            return keep
        i = torch.arange(groups)
        t0 = i % stride
        r0, c0 = t0 // W4, t0 % W4
        trips = i // stride
        c = c0 + trips * (stride % W4)
        r = r0 + trips * (stride // W4)  # the wraps' row increments left out
        c = c % W4
        big = keep_mask(seed, (rows, W), p, device=CPU).view(rows, W4, 4)
        return big[r.clamp_max(rows - 1), c].reshape(shape)

    def epi32(self, y, bias, aux, out, kind, p, seed, hi=None, lo=None):
        v = y if bias is None else y + bias
        if kind == 0:
            o = v.clone()
        elif kind == 1:
            y.copy_(v)
            o = ref.gelu(v)
        elif kind == 2:
            if p > 0:
                v = v * (self._rows_wrong(tuple(y.shape), p, seed).float() * (1.0 / (1.0 - p)))
            o = v + aux
        elif kind == 3:
            o = v + aux
        else:
            x = aux.clone().requires_grad_()
            ref.gelu(x).backward(v)
            o = x.grad
        if out is not None:
            out.copy_(o)
        self._put_halves(o, hi, lo)

    def dropout32(self, x, out, p, seed, hi=None, lo=None):
        o = ref.dropout(x.clone(), p, seed)
        out.copy_(o)
        self._put_halves(o, hi, lo)

    def colsum32(self, x, d):
        d += x.sum(0)

    # LayerNorm
    def ln32_fwd(self, x, g, b, out, mean, rstd, eps, hi=None, lo=None):
        mu = x.mean(1)
        if self.wrong == "one_pass":
            var = (x * x).mean(1) - mu * mu
        else:
            var = ((x - mu[:, None]) ** 2).mean(1)
        rs = (var + eps).rsqrt()
        o = (x - mu[:, None]) * rs[:, None] * g + b
        out.copy_(o)
        mean.copy_(mu)
        rstd.copy_(rs)
        self._put_halves(o, hi, lo)

    def ln32_bwd(self, dy, x, mean, rstd, g, dx, dg, db):
        # the given statistics, as the kernel takes them (the formula is pinned against autograd above)
        xh = (x - mean[:, None]) * rstd[:, None]
        dyg = dy * g
        s1, s2 = dyg.mean(1, keepdim=True), (dyg * xh).mean(1, keepdim=True)
        dg += (dy * xh).sum(0)
        db += dy.sum(0)
        dx.copy_(rstd[:, None] * (dyg - s1 - xh * s2))

    # embeddings
    def embed32_gather(self, ids, pids, tids, word, pos, typ, x):
        v = word[ids] + pos[pids]
        if typ is not None:
            v = v + (typ[tids] if tids is not None else typ[0])
        x.copy_(v)

    def embed32_scatter(self, dx, ids, pids, tids, gword, gpos, gtype):
        gword.index_add_(0, ids, dx)
        if gpos is not None:
            gpos.index_add_(0, pids, dx)
        if gtype is not None:
            gtype.index_add_(0, tids if tids is not None else torch.zeros_like(ids), dx)

    # classification head
    def cls32_fwd(self, pre, W2, b2, labels, t_out, logits, stats, act, p, seed):
        t = ref.dropout(torch.tanh(pre) if act == 0 else torch.relu(pre), p, seed)
        lg = TF.linear(t, W2, b2)
        t_out.copy_(t)
        logits.copy_(lg)
        stats[0] += TF.cross_entropy(lg, labels, reduction="sum")
        if self.wrong == "last_max":
            am = lg.shape[1] - 1 - lg.flip(1).argmax(1)
        else:
            am = lg.argmax(1)
        stats[1] += (am == labels).sum()

    def cls32_bwd(self, pre, t, W2, logits, labels, dloss, dpre, dW2, db2, act, p, seed):
        lg = logits.clone().requires_grad_()
        (TF.cross_entropy(lg, labels) * dloss[0]).backward()
        dl = lg.grad
        db2 += dl.sum(0)
        dW2 += dl.t() @ t
        x = pre.clone().requires_grad_()
        a = torch.tanh(x) if act == 0 else torch.relu(x)
        ref.dropout(a, p, seed).backward(dl @ W2)
        dpre.copy_(x.grad)

    # attention
    def _attn(self, qkv, mask, B, S, heads, p, seed):
        if mask is not None and self.wrong == "no_log2e":
            # the scores live in the log2 domain: a bias that misses its log2(e) factor is mask / log2(e) in the natural
            # one (the clamp at -1e30 hides that for the -inf-like masks)
            mask = torch.where(mask < -1e30, mask, mask / F.LOG2E)
        return ref.attention(qkv, mask, B, S, heads, p, seed, True)

    def attn32_fwd(self, qkv, mask, out, lse, B, S, heads, p, seed):
        out.copy_(self._attn(qkv, mask, B, S, heads, p, seed))
        x = qkv.view(B, S, 3, heads, 64).permute(2, 0, 3, 1, 4)
        s = torch.matmul(x[0], x[1].transpose(-1, -2)) * 0.125
        if mask is not None:
            s = s + mask.view(B, 1, 1, S)
        l = torch.logsumexp(s, -1) * F.LOG2E
        lse.copy_(torch.where(l < -1e30, torch.full_like(l, -1e30), l).reshape(-1))

    def attn32_bwd(self, qkv, mask, o, dout, lse, dqkv, delta, B, S, heads, p, seed):
        q = qkv.clone().requires_grad_()
        self._attn(q, mask, B, S, heads, p, seed).backward(dout)
        dqkv.copy_(q.grad)
        delta.copy_((o * dout).view(B, S, heads, 64).sum(-1).permute(0, 2, 1).reshape(-1))


EMU = Emu()


# ------------------------------------------------------------------------------------------------ the GPU checks on it
@pytest.mark.parametrize("C", [40, 12])
def test_emulated_split_patterns(C):
    G.test_split3_every_pattern_bit_exact(EMU, CPU, C)
    with pytest.raises(AssertionError):
        G.test_split3_every_pattern_bit_exact(Emu("bit_order"), CPU, C)


def test_emulated_small_splits_and_split2():
    for R, C, why in F.SPLIT_SMALL:
        G.test_split3_small_shapes(EMU, CPU, R, C, why)
    for n in (4, 1200):
        G.test_split2_bit_exact_with_tail_past_the_block_cap(EMU, CPU, n)


@pytest.mark.parametrize("M,N", F.EPI_SHAPES)
def test_emulated_epilogues(M, N):
    G.test_epi32_bias_residual_kinds_bit_exact(EMU, CPU, M, N)
    G.test_epi32_dropout_residual_matches_keep_mask(EMU, CPU, M, N)


def test_emulated_gelu_epilogues():
    G.test_epi32_gelu_forward_against_fp64(EMU, CPU)
    G.test_epi32_gelu_backward_against_fp64(EMU, CPU)


def test_emulated_second_trip_of_the_epilogue_sees_a_missing_row_wrap():
    G.test_epi32_second_grid_stride_trip(EMU, CPU)
    with pytest.raises(AssertionError):
        G.test_epi32_second_grid_stride_trip(Emu("row_wrap"), CPU)


@pytest.mark.parametrize("shape", F.DROPOUT_SHAPES)
def test_emulated_dropout(shape):
    G.test_dropout32_equals_reference_bit_for_bit(EMU, CPU, shape)


def test_emulated_colsum():
    for N in F.COLSUM_VECTOR_N:
        for M in F.COLSUM_VECTOR_M + F.COLSUM_LONG_M:
            G.test_colsum32_vector_path(EMU, CPU, M, N)
    for N in F.COLSUM_SCALAR_N:
        for M in F.COLSUM_SCALAR_M:
            G.test_colsum32_scalar_path(EMU, CPU, M, N)


@pytest.mark.parametrize("H", F.LN_H)
def test_emulated_layernorm(H):
    G.test_ln32_fwd_widths_and_offset_rows(EMU, CPU, H)
    G.test_ln32_bwd_widths(EMU, CPU, H)
    with pytest.raises(AssertionError):
        G.test_ln32_fwd_widths_and_offset_rows(Emu("one_pass"), CPU, H)


def test_emulated_layernorm_constant_and_long():
    for H in (4, 260, 1024):
        G.test_ln32_fwd_constant_rows(EMU, CPU, H)
    for R, H in F.LN_BWD_LONG:
        G.test_ln32_bwd_several_rows_per_wave(EMU, CPU, R, H)


def test_emulated_embeddings():
    for H in F.GATHER_H:
        for R in F.EMBED_R:
            G.test_embed32_gather_bit_exact(EMU, CPU, H, R)
    for H in F.SCATTER_H:
        G.test_embed32_scatter_into_nonzero_gradients(EMU, CPU, H)


@pytest.mark.parametrize("C", F.CLS_C)
def test_emulated_cls_head(C):
    for H in F.CLS_H:
        G.test_cls32_head_forward_and_backward(EMU, CPU, C, H)


def test_emulated_cls_tie_goes_to_the_first_index():
    for C, a, b in ((2, 0, 1), (8, 2, 5)):
        G.test_cls32_first_of_two_equal_maxima_wins(EMU, CPU, C, a, b)
        with pytest.raises(AssertionError):
            G.test_cls32_first_of_two_equal_maxima_wins(Emu("last_max"), CPU, C, a, b)


@pytest.mark.parametrize("mask_kind", F.ATTN_MASKS)
@pytest.mark.parametrize("S", F.ATTN_S)
def test_emulated_attention(S, mask_kind):
    for p in (0.0, 0.1):
        G.test_attn32_vector_kernels_against_fp64(EMU, CPU, S, mask_kind, p)
    if mask_kind == "soft":
        with pytest.raises(AssertionError):
            G.test_attn32_vector_kernels_against_fp64(Emu("no_log2e"), CPU, S, mask_kind, 0.0)
