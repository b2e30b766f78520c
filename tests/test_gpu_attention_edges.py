"""Attention kernels at the lengths, masks and shapes the rest of the suite does not reach, vs ops/reference.py on the
fp32 copy of the same inputs (same seed: the dropout bits match).

* lengths: every dispatch branch of launch_attn_fwd / launch_attn_bwd -- the tiled generic kernel natively with partial
  key tiles and query blocks (S = 64, 80), its S > 128 path (fp32 dQ atomics + conversion pass; S = 200, 320) and
  beyond the streaming maximum (S = 1152), attention128 (S = 128), the streaming kernels up to their advertised
  maximum (S = 256, 640, 1024); the fp32 pair likewise;
* masks: a fully masked sequence, a left-padded one (a whole first key tile masked), holes, and finite additive biases
  (which a wrong log2(e) factor on the mask term moves far outside the tolerances);
* shape: B = 4 sequences x 3 heads, so a swapped batch / head decomposition cannot pass;
* the fused QKV bias gradient of attn_bwd against the column sums of the reference's dqkv, into a non-zero destination;
* hip.key_mask_bias bit for bit; attn_block at a ragged and at an odd length.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from huggingface_sagemaker_tensorflow_distributed_amd.ops import reference as ref  # noqa: E402

B, HEADS = 4, 3
H = HEADS * 64
SEED = 777


def _hip():
    from huggingface_sagemaker_tensorflow_distributed_amd.ops import hip

    return hip


def _h32():
    from huggingface_sagemaker_tensorflow_distributed_amd.ops import hip32

    return hip32


def _close(a, b, atol, rtol, what=""):
    """At most 0.1 % of the elements beyond tolerance (bf16 rounding flips), and NONE beyond 4x the tolerance.
    (tests/test_gpu_ops.py, verbatim)"""
    a = a.float()
    b = b.float()
    err = (a - b).abs()
    # atol is relative to the tensor's scale (bf16 outputs of long reductions), rtol per element
    tol = atol * b.abs().max().clamp_min(1e-6) + rtol * b.abs()
    bad = (err > tol).float().mean().item()
    worst = (err / tol).max().item()
    assert bad <= 1e-3, f"{what}: {bad*100:.3f}% elements out of tol, max err {err.max().item():.4g}"
    assert worst <= 4.0, f"{what}: an element is {worst:.2f}x beyond tolerance (max err {err.max().item():.4g})"


def _rel(a, b):
    """(tests/test_gpu_fp32.py, verbatim)"""
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _pad_len(S):
    return 32 if S <= 64 else (64 if S < 256 else 128)


def _edge_mask(S, device, rows=(0, 1, 2, 3)):
    """[len(rows), S] 0/1: row 0 all keys masked, row 1 left-padded by a whole first key tile, row 2 holes (keys 10..19
    and the last 7), row 3 nothing masked."""
    am = torch.ones(4, S, dtype=torch.long, device=device)
    am[0] = 0
    am[1, :_pad_len(S)] = 0
    am[2, 10:20] = 0
    am[2, S - 7:] = 0
    return am[list(rows)].contiguous()


def _bias(kind, S, device):
    """(0/1 mask or None, additive key bias [B, S] fp32)."""
    if kind == "edge":
        am = _edge_mask(S, device)
        return am, ref.key_mask_bias(am)
    g = torch.Generator(device="cpu").manual_seed(1000 + S)
    return None, (-6 * torch.rand(B, S, generator=g)).to(device)


_CASES = {}


def _case(S, p, kind, device, bf16=True):
    """Inputs and the fp32 reference's output / dqkv of one case (never modified). The cases more than one test uses
    (S <= 256) are computed once and kept."""
    key = (S, p, kind, bf16)
    c = _CASES.get(key)
    if c is None:
        g = torch.Generator(device="cpu").manual_seed(3 + S)
        qkv = torch.randn(B * S, 3 * H, generator=g).to(device)
        dout = torch.randn(B * S, H, generator=g).to(device)
        if bf16:
            qkv, dout = qkv.bfloat16(), dout.bfloat16()
        am, mb = _bias(kind, S, device)
        q32 = qkv.detach().float().requires_grad_()
        r = ref.attention(q32, mb, B, S, HEADS, p, SEED, p > 0)
        r.backward(dout.float())
        c = dict(qkv=qkv, dout=dout, am=am, mb=mb, out=r.detach(), dqkv=q32.grad.detach())
        if S <= 256:
            _CASES[key] = c
    return c


def _assert_masked_keys_get_no_gradient(dqkv, am, S):
    """dK and dV rows of the masked keys of the left-padded and the holes sequences: exactly zero (the reference's
    are: their probabilities underflow to 0)."""
    g = dqkv.view(B, S, 3, H)
    for b in (1, 2):
        rows = g[b][am[b] == 0]
        assert rows.shape[0] > 0
        assert torch.count_nonzero(rows[:, 1:]) == 0, f"sequence {b}: a masked key has a dK / dV"


@pytest.mark.parametrize("kind", ["edge", "soft"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("S", [64, 80, 128, 200, 256, 320, 640, 1024, 1152])
def test_attention_edge_lengths_and_masks(gpu, S, p, kind):
    hip = _hip()
    c = _case(S, p, kind, gpu)
    x = c["qkv"].clone().requires_grad_()
    out = hip.attention(x, c["mb"], B, S, HEADS, p, SEED)
    out.backward(c["dout"])
    g = x.grad
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(g).all())
    _close(out, c["out"], 2e-2, 2e-2, "fwd")
    for i, name in enumerate("qkv"):
        _close(g[:, i * H:(i + 1) * H], c["dqkv"][:, i * H:(i + 1) * H], 3e-2, 3e-2, f"d{name}")
    if kind == "edge":
        _assert_masked_keys_get_no_gradient(g, c["am"], S)


@pytest.mark.parametrize("kind", ["edge", "soft"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("path,S", [("mfma", 128), ("mfma", 256), ("mfma", 1024), ("valu", 80), ("valu", 128),
                                    ("valu", 200)])
def test_attention32_edge_lengths_and_masks(gpu, path, S, p, kind, monkeypatch):
    """The fp32 pair: the split-product MFMA kernels (attention32m.hip) and the vector kernels (fp32.hip), at the
    bounds of test_attention32_fwd_bwd."""
    h32 = _h32()
    monkeypatch.setattr(h32, "_ATTN32M", path == "mfma")
    assert bool(h32._C.attn32m_supported(S)) or path == "valu"
    c = _case(S, p, kind, gpu, bf16=False)
    x = c["qkv"].clone().requires_grad_()
    out = h32.attention(x, c["mb"], B, S, HEADS, p, SEED)
    out.backward(c["dout"])
    g = x.grad
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(g).all())
    assert _rel(out.detach(), c["out"]) < 2e-5
    assert _rel(g, c["dqkv"]) < 2e-4
    if kind == "edge":
        _assert_masked_keys_get_no_gradient(g, c["am"], S)


@pytest.mark.parametrize("S,use_km", [(80, False), (128, False), (200, False), (256, False), (256, True)])
def test_attention_backward_bias_gradient_matches_column_sums(gpu, S, use_km):
    """attn_bwd's dbias: the column sums of dqkv ADDED to what the destination held (the generic kernel's colsum pass,
    attention128's and the streaming kernels' fused partial sums), vs the column sums of the reference's dqkv; and
    asking for it changes nothing in dqkv."""
    hip = _hip()
    C_ = hip._C
    p = 0.1
    c = _case(S, p, "edge", gpu)
    qkv, dout = c["qkv"], c["dout"]
    mb = c["mb"].float().contiguous()
    prefill = torch.randn(3 * H, generator=torch.Generator(device="cpu").manual_seed(5)).to(gpu)
    res = []
    for with_dbias in (True, False):
        out = torch.empty(B * S, H, device=gpu, dtype=torch.bfloat16)
        lse = torch.empty(B * HEADS * S, device=gpu)
        km = hip._keep_mask(B, S, HEADS, p, gpu) if use_km else None
        assert (km is not None) == use_km
        C_.attn_fwd(qkv, mb, out, lse, B, S, HEADS, p, SEED, km)
        dqkv = torch.empty_like(qkv)
        db = prefill.clone() if with_dbias else None
        C_.attn_bwd(qkv, mb, out, dout, lse, dqkv, hip._attn_ws(B, S, HEADS, gpu), B, S, HEADS, p, SEED, db, km)
        torch.cuda.synchronize()
        res.append((dqkv, db))
    (g1, db), (g0, _) = res
    _close(db - prefill, c["dqkv"].sum(0), 3e-2, 3e-2, "dbias")
    assert torch.equal(g1[:, H:], g0[:, H:])
    if S <= 128 or bool(C_.attn_keep_mask_supported(S)):
        # dQ written once per element (one workgroup per head, or the streaming dQ pass): no fp32 atomics feed it
        assert torch.equal(g1[:, :H], g0[:, :H])


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("shape", [(1, 1), (4, 80), (1, 2048 * 256 + 3)])
def test_key_mask_bias_kernel_is_bit_exact(gpu, shape, dtype):
    """mask_bias_kernel == ops/reference.py key_mask_bias bit for bit (the sign of zero included); the last shape is
    past the 2048-block grid cap (the grid-stride trip)."""
    hip = _hip()
    g = torch.Generator(device="cpu").manual_seed(shape[1])
    am = torch.randint(0, 2, shape, generator=g).to(dtype).to(gpu)
    got, want = hip.key_mask_bias(am), ref.key_mask_bias(am)
    assert got.dtype == want.dtype == torch.float32 and got.shape == want.shape
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("S", [80, 77])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attn_block_at_ragged_and_odd_lengths(gpu, p, S):
    """hip.attn_block vs the composed fp32 reference ops (as test_fused_blocks_vs_reference composes it) at a length
    that is no multiple of a tile (the generic attention kernel with its colsum bias gradient) and at an odd one (the
    reference attention between the HIP linear layers: the kernels' dropout column pairs need an even S)."""
    hip = _hip()
    torch.manual_seed(5)
    Hb, heads, Bb = 256, 4, 2
    T = Bb * S
    mk = lambda *s, sc=0.05: (torch.randn(*s, device=gpu) * sc).bfloat16().requires_grad_()  # noqa: E731
    h = torch.randn(T, Hb, device=gpu).bfloat16().requires_grad_()
    qw, qb, ow, ob = mk(3 * Hb, Hb), mk(3 * Hb), mk(Hb, Hb), mk(Hb)
    lw, lb = (1 + 0.1 * torch.randn(Hb, device=gpu)).bfloat16().requires_grad_(), mk(Hb)
    mb = ref.key_mask_bias(_edge_mask(S, gpu, rows=(1, 2)))
    params = [h, qw, qb, ow, ob, lw, lb]

    def run(hip_path):
        for t in params:
            t.grad = None
        if hip_path:
            out = hip.attn_block(h, qw, qb, ow, ob, lw, lb, 1e-12, mb, Bb, S, heads, p, 11, p, 12)
            used = params
        else:
            f = [t.detach().float().requires_grad_() for t in params]
            qkv = ref.linear(f[0], f[1], f[2])
            ctx_ = ref.attention(qkv, mb, Bb, S, heads, p, 11, p > 0)
            out = ref.layer_norm(ref.linear_dropout_residual(ctx_, f[3], f[4], f[0], p, 12, p > 0), f[5], f[6], 1e-12)
            used = f
        g = torch.randn(out.shape, device=gpu, generator=torch.Generator(device=gpu).manual_seed(9))
        out.backward(g.to(out.dtype))
        return out.float(), [t.grad.float() for t in used]

    o1, g1 = run(True)
    o2, g2 = run(False)
    assert bool(torch.isfinite(o1).all())
    # the op dispatch (what the model calls) takes the same route: the same kernels, bit for bit
    from huggingface_sagemaker_tensorflow_distributed_amd import ops

    with torch.no_grad():
        o3 = ops.attn_block(h, qw, qb, ow, ob, lw, lb, 1e-12, mb, Bb, S, heads, p, 11, p, 12)
    assert torch.equal(o3.float(), o1)
    _close(o1, o2, 3e-2, 3e-2, "out")
    for n, a, b in zip(["h", "qw", "qb", "ow", "ob", "lw", "lb"], g1, g2):
        rel = (a - b).norm() / (b.norm() + 1e-6)
        assert rel < 4e-2, f"{n}: rel err {rel:.3g}"
