"""Head-dim-32 attention kernels (csrc/kernels/attention_d32.hip), padded and packed, vs ops/reference.py on the fp32
copy of the same bf16 inputs (same seed: the dropout bits match). Four heads everywhere: two head pairs with both heads
of each pair distinct, so a swapped head, a swapped pair or a wrong row decomposition cannot pass. Bounds: the project's
for this op at d = 64 (tests/test_gpu_varlen.py) -- the same randn inputs, the same score distribution under the
1/sqrt(d) scale, a shorter QK^T reduction."""
import numpy as np
import pytest
import torch

from huggingface_sagemaker_tensorflow_distributed_amd.ops import reference as ref

HEADS = 4
H = HEADS * 32
SEED = 777
BATCHES = {"A": [1, 7, 32, 33, 64, 65, 127, 128, 129, 200, 320], "C": [(i % 5) + 1 for i in range(64)]}


def _hip():
    from huggingface_sagemaker_tensorflow_distributed_amd.ops import hip

    return hip


def _close(a, b, atol, rtol, what=""):
    """At most 0.1 % of the elements beyond tolerance (bf16 rounding flips), and NONE beyond 4x the tolerance.
    (tests/test_gpu_varlen.py, verbatim)"""
    a = a.float()
    b = b.float()
    err = (a - b).abs()
    # atol is relative to the tensor's scale (bf16 outputs of long reductions), rtol per element
    tol = atol * b.abs().max().clamp_min(1e-6) + rtol * b.abs()
    bad = (err > tol).float().mean().item()
    worst = (err / tol).max().item()
    assert bad <= 1e-3, f"{what}: {bad*100:.3f}% elements out of tol, max err {err.max().item():.4g}"
    assert worst <= 4.0, f"{what}: an element is {worst:.2f}x beyond tolerance (max err {err.max().item():.4g})"


def _assert_close4(out, dqkv, c, what):
    assert torch.isfinite(out.float()).all() and torch.isfinite(dqkv.float()).all()
    _close(out, c["out"], 2e-2, 2e-2, f"{what} out")
    for i, part in enumerate(("dq", "dk", "dv")):
        _close(dqkv[:, i * H:(i + 1) * H], c["dqkv"][:, i * H:(i + 1) * H], 3e-2, 3e-2, f"{what} {part}")


_CASES = {}


def _case(key, device):
    """Inputs and the fp32 reference's out / dqkv of one case (computed once, never modified). key = ("packed", name, p)
    or ("padded", S, masked, p) with B = 2; the mask cuts sequence 1 one key into the last 64-key tile (an odd length)."""
    c = _CASES.get(key)
    if c is not None:
        return c
    p = key[-1]
    if key[0] == "packed":
        lengths = BATCHES[key[1]]
        cu = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
        T, B, S = -(-int(cu[-1]) // 256) * 256, len(lengths), max(lengths)
        c = dict(cu=torch.from_numpy(cu).to(device), mb=None, t_real=int(cu[-1]))
    else:
        B, S = 2, key[1]
        T, mb = B * S, None
        if key[2]:
            am = torch.ones(B, S, dtype=torch.long)
            am[1, 64 * ((S - 1) // 64) + 1:] = 0
            mb = ref.key_mask_bias(am).to(device)
        c = dict(cu=None, mb=mb, t_real=T)
    g = torch.Generator(device="cpu").manual_seed(11 + T)
    qkv = torch.randn(T, 3 * H, generator=g).to(device).bfloat16()
    dout = torch.randn(T, H, generator=g).to(device).bfloat16()
    q32 = qkv.detach().float().requires_grad_()
    if c["cu"] is not None:
        r = ref.attention_varlen(q32, c["cu"], S, HEADS, p, SEED, p > 0)
    else:
        r = ref.attention(q32, mb, B, S, HEADS, p, SEED, p > 0)
    r.backward(dout.float())
    c.update(qkv=qkv, dout=dout, B=B, S=S, T=T, p=p, out=r.detach(), dqkv=q32.grad.detach())
    _CASES[key] = c
    return c


def _fwd_bwd(c):
    qkv = c["qkv"].detach().clone().requires_grad_()
    if c["cu"] is not None:
        out = _hip().attention_d32_varlen(qkv, c["cu"], c["S"], HEADS, c["p"], SEED)
    else:
        out = _hip().attention_d32(qkv, c["mb"], c["B"], c["S"], HEADS, c["p"], SEED)
    out.backward(c["dout"])
    torch.cuda.synchronize()
    return out.detach(), qkv.grad.detach()


# ------------------------------------------------------------------------------------------ 1 / 2. kernels vs reference
@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("S", [2, 34, 64, 66, 128, 130, 320])
def test_padded_d32_attention_matches_reference(gpu, S, masked, p):
    c = _case(("padded", S, masked, p), gpu)
    _assert_close4(*_fwd_bwd(c), c, f"S={S}")


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("name", ["A", "C"])
def test_packed_d32_attention_matches_reference(gpu, name, p):
    c = _case(("packed", name, p), gpu)
    _assert_close4(*_fwd_bwd(c), c, name)


# ------------------------------------------------------------------------------------------ 3. every row written
@pytest.mark.gpu
@pytest.mark.parametrize("key", [("packed", "A", 0.1), ("padded", 66, False, 0.1)])
def test_d32_kernels_write_every_row_and_zero_the_dead_rows(gpu, key):
    C_ = _hip()._C
    c = _case(key, gpu)
    T, B, S, t_real = c["T"], c["B"], c["S"], c["t_real"]
    nan = float("nan")
    out = torch.full((T, H), nan, device=gpu, dtype=torch.bfloat16)
    lse = torch.full((HEADS * T,), nan, device=gpu)
    dqkv = torch.full((T, 3 * H), nan, device=gpu, dtype=torch.bfloat16)
    C_.attn_d32_fwd(c["qkv"], c["cu"], None, out, lse, B, S, HEADS, c["p"], SEED)
    C_.attn_d32_bwd(c["qkv"], c["cu"], None, out, c["dout"], lse, dqkv, B, S, HEADS, c["p"], SEED)
    torch.cuda.synchronize()
    assert (t_real < T) == (key[0] == "packed")
    lse_rows = lse.view(HEADS, T).t() if key[0] == "packed" else lse.view(B, HEADS, S).permute(0, 2, 1).reshape(T, HEADS)
    for what, t in (("out", out), ("lse2", lse_rows), ("dqkv", dqkv)):
        assert not torch.isnan(t.float()).any(), f"{what}: a row was not written"
        assert torch.count_nonzero(t[t_real:]) == 0, f"{what}: a dead row is not zero"
    _assert_close4(out, dqkv, c, "direct")


# ------------------------------------------------------------------------------------------ 4. determinism
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A"])
def test_d32_forward_and_backward_are_bit_identical_run_to_run(gpu, name):
    c = _case(("packed", name, 0.1), gpu)
    out0, d0 = _fwd_bwd(c)
    out1, d1 = _fwd_bwd(c)
    assert torch.equal(out0, out1) and torch.equal(d0, d1)


# ------------------------------------------------------------------------------------------ 5. one kernel, two addressings
@pytest.mark.gpu
@pytest.mark.parametrize("B,S", [(3, 130)])
def test_padded_form_equals_packed_form_bit_for_bit(gpu, B, S):
    g = torch.Generator(device="cpu").manual_seed(3)
    qkv = torch.randn(B * S, 3 * H, generator=g).to(gpu).bfloat16()
    dout = torch.randn(B * S, H, generator=g).to(gpu).bfloat16()
    cu = torch.arange(B + 1, dtype=torch.int32, device=gpu) * S
    res = []
    for packed in (False, True):
        x = qkv.clone().requires_grad_()
        out = (_hip().attention_d32_varlen(x, cu, S, HEADS, 0.0, SEED) if packed
               else _hip().attention_d32(x, None, B, S, HEADS, 0.0, SEED))
        out.backward(dout)
        res.append((out.detach(), x.grad.detach()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert res[0][1].float().abs().sum() > 0


# ------------------------------------------------------------------------------------------ 6. what the explicit ops take
@pytest.mark.gpu
@pytest.mark.parametrize("d,heads,S,want", [(32, 4, 64, True), (32, 3, 64, False), (32, 4, 63, False),
                                            (64, 4, 64, False)])
def test_attention_d32_ok_and_the_unchanged_dispatch(gpu, d, heads, S, want):
    qkv = torch.empty(2 * S, 3 * heads * d, dtype=torch.bfloat16, device=gpu)
    assert _hip().attention_d32_ok(qkv, S, heads) is want
    assert _hip()._C.attn_d32_supported(heads, d, S) is want
    assert _hip().attention_ok(qkv, S, heads) is (d == 64)
    if not want:
        with pytest.raises(ValueError):
            _hip().attention_d32(qkv, None, 2, S, heads, 0.0, SEED)
