"""The properties of ops/reference.py attention that tests/test_gpu_attention_edges.py leans on, pinned on the CPU: an
edit to the reference cannot quietly hollow those GPU tests out.

* the edge-mask pattern (a fully masked sequence, a left-padded one, holes) gives finite outputs and gradients, exactly
  zero dK / dV for the masked keys of a partly masked sequence, and the uniform softmax for the fully masked one;
* an odd sequence length runs;
* a finite additive key bias matters: scaling it by log2(e) (the factor a kernel working in the log2 domain could drop
  or double) moves the output far beyond the kernel tests' tolerances.
"""
import math

import pytest
import torch

from huggingface_sagemaker_tensorflow_distributed_amd.ops import reference as ref

B, HEADS = 4, 3
H = HEADS * 64
SEED = 777


def _edge_mask(S):
    """The pattern of tests/test_gpu_attention_edges.py: row 0 all keys masked, row 1 left-padded, row 2 holes, row 3
    nothing masked."""
    am = torch.ones(B, S, dtype=torch.long)
    am[0] = 0
    am[1, :(32 if S <= 64 else (64 if S < 256 else 128))] = 0
    am[2, 10:20] = 0
    am[2, S - 7:] = 0
    return am


def _inputs(S):
    g = torch.Generator().manual_seed(3 + S)
    qkv = torch.randn(B * S, 3 * H, generator=g).bfloat16().float()
    dout = torch.randn(B * S, H, generator=g).bfloat16().float()
    return qkv, dout


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("S", [80, 128, 200])
def test_reference_attention_on_the_edge_mask(S, p):
    qkv, dout = _inputs(S)
    am = _edge_mask(S)
    x = qkv.clone().requires_grad_()
    out = ref.attention(x, ref.key_mask_bias(am), B, S, HEADS, p, SEED, p > 0)
    out.backward(dout)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(x.grad).all())
    g = x.grad.view(B, S, 3, H)
    for b in (1, 2):
        rows = g[b][am[b] == 0]
        assert rows.shape[0] > 0 and torch.count_nonzero(rows[:, 1:]) == 0
    # the fully masked sequence still takes gradients (the uniform softmax's), which the kernels must reproduce
    assert float(g[0].abs().max()) > 0
    if p == 0:
        v = qkv.view(B, S, 3, H)[0, :, 2]  # [S, H]: head h at columns h * 64
        want = v.mean(0, keepdim=True).expand(S, H)
        assert float((out.detach().view(B, S, H)[0] - want).abs().max()) <= 1e-6


def test_reference_attention_takes_an_odd_length():
    S = 77
    qkv, dout = _inputs(S)
    x = qkv.clone().requires_grad_()
    out = ref.attention(x, ref.key_mask_bias(_edge_mask(S)), B, S, HEADS, 0.1, SEED, True)
    out.backward(dout)
    assert out.shape == (B * S, H)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(x.grad).all())


@pytest.mark.parametrize("S", [80, 128, 200])
def test_soft_bias_scale_moves_the_reference_output(S):
    qkv, _ = _inputs(S)
    bias = -6 * torch.rand(B, S, generator=torch.Generator().manual_seed(1000 + S))
    a = ref.attention(qkv, bias, B, S, HEADS, 0.0, SEED, False)
    b = ref.attention(qkv, bias * math.log2(math.e), B, S, HEADS, 0.0, SEED, False)
    assert float((a - b).norm() / a.norm()) > 0.10
