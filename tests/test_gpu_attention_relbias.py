"""Relative-position-bias attention kernels (csrc/kernels/attention_relbias.hip), padded and packed, vs
ops/reference.py attention_relbias[_varlen] on fp32 copies of the same bf16 inputs (fp64 for drel; same seed: the
dropout bits match). Two distinct heads, B = 2, rel ~ N(0, 1) so the bias weighs as much as the scores. Bounds for out /
dq / dk / dv: the project's for kernels of this structure (tests/test_gpu_attention_d32.py). drel has no project number:
its bound is twice the max error of the reference op run in bf16 arithmetic on the same inputs, per case (the kernel
accumulates in fp32). rel has R = 2 S + 1 columns: the first and the last are out of every sequence's reach."""
import numpy as np
import pytest
import torch

from huggingface_sagemaker_tensorflow_distributed_amd import ops
from huggingface_sagemaker_tensorflow_distributed_amd.data.packing import pack_batch, position_rule
from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model, resolve_config
from huggingface_sagemaker_tensorflow_distributed_amd.ops import reference as ref

HEADS = 2
H = HEADS * 64
SEED = 777
BATCHES = {"A": [1, 64, 65, 130], "B": [3, 257]}
TABLE = "encoder.embeddings.relative_attention_table"


def _hip():
    from huggingface_sagemaker_tensorflow_distributed_amd.ops import hip

    return hip


def _close(a, b, atol, rtol, what=""):
    """At most 0.1 % of the elements beyond tolerance (bf16 rounding flips), and NONE beyond 4x the tolerance.
    (tests/test_gpu_attention_d32.py, verbatim)"""
    a = a.float()
    b = b.float()
    err = (a - b).abs()
    tol = atol * b.abs().max().clamp_min(1e-6) + rtol * b.abs()
    bad = (err > tol).float().mean().item()
    worst = (err / tol).max().item()
    assert bad <= 1e-3, f"{what}: {bad*100:.3f}% elements out of tol, max err {err.max().item():.4g}"
    assert worst <= 4.0, f"{what}: an element is {worst:.2f}x beyond tolerance (max err {err.max().item():.4g})"


def _drel_rule(drel, want64, yard, what):
    """|drel - fp64 oracle| <= 2 x |yardstick - fp64 oracle| (max over the entries); prints the measured pair."""
    err, bound = (drel.double() - want64).abs().max().item(), (yard.double() - want64).abs().max().item()
    print(f"drel {what}: kernel max err {err:.3e}, bf16-arithmetic reference max err {bound:.3e}, "
          f"max |drel| {want64.abs().max().item():.3e}")
    assert want64.abs().max() > 0 and err <= 2.0 * bound, f"{what}: drel max err {err:.3e} > 2 x {bound:.3e}"


def _reference(c, dtype, compute_dtype=None):
    q = c["qkv"].detach().to(dtype).requires_grad_()
    rel = c["rel"].detach().to(dtype).requires_grad_()
    p = c["p"]
    if c["cu"] is not None:
        r = ref.attention_relbias_varlen(q, rel, c["cu"], c["S"], HEADS, p, SEED, p > 0, compute_dtype)
    else:
        r = ref.attention_relbias(q, rel, c["mb"], c["B"], c["S"], HEADS, p, SEED, p > 0, compute_dtype)
    r.backward(c["dout"].to(dtype))
    return r.detach(), q.grad.detach(), rel.grad.detach()


_CASES = {}


def _case(key, device):
    """Inputs and the references' results of one case (computed once, never modified). key = ("packed", name, p) or
    ("padded", S, masked, p) with B = 2; the mask cuts sequence 1 one key into the last 64-key tile."""
    c = _CASES.get(key)
    if c is not None:
        return c
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
    c.update(qkv=torch.randn(T, 3 * H, generator=g).to(device).bfloat16(),
             dout=torch.randn(T, H, generator=g).to(device).bfloat16(),
             rel=torch.randn(HEADS, 2 * S + 1, generator=g).to(device), B=B, S=S, T=T, p=key[-1])
    c["out"], c["dqkv"], _ = _reference(c, torch.float32)
    c["drel64"] = _reference(c, torch.float64)[2]
    c["drel_bf16"] = _reference(c, torch.bfloat16, torch.bfloat16)[2]
    _CASES[key] = c
    return c


def _fwd_bwd(c, rel=None):
    qkv = c["qkv"].detach().clone().requires_grad_()
    rel = (c["rel"] if rel is None else rel).detach().clone().requires_grad_()
    if c["cu"] is not None:
        out = ops.attention_relbias_varlen(qkv, rel, c["cu"], c["S"], HEADS, c["p"], SEED)
    else:
        out = ops.attention_relbias(qkv, rel, c["mb"], c["B"], c["S"], HEADS, c["p"], SEED)
    out.backward(c["dout"])
    torch.cuda.synchronize()
    return out.detach(), qkv.grad.detach(), rel.grad.detach()


def _check(c, what):
    assert _hip().attention_relbias_ok(c["qkv"], c["rel"], c["S"], HEADS, c["cu"] is None)  # the kernels, not the reference
    out, dqkv, drel = _fwd_bwd(c)
    assert torch.isfinite(out.float()).all() and torch.isfinite(dqkv.float()).all()
    _close(out, c["out"], 2e-2, 2e-2, f"{what} out")
    for i, part in enumerate(("dq", "dk", "dv")):
        _close(dqkv[:, i * H:(i + 1) * H], c["dqkv"][:, i * H:(i + 1) * H], 3e-2, 3e-2, f"{what} {part}")
    _drel_rule(drel, c["drel64"], c["drel_bf16"], what)
    assert torch.count_nonzero(drel[:, [0, -1]]) == 0, "an entry of rel that no sequence reaches has a gradient"
    assert torch.count_nonzero(out[c["t_real"]:]) == 0 and torch.count_nonzero(dqkv[c["t_real"]:]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("S", [2, 66, 128, 130, 320])
def test_padded_relbias_attention_matches_reference(gpu, S, masked, p):
    _check(_case(("padded", S, masked, p), gpu), f"S={S} masked={masked} p={p}")


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("name", ["A", "B"])
def test_packed_relbias_attention_matches_reference_and_zeroes_dead_rows(gpu, name, p):
    c = _case(("packed", name, p), gpu)
    assert c["t_real"] < c["T"]
    _check(c, f"packed {name} p={p}")


@pytest.mark.gpu
def test_relbias_forward_and_backward_are_bit_identical_run_to_run(gpu):
    c = _case(("packed", "A", 0.1), gpu)
    assert all(torch.equal(a, b) for a, b in zip(_fwd_bwd(c), _fwd_bwd(c)))


@pytest.mark.gpu
@pytest.mark.parametrize("B,S", [(3, 130)])
def test_padded_form_equals_packed_form_bit_for_bit(gpu, B, S):
    """drel included: both forms index the partial-row slab by (sequence, head, block) and reduce it in one order."""
    g = torch.Generator(device="cpu").manual_seed(3)
    c = dict(qkv=torch.randn(B * S, 3 * H, generator=g).to(gpu).bfloat16(),
             dout=torch.randn(B * S, H, generator=g).to(gpu).bfloat16(),
             rel=torch.randn(HEADS, 2 * S - 1, generator=g).to(gpu), mb=None, B=B, S=S, p=0.0)
    padded = _fwd_bwd(dict(c, cu=None))
    packed = _fwd_bwd(dict(c, cu=torch.arange(B + 1, dtype=torch.int32, device=gpu) * S))
    assert all(torch.equal(a, b) for a, b in zip(padded, packed))
    assert padded[1].float().abs().sum() > 0 and padded[2].abs().sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("key", [("padded", 130, True, 0.0), ("packed", "A", 0.0)])
def test_zero_bias_equals_the_plain_attention_kernels(gpu, key):
    c = _case(key, gpu)
    out = _fwd_bwd(c, torch.zeros_like(c["rel"]))[0]
    if c["cu"] is not None:
        want = ops.attention_varlen(c["qkv"], c["cu"], c["S"], HEADS, 0.0, SEED)
    else:
        want = ops.attention(c["qkv"], c["mb"], c["B"], c["S"], HEADS, 0.0, SEED)
    _close(out, want, 2e-2, 2e-2, "rel = 0")


# ------------------------------------------------------------------------------------------ the model on the kernels
@pytest.mark.gpu
@pytest.mark.parametrize("packed", [False, True])
def test_mpnet_training_step_hip_vs_fp32_cpu_model(gpu, packed):
    """One bf16 step of hsd-tiny-mpnet widened to d = 64 (the kernels run) with dropout vs the fp32 CPU model on the same
    (bf16-rounded) weights: the loss / logits / gradient bounds of tests/test_gpu_varlen.py's model test, and the
    table's gradient within the drel rule, its yardstick the same bf16 model on the reference ops."""
    cfg = resolve_config("hsd-tiny-mpnet").replace(hidden_size=128, num_attention_heads=2, intermediate_size=256)
    cpu = build_model(cfg, seed=0).train()
    with torch.no_grad():
        cpu.encoder.embeddings.relative_attention_table.normal_(0.0, 1.0, generator=torch.Generator().manual_seed(1))
        for prm in cpu.parameters():
            prm.copy_(prm.bfloat16().float())
    dev = build_model(cfg, seed=0).to(gpu).bfloat16().train()
    dev.load_state_dict(cpu.state_dict())
    g = np.random.default_rng(0)
    mask = (np.arange(64)[None, :] < np.array([64, 40, 17, 2])[:, None]).astype(np.int64)
    ids = np.where(mask != 0, g.integers(5, cfg.vocab_size, size=(4, 64)), cfg.pad_token_id)
    labels = g.integers(0, 2, size=(4,))
    kw = dict(input_ids=ids, attention_mask=mask, labels=labels)
    if packed:
        pk = pack_batch(ids, mask, labels, **position_rule(cfg))
        kw = dict(input_ids=pk["input_ids"], labels=labels, cu_seqlens=pk["cu_seqlens"], position_ids=pk["position_ids"])

    def run(model, device, force_torch=False):
        old, ops._FORCE_TORCH = ops._FORCE_TORCH, force_torch
        try:
            model.zero_grad(set_to_none=True)
            model.rng.new_step(5)
            extra = dict(max_seqlen=pk["max_seqlen"]) if packed else {}
            loss, logits = model(**{k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in kw.items()},
                                 **extra)
            loss.backward()
            return loss.detach().float().cpu(), logits.detach().float().cpu(), \
                {n: p.grad.float().cpu() for n, p in model.named_parameters()}
        finally:
            ops._FORCE_TORCH = old

    (l0, lg0, g0), (l1, lg1, g1), (_, _, g2) = run(cpu, "cpu"), run(dev, gpu), run(dev, gpu, True)
    assert torch.isfinite(l1) and torch.allclose(l1, l0, atol=2e-2, rtol=2e-2), (l1, l0)
    assert torch.allclose(lg1, lg0, atol=5e-2, rtol=5e-2)
    for n in g0:
        rel = (g1[n] - g0[n]).norm() / (g0[n].norm() + 1e-6)
        assert rel < 5e-2, f"{n}: rel grad err {rel:.3g}"
    _drel_rule(g1[TABLE], g0[TABLE].double(), g2[TABLE], f"model table packed={packed}")
