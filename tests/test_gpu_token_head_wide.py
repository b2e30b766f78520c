"""The fused token-classification head for 17 .. 64 classes (csrc/kernels/token_head_wide.hip) against the fp32 torch
head on the same bf16 inputs (ref.dropout -> F.linear -> F.cross_entropy(ignore_index=-100, label_smoothing=eps)), at
the bounds of tests/test_gpu_token_head.py; the helpers are that file's."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from huggingface_sagemaker_tensorflow_distributed_amd import ops  # noqa: E402
from huggingface_sagemaker_tensorflow_distributed_amd.data.packing import pack_batch, position_rule  # noqa: E402
from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model, resolve_config  # noqa: E402
from huggingface_sagemaker_tensorflow_distributed_amd.ops import reference as ref  # noqa: E402

SEED = 0x5EED0123456789AB
TASK = "token-classification"


def _hip():
    from huggingface_sagemaker_tensorflow_distributed_amd.ops import hip

    return hip


def _close(a, b, atol, rtol, what=""):
    """tests/test_gpu_ops.py _close: at most 0.1 % of the elements beyond tolerance, none beyond 4x."""
    a = a.float()
    b = b.float()
    err = (a - b).abs()
    tol = atol * b.abs().max().clamp_min(1e-6) + rtol * b.abs()
    bad = (err > tol).float().mean().item()
    worst = (err / tol).max().item()
    assert bad <= 1e-3, f"{what}: {bad*100:.3f}% elements out of tol, max err {err.max().item():.4g}"
    assert worst <= 4.0, f"{what}: an element is {worst:.2f}x beyond tolerance (max err {err.max().item():.4g})"


def _inputs(gpu, R, H, C, seed=17, ignore=0.25):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(R, H, generator=g).to(gpu).bfloat16().requires_grad_()
    w = (torch.randn(C, H, generator=g) * 0.05).to(gpu).bfloat16().requires_grad_()
    b = (torch.randn(C, generator=g) * 0.5).to(gpu).bfloat16().requires_grad_()
    labels = torch.randint(0, C, (R,), generator=g)
    if R > 1:
        labels[torch.rand(R, generator=g) < ignore] = -100  # scattered
        labels[0] = 0  # at least one valid row
    return h, w, b, labels.to(gpu)


def _reference(h, w, b, labels, p, eps=0.0):
    f = [t.detach().float().requires_grad_() for t in (h, w, b)]
    lg = torch.nn.functional.linear(ref.dropout(f[0], p, SEED, True), f[1], f[2])
    loss = torch.nn.functional.cross_entropy(lg, labels, ignore_index=-100, label_smoothing=eps)
    loss.backward()
    return loss.detach(), lg.detach(), [t.grad for t in f]


def _raw_backward(h, w, logits, labels, stats, p, eps=0.0):
    """The backward launch itself on fresh buffers: dh pre-filled with NaN, dW / db from zero."""
    hip = _hip()
    (R, H), C = h.shape, w.shape[0]
    dh = torch.full((R, H), float("nan"), dtype=torch.bfloat16, device=h.device)
    dW = torch.zeros(C * H, dtype=torch.float32, device=h.device)
    db = torch.zeros(C, dtype=torch.float32, device=h.device)
    part = torch.empty(hip._C.token_head_wide_bwd_blocks(R, H) * (C * H + C), dtype=torch.float32, device=h.device)
    dl = torch.ones(1, dtype=torch.float32, device=h.device)
    hip._C.token_head_wide_bwd(h.detach(), w.detach(), logits, labels, stats, dl, dh, part, dW, db, float(p),
                               hip._s64(SEED), eps)
    return dh, dW.view(C, H), db


def _bounds(loss, logits, grads, h, w, b, labels, p, eps=0.0):
    """test_token_head_vs_reference's bounds: logits _close(3e-2, 3e-2), loss 2e-2·max(1, |ref|), gradients 4e-2."""
    loss_ref, lg_ref, g_ref = _reference(h, w, b, labels, p, eps)
    print(f"loss {loss.item():.5f} ref {loss_ref.item():.5f}")
    _close(logits, lg_ref, 3e-2, 3e-2, "logits")
    assert abs(loss.item() - loss_ref.item()) < 2e-2 * max(1.0, abs(loss_ref.item())), (loss.item(), loss_ref.item())
    for n, a, r_ in zip(["h", "w", "b"], grads, g_ref):
        rel = (a.float() - r_).norm() / (r_.norm() + 1e-6)
        print(f"  d{n}: rel err {rel:.3g}")
        assert rel < 4e-2, f"{n}: rel err {rel:.3g}"


def _check(gpu, R, H, C, p, eps):
    h, w, b, labels = _inputs(gpu, R, H, C)
    loss, logits = ops.token_head(h, w, b, labels, p, SEED, label_smoothing=eps)
    stats = getattr(loss, "_hsd_stats", None)
    assert stats is not None and logits.dtype == torch.bfloat16 and tuple(logits.shape) == (R, C)
    loss.backward()
    _bounds(loss, logits, (h.grad, w.grad, b.grad), h, w, b, labels, p, eps)
    valid = labels.ne(-100)
    assert stats[2].item() == valid.sum().item()
    lg_cpu, lab_cpu = logits.float().cpu(), labels.cpu()
    hits = int(((lg_cpu.argmax(-1) == lab_cpu) & lab_cpu.ne(-100)).sum())  # first maximum of the kernel's own logits
    assert stats[1].item() == hits
    assert abs(stats[0].item() * max(1.0, stats[2].item()) - stats[3].item()) <= 1e-5 * max(1.0, abs(stats[3].item()))
    # every element of dh is written (NaN pre-fill), ignored rows are exactly zero, and the launch on its own buffers
    # gives the bits autograd returned (a padding class that leaked into g, dW or db would break the last two)
    dh, dW, db = _raw_backward(h, w, logits, labels, stats, p, eps)
    assert not torch.isnan(dh.float()).any()
    assert torch.count_nonzero(dh[~valid]) == 0
    assert torch.equal(dh, h.grad) and torch.equal(dW.to(torch.bfloat16), w.grad) and torch.equal(db.bfloat16(), b.grad)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("C", [17, 32, 33, 45, 64])
@pytest.mark.parametrize("H", [64, 72, 328, 768, 1024])
@pytest.mark.parametrize("R", [1, 17, 255, 1000])
def test_wide_head_vs_reference(gpu, R, H, C, p):
    """One row, a partial tile, several blocks, a row count that is no multiple of 16; H under one slice per wave,
    with a ragged last slice (72), with a ragged second 256-column range (328), bert-base's and the limit; C at the
    first class of a second MFMA group, at group edges, one past an edge, PTB's 45 and the limit."""
    _check(gpu, R, H, C, p, 0.0)


@pytest.mark.parametrize("R,H,C,p", [(255, 768, 45, 0.1), (1000, 1024, 64, 0.0), (17, 72, 17, 0.1),
                                     (16405, 768, 33, 0.1), (40005, 328, 45, 0.1)])
def test_wide_head_smoothed(gpu, R, H, C, p):
    """eps = 0.1 (the kSmooth instantiations). The last two row counts are where the forward takes 8-wave (more than
    4·256 tiles) and 12-wave blocks (more than 8·256 tiles); everything smaller runs 4-wave blocks."""
    _check(gpu, R, H, C, p, 0.1)


@pytest.mark.parametrize("R,H,C", [(255, 768, 45), (16, 64, 17)])
def test_all_rows_ignored(gpu, R, H, C):
    h, w, b, labels = _inputs(gpu, R, H, C)
    labels = torch.full_like(labels, -100)
    loss, logits = ops.token_head(h, w, b, labels, 0.1, SEED)
    loss.backward()
    assert loss.item() == 0.0 and loss._hsd_stats[2].item() == 0.0 and loss._hsd_stats[1].item() == 0.0
    _close(logits, _reference(h, w, b, torch.zeros_like(labels), 0.1)[1], 3e-2, 3e-2, "logits")
    dh, dW, db = _raw_backward(h, w, logits, labels, loss._hsd_stats, 0.1)
    for t in (dh, dW, db, h.grad, w.grad, b.grad):
        assert torch.count_nonzero(t) == 0 and not torch.isnan(t.float()).any()


def test_two_runs_give_the_same_bits_and_add_into_main_grad(gpu):
    """H = 768 is 3 column ranges, so the persistent backward grid has 512 // 3 = 170 row blocks; 16·170·3 + 5 rows
    are 511 tiles: 3 tiles per block (4 in one) and 170 slabs through the reducer, twice. Then the same gradients into
    pre-filled main_grad buffers (+=), as test_backward_adds_into_main_grad does."""
    R, H, C = 16 * 170 * 3 + 5, 768, 45
    assert _hip()._C.token_head_wide_bwd_blocks(R, H) == 170 < (R + 15) // 16
    h, w, b, labels = _inputs(gpu, R, H, C)
    outs = []
    for _ in range(2):
        for t in (h, w, b):
            t.grad = None
        loss, logits = ops.token_head(h, w, b, labels, 0.1, SEED)
        loss.backward()
        outs.append((loss.detach().clone(), logits.clone(), h.grad.clone(), w.grad.clone(), b.grad.clone()))
    for a, c in zip(*outs):
        assert torch.equal(a, c)
    assert outs[0][2].float().abs().sum() > 0 and outs[0][3].float().abs().sum() > 0
    _, want_w, want_b = _raw_backward(h, w, logits, labels, loss._hsd_stats, 0.1)  # fp32, from zeroed buffers
    g = torch.Generator().manual_seed(3)
    pre_w = torch.randint(-4, 5, (C, H), generator=g).float().to(gpu)  # small integers: the sums below are exact
    pre_b = torch.randint(-4, 5, (C,), generator=g).float().to(gpu)
    w2, b2 = w.detach().clone().requires_grad_(), b.detach().clone().requires_grad_()
    w2.main_grad, b2.main_grad = pre_w.clone(), pre_b.clone()
    loss2, _ = ops.token_head(h.detach(), w2, b2, labels, 0.1, SEED)  # no input gradient asked for
    loss2.backward()
    assert w2.grad is None and b2.grad is None  # the gradient went into main_grad
    # (prefill + g) - prefill: one fp32 rounding at magnitude <= 8, i.e. at most 2^-21 = 4.8e-7 off g
    torch.testing.assert_close((w2.main_grad - pre_w), want_w, atol=1e-6, rtol=0)
    torch.testing.assert_close((b2.main_grad - pre_b), want_b, atol=1e-6, rtol=0)
    assert want_w.abs().max() > 1e-3 and not torch.equal(w2.main_grad, pre_w)


@pytest.mark.parametrize("C,H,fp32,fused,wide", [(17, 768, False, True, True), (64, 768, False, True, True),
                                                 (45, 768, False, True, True), (16, 768, False, True, False),
                                                 (65, 768, False, True, False), (45, 1032, False, True, False),
                                                 (45, 768, True, True, False), (45, 768, False, False, False)])
def test_dispatch(gpu, monkeypatch, C, H, fp32, fused, wide):
    """ops.token_head takes the wide kernels for 17 <= C <= 64 bf16 rows of H <= 1024, once and without the narrow
    entry; 16 classes, 65 classes, H = 1032, fp32 tensors and the composed knob never reach them."""
    hip = _hip()
    calls = {"wide": 0, "narrow": 0}
    real_w, real_n = hip.token_head_wide, hip.token_head
    monkeypatch.setattr(hip, "token_head_wide", lambda *a: (calls.update(wide=calls["wide"] + 1), real_w(*a))[1])
    monkeypatch.setattr(hip, "token_head", lambda *a: (calls.update(narrow=calls["narrow"] + 1), real_n(*a))[1])
    monkeypatch.setattr(ops, "TOKEN_HEAD_FUSED", fused)
    h, w, b, labels = _inputs(gpu, 64, H, C)
    if fp32:
        h, w, b = (t.detach().float().requires_grad_() for t in (h, w, b))
    assert hip.token_head_wide_ok(h, w) == (wide or not fused)
    loss, logits = ops.token_head(h, w, b, labels, 0.1, SEED)
    loss.backward()
    assert calls == {"wide": int(wide), "narrow": int(C == 16)}
    _bounds(loss, logits, (h.grad, w.grad, b.grad), h, w, b, labels, 0.1)


# ------------------------------------------------------------------------------------------ model step
def _model_step(model, kw, force_torch):
    old = ops._FORCE_TORCH
    ops._FORCE_TORCH = force_torch
    try:
        model.zero_grad(set_to_none=True)
        model.rng.new_step(5)
        loss, logits = model(**kw)
        loss.backward()
        return loss.detach().float(), logits.detach().float(), {n: p.grad.float().clone()
                                                                for n, p in model.named_parameters()}
    finally:
        ops._FORCE_TORCH = old


@pytest.mark.parametrize("packed", [False, True])
def test_model_step_37_labels_vs_fp32_reference_model(gpu, packed):
    """tests/test_gpu_token_head.py test_model_step_vs_fp32_reference_model (its shape, batch and bounds) with
    OntoNotes' 37 labels: the tiny bert's head runs the wide kernels, padded and packed."""
    L = 37
    cfg = resolve_config("hsd-tiny-bert", num_labels=L).replace(hidden_size=128, num_attention_heads=2,
                                                               intermediate_size=256)
    m32 = build_model(cfg, task=TASK, seed=0).to(gpu)
    m16 = copy.deepcopy(m32).bfloat16()
    with torch.no_grad():  # the reference holds the bf16-rounded weights
        for p32, p16 in zip(m32.parameters(), m16.parameters()):
            p32.copy_(p16.float())
    g = np.random.default_rng(0)
    B, S = 4, 128
    ids = g.integers(5, cfg.vocab_size, size=(B, S)).astype(np.int64)
    mask = (np.arange(S)[None, :] < np.array([S, S * 5 // 8, S // 4 + 1, 2])[:, None]).astype(np.int64)
    ids[mask == 0] = cfg.pad_token_id
    labels = g.integers(0, L, size=(B, S)).astype(np.int64)
    labels[g.random((B, S)) < 0.25] = -100
    labels[:, 0] = -100
    labels[mask == 0] = -100
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    if packed:
        pk = pack_batch(ids, mask, labels, **position_rule(cfg))
        kw = dict(input_ids=t(pk["input_ids"]), labels=t(pk["labels"]), cu_seqlens=t(pk["cu_seqlens"]),
                  max_seqlen=pk["max_seqlen"], position_ids=t(pk["position_ids"]))
    else:
        kw = dict(input_ids=t(ids), attention_mask=t(mask), labels=t(labels))
    l1, lg1, g1 = _model_step(m16, kw, False)
    l2, lg2, g2 = _model_step(m32, kw, True)
    assert torch.allclose(l1, l2, atol=2e-2, rtol=2e-2), (l1, l2)
    real = kw["labels"].reshape(-1).ne(-100)
    assert torch.allclose(lg1.reshape(-1, L)[real], lg2.reshape(-1, L)[real], atol=5e-2, rtol=5e-2)
    for n in g1:
        rel = (g1[n] - g2[n]).norm() / (g2[n].norm() + 1e-6)
        assert rel < 5e-2, f"{n}: rel grad err {rel:.3g}"
