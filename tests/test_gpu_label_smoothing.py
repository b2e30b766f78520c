"""--label_smoothing_factor on the GPU: the smoothed instantiations of xent.hip, token_head.hip and seq_head.hip, the
heads and model steps on top of them, against ``torch.nn.functional.cross_entropy(fp32 copy, label_smoothing=eps)``.

Every shape is the smallest that reaches its code path. Bounds are the ones the existing test of the same kernel uses at
eps = 0 (named where they are used). Because eps/C is far below an elementwise tolerance at a large C, each kernel also
gets a sharp check: the gradient of a valid row sums to zero over its classes (softmax sums to 1, the smoothed target
sums to 1), so ``|Σ_c dz[c]| <= 0.1·eps·scale``; a missing uniform term or a wrong (1-eps) leaves exactly eps·scale.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from huggingface_sagemaker_tensorflow_distributed_amd import ops  # noqa: E402
from huggingface_sagemaker_tensorflow_distributed_amd.data.packing import pack_batch, position_rule  # noqa: E402
from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model, resolve_config  # noqa: E402
from huggingface_sagemaker_tensorflow_distributed_amd.ops import reference as ref  # noqa: E402

SEED = 0x5EED0123456789AB
EPS = [0.1, 0.5]
# The fused token head's loss against the float64 formula on the kernel's OWN stored bf16 logits, relative. 4 x the
# largest value of the same quantity at eps = 0 (the unsmoothed instantiations) over the shapes of
# test_token_head_smoothed on one MI355X: profiles/label_smoothing/README.md "T_loss".
T_LOSS = 4 * 1.2963e-7
# the same quantity for the sequence head: the bound of tests/test_gpu_seq_head.py test_seq_head_vs_reference
T_LOSS_SEQ = 1e-4


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


def _formula64(logits, labels, eps):
    """(mean loss, n_valid) of the issue's definition in float64: term = lse - (1-eps)·z[y] - (eps/C)·Σ_c z[c]."""
    z = logits.double()
    C = z.shape[-1]
    ok = (labels >= 0) & (labels < C)
    y = labels.clamp(0, C - 1)
    term = torch.logsumexp(z, -1) - (1.0 - eps) * z.gather(1, y[:, None])[:, 0] - eps / C * z.sum(-1)
    n = int(ok.sum())
    return float(term[ok].sum()) / max(n, 1), n


# ------------------------------------------------------------------------------------------------ xent.hip
def _xent_case(gpu, R, V, dtype):
    torch.manual_seed(8)
    logits = (torch.randn(R, V, device=gpu) * 3).to(dtype)
    labels = torch.randint(0, V, (R,), device=gpu)
    labels[4::5] = -100  # every fifth label
    return logits, labels


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("R,V", [(1, 2), (5, 7), (64, 33), (9, 1000)])
def test_xent_smoothed(gpu, R, V, dtype, eps):
    """V = 7 and 33: unaligned rows in both dtypes, the scalar path; V = 1000: the vector path with a partial last
    trip; (1, 2): one row. Bounds: tests/test_gpu_ops.py test_fused_cross_entropy (loss 1e-3·max(1, |ref|), gradient
    _close(2e-2 bf16 | 1e-5 fp32, 1e-3), hits exact)."""
    hip = _hip()
    logits, labels = _xent_case(gpu, R, V, dtype)
    logits.requires_grad_()
    loss, correct = hip.cross_entropy(logits, labels, eps)
    loss.backward()
    l32 = logits.detach().float().requires_grad_()
    want = F.cross_entropy(l32, labels, ignore_index=-100, label_smoothing=eps)
    want.backward()
    print(f"R={R} V={V} {dtype} eps={eps}: loss {loss.item():.6f} ref {want.item():.6f}")
    assert abs(loss.item() - want.item()) < 1e-3 * max(1.0, abs(want.item()))
    _close(logits.grad, l32.grad, 2e-2 if dtype == torch.bfloat16 else 1e-5, 1e-3, "dlogits")
    keep = labels.ne(-100)
    assert int(correct.item()) == int((l32.argmax(-1) == labels)[keep].sum().item())
    assert torch.count_nonzero(logits.grad[~keep]) == 0  # (c)
    # (a) row sums, from the fp32-output variant of the same logits
    g32 = logits.grad
    if dtype == torch.bfloat16:
        x = logits.detach().float().requires_grad_()
        hip.cross_entropy(x, labels, eps)[0].backward()
        g32 = x.grad
        assert torch.count_nonzero(g32[~keep]) == 0
    scale = 1.0 / max(int(keep.sum()), 1)
    rows = g32.double().sum(-1)[keep].abs().max().item()
    print(f"  max |row sum| {rows:.3g}  (bound {0.1 * eps * scale:.3g})")
    assert rows <= 0.1 * eps * scale


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_xent_smoothed_all_rows_ignored(gpu, dtype):
    hip = _hip()  # (d)
    logits = (torch.randn(9, 33, device=gpu) * 3).to(dtype).requires_grad_()
    labels = torch.full((9,), -100, device=gpu, dtype=torch.long)
    loss, correct = hip.cross_entropy(logits, labels, 0.1)
    loss.backward()
    assert loss.item() == 0.0 and correct.item() == 0.0 and torch.count_nonzero(logits.grad) == 0


@pytest.mark.parametrize("eps", EPS)
def test_xent_smoothed_padded_vocabulary(gpu, eps):
    """R = 8, V = 50265 in a [8, 50432] buffer through _C.xent(..., vocab): the unrolled trips of both passes; C is the
    REAL class count, and the padding columns (random junk here) keep an exactly zero gradient (b)."""
    hip = _hip()
    R, V, ld = 8, 50265, 50432
    torch.manual_seed(9)
    logits = (torch.randn(R, ld, device=gpu) * 3).bfloat16()
    labels = torch.randint(0, V, (R,), device=gpu)
    labels[4::5] = -100
    keep = labels.ne(-100)
    n_valid = keep.sum().float().reshape(1)
    outs = {}
    for name, lg in (("bf16", logits), ("fp32", logits.float())):
        dl = torch.full_like(lg, float("nan"))
        stats = torch.zeros(2, device=gpu)
        hip._C.xent(lg, labels, dl, stats, n_valid, V, eps)
        outs[name] = (dl, stats)
    l32 = logits[:, :V].float().requires_grad_()
    want = F.cross_entropy(l32, labels, ignore_index=-100, label_smoothing=eps)
    want.backward()
    for name, (dl, stats) in outs.items():
        loss = stats[0].item() / n_valid.item()
        assert abs(loss - want.item()) < 1e-3 * max(1.0, abs(want.item())), (name, loss, want.item())
        assert not torch.isnan(dl.float()).any()
        assert torch.count_nonzero(dl[:, V:]) == 0  # (b)
        assert torch.count_nonzero(dl[~keep]) == 0  # (c)
        _close(dl[:, :V], l32.grad, 2e-2 if name == "bf16" else 1e-5, 1e-3, f"dlogits {name}")
        assert int(stats[1].item()) == int((l32.argmax(-1) == labels)[keep].sum().item())
    scale = 1.0 / n_valid.item()
    rows = outs["fp32"][0].double().sum(-1)[keep].abs().max().item()
    print(f"eps={eps}: max |row sum| {rows:.3g}  (bound {0.1 * eps * scale:.3g})")
    assert rows <= 0.1 * eps * scale  # (a)


def test_xent_binding_keeps_its_positional_form_and_refuses_a_bad_eps(gpu):
    hip = _hip()
    logits, labels = _xent_case(gpu, 9, 33, torch.float32)
    n_valid = labels.ne(-100).sum().float().reshape(1)
    a, b = torch.zeros(2, device=gpu), torch.zeros(2, device=gpu)
    da, db = torch.empty_like(logits), torch.empty_like(logits)
    hip._C.xent(logits, labels, da, a, n_valid)
    hip._C.xent(logits, labels, db, b, n_valid, 0, 0.0)
    # the gradient bit for bit; the loss sum is added by fp32 atomics over the rows, in whichever order they arrive
    assert torch.equal(da, db) and a[1].item() == b[1].item()
    assert abs(a[0].item() - b[0].item()) <= 1e-6 * abs(a[0].item())
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises((RuntimeError, ValueError)):
            hip._C.xent(logits, labels, da, a, n_valid, 0, bad)
        with pytest.raises(ValueError, match="label_smoothing"):
            ops.cross_entropy(logits, labels, label_smoothing=bad)


# ------------------------------------------------------------------------------------------------ token head
def _tok_inputs(gpu, R, H, C, seed=17, ignore=0.25):
    """tests/test_gpu_token_head.py _inputs."""
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(R, H, generator=g).to(gpu).bfloat16().requires_grad_()
    w = (torch.randn(C, H, generator=g) * 0.05).to(gpu).bfloat16().requires_grad_()
    b = (torch.randn(C, generator=g) * 0.5).to(gpu).bfloat16().requires_grad_()
    labels = torch.randint(0, C, (R,), generator=g)
    if R > 1:
        labels[torch.rand(R, generator=g) < ignore] = -100
        labels[0] = 0
    return h, w, b, labels.to(gpu)


def _tok_reference(h, w, b, labels, p, eps):
    f = [t.detach().float().requires_grad_() for t in (h, w, b)]
    lg = F.linear(ref.dropout(f[0], p, SEED, True), f[1], f[2])
    loss = F.cross_entropy(lg, labels, ignore_index=-100, label_smoothing=eps)
    loss.backward()
    return loss.detach(), lg.detach(), [t.grad for t in f]


def _tok_raw_backward(h, w, logits, labels, stats, p, eps):
    """The backward launch itself on fresh buffers: dh NaN pre-filled, dW / db fp32 from zero, dloss = 1."""
    hip = _hip()
    R, H = h.shape
    C = w.shape[0]
    dh = torch.full((R, H), float("nan"), dtype=torch.bfloat16, device=h.device)
    dW = torch.zeros(C * H, dtype=torch.float32, device=h.device)
    db = torch.zeros(C, dtype=torch.float32, device=h.device)
    part = torch.empty(hip._C.token_head_bwd_blocks(R) * (C * H + C), dtype=torch.float32, device=h.device)
    dl = torch.ones(1, dtype=torch.float32, device=h.device)
    hip._C.token_head_bwd(h.detach(), w.detach(), logits, labels, stats, dl, dh, part, dW, db, float(p),
                          hip._s64(SEED), eps)
    return dh, dW.view(C, H), db


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("C", [2, 3, 9, 16])
@pytest.mark.parametrize("H", [64, 768])
@pytest.mark.parametrize("R", [1, 17, 255])
def test_token_head_smoothed(gpu, R, H, C, p, eps):
    """Bounds: tests/test_gpu_token_head.py test_token_head_vs_reference (logits _close(3e-2, 3e-2), loss 2e-2·max(1,
    |ref|), each gradient's relative error < 4e-2, n / hits exact, stats[0]·n == stats[3] within 1e-5)."""
    h, w, b, labels = _tok_inputs(gpu, R, H, C)
    loss, logits = ops.token_head(h, w, b, labels, p, SEED, label_smoothing=eps)
    stats = getattr(loss, "_hsd_stats", None)
    assert stats is not None and "TokenHead" in type(loss.grad_fn).__name__, "the fused HIP head did not run"
    loss.backward()
    loss_ref, lg_ref, g_ref = _tok_reference(h, w, b, labels, p, eps)
    valid = labels.ne(-100)
    print(f"R={R} H={H} C={C} p={p} eps={eps}: loss {loss.item():.5f} ref {loss_ref.item():.5f}")
    _close(logits, lg_ref, 3e-2, 3e-2, "logits")
    assert abs(loss.item() - loss_ref.item()) < 2e-2 * max(1.0, abs(loss_ref.item())), (loss.item(), loss_ref.item())
    for n, a, r_ in zip(["h", "w", "b"], (h.grad, w.grad, b.grad), g_ref):
        rel = (a.float() - r_).norm() / (r_.norm() + 1e-6)
        print(f"  d{n}: rel err {rel:.3g}")
        assert rel < 4e-2, f"{n}: rel err {rel:.3g}"
    assert stats[2].item() == valid.sum().item()
    lg_cpu, lab_cpu = logits.float().cpu(), labels.cpu()
    hits = int(((lg_cpu.argmax(-1) == lab_cpu) & lab_cpu.ne(-100)).sum())
    assert stats[1].item() == hits  # the argmax does not depend on eps
    assert abs(stats[0].item() * max(1.0, stats[2].item()) - stats[3].item()) <= 1e-5 * max(1.0, abs(stats[3].item()))
    dh, dW, db = _tok_raw_backward(h, w, logits, labels, stats, p, eps)
    assert not torch.isnan(dh.float()).any()
    assert torch.count_nonzero(dh[~valid]) == 0
    assert torch.equal(dh, h.grad) and torch.equal(dW.to(torch.bfloat16), w.grad) and torch.equal(db.bfloat16(), b.grad)
    # sharp: Σ_c db[c] = Σ_rows Σ_c g = 0, and the loss is the formula on the kernel's own logits
    print(f"  |Σ db| {db.double().sum().abs().item():.3g}  (bound {0.1 * eps:.3g})")
    assert db.double().sum().abs().item() <= 0.1 * eps
    l64, n64 = _formula64(logits, labels, eps)
    rel = abs(stats[0].item() - l64) / max(abs(l64), 1e-12)
    print(f"  loss vs float64 formula on the stored logits: rel {rel:.3g}")
    assert n64 == stats[2].item() and rel <= T_LOSS, (stats[0].item(), l64)


def test_token_head_smoothed_two_runs_give_the_same_bits(gpu):
    h, w, b, labels = _tok_inputs(gpu, 255, 768, 9)
    outs = []
    for _ in range(2):
        for t in (h, w, b):
            t.grad = None
        loss, logits = ops.token_head(h, w, b, labels, 0.1, SEED, label_smoothing=0.1)
        loss.backward()
        outs.append((loss.detach().clone(), logits.clone(), h.grad.clone(), w.grad.clone(), b.grad.clone()))
    for a, c in zip(*outs):
        assert torch.equal(a, c)
    # and eps = 0 is the call without the keyword
    res = []
    for kw in ({}, {"label_smoothing": 0.0}):
        for t in (h, w, b):
            t.grad = None
        loss, logits = ops.token_head(h, w, b, labels, 0.1, SEED, **kw)
        loss.backward()
        res.append((loss.detach().clone(), logits.clone(), h.grad.clone(), w.grad.clone(), b.grad.clone()))
    for a, c in zip(*res):
        assert torch.equal(a, c)
    assert not torch.equal(res[0][0], outs[0][0])


def test_token_head_smoothed_all_rows_ignored_and_composed(gpu, monkeypatch):
    h, w, b, labels = _tok_inputs(gpu, 255, 768, 9)
    loss, _ = ops.token_head(h, w, b, torch.full_like(labels, -100), 0.1, SEED, label_smoothing=0.1)
    loss.backward()
    assert loss.item() == 0.0 and loss._hsd_stats[2].item() == 0.0
    for t in (h, w, b):
        assert torch.count_nonzero(t.grad) == 0
        t.grad = None
    # HSD_TOKEN_HEAD=composed carries eps through _sum_ce: the fused-against-composed bounds of
    # tests/test_gpu_token_head.py test_fused_path_runs_and_unsupported_shapes_fall_back
    fused, lg_f = ops.token_head(h, w, b, labels, 0.1, SEED, label_smoothing=0.1)
    monkeypatch.setattr(ops, "TOKEN_HEAD_FUSED", False)
    comp, lg_c = ops.token_head(h, w, b, labels, 0.1, SEED, label_smoothing=0.1)
    assert "TokenHead" not in type(comp.grad_fn).__name__
    assert abs(fused.item() - comp.item()) < 2e-2 * max(1.0, abs(comp.item()))
    _close(lg_f, lg_c, 3e-2, 3e-2, "fused vs composed logits")
    # the composed path did smooth: its loss is the formula on its own logits (fp32 sums of 191 rows: 1e-5), and the
    # unsmoothed formula on the same logits is far from it
    l64, _ = _formula64(lg_c, labels, 0.1)
    l64_plain, _ = _formula64(lg_c, labels, 0.0)
    assert abs(comp.item() - l64) <= 1e-5 * abs(l64) and abs(l64 - l64_plain) > 10 * 1e-5 * abs(l64)


# ------------------------------------------------------------------------------------------------ sequence head
def _seq_inputs(R, C, H, gpu, S=3, seed=17):
    """tests/test_gpu_seq_head.py _inputs."""
    torch.manual_seed(seed)
    mk = lambda *s, sc=0.05: (torch.randn(*s, device=gpu) * sc).bfloat16().requires_grad_()  # noqa: E731
    h = torch.randn(R, S, H, device=gpu).bfloat16().requires_grad_()
    return [h, mk(H, H, sc=H ** -0.5), mk(H, sc=0.5), mk(C, H, sc=H ** -0.5), mk(C, sc=0.5)]


def _seq_labels(R, C, gpu):
    g = torch.Generator().manual_seed(3 + 7 * R + C)
    lab = torch.randint(0, C, (R,), generator=g)
    if R > 1:
        lab[1] = -100
    if R > 8:
        lab[5::7] = -100
    return lab.to(gpu)


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("C", [2, 3, 5, 64])
@pytest.mark.parametrize("H", [64, 768])
@pytest.mark.parametrize("B", [1, 8, 37])
def test_seq_head_smoothed(gpu, monkeypatch, B, H, C, eps):
    """ops.cls_head(..., label_smoothing=eps): every single-label C runs seq_head.hip (C = 2 and 3 leave cls_head.hip).
    Bounds: tests/test_gpu_seq_head.py test_seq_head_vs_reference (loss 2e-2·max(1, |ref|), logits _close(3e-2, 3e-2),
    each gradient < 4e-2, hits / n exact from the returned logits, loss within 1e-4 of the float64 recomputation)."""
    hip = _hip()
    calls = []
    real = hip.seq_head
    monkeypatch.setattr(hip, "seq_head", lambda *a, **k: (calls.append(a[3].shape[0]), real(*a, **k))[1])
    act, p = (("tanh", 0.1), ("relu", 0.1), ("tanh", 0.0))[(B + C) % 3]
    p_in = p if act == "tanh" and B % 2 else 0.0
    params = _seq_inputs(B, C, H, gpu)
    params[4].main_grad = torch.zeros(C, device=gpu)  # db2 in fp32 for the sharp check
    labels = _seq_labels(B, C, gpu)
    loss, logits = ops.cls_head(*params, labels, act, p_in, 21, p, 22, label_smoothing=eps)
    stats = getattr(loss, "_hsd_stats", None)
    assert calls == [C] and stats is not None and "SeqHead" in type(loss.grad_fn).__name__, "seq_head.hip did not run"
    loss.backward()
    db2 = params[4].main_grad
    g_hip = [t.grad.float() for t in params[:4]] + [db2]
    f = [t.detach().float().requires_grad_() for t in params]
    lg_ref = ref.cls_head(f[0][:, 0], f[1], f[2], f[3], f[4], act, p_in, 21, p, 22, True)
    loss_ref = F.cross_entropy(lg_ref, labels, ignore_index=-100, label_smoothing=eps)
    loss_ref.backward()
    print(f"B={B} H={H} C={C} eps={eps}: loss {loss.item():.5f} ref {loss_ref.item():.5f}")
    assert abs(loss.item() - loss_ref.item()) < 2e-2 * max(1.0, abs(loss_ref.item())), (loss.item(), loss_ref.item())
    _close(logits, lg_ref, 3e-2, 3e-2, "logits")
    for n, a, b in zip(["h", "w1", "b1", "w2", "b2"], g_hip, [t.grad for t in f]):
        rel = (a - b).norm() / (b.norm() + 1e-6)
        assert rel < 4e-2, f"{n}: rel err {rel:.3g}"
    assert torch.count_nonzero(g_hip[0][:, 1:]) == 0
    if B > 1:
        assert torch.count_nonzero(g_hip[0][1]) == 0  # the ignored row
    valid = labels.ne(-100)
    hits = int(((logits.float().argmax(-1) == labels) & valid).sum())
    assert int(stats[1].item()) == hits and int(stats[2].item()) == int(valid.sum())
    assert abs(stats[0].item() * max(1.0, stats[2].item()) - stats[3].item()) <= 1e-5 * max(1.0, abs(stats[3].item()))
    print(f"  |Σ db2| {db2.double().sum().abs().item():.3g}  (bound {0.1 * eps:.3g})")
    assert db2.double().sum().abs().item() <= 0.1 * eps
    l64, n64 = _formula64(logits, labels, eps)
    rel = abs(stats[0].item() - l64) / max(abs(l64), 1e-12)
    print(f"  loss vs float64 formula on the stored logits: rel {rel:.3g}")
    assert rel <= T_LOSS_SEQ, (stats[0].item(), l64)


def _seq_raw(gpu, R, C, H, eps, labels):
    """tests/test_gpu_seq_head.py _raw_bwd: one forward + two backward launches on the bindings."""
    C_ = _hip()._C
    torch.manual_seed(5)
    pre = torch.randn(R, H, device=gpu).bfloat16()
    w2 = (torch.randn(C, H, device=gpu) * H ** -0.5).bfloat16()
    b2 = (torch.randn(C, device=gpu) * 0.5).bfloat16()
    t, logits = torch.empty_like(pre), torch.empty(R, C, device=gpu, dtype=torch.bfloat16)
    partials = torch.empty(C_.seq_head_blocks(R) * 4, device=gpu)
    stats = torch.empty(4, device=gpu)
    C_.seq_head_fwd(pre, w2, b2, labels, t, logits, partials, stats, 0, 0.5, 0, 0.1, 77, eps)
    out = []
    for _ in range(2):
        dpre = torch.full_like(pre, float("nan"))  # every element must be written
        dW2, db2 = torch.zeros(C * H, device=gpu), torch.zeros(C, device=gpu)
        g = torch.empty(R * C, device=gpu)
        part = torch.empty(C_.seq_head_workspace(R, H, C), device=gpu)
        C_.seq_head_bwd(t, w2, logits, labels, stats, torch.ones(1, device=gpu), dpre, g, part, dW2, db2, 0, 0, 0.1, 77,
                        eps)
        out.append((dpre, dW2, db2))
    return stats, out


def test_seq_head_smoothed_is_bit_reproducible_fully_written_and_zero_when_all_ignored(gpu):
    R, C, H = 37, 5, 768
    labels = _seq_labels(R, C, gpu)
    stats, (a, b) = _seq_raw(gpu, R, C, H, 0.1, labels)
    for x, y, n in zip(a, b, ("dpre", "dW2", "db2")):
        assert torch.equal(x, y), n
        assert bool(torch.isfinite(x).all()), n
    assert torch.count_nonzero(a[0][1]) == 0 and torch.count_nonzero(a[0][2]) > 0
    stats, (a, _) = _seq_raw(gpu, R, C, H, 0.1, torch.full_like(labels, -100))
    assert stats[0].item() == 0.0 and stats[2].item() == 0.0
    for x in a:
        assert torch.count_nonzero(x) == 0
    with pytest.raises(RuntimeError, match="label_smoothing"):  # BCE / MSE are not smoothed
        _hip()._C.seq_head_fwd(torch.zeros(4, 64, device=gpu).bfloat16(), torch.zeros(2, 64, device=gpu).bfloat16(),
                               torch.zeros(2, device=gpu).bfloat16(), torch.zeros(4, 2, device=gpu),
                               torch.zeros(4, 64, device=gpu).bfloat16(), torch.zeros(4, 2, device=gpu).bfloat16(),
                               torch.zeros(4, device=gpu), torch.zeros(4, device=gpu), 1, 0.5, 0, 0.0, 0, 0.1)


def test_seq_head_eps_zero_is_todays_dispatch_and_composed_agrees(gpu, monkeypatch):
    """C = 2, eps = 0: label_smoothing=0.0 is the call without the keyword (cls_head.hip), bit for bit (B = 8: at most
    two addends per atomic, whose sum does not depend on their order). HSD_SEQ_HEAD=composed against the fused path:
    the bounds of tests/test_gpu_seq_head.py test_dispatch (loss 2e-2·max(1, |loss|), logits _close(3e-2, 3e-2))."""
    hip = _hip()
    labels = _seq_labels(8, 2, gpu)
    res = []
    for kw in ({}, {"label_smoothing": 0.0}):
        params = _seq_inputs(8, 2, 64, gpu)
        loss, logits = ops.cls_head(*params, labels, "tanh", 0.0, 0, 0.1, 9, **kw)
        assert "ClsHead" in type(loss.grad_fn).__name__
        loss.backward()
        res.append([loss.detach(), logits] + [t.grad for t in params])
    for a, b in zip(*res):
        assert torch.equal(a, b)
    for C in (2, 5):
        params = _seq_inputs(37, C, 768, gpu)
        labels = _seq_labels(37, C, gpu)
        loss, logits = ops.cls_head(*params, labels, "relu", 0.0, 0, 0.1, 9, label_smoothing=0.1)
        assert "SeqHead" in type(loss.grad_fn).__name__
        monkeypatch.setattr(ops, "SEQ_HEAD_FUSED", False)
        loss2, logits2 = ops.cls_head(*params, labels, "relu", 0.0, 0, 0.1, 9, label_smoothing=0.1)
        monkeypatch.setattr(ops, "SEQ_HEAD_FUSED", True)
        assert "SeqHead" not in type(loss2.grad_fn).__name__
        assert abs(loss.item() - loss2.item()) < 2e-2 * max(1.0, abs(loss2.item()))
        _close(logits, logits2, 3e-2, 3e-2, "fused vs composed logits")
        # the composed path did smooth: its loss is the formula on its own logits, the unsmoothed one is not
        l64, _ = _formula64(logits2, labels, 0.1)
        l64_plain, _ = _formula64(logits2, labels, 0.0)
        assert abs(loss2.item() - l64) <= T_LOSS_SEQ * abs(l64) and abs(l64 - l64_plain) > 10 * T_LOSS_SEQ * abs(l64)
    with pytest.raises(ValueError, match="label_smoothing"):
        ops.cls_head(*_seq_inputs(4, 2, 64, gpu), torch.zeros(4, 2, device=gpu), "tanh", 0.0, 0, 0.0, 0,
                     problem_type="regression", label_smoothing=0.1)


# ------------------------------------------------------------------------------------------------ MLM head
@pytest.mark.parametrize("fixed", [False, True])
def test_mlm_head_smoothed(gpu, fixed):
    """ops.mlm_head / ops.mlm_head_fixed at H = 256, V = 50265 (padded 50432), eps = 0.1. Bounds: tests/test_gpu_ops.py
    test_mlm_head_vs_reference (loss 1e-2 relative, logits _close(3e-2, 3e-2), each gradient < 5e-2, padding exactly
    zero). The decoder-bias gradient is the column sum of dz: it sums to 0 over the real columns."""
    from huggingface_sagemaker_tensorflow_distributed_amd.ops.rng import MlmMask

    eps = 0.1
    torch.manual_seed(23)
    H, V, Vp, T = 256, 50265, 50432, 512
    mk = lambda *s, sc=0.05: (torch.randn(*s, device=gpu) * sc).bfloat16()  # noqa: E731
    h = torch.randn(T, H, device=gpu).bfloat16().requires_grad_()
    w1, b1 = mk(H, H).requires_grad_(), mk(H).requires_grad_()
    lw = (1 + 0.1 * torch.randn(H, device=gpu)).bfloat16().requires_grad_()
    lb = mk(H).requires_grad_()
    wemb = mk(Vp, H)
    wemb[V:] = 0
    wemb.requires_grad_()
    bias = mk(Vp)
    bias[V:] = 0
    bias.requires_grad_()
    bias.main_grad = torch.zeros(Vp, device=gpu)  # fp32, for the sum below
    labels = torch.full((T,), -100, device=gpu, dtype=torch.long)
    pos = torch.randperm(T, device=gpu)[:80].sort().values  # 80 selected rows (64 .. 128)
    labels[pos] = torch.randint(0, V, (80,), device=gpu)
    params = [h, w1, b1, lw, lb, wemb, bias]
    if fixed:
        cap = 128
        sel = torch.zeros(cap, dtype=torch.long, device=gpu)
        sel[:80] = pos
        tgt = torch.full((cap,), -100, dtype=torch.long, device=gpu)
        tgt[:80] = labels[pos]
        inv = torch.full((T,), -1, dtype=torch.int32, device=gpu)
        inv[pos] = torch.arange(80, dtype=torch.int32, device=gpu)
        mask = MlmMask(None, None, sel, tgt, inv, torch.tensor([80, 0], dtype=torch.int32, device=gpu),
                       torch.full((1,), 80.0, device=gpu), cap)
        loss, logits = ops.mlm_head_fixed(h, mask, w1, b1, lw, lb, 1e-5, wemb, bias, V, label_smoothing=eps)
        assert getattr(loss, "_hsd_stats", None) is not None, "the fused HIP head did not run"
        assert logits.shape == (cap, V) and loss._hsd_stats[2].item() == 80
        logits = logits[:80]
    else:
        loss, logits = ops.mlm_head(h, labels, w1, b1, lw, lb, 1e-5, wemb, bias, V, label_smoothing=eps)
        assert logits.shape == (80, V)
    assert getattr(loss, "_hsd_correct", None) is not None, "the fused HIP head did not run"
    loss.backward()
    g_hip = [t.grad.float() for t in params[:6]] + [bias.main_grad]
    f = [t.detach().float().requires_grad_() for t in params]
    loss_ref, lg_ref = ref.mlm_head(f[0], labels, f[1], f[2], f[3], f[4], 1e-5, f[5], f[6], V, eps)
    loss_ref.backward()
    plain = F.cross_entropy(lg_ref.detach(), labels[pos])
    print(f"fixed={fixed}: loss {loss.item():.5f} ref {loss_ref.item():.5f} (unsmoothed {plain.item():.5f})")
    assert abs(loss.item() - loss_ref.item()) < 1e-2 * abs(loss_ref.item()), (loss.item(), loss_ref.item())
    _close(logits, lg_ref, 3e-2, 3e-2, "logits")
    for n, a, b in zip(["h", "w1", "b1", "ln_w", "ln_b", "wemb", "bias"], g_hip, [t.grad for t in f]):
        rel = (a - b).norm() / (b.norm() + 1e-6)
        print(f"  {n}: rel err {rel:.3g}")
        assert rel < 5e-2, f"{n}: rel err {rel:.3g}"
    assert torch.count_nonzero(g_hip[5][V:]) == 0 and torch.count_nonzero(g_hip[6][V:]) == 0  # padding stays 0
    tot = g_hip[6][:V].double().sum().abs().item()
    print(f"  |Σ dbias| {tot:.3g}  (bound {0.1 * eps:.3g})")
    assert tot <= 0.1 * eps


# ------------------------------------------------------------------------------------------------ fp32 on the GPU
def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / (b.double().norm().cpu() + 1e-30))


@pytest.mark.parametrize("head", ["sequence", "token"])
def test_fp32_heads_smoothed(gpu, head):
    """fp32 tensors on the GPU, eps = 0.1, against the CPU reference at the bounds of tests/test_gpu_fp32.py
    test_fp32_bert_step_on_kernels_matches_cpu (loss 1e-4 relative, each gradient 1e-3 relative). The sequence head
    skips the fp32 fused tail and ends in xent_kernel<false, true>."""
    eps = 0.1
    torch.manual_seed(3)
    if head == "sequence":
        B, S, H, C = 37, 3, 768, 3
        cpu = [torch.randn(B, S, H), torch.randn(H, H) * H ** -0.5, torch.randn(H) * 0.5, torch.randn(C, H) * H ** -0.5,
               torch.randn(C) * 0.5]
        labels = torch.randint(0, C, (B,))
        labels[1] = -100
        run = lambda t, lab: ops.cls_head(*t, lab, "tanh", 0.1, 21, 0.1, 22, label_smoothing=eps)  # noqa: E731
    else:
        R, H, C = 255, 768, 8
        cpu = [torch.randn(R, H), torch.randn(C, H) * 0.05, torch.randn(C) * 0.5]
        labels = torch.randint(0, C, (R,))
        labels[torch.rand(R) < 0.25] = -100
        run = lambda t, lab: ops.token_head(*t, lab, 0.1, SEED, label_smoothing=eps)  # noqa: E731
    dev = [t.clone().to(gpu).requires_grad_() for t in cpu]
    cpu = [t.requires_grad_() for t in cpu]
    l_gpu, lg_gpu = run(dev, labels.to(gpu))
    l_cpu, lg_cpu = run(cpu, labels)
    if head == "sequence":
        assert "CrossEntropy" in type(l_gpu.grad_fn).__name__, "xent_kernel<false, true> did not run"
    l_gpu.backward()
    l_cpu.backward()
    l64, _ = _formula64(lg_cpu.detach(), labels, eps)
    assert abs(float(l_cpu) - l64) <= 1e-5 * abs(l64)
    assert abs(float(l_gpu) - float(l_cpu)) <= 1e-4 * abs(float(l_cpu)), (float(l_gpu), float(l_cpu))
    for i, (a, b) in enumerate(zip(dev, cpu)):
        r = _rel(a.grad, b.grad)
        assert r < 1e-3, (i, r)


# ------------------------------------------------------------------------------------------------ model steps
def _model_step(model, kw, force_torch):
    """tests/test_gpu_token_head.py _model_step."""
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


def _pair(gpu, name, task, **cfg_kw):
    cfg = resolve_config(name, **cfg_kw).replace(hidden_size=128, num_attention_heads=2, intermediate_size=256)
    m32 = build_model(cfg, task=task, seed=0).to(gpu)
    assert m32.label_smoothing == 0.0
    m16 = copy.deepcopy(m32).bfloat16()
    with torch.no_grad():  # the reference holds the bf16-rounded weights
        for p32, p16 in zip(m32.parameters(), m16.parameters()):
            p32.copy_(p16.float())
    m32.label_smoothing = m16.label_smoothing = 0.1
    return cfg, m32, m16


def _ragged(cfg, B, S, seed=0):
    g = np.random.default_rng(seed)
    lengths = np.array([S, S * 5 // 8, S // 4 + 1, 2] * (B // 4))
    ids = g.integers(5, cfg.vocab_size, size=(B, S)).astype(np.int64)
    mask = (np.arange(S)[None, :] < lengths[:, None]).astype(np.int64)
    ids[mask == 0] = cfg.pad_token_id
    return g, ids, mask


def _compare(out16, out32, real=None, C=None):
    """The model-step bounds of tests/test_gpu_token_head.py test_model_step_vs_fp32_reference_model (tests/
    test_gpu_e2e.py's): loss atol = rtol = 2e-2, logits 5e-2, each parameter gradient's relative error < 5e-2."""
    (l1, lg1, g1), (l2, lg2, g2) = out16, out32
    assert torch.allclose(l1, l2, atol=2e-2, rtol=2e-2), (l1, l2)
    if real is not None:
        assert torch.allclose(lg1.reshape(-1, C)[real], lg2.reshape(-1, C)[real], atol=5e-2, rtol=5e-2)
    for n in g1:
        rel = (g1[n] - g2[n]).norm() / (g2[n].norm() + 1e-6)
        assert rel < 5e-2, f"{n}: rel grad err {rel:.3g}"


def test_model_step_sequence_classification_smoothed(gpu):
    cfg, m32, m16 = _pair(gpu, "hsd-tiny-bert", "sequence-classification", num_labels=2)
    g, ids, mask = _ragged(cfg, 8, 64)
    labels = g.integers(0, 2, size=(8,)).astype(np.int64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    kw = dict(input_ids=t(ids), attention_mask=t(mask), labels=t(labels))
    out16, out32 = _model_step(m16, kw, False), _model_step(m32, kw, True)
    _compare(out16, out32, torch.ones(8, dtype=torch.bool, device=gpu), 2)
    l64, _ = _formula64(out16[1], kw["labels"], 0.1)
    assert abs(out16[0].item() - l64) <= T_LOSS_SEQ * abs(l64)  # the smoothed loss of the returned logits


@pytest.mark.parametrize("packed", [False, True])
def test_model_step_token_classification_smoothed(gpu, packed):
    cfg, m32, m16 = _pair(gpu, "hsd-tiny-roberta", "token-classification", num_labels=9)
    g, ids, mask = _ragged(cfg, 4, 128)
    labels = g.integers(0, 9, size=(4, 128)).astype(np.int64)
    labels[g.random((4, 128)) < 0.25] = -100
    labels[:, 0] = -100
    labels[mask == 0] = -100
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    if packed:
        pk = pack_batch(ids, mask, labels, **position_rule(cfg))
        kw = dict(input_ids=t(pk["input_ids"]), labels=t(pk["labels"]), cu_seqlens=t(pk["cu_seqlens"]),
                  max_seqlen=pk["max_seqlen"], position_ids=t(pk["position_ids"]))
    else:
        kw = dict(input_ids=t(ids), attention_mask=t(mask), labels=t(labels))
    out16, out32 = _model_step(m16, kw, False), _model_step(m32, kw, True)
    _compare(out16, out32, kw["labels"].reshape(-1).ne(-100), 9)
    l64, _ = _formula64(out16[1].reshape(-1, 9), kw["labels"].reshape(-1), 0.1)
    assert abs(out16[0].item() - l64) <= T_LOSS * abs(l64)


def test_model_step_masked_lm_dynamic_smoothed(gpu, monkeypatch):
    hip = _hip()
    seen = []
    real = hip.mlm_head_fixed
    monkeypatch.setattr(hip, "mlm_head_fixed", lambda *a: (seen.append(a[-1]), real(*a))[1])
    cfg, m32, m16 = _pair(gpu, "hsd-tiny-roberta", "masked-lm")
    g, ids, mask = _ragged(cfg, 4, 128)
    for m in (m32, m16):
        m.set_mlm_masking("dynamic", 0.15)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    kw = dict(input_ids=t(ids), attention_mask=t(mask), labels=t(np.where(mask != 0, 0, -100).astype(np.int64)))
    out16, out32 = _model_step(m16, kw, False), _model_step(m32, kw, True)
    _compare(out16, out32)
    assert seen == [0.1], "the fused fixed-capacity head did not run with the model's label_smoothing"


# ------------------------------------------------------------------------------------------------ whole-step graph
def _trainer(gpu, graph_replay):
    """tests/test_gpu_token_head.py _trainer with model.label_smoothing = 0.1."""
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedAdam
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore
    from huggingface_sagemaker_tensorflow_distributed_amd.train.trainer import Trainer

    cfg = resolve_config("bert-base-uncased", num_labels=9).replace(num_hidden_layers=2)
    model = build_model(cfg, task="token-classification", seed=0).to(gpu)
    model.rng.base_seed = 5
    model.label_smoothing = 0.1
    store = FlatParamStore(model, gpu, compute_dtype=torch.bfloat16)
    opt = FusedAdam(store, lr=1e-4, weight_decay=0.01)
    tr = Trainer(model, store, opt, None, gpu, hip_graph=True, lr_schedule="linear", lr_warmup_steps=2)
    tr._graph_replay = graph_replay
    return tr


def test_whole_step_graph_replay_matches_eager_smoothed(gpu, monkeypatch):
    """tests/test_gpu_token_head.py test_whole_step_graph_replay_matches_eager with eps = 0.1: eps is a host constant
    of the launches, so the captured graph carries it (same bounds: losses 2e-3·max(1, |loss|), weights 1e-4)."""
    monkeypatch.setenv("HSD_GRAPH_FULL", "1")
    g = torch.Generator().manual_seed(0)
    batches = []
    for _ in range(3):
        ids = torch.randint(1000, 30000, (16, 128), generator=g)
        am = torch.ones(16, 128, dtype=torch.long)
        am[3, 70:] = 0
        labels = torch.randint(0, 9, (16, 128), generator=g)
        labels[torch.rand(16, 128, generator=g) < 0.25] = -100
        labels[am == 0] = -100
        batches.append({"input_ids": ids.to(gpu), "attention_mask": am.to(gpu), "labels": labels.to(gpu)})
    res = {}
    for replay in (False, True):
        tr = _trainer(gpu, replay)
        tr.total_steps = 3
        losses = [float(tr.train_step([b])) for b in batches]
        if replay:
            assert len(tr._graphs) == 1 and tr._full_graph
        assert tr.optimizer.step_count == 3
        torch.cuda.synchronize()
        res[replay] = (losses, tr.store.master.clone())
        tr._seed.close()
    (l0, w0), (l1, w1) = res[False], res[True]
    for a, b in zip(l0, l1):
        assert abs(a - b) <= 2e-3 * max(1.0, abs(a)), (l0, l1)
    rel = (w0 - w1).norm() / w0.norm()
    assert rel < 1e-4, float(rel)
    # C = 9, eps = 0.1: no smoothed loss lies below -Σ q·log q of the smoothed target (0.4848)
    assert min(l1) > 0.48
