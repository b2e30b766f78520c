"""The fused sequence-level head of --problem_type (csrc/kernels/seq_head.hip, ops/hip.py _SeqHead), GPU tier.

Single-label CE for 5..64 classes, multi-label BCE-with-logits and regression MSE for 1..64 columns are checked against
the fp32 reference head + ``reference.seq_loss`` with the bounds tests/test_gpu_ops.py uses for cls_head.hip (loss 2e-2
relative, logits ``_close(3e-2, 3e-2)``, each gradient ``|d| / |ref| < 4e-2``); loss and hits are recomputed in float64
from the bf16 logits the head returns (hits exactly, loss within 1e-4: far above fp32 summation error at these sizes,
far below a wrong divisor or sign)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

from huggingface_sagemaker_tensorflow_distributed_amd import ops  # noqa: E402
from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model, resolve_config  # noqa: E402
from huggingface_sagemaker_tensorflow_distributed_amd.ops import reference as ref  # noqa: E402

CE, BCE, MSE = "single_label_classification", "multi_label_classification", "regression"
NAN = float("nan")


def _hip():
    from huggingface_sagemaker_tensorflow_distributed_amd.ops import hip

    return hip


def _close(a, b, atol, rtol, what=""):
    """tests/test_gpu_ops.py ``_close``: at most 0.1 % of the elements beyond tolerance, none beyond 4x."""
    a = a.float()
    b = b.float()
    err = (a - b).abs()
    tol = atol * b.abs().max().clamp_min(1e-6) + rtol * b.abs()
    bad = (err > tol).float().mean().item()
    worst = (err / tol).max().item()
    assert bad <= 1e-3, f"{what}: {bad*100:.3f}% elements out of tol, max err {err.max().item():.4g}"
    assert worst <= 4.0, f"{what}: an element is {worst:.2f}x beyond tolerance (max err {err.max().item():.4g})"


def _labels(ptype, R, C, gpu, ignore=None, gen_seed=3):
    g = torch.Generator().manual_seed(gen_seed + 7 * R + C)
    if ptype == CE:
        lab = torch.randint(0, C, (R,), generator=g)
        if ignore is not None:
            lab[ignore] = -100
    else:
        lab = (torch.rand(R, C, generator=g) < 0.3).float() if ptype == BCE else torch.randn(R, C, generator=g)
        if ignore is not None:
            lab[ignore] = NAN
    return lab.to(gpu)


def _inputs(R, C, H, gpu, S=3, seed=17):
    torch.manual_seed(seed)
    mk = lambda *s, sc=0.05: (torch.randn(*s, device=gpu) * sc).bfloat16().requires_grad_()  # noqa: E731
    h = torch.randn(R, S, H, device=gpu).bfloat16().requires_grad_()
    # W2 ~ 1 / sqrt(H): logits O(1) (the 0.5 of the cls_head tests would saturate the sigmoid)
    return [h, mk(H, H, sc=H ** -0.5), mk(H, sc=0.5), mk(C, H, sc=H ** -0.5), mk(C, sc=0.5)]


def _recompute64(logits, labels, ptype, tol):
    """(loss, hits, n) in float64 from the stored bf16 logits."""
    z = logits.double()
    C = z.shape[1]
    if ptype == CE:
        ok = (labels >= 0) & (labels < C)
        lab = labels.clamp(0, C - 1)
        per = torch.logsumexp(z, -1) - z.gather(1, lab[:, None])[:, 0]
        good = z.argmax(-1) == lab
    else:
        y = labels.double().view(-1, C)
        ok = ~torch.isnan(y[:, 0])
        y = torch.where(ok[:, None], y, torch.zeros_like(y))
        if ptype == BCE:
            per = (z.clamp(min=0) - z * y + torch.log1p(torch.exp(-z.abs()))).sum(-1) / C
            good = ((z > 0) == (y > 0.5)).all(-1)
        else:
            per = ((z - y) ** 2).sum(-1) / C
            good = ((z - y).abs() <= tol).all(-1)
    n = int(ok.sum())
    return float(per[ok].sum()) / max(n, 1), int((good & ok).sum()), n


# every C (a single lane, a full group of 4, a group remainder of 1, past lane 32, a full wave), R (the row-loop
# breaks, one to three partial blocks) and H (one chunk, a partial second chunk row, both chunks) of the issue, each
# with several of the others
_SHAPES = [(1, 1, 8), (1, 17, 1024), (4, 5, 520), (4, 33, 8), (5, 17, 1024), (5, 33, 520), (33, 33, 520), (33, 5, 8),
           (64, 33, 1024), (64, 1, 8), (64, 17, 520), (33, 1, 1024)]
_CASES = [(pt, C, R, H, act, p) for (C, R, H) in _SHAPES for pt in (CE, BCE, MSE) if pt != CE or C >= 5
          for (act, p) in (("tanh", 0.0), ("relu", 0.1), ("tanh", 0.1), ("relu", 0.0))]


@pytest.mark.parametrize("ptype,C,R,H,act,p", _CASES)
def test_seq_head_vs_reference(gpu, ptype, C, R, H, act, p):
    tol = 0.5
    params = _inputs(R, C, H, gpu)
    labels = _labels(ptype, R, C, gpu, ignore=1 if R > 1 else None)
    p_in = p if act == "tanh" and R % 2 else 0.0  # the roberta head's input dropout on some cases
    loss, logits = ops.cls_head(*params, labels, act, p_in, 21, p, 22, problem_type=ptype, tol=tol)
    stats = getattr(loss, "_hsd_stats", None)
    assert stats is not None and "SeqHead" in type(loss.grad_fn).__name__, "the fused HIP head did not run"
    loss.backward()
    g_hip = [t.grad.float() for t in params]
    f = [t.detach().float().requires_grad_() for t in params]
    lg_ref = ref.cls_head(f[0][:, 0], f[1], f[2], f[3], f[4], act, p_in, 21, p, 22, True)
    loss_ref, stats_ref = ref.seq_loss(lg_ref, labels, ptype, tol)
    loss_ref.backward()
    assert abs(loss.item() - loss_ref.item()) < 2e-2 * max(1.0, abs(loss_ref.item())), (loss.item(), loss_ref.item())
    _close(logits, lg_ref, 3e-2, 3e-2, "logits")
    assert stats[2].item() == stats_ref[2].item()
    for n, a, b in zip(["h", "w1", "b1", "w2", "b2"], g_hip, [t.grad for t in f]):
        rel = (a - b).norm() / (b.norm() + 1e-6)
        assert rel < 4e-2, f"{n}: rel err {rel:.3g}"
    assert torch.count_nonzero(g_hip[0][:, 1:]) == 0  # only the first-token rows receive gradient
    if R > 1:
        assert torch.count_nonzero(g_hip[0][1]) == 0  # the ignored row
    # loss and hits from the returned logits, in float64
    l64, hits64, n64 = _recompute64(logits, labels, ptype, tol)
    assert int(stats[1].item()) == hits64 and int(stats[2].item()) == n64
    rel = abs(stats[0].item() - l64) / max(abs(l64), 1e-12)
    print(f"loss vs float64 recomputation: rel {rel:.3g}")  # the largest one seen: profiles/seq_head/README.md
    assert rel < 1e-4, (stats[0].item(), l64)
    assert abs(stats[3].item() - l64 * max(n64, 1)) <= 1e-4 * max(abs(l64 * max(n64, 1)), 1e-12)


def _raw_bwd(R, C, H, mode, gpu, labels, p=0.1, act=0):
    """One forward + backward on the bindings; returns (stats, dpre, dW2, db2)."""
    C_ = _hip()._C
    torch.manual_seed(5)
    pre = torch.randn(R, H, device=gpu).bfloat16()
    w2 = (torch.randn(C, H, device=gpu) * H ** -0.5).bfloat16()
    b2 = (torch.randn(C, device=gpu) * 0.5).bfloat16()
    t, logits = torch.empty_like(pre), torch.empty(R, C, device=gpu, dtype=torch.bfloat16)
    partials = torch.empty(C_.seq_head_blocks(R) * 4, device=gpu)
    stats = torch.empty(4, device=gpu)
    C_.seq_head_fwd(pre, w2, b2, labels, t, logits, partials, stats, mode, 0.5, act, p, 77)
    out = []
    for _ in range(2):
        dpre = torch.full_like(pre, NAN)  # every element must be written
        dW2, db2 = torch.zeros(C * H, device=gpu), torch.zeros(C, device=gpu)
        g = torch.empty(R * C, device=gpu)
        part = torch.empty(C_.seq_head_workspace(R, H, C), device=gpu)
        C_.seq_head_bwd(t, w2, logits, labels, stats, torch.ones(1, device=gpu), dpre, g, part, dW2, db2, mode, act,
                        p, 77)
        torch.cuda.synchronize()
        out.append((dpre, dW2, db2))
    return stats, out


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_backward_is_bit_reproducible(gpu, mode):
    R, C, H = 300, 33, 768
    ptype = (CE, BCE, MSE)[mode]
    stats, (a, b) = _raw_bwd(R, C, H, mode, gpu, _labels(ptype, R, C, gpu, ignore=7))
    for x, y, n in zip(a, b, ("dpre", "dW2", "db2")):
        assert torch.equal(x, y), n
        assert bool(torch.isfinite(x).all()), n
    assert float(a[1].abs().sum()) > 0 and float(a[2].abs().sum()) > 0
    assert torch.count_nonzero(a[0][7]) == 0  # the ignored row's dpre is exactly zero
    assert torch.count_nonzero(a[0][8]) > 0


@pytest.mark.parametrize("ptype", [CE, BCE, MSE])
def test_all_rows_ignored(gpu, ptype):
    R, C, H = 19, 6, 256
    params = _inputs(R, C, H, gpu)
    labels = _labels(ptype, R, C, gpu, ignore=slice(None))
    loss, _ = ops.cls_head(*params, labels, "tanh", 0.0, 0, 0.1, 9, problem_type=ptype)
    assert "SeqHead" in type(loss.grad_fn).__name__
    loss.backward()
    assert loss.item() == 0.0 and loss._hsd_stats[2].item() == 0 and loss._hsd_stats[1].item() == 0
    for t in params:
        assert torch.count_nonzero(t.grad) == 0 and bool(torch.isfinite(t.grad).all())


def test_dispatch(gpu, monkeypatch):
    hip = _hip()
    C_ = hip._C
    # C = 3 single-label: cls_head.hip, bit for bit what its binding returns
    R, H = 21, 256
    params = _inputs(R, 3, H, gpu, S=1)
    h, w1, b1, w2, b2 = [t.detach() for t in params]
    labels = _labels(CE, R, 3, gpu, ignore=1)
    for pt in (None, CE):
        loss, logits = ops.cls_head(h, w1, b1, w2, b2, labels, "tanh", 0.0, 0, 0.1, 9, problem_type=pt)
        pre = hip.gemm_fwd(h[:, 0], w1, hip.EPI_BIAS, bias=b1) if hip._nt_ok(R, H, H, hip.EPI_BIAS) \
            else torch.addmm(b1, h[:, 0], w1.t())
        t, lg = torch.empty_like(pre), torch.empty(R, 3, device=gpu, dtype=torch.bfloat16)
        partials, stats = torch.empty(C_.cls_head_blocks(R) * 4, device=gpu), torch.empty(4, device=gpu)
        C_.cls_head_fwd(pre, w2, b2, labels, t, lg, partials, stats, 0, 0.1, 9)
        assert torch.equal(logits, lg) and torch.equal(loss._hsd_stats, stats)
    # C = 6 single-label and both new types: the fused seq head; HSD_SEQ_HEAD=composed: the other path
    for pt, C in ((None, 6), (CE, 6), (BCE, 6), (MSE, 1), (MSE, 3), (BCE, 64)):
        params = _inputs(R, C, H, gpu)
        labels = _labels(pt or CE, R, C, gpu, ignore=2)
        monkeypatch.setattr(ops, "SEQ_HEAD_FUSED", True)
        loss, logits = ops.cls_head(*params, labels, "relu", 0.0, 0, 0.1, 9, problem_type=pt)
        assert "SeqHead" in type(loss.grad_fn).__name__ and loss._hsd_stats is not None
        monkeypatch.setattr(ops, "SEQ_HEAD_FUSED", False)
        loss2, logits2 = ops.cls_head(*params, labels, "relu", 0.0, 0, 0.1, 9, problem_type=pt)
        assert "SeqHead" not in type(loss2.grad_fn).__name__
        assert abs(loss.item() - loss2.item()) < 2e-2 * max(1.0, abs(loss2.item()))
        _close(logits, logits2, 3e-2, 3e-2, "fused vs composed logits")
        if pt is not None:
            assert loss2._hsd_stats[2].item() == R - 1
    # beyond 64 classes: composed
    monkeypatch.setattr(ops, "SEQ_HEAD_FUSED", True)
    params = _inputs(R, 65, H, gpu)
    loss, _ = ops.cls_head(*params, _labels(BCE, R, 65, gpu), "tanh", 0.0, 0, 0.0, 0, problem_type=BCE)
    assert "SeqHead" not in type(loss.grad_fn).__name__


# ------------------------------------------------------------------------------------------ model level
def _cfg(C):
    return resolve_config("hsd-tiny-bert", num_labels=C).replace(num_hidden_layers=2, hidden_size=128,
                                                                 num_attention_heads=2, intermediate_size=512)


def _batch(cfg, B, S, ptype, gpu, seed=11):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(5, cfg.vocab_size, (B, S), generator=g)
    am = torch.ones(B, S, dtype=torch.long)
    for b in range(B):
        am[b, S - (b * 3) % (S - 1):] = 0 if b % 4 else 1
    C = cfg.num_labels
    y = (torch.rand(B, C, generator=g) < 0.3).float() if ptype == BCE else torch.randn(B, C, generator=g)
    y[B - 1] = NAN  # a row that only pads an eval shard
    return {"input_ids": ids.to(gpu), "attention_mask": am.to(gpu), "labels": y.to(gpu)}


@pytest.mark.parametrize("ptype,C", [(MSE, 1), (MSE, 3), (BCE, 6)])
def test_model_step_matches_fp32_reference(gpu, monkeypatch, ptype, C):
    """A 2-layer bert, B = 8, S = 32, one Trainer step against the fp32 model on the reference ops, with the bounds of
    tests/test_gpu_cls_rows.py (loss 2e-2, gradients ``_close(5e-2, 5e-2)``)."""
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedAdam
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore
    from huggingface_sagemaker_tensorflow_distributed_amd.train.trainer import Trainer

    cfg = _cfg(C)
    base = build_model(cfg, seed=0, problem_type=ptype)
    with torch.no_grad():
        for p_ in base.parameters():
            p_.copy_(p_.bfloat16().float())  # the weights the bf16 step sees
    batch = _batch(base.cfg, 8, 32, ptype, gpu)
    m32 = copy.deepcopy(base).to(gpu)
    monkeypatch.setattr(ops, "_FORCE_TORCH", True)
    m32.train()
    m32.rng.new_step(0)
    l_ref, _ = m32(**batch)
    l_ref.backward()
    g_ref = {n: p.grad.detach().float() for n, p in m32.named_parameters()}
    monkeypatch.setattr(ops, "_FORCE_TORCH", False)
    monkeypatch.setenv("HSD_OPT_OVERLAP", "0")
    model = copy.deepcopy(base).to(gpu)
    store = FlatParamStore(model, gpu, compute_dtype=torch.bfloat16)
    tr = Trainer(model, store, FusedAdam(store, lr=1e-5), None, gpu)
    tr.zero_grad_in_optimizer = False
    loss = tr.train_step([batch]).detach().float()
    torch.cuda.synchronize()
    assert torch.allclose(loss, l_ref.detach().float(), atol=2e-2, rtol=2e-2), (loss, l_ref)
    for n, p in model.named_parameters():
        _close(p.main_grad.float().view(g_ref[n].shape), g_ref[n], 5e-2, 5e-2, n)


def test_regression_step_with_accumulation(gpu, monkeypatch):
    """One regression optimizer step over two micro-batches (dropout off): its loss is the mean of the two fp32
    reference losses (the 2e-2 of the step test above) and the weights move."""
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedAdam
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore
    from huggingface_sagemaker_tensorflow_distributed_amd.train.trainer import Trainer

    cfg = _cfg(3).replace(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    base = build_model(cfg, seed=0, problem_type=MSE)
    with torch.no_grad():
        for p_ in base.parameters():
            p_.copy_(p_.bfloat16().float())
    mbs = [_batch(base.cfg, 8, 32, MSE, gpu, seed=40 + k) for k in range(2)]
    m32 = copy.deepcopy(base).to(gpu).train()
    monkeypatch.setattr(ops, "_FORCE_TORCH", True)
    want = sum(float(m32(**mb)[0].detach()) for mb in mbs) / 2
    monkeypatch.setattr(ops, "_FORCE_TORCH", False)
    model = copy.deepcopy(base).to(gpu)
    store = FlatParamStore(model, gpu, compute_dtype=torch.bfloat16)
    tr = Trainer(model, store, FusedAdam(store, lr=1e-3), None, gpu, grad_accum=2)
    before = store.master.clone()
    loss = float(tr.train_step(mbs))
    torch.cuda.synchronize()
    assert abs(loss - want) <= 2e-2 * max(1.0, abs(want)), (loss, want)
    assert bool(torch.isfinite(store.master).all()) and not torch.equal(before, store.master)


def test_whole_step_graph_replay_matches_eager(gpu, monkeypatch):
    """--hip_graph true on a regression model: the captured whole step replays what the eager step computes
    (tests/test_gpu_graph.py's criterion: losses within 2e-3 relative, master weights within 1e-4)."""
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedAdam
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore
    from huggingface_sagemaker_tensorflow_distributed_amd.train.trainer import Trainer

    monkeypatch.setenv("HSD_GRAPH_FULL", "1")
    cfg = resolve_config("bert-base-uncased", num_labels=3).replace(num_hidden_layers=2)
    batches = [_batch(cfg, 8, 64, MSE, gpu, seed=100 + s) for s in range(3)]
    res = {}
    for replay in (False, True):
        model = build_model(cfg, seed=0, problem_type=MSE).to(gpu)
        model.rng.base_seed = 5
        store = FlatParamStore(model, gpu, compute_dtype=torch.bfloat16)
        tr = Trainer(model, store, FusedAdam(store, lr=1e-4), None, gpu, hip_graph=True)
        tr._graph_replay = replay
        losses = [float(tr.train_step([b])) for b in batches]
        if replay:
            assert tr._full_graph and len(tr._graphs) == 1
        torch.cuda.synchronize()
        res[replay] = (losses, tr.store.master.clone())
        tr._seed.close()
    (l0, w0), (l1, w1) = res[False], res[True]
    assert all(x == x and x > 0 for x in l0)
    for a, b in zip(l0, l1):
        assert abs(a - b) <= 2e-3 * max(1.0, abs(a)), (l0, l1)
    assert (w0 - w1).norm() / w0.norm() < 1e-4
