"""The fused token-classification head (csrc/kernels/token_head.hip) against the fp32 reference head with
torch.nn.functional.cross_entropy(ignore_index=-100), the model step and the whole-step graph on top of it."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from huggingface_sagemaker_tensorflow_distributed_amd import ops  # noqa: E402
from huggingface_sagemaker_tensorflow_distributed_amd.data.packing import pack_batch, position_rule  # noqa: E402
from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model, resolve_config  # noqa: E402
from huggingface_sagemaker_tensorflow_distributed_amd.ops import reference as ref  # noqa: E402
from huggingface_sagemaker_tensorflow_distributed_amd.ops.rng import keep_mask  # noqa: E402

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


def _reference(h, w, b, labels, p):
    f = [t.detach().float().requires_grad_() for t in (h, w, b)]
    lg = torch.nn.functional.linear(ref.dropout(f[0], p, SEED, True), f[1], f[2])
    loss = torch.nn.functional.cross_entropy(lg, labels, ignore_index=-100)
    loss.backward()
    return loss.detach(), lg.detach(), [t.grad for t in f]


def _raw_backward(h, w, logits, labels, stats, p, dh_fill=float("nan")):
    """The backward launch itself on fresh buffers: dh pre-filled, dW / db from zero."""
    hip = _hip()
    R, H = h.shape
    C = w.shape[0]
    dh = torch.full((R, H), dh_fill, dtype=torch.bfloat16, device=h.device)
    dW = torch.zeros(C * H, dtype=torch.float32, device=h.device)
    db = torch.zeros(C, dtype=torch.float32, device=h.device)
    part = torch.empty(hip._C.token_head_bwd_blocks(R) * (C * H + C), dtype=torch.float32, device=h.device)
    dl = torch.ones(1, dtype=torch.float32, device=h.device)
    hip._C.token_head_bwd(h.detach(), w.detach(), logits, labels, stats, dl, dh, part, dW, db, float(p),
                          hip._s64(SEED))
    return dh, dW.view(C, H), db


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("C", [2, 3, 9, 16])
@pytest.mark.parametrize("H", [64, 768, 1024])
@pytest.mark.parametrize("R", [1, 17, 255, 1000])
def test_token_head_vs_reference(gpu, R, H, C, p):
    """Forward + backward at one row, a partial tile, several blocks and a row count that is no multiple of the
    16-row tile; H below one 32-column slice per wave, bert-base's and the 1,024 limit; C at both limits, odd, and
    the headline's 9. About a quarter of the labels are -100, scattered."""
    h, w, b, labels = _inputs(gpu, R, H, C)
    loss, logits = ops.token_head(h, w, b, labels, p, SEED)
    stats = getattr(loss, "_hsd_stats", None)
    assert stats is not None and logits.dtype == torch.bfloat16 and tuple(logits.shape) == (R, C)
    loss.backward()
    loss_ref, lg_ref, g_ref = _reference(h, w, b, labels, p)
    valid = labels.ne(-100)
    print(f"R={R} H={H} C={C} p={p}: loss {loss.item():.5f} ref {loss_ref.item():.5f}")
    _close(logits, lg_ref, 3e-2, 3e-2, "logits")
    assert abs(loss.item() - loss_ref.item()) < 2e-2 * max(1.0, abs(loss_ref.item())), (loss.item(), loss_ref.item())
    for n, a, r_ in zip(["h", "w", "b"], (h.grad, w.grad, b.grad), g_ref):
        rel = (a.float() - r_).norm() / (r_.norm() + 1e-6)
        print(f"  d{n}: rel err {rel:.3g}")
        assert rel < 4e-2, f"{n}: rel err {rel:.3g}"
    assert stats[2].item() == valid.sum().item()
    lg_cpu, lab_cpu = logits.float().cpu(), labels.cpu()
    hits = int(((lg_cpu.argmax(-1) == lab_cpu) & lab_cpu.ne(-100)).sum())  # first maximum of the kernel's own logits
    assert stats[1].item() == hits
    assert abs(stats[0].item() * max(1.0, stats[2].item()) - stats[3].item()) <= 1e-5 * max(1.0, abs(stats[3].item()))
    # every element of dh is written (NaN pre-fill), ignored rows are exactly zero, and the launch on its own
    # buffers gives the bits autograd returned
    dh, dW, db = _raw_backward(h, w, logits, labels, stats, p)
    assert not torch.isnan(dh.float()).any()
    assert torch.count_nonzero(dh[~valid]) == 0
    assert torch.equal(dh, h.grad) and torch.equal(dW.to(torch.bfloat16), w.grad) and torch.equal(db.bfloat16(), b.grad)


@pytest.mark.parametrize("R,H,C", [(255, 768, 9), (16, 64, 2)])
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


def test_two_runs_give_the_same_bits(gpu):
    """More tiles than the persistent backward grid has blocks (8,192 tiles over 512 blocks): several tiles per
    block and 512 partial slabs through the reducer, twice."""
    h, w, b, labels = _inputs(gpu, 131072 + 5, 768, 9)
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


def test_element_offsets_past_2_31(gpu):
    """2,800,000 x 768 rows: the element offsets of h and dh pass 2^31 (2.15e9 elements, 4.3 GB each), so a 32-bit
    offset anywhere in the kernels shows in the last rows. p = 0 (the reference mask of 2e9 elements would take
    longer than the rest of the file); fp32 reference on the GPU from the same bf16 inputs."""
    R, H, C = 2_800_000, 768, 9
    g = torch.Generator(device=gpu).manual_seed(5)
    h = torch.randn(R, H, device=gpu, dtype=torch.bfloat16, generator=g).requires_grad_()
    w = (torch.randn(C, H, device=gpu, generator=g) * 0.05).bfloat16().requires_grad_()
    b = (torch.randn(C, device=gpu, generator=g) * 0.5).bfloat16().requires_grad_()
    labels = torch.randint(0, C, (R,), device=gpu, generator=g)
    labels[torch.rand(R, device=gpu, generator=g) < 0.25] = -100
    loss, logits = ops.token_head(h, w, b, labels, 0.0, SEED)
    loss.backward()
    with torch.no_grad():
        valid = labels.ne(-100)
        n = valid.sum()
        lg_ref = torch.addmm(b.float(), h.float(), w.float().t())
        loss_ref = torch.nn.functional.cross_entropy(lg_ref, labels, ignore_index=-100)
        gref = torch.softmax(lg_ref, -1)
        gref[valid, labels[valid]] -= 1.0
        gref = gref * valid.unsqueeze(1) / n
        tail = slice(R - 4096, R)
        assert loss._hsd_stats[2].item() == n.item()
        assert abs(loss.item() - loss_ref.item()) < 2e-2 * max(1.0, abs(loss_ref.item()))
        _close(logits[tail], lg_ref[tail], 3e-2, 3e-2, "last logits")
        _close(logits[:4096], lg_ref[:4096], 3e-2, 3e-2, "first logits")
        dh_tail = gref[tail] @ w.float()
        rel = (h.grad[tail].float() - dh_tail).norm() / dh_tail.norm()
        assert rel < 4e-2, f"dh of the last rows: rel err {rel:.3g}"
        assert torch.count_nonzero(h.grad[tail][~valid[tail]]) == 0
        dw_ref = gref.t() @ h.float()
        rel = (w.grad.float() - dw_ref).norm() / dw_ref.norm()
        assert rel < 4e-2, f"dW: rel err {rel:.3g}"
        rel = (b.grad.float() - gref.sum(0)).norm() / gref.sum(0).norm()
        assert rel < 4e-2, f"db: rel err {rel:.3g}"


def test_backward_adds_into_main_grad(gpu):
    h, w, b, labels = _inputs(gpu, 255, 768, 9)
    loss, logits = ops.token_head(h, w, b, labels, 0.1, SEED)
    loss.backward()
    _, want_w, want_b = _raw_backward(h, w, logits, labels, loss._hsd_stats, 0.1)  # fp32, from zeroed buffers
    g = torch.Generator().manual_seed(3)
    pre_w = torch.randint(-4, 5, (9, 768), generator=g).float().to(gpu)  # small integers: the sums below are exact
    pre_b = torch.randint(-4, 5, (9,), generator=g).float().to(gpu)
    w2, b2 = w.detach().clone().requires_grad_(), b.detach().clone().requires_grad_()
    w2.main_grad, b2.main_grad = pre_w.clone(), pre_b.clone()
    loss2, _ = ops.token_head(h.detach().requires_grad_(), w2, b2, labels, 0.1, SEED)
    loss2.backward()
    assert w2.grad is None and b2.grad is None  # the gradient went into main_grad
    # (prefill + g) - prefill: one fp32 rounding at magnitude <= 8, i.e. at most 2^-21 = 4.8e-7 off g
    torch.testing.assert_close((w2.main_grad - pre_w), want_w, atol=1e-6, rtol=0)
    torch.testing.assert_close((b2.main_grad - pre_b), want_b, atol=1e-6, rtol=0)
    assert want_w.abs().max() > 1e-3
    assert not torch.equal(w2.main_grad, pre_w)
    # no input gradient asked for: parameter gradients only, the same ones
    w3, b3 = w.detach().clone().requires_grad_(), b.detach().clone().requires_grad_()
    loss3, _ = ops.token_head(h.detach(), w3, b3, labels, 0.1, SEED)
    loss3.backward()
    assert torch.equal(w3.grad, w.grad) and torch.equal(b3.grad, b.grad)


@pytest.mark.parametrize("R,H,p", [(255, 768, 0.5), (37, 1024, 0.1), (64, 72, 0.5)])
def test_dropout_mask_is_keep_mask_of_the_flat_buffer(gpu, R, H, p):
    """dh = (g·W)·keep/(1-p): on scored rows dh is zero exactly where the element was dropped. Forward: with
    W = the first C unit vectors, b = 0 and h = 1, logits[r][c] = keep[r][c]/(1-p)."""
    C = 16
    h, w, b, labels = _inputs(gpu, R, H, C, ignore=0.0)
    loss, logits = ops.token_head(h, w, b, labels, p, SEED)
    loss.backward()
    keep = keep_mask(SEED, (R, H), p, device=gpu)
    assert torch.equal(h.grad != 0, keep)
    ones = torch.ones(R, H, device=gpu, dtype=torch.bfloat16)
    eye = torch.eye(C, H, device=gpu, dtype=torch.bfloat16)
    lg = ops.token_head(ones, eye, torch.zeros(C, device=gpu, dtype=torch.bfloat16), None, p, SEED)
    assert torch.equal(lg != 0, keep[:, :C])
    assert torch.equal(lg[keep[:, :C]].float().unique(), torch.tensor([1.0 / (1.0 - p)], device=gpu).bfloat16().float())


def test_fused_path_runs_and_unsupported_shapes_fall_back(gpu, monkeypatch):
    hip = _hip()
    calls = []
    real = hip.token_head
    monkeypatch.setattr(hip, "token_head", lambda *a: (calls.append(a[0].shape), real(*a))[1])
    for R, H, C, fused in [(64, 768, 9, True), (64, 768, 17, False), (64, 1032, 9, False), (64, 768, 1, False)]:
        h, w, b, labels = _inputs(gpu, R, H, C)
        assert hip.token_head_ok(h, w) == fused
        n0 = len(calls)
        loss, logits = ops.token_head(h, w, b, labels, 0.1, SEED)
        loss.backward()
        assert (len(calls) == n0 + 1) == fused
        assert getattr(loss, "_hsd_stats", None) is not None
        loss_ref, lg_ref, g_ref = _reference(h, w, b, labels, 0.1)
        _close(logits, lg_ref, 3e-2, 3e-2, f"logits C={C} H={H}")
        assert abs(loss.item() - loss_ref.item()) < 2e-2 * max(1.0, abs(loss_ref.item()))
        rel = (h.grad.float() - g_ref[0]).norm() / (g_ref[0].norm() + 1e-6)
        assert rel < 4e-2, (C, H, float(rel))
    # fp32 GPU tensors and the composed knob take the composed ops too
    h, w, b, labels = _inputs(gpu, 64, 768, 9)
    n0 = len(calls)
    ops.token_head(h.detach().float(), w.detach().float(), b.detach().float(), labels, 0.1, SEED)
    monkeypatch.setattr(ops, "TOKEN_HEAD_FUSED", False)
    ops.token_head(h, w, b, labels, 0.1, SEED)
    assert len(calls) == n0


# ------------------------------------------------------------------------------------------ model step
def _batch(cfg, B, S, seed=0):
    g = np.random.default_rng(seed)
    lengths = np.array([S, S * 5 // 8, S // 4 + 1, 2] * (B // 4))
    ids = g.integers(5, cfg.vocab_size, size=(B, S)).astype(np.int64)
    mask = (np.arange(S)[None, :] < lengths[:, None]).astype(np.int64)
    ids[mask == 0] = cfg.pad_token_id
    labels = g.integers(0, cfg.num_labels, size=(B, S)).astype(np.int64)
    labels[g.random((B, S)) < 0.25] = -100
    labels[:, 0] = -100
    labels[mask == 0] = -100
    return ids, mask, labels


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
@pytest.mark.parametrize("name", ["hsd-tiny-bert", "hsd-tiny-roberta"])
def test_model_step_vs_fp32_reference_model(gpu, name, packed):
    """2 layers, B = 4, S = 128, bf16 with dropout on (the hash masks are shared), padded and packed, against the same
    weights in fp32 on the reference ops, at tests/test_gpu_e2e.py's tolerances."""
    cfg = resolve_config(name, num_labels=9).replace(hidden_size=128, num_attention_heads=2, intermediate_size=256)
    m32 = build_model(cfg, task=TASK, seed=0).to(gpu)
    m16 = copy.deepcopy(m32).bfloat16()
    with torch.no_grad():  # the reference holds the bf16-rounded weights
        for p32, p16 in zip(m32.parameters(), m16.parameters()):
            p32.copy_(p16.float())
    ids, mask, labels = _batch(cfg, 4, 128)
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
    assert torch.allclose(lg1.reshape(-1, 9)[real], lg2.reshape(-1, 9)[real], atol=5e-2, rtol=5e-2)
    for n in g1:
        rel = (g1[n] - g2[n]).norm() / (g2[n].norm() + 1e-6)
        assert rel < 5e-2, f"{n}: rel grad err {rel:.3g}"


# ------------------------------------------------------------------------------------------ whole-step graph
def _trainer(gpu, graph_replay):
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedAdam
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore
    from huggingface_sagemaker_tensorflow_distributed_amd.train.trainer import Trainer

    cfg = resolve_config("bert-base-uncased", num_labels=9).replace(num_hidden_layers=2)
    model = build_model(cfg, task=TASK, seed=0).to(gpu)
    model.rng.base_seed = 5
    store = FlatParamStore(model, gpu, compute_dtype=torch.bfloat16)
    opt = FusedAdam(store, lr=1e-4, weight_decay=0.01)
    tr = Trainer(model, store, opt, None, gpu, hip_graph=True, lr_schedule="linear", lr_warmup_steps=2)
    tr._graph_replay = graph_replay
    return tr


def test_whole_step_graph_replay_matches_eager(gpu, monkeypatch):
    """Three optimizer steps of a 2-layer bert-base (B = 16, S = 128, per-token labels) captured and replayed as
    one graph each, against the same steps run eagerly with the same seeds (tests/test_gpu_graph.py's bounds)."""
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
    assert len({round(x, 6) for x in l1}) == 3  # the head's dropout mask moves with the step
