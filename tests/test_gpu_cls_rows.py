"""The last encoder layer on the first-token rows only (ops/hip.py _AttnBlockCls), GPU tier.

The one-query attention kernels (csrc/kernels/attention_cls.hip) are checked against the fp32 torch reference
attention restricted to query 0, never only against other HIP kernels; the dropout row multiplier against
ops/rng.py; the model-level step of BOTH paths against the fp32 reference model. Tolerances are the ones
tests/test_gpu_ops.py uses for attention (2e-2 forward, 3e-2 gradients under its ``_close`` rule) and
tests/test_gpu_e2e.py uses for its HIP-vs-reference step (2e-2 loss, 5e-2 gradients)."""
import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from huggingface_sagemaker_tensorflow_distributed_amd import ops  # noqa: E402
from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model, resolve_config  # noqa: E402
from huggingface_sagemaker_tensorflow_distributed_amd.ops import reference as ref  # noqa: E402
from huggingface_sagemaker_tensorflow_distributed_amd.ops.rng import keep_mask  # noqa: E402

LOG2E = 1.4426950408889634


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


def _attention_mask(kind, B, S, gpu):
    if kind == "none":
        return None
    am = torch.ones(B, S, dtype=torch.long, device=gpu)
    if kind == "ragged":
        for b in range(B):
            am[b, max(1, S - (b * S) // (B + 1) - S // 3):] = 0
    elif kind == "first_key":
        am[0, 1:] = 0
    elif kind == "all_masked":
        am[B - 1, :] = 0
    return am


# ------------------------------------------------------------------------------------------ attention kernels
@pytest.mark.parametrize("kind", ["none", "ragged", "first_key", "all_masked"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B,heads", [(1, 1), (3, 2), (5, 12)])
@pytest.mark.parametrize("S", [2, 64, 128, 130, 512, 1024])
def test_attention_cls_kernels(gpu, S, B, heads, p, kind):
    hip = _hip()
    C = hip._C
    torch.manual_seed(S + 7 * B)
    H, seed = heads * 64, 777
    qkv = torch.randn(B * S, 3 * H, device=gpu, dtype=torch.bfloat16)
    am = _attention_mask(kind, B, S, gpu)
    mb = ref.key_mask_bias(am) if am is not None else None
    out = torch.empty(B, H, device=gpu, dtype=torch.bfloat16)
    lse = torch.empty(B * heads, device=gpu, dtype=torch.float32)
    C.attn_cls_fwd(qkv, mb, out, lse, B, S, heads, p, seed)

    # fp32 torch reference, query 0 only
    q32 = qkv.detach().float().requires_grad_()
    r = ref.attention_cls(q32, mb, B, S, heads, p, seed, p > 0)
    _close(out, r, 2e-2, 2e-2, "fwd")
    x = q32.detach().view(B, S, 3, heads, 64)
    s = torch.einsum("bhd,bshd->bhs", x[:, 0, 0], x[:, :, 1]) / math.sqrt(64.0)
    if mb is not None:
        s = s + mb.view(B, 1, S)
    lse_ref = torch.logsumexp(s, dim=-1) * LOG2E  # [B, heads]
    lse_k = lse.view(B, heads)
    dead = (am.sum(1) == 0) if am is not None else torch.zeros(B, dtype=torch.bool, device=gpu)
    # a sequence with every key masked saves the clamp (common.h all_masked_scale); the others their log2-sum-exp
    assert bool((lse_k[dead] <= -1e30).all())
    if bool((~dead).any()):
        _close(lse_k[~dead], lse_ref[~dead], 2e-2, 2e-2, "lse2")

    d = torch.randn(B, H, device=gpu, dtype=torch.bfloat16)
    dqkv = torch.full_like(qkv, float("nan"))  # every element must be written
    dbias = torch.zeros(3 * H, device=gpu, dtype=torch.float32)
    C.attn_cls_bwd(qkv, mb, d, lse, dqkv, B, S, heads, p, seed, dbias)
    r.backward(d.float())
    g, gr = dqkv.float().view(B, S, 3 * H), q32.grad.view(B, S, 3 * H)
    _close(g[:, 0, :H], gr[:, 0, :H], 3e-2, 3e-2, "dq row 0")
    _close(g[:, :, H:2 * H], gr[:, :, H:2 * H], 3e-2, 3e-2, "dk")
    _close(g[:, :, 2 * H:], gr[:, :, 2 * H:], 3e-2, 3e-2, "dv")
    assert torch.count_nonzero(dqkv.view(B, S, 3 * H)[:, 1:, :H]) == 0  # every other dQ row exactly zero
    _close(dbias, gr.sum((0, 1)), 3e-2, 3e-2, "dbias")

    # two runs give the same bits
    out2, lse2, dqkv2 = torch.empty_like(out), torch.empty_like(lse), torch.empty_like(dqkv)
    C.attn_cls_fwd(qkv, mb, out2, lse2, B, S, heads, p, seed)
    C.attn_cls_bwd(qkv, mb, d, lse, dqkv2, B, S, heads, p, seed, None)
    assert torch.equal(out, out2) and torch.equal(lse, lse2) and torch.equal(dqkv, dqkv2)

    # on the first-token rows it agrees with the full kernels fed a dout that is zero off those rows
    qf = qkv.detach().clone().requires_grad_()
    full = hip.attention(qf, mb, B, S, heads, p, seed)
    _close(out, full.view(B, S, H)[:, 0], 2e-2, 2e-2, "fwd vs full kernel")
    dfull = torch.zeros(B, S, H, device=gpu, dtype=torch.bfloat16)
    dfull[:, 0] = d
    full.backward(dfull.view(B * S, H))
    gf = qf.grad.float().view(B, S, 3 * H)
    # one tensor (dQ row 0, dK, dV), so the tolerance's scale is the gradient's: where a part is exactly zero in
    # exact arithmetic (dQ and dK of a sequence that sees one key) the full kernels leave bf16 rounding noise of
    # dP - delta, this kernel and the fp32 reference give 0, and a scale taken from that part alone would be noise
    both = lambda t: torch.cat([t[:, 0, :H].reshape(-1), t[:, :, H:].reshape(-1)])  # noqa: E731
    _close(both(g), both(gf), 3e-2, 3e-2, "dq row 0 / dk / dv vs full kernel")

    if p > 0 and kind == "none":
        # the kept keys, bit for bit: dV_j = Pd_j dO is exactly zero for a dropped key and, with dO = 1 and no key
        # masked (P_j > 0), non-zero for a kept one; element (b, head, 0, j) is row (b heads + head) S of the site
        ones = torch.ones_like(d)
        C.attn_cls_bwd(qkv, None, ones, lse, dqkv2, B, S, heads, p, seed, None)
        kept = dqkv2.view(B, S, 3, heads, 64)[:, :, 2].float().abs().sum(-1).permute(0, 2, 1) != 0  # [B, heads, S]
        want = keep_mask(seed, (B * heads, S), p, device=gpu, row_mul=S).view(B, heads, S)
        assert torch.equal(kept, want)
        assert torch.equal(want, keep_mask(seed, (B * heads * S, S), p, device=gpu)[::S].view(B, heads, S))


# ------------------------------------------------------------------------------------------ row multiplier
@pytest.mark.parametrize("K", [64, 768])
@pytest.mark.parametrize("N", [128, 768])
@pytest.mark.parametrize("S", [2, 128])
def test_gemm_dropout_epilogue_row_multiplier(gpu, S, N, K):
    hip = _hip()
    torch.manual_seed(1)
    M, p, seed = 64, 0.1, 4242
    x = torch.randn(M, K, device=gpu, dtype=torch.bfloat16)
    w = (torch.randn(N, K, device=gpu) * 0.05).bfloat16()
    # |x wT + b| stays well above zero, so a kept element never equals its residual
    b = torch.full((N,), 4.0, device=gpu).bfloat16()
    big = torch.randn(M, S * N, device=gpu, dtype=torch.bfloat16)
    aux = big[:, :N]  # rows read in place, row stride S * N (the first-token view of a [M * S, N] activation)
    out = hip.gemm_fwd(x, w, hip.EPI_BIAS_DROP_RES, bias=b, aux=aux, p=p, seed=seed, row_mul=S)
    keep = keep_mask(seed, (M, N), p, device=gpu, row_mul=S)
    assert torch.equal(keep, keep_mask(seed, (M * S, N), p, device=gpu)[::S])
    assert torch.equal(out != aux, keep)
    want = ref.linear_dropout_residual(x.float(), w.float(), b.float(), aux.float(), p, seed, True, row_mul=S)
    _close(out, want, 3e-2, 2e-2, "values")
    # row_mul = 1 reproduces the call without the argument, bit for bit
    o1 = hip.gemm_fwd(x, w, hip.EPI_BIAS_DROP_RES, bias=b, aux=aux, p=p, seed=seed, row_mul=1)
    o0 = hip.gemm_fwd(x, w, hip.EPI_BIAS_DROP_RES, bias=b, aux=aux, p=p, seed=seed)
    assert torch.equal(o1, o0)
    if S > 1:
        assert not torch.equal(o1, out)


@pytest.mark.parametrize("H", [128, 768])
@pytest.mark.parametrize("S", [2, 128])
def test_ln_bwd_and_dropout_row_multiplier(gpu, S, H):
    C = _hip()._C
    torch.manual_seed(2)
    M, p, seed = 64, 0.1, 99
    z = torch.randn(M, H, device=gpu, dtype=torch.bfloat16)
    dout = torch.randn(M, H, device=gpu, dtype=torch.bfloat16)
    gamma = (1 + 0.1 * torch.randn(H, device=gpu)).bfloat16()
    mean = z.float().mean(1)
    rstd = torch.rsqrt(z.float().var(1, unbiased=False) + 1e-12)

    def run(*extra):
        dz, dy = torch.empty_like(z), torch.empty_like(z)
        acc = [torch.zeros(H, device=gpu) for _ in range(3)]
        C.ln_bwd(dout, z, mean, rstd, gamma, dz, dy, None, acc[0], acc[1], acc[2], p, seed, *extra)
        return dz, dy, acc

    dz, dy, acc = run(S)
    keep = keep_mask(seed, (M, H), p, device=gpu, row_mul=S)
    live = dz != 0
    assert torch.equal((dy != 0) & live, keep & live)
    _close(dy, dz.float() * keep / (1 - p), 1e-2, 1e-2, "dy")
    # fp32 reference of the LayerNorm backward for dz
    z32 = z.float().requires_grad_()
    y = torch.nn.functional.layer_norm(z32, (H,), gamma.float(), torch.zeros(H, device=gpu), 1e-12)
    y.backward(dout.float())
    _close(dz, z32.grad, 3e-2, 2e-2, "dz")
    _close(acc[2], (dy.float()).sum(0), 1e-2, 1e-2, "dbias")
    a, b = run(1), run()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])

    x = torch.ones(M, H, device=gpu, dtype=torch.bfloat16)
    o = torch.empty_like(x)
    C.dropout(x, o, p, seed, S)
    assert torch.equal(o != 0, keep)
    _close(o, keep.float() / (1 - p), 1e-2, 1e-2, "dropout values")
    o1, o0 = torch.empty_like(x), torch.empty_like(x)
    C.dropout(x, o1, p, seed, 1)
    C.dropout(x, o0, p, seed)
    assert torch.equal(o1, o0) and torch.equal(o0 != 0, keep_mask(seed, (M, H), p, device=gpu))


@pytest.mark.parametrize("H", [64, 768])
@pytest.mark.parametrize("S", [2, 128])
@pytest.mark.parametrize("B", [1, 64])
def test_add_rows_strided_is_exact_and_touches_no_other_row(gpu, B, S, H):
    C = _hip()._C
    torch.manual_seed(3)
    dst = torch.randn(B * S, H, device=gpu, dtype=torch.bfloat16)
    src = torch.randn(B, H, device=gpu, dtype=torch.bfloat16)
    want = dst.clone()
    want[::S] = (dst[::S].float() + src.float()).bfloat16()
    C.add_rows_strided(dst, src, S)
    assert torch.equal(dst, want)


# ------------------------------------------------------------------------------------------ model level
def _cfg(name, layers):
    return resolve_config(name).replace(num_hidden_layers=layers, hidden_size=128, num_attention_heads=2,
                                        intermediate_size=512)


def _batch(cfg, B, S, padded, gpu, labels=True):
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(5, cfg.vocab_size, (B, S), generator=g)
    am = torch.ones(B, S, dtype=torch.long)
    if padded:
        for b in range(B):
            am[b, S - (b * 3) % (S - 1):] = 0 if b % 4 else 1
    out = {"input_ids": ids.to(gpu), "attention_mask": am.to(gpu)}
    if labels:
        out["labels"] = torch.randint(0, 2, (B,), generator=g).to(gpu)
    return out


def _reference_step(model32, batch):
    """Loss and gradients of the fp32 model on the torch reference ops, seeds of the Trainer's first step."""
    old = ops._FORCE_TORCH
    ops._FORCE_TORCH = True
    try:
        model32.train()
        model32.zero_grad(set_to_none=True)
        model32.rng.new_step(0)
        loss, _ = model32(**batch)
        loss.backward()
        return loss.detach().float(), {n: p.grad.detach().float() for n, p in model32.named_parameters()}
    finally:
        ops._FORCE_TORCH = old


def _trainer_step(model, batch, gpu, monkeypatch, pruned):
    """One Trainer step; the fp32 main_grad of every parameter (the optimizer neither overlaps nor clears them)."""
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedAdam
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore
    from huggingface_sagemaker_tensorflow_distributed_amd.train.trainer import Trainer

    monkeypatch.setenv("HSD_OPT_OVERLAP", "0")
    monkeypatch.setattr(ops, "CLS_ROWS_ONLY", pruned)
    store = FlatParamStore(model, gpu, compute_dtype=torch.bfloat16)
    tr = Trainer(model, store, FusedAdam(store, lr=1e-5), None, gpu)
    tr.zero_grad_in_optimizer = False
    shapes = []
    hook = model.encoder.register_forward_hook(lambda m, a, o: shapes.append(tuple(o.shape)))
    loss = tr.train_step([batch]).detach().float()
    hook.remove()
    torch.cuda.synchronize()
    B, S = batch["input_ids"].shape
    assert shapes == [(B, 1 if pruned else S, model.cfg.hidden_size)]
    return loss, {n: p.main_grad.detach().float().clone() for n, p in model.named_parameters()}


def _check_both_paths(name, layers, B, S, padded, gpu, monkeypatch):
    cfg = _cfg(name, layers)
    base = build_model(cfg, seed=0)
    with torch.no_grad():
        for p_ in base.parameters():
            p_.copy_(p_.bfloat16().float())  # the weights the bf16 step sees
    batch = _batch(cfg, B, S, padded, gpu)
    l_ref, g_ref = _reference_step(copy.deepcopy(base).to(gpu), batch)
    for pruned in (True, False):
        loss, grads = _trainer_step(copy.deepcopy(base).to(gpu), batch, gpu, monkeypatch, pruned)
        what = "pruned" if pruned else "full"
        assert torch.allclose(loss, l_ref, atol=2e-2, rtol=2e-2), (what, loss, l_ref)
        assert set(grads) == set(g_ref)
        for n in grads:
            _close(grads[n].view(g_ref[n].shape), g_ref[n], 5e-2, 5e-2, f"{what} {n}")


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("S", [64, 128])
def test_trainer_step_of_both_paths_matches_fp32_reference(gpu, monkeypatch, S, padded):
    _check_both_paths("hsd-tiny-bert", 2, 64, S, padded, gpu, monkeypatch)


def test_one_layer_model_matches_fp32_reference(gpu, monkeypatch):
    # layer 0 is then the last layer and the embeddings still need dh
    _check_both_paths("hsd-tiny-bert", 1, 64, 64, True, gpu, monkeypatch)


def test_batch_under_one_k_tile_matches_fp32_reference(gpu, monkeypatch):
    # B = 8 first-token rows: the B-row weight gradients run on the small-T kernel (ops/hip.py wgrad_done)
    _check_both_paths("hsd-tiny-bert", 2, 8, 64, True, gpu, monkeypatch)


def test_roberta_head_input_dropout_matches_fp32_reference(gpu, monkeypatch):
    _check_both_paths("hsd-tiny-roberta", 2, 64, 64, True, gpu, monkeypatch)


def test_eval_without_labels(gpu, monkeypatch):
    cfg = _cfg("hsd-tiny-bert", 2)
    base = build_model(cfg, seed=0)
    batch = _batch(cfg, 64, 64, True, gpu, labels=False)
    m32 = copy.deepcopy(base).to(gpu).eval()
    monkeypatch.setattr(ops, "_FORCE_TORCH", True)
    with torch.no_grad():
        want = m32(**batch).float()
    monkeypatch.setattr(ops, "_FORCE_TORCH", False)
    m = copy.deepcopy(base).to(gpu).bfloat16().eval()
    for pruned in (True, False):
        monkeypatch.setattr(ops, "CLS_ROWS_ONLY", pruned)
        with torch.no_grad():
            h = m.encoder(batch["input_ids"], batch["attention_mask"], None, m.rng, False, first_token_only=True)
            got = m(**batch).float()
        assert h.shape[1] == (1 if pruned else 64)
        assert torch.allclose(got, want, atol=5e-2, rtol=5e-2), (pruned, (got - want).abs().max())


def test_fp8_and_packed_batches_keep_the_full_last_layer(gpu, monkeypatch):
    from huggingface_sagemaker_tensorflow_distributed_amd.data.packing import pack_batch, position_rule

    monkeypatch.setattr(ops, "CLS_ROWS_ONLY", True)
    cfg = _cfg("hsd-tiny-bert", 2)
    m = build_model(cfg, seed=0).to(gpu).bfloat16().eval()
    batch = _batch(cfg, 8, 64, True, gpu, labels=False)
    args = (batch["input_ids"], batch["attention_mask"], None, m.rng, False)
    with torch.no_grad():
        assert m.encoder(*args, first_token_only=True).shape == (8, 1, 128)
        ops.set_fp8(True)
        try:
            assert m.encoder(*args, first_token_only=True).shape == (8, 64, 128)
        finally:
            ops.set_fp8(False)
        pk = pack_batch(batch["input_ids"].cpu().numpy(), batch["attention_mask"].cpu().numpy(), None,
                        **position_rule(cfg))
        t = lambda a: torch.as_tensor(a).to(gpu)  # noqa: E731
        h = m.encoder(t(pk["input_ids"]), None, None, m.rng, False, cu_seqlens=t(pk["cu_seqlens"]),
                      max_seqlen=pk["max_seqlen"], position_ids=t(pk["position_ids"]), first_token_only=True)
        assert h.dim() == 2 and h.shape[0] == t(pk["input_ids"]).shape[1]


# ------------------------------------------------------------------------------------------ whole-step graph
def test_whole_step_graph_matches_eager_on_the_pruned_path(gpu, monkeypatch):
    """B = 8, S = 128 with ``hip_graph``: the captured whole step replays what the eager step computes, the way
    tests/test_gpu_graph.py checks it (same seeding in both, so only capture / replay differs)."""
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedAdam
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore
    from huggingface_sagemaker_tensorflow_distributed_amd.train.trainer import Trainer

    monkeypatch.setenv("HSD_GRAPH_FULL", "1")
    monkeypatch.setattr(ops, "CLS_ROWS_ONLY", True)
    cfg = resolve_config("bert-base-uncased").replace(num_hidden_layers=2)
    g = torch.Generator().manual_seed(0)
    batches = []
    for _ in range(3):
        am = torch.ones(8, 128, dtype=torch.long)
        am[3, 70:] = 0
        batches.append({"input_ids": torch.randint(1000, 30000, (8, 128), generator=g).to(gpu),
                        "attention_mask": am.to(gpu), "labels": torch.randint(0, 2, (8,), generator=g).to(gpu)})
    res = {}
    for replay in (False, True):
        model = build_model(cfg, seed=0).to(gpu)
        model.rng.base_seed = 5
        store = FlatParamStore(model, gpu, compute_dtype=torch.bfloat16)
        tr = Trainer(model, store, FusedAdam(store, lr=1e-4), None, gpu, hip_graph=True)
        tr._graph_replay = replay
        shapes = []
        hook = model.encoder.register_forward_hook(lambda m, a, o: shapes.append(tuple(o.shape)))
        losses = [float(tr.train_step([b])) for b in batches]
        hook.remove()
        if replay:
            assert tr._full_graph and len(tr._graphs) == 1
        assert shapes and all(s == (8, 1, cfg.hidden_size) for s in shapes)
        torch.cuda.synchronize()
        res[replay] = (losses, tr.store.master.clone())
        tr._seed.close()
    (l0, w0), (l1, w1) = res[False], res[True]
    for a, b in zip(l0, l1):
        assert abs(a - b) <= 2e-3 * max(1.0, abs(a)), (l0, l1)
    assert (w0 - w1).norm() / w0.norm() < 1e-4
