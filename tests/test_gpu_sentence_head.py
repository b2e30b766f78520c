"""The sentence-embedding head (csrc/kernels/sent_head.hip): pooling and the streamed contrastive loss against fp64 torch
(ops/reference.py on double copies of the same inputs), bit equality, and the model step against the fp32 reference model.

The yardstick for the fp32 outputs is the fp32 reference op's own error against fp64 on the same inputs (run on the
CPU): the kernel may be off by at most twice that, per case, max over the entries; every measured pair is printed
(profiles/sent_head/error_pairs.log)."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from huggingface_sagemaker_tensorflow_distributed_amd import ops  # noqa: E402
from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model, resolve_config  # noqa: E402
from huggingface_sagemaker_tensorflow_distributed_amd.ops import reference as ref  # noqa: E402

LENGTHS = [0, 1, 2, 127, 128, 129, 300]  # the pooling chunk is 128 rows
SCALE = 20.0


def _hip():
    from huggingface_sagemaker_tensorflow_distributed_amd.ops import hip

    return hip


def _within_twice(what, got, want64, yard):
    err, bound = (got.double().cpu() - want64).abs().max().item(), (yard.double() - want64).abs().max().item()
    print(f"{what}: kernel max err {err:.3e}, fp32 reference max err {bound:.3e}, max |ref| {want64.abs().max().item():.3e}")
    assert err <= 2.0 * bound, f"{what}: {err:.3e} > 2 x {bound:.3e}"


def _pool_inputs(H, packed, seed=5):
    """Packed: the lengths back to back and 5 dead rows. Padded: S = 300 with those real lengths and a hole in the mask
    at position 1 of every sequence of 3 or more rows."""
    g = torch.Generator().manual_seed(seed + H)
    n = len(LENGTHS)
    if packed:
        cu = torch.tensor(np.concatenate([[0], np.cumsum(LENGTHS)]), dtype=torch.int32)
        R, mask = int(cu[-1]) + 5, None
        live = torch.arange(R) < int(cu[-1])
    else:
        S = max(LENGTHS)
        cu = torch.arange(n + 1, dtype=torch.int32) * S
        mask = (torch.arange(S)[None, :] < torch.tensor(LENGTHS)[:, None]).long()
        mask[torch.tensor(LENGTHS) >= 3, 1] = 0
        mask = mask.reshape(-1)
        R, live = n * S, mask.bool()
    return torch.randn(R, H, generator=g).bfloat16(), torch.randn(n, H, generator=g), cu, mask, live


def _pool_reference(h, de, cu, mask, dtype):
    x = h.to(dtype).requires_grad_()
    e = ref.pool_normalize(x, cu, mask)
    e.backward(de.to(e.dtype))
    return e.detach(), x.grad


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("H", [64, 768, 1024])
def test_pooling_vs_fp64(gpu, H, packed):
    h, de, cu, mask, live = _pool_inputs(H, packed)
    e64, dh64 = _pool_reference(h, de, cu, mask, torch.float64)
    e32, dh32 = _pool_reference(h, de, cu, mask, torch.float32)
    hg, cug = h.to(gpu).requires_grad_(), cu.to(gpu)
    mg = None if mask is None else mask.to(gpu)
    e = ops.pool_normalize(hg, cug, mg, max_seqlen=max(LENGTHS))
    assert e.dtype == torch.float32 and tuple(e.shape) == (len(LENGTHS), H)
    e.backward(de.to(gpu))
    _within_twice(f"pool e H={H} packed={packed}", e.detach(), e64, e32)
    assert torch.count_nonzero(e[0]) == 0  # the empty sequence
    dh = hg.grad.float().cpu().double()
    floor = (dh32.double() - dh64).abs().max().item()
    excess = ((dh - dh64).abs() - 2.0 ** -8 * dh64.abs()).max().item()
    print(f"pool dh H={H} packed={packed}: max excess over one bf16 rounding {excess:.3e}, fp32 reference err {floor:.3e}")
    assert excess <= floor
    # the raw launch on a NaN-filled buffer: every row written, masked and dead rows exactly zero, autograd's bits
    hip = _hip()
    raw = torch.full_like(hg.detach(), float("nan"))
    hip._C.sent_pool_bwd(de.to(gpu), *_saved(hip, hg, cug, mg), raw, max(LENGTHS))
    assert torch.equal(raw, hg.grad) and torch.count_nonzero(raw[~live.to(gpu)]) == 0
    assert torch.count_nonzero(raw[live.to(gpu)]) > 0


@pytest.mark.parametrize("hint", [128, 200])
def test_rows_past_an_understated_longest_sequence_take_no_part(gpu, hint):
    """max_seqlen below the longest sequence (300 rows): the bits of a row mask over the rows past the 1 or 2 chunks."""
    g = torch.Generator().manual_seed(11)
    h, de = torch.randn(305, 64, generator=g).to(gpu).bfloat16(), torch.randn(2, 64, generator=g).to(gpu)
    cu = torch.tensor([0, 300, 305], dtype=torch.int32, device=gpu)
    mask = torch.ones(305, dtype=torch.long, device=gpu)
    mask[-(-hint // 128) * 128:300] = 0
    out = []
    for m, longest in ((None, hint), (mask, 300)):
        x = h.clone().requires_grad_()
        e = ops.pool_normalize(x, cu, m, max_seqlen=longest)
        e.backward(de)
        out.append((e.detach(), x.grad))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert torch.count_nonzero(out[0][1][:128]) > 0


def _saved(hip, hg, cug, mg):
    """(e, aux, cu, mask) of a raw forward launch, in sent_pool_bwd's order after de."""
    n, H = cug.numel() - 1, hg.shape[1]
    ch = hip._C.sent_pool_chunks(max(LENGTHS))
    e = torch.empty((n, H), dtype=torch.float32, device=hg.device)
    aux = torch.empty((n, 2), dtype=torch.float32, device=hg.device)
    ws = torch.empty(n * ch * H, dtype=torch.float32, device=hg.device)
    wsc = torch.empty(n * ch, dtype=torch.int32, device=hg.device)
    hip._C.sent_pool_fwd(hg.detach(), cug, mg, e, aux, ws, wsc, max(LENGTHS))
    return e, aux, cug, mg


def _score_inputs(B, H, invalid, seed=9):
    """Noisy positives (cos 0.45), every fifth resembling the next anchor: loss O(1), hits strictly between 0 and n_valid
    (B > 1). Pairs 2 and 32 copy pairs 1 and 31: exact ties, one across the 32-row seam, for the first argmax."""
    g = torch.Generator().manual_seed(seed + B + H)
    a = torch.randn(B, H, generator=g)
    src = torch.arange(B)
    src[4::5] = (src[4::5] + 1) % B
    p = a[src] + 2.0 * torch.randn(B, H, generator=g)
    for j, k in ((1, 2), (31, 32)):
        if k < B:
            a[k], p[k] = a[j], p[j]
    e = torch.nn.functional.normalize(torch.stack([a, p], dim=1).reshape(2 * B, H), dim=1)
    valid = torch.ones(B, dtype=torch.int32)
    if invalid:
        valid[::3] = 0
    return e, valid


def _score_reference(e, valid, dtype):
    x = e.clone().to(dtype).requires_grad_()
    loss, stats = ref.contrastive_loss(x, valid, SCALE)
    loss.backward()
    return loss.detach().reshape(1), stats, x.grad


@pytest.mark.parametrize("invalid", [False, True])
@pytest.mark.parametrize("H", [64, 768])
@pytest.mark.parametrize("B", [1, 3, 33, 65, 130])
def test_scores_vs_fp64(gpu, B, H, invalid):
    """Loss and de within twice the fp32 reference's error, hits and counts equal, zero rows exact; B = 1: exact zeros."""
    e, valid = _score_inputs(B, H, invalid)
    l64, s64, de64 = _score_reference(e, valid, torch.float64)
    l32, _, de32 = _score_reference(e, valid, torch.float32)
    eg = e.clone().to(gpu).requires_grad_()
    loss = ops.contrastive_loss(eg, valid.to(gpu), SCALE)
    loss.backward()
    what = f"B={B} H={H} invalid={invalid}"
    _within_twice(f"score loss {what}", loss.detach().reshape(1), l64, l32)
    _within_twice(f"score de {what}", eg.grad, de64, de32)
    assert loss._hsd_stats[1:3].tolist() == s64[1:3].tolist() and loss._hsd_correct.item() == s64[1].item()
    assert torch.count_nonzero(eg.grad.view(B, 2, H)[valid.to(gpu) == 0]) == 0
    if B == 1 and not invalid:
        assert loss.item() == 0.0 and torch.count_nonzero(eg.grad) == 0
    if invalid:  # every pair invalid: loss 0, zero gradients
        eg.grad = None
        loss = ops.contrastive_loss(eg, torch.zeros(B, dtype=torch.int32, device=gpu), SCALE)
        loss.backward()
        assert loss.item() == 0.0 and loss._hsd_stats.tolist() == [0.0] * 4 and torch.count_nonzero(eg.grad) == 0


def _head_step(h, cu, mask, valid, S):
    x = h.detach().requires_grad_()
    loss, e = ops.sentence_head(x, cu, mask, valid, SCALE, max_seqlen=S)
    loss.backward()
    return loss.detach().clone(), e.detach().clone(), loss._hsd_stats.clone(), x.grad.clone()


def test_two_runs_and_both_layouts_give_the_same_bits(gpu):
    """n = 70 full-length sequences of 130 rows (two pooling chunks, two score tiles, H = 768: 6 fragment chunks and 3
    gradient slabs): every kernel twice, and padded (mask of ones) against packed (no mask)."""
    g = torch.Generator().manual_seed(3)
    B, S, H = 35, 130, 768
    h = torch.randn(2 * B * S, H, generator=g).to(gpu).bfloat16()
    cu = torch.arange(2 * B + 1, dtype=torch.int32, device=gpu) * S
    valid = torch.ones(B, dtype=torch.int32, device=gpu)
    valid[4] = 0
    ones = torch.ones(2 * B * S, dtype=torch.long, device=gpu)
    runs = [_head_step(h, cu, ones, valid, S), _head_step(h, cu, ones, valid, S), _head_step(h, cu, None, valid, S)]
    for other in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], other))
    assert runs[0][3].float().abs().sum() > 0 and runs[0][2][2].item() == B - 1


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("name", ["hsd-tiny-mpnet", "hsd-tiny-bert"])
def test_model_step_vs_fp32_reference_model(gpu, name, packed):
    """2 layers, B = 4 pairs, S = 64, bf16 with dropout on (the hash masks are shared) against the same weights in fp32
    on the reference ops, at the model-step tolerances of tests/test_gpu_qa_head.py: loss 2e-2, every matrix and the
    concatenated vectors 5e-2 relative."""
    from huggingface_sagemaker_tensorflow_distributed_amd.data.packing import pack_batch, position_rule

    cfg = resolve_config(name).replace(hidden_size=128, num_attention_heads=2, intermediate_size=256)
    m32 = build_model(cfg, task="sentence-embedding", seed=0).to(gpu)
    m16 = copy.deepcopy(m32).bfloat16()
    with torch.no_grad():
        for p32, p16 in zip(m32.parameters(), m16.parameters()):
            p32.copy_(p16.float())
    B, S = 4, 64
    rng = np.random.default_rng(0)
    lengths = np.array([S, 40, 17, 5, S, 33, 64, 9])
    ids = rng.integers(5, cfg.vocab_size, size=(2 * B, S)).astype(np.int64)
    ids[1::2, :4] = ids[0::2, :4]  # positives share their anchor's first tokens
    mask = (np.arange(S)[None, :] < lengths[:, None]).astype(np.int64)
    ids[mask == 0] = cfg.pad_token_id
    labels = np.array([0, 0, -100, 0])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    if packed:
        pk = pack_batch(ids, mask, np.zeros(2 * B, dtype=np.int64), **position_rule(cfg))
        kw = dict(input_ids=t(pk["input_ids"]), labels=t(labels), cu_seqlens=t(pk["cu_seqlens"]),
                  max_seqlen=pk["max_seqlen"], position_ids=t(pk["position_ids"]))
    else:
        kw = dict(input_ids=t(ids.reshape(B, 2 * S)), attention_mask=t(mask.reshape(B, 2 * S)), labels=t(labels))
    out = []
    for model, force in ((m16, False), (m32, True)):
        old, ops._FORCE_TORCH = ops._FORCE_TORCH, force
        try:
            model.zero_grad(set_to_none=True)
            model.rng.new_step(5)
            loss, e = model(**kw)
            loss.backward()
        finally:
            ops._FORCE_TORCH = old
        out.append((loss.detach().float(), e.detach().float(), loss._hsd_stats[2].item(),
                    {n: p.grad.float() for n, p in model.named_parameters()}))
    (l1, e1, n1, g1), (l2, e2, n2, g2) = out
    assert n1 == n2 == 3.0 and tuple(e1.shape) == (2 * B, 128)
    assert torch.allclose(l1, l2, atol=2e-2, rtol=2e-2), (l1, l2)
    assert torch.allclose(e1, e2, atol=2e-2, rtol=2e-2)
    vec = [torch.cat([g[n].reshape(-1) for n in g1 if g1[n].dim() < 2]) for g in (g1, g2)]
    for n, a, b in [(n, g1[n], g2[n]) for n in g1 if g1[n].dim() >= 2] + [("all 1-D parameters", *vec)]:
        rel = (a - b).norm() / (b.norm() + 1e-6)
        print(f"  d{n}: rel err {rel:.3g}")
        assert rel < 5e-2, (n, float(rel))
