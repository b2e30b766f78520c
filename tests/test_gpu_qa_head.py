"""The fused question-answering head: span_ce_kernel / span_stats_kernel (csrc/kernels/qa_head.hip) against fp64 torch
on the kernel's own logits, the whole head (token_head.hip's logits pass and given-gradient backward around them)
against the fp32 reference head, the dispatch, and the model step, trainer step and whole-step graph on top of it."""
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
TASK = "question-answering"      # the command line's name, also taken by from_pretrained
MODEL_TASK = "span-extraction"   # build_model's key for it
EDGE_LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 1024]  # the span kernel strides a sequence 256 rows at a time


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


# The bias gradient of this loss is ZERO in exact arithmetic: a column's softmax runs along the sequence, so
# Σ_rows (softmax - onehot) = 1 - 1 for every sequence whose position is valid (the loss does not change when a constant
# is added to a column). What either implementation returns is the rounding of that sum, and a relative error between
# two roundings of zero says nothing. Bound instead: a sequence's Σ softmax is off by at most L terms of 2^-22 each (the
# exponential's and the addition's rounding), L <= 1,024, and the factors ½ / n_c over the sequences sum to ½.
BIAS_GRAD_ABS = 1024 * 2.0 ** -22


def _grad_close(name, got, want, tol):
    if name in ("b", "qa_outputs_bias"):
        assert got.float().abs().max().item() <= BIAS_GRAD_ABS, (name, got)
        assert want.float().abs().max().item() <= BIAS_GRAD_ABS, (name, want)
        return
    rel = (got.float() - want).norm() / (want.norm() + 1e-6)
    print(f"  d{name}: rel err {rel:.3g}")
    assert rel < tol, f"{name}: rel err {rel:.3g}"


def _model_grads_close(g1, g2, tol):
    """Model gradients against the reference model's: every matrix and embedding table on its own at ``tol``
    relative; the qa_outputs bias by BIAS_GRAD_ABS; the other vectors (biases, LayerNorm weights) as ONE concatenated
    vector at ``tol``. A bias gradient is the sum over the rows of a gradient whose row sum is zero at the head (see
    above) and stays partly cancelled below it, so a single small vector's relative error measures its conditioning
    more than the kernels: layer 0's ln1_bias came out at 0.056 against the fp32 model on one MI355X while its matrices
    were at 0.006 - 0.015."""
    vec1, vec2 = [], []
    for n in g1:
        if n == "qa_outputs_bias" or g1[n].dim() >= 2:
            _grad_close(n, g1[n], g2[n], tol)
        else:
            vec1.append(g1[n].reshape(-1))
            vec2.append(g2[n].reshape(-1))
    _grad_close("all 1-D parameters", torch.cat(vec1), torch.cat(vec2), tol)


# ------------------------------------------------------------------------------------------ 1. the span kernel alone
def _span_kernel(logits, cu, mask, pos, mal):
    """The raw launch: (rec [B, 8], pred [B, 2], g0 [R, 2], stats [8]); g0 pre-filled with NaN."""
    hip = _hip()
    R, B = logits.shape[0], cu.numel() - 1
    dev = logits.device
    rec = torch.full((B * 8,), float("nan"), dtype=torch.float32, device=dev)
    pred = torch.full((B, 2), -7, dtype=torch.int32, device=dev)
    g0 = torch.full((R, 2), float("nan"), dtype=torch.float32, device=dev)
    stats = torch.full((8,), float("nan"), dtype=torch.float32, device=dev)
    hip._C.span_ce(logits, cu, mask, pos, int(mal), rec, pred, g0, stats)
    return rec.view(B, 8), pred, g0, stats


def _span_fp64(logits, cu, mask, pos, mal):
    """The definition, sequence by sequence, in fp64 on the CPU (the best span with ONE fp32 add, as specified)."""
    x = logits.float().cpu().numpy()
    cu = cu.cpu().numpy().astype(np.int64)
    mask = np.ones(x.shape[0], dtype=bool) if mask is None else mask.cpu().numpy() != 0
    pos = pos.cpu().numpy()
    B = len(cu) - 1
    out = {"lse": np.zeros((B, 2)), "loss": np.zeros((B, 2)), "valid": np.zeros((B, 2), dtype=bool),
           "pred": np.zeros((B, 2), dtype=np.int64), "g0": np.zeros(x.shape, dtype=np.float64)}
    for b in range(B):
        a, z = int(cu[b]), int(cu[b + 1])
        n = z - a
        real = mask[a:z]
        if n == 0 or not real.any():
            continue
        xs = x[a:z].astype(np.float64)
        for c in range(2):
            v = xs[real, c]
            m = v.max()
            lse = m + np.log(np.exp(v - m).sum())
            out["lse"][b, c] = lse
            p = int(pos[b, c])
            if 0 <= p < n and real[p]:
                out["valid"][b, c] = True
                out["loss"][b, c] = lse - xs[p, c]
                g = np.where(real, np.exp(xs[:, c] - lse), 0.0)
                g[p] -= 1.0
                out["g0"][a:z, c] = g
        sc = x[a:z, 0][:, None].astype(np.float32) + x[a:z, 1][None, :].astype(np.float32)
        i = np.arange(n)
        ok = (i[None, :] >= i[:, None]) & (i[None, :] - i[:, None] < mal) & real[:, None] & real[None, :]
        k = int(np.argmax(np.where(ok, sc, -np.inf)))  # the first maximum in (s, e) order
        out["pred"][b] = (k // n, k % n)
    return out


def _span_inputs(lengths, dead, seed, mask_lengths=None, ignore=()):
    """CPU tensors. ``lengths``: the segments (cu); ``mask_lengths``: real rows per segment (the padded form), else no
    mask; ``ignore``: (sequence, column, value) positions to overwrite."""
    g = torch.Generator().manual_seed(seed)
    cu = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int32)
    R = int(cu[-1]) + dead
    logits = (torch.randn(R, 2, generator=g) * 2.0).bfloat16()
    mask = None
    reals = list(lengths)
    if mask_lengths is not None:
        reals = list(mask_lengths)
        mask = torch.cat([(torch.arange(n) < r).long() for n, r in zip(lengths, reals)] + [torch.zeros(dead).long()])
    pos = torch.stack([torch.tensor([int(torch.randint(0, max(r, 1), (1,), generator=g)) for r in reals])
                       for _ in range(2)], dim=1).sort(dim=1).values
    for b, c, v in ignore:
        pos[b, c] = v
    return logits, cu, mask, pos


def _check_span(gpu, lengths, dead, seed, mal=30, mask_lengths=None, ignore=()):
    logits, cu, mask, pos = _span_inputs(lengths, dead, seed, mask_lengths, ignore)
    want = _span_fp64(logits, cu, mask, pos, mal)
    rec, pred, g0, stats = _span_kernel(logits.to(gpu), cu.to(gpu), None if mask is None else mask.to(gpu),
                                        pos.to(gpu), mal)
    rec, pred, g0, stats = rec.cpu().double().numpy(), pred.cpu().numpy(), g0.cpu().double().numpy(), \
        stats.cpu().double().numpy()
    B = len(lengths)
    tgt = logits.float().double().numpy()
    for b in range(B):
        for c in range(2):
            assert bool(rec[b, 2 + c]) == bool(want["valid"][b, c]), (b, c)
            if want["valid"][b, c]:
                loss_ref, lse_ref = want["loss"][b, c], want["lse"][b, c]
                lse = rec[b, c] + tgt[int(cu[b]) + int(pos[b, c]), c]
                print(f"  L={lengths[b]} col {c}: lse {lse:.7f} ref {lse_ref:.7f}, loss {rec[b, c]:.7f} ref {loss_ref:.7f}")
                assert abs(lse - lse_ref) <= 1e-4 * abs(lse_ref), (b, c, lse, lse_ref)
                assert abs(rec[b, c] - loss_ref) <= 1e-4 * abs(loss_ref), (b, c, rec[b, c], loss_ref)
            else:
                assert rec[b, c] == 0.0
    assert np.array_equal(pred, want["pred"]), (pred, want["pred"])
    valid = want["valid"]
    both = valid.all(axis=1)
    eq = (want["pred"] == pos.numpy()) & valid
    n0, n1 = valid[:, 0].sum(), valid[:, 1].sum()
    loss_ref = 0.5 * (want["loss"][:, 0].sum() / max(n0, 1) + want["loss"][:, 1].sum() / max(n1, 1))
    assert abs(stats[0] - loss_ref) <= 1e-4 * abs(loss_ref), (stats[0], loss_ref)
    assert stats[1:3].tolist() == [float((eq.all(axis=1) & both).sum()), float(both.sum())]
    assert abs(stats[3] - stats[0] * both.sum()) <= 1e-6 * max(1.0, abs(stats[3]))
    assert stats[4:].tolist() == [float(n0), float(n1), float(eq[:, 0].sum()), float(eq[:, 1].sum())]
    # g0: every element written; exact zeros on masked rows, dead rows and ignored columns; softmax - onehot elsewhere
    assert not np.isnan(g0).any()
    assert np.abs(g0[want["g0"] == 0.0]).sum() == 0.0
    assert np.abs(g0 - want["g0"]).max() <= 1e-5  # exp of an argument good to |lse| 2^-23, values <= 1
    return want, pos


@pytest.mark.parametrize("L", EDGE_LENGTHS)
def test_span_kernel_single_sequence(gpu, L):
    """B = 1 at every edge length, 5 dead rows after the sequence. lse and loss within 1e-4 relative of fp64 (at most
    1,024 fp32 additions at 2^-24 each plus the fast exponential and logarithm); L = 1 gives lse = the logit and
    loss = 0 exactly on both sides. pred, hits and the n counts exact."""
    want, _ = _check_span(gpu, [L], 5, seed=100 + L)
    assert want["valid"].all()
    if L == 1:
        assert (want["loss"] == 0.0).all()


def test_span_kernel_mixed_lengths_in_one_packed_buffer(gpu):
    _check_span(gpu, EDGE_LENGTHS, 13, seed=7)
    _check_span(gpu, [65, 1, 257], 0, seed=8)  # B = 3, no dead rows
    for mal in (1, 2, 5000):  # max_answer_length of 1 and of more than any sequence
        want, _ = _check_span(gpu, [65, 1, 257, 1024], 3, seed=9, mal=mal)
        assert ((want["pred"][:, 1] - want["pred"][:, 0]) < mal).all() and (want["pred"][:, 1] >= want["pred"][:, 0]).all()


def test_span_kernel_padded_form_with_a_mask_and_ignored_positions(gpu):
    """cu = arange(B+1)·S with the flat attention mask: B = 5, S = 300, real lengths 300 / 257 / 64 / 1 / 0 (a
    sequence with no real row contributes nothing); one label past its sequence, one negative, one on a padding row."""
    S = 300
    want, pos = _check_span(gpu, [S] * 5, 0, seed=11, mask_lengths=[300, 257, 64, 1, 0],
                            ignore=[(0, 1, 300), (1, 0, -100), (2, 1, 64)])
    assert want["valid"].tolist() == [[True, False], [False, True], [True, False], [True, True], [False, False]]
    assert want["pred"][4].tolist() == [0, 0]
    # all labels ignored: loss 0, counts 0, g0 all zeros
    want, _ = _check_span(gpu, [S] * 3, 0, seed=12, mask_lengths=[300, 64, 1],
                          ignore=[(b, c, -100) for b in range(3) for c in range(2)])
    assert not want["valid"].any()


def test_span_kernel_tie_rule_on_equal_logits(gpu):
    cu = torch.tensor([0, 300, 600], dtype=torch.int32, device=gpu)
    lg = torch.zeros(600, 2, dtype=torch.bfloat16, device=gpu)
    pos = torch.tensor([[0, 0], [5, 5]], device=gpu)
    rec, pred, g0, stats = _span_kernel(lg, cu, None, pos, 30)
    assert pred.tolist() == [[0, 0], [0, 0]] and stats[1:3].tolist() == [1.0, 2.0]
    mask = torch.ones(600, dtype=torch.long, device=gpu)
    mask[:260] = 0  # the first real row of sequence 0 belongs to the second 256-row stride
    lg[270, 0] = lg[299, 0] = 1.0   # equal starts: the first
    lg[280, 1] = lg[290, 1] = 2.0   # equal ends: the first within max_answer_length
    lg[300 + 299, 0] = 1.0          # sequence 1: the best start is the last row, the span is (299, 299)
    _, pred, _, _ = _span_kernel(lg, cu, mask, pos, 30)
    assert pred.tolist() == [[270, 280], [299, 299]]
    _, pred, _, _ = _span_kernel(lg, cu, mask, pos, 5)  # 270 + 5 does not reach 280: 0 + 2 at (276, 280) ties 1 + 2?
    want = ref.span_best(lg, cu, mask, 5)
    assert pred.tolist() == want.tolist() and pred[0, 1] - pred[0, 0] < 5
    # labels absent: pred only
    hip = _hip()
    pred2 = torch.full((2, 2), -7, dtype=torch.int32, device=gpu)
    none = torch.empty(0, dtype=torch.float32, device=gpu)
    hip._C.span_ce(lg, cu, mask, None, 5, none, pred2, none, none)
    assert torch.equal(pred2, pred)


# ------------------------------------------------------------------------------------------ 2. the whole head
def _head_inputs(gpu, H, packed, seed=17):
    """Padded: B = 4, S = 80, real lengths 80 / 63 / 2 / 1. Packed: lengths 1 / 2 / 63 / 65 / 257 and 7 dead rows."""
    g = torch.Generator().manual_seed(seed)
    if packed:
        lengths = [1, 2, 63, 65, 257]
        cu = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int32)
        R, mask, reals = int(cu[-1]) + 7, None, lengths
    else:
        S, reals = 80, [80, 63, 2, 1]
        cu = torch.arange(5, dtype=torch.int32) * S
        R = 4 * S
        mask = torch.cat([(torch.arange(S) < r).long() for r in reals])
    h = torch.randn(R, H, generator=g).to(gpu).bfloat16().requires_grad_()
    w = (torch.randn(2, H, generator=g) * 0.05).to(gpu).bfloat16().requires_grad_()
    b = (torch.randn(2, generator=g) * 0.5).to(gpu).bfloat16().requires_grad_()
    pos = torch.stack([torch.tensor([int(torch.randint(0, r, (1,), generator=g)) for r in reals])
                       for _ in range(2)], dim=1).sort(dim=1).values
    pos[0, 1] = 4000  # one ignored label
    live = torch.zeros(R, dtype=torch.bool)
    for i, r in enumerate(reals):
        live[int(cu[i]):int(cu[i]) + r] = True
    return h, w, b, pos.to(gpu), cu.to(gpu), None if mask is None else mask.to(gpu), live.to(gpu)


def _reference(h, w, b, pos, cu, mask, p, mal=30):
    f = [x.detach().float().requires_grad_() for x in (h, w, b)]
    loss, logits, stats, pred = ref.qa_head(f[0], f[1], f[2], pos, cu, mask, p, SEED, mal)
    loss.backward()
    return loss.detach(), logits.detach(), [x.grad for x in f]


def _raw_backward(h, w, g0, stats, p):
    hip = _hip()
    R, H = h.shape
    dh = torch.full((R, H), float("nan"), dtype=torch.bfloat16, device=h.device)
    dW = torch.zeros(2 * H, dtype=torch.float32, device=h.device)
    db = torch.zeros(2, dtype=torch.float32, device=h.device)
    part = torch.empty(hip._C.token_head_bwd_blocks(R) * (2 * H + 2), dtype=torch.float32, device=h.device)
    dl = torch.ones(1, dtype=torch.float32, device=h.device)
    hip._C.token_head_bwd_given(h.detach(), w.detach(), g0, stats[4:6], 0.5, dl, dh, part, dW, db, float(p),
                                hip._s64(SEED))
    return dh, dW.view(2, H), db


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("H", [64, 768, 1024])
def test_qa_head_vs_reference(gpu, H, p, packed):
    """Forward + backward at the bounds of tests/test_gpu_token_head.py::test_token_head_vs_reference (the arithmetic
    from g on is the same code): logits 3e-2 / 3e-2 under the 0.1 % / 4x rule, loss 2e-2, gradients 4e-2 relative."""
    h, w, b, pos, cu, mask, live = _head_inputs(gpu, H, packed)
    loss, logits = ops.qa_head(h, w, b, pos, cu, mask, p, SEED, 30)
    stats, pred = loss._hsd_stats, loss._hsd_pred
    assert logits.dtype == torch.bfloat16 and tuple(logits.shape) == (h.shape[0], 2) and stats.shape == (8,)
    loss.backward()
    loss_ref, lg_ref, g_ref = _reference(h, w, b, pos, cu, mask, p)
    print(f"H={H} p={p} packed={packed}: loss {loss.item():.5f} ref {loss_ref.item():.5f}")
    _close(logits, lg_ref, 3e-2, 3e-2, "logits")
    assert abs(loss.item() - loss_ref.item()) < 2e-2 * max(1.0, abs(loss_ref.item())), (loss.item(), loss_ref.item())
    for n, a, r_ in zip(["h", "w", "b"], (h.grad, w.grad, b.grad), g_ref):
        _grad_close(n, a, r_, 4e-2)
    # pred / hits / n: exact, from the kernel's own rounded logits
    _, stats_ref, pred_ref = ref.span_loss(logits.float(), pos, cu, mask, 30)
    assert torch.equal(pred, pred_ref)
    assert stats[1:3].tolist() == stats_ref[1:3].tolist() and stats[4:].tolist() == stats_ref[4:].tolist()
    B = cu.numel() - 1
    assert stats[4].item() == B and stats[5].item() == B - 1 and stats[2].item() == B - 1
    # the raw launches on fresh buffers: every element of dh written (NaN pre-fill), padding and dead rows exactly
    # zero, and the bits autograd returned
    rec, pred_raw, g0, stats_raw = _span_kernel(logits, cu, mask, pos, 30)
    assert torch.equal(stats_raw, stats) and torch.equal(pred_raw, pred)
    dh, dW, db = _raw_backward(h, w, g0, stats_raw, p)
    assert not torch.isnan(dh.float()).any()
    assert torch.count_nonzero(dh[~live]) == 0 and torch.count_nonzero(g0[~live]) == 0
    assert torch.count_nonzero(dh[live]) > 0
    assert torch.equal(dh, h.grad) and torch.equal(dW.to(torch.bfloat16), w.grad) and torch.equal(db.bfloat16(), b.grad)
    # labels absent: the inference entry gives the same logits and spans
    lg2, pred2 = ops.qa_head(h.detach(), w.detach(), b.detach(), None, cu, mask, p, SEED, 30)
    assert torch.equal(lg2, logits) and torch.equal(pred2, pred)


def test_all_labels_ignored_gives_zero_loss_and_zero_gradients(gpu):
    h, w, b, pos, cu, mask, live = _head_inputs(gpu, 768, False)
    loss, _ = ops.qa_head(h, w, b, torch.full_like(pos, -100), cu, mask, 0.1, SEED, 30)
    loss.backward()
    assert loss.item() == 0.0 and loss._hsd_stats.tolist() == [0.0] * 8
    for x in (h.grad, w.grad, b.grad):
        assert torch.count_nonzero(x) == 0 and not torch.isnan(x.float()).any()


def test_two_runs_give_the_same_bits(gpu):
    """B = 24 sequences of 384 rows: 576 16-row tiles over the backward's 512 persistent blocks (several tiles per
    block, 512 partial slabs through the reducer), twice."""
    g = torch.Generator().manual_seed(3)
    B, S, H = 24, 384, 768
    h = torch.randn(B * S, H, generator=g).to(gpu).bfloat16().requires_grad_()
    w = (torch.randn(2, H, generator=g) * 0.05).to(gpu).bfloat16().requires_grad_()
    b = torch.zeros(2, device=gpu, dtype=torch.bfloat16).requires_grad_()
    cu = torch.arange(B + 1, dtype=torch.int32, device=gpu) * S
    mask = (torch.arange(S)[None, :] < torch.randint(12, S + 1, (B, 1), generator=g)).long().reshape(-1).to(gpu)
    pos = torch.randint(0, 12, (B, 2), generator=g).sort(dim=1).values.to(gpu)
    assert _hip()._C.token_head_bwd_blocks(B * S) < B * S // 16
    outs = []
    for _ in range(2):
        for x in (h, w, b):
            x.grad = None
        loss, logits = ops.qa_head(h, w, b, pos, cu, mask, 0.1, SEED, 30)
        loss.backward()
        outs.append((loss.detach().clone(), logits.clone(), loss._hsd_stats.clone(), loss._hsd_pred.clone(),
                     h.grad.clone(), w.grad.clone(), b.grad.clone()))
    for a, c in zip(*outs):
        assert torch.equal(a, c)
    assert outs[0][4].float().abs().sum() > 0 and outs[0][5].float().abs().sum() > 0


def test_backward_adds_into_main_grad(gpu):
    h, w, b, pos, cu, mask, _ = _head_inputs(gpu, 768, True)
    loss, logits = ops.qa_head(h, w, b, pos, cu, mask, 0.0, SEED, 30)
    loss.backward()
    g = torch.Generator().manual_seed(3)
    pre_w = torch.randint(-4, 5, (2, 768), generator=g).float().to(gpu)
    w2, b2 = w.detach().clone().requires_grad_(), b.detach().clone().requires_grad_()
    w2.main_grad, b2.main_grad = pre_w.clone(), torch.zeros(2, device=gpu)
    loss2, _ = ops.qa_head(h.detach().requires_grad_(), w2, b2, pos, cu, mask, 0.0, SEED, 30)
    loss2.backward()
    assert w2.grad is None and b2.grad is None
    # (prefill + g) - prefill: one fp32 rounding at magnitude <= 8, i.e. at most 2^-21 off g; w.grad is bf16(g)
    torch.testing.assert_close((w2.main_grad - pre_w).bfloat16().float(), w.grad.float(), atol=1e-6, rtol=2 ** -7)
    assert torch.equal(b2.main_grad.bfloat16(), b.grad)


# ------------------------------------------------------------------------------------------ 3. dispatch
def test_fused_path_runs_and_everything_else_takes_the_composed_ops(gpu, monkeypatch):
    hip = _hip()
    calls = []
    real = hip.qa_head
    monkeypatch.setattr(hip, "qa_head", lambda *a: (calls.append(a[0].shape), real(*a))[1])

    def run(h, w, b, pos, cu, mask, **kw):
        for x in (h, w, b):
            x.grad = None
        loss, logits = ops.qa_head(h, w, b, pos, cu, mask, 0.1, SEED, 30, **kw)
        loss.backward()
        assert loss._hsd_stats.shape == (8,) and loss._hsd_pred.dtype == torch.int32
        return loss.detach().float(), logits.detach().float(), h.grad.float().clone()

    def agree(got, want, what):
        _close(got[1], want[1], 3e-2, 3e-2, f"{what}: logits")
        assert abs(got[0].item() - want[0].item()) < 2e-2 * max(1.0, abs(want[0].item())), what
        rel = (got[2] - want[2]).norm() / (want[2].norm() + 1e-6)
        assert rel < 4e-2, (what, float(rel))

    h, w, b, pos, cu, mask, _ = _head_inputs(gpu, 768, False)
    fused = run(h, w, b, pos, cu, mask, max_seqlen=80)
    assert len(calls) == 1 and hip.qa_head_ok(h, w, cu, 80)
    lr, lgr, gr = _reference(h, w, b, pos, cu, mask, 0.1)
    agree(fused, (lr, lgr, gr[0]), "fused vs reference")
    # a sequence longer than the kernel holds: composed
    assert not hip.qa_head_ok(h, w, cu, 1025)
    agree(run(h, w, b, pos, cu, mask, max_seqlen=1025), fused, "max_seqlen 1025")
    # fp32 tensors
    f = [x.detach().float().requires_grad_() for x in (h, w, b)]
    agree(run(f[0], f[1], f[2], pos, cu, mask), fused, "fp32")
    # H outside the limits (no fused form exists: against the reference)
    g = torch.Generator().manual_seed(1)
    h2 = torch.randn(320, 1032, generator=g).to(gpu).bfloat16().requires_grad_()
    w2 = (torch.randn(2, 1032, generator=g) * 0.05).to(gpu).bfloat16().requires_grad_()
    assert not hip.qa_head_ok(h2, w2, cu, 80)
    lr, lgr, gr = _reference(h2, w2, b, pos, cu, mask, 0.1)
    agree(run(h2, w2, b, pos, cu, mask, max_seqlen=80), (lr, lgr, gr[0]), "H = 1032")
    # the knob
    monkeypatch.setattr(ops, "QA_HEAD_FUSED", False)
    agree(run(h, w, b, pos, cu, mask, max_seqlen=80), fused, "HSD_QA_HEAD=composed")
    assert len(calls) == 1  # only the first call ran the fused kernels


# ------------------------------------------------------------------------------------------ 4. model level
def _batch(cfg, B, S, seed=0, segments=False):
    g = np.random.default_rng(seed)
    lengths = np.array([S, S * 5 // 8, S // 4 + 1, 12] * (B // 4))
    ids = g.integers(5, cfg.vocab_size, size=(B, S)).astype(np.int64)
    mask = (np.arange(S)[None, :] < lengths[:, None]).astype(np.int64)
    ids[mask == 0] = cfg.pad_token_id
    start = (g.random(B) * (lengths - 4)).astype(np.int64)
    labels = np.stack([start, start + g.integers(0, 4, size=B)], axis=1)
    labels[1] = (-100, -100)
    tt = ((np.arange(S)[None, :] >= 5) & (mask != 0)).astype(np.int64) if segments else None
    return ids, mask, labels, tt


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


def _model_kwargs(gpu, cfg, packed, segments):
    ids, mask, labels, tt = _batch(cfg, 4, 128, segments=segments)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    if packed:
        pk = pack_batch(ids, mask, labels, **position_rule(cfg), span_labels=True, token_type_ids=tt)
        kw = dict(input_ids=t(pk["input_ids"]), labels=t(pk["labels"]), cu_seqlens=t(pk["cu_seqlens"]),
                  max_seqlen=pk["max_seqlen"], position_ids=t(pk["position_ids"]))
        if tt is not None:
            kw["token_type_ids"] = t(pk["token_type_ids"])
        real = torch.ones(int(pk["real_tokens"]), dtype=torch.bool)
        real = torch.cat([real, torch.zeros(pk["input_ids"].shape[1] - real.numel(), dtype=torch.bool)])
    else:
        kw = dict(input_ids=t(ids), attention_mask=t(mask), labels=t(labels))
        if tt is not None:
            kw["token_type_ids"] = t(tt)
        real = torch.from_numpy(mask.reshape(-1) != 0)
    return kw, real.to(gpu)


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("name", ["hsd-tiny-bert", "hsd-tiny-distilbert"])
def test_model_step_vs_fp32_reference_model(gpu, name, packed):
    """2 layers, B = 4, S = 128, bf16 with dropout on (the hash masks are shared), padded and packed, against the same
    weights in fp32 on the reference ops, at tests/test_gpu_token_head.py's model-step tolerances. BERT runs with
    non-zero segment ids, DistilBERT with its head dropout."""
    cfg = resolve_config(name).replace(hidden_size=128, num_attention_heads=2, intermediate_size=256)
    m32 = build_model(cfg, task=MODEL_TASK, seed=0).to(gpu)
    assert (m32.head_dropout() > 0) == (name == "hsd-tiny-distilbert")
    m16 = copy.deepcopy(m32).bfloat16()
    with torch.no_grad():
        for p32, p16 in zip(m32.parameters(), m16.parameters()):
            p32.copy_(p16.float())
    kw, real = _model_kwargs(gpu, cfg, packed, segments=name == "hsd-tiny-bert")
    l1, lg1, g1 = _model_step(m16, kw, False)
    l2, lg2, g2 = _model_step(m32, kw, True)
    assert torch.allclose(l1, l2, atol=2e-2, rtol=2e-2), (l1, l2)
    assert torch.allclose(lg1.reshape(-1, 2)[real], lg2.reshape(-1, 2)[real], atol=5e-2, rtol=5e-2)
    _model_grads_close(g1, g2, 5e-2)


def test_packed_step_matches_padded_step_on_the_gpu(gpu):
    """The same bf16 weights, dropout off, padded and packed on the HIP path: both are within the bounds above of the
    fp32 model, so of each other at twice them; the counts are exact."""
    cfg = resolve_config("hsd-tiny-bert").replace(hidden_size=128, num_attention_heads=2, intermediate_size=256,
                                                  hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    m = build_model(cfg, task=MODEL_TASK, seed=0).to(gpu).bfloat16()
    kw0, _ = _model_kwargs(gpu, cfg, False, True)
    kw1, _ = _model_kwargs(gpu, cfg, True, True)
    l0, _, g0 = _model_step(m, kw0, False)
    l1, _, g1 = _model_step(m, kw1, False)
    assert torch.allclose(l0, l1, atol=4e-2, rtol=4e-2), (l0, l1)
    _model_grads_close(g1, g0, 1e-1)


def _trainer(gpu, graph, graph_replay=True, accum=1):
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedAdam
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore
    from huggingface_sagemaker_tensorflow_distributed_amd.train.trainer import Trainer

    cfg = resolve_config("bert-base-uncased").replace(num_hidden_layers=2)
    model = build_model(cfg, task=MODEL_TASK, seed=0).to(gpu)
    model.rng.base_seed = 5
    store = FlatParamStore(model, gpu, compute_dtype=torch.bfloat16)
    opt = FusedAdam(store, lr=1e-4, weight_decay=0.01)
    tr = Trainer(model, store, opt, None, gpu, hip_graph=graph, grad_accum=accum, lr_schedule="linear",
                 lr_warmup_steps=2)
    if graph:
        tr._graph_replay = graph_replay
    return tr


def _trainer_batches(gpu, n, B=16, S=128):
    g = torch.Generator().manual_seed(0)
    out = []
    for _ in range(n):
        ids = torch.randint(1000, 30000, (B, S), generator=g)
        am = torch.ones(B, S, dtype=torch.long)
        am[3, 70:] = 0
        tt = torch.zeros(B, S, dtype=torch.long)
        tt[:, 9:] = 1
        tt = tt * am
        start = torch.randint(9, 60, (B, 1), generator=g)
        labels = torch.cat([start, start + torch.randint(0, 4, (B, 1), generator=g)], dim=1)
        labels[5] = -100
        out.append({"input_ids": ids.to(gpu), "attention_mask": am.to(gpu), "token_type_ids": tt.to(gpu),
                    "labels": labels.to(gpu)})
    return out


def test_trainer_step_with_accumulation(gpu):
    """One optimizer step over two micro-batches: the meter sums the fused records of both, the weights move, and the
    segment ids reach the model (zeroing them changes the loss)."""
    from huggingface_sagemaker_tensorflow_distributed_amd.train.trainer import _Meter

    tr = _trainer(gpu, graph=False, accum=2)
    mbs = _trainer_batches(gpu, 2)
    before = tr.store.master.clone()
    meter = _Meter(gpu)
    loss = tr.train_step(mbs, meter)
    res = meter.result(global_=False)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and tr.optimizer.step_count == 1
    assert not torch.equal(before, tr.store.master)
    assert float(meter.t[2]) == 30.0  # 2 x (16 - 1) sequences with both labels valid
    assert np.isfinite(res["loss"]) and 0.0 <= res["sparse_categorical_accuracy"] <= 1.0
    tr.model.eval()
    with torch.no_grad():
        a, _ = tr._forward_loss(mbs[0])
        b, _ = tr._forward_loss({k: v for k, v in mbs[0].items() if k != "token_type_ids"})
    assert abs(float(a) - float(b)) > 1e-4


def test_whole_step_graph_replay_matches_eager(gpu, monkeypatch):
    """Three optimizer steps of a 2-layer bert-base (B = 16, S = 128, span labels, segment ids) captured and replayed
    as one graph each, against the same steps run eagerly with the same seeds (tests/test_gpu_graph.py's bounds)."""
    monkeypatch.setenv("HSD_GRAPH_FULL", "1")
    batches = _trainer_batches(gpu, 3)
    res = {}
    for replay in (False, True):
        tr = _trainer(gpu, graph=True, graph_replay=replay)
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
    assert len({round(x, 6) for x in l1}) == 3
