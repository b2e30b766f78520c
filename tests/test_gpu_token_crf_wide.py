"""The fused linear-chain CRF head for 17 .. 64 tags (csrc/kernels/crf_head_wide.hip, token_head_wide.hip's
given-gradient backward) against ``reference.crf_loss`` in fp64 on the same bf16-rounded emissions; the model step and
the whole-step graph on top of it. Shapes, batch and bounds are those of tests/test_gpu_token_crf.py."""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from huggingface_sagemaker_tensorflow_distributed_amd import ops  # noqa: E402
from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model, resolve_config  # noqa: E402
from huggingface_sagemaker_tensorflow_distributed_amd.ops import reference as ref  # noqa: E402

import test_gpu_token_head as tok  # noqa: E402  (the token head's batch builder, model step and trainer set-up)

H, S_PAD, DEAD = 64, 608, 7
LENGTHS = (1, 2, 63, 64, 65, 130, 5, 600)  # chunk edges (64 rows), an empty chain (the 5), a long recursion
WIDE = [17, 33, 64]  # 17 and 33: one tag alone in the last wave; 64: no padding


@functools.lru_cache(maxsize=None)
def _case(C, padded):
    """One batch, packed (dead rows carrying a valid tag after the last sequence) or padded to S = 608, run once through
    ``hip.token_crf`` (forward + backward) and through the three launches on their own buffers; plus, for the packed
    form, the reference in fp64 and fp32 on the op's own emissions."""
    from huggingface_sagemaker_tensorflow_distributed_amd.ops import hip

    gpu, g = torch.device("cuda"), torch.Generator().manual_seed(100 + C)
    hs, labs = [], []
    for n in LENGTHS:
        lab = torch.randint(0, C, (n,), generator=g)
        if n in (63, 64, 65):
            lab[torch.rand(n, generator=g) < 0.25] = -100
        if n == 130:  # gaps at both ends and across the chunk edge
            lab[:3], lab[60:70], lab[-2:] = -100, -100, -100
        if n == 5:
            lab[:] = -100
        pad = S_PAD - n if padded else 0
        labs.append(torch.cat([lab, torch.full((pad,), -100)]))
        hs.append(torch.cat([torch.randn(n, H, generator=g), torch.ones(pad, H)]))
    if not padded:
        labs.append(torch.zeros(DEAD, dtype=torch.long))
        hs.append(torch.ones(DEAD, H))
    lens = torch.tensor([S_PAD] * len(LENGTHS) if padded else LENGTHS)
    cu = torch.cat([torch.zeros(1, dtype=torch.long), lens.cumsum(0)]).to(torch.int32).to(gpu)
    labels = torch.cat(labs).to(gpu)
    h = torch.cat(hs).to(gpu).bfloat16().requires_grad_()
    w = (torch.randn(C, H, generator=g) * 0.25).to(gpu).bfloat16().requires_grad_()
    b = (torch.randn(C, generator=g) * 0.5).to(gpu).bfloat16().requires_grad_()
    start, end, trans = ((torch.rand(*s, generator=g) - 0.5).to(gpu).requires_grad_() for s in ((C,), (C,), (C, C)))
    loss, logits, stats, pred = hip.token_crf(h, w, b, labels, cu, start, end, trans, 0.0, 0)
    assert logits.dtype == torch.bfloat16
    loss.backward()
    out = dict(labels=labels, cu=cu, logits=logits, loss=loss.detach(), stats=stats, pred=pred, h=h, w=w, b=b,
               grads=[t.grad for t in (h, w, b, start, end, trans)], params=(start, end, trans),
               rows=torch.cat([torch.arange(n) + int(cu[i]) for i, n in enumerate(LENGTHS)]).to(gpu))
    R, B, P, cp = labels.numel(), len(LENGTHS), C * C + 2 * C, 16 * ((C + 15) // 16)
    alpha, bp, slab = hip._crf_workspace(R, B * P, gpu, cp)
    raw = [torch.full((R, C), float("nan"), device=gpu), torch.empty(4 + 64 + P, device=gpu),
           torch.empty(R, dtype=torch.int32, device=gpu), torch.empty(4 * B, device=gpu)]
    theta = hip._crf_theta(start, end, trans)
    hip._C.crf_wide_forward(logits, cu, labels, None, theta, alpha, bp, raw[2], raw[3])
    hip._C.crf_wide_marginals(logits, cu, labels, theta, alpha, raw[0], slab)
    hip._C.crf_wide_reduce(raw[3], slab, B, C, raw[1][:4], raw[1][4:68], raw[1][68:])
    out["g0"], out["red"], out["raw_pred"] = raw[0], raw[1], raw[2]
    if not padded:
        for dt in (torch.float64, torch.float32):
            prm = [t.detach().to(dt).requires_grad_() for t in (logits, start, end, trans)]
            l, _, best = ref.crf_loss(prm[0], labels, cu, *prm[1:], max_seqlen=max(LENGTHS))
            out[dt] = [l.detach()] + list(torch.autograd.grad(l, prm)) + [best]
    return out


@pytest.mark.parametrize("C", WIDE)
def test_kernels_vs_fp64_reference(gpu, C):
    """Loss, g0 / N and the three parameter gradients: the kernels' error against fp64 stays within 4x the error of the
    fp32 reference op on the same inputs (the margin is for the summation order) plus 8 fp32 ulps of the largest
    reference value (the fp32 run can be exact by chance). dh, dW and db, which pass through bf16: the relative bound of
    tests/test_gpu_token_head.py."""
    k = _case(C, False)
    r64, r32, n = k[torch.float64], k[torch.float32], k["stats"][2]
    assert n == (k["labels"][k["rows"]] >= 0).sum() and torch.equal(k["red"][4:68], n.expand(64))
    got = [k["loss"], k["g0"] / n] + k["grads"][3:]
    for name, a, w64, w32 in zip(("loss", "g0/N", "dstart", "dend", "dtrans"), got, r64, r32):
        err, ref_err = (a.double() - w64).abs().max().item(), (w32.double() - w64).abs().max().item()
        floor = 8 * 2.0 ** -23 * w64.abs().max().item()
        print(f"C={C} {name}: kernel err {err:.3e}  fp32 reference err {ref_err:.3e}  floor {floor:.3e}")
        assert err <= 4 * ref_err + floor, (name, err, ref_err, floor)
    dlog = r64[1]
    want = (dlog @ k["w"].detach().double(), dlog.t() @ k["h"].detach().double(), dlog.sum(0))
    for name, a, w_ in zip(("dh", "dW", "db"), k["grads"][:3], want):
        rel = ((a.double() - w_).norm() / (w_.norm() + 1e-6)).item()
        print(f"C={C} {name}: rel err {rel:.3e}")
        assert rel < 4e-2, (name, rel)


@pytest.mark.parametrize("C", WIDE)
def test_viterbi_path_scores_within_fp32_of_the_optimum(gpu, C):
    """Tags are not compared (near-ties): the kernel's path, scored in fp64, lies within what fp32 sums of n terms can
    lose below the fp64 optimum, n · 2^-22 · max|score|, and (up to fp64 rounding) not above it. ``token_crf_decode``
    with the chain as ``keep`` gives the labelled call's tags."""
    from huggingface_sagemaker_tensorflow_distributed_amd.ops import hip

    k = _case(C, False)
    e, (start, end, trans) = k["logits"].double(), [t.detach().double() for t in k["params"]]
    labels, pred, best = k["labels"], k["pred"].long(), k[torch.float64][-1].long()
    assert torch.equal(k["pred"], k["raw_pred"])
    for i, n in enumerate(LENGTHS):
        rows = torch.arange(int(k["cu"][i]), int(k["cu"][i]) + n, device=gpu)
        rows = rows[labels[rows] >= 0]
        if rows.numel() == 0:
            continue
        score = lambda t: (start[t[0]] + end[t[-1]] + e[rows, t].sum() + trans[t[:-1], t[1:]].sum()).item()  # noqa: E731
        got, opt = score(pred[rows]), score(best[rows])
        assert pred[rows].min() >= 0 and pred[rows].max() < C
        assert opt - rows.numel() * 2.0 ** -22 * max(abs(opt), abs(got)) <= got <= opt + 1e-9 * max(1.0, abs(opt)), (n, got, opt)
    on = torch.zeros_like(labels, dtype=torch.bool)
    on[k["rows"]] = labels[k["rows"]] >= 0
    assert (pred[~on] == -1).all() and k["stats"][1] == ((pred == labels) & on).sum()
    logits, dec = hip.token_crf_decode(k["h"], k["w"], k["b"], on.long(), k["cu"], *k["params"], 0.0, 0)
    assert torch.equal(logits, k["logits"]) and torch.equal(dec, k["pred"])


@pytest.mark.parametrize("C", WIDE)
def test_exact_properties(gpu, C):
    """Rows off the chain have all-zero g0 and dh and every element of g0 is written (NaN pre-fill); the padded form of
    the batch gives the packed form's bits sequence by sequence; a second run gives the first one's bits."""
    k, kp = _case(C, False), _case(C, True)
    on = torch.zeros_like(k["labels"], dtype=torch.bool)
    on[k["rows"]] = k["labels"][k["rows"]] >= 0
    assert not torch.isnan(k["g0"]).any() and not k["g0"][~on].any() and not k["grads"][0][~on].any()
    assert k["g0"][on].abs().sum(1).min() > 0
    assert torch.equal(k["loss"], kp["loss"]) and torch.equal(k["red"], kp["red"])
    for name in ("g0", "pred"):
        assert torch.equal(k[name][k["rows"]], kp[name][kp["rows"]]), name
    for a, b in zip(k["grads"][3:], kp["grads"][3:]):
        assert torch.equal(a, b)
    _case.cache_clear()
    again = _case(C, False)
    for name in ("loss", "stats", "pred", "g0", "red"):
        assert torch.equal(k[name], again[name]), name
    for a, b in zip(k["grads"], again["grads"]):
        assert torch.equal(a, b)


def test_dispatch(gpu):
    """``crf_head_ok`` holds up to 64 tags and not beyond; ``ops.token_crf_head`` at 17 tags is ``hip.token_crf``."""
    from huggingface_sagemaker_tensorflow_distributed_amd.ops import hip

    k = _case(17, False)
    h, cu = k["h"].detach(), k["cu"]
    for C, ok in ((17, True), (64, True), (65, False)):
        w = torch.zeros(C, H, device=gpu, dtype=torch.bfloat16)
        prm = [torch.zeros(*s, device=gpu) for s in ((C,), (C,), (C, C))]
        assert hip.crf_head_ok(h, w, cu, *prm) == ok, C
    args = [t.detach().clone().requires_grad_() for t in (k["h"], k["w"], k["b"], *k["params"])]
    loss, logits = ops.token_crf_head(*args[:3], k["labels"], cu, *args[3:], 0.0, 0)
    loss.backward()
    assert torch.equal(loss.detach(), k["loss"]) and torch.equal(logits, k["logits"])
    assert torch.equal(loss._hsd_pred, k["pred"]) and torch.equal(loss._hsd_stats, k["stats"])
    for a, g in zip(args, k["grads"]):
        assert torch.equal(a.grad, g)


@pytest.mark.parametrize("packed", [False, True])
def test_model_step_vs_fp32_reference_model(gpu, packed):
    """tests/test_gpu_token_head.py's model step with ``use_crf`` at 37 tags: bf16 on the kernels against the same
    weights in fp32 on the reference ops (HSD_OPS=torch), at its tolerances."""
    from huggingface_sagemaker_tensorflow_distributed_amd.data.packing import pack_batch, position_rule

    cfg = resolve_config("hsd-tiny-bert", num_labels=37).replace(hidden_size=128, num_attention_heads=2,
                                                                 intermediate_size=256)
    m32 = build_model(cfg, task=tok.TASK, seed=0, use_crf=True).to(gpu)
    m16 = copy.deepcopy(m32).bfloat16()
    with torch.no_grad():  # the reference holds the bf16-rounded weights
        for p32, p16 in zip(m32.parameters(), m16.parameters()):
            p32.copy_(p16.float())
    ids, mask, labels = tok._batch(cfg, 4, 128)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    kw = dict(input_ids=t(ids), attention_mask=t(mask), labels=t(labels))
    if packed:
        pk = pack_batch(ids, mask, labels, **position_rule(cfg))
        kw = dict(input_ids=t(pk["input_ids"]), labels=t(pk["labels"]), cu_seqlens=t(pk["cu_seqlens"]),
                  max_seqlen=pk["max_seqlen"], position_ids=t(pk["position_ids"]))
    l1, _, g1 = tok._model_step(m16, kw, False)
    l2, _, g2 = tok._model_step(m32, kw, True)
    assert torch.allclose(l1, l2, atol=2e-2, rtol=2e-2), (l1, l2)
    assert "crf_transition_bias" in g1
    for n in g1:
        rel = (g1[n] - g2[n]).norm() / (g2[n].norm() + 1e-6)
        assert rel < 5e-2, f"{n}: rel grad err {rel:.3g}"


def test_whole_step_graph_replay_matches_eager(gpu, monkeypatch):
    """Three optimizer steps of a 2-layer bert-base with the CRF head at 37 tags (B = 16, S = 128) captured and
    replayed as one graph each, against the same steps run eagerly with the same seeds (tests/test_gpu_graph.py's
    bounds): no wide launch path reads a device value on the host."""
    monkeypatch.setenv("HSD_GRAPH_FULL", "1")
    crf_model = lambda cfg, **kw: build_model(cfg.replace(num_labels=37), use_crf=True, **kw)  # noqa: E731
    monkeypatch.setattr(tok, "build_model", crf_model)
    g = torch.Generator().manual_seed(0)
    batches = []
    for _ in range(3):
        labels = torch.randint(0, 37, (16, 128), generator=g)
        labels[torch.rand(16, 128, generator=g) < 0.25] = -100
        batches.append({"input_ids": torch.randint(1000, 30000, (16, 128), generator=g).to(gpu),
                        "attention_mask": torch.ones(16, 128, dtype=torch.long, device=gpu), "labels": labels.to(gpu)})
    res = {}
    for replay in (False, True):
        tr = tok._trainer(gpu, replay)
        assert tr.model.cfg.use_crf and tr.model.cfg.num_labels == 37
        tr.total_steps = 3
        losses = [float(tr.train_step([b])) for b in batches]
        if replay:
            assert len(tr._graphs) == 1 and tr._full_graph
        torch.cuda.synchronize()
        res[replay] = (losses, tr.store.master.clone())
        tr._seed.close()
    (l0, w0), (l1, w1) = res[False], res[True]
    for a, b in zip(l0, l1):
        assert abs(a - b) <= 2e-3 * max(1.0, abs(a)), (l0, l1)
    assert (w0 - w1).norm() / w0.norm() < 1e-4
