"""Global-norm gradient clipping inside the fused optimizer step (csrc/kernels/gradnorm.hip, optim/adam.py
``max_grad_norm``): the norm kernels against fp64 torch, the clipped Adam against a host-rescaled Adam bit for bit,
and whole trainer steps (overlapped / not, accumulation, captured graph, RCCL engine stream, fp8 / fp32 stores) against
a per-step replay.

Error bound of the device norm. Every term is a non-negative square, so the relative error of a sum is at most
(longest fp32 addition chain + 1) x 2^-24 (the + 1 is the rounding of the square itself; block partials are combined in
fp64, which adds nothing at this scale). grad_sumsq runs at most 512 blocks x 256 threads, and every thread keeps 16
independent accumulators (4 load slots x 4 lanes), so its chain is

    trips (fp32; 2 x trips for bf16: two squares per lane per 16-B chunk)  +  2 (lanes)  +  2 (slots)
    +  6 (wave butterfly)  +  3 (the block's 4 waves)

with trips = ceil(16-B chunks / (blocks x 256 x 4)).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _hip():
    from huggingface_sagemaker_tensorflow_distributed_amd.ops import hip

    return hip


NAN = float("nan")
SIZES = [64, 64 * 1024 + 64, 1048576 + 192]  # under one wave; a tail after full trips; 512 blocks with a tail
# chain at these sizes: one trip everywhere (1,048,768 fp32 = 262,192 chunks < 512 x 256 x 4 slots), so 1 + 13 = 14
# additions for fp32 and 2 + 13 = 15 for bf16 -> bound 16 x 2^-24 = 9.5e-7, inside the 1e-5 asserted
NORM_RTOL = 1e-5


def _slice_in_nan_buffer(n, dtype, gpu, seed):
    """``n`` random gradients at offset 1024 of a larger buffer that is NaN everywhere else: any read outside the
    slice poisons the norm."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((1024 + n + 1024,), NAN, dtype=dtype, device=gpu)
    vals = (torch.randn(n, generator=g) * 0.37).to(dtype)
    buf[1024:1024 + n] = vals.to(gpu)
    return buf, buf[1024:1024 + n], vals.double()


def _norm(hip, slices, gscale, max_norm, gpu, coef=None):
    """grad_sumsq of every slice into consecutive partial ranges of one NaN-filled buffer, then finalize."""
    counts = [hip.grad_sumsq_blocks(s.numel(), s.dtype == torch.bfloat16) for s in slices]
    pad = 5
    partials = torch.full((pad + sum(counts) + pad,), NAN, device=gpu)
    base = pad
    for s, c in zip(slices, counts):
        assert hip.grad_sumsq(s, partials, base) == c
        base += c
    out = torch.full((2,), NAN, device=gpu)
    hip.grad_clip_finalize(partials[pad:], sum(counts), gscale, max_norm, out, coef)
    torch.cuda.synchronize()
    # only the slots of these launches were written
    assert torch.isnan(partials[:pad]).all() and torch.isnan(partials[pad + sum(counts):]).all()
    assert not torch.isnan(partials[pad:pad + sum(counts)]).any()
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", SIZES)
def test_grad_sumsq_and_finalize_match_fp64(gpu, dtype, n):
    hip = _hip()
    _buf, sl, vals = _slice_in_nan_buffer(n, dtype, gpu, seed=n)
    gscale = 1.0 / 3.0
    ref = float(vals.square().sum().sqrt()) * float(np.float32(gscale))
    c = 0.5 * ref
    out = _norm(hip, [sl], gscale, c, gpu)
    norm, coef = float(out[0]), float(out[1])
    print(f"n={n} {dtype}: norm {norm!r} ref {ref!r} rel {abs(norm - ref) / ref:.3g} coef {coef!r}")
    assert abs(norm - ref) <= NORM_RTOL * ref
    assert abs(coef - float(np.float32(c)) / ref) <= NORM_RTOL * coef
    again = _norm(hip, [sl], gscale, c, gpu)
    assert torch.equal(out, again)  # no atomics: bit-reproducible
    # the gradient scale from a captured step's device scalars (coef[2]) instead of the host argument
    dco = torch.tensor([7.0, 7.0, gscale, 7.0], device=gpu)
    assert torch.equal(_norm(hip, [sl], 123.0, c, gpu, coef=dco), out)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_two_slices_finalized_together_equal_their_concatenation(gpu, dtype):
    hip = _hip()
    _b1, s1, v1 = _slice_in_nan_buffer(SIZES[1], dtype, gpu, seed=1)
    _b2, s2, v2 = _slice_in_nan_buffer(SIZES[2], dtype, gpu, seed=2)
    ref = float(torch.cat([v1, v2]).square().sum().sqrt())
    out = _norm(hip, [s1, s2], 1.0, float("inf"), gpu)
    print(f"{dtype}: norm {float(out[0])!r} ref {ref!r}")
    assert abs(float(out[0]) - ref) <= NORM_RTOL * ref
    assert float(out[1]) == 1.0


def test_finalize_edge_cases(gpu):
    """An infinite norm gives coef 0, a NaN norm leaves 1 (the comparison is false), a norm under C leaves 1."""
    hip = _hip()
    out = torch.zeros(2, device=gpu)
    for parts, c, want_norm, want_coef in (([float("inf"), 1.0], 1.0, float("inf"), 0.0),
                                           ([NAN, 1.0], 1.0, NAN, 1.0),
                                           ([9.0, 16.0], 6.0, 5.0, 1.0),
                                           ([9.0, 16.0], 2.5, 5.0, 0.5)):
        hip.grad_clip_finalize(torch.tensor(parts, device=gpu), 2, 1.0, c, out)
        norm, coef = float(out[0]), float(out[1])
        assert (norm != norm) if want_norm != want_norm else norm == want_norm
        assert coef == want_coef
    with pytest.raises(RuntimeError):  # slots outside the partials buffer are refused on the host
        hip.grad_sumsq(torch.zeros(64, device=gpu), torch.zeros(4, device=gpu), 4)
    with pytest.raises(RuntimeError):
        hip.grad_clip_finalize(torch.zeros(4, device=gpu), 5, 1.0, 1.0, out)


# ------------------------------------------------------------------------------------------ adam_step(clip=)
ADAM_N = 64 * 1105  # 64-aligned, no multiple of the 1024-element tile, several blocks


def _adam_state(gpu, n=ADAM_N):
    g = torch.Generator().manual_seed(11)
    p = torch.randn(n, generator=g).to(gpu)
    m = (torch.randn(n, generator=g) * 1e-2).to(gpu)
    v = (torch.rand(n, generator=g) * 1e-4).to(gpu)
    grad = torch.randn(n, generator=g).to(gpu)
    decay = (torch.rand(n // 64, generator=g) < 0.5).to(torch.uint8).to(gpu)
    return p, m, v, grad, decay


def _adam(hip, state, gscale, clip=None, zero_grad=False, coef=None):
    p, m, v, grad, decay = (t.clone() for t in state)
    out = torch.empty(p.numel(), dtype=torch.bfloat16, device=p.device)
    hip.adam_step(p, m, v, grad, out, decay, 1e-3, 1e-7, 0.9, 0.999, gscale, 1e-5, coef, None, zero_grad=zero_grad,
                  clip=clip)
    torch.cuda.synchronize()
    return p, m, v, out, grad


@pytest.mark.parametrize("zero_grad", [False, True])
@pytest.mark.parametrize("device_coef", [False, True])
def test_clipped_adam_is_exactly_a_rescaled_adam(gpu, zero_grad, device_coef):
    hip = _hip()
    state = _adam_state(gpu)
    gscale = 1.0 / 3.0
    norm0 = float(state[3].double().square().sum().sqrt()) * gscale
    ws = _norm(hip, [state[3]], gscale, 0.5 * norm0, gpu)
    coef = float(ws[1])
    assert 0.49 < coef < 0.51
    host_scale = float(np.float32(gscale) * np.float32(coef))
    if device_coef:  # the step's scalars on the device (captured steps): host arguments are ignored
        a = _adam(hip, state, 55.0, clip=ws[1:2], zero_grad=zero_grad,
                  coef=torch.tensor([1e-3, 1e-7, gscale, 1e-5], device=gpu))
        b = _adam(hip, state, 55.0, zero_grad=zero_grad, coef=torch.tensor([1e-3, 1e-7, host_scale, 1e-5], device=gpu))
    else:
        a = _adam(hip, state, gscale, clip=ws[1:2], zero_grad=zero_grad)
        b = _adam(hip, state, host_scale, zero_grad=zero_grad)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert (int(torch.count_nonzero(a[4])) == 0) == zero_grad
    unclipped = _adam(hip, state, gscale)
    assert not torch.equal(unclipped[0], a[0])


@pytest.mark.parametrize("c", [float("inf"), 1e30])
def test_never_clipping_is_bit_identical_to_no_clip(gpu, c):
    hip = _hip()
    state = _adam_state(gpu)
    ws = _norm(hip, [state[3]], 0.25, c, gpu)
    assert float(ws[1]) == 1.0 and float(ws[0]) > 0
    a = _adam(hip, state, 0.25, clip=ws[1:2])
    b = _adam(hip, state, 0.25)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------ trainer level
def _batches(gpu, n=4, b=8):
    from huggingface_sagemaker_tensorflow_distributed_amd import data as hdata

    ds = hdata.synthetic_classification(b * n, 128, 30522, seed=0)
    return [{k: torch.from_numpy(v[b * i:b * (i + 1)]).long().to(gpu) for k, v in
             (("input_ids", ds.input_ids), ("attention_mask", ds.attention_mask), ("labels", ds.labels))}
            for i in range(n)]


def _first_norm_then_reset(tr, st, opt, mbs):
    """The first step's gradient norm, measured with C = inf (never clips) on this very trainer, which is then put
    back to its initial state."""
    assert opt.max_grad_norm == float("inf")
    p_init = st.master.clone()
    tr.train_step(mbs)
    norm = opt.grad_norm()
    assert float(opt.last_clip_coef) == 1.0 and 0 < norm < float("inf")
    st.load_master(p_init)
    opt.exp_avg.zero_()
    opt.exp_avg_sq.zero_()
    opt.step_count = 0
    tr.global_step = 0
    return norm


def _check_clipped_step(hip, st, opt, before, gscale, c):
    """After a trainer step that left the raw gradients in place: the device norm against fp64, the device coef, and
    master / moments / compute copies against ONE adam_step replay on the pre-step state with gscale x coef.

    Chain bound of the norm here: the whole 110M-element fp32 buffer as one slice is 53 trips + 13 = 66 additions
    (4 MiB slices: the 23M-element embedding slice, 12 trips + 13), so at most 67 x 2^-24 = 4e-6 < the 1e-4 asserted."""
    p0, m0, v0 = before
    norm, coef = opt.grad_norm(), float(opt.last_clip_coef)
    ref = float(st.grad.double().square().sum().sqrt()) * float(np.float32(gscale))
    print(f"norm {norm!r} ref {ref!r} rel {abs(norm - ref) / ref:.3g} coef {coef!r} C {c!r}")
    assert abs(norm - ref) <= 1e-4 * ref
    want = float(np.float32(c)) / norm if norm > float(np.float32(c)) else 1.0
    assert abs(coef - want) <= 2.0 ** -22 * want  # fp32 rounding of norm and of coef
    s, eps = opt._coeffs()
    out = lo = None
    if st.split_hi is not None:
        out, lo = torch.empty_like(st.split_hi), torch.empty_like(st.split_lo)
    elif st.compute is not st.master:
        out = torch.empty_like(st.compute)
    hip.adam_step(p0, m0, v0, st.grad, out, None, s, eps, opt.beta1, opt.beta2,
                  float(np.float32(gscale) * np.float32(coef)), 0.0, None, lo)
    torch.cuda.synchronize()
    assert torch.equal(p0, st.master) and torch.equal(m0, opt.exp_avg) and torch.equal(v0, opt.exp_avg_sq)
    if lo is not None:
        assert torch.equal(out, st.split_hi) and torch.equal(lo, st.split_lo)
    elif out is not None:
        assert torch.equal(out, st.compute)
    for p in st.params:
        if hasattr(p, "_hsd_wt"):
            assert torch.equal(p._hsd_wt, p.detach().t())
    return coef


def _run_clipped_steps(hip, tr, st, opt, batches, accum, steps=3):
    tr.zero_grad_in_optimizer = False  # the replay reads the step's final gradients after the step
    c = 0.5 * _first_norm_then_reset(tr, st, opt, batches[:accum])
    opt.max_grad_norm = c
    for step in range(steps):
        before = (st.master.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone())
        tr.train_step([batches[(step * accum + j) % len(batches)] for j in range(accum)])
        torch.cuda.synchronize()
        coef = _check_clipped_step(hip, st, opt, before, 1.0 / accum, c)
        if step == 0:
            assert coef < 0.75  # half the norm this same step had a moment ago: certainly clipped


@pytest.mark.parametrize("overlap", ["1", "0"])
@pytest.mark.parametrize("accum", [1, 2])
def test_trainer_steps_clip_by_the_global_norm(gpu, monkeypatch, accum, overlap):
    from huggingface_sagemaker_tensorflow_distributed_amd.train.runner import build
    from huggingface_sagemaker_tensorflow_distributed_amd.utils.args import build_parser

    hip = _hip()
    monkeypatch.setenv("HSD_OPT_OVERLAP", overlap)
    monkeypatch.setenv("HSD_OPT_BUCKET_MB", "4")  # many slices
    monkeypatch.setenv("HSD_WT", "1")  # keep the Wᵀ copies at this small step
    args, _ = build_parser("train").parse_known_args(
        ["--model_name_or_path", "bert-base-uncased", "--train_batch_size", "8", "--learning_rate", "1e-4",
         "--dtype", "bf16", "--log_every", "0", "--hip_graph", "false", "--seed", "3", "--max_grad_norm", "inf"])
    parts = build(args, "train")
    tr, st, opt = parts["trainer"], parts["store"], parts["optimizer"]
    assert (tr._opt_overlap is not None) == (overlap == "1")
    if overlap == "1":
        assert len(opt._ranges) > 10 and len(opt._clip_bases) == len(opt._ranges)
    assert len([p for p in st.params if hasattr(p, "_hsd_wt")]) == 48
    _run_clipped_steps(hip, tr, st, opt, _batches(gpu), accum)


def test_clipped_steps_on_the_engine_stream(gpu, monkeypatch):
    """Data-parallel form: each bucket's sum of squares runs on the RCCL engine's stream right after the bucket's
    all-reduce (world-of-one communicator)."""
    from huggingface_sagemaker_tensorflow_distributed_amd.ops._ext import load
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import GradBucketer
    from huggingface_sagemaker_tensorflow_distributed_amd.train.runner import build
    from huggingface_sagemaker_tensorflow_distributed_amd.train.trainer import Trainer
    from huggingface_sagemaker_tensorflow_distributed_amd.utils.args import build_parser

    hip = _hip()
    monkeypatch.setenv("HSD_OPT_OVERLAP", "1")
    monkeypatch.setenv("HSD_WT", "1")
    args, _ = build_parser("train").parse_known_args(
        ["--model_name_or_path", "bert-base-uncased", "--train_batch_size", "8", "--dtype", "bf16",
         "--learning_rate", "1e-4", "--log_every", "0", "--hip_graph", "false", "--max_grad_norm", "inf"])
    parts = build(args, "train")
    model, st, opt = parts["model"], parts["store"], parts["optimizer"]
    C = load()
    eng = C.CommEngine(0, 1, C.CommEngine.unique_id(), gpu.index, True)
    buck = GradBucketer(st, bucket_mb=4, engine=eng)
    tr = Trainer(model, st, opt, buck, gpu)
    assert tr._opt_overlap == "engine" and len(opt._clip_bases) == len(buck.buckets) > 10
    _run_clipped_steps(hip, tr, st, opt, _batches(gpu, n=2), 1)
    assert eng.launched_count() == len(buck.buckets)


@pytest.mark.parametrize("dtype", ["fp8", "fp32"])
def test_clipped_steps_with_fp8_and_fp32_stores(gpu, monkeypatch, dtype):
    from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model, resolve_config
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedAdam
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore
    from huggingface_sagemaker_tensorflow_distributed_amd.train.trainer import Trainer

    hip = _hip()
    monkeypatch.setenv("HSD_OPT_BUCKET_MB", "1")
    cfg = resolve_config("hsd-tiny-bert").replace(hidden_size=256, num_attention_heads=4, intermediate_size=512)
    m = build_model(cfg, seed=0).to(gpu)
    g = torch.Generator().manual_seed(0)
    batches = [{"input_ids": torch.randint(5, cfg.vocab_size, (4, 128), generator=g).to(gpu),
                "attention_mask": torch.ones(4, 128, dtype=torch.long, device=gpu),
                "labels": torch.randint(0, 2, (4,), generator=g).to(gpu)} for _ in range(2)]
    fp8 = dtype == "fp8"
    if fp8:
        hip.set_fp8(True)
    try:
        st = FlatParamStore(m, gpu, compute_dtype=torch.bfloat16 if fp8 else torch.float32, fp8=fp8)
        opt = FusedAdam(st, lr=1e-4, max_grad_norm=float("inf"))
        tr = Trainer(m, st, opt, None, gpu)
        assert tr._opt_overlap is not None and len(opt._ranges) > 1
        assert (st.split_hi is not None) == (not fp8)
        tr.zero_grad_in_optimizer = False
        c = 0.5 * _first_norm_then_reset(tr, st, opt, batches[:1])
        opt.max_grad_norm = c
        for step in range(2):
            before = (st.master.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone())
            tr.train_step([batches[step]])
            torch.cuda.synchronize()
            _check_clipped_step(hip, st, opt, before, 1.0, c)
            if fp8:  # the fp8 weight copies were re-quantised from the updated weights at the end of the step
                q, qt, si = st.fp8_w.clone(), st.fp8_wt.clone(), st.fp8_sinv.clone()
                st.refresh_fp8()
                torch.cuda.synchronize()
                assert torch.equal(q, st.fp8_w) and torch.equal(qt, st.fp8_wt) and torch.equal(si, st.fp8_sinv)
    finally:
        if fp8:
            hip.set_fp8(False)


# ------------------------------------------------------------------------------------------ whole-step graph
def _graph_trainer(gpu, graph_replay, max_grad_norm):
    from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model, resolve_config
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedAdam
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore
    from huggingface_sagemaker_tensorflow_distributed_amd.train.trainer import Trainer

    cfg = resolve_config("bert-base-uncased").replace(num_hidden_layers=2)
    model = build_model(cfg, seed=0).to(gpu)
    model.rng.base_seed = 5
    store = FlatParamStore(model, gpu, compute_dtype=torch.bfloat16)
    opt = FusedAdam(store, lr=1e-4, weight_decay=0.01, max_grad_norm=max_grad_norm)
    tr = Trainer(model, store, opt, None, gpu, hip_graph=True, lr_schedule="linear", lr_warmup_steps=2)
    tr._graph_replay = graph_replay
    tr.total_steps = 3
    return tr


def test_whole_step_graph_replays_the_clipped_step(gpu, monkeypatch):
    """The setup and tolerances of test_gpu_graph.py::test_graph_replay_matches_eager (losses 2e-3, weights 1e-4
    relative) with clipping on: the norm, finalize and clipped Adam launches are captured with the step, and every
    replay computes its own norm and coefficient on the device."""
    monkeypatch.setenv("HSD_GRAPH_FULL", "1")
    g = torch.Generator().manual_seed(0)
    batches = []
    for _ in range(3):
        ids = torch.randint(1000, 30000, (16, 128), generator=g)
        am = torch.ones(16, 128, dtype=torch.long)
        am[3, 70:] = 0
        batches.append({"input_ids": ids.to(gpu), "attention_mask": am.to(gpu),
                        "labels": torch.randint(0, 2, (16,), generator=g).to(gpu)})
    # the first step's norm, from an eager trainer that never clips
    tr = _graph_trainer(gpu, False, float("inf"))
    tr.train_step([batches[0]])
    c = 0.5 * tr.optimizer.grad_norm()
    tr._seed.close()
    res = {}
    for replay in (False, True):
        tr = _graph_trainer(gpu, replay, c)
        losses, norms, coefs = [], [], []
        for b in batches:
            losses.append(float(tr.train_step([b])))
            norms.append(tr.optimizer.grad_norm())
            coefs.append(float(tr.optimizer.last_clip_coef))
        if replay:
            assert len(tr._graphs) == 1 and tr._full_graph
        assert tr.optimizer.step_count == 3
        torch.cuda.synchronize()
        res[replay] = (losses, tr.store.master.clone(), norms, coefs)
        tr._seed.close()
    (l0, w0, n0, c0), (l1, w1, n1, c1) = res[False], res[True]
    print("eager", l0, n0, c0, "replay", l1, n1, c1)
    for a, b in zip(l0, l1):
        assert abs(a - b) <= 2e-3 * max(1.0, abs(a)), (l0, l1)
    rel = (w0 - w1).norm() / w0.norm()
    assert rel < 1e-4, float(rel)
    assert c0[0] < 0.75 and c1[0] < 0.75  # clipping was active
    # the coefficient is not frozen into the graph: every replayed step has its own norm (and coef = C / norm)
    assert len(set(n1)) == 3, n1
    for n, k in zip(n1, c1):
        want = float(np.float32(c)) / n if n > float(np.float32(c)) else 1.0
        assert abs(k - want) <= 2.0 ** -22 * want
