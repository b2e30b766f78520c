"""Per-parameter learning-rate multipliers on the GPU (``lr_mul`` of ``adam_step`` / ``lamb_step``, csrc/kernels/adam.hip
and lamb.hip; ``lr_multipliers=`` of FusedAdam / FusedLamb; ``--layerwise_lr_decay`` / ``--head_lr_multiplier``).

Everything at the kernel level is bit for bit, because the rounding is part of the definition: the kernel forms
``step·μ`` and ``lr_wd·μ`` (LAMB: ``lr·μ``) by ONE fp32 multiply each and then runs the expressions it always ran. So a
table of ones gives the bits of no table, and any table gives, on each segment, the bits the kernel WITHOUT a table gives
when launched on that segment alone with the host scalars ``float32(step·μ)``, ``float32(lr_wd·μ)`` (``float32(lr·μ)``).
The trainer-level tests replay each step with one launch over the whole buffer, as tests/test_gpu_e2e.py and
tests/test_gpu_lamb.py do."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 1024
F32 = np.float32


def _hip():
    from huggingface_sagemaker_tensorflow_distributed_amd.ops import hip

    return hip


def f32(x):
    return float(F32(x))


def fmul(a, b):
    """One fp32 multiply of two fp32-rounded scalars, as a Python float."""
    return float(F32(a) * F32(b))


# ------------------------------------------------------------------------------------------ kernel level: the case
STEP, EPS, B1, B2, GSCALE, LR_WD = 1.7e-3, 1e-7, 0.9, 0.999, 1.0 / 3.0, 2e-5
LAMB_LR, LAMB_EPS, LAMB_WD, T_STEP = 2e-3, 1e-6, 0.01, 3
IBC1, IBC2 = 1.0 / (1.0 - B1 ** T_STEP), 1.0 / (1.0 - B2 ** T_STEP)
# one multiplier per segment: distinct, 1.0 among them, one below 2^-10
MU = [0.512, 1.0, 0.64, 1.3 * 2.0 ** -11, 0.8, 4.0, 0.3, 1.7, 0.9, 2.5]
NO_DECAY = (1, 5)  # two segments excluded from decay (and from LAMB's layer adaptation)
TRIP = 2048 * 256 * 8  # elements one trip of adam_kernel's grid-stride loop covers at the full grid


class _Case:
    """A flat buffer of back-to-back 64-aligned segments and a step's state on the CPU: random inside the segments,
    exactly zero in the alignment padding."""

    def __init__(self, lens, mu, no_decay, seed):
        self.lens = list(lens)
        self.mu = [f32(x) for x in mu]
        assert len(self.mu) == len(self.lens) and len(set(self.mu)) == len(self.mu)
        self.decay = [0 if i in no_decay else 1 for i in range(len(lens))]
        self.spans = [(k + 63) // 64 * 64 for k in lens]
        self.offs = [sum(self.spans[:i]) for i in range(len(lens))]
        self.n = sum(self.spans)
        gen = torch.Generator().manual_seed(seed)
        self.w, self.m, self.v, self.g = (torch.zeros(self.n) for _ in range(4))
        for o, k in zip(self.offs, self.lens):
            self.w[o:o + k] = torch.randn(k, generator=gen) * 0.5
            self.m[o:o + k] = torch.randn(k, generator=gen) * 1e-2
            self.v[o:o + k] = torch.rand(k, generator=gen) * 1e-4
            self.g[o:o + k] = torch.randn(k, generator=gen)
        self.mask = torch.zeros(self.n // 64, dtype=torch.uint8)
        self.table = torch.ones(self.n // 64)
        for o, sp, d, x in zip(self.offs, self.spans, self.decay, self.mu):
            self.mask[o // 64:(o + sp) // 64] = d
            self.table[o // 64:(o + sp) // 64] = x
        self.pad = torch.ones(self.n, dtype=torch.bool)
        for o, k in zip(self.offs, self.lens):
            self.pad[o:o + k] = False


@functools.lru_cache(maxsize=None)
def _case():
    tile = _hip().lamb_tile()
    c = _Case([1, 2, 63, 64, 65, 130, 1024, tile - 64, tile + 64, 3 * tile + 192], MU, NO_DECAY, seed=23)
    assert int(c.pad.sum()) > 0 and min(c.mu) < 2.0 ** -10 and 1.0 in c.mu
    return c


@functools.lru_cache(maxsize=None)
def _large_case():
    """2,048·256·8 + 192 elements: the second trip of the grid-stride loop, and its 192-element tail, read the table.
    A segment boundary 128 elements before the end of the first trip, then three 64-element blocks of their own."""
    c = _Case([TRIP - 128, 190, 64, 63], [0.7, 1.9, 1.1 * 2.0 ** -11, 1.0], (2,), seed=29)
    assert c.n == TRIP + 192
    return c


def _guarded(t, gpu, dtype=None):
    """``t`` at offset GUARD of a larger buffer that is NaN everywhere else."""
    dtype = dtype or t.dtype
    big = torch.full((GUARD + t.numel() + GUARD,), NAN, dtype=dtype, device=gpu)
    view = big[GUARD:GUARD + t.numel()]
    if t is not None and t.dtype == dtype:
        view.copy_(t.to(gpu))
    return big, view


def _guards_intact(big):
    return bool(torch.isnan(big[:GUARD]).all()) and bool(torch.isnan(big[-GUARD:]).all())


def _bits(x):
    if x.dtype == torch.bfloat16:
        return x.view(torch.int16)
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _same_bits(a, b, keys):
    for k in keys:
        if a[k] is None:
            assert b[k] is None, k
            continue
        assert torch.equal(_bits(a[k]), _bits(b[k])), k  # raw bits: NaN slots no launch wrote must match too


ADAM_KEYS = ("w", "m", "v", "g", "out", "lo")


def _adam_buffers(case, gpu, grad_dtype, out_kind):
    bigs, views = {}, {}
    for name, t in (("w", case.w), ("m", case.m), ("v", case.v), ("g", case.g.to(grad_dtype))):
        bigs[name], views[name] = _guarded(t, gpu)
    views["out"] = views["lo"] = None
    empty = torch.empty(case.n)
    if out_kind in ("bf16", "halves"):
        bigs["out"], views["out"] = _guarded(empty, gpu, torch.bfloat16)
    if out_kind == "halves":
        bigs["lo"], views["lo"] = _guarded(empty, gpu, torch.bfloat16)
    return bigs, views


def _adam_launch(views, st, e, mask, scalars, device_coef, clip, zero_grad, lr_mul):
    """adam_step on [st, e) of the buffers. ``device_coef``: the scalars travel in the fp32 [4] device tensor and the
    host arguments are garbage."""
    hip = _hip()
    step, lr_wd = scalars
    coef = None
    host = (step, EPS, GSCALE, lr_wd)
    if device_coef:
        coef = torch.tensor([step, EPS, GSCALE, lr_wd], dtype=torch.float32, device=views["w"].device)
        host = (55.0, 3.0, 123.0, 0.25)
    sl = slice(st, e)
    out = views["out"][sl] if views["out"] is not None else None
    lo = views["lo"][sl] if views["lo"] is not None else None
    hip.adam_step(views["w"][sl], views["m"][sl], views["v"][sl], views["g"][sl], out, mask[st // 64:e // 64], host[0],
                  host[1], B1, B2, host[2], host[3], coef, lo, zero_grad=zero_grad, clip=clip, lr_mul=lr_mul)


def _adam_run(gpu, case, table=None, slices=None, grad_dtype=torch.float32, out_kind="bf16", device_coef=False,
              clip=None, zero_grad=False, per_segment=False):
    """One Adam step of ``case``, every buffer embedded in a NaN-filled one. ``table``: the fp32 per-block table (CPU) or
    None; ``slices``: the [st, e) launches (default: one over everything), the table sliced alongside.
    ``per_segment``: instead, the kernel WITHOUT a table on each segment's span alone (those inside ``slices``) with the
    host scalars float32(step·μ), float32(lr_wd·μ) -- the replay the definition names."""
    bigs, views = _adam_buffers(case, gpu, grad_dtype, out_kind)
    mask = case.mask.to(gpu)
    tbig = None
    if table is not None:
        tbig, tview = _guarded(table, gpu)
    cl = torch.tensor([clip], dtype=torch.float32, device=gpu) if clip is not None else None
    for st, e in (slices or [(0, case.n)]):
        if per_segment:
            for o, sp, x in zip(case.offs, case.spans, case.mu):
                if st <= o < e:
                    _adam_launch(views, o, o + sp, mask, (fmul(STEP, x), fmul(LR_WD, x)), False, cl, zero_grad, None)
        else:
            _adam_launch(views, st, e, mask, (STEP, LR_WD), device_coef, cl, zero_grad,
                         tview[st // 64:e // 64] if table is not None else None)
    torch.cuda.synchronize()
    for name, big in bigs.items():
        assert _guards_intact(big), f"{name}: a guard outside the buffer was written"
    if tbig is not None:
        assert _guards_intact(tbig) and torch.equal(tview.cpu(), table)  # the table is read only
    return {k: (v.clone() if v is not None else None) for k, v in views.items()}


# ------------------------------------------------------------------------------------------ kernel level: Adam
@pytest.mark.parametrize("out_kind", [None, "bf16", "halves"])
@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16])
def test_adam_all_ones_table_equals_no_table(gpu, grad_dtype, out_kind):
    case = _case()
    ones = torch.ones(case.n // 64)
    for clip in (None, 0.37):
        for zero_grad in (False, True):
            for device_coef in (False, True):
                kw = dict(grad_dtype=grad_dtype, out_kind=out_kind, device_coef=device_coef, clip=clip,
                          zero_grad=zero_grad)
                a, b = _adam_run(gpu, case, table=ones, **kw), _adam_run(gpu, case, **kw)
                _same_bits(a, b, ADAM_KEYS)
                assert not torch.equal(a["w"].cpu(), case.w)  # the step ran
                assert (int(torch.count_nonzero(a["g"])) == 0) == zero_grad


@pytest.mark.parametrize("device_coef", [False, True])
@pytest.mark.parametrize("out_kind", ["bf16", "halves"])
@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16])
def test_adam_table_equals_the_plain_kernel_per_segment(gpu, grad_dtype, out_kind, device_coef):
    case = _case()
    for clip, zero_grad in ((None, False), (0.37, True)):
        kw = dict(grad_dtype=grad_dtype, out_kind=out_kind, clip=clip, zero_grad=zero_grad)
        got = _adam_run(gpu, case, table=case.table, device_coef=device_coef, **kw)
        want = _adam_run(gpu, case, per_segment=True, **kw)
        _same_bits(got, want, ADAM_KEYS)
        # the gradient is cleared exactly where zero_grad says, the padding is still zero, and the rates are visible
        g = got["g"].cpu()
        assert int(torch.count_nonzero(g)) == 0 if zero_grad else torch.equal(g, case.g.to(grad_dtype))
        for key in ("w", "m", "v", "out"):
            assert int(torch.count_nonzero(got[key].cpu()[case.pad])) == 0, key
        plain = _adam_run(gpu, case, **kw)
        _same_bits(got, plain, ("m", "v"))  # the moments do not see the multipliers
        one = case.mu.index(1.0)
        for i, (o, k) in enumerate(zip(case.offs, case.lens)):
            assert torch.equal(got["w"][o:o + k], plain["w"][o:o + k]) == (i == one), i


@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16])
def test_adam_two_slices_at_an_offset_with_the_table_sliced_alongside(gpu, grad_dtype):
    case = _case()
    st, mid = case.offs[2], case.offs[7]
    slices = [(st, mid), (mid, case.n)]
    kw = dict(grad_dtype=grad_dtype, out_kind="bf16", zero_grad=True, slices=slices)
    got = _adam_run(gpu, case, table=case.table, **kw)
    _same_bits(got, _adam_run(gpu, case, per_segment=True, **kw), ADAM_KEYS)
    # ... which are the bits of the same range in one whole-buffer launch, and nothing ahead of the slices was touched
    whole = _adam_run(gpu, case, table=case.table, grad_dtype=grad_dtype, out_kind="bf16", zero_grad=True)
    for k in ("w", "m", "v", "g", "out"):
        assert torch.equal(_bits(got[k][st:]), _bits(whole[k][st:])), k
    assert torch.equal(got["w"][:st].cpu(), case.w[:st]) and torch.equal(got["m"][:st].cpu(), case.m[:st])
    g = got["g"].cpu()
    assert torch.equal(g[:st], case.g.to(grad_dtype)[:st]) and int(torch.count_nonzero(g[st:])) == 0
    assert bool(torch.isnan(got["out"][:st].float()).all())  # never written


def test_adam_second_trip_and_tail_read_the_table(gpu):
    case = _large_case()
    got = _adam_run(gpu, case, table=case.table, zero_grad=True)
    _same_bits(got, _adam_run(gpu, case, per_segment=True, zero_grad=True), ADAM_KEYS)
    plain = _adam_run(gpu, case, zero_grad=True)
    for i, (o, k) in enumerate(zip(case.offs, case.lens)):
        assert torch.equal(got["w"][o:o + k], plain["w"][o:o + k]) == (case.mu[i] == 1.0), i
    assert case.offs[1] == TRIP - 128 and case.offs[2] == TRIP + 64  # a boundary inside each trip
    assert int(torch.count_nonzero(got["g"])) == 0


# ------------------------------------------------------------------------------------------ kernel level: LAMB
LAMB_KEYS = ("w", "m", "v", "g", "out", "lo", "partials", "ratio")


def _lamb_run(gpu, case, mul=None, per_segment=False, grad_dtype=torch.float32, out_kind="bf16", device_coef=False,
              clip=None, zero_grad=False):
    """One LAMB step of ``case`` in NaN-guarded buffers. ``mul``: the fp32 [segments] table (CPU) or None.
    ``per_segment``: instead, lamb_step WITHOUT a table on each segment alone (seg0 = i, nsegs = 1) with the host scalar
    float32(lr·μ)."""
    hip = _hip()
    plan = hip.lamb_plan(case.offs, case.spans, case.decay, case.n, torch.zeros(1, device=gpu))
    bigs, views = _adam_buffers(case, gpu, grad_dtype, out_kind)
    pad = 5
    pbig = torch.full((pad + 2 * plan.ntiles + pad,), NAN, device=gpu)
    rbig = torch.full((pad + 3 * plan.nsegs + pad,), NAN, device=gpu)
    partials, ratio = pbig[pad:pad + 2 * plan.ntiles], rbig[pad:pad + 3 * plan.nsegs]
    cl = torch.tensor([clip], dtype=torch.float32, device=gpu) if clip is not None else None
    mbig = None
    if mul is not None:
        mbig = torch.full((pad + plan.nsegs + pad,), NAN, device=gpu)
        mview = mbig[pad:pad + plan.nsegs]
        mview.copy_(mul.to(gpu))

    def launch(s0, k, lr, table):
        coef, host = None, (lr, IBC1, IBC2, LAMB_EPS, GSCALE, LAMB_WD)
        if device_coef:
            coef = torch.tensor([lr, IBC1, IBC2, LAMB_EPS, GSCALE, LAMB_WD, NAN, NAN], dtype=torch.float32, device=gpu)
            host = (55.0, 7.0, 0.5, 3.0, 123.0, 9.0)
        hip.lamb_step(plan, s0, k, views["w"], views["m"], views["v"], views["g"], views["out"], views["lo"], partials,
                      ratio, host[0], host[1], host[2], host[3], B1, B2, host[4], host[5], coef, cl, zero_grad,
                      lr_mul=table)

    if per_segment:
        for i, x in enumerate(case.mu):
            launch(i, 1, fmul(LAMB_LR, x), None)
    else:
        launch(0, plan.nsegs, LAMB_LR, mview if mul is not None else None)
    torch.cuda.synchronize()
    for name, big in bigs.items():
        assert _guards_intact(big), f"{name}: a guard outside the buffer was written"
    for big in (pbig, rbig) + ((mbig,) if mbig is not None else ()):
        assert torch.isnan(big[:pad]).all() and torch.isnan(big[-pad:]).all()
    res = {k: (v.clone() if v is not None else None) for k, v in views.items()}
    res.update(partials=partials.clone(), ratio=ratio.clone())
    return res


@pytest.mark.parametrize("device_coef", [False, True])
@pytest.mark.parametrize("out_kind", ["bf16", "halves"])
@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16])
def test_lamb_table_equals_the_plain_step_per_segment_and_leaves_the_ratios(gpu, grad_dtype, out_kind, device_coef):
    case = _case()
    mul = torch.tensor(case.mu)
    kw = dict(grad_dtype=grad_dtype, out_kind=out_kind, zero_grad=True)
    got = _lamb_run(gpu, case, mul=mul, device_coef=device_coef, **kw)
    _same_bits(got, _lamb_run(gpu, case, per_segment=True, **kw), LAMB_KEYS)
    plain = _lamb_run(gpu, case, **kw)
    _same_bits(got, plain, ("m", "v", "g", "partials", "ratio"))  # (r, Σw², Σu²): bit-identical without multipliers
    r = got["ratio"].view(-1, 3)[:, 0].cpu()
    assert all(float(r[i]) == 1.0 for i in NO_DECAY) and sum(float(x) != 1.0 for x in r) == len(case.mu) - len(NO_DECAY)
    one = case.mu.index(1.0)
    for i, (o, k) in enumerate(zip(case.offs, case.lens)):
        assert torch.equal(got["w"][o:o + k], plain["w"][o:o + k]) == (i == one), i
    for key in ("w", "m", "v", "out"):
        assert int(torch.count_nonzero(got[key].cpu()[case.pad])) == 0, key


@pytest.mark.parametrize("clip", [None, 0.37])
@pytest.mark.parametrize("out_kind", [None, "bf16", "halves"])
def test_lamb_all_ones_table_equals_no_table(gpu, out_kind, clip):
    case = _case()
    for grad_dtype in (torch.float32, torch.bfloat16):
        for device_coef in (False, True):
            kw = dict(grad_dtype=grad_dtype, out_kind=out_kind, device_coef=device_coef, clip=clip)
            _same_bits(_lamb_run(gpu, case, mul=torch.ones(len(case.mu)), **kw), _lamb_run(gpu, case, **kw), LAMB_KEYS)


# ------------------------------------------------------------------------------------------ kernel level: arguments
def test_bad_tables_raise_from_the_binding_without_a_launch(gpu):
    hip = _hip()
    case = _case()
    n, nb = case.n, case.n // 64
    plan = hip.lamb_plan(case.offs, case.spans, case.decay, n, torch.zeros(1, device=gpu))
    good_adam = torch.ones(nb, device=gpu)
    good_lamb = torch.ones(plan.nsegs, device=gpu)

    def bad_tables(k):
        return {"fp64": torch.ones(k, dtype=torch.float64, device=gpu),
                "bf16": torch.ones(k, dtype=torch.bfloat16, device=gpu),
                "short": torch.ones(k - 1, device=gpu), "long": torch.ones(k + 1, device=gpu),
                "cpu": torch.ones(k), "strided": torch.ones(2 * k, device=gpu)[::2]}

    def adam(b, table):
        hip.adam_step(b[0], b[1], b[2], b[3], None, None, STEP, EPS, B1, B2, 1.0, 0.0, lr_mul=table)

    def lamb(b, table):
        hip.lamb_step(plan, 0, plan.nsegs, b[0], b[1], b[2], b[3], None, None, torch.zeros(2 * plan.ntiles, device=gpu),
                      torch.zeros(3 * plan.nsegs, device=gpu), LAMB_LR, IBC1, IBC2, LAMB_EPS, B1, B2, 1.0, 0.0,
                      lr_mul=table)

    for call, k, good in ((adam, nb, good_adam), (lamb, plan.nsegs, good_lamb)):
        for what, table in bad_tables(k).items():
            assert what != "strided" or (not table.is_contiguous() and table.numel() == k)
            b = [torch.ones(n, device=gpu) for _ in range(4)]
            with pytest.raises(RuntimeError, match="lr_mul"):
                call(b, table)
            torch.cuda.synchronize()
            assert all(bool((t == 1).all()) for t in b), (call.__name__, what)  # nothing ran
        b = [torch.ones(n, device=gpu) for _ in range(4)]
        call(b, good)
        torch.cuda.synchronize()
        assert not bool((b[0] == 1).all())
    # a slice takes exactly its own blocks: the whole table with half the buffer is refused
    b = [torch.ones(n, device=gpu) for _ in range(4)]
    half = n // 2 // 64 * 64
    with pytest.raises(RuntimeError, match="lr_mul"):
        adam([t[:half] for t in b], good_adam)
    # every call that gave no table keeps working, positional or keyword (tests/test_gpu_lamb.py, test_gpu_e2e.py)
    hip._C.adam_step(b[0], b[1], b[2], b[3], None, None, STEP, EPS, B1, B2, 1.0, 0.0, None, None, False, None)
    hip._C.adam_step(b[0], b[1], b[2], b[3], None, None, STEP, EPS, B1, B2, 1.0, 0.0, zero_grad=True)
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(b[3])) == 0


# ------------------------------------------------------------------------------------------ trainer level
DECAY, HEAD = 0.5, 4.0


def _tiny_cfg(wide=False):
    from huggingface_sagemaker_tensorflow_distributed_amd.models import resolve_config

    cfg = resolve_config("hsd-tiny-bert")
    if wide:  # the shapes tests/test_gpu_lamb.py uses for the fp32 store
        cfg = cfg.replace(hidden_size=256, num_attention_heads=4, intermediate_size=512)
    assert cfg.hidden_dropout_prob > 0 and cfg.attention_probs_dropout_prob > 0  # dropout on
    return cfg


def _tiny_batches(cfg, gpu, n=3, b=4, s=128):
    g = torch.Generator().manual_seed(0)
    out = []
    for _ in range(n):
        am = torch.ones(b, s, dtype=torch.long)
        am[1, 70:] = 0
        out.append({"input_ids": torch.randint(5, cfg.vocab_size, (b, s), generator=g).to(gpu),
                    "attention_mask": am.to(gpu), "labels": torch.randint(0, 2, (b,), generator=g).to(gpu)})
    return out


def _trainer(gpu, cfg, optimizer, dtype="bf16", max_grad_norm=0.0, lr=2e-3, weight_decay=0.01, multipliers=True, **kw):
    from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedAdam, FusedLamb, groups
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore
    from huggingface_sagemaker_tensorflow_distributed_amd.train.trainer import Trainer

    model = build_model(cfg, seed=0).to(gpu)
    model.rng.base_seed = 5
    store = FlatParamStore(model, gpu, compute_dtype=torch.float32 if dtype == "fp32" else torch.bfloat16)
    mul = groups.lr_multipliers(store.names, cfg.num_hidden_layers, DECAY, HEAD) if multipliers else None
    opt = (FusedLamb if optimizer == "lamb" else FusedAdam)(store, lr=lr, weight_decay=weight_decay,
                                                            max_grad_norm=max_grad_norm, lr_multipliers=mul)
    tr = Trainer(model, store, opt, None, gpu, **kw)
    tr._mul = mul
    return tr


def _snapshot(tr):
    return tr.store.master.clone(), tr.optimizer.exp_avg.clone(), tr.optimizer.exp_avg_sq.clone()


def _replay(tr, before):
    """ONE launch over the whole buffer, with the table built here from the names, on the pre-step state and the step's
    final gradients (left in place: zero_grad_in_optimizer off) gives the bits the trainer's step left, however it was
    sliced, overlapped and clipped."""
    hip = _hip()
    st, opt = tr.store, tr.optimizer
    p0, m0, v0 = before
    out = lo = None
    if st.split_hi is not None:
        out, lo = torch.zeros_like(st.split_hi), torch.zeros_like(st.split_lo)
    elif st.compute is not st.master:
        out = torch.zeros_like(st.compute)
    clip = opt._clip_out[1:2] if opt._clip_out is not None else None
    per_segment = [tr._mul[n] for n in st.names]
    if opt.kind == "lamb":
        plan = opt._plan
        partials = torch.zeros(2 * plan.ntiles, device=p0.device)
        ratio = torch.zeros(plan.nsegs, 3, device=p0.device)
        ibc1, ibc2 = opt._coeffs()
        hip.lamb_step(plan, 0, plan.nsegs, p0, m0, v0, st.grad.clone(), out, lo, partials, ratio, opt.lr, ibc1, ibc2,
                      opt.eps, opt.beta1, opt.beta2, 1.0, opt.weight_decay, None, clip,
                      lr_mul=torch.tensor(per_segment, dtype=torch.float32, device=p0.device))
        torch.cuda.synchronize()
        assert torch.equal(ratio[:, 0], opt.last_trust_ratios)
    else:
        step, eps = opt._coeffs()
        table = st.block_table(per_segment)
        assert table.numel() == st.numel // 64 and table.data_ptr() != opt._lr_mul.data_ptr()
        hip.adam_step(p0, m0, v0, st.grad.clone(), out, st.decay_block_mask(64), step, eps, opt.beta1, opt.beta2, 1.0,
                      opt.lr * opt.weight_decay, None, lo, clip=clip, lr_mul=table)
        torch.cuda.synchronize()
    assert torch.equal(p0, st.master) and torch.equal(m0, opt.exp_avg) and torch.equal(v0, opt.exp_avg_sq)
    if lo is not None:
        assert torch.equal(out, st.split_hi) and torch.equal(lo, st.split_lo)
    elif out is not None:
        # the tail of the buffer after the last segment belongs to no LAMB tile and stays the zero it always was
        assert torch.equal(out, st.compute)


@pytest.mark.parametrize("mode", ["overlap", "no_overlap", "clip"])
@pytest.mark.parametrize("optimizer", ["adam", "lamb"])
def test_trainer_steps_equal_one_whole_buffer_replay_with_the_table(gpu, monkeypatch, optimizer, mode):
    monkeypatch.setenv("HSD_OPT_OVERLAP", "0" if mode == "no_overlap" else "1")
    monkeypatch.setenv("HSD_OPT_BUCKET_MB", "0.05")  # several slices of this small model
    monkeypatch.setenv("HSD_WT", "1")
    cfg = _tiny_cfg()
    tr = _trainer(gpu, cfg, optimizer, max_grad_norm=1.0 if mode == "clip" else 0.0)
    opt = tr.optimizer
    assert (tr._opt_overlap is not None) == (mode != "no_overlap")
    if mode != "no_overlap":
        assert len(opt._ranges) > 3
    mul = opt.lr_multipliers()
    L = cfg.num_hidden_layers
    assert mul["classifier_weight"] == HEAD and mul["encoder.embeddings.word_embeddings"] == DECAY ** (L + 1)
    assert mul[f"encoder.layers.{L - 1}.qkv_weight"] == DECAY
    tr.zero_grad_in_optimizer = False  # the replay reads the step's final gradients after the step
    batches = _tiny_batches(cfg, gpu)
    table_at = opt._lr_mul.data_ptr()
    for step in range(3):
        before = _snapshot(tr)
        tr.train_step([batches[step]])
        torch.cuda.synchronize()
        _replay(tr, tuple(t.clone() for t in before))
        assert not torch.equal(before[0], tr.store.master)
    assert opt.step_count == 3 and opt._lr_mul.data_ptr() == table_at
    if mode == "clip":
        assert opt.grad_norm() > 0.0


def test_trainer_steps_with_the_fp32_store_write_the_halves(gpu, monkeypatch):
    monkeypatch.setenv("HSD_OPT_BUCKET_MB", "1")
    cfg = _tiny_cfg(wide=True)
    tr = _trainer(gpu, cfg, "adam", dtype="fp32")
    assert tr.store.split_hi is not None and tr._opt_overlap is not None and len(tr.optimizer._ranges) > 1
    tr.zero_grad_in_optimizer = False
    batches = _tiny_batches(cfg, gpu, n=2)
    for step in range(2):
        before = _snapshot(tr)
        tr.train_step([batches[step]])
        torch.cuda.synchronize()
        _replay(tr, before)


@pytest.mark.parametrize("optimizer", ["adam", "lamb"])
def test_whole_step_graph_replays_the_step_with_the_table(gpu, monkeypatch, optimizer):
    """--hip_graph true against the eager run, with the tolerances of test_gpu_graph.py::test_graph_replay_matches_eager
    (losses 2e-3, weights 1e-4 relative): the captured launches read the table, and a run WITHOUT the table is far
    outside that tolerance, so a replay that dropped it would fail."""
    monkeypatch.setenv("HSD_GRAPH_FULL", "1")
    monkeypatch.setenv("HSD_OPT_BUCKET_MB", "0.05")
    cfg = _tiny_cfg()
    batches = _tiny_batches(cfg, gpu)
    res = {}
    for key, replay, multipliers in (("eager", False, True), ("graph", True, True), ("plain", False, False)):
        tr = _trainer(gpu, cfg, optimizer, multipliers=multipliers, hip_graph=True, lr_schedule="linear",
                      lr_warmup_steps=2)
        tr._graph_replay = replay
        tr.total_steps = 3
        losses = [float(tr.train_step([b]).detach()) for b in batches]
        if replay:
            assert len(tr._graphs) == 1 and tr._full_graph
        assert tr.optimizer.step_count == 3
        torch.cuda.synchronize()
        res[key] = (losses, tr.store.master.clone())
        tr._seed.close()
    (l0, w0), (l1, w1) = res["eager"], res["graph"]
    print("eager", l0, "replay", l1)
    for a, b in zip(l0, l1):
        assert abs(a - b) <= 2e-3 * max(1.0, abs(a)), (l0, l1)
    rel = float((w0 - w1).norm() / w0.norm())
    without = float((w0 - res["plain"][1]).norm() / w0.norm())
    print("eager vs replay", rel, "eager vs no multipliers", without)
    assert rel < 1e-4 and without > 5e-4


def test_one_step_moves_each_parameter_by_its_own_rate(gpu, monkeypatch):
    """From m = v = 0 (Keras eps mode, no decay) Adam's first update of an element with gradient g is

        |Δθ| = step·μ·(1-β1)|g| / (√(1-β2)·|g| + ε) = base·μ / (1 + e),   e = ε / (√(1-β2)·|g|),

    with base = step·(1-β1) / √(1-β2) ≈ lr the same for every element ((1-β) as the kernel forms them, in fp32). So two
    elements' updates differ by the ratio of their μ, times (1 + e_b) / (1 + e_a) in [1 / (1 + e_a), 1 + e_b]. In fp32
    each observed |Δθ| also carries at most 12 roundings, d = 12u relative (g', m, g'², v, the root, the sum, step,
    step·μ, the product, the quotient; u = 2^-24), and u·|θ'| absolute from the final subtraction. Asserted: the observed
    ratio lies within (μ_a / μ_b)·(1 ± 1.01·(e_a + e_b + d_a + d_b)) with d_x = 12u + u·|θ'_x| / |Δθ_x|. The compared
    elements are the ones with the largest |g| of an embedding table and of the classifier weight, where e is
    smallest."""
    monkeypatch.setenv("HSD_OPT_BUCKET_MB", "0.05")
    u = 2.0 ** -24
    cfg = _tiny_cfg()
    lr = 1e-3
    tr = _trainer(gpu, cfg, "adam", lr=lr, weight_decay=0.0)
    st, opt = tr.store, tr.optimizer
    assert opt.eps_mode == "keras" and opt._decay_mask is None
    tr.zero_grad_in_optimizer = False
    before = st.master.clone()
    tr.train_step([_tiny_batches(cfg, gpu, n=1)[0]])
    torch.cuda.synchronize()
    mul, seg = opt.lr_multipliers(), {s.name: s for s in st.segments}
    omb1, omb2 = float(F32(1) - F32(opt.beta1)), float(F32(1) - F32(opt.beta2))
    base = opt._coeffs()[0] * omb1 / omb2 ** 0.5
    assert abs(base / lr - 1.0) < 1e-4
    obs = {}
    for name in ("encoder.embeddings.word_embeddings", "classifier_weight"):
        s = seg[name]
        g = st.grad[s.offset:s.offset + s.numel].double()
        i = int(g.abs().argmax())
        ag = float(g[i].abs())
        e = opt.eps / (omb2 ** 0.5 * ag)
        delta = abs(float(st.master[s.offset + i].double() - before[s.offset + i].double()))
        d = 12 * u + u * abs(float(st.master[s.offset + i])) / delta
        print(f"{name}[{i}]: |g| {ag:.3g} e {e:.3g} |dtheta| {delta:.6g} base*mu {base * mul[name]:.6g} d {d:.3g}")
        assert ag > 1e3 * opt.eps and abs(delta / (base * mul[name]) - 1.0) <= 1.01 * (e + d)
        obs[name] = (delta, e, d)
    (da, ea, d_a), (db, eb, d_b) = obs["classifier_weight"], obs["encoder.embeddings.word_embeddings"]
    want = HEAD / DECAY ** (cfg.num_hidden_layers + 1)
    assert want == 32.0
    assert abs((da / db) / want - 1.0) <= 1.01 * (ea + eb + d_a + d_b), (da / db, want)
