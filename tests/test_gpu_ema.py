"""The weight average on the GPU (``ema`` / ``ema_omd`` of ``adam_step`` / ``lamb_step``, csrc/kernels/adam.hip and
lamb.hip; ``ema_decay=`` of FusedAdam / FusedLamb; ``--ema_decay`` / ``--ema_warmup``).

The rounding is part of the definition: ``ema <- e + w·(θ - e)`` is three separately rounded fp32 operations on the
weight the launch wrote, so everything at the kernel level is bit for bit against the torch fp32 replay
``e + w * (p_new - e)``, and every other buffer a launch writes holds the bits of the launch without ``ema``. The
structure follows tests/test_gpu_lr_groups.py (NaN-guarded buffers, one whole-buffer replay of the trainer's steps)."""
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


# ------------------------------------------------------------------------------------------ kernel level: the case
STEP, EPS, B1, B2, GSCALE, LR_WD = 1.7e-3, 1e-7, 0.9, 0.999, 1.0 / 3.0, 2e-5
LAMB_LR, LAMB_EPS, LAMB_WD, T_STEP = 2e-3, 1e-6, 0.01, 3
IBC1, IBC2 = 1.0 / (1.0 - B1 ** T_STEP), 1.0 / (1.0 - B2 ** T_STEP)
NO_DECAY = (1, 5)
TRIP = 2048 * 256 * 2 * 4  # elements one trip of adam_kernel's grid-stride loop covers at the full grid
# 1 - 0.999 (the usual decay), the first warm-up step (d_0 = 0.1), and 0 (the average must not move)
OMEGAS = (1.0 - 0.999, 0.9, 0.0)


class _Case:
    """A flat buffer of back-to-back 64-aligned segments padded to a multiple of 1,024 (FlatParamStore's layout) and a
    step's state on the CPU: random in the normal fp32 range inside the segments, zero in the alignment padding and the
    tail. ``e`` is the average before the step: near the weights, as after some steps."""

    def __init__(self, lens, no_decay, seed):
        self.lens = list(lens)
        self.decay = [0 if i in no_decay else 1 for i in range(len(lens))]
        self.spans = [(k + 63) // 64 * 64 for k in lens]
        self.offs = [sum(self.spans[:i]) for i in range(len(lens))]
        self.n = (sum(self.spans) + 1023) // 1024 * 1024
        gen = torch.Generator().manual_seed(seed)
        self.w, self.m, self.v, self.g, self.e = (torch.zeros(self.n) for _ in range(5))
        for o, k in zip(self.offs, self.lens):
            self.w[o:o + k] = torch.randn(k, generator=gen) * 0.5
            self.m[o:o + k] = torch.randn(k, generator=gen) * 1e-2
            self.v[o:o + k] = torch.rand(k, generator=gen) * 1e-4
            self.g[o:o + k] = torch.randn(k, generator=gen)
            self.e[o:o + k] = self.w[o:o + k] + torch.randn(k, generator=gen) * 1e-2
        self.mask = torch.zeros(self.n // 64, dtype=torch.uint8)
        self.table = torch.ones(self.n // 64)  # a learning-rate multiplier per 64-element block (adam_step's lr_mul)
        self.mu = [0.5 + 0.25 * i for i in range(len(lens))]
        for o, sp, d, x in zip(self.offs, self.spans, self.decay, self.mu):
            self.mask[o // 64:(o + sp) // 64] = d
            self.table[o // 64:(o + sp) // 64] = x
        for t in (self.w, self.e):
            inside = t[t != 0].abs()
            assert float(inside.min()) > 2.0 ** -126 and bool(torch.isfinite(t).all())  # normal fp32 values


@functools.lru_cache(maxsize=None)
def _case():
    tile = _hip().lamb_tile()
    assert tile == 4096
    # 64 .. one LAMB tile, one tile + 64, two tiles + 64, and two that end inside a 64-element block
    c = _Case([64, 192, 1024, tile, tile + 64, 2 * tile + 64, 130, 3 * tile + 321], NO_DECAY, seed=31)
    assert c.n % 1024 == 0 and c.n > sum(c.spans)  # a tail that belongs to no segment
    return c


@functools.lru_cache(maxsize=None)
def _large_case():
    """Past one grid-stride trip of adam_kernel (2,048 x 256 x 2 x 4 = 4,194,304 elements) plus a 1,024-element tail
    that is no multiple of the trip; a segment boundary 128 elements before the end of the first trip."""
    c = _Case([TRIP - 128, 190, 64, 63, 600], (2,), seed=37)
    assert c.n == TRIP + 1024
    return c


def _guarded(t, gpu, dtype=None):
    """``t`` at offset GUARD of a larger buffer that is NaN everywhere else (the canary margins)."""
    dtype = dtype or t.dtype
    big = torch.full((GUARD + t.numel() + GUARD,), NAN, dtype=dtype, device=gpu)
    view = big[GUARD:GUARD + t.numel()]
    if t.dtype == dtype:
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


def _replay(e, w, p_new):
    """The definition in torch fp32: a subtract, a multiply by float32(w), an add, each rounded."""
    return e + torch.tensor(w, dtype=torch.float32, device=e.device) * (p_new - e)


STEP_KEYS = ("w", "m", "v", "g", "out", "lo")


def _buffers(case, gpu, grad_dtype, out_kind, with_ema):
    bigs, views = {}, {}
    for name, t in (("w", case.w), ("m", case.m), ("v", case.v), ("g", case.g.to(grad_dtype))):
        bigs[name], views[name] = _guarded(t, gpu)
    views["out"] = views["lo"] = views["e"] = None
    empty = torch.empty(case.n)
    if out_kind in ("bf16", "halves"):
        bigs["out"], views["out"] = _guarded(empty, gpu, torch.bfloat16)
    if out_kind == "halves":
        bigs["lo"], views["lo"] = _guarded(empty, gpu, torch.bfloat16)
    if with_ema:
        bigs["e"], views["e"] = _guarded(case.e, gpu)
    return bigs, views


def _check_guards(bigs):
    torch.cuda.synchronize()
    for name, big in bigs.items():
        assert _guards_intact(big), f"{name}: a canary outside the buffer was written"


def _adam_run(gpu, case, omega=None, slices=None, grad_dtype=torch.float32, out_kind="bf16", device_coef=False,
              clip=None, zero_grad=False, table=False):
    """One Adam step of ``case`` in NaN-guarded buffers, as the [st, e) launches ``slices`` (default: one over
    everything) with ``ema`` sliced alongside. ``omega``: 1 - decay, None = no ``ema``. ``device_coef``: the scalars,
    ``omega`` among them (slot 4 of fp32 [8]), travel on the device and the host arguments are garbage."""
    hip = _hip()
    bigs, views = _buffers(case, gpu, grad_dtype, out_kind, omega is not None)
    mask = case.mask.to(gpu)
    tab = case.table.to(gpu) if table else None
    cl = torch.tensor([clip], dtype=torch.float32, device=gpu) if clip is not None else None
    coef, host, host_w = None, (STEP, EPS, GSCALE, LR_WD), omega
    if device_coef:
        coef = torch.tensor([STEP, EPS, GSCALE, LR_WD, omega if omega is not None else NAN, NAN, NAN, NAN],
                            dtype=torch.float32, device=gpu)
        host, host_w = (55.0, 3.0, 123.0, 0.25), 0.5
    for st, e in (slices or [(0, case.n)]):
        sl = slice(st, e)
        kw = {}
        if omega is not None:
            kw = {"ema": views["e"][sl], "ema_omd": host_w}
        hip.adam_step(views["w"][sl], views["m"][sl], views["v"][sl], views["g"][sl],
                      views["out"][sl] if views["out"] is not None else None, mask[st // 64:e // 64], host[0], host[1],
                      B1, B2, host[2], host[3], coef, views["lo"][sl] if views["lo"] is not None else None,
                      zero_grad=zero_grad, clip=cl, lr_mul=tab[st // 64:e // 64] if table else None, **kw)
        _check_guards(bigs)  # after every launch
    return {k: (v.clone() if v is not None else None) for k, v in views.items()}


LAMB_KEYS = STEP_KEYS + ("partials", "ratio")


def _lamb_run(gpu, case, omega=None, seg_slices=None, grad_dtype=torch.float32, out_kind="bf16", device_coef=False,
              clip=None, zero_grad=False, table=False):
    """One LAMB step of ``case`` in NaN-guarded buffers, as the (seg0, nsegs) launches ``seg_slices`` (default: one over
    every segment); LAMB addresses by tile, so every launch takes the whole buffers, ``ema`` included."""
    hip = _hip()
    plan = hip.lamb_plan(case.offs, case.spans, case.decay, case.n, torch.zeros(1, device=gpu))
    bigs, views = _buffers(case, gpu, grad_dtype, out_kind, omega is not None)
    bigs["partials"] = torch.full((GUARD + 2 * plan.ntiles + GUARD,), NAN, device=gpu)
    bigs["ratio"] = torch.full((GUARD + 3 * plan.nsegs + GUARD,), NAN, device=gpu)
    partials, ratio = bigs["partials"][GUARD:-GUARD], bigs["ratio"][GUARD:-GUARD]
    cl = torch.tensor([clip], dtype=torch.float32, device=gpu) if clip is not None else None
    tab = torch.tensor(case.mu, dtype=torch.float32, device=gpu) if table else None
    coef, host, host_w = None, (LAMB_LR, IBC1, IBC2, LAMB_EPS, GSCALE, LAMB_WD), omega
    if device_coef:
        coef = torch.tensor([LAMB_LR, IBC1, IBC2, LAMB_EPS, GSCALE, LAMB_WD, omega if omega is not None else NAN, NAN],
                            dtype=torch.float32, device=gpu)
        host, host_w = (55.0, 7.0, 0.5, 3.0, 123.0, 9.0), 0.5
    kw = {"ema": views["e"], "ema_omd": host_w} if omega is not None else {}
    for s0, k in (seg_slices or [(0, plan.nsegs)]):
        hip.lamb_step(plan, s0, k, views["w"], views["m"], views["v"], views["g"], views["out"], views["lo"], partials,
                      ratio, host[0], host[1], host[2], host[3], B1, B2, host[4], host[5], coef, cl, zero_grad,
                      lr_mul=tab, **kw)
        _check_guards(bigs)
    res = {k: (v.clone() if v is not None else None) for k, v in views.items()}
    res.update(partials=partials.clone(), ratio=ratio.clone())
    return res


RUNS = {"adam": (_adam_run, STEP_KEYS), "lamb": (_lamb_run, LAMB_KEYS)}


# ------------------------------------------------------------------------------------------ 1. the step is undisturbed
@pytest.mark.parametrize("out_kind", [None, "bf16", "halves"])
@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("optimizer", ["adam", "lamb"])
def test_the_step_writes_the_same_bits_with_and_without_ema(gpu, optimizer, grad_dtype, out_kind):
    case = _case()
    run, keys = RUNS[optimizer]
    for zero_grad in (False, True):
        kw = dict(grad_dtype=grad_dtype, out_kind=out_kind, zero_grad=zero_grad)
        with_ema, without = run(gpu, case, omega=1.0 - 0.999, **kw), run(gpu, case, **kw)
        _same_bits(with_ema, without, keys)  # p, m, v, the outputs, the cleared gradient, LAMB's partials and ratios
        assert not torch.equal(without["w"].cpu(), case.w)  # the step ran
        assert (int(torch.count_nonzero(with_ema["g"][:sum(case.spans)])) == 0) == zero_grad
        assert not torch.equal(with_ema["e"].cpu(), case.e)  # ... and so did the average


# ------------------------------------------------------------------------------------------ 2. the definition
def _check_definition(case, got, omega, gpu):
    e0 = case.e.to(gpu)
    want = _replay(e0, omega, got["w"])
    assert torch.equal(_bits(got["e"]), _bits(want))
    if omega == 0.0:
        assert torch.equal(_bits(got["e"]), _bits(e0))  # the bits did not move
    else:
        assert not torch.equal(got["e"], e0)


@pytest.mark.parametrize("device_coef", [False, True])
@pytest.mark.parametrize("out_kind", [None, "bf16", "halves"])
@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("optimizer", ["adam", "lamb"])
def test_the_average_is_the_three_operation_formula(gpu, optimizer, grad_dtype, out_kind, device_coef):
    case = _case()
    run, _ = RUNS[optimizer]
    for omega in OMEGAS:
        got = run(gpu, case, omega=omega, grad_dtype=grad_dtype, out_kind=out_kind, device_coef=device_coef)
        _check_definition(case, got, omega, gpu)


@pytest.mark.parametrize("device_coef", [False, True])
@pytest.mark.parametrize("optimizer", ["adam", "lamb"])
def test_the_formula_with_the_clip_pointer_and_the_lr_table(gpu, optimizer, device_coef):
    """The kClip and kLrMul instantiations of the kEma kernels: the average follows the weight THEY wrote, and the step
    is still the step without ``ema``."""
    case = _case()
    run, keys = RUNS[optimizer]
    for clip, table in ((0.37, False), (None, True), (0.37, True)):
        kw = dict(out_kind="bf16", device_coef=device_coef, clip=clip, table=table, zero_grad=True)
        plain = run(gpu, case, **kw)
        for omega in OMEGAS:
            got = run(gpu, case, omega=omega, **kw)
            _check_definition(case, got, omega, gpu)
            _same_bits(got, plain, keys)
        assert not torch.equal(plain["w"], run(gpu, case, out_kind="bf16", zero_grad=True)["w"])  # clip / table seen


# ------------------------------------------------------------------------------------------ 3. slices
@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16])
def test_adam_two_slices_at_an_offset_equal_the_whole_buffer_launch(gpu, grad_dtype):
    case = _case()
    omega = 1.0 - 0.999
    st, mid, end = case.offs[2], case.offs[5], case.offs[7]
    kw = dict(omega=omega, grad_dtype=grad_dtype, out_kind="halves", zero_grad=True)
    got = _adam_run(gpu, case, slices=[(st, mid), (mid, end)], **kw)
    whole = _adam_run(gpu, case, **kw)
    for k in STEP_KEYS + ("e",):
        assert torch.equal(_bits(got[k][st:end]), _bits(whole[k][st:end])), k
    # nothing outside [st, end) was written, in any buffer
    outside = torch.ones(case.n, dtype=torch.bool)
    outside[st:end] = False
    for k, t in (("w", case.w), ("m", case.m), ("v", case.v), ("g", case.g.to(grad_dtype)), ("e", case.e)):
        assert torch.equal(_bits(got[k].cpu()[outside]), _bits(t[outside])), k
    for k in ("out", "lo"):
        assert bool(torch.isnan(got[k].float()[outside.to(gpu)]).all()), k  # never written


@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16])
def test_lamb_two_segment_ranges_equal_the_whole_buffer_launch(gpu, grad_dtype):
    case = _case()
    omega = 1.0 - 0.999
    kw = dict(omega=omega, grad_dtype=grad_dtype, out_kind="halves", zero_grad=True)
    got = _lamb_run(gpu, case, seg_slices=[(2, 3), (5, 2)], **kw)  # segments 2 .. 6
    whole = _lamb_run(gpu, case, **kw)
    st, end = case.offs[2], case.offs[7]
    for k in STEP_KEYS + ("e",):
        assert torch.equal(_bits(got[k][st:end]), _bits(whole[k][st:end])), k
    assert torch.equal(_bits(got["ratio"][6:21]), _bits(whole["ratio"][6:21]))
    outside = torch.ones(case.n, dtype=torch.bool)
    outside[st:end] = False
    for k, t in (("w", case.w), ("m", case.m), ("v", case.v), ("g", case.g.to(grad_dtype)), ("e", case.e)):
        assert torch.equal(_bits(got[k].cpu()[outside]), _bits(t[outside])), k
    for k in ("out", "lo"):
        assert bool(torch.isnan(got[k].float()[outside.to(gpu)]).all()), k
    assert bool(torch.isnan(got["ratio"][:6]).all()) and bool(torch.isnan(got["ratio"][21:]).all())


# ------------------------------------------------------------------------------------------ 4. second trip and tail
@pytest.mark.parametrize("optimizer", ["adam", "lamb"])
def test_second_trip_and_tail(gpu, optimizer):
    case = _large_case()
    run, keys = RUNS[optimizer]
    omega = 1.0 - 0.999
    got = run(gpu, case, omega=omega, zero_grad=True)
    _check_definition(case, got, omega, gpu)  # every element
    _same_bits(got, run(gpu, case, zero_grad=True), keys)
    moved = got["e"].cpu() != case.e
    for o, k in zip(case.offs, case.lens):  # ... and it moved in every segment, on both sides of the trip boundary
        assert int(moved[o:o + k].sum()) > k // 2, o
    assert case.offs[1] == TRIP - 128 and case.offs[2] == TRIP + 64


# ------------------------------------------------------------------------------------------ 5. against fp64
def test_fifty_adam_launches_against_an_fp64_average(gpu):
    """50 consecutive launches at d = 0.9 against the fp64 average (same w = float32(1 - d)) of the fp32 weight
    trajectory the launches produced.

    The bound, derived: one update is e' = fl(e + fl(w·fl(θ - e))). With u = 2⁻²⁴ and M = max(|θ|, |e|, |e'|): the
    subtract errs by at most u·|θ - e| <= 2uM, which the product scales by w; the product errs by at most
    u·w·|θ - e| <= 2uwM; the sum by at most u·|e'| <= uM. Together (1 + 4w)·uM, which is <= 3uM for every w <= 1/2 and
    here (w = 0.1) 1.4·uM. The error the average carried into the step is multiplied by (1 - w) = d. So after step t
    the error is at most B_t = d·B_{t-1} + 3·u·M_t, B_0 = 0: the per-step term summed geometrically over the steps."""
    hip = _hip()
    case = _case()
    d, u = 0.9, 2.0 ** -24
    omega = 1.0 - d
    w64 = f32(omega)
    assert w64 <= 0.5
    bigs, views = _buffers(case, gpu, torch.float32, None, True)
    mask = case.mask.to(gpu)
    ref = case.e.to(gpu).double()
    bound = torch.zeros(case.n, dtype=torch.float64, device=gpu)
    worst = 0.0
    for t in range(50):
        e_before = views["e"].clone()
        hip.adam_step(views["w"], views["m"], views["v"], views["g"], None, mask, STEP, EPS, B1, B2, GSCALE, LR_WD,
                      ema=views["e"], ema_omd=omega)
        _check_guards(bigs)
        theta = views["w"]
        ref = ref + w64 * (theta.double() - ref)
        mag = torch.maximum(theta.abs(), torch.maximum(e_before.abs(), views["e"].abs())).double()
        bound = d * bound + 3.0 * u * mag
        err = (views["e"].double() - ref).abs()
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all()), (t, float(err.max()), float(bound.max()))
    print(f"largest error / bound over 50 steps: {worst:.3f}")
    assert float((views["e"] - case.e.to(gpu)).abs().max()) > 100 * STEP * 0.1  # the average travelled


# ------------------------------------------------------------------------------------------ 6. bad arguments
def test_bad_ema_arguments_raise_before_any_launch(gpu):
    hip = _hip()
    n = 4096
    plan = hip.lamb_plan([0, 1024], [1024, 3072], [1, 0], n, torch.zeros(1, device=gpu))
    other = torch.device("cuda", 1) if torch.cuda.device_count() > 1 else None

    def bufs():
        return [torch.ones(n, device=gpu) for _ in range(4)]

    def adam(b, ema, omd=0.1):
        hip.adam_step(b[0], b[1], b[2], b[3], None, None, STEP, EPS, B1, B2, 1.0, 0.0, ema=ema, ema_omd=omd)

    def lamb(b, ema, omd=0.1):
        hip.lamb_step(plan, 0, plan.nsegs, b[0], b[1], b[2], b[3], None, None, torch.zeros(2 * plan.ntiles, device=gpu),
                      torch.zeros(3 * plan.nsegs, device=gpu), LAMB_LR, IBC1, IBC2, LAMB_EPS, B1, B2, 1.0, 0.0,
                      ema=ema, ema_omd=omd)

    for call in (adam, lamb):
        b = bufs()
        bad = {"fp64": torch.ones(n, dtype=torch.float64, device=gpu),
               "bf16": torch.ones(n, dtype=torch.bfloat16, device=gpu),
               "strided": torch.ones(2 * n, device=gpu)[::2], "cpu": torch.ones(n),
               "short": torch.ones(n - 64, device=gpu), "long": torch.ones(n + 64, device=gpu),
               "misaligned": torch.ones(n + 4, device=gpu)[1:n + 1],
               "is p": b[0], "is m": b[1], "is v": b[2], "is g": b[3]}
        if other is not None:
            bad["other device"] = torch.ones(n, device=other)
        assert not bad["strided"].is_contiguous() and bad["misaligned"].data_ptr() % 16 == 4
        for what, ema in bad.items():
            keep = ema.clone()
            with pytest.raises(RuntimeError, match="ema"):
                call(b, ema)
            torch.cuda.synchronize()
            assert all(bool((t == 1).all()) for t in b), (call.__name__, what)  # nothing ran
            assert torch.equal(ema, keep), (call.__name__, what)
        # storage shared with p through another view of it
        big = torch.ones(2 * n, device=gpu)
        with pytest.raises(RuntimeError, match="ema"):
            call([big[:n], b[1], b[2], b[3]], big[n:])
        for omd in (NAN, float("inf"), float("-inf"), -1e-9, 1.0 + 1e-9, 2.0):
            ema = torch.full((n,), 3.0, device=gpu)
            with pytest.raises(RuntimeError, match="ema_omd"):
                call(b, ema, omd)
            torch.cuda.synchronize()
            assert all(bool((t == 1).all()) for t in b) and bool((ema == 3).all()), (call.__name__, omd)
        # the bounds themselves are fine, and a good call runs
        for omd in (0.0, 1.0):
            b, ema = bufs(), torch.full((n,), 3.0, device=gpu)
            call(b, ema, omd)
            torch.cuda.synchronize()
            assert not bool((b[0] == 1).all())
            assert torch.equal(ema, _replay(torch.full_like(ema, 3.0), omd, b[0]))
            assert bool((ema == 3).all()) == (omd == 0.0)
    # a device-side coefficient tensor of the old size with ema is refused (slot 4 would lie outside it)
    b, ema = bufs(), torch.full((n,), 3.0, device=gpu)
    with pytest.raises(RuntimeError, match="ema"):
        hip.adam_step(b[0], b[1], b[2], b[3], None, None, STEP, EPS, B1, B2, 1.0, 0.0,
                      torch.zeros(4, device=gpu), ema=ema, ema_omd=0.1)
    torch.cuda.synchronize()
    assert all(bool((t == 1).all()) for t in b) and bool((ema == 3).all())


# ------------------------------------------------------------------------------------------ trainer level
def _tiny_cfg(wide=False):
    from huggingface_sagemaker_tensorflow_distributed_amd.models import resolve_config

    cfg = resolve_config("hsd-tiny-bert")
    if wide:  # the shapes tests/test_gpu_lamb.py uses for the fp32 and fp8 stores
        cfg = cfg.replace(hidden_size=256, num_attention_heads=4, intermediate_size=512)
    assert cfg.num_hidden_layers == 2 and cfg.hidden_dropout_prob > 0
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


def _trainer(gpu, cfg, optimizer, dtype="bf16", max_grad_norm=0.0, decay=0.9, warmup=True, **kw):
    from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedAdam, FusedLamb
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore
    from huggingface_sagemaker_tensorflow_distributed_amd.train.trainer import Trainer

    model = build_model(cfg, seed=0).to(gpu)
    model.rng.base_seed = 5
    store = FlatParamStore(model, gpu, compute_dtype=torch.float32 if dtype == "fp32" else torch.bfloat16,
                           fp8=dtype == "fp8")
    opt = (FusedLamb if optimizer == "lamb" else FusedAdam)(store, lr=2e-3, weight_decay=0.01,
                                                            max_grad_norm=max_grad_norm, ema_decay=decay,
                                                            ema_warmup=warmup)
    return Trainer(model, store, opt, None, gpu, **kw)


def _decay_at(d, warmup, t):
    return min(d, (1.0 + t) / (10.0 + t)) if warmup else d


def _steps_follow_the_replay(tr, micro_batch_lists, d, warmup):
    """After every optimizer step ``optimizer.ema`` is the three-operation replay over the master snapshots."""
    opt, st = tr.optimizer, tr.store
    assert torch.equal(opt.ema, st.master) and opt.ema.data_ptr() != st.master.data_ptr()
    at = opt.ema.data_ptr()
    e = opt.ema.clone()
    for t, mbs in enumerate(micro_batch_lists):
        before = st.master.clone()
        tr.train_step(mbs)
        torch.cuda.synchronize()
        assert not torch.equal(before, st.master)
        assert opt.ema_decay_at(t) == _decay_at(d, warmup, t)
        e = _replay(e, 1.0 - _decay_at(d, warmup, t), st.master)
        assert torch.equal(_bits(opt.ema), _bits(e)), t
    assert opt.step_count == len(micro_batch_lists) and opt.ema.data_ptr() == at
    assert not torch.equal(opt.ema, st.master)


@pytest.mark.parametrize("warmup", [False, True])
@pytest.mark.parametrize("mode", ["overlap", "no_overlap", "clip"])
@pytest.mark.parametrize("optimizer", ["adam", "lamb"])
def test_trainer_steps_keep_the_average(gpu, monkeypatch, optimizer, mode, warmup):
    monkeypatch.setenv("HSD_OPT_OVERLAP", "0" if mode == "no_overlap" else "1")
    monkeypatch.setenv("HSD_OPT_BUCKET_MB", "0.05")  # several slices of this small model
    monkeypatch.setenv("HSD_WT", "1")
    cfg = _tiny_cfg()
    tr = _trainer(gpu, cfg, optimizer, max_grad_norm=1.0 if mode == "clip" else 0.0, warmup=warmup)
    assert (tr._opt_overlap is not None) == (mode != "no_overlap")
    if mode != "no_overlap":
        assert len(tr.optimizer._ranges) > 3
    _steps_follow_the_replay(tr, [[b] for b in _tiny_batches(cfg, gpu)], 0.9, warmup)


@pytest.mark.parametrize("dtype", ["fp32", "fp8"])
def test_trainer_steps_keep_the_average_with_the_fp32_and_fp8_stores(gpu, monkeypatch, dtype):
    monkeypatch.setenv("HSD_OPT_BUCKET_MB", "1")
    hip = _hip()
    cfg = _tiny_cfg(wide=True)
    if dtype == "fp8":
        hip.set_fp8(True)
    try:
        tr = _trainer(gpu, cfg, "adam", dtype=dtype, warmup=False)
        assert (tr.store.split_hi is not None) == (dtype == "fp32") and len(tr.optimizer._ranges) > 1
        assert (getattr(tr.store, "_fp8_desc", None) is not None) == (dtype == "fp8")
        _steps_follow_the_replay(tr, [[b] for b in _tiny_batches(cfg, gpu)], 0.9, False)
    finally:
        if dtype == "fp8":
            hip.set_fp8(False)


@pytest.mark.parametrize("optimizer", ["adam", "lamb"])
def test_accumulation_moves_the_average_once_per_optimizer_step(gpu, monkeypatch, optimizer):
    monkeypatch.setenv("HSD_OPT_BUCKET_MB", "0.05")
    cfg = _tiny_cfg()
    tr = _trainer(gpu, cfg, optimizer, warmup=True, grad_accum=2)
    b = _tiny_batches(cfg, gpu, n=6)
    _steps_follow_the_replay(tr, [b[0:2], b[2:4], b[4:6]], 0.9, True)  # t advances per optimizer step: 0, 1, 2


# ------------------------------------------------------------------------------------------ 8. whole-step graph
@pytest.mark.parametrize("optimizer", ["adam", "lamb"])
def test_captured_optimizer_steps_give_the_eager_bits(gpu, optimizer):
    """Eager and captured optimizer steps from the same start and the same gradients: the same ``ema`` (and weight)
    bits after 3 replays, with warm-up on so the averaging weight changes every step and has to come from the device
    scalars. The step is captured on its own, without a backward: the backward's fp32 atomics reduce in a different
    order from run to run (tests/test_gpu_graph.py), so two runs of whole training steps are not comparable bit for
    bit, eager or captured; :func:`test_whole_step_graph_keeps_the_average` covers the trainer's captured steps."""
    cfg = _tiny_cfg()
    res = {}
    for captured in (False, True):
        tr = _trainer(gpu, cfg, optimizer, warmup=True)
        opt, st = tr.optimizer, tr.store
        gen = torch.Generator().manual_seed(11)
        grads = [(torch.randn(st.numel, generator=gen) * 1e-2).to(gpu) for _ in range(3)]
        keep = torch.zeros(st.numel, dtype=torch.bool, device=gpu)
        for s in st.segments:
            keep[s.offset:s.offset + s.numel] = True
        graph = None
        if captured:
            opt.use_device_coef()
            st.grad.copy_(grads[0] * keep)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            step0 = opt.step_count
            with opt.capturing(), torch.cuda.graph(graph, capture_error_mode="thread_local"):
                opt.step(grad_scale=0.5)
            opt.step_count = step0  # capturing ran no kernel and must not count as a step
            assert torch.equal(opt.ema, st.master)
        for g in grads:
            st.grad.copy_(g * keep)
            if captured:
                opt.prepare_device_step(0.5)
                graph.replay()
            else:
                opt.step(grad_scale=0.5)
        torch.cuda.synchronize()
        assert opt.step_count == 3
        res[captured] = (st.master.clone(), opt.ema.clone(), opt.exp_avg.clone())
    for a, b in zip(res[False], res[True]):
        assert torch.equal(_bits(a), _bits(b))
    assert not torch.equal(res[True][0], res[True][1])


@pytest.mark.parametrize("optimizer", ["adam", "lamb"])
def test_whole_step_graph_keeps_the_average(gpu, monkeypatch, optimizer):
    """--hip_graph true with warm-up on: after each replay of the captured whole training step the average is the
    three-operation replay over that run's own master snapshots, bit for bit (each step's weight reached the captured
    launches through the device scalars), and it agrees with the eager run within test_gpu_graph.py's tolerance for the
    weights (1e-4 relative: the backward's atomics)."""
    monkeypatch.setenv("HSD_GRAPH_FULL", "1")
    monkeypatch.setenv("HSD_OPT_BUCKET_MB", "0.05")
    cfg = _tiny_cfg()
    batches = _tiny_batches(cfg, gpu)
    res = {}
    for replay in (False, True):
        tr = _trainer(gpu, cfg, optimizer, warmup=True, hip_graph=True)
        tr._graph_replay = replay
        _steps_follow_the_replay(tr, [[b] for b in batches], 0.9, True)
        if replay:
            assert len(tr._graphs) == 1 and tr._full_graph
        res[replay] = (tr.store.master.clone(), tr.optimizer.ema.clone())
        tr._seed.close()
    for a, b, what in zip(res[False], res[True], ("master", "ema")):
        rel = float((a - b).norm() / a.norm())
        print(f"eager vs replay, {what}: relative difference {rel:.3g}, same bits: {torch.equal(a, b)}")
        assert rel < 1e-4


# ------------------------------------------------------------------------------------------ 9. the swap
def _store_buffers(tr):
    st, opt = tr.store, tr.optimizer
    named = {"master": st.master, "ema": opt.ema, "m": opt.exp_avg, "v": opt.exp_avg_sq}
    if st.compute is not st.master:
        named["compute"] = st.compute
    for name in ("transposed", "split_hi", "split_lo"):
        if getattr(st, name, None) is not None:
            named[name] = getattr(st, name)
    if getattr(st, "_fp8_desc", None) is not None:
        for name in ("fp8_w", "fp8_wt", "fp8_sinv", "fp8_amax", "fp8_act"):
            named[name] = getattr(st, name)
    return named


def _eval_logits(tr, batch):
    tr.model.eval()
    with torch.no_grad():
        return tr._forward_loss(batch)[1].float().clone()


def _same_loss(a, b, dtype):
    """Two evaluations of the same weights. bf16 / fp8: the same kernels in the same order, identical sums
    (tests/test_gpu_graph.py). The fp32 head adds the rows' losses with fp32 atomics (csrc/kernels/fp32.hip), so two
    runs add the same B = 4 positive terms in another order: each of the 3 additions rounds by at most 2⁻²⁴ of a
    partial sum that is at most the total, on either side -- 6·2⁻²⁴ of the loss, asserted as 2⁻²¹."""
    if dtype != "fp32":
        return a == b
    return abs(a - b) <= 2.0 ** -21 * abs(a)


def _same_metrics(a, b, dtype):
    return set(a) == set(b) and all(_same_loss(a[k], b[k], dtype) if k == "loss" else a[k] == b[k] for k in a)


@pytest.mark.parametrize("dtype", ["bf16", "fp32", "fp8"])
def test_ema_weights_swaps_in_place_and_restores_every_buffer(gpu, monkeypatch, dtype):
    from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore

    monkeypatch.setenv("HSD_OPT_BUCKET_MB", "1")
    monkeypatch.setenv("HSD_WT", "1")
    hip = _hip()
    cfg = _tiny_cfg(wide=True)
    batches = _tiny_batches(cfg, gpu, n=4)
    if dtype == "fp8":
        hip.set_fp8(True)
    try:
        tr, twin = (_trainer(gpu, cfg, "adam", dtype=dtype, warmup=False, eval_hip_graph=True) for _ in range(2))
        for t in (tr, twin):
            for b in batches[:2]:
                t.train_step([b])
        torch.cuda.synchronize()
        st, opt = tr.store, tr.optimizer
        raw_graph = tr.evaluate(batches[2:3])  # captures the eval graph, at the raw weights
        assert tr.eval_graph_active and len(tr._eval_graphs) == 1
        torch.cuda.synchronize()
        named = _store_buffers(tr)
        expect = {"bf16": {"compute", "transposed"}, "fp32": {"split_hi", "split_lo"},
                  "fp8": {"compute", "transposed", "fp8_w", "fp8_wt", "fp8_sinv", "fp8_amax", "fp8_act"}}[dtype]
        assert set(named) == {"master", "ema", "m", "v"} | expect
        snap = {k: v.clone() for k, v in named.items()}
        at = {k: v.data_ptr() for k, v in named.items()}
        # the twin took the same two steps (its backward's atomics may have left other last bits), continues from a
        # copy of this state and never enters the context
        for name, t in snap.items():
            _store_buffers(twin)[name].copy_(t)
        twin.optimizer.step_count, twin.global_step = opt.step_count, tr.global_step
        twin.store.refresh_splits()
        with opt.ema_weights():
            torch.cuda.synchronize()
            assert {k: v.data_ptr() for k, v in _store_buffers(tr).items()} == at  # contents move, tensors stay
            assert torch.equal(_bits(st.master), _bits(snap["ema"]))
            assert torch.equal(_bits(opt.ema), _bits(snap["master"]))
            if dtype != "fp32":
                assert torch.equal(_bits(st.compute), _bits(snap["ema"].to(torch.bfloat16)))
            # a fresh model loaded with the averaged weights gives the same logits
            fresh_model = build_model(cfg, seed=1).to(gpu)
            fresh = FlatParamStore(fresh_model, gpu, compute_dtype=st.compute_dtype, fp8=dtype == "fp8")
            fresh.load_master(snap["ema"])
            if dtype == "fp8":
                # delayed scaling: the activation amax history and which sites are calibrated are run state, not
                # weights; the fresh model takes them over, so that only the weights are under test
                fresh.fp8_act.copy_(st.fp8_act)
                for p_run, p_new in zip(st.params, fresh.params):
                    for site in ("_hsd_fp8_x", "_hsd_fp8_g"):
                        if getattr(getattr(p_run, site, None), "_hsd_cal", False):
                            getattr(p_new, site)._hsd_cal = True
            fresh_model.eval()
            with torch.no_grad():
                want = fresh_model(batches[2]["input_ids"], attention_mask=batches[2]["attention_mask"],
                                   labels=batches[2]["labels"])[1].float()
            got = _eval_logits(tr, batches[2])
            assert torch.equal(got, want)
            # a replay of the eval graph captured before the swap reads the averaged weights: equal to eager
            ema_graph = tr.evaluate(batches[2:3])
            assert tr.eval_graph_active and len(tr._eval_graphs) == 1
            tr.eval_hip_graph = False
            ema_eager = tr.evaluate(batches[2:3])
            tr.eval_hip_graph = True
            assert _same_metrics(ema_graph, ema_eager, dtype), (ema_graph, ema_eager)
            assert abs(ema_graph["loss"] - raw_graph["loss"]) > 2.0 ** -18 * raw_graph["loss"], (ema_graph, raw_graph)
            with pytest.raises(RuntimeError, match="ema_weights"):
                tr.train_step([batches[3]])
        torch.cuda.synchronize()
        for again in range(2):
            for k, v in _store_buffers(tr).items():
                assert v.data_ptr() == at[k] and torch.equal(_bits(v), _bits(snap[k])), (k, again)
            if again == 0:  # Trainer.evaluate(weights="ema") is the same scope
                assert _same_metrics(tr.evaluate(batches[2:3], weights="ema"), ema_graph, dtype)
                torch.cuda.synchronize()
        assert opt.step_count == 2
        # the next training step is the twin's. Forward and loss are deterministic; the weights agree to the backward's
        # atomics (test_gpu_graph.py's tolerance between two runs: 1e-4 relative)
        la, lb = (float(t.train_step([batches[3]]).detach()) for t in (tr, twin))
        torch.cuda.synchronize()
        rel = float((st.master - twin.store.master).norm() / st.master.norm())
        rel_e = float((opt.ema - twin.optimizer.ema).norm() / opt.ema.norm())
        print(f"{dtype}: loss {la} vs twin {lb}; master relative difference {rel:.3g}, ema {rel_e:.3g}")
        assert _same_loss(la, lb, dtype) and rel < 1e-4 and rel_e < 1e-4
    finally:
        if dtype == "fp8":
            hip.set_fp8(False)
