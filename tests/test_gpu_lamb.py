"""Fused LAMB on the GPU (csrc/kernels/lamb.hip, optim/lamb.py, ``--optimizer lamb``): the three kernels against an
fp64 LAMB with derived error bounds, their determinism and argument checks, and whole trainer steps (overlapped / not,
accumulation, clipping, captured graph, bf16 / fp32 / fp8 stores) against per-step replays.

Error bounds of the kernel-level checks (u = 2^-24, the fp32 unit roundoff; fp32 division and square root are
correctly rounded; the reference is fp64 arithmetic on the SAME fp32 inputs and fp32-rounded scalars, so it carries no
error at this scale). Per element, with g' = g x gscale, a = b1 m, c = (1 - b1) g':

    m' = a + c            |dm'| <= 4u (|a| + |c|)      (roundings of g', a, c and the sum; no bound relative to m':
                                                        a and c may cancel)
    v' = b2 v + (1-b2) g'^2    |dv'| <= 6u v'           (all terms non-negative: g'^2 3u, x (1-b2) 1u, b2 v 1u, sum 1u)
    q  = m̂ / (sqrt(v̂) + eps)   |dq|  <= ibc1 |dm'| / den + 10u |q|
                               (m̂ = m' x ibc1: 1u; v̂: 7u, its root 3.5u + 1u, + eps 1u: den <= 6u; the quotient 1u)
    u  = q + wd w               |du|  <= |dq| + 2u |wd w| + 2u |u|

Sums. Every thread of a tile's workgroup keeps 2 x 4 independent accumulators per norm, a tile holds at most
TILE = 4,096 elements = 2 trips, so the longest fp32 addition chain is

    2 (trips) + 2 (lanes) + 1 (slots) + 6 (wave butterfly) + 3 (the block's 4 waves) = 14

additions, + 1 for the square and + 1 for the final cast of the fp64 segment sum to fp32: relative error at most
16 u = 9.5e-7 on a sum of exact squares. Asserted: 2e-6 for Σw². Σu² is a sum of squares of the ROUNDED u, so it also
carries Σ (2 |u| |du| + du²): asserted 2e-6 Σu² + 1.05 x that term. The ratio is formed in fp64 from the fp64 sums and
rounded once: |dr| / r <= (rel Σw² + rel Σu²) / 2 + 2u. The update w' = fma(-(lr x r), u, w) has

    |dw'| <= lr r |du| + lr r |u| (|dr| / r + 2u) + u |w'|

(the product lr x r rounded once, the fma once). The asserted bounds are these expressions x 1.01 (second-order terms).
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
U = 2.0 ** -24
GUARD = 1024


def _hip():
    from huggingface_sagemaker_tensorflow_distributed_amd.ops import hip

    return hip


def f32(x):
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------ kernel level: the case
LR, B1, B2, EPS, GSCALE, T_STEP = 2e-3, 0.9, 0.999, 1e-6, 1.0 / 3.0, 3
IBC1, IBC2 = 1.0 / (1.0 - B1 ** T_STEP), 1.0 / (1.0 - B2 ** T_STEP)
ZERO_SEG = 9  # the all-zero weight


@functools.lru_cache(maxsize=None)
def _layout():
    """Segment lengths at the tile edges: 1, 2 (the classifier bias: excluded), 63, 64, TILE - 64, TILE, TILE + 64,
    3 TILE + 192, a second excluded segment, and an all-zero weight; offsets 64-aligned, back to back."""
    tile = _hip().lamb_tile()
    lens = [1, 2, 63, 64, tile - 64, tile, tile + 64, 3 * tile + 192, 130, 200]
    adapt = [1, 0, 1, 1, 1, 1, 1, 1, 0, 1]
    spans = [(n + 63) // 64 * 64 for n in lens]
    offs = [sum(spans[:i]) for i in range(len(lens))]
    return tile, lens, adapt, spans, offs, sum(spans)


@functools.lru_cache(maxsize=None)
def _state(grad_dtype):
    """(w, m, v, g) on the CPU: random inside the segments, exactly zero in the alignment padding."""
    _tile, lens, _adapt, _spans, offs, n = _layout()
    gen = torch.Generator().manual_seed(17)
    w, m, v, g = (torch.zeros(n) for _ in range(4))
    for i, (o, k) in enumerate(zip(offs, lens)):
        if i != ZERO_SEG:
            w[o:o + k] = torch.randn(k, generator=gen) * 0.5
        m[o:o + k] = torch.randn(k, generator=gen) * 1e-2
        v[o:o + k] = torch.rand(k, generator=gen) * 1e-4
        g[o:o + k] = torch.randn(k, generator=gen)
    return w, m, v, g.to(grad_dtype)


@functools.lru_cache(maxsize=None)
def _reference(grad_dtype, wd):
    """The fp64 LAMB step of the case and the per-element / per-segment error bounds of the module docstring."""
    _tile, _lens, adapt, spans, offs, n = _layout()
    w, m, v, g = (t.double() for t in _state(grad_dtype))
    b1, b2, omb1, omb2 = f32(B1), f32(B2), f32(np.float32(1) - np.float32(B1)), f32(np.float32(1) - np.float32(B2))
    gs, ibc1, ibc2, eps, lr, wdf = f32(GSCALE), f32(IBC1), f32(IBC2), f32(EPS), f32(LR), f32(wd)
    gk = g * gs
    a, c = b1 * m, omb1 * gk
    m2 = a + c
    err_m = 4 * U * (a.abs() + c.abs())
    v2 = b2 * v + omb2 * gk * gk
    err_v = 6 * U * v2
    den = (v2 * ibc2).sqrt() + eps
    q = (m2 * ibc1) / den
    wdv = torch.zeros(n, dtype=torch.float64)
    for o, sp, ad in zip(offs, spans, adapt):
        wdv[o:o + sp] = wdf if ad else 0.0
    d = wdv * w
    u = q + d
    err_u = ibc1 * err_m / den + 10 * U * q.abs() + 2 * U * d.abs() + 2 * U * u.abs()
    segs = []
    w2, err_w = torch.empty_like(w), torch.empty_like(w)
    for o, sp, ad in zip(offs, spans, adapt):
        sl = slice(o, o + sp)
        sw, su = float((w[sl] ** 2).sum()), float((u[sl] ** 2).sum())
        bound_su = 2e-6 * su + 1.05 * float((2 * u[sl].abs() * err_u[sl] + err_u[sl] ** 2).sum())
        if ad and sw > 0 and su > 0:
            r, rel_r = (sw / su) ** 0.5, 0.5 * (2e-6 + bound_su / su) + 2 * U
        else:
            r, rel_r = 1.0, 0.0
        step = lr * r
        w2[sl] = w[sl] - step * u[sl]
        err_w[sl] = step * err_u[sl] + (step * u[sl]).abs() * (rel_r + 2 * U) + U * w2[sl].abs()
        segs.append({"sw": sw, "su": su, "bound_su": bound_su, "r": r, "rel_r": rel_r})
    return {"w": w2, "m": m2, "v": v2, "err_w": err_w, "err_m": err_m, "err_v": err_v, "segs": segs}


def _guarded(t, gpu, fill=None):
    """``t`` at offset GUARD of a larger buffer that is NaN everywhere else."""
    big = torch.full((GUARD + t.numel() + GUARD,), NAN, dtype=t.dtype, device=gpu)
    view = big[GUARD:GUARD + t.numel()]
    if fill is None:
        view.copy_(t.to(gpu))
    return big, view


def _guards_intact(big):
    return bool(torch.isnan(big[:GUARD]).all()) and bool(torch.isnan(big[-GUARD:]).all())


def _plan(gpu):
    hip = _hip()
    _tile, _lens, adapt, spans, offs, n = _layout()
    return hip.lamb_plan(offs, spans, adapt, n, torch.zeros(1, device=gpu))


def _run(gpu, grad_dtype=torch.float32, wd=0.01, slices=None, out_kind="bf16", coef=None, clip=None, zero_grad=False,
         host=None):
    """One LAMB step of the case, every buffer embedded in a NaN-filled one. ``slices``: the (seg0, nsegs) launches
    (default: one over everything). ``host``: override the host scalars (lr, ibc1, ibc2, eps, gscale, wd)."""
    hip = _hip()
    plan = _plan(gpu)
    n = plan.numel
    bigs, views = {}, {}
    for name, t in zip("wmvg", _state(grad_dtype)):
        bigs[name], views[name] = _guarded(t, gpu)
    out = lo = None
    if out_kind in ("bf16", "halves"):
        bigs["out"], out = _guarded(torch.empty(n, dtype=torch.bfloat16), gpu, fill=NAN)
    if out_kind == "halves":
        bigs["lo"], lo = _guarded(torch.empty(n, dtype=torch.bfloat16), gpu, fill=NAN)
    pad = 5
    pbig = torch.full((pad + 2 * plan.ntiles + pad,), NAN, device=gpu)
    rbig = torch.full((pad + 3 * plan.nsegs + pad,), NAN, device=gpu)
    partials, ratio = pbig[pad:pad + 2 * plan.ntiles], rbig[pad:pad + 3 * plan.nsegs]
    lr, ibc1, ibc2, eps, gs, wdh = host if host is not None else (LR, IBC1, IBC2, EPS, GSCALE, wd)
    for s0, k in (slices or [(0, plan.nsegs)]):
        hip.lamb_step(plan, s0, k, views["w"], views["m"], views["v"], views["g"], out, lo, partials, ratio, lr, ibc1,
                      ibc2, eps, B1, B2, gs, wdh, coef, clip, zero_grad)
    torch.cuda.synchronize()
    for name, big in bigs.items():
        assert _guards_intact(big), f"{name}: a guard outside the buffer was written"
    assert torch.isnan(pbig[:pad]).all() and torch.isnan(pbig[-pad:]).all()
    assert torch.isnan(rbig[:pad]).all() and torch.isnan(rbig[-pad:]).all()
    res = {k: v.clone() for k, v in views.items()}
    res.update(out=out, lo=lo, partials=partials.clone(), ratio=ratio.clone().view(-1, 3), plan=plan)
    return res


def _same_bits(a, b, keys=("w", "m", "v", "g", "out", "lo", "partials", "ratio")):
    for k in keys:
        if a[k] is None:
            assert b[k] is None
            continue
        x, y = a[k], b[k]
        # NaN slots (launches that never ran) must match too: compare the raw bits
        if x.dtype == torch.bfloat16:
            x, y = x.view(torch.int16), y.view(torch.int16)
        elif x.dtype == torch.float32:
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), k


# ------------------------------------------------------------------------------------------ kernel level: the tests
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16])
def test_norms_ratios_and_update_match_fp64(gpu, grad_dtype, wd):
    _tile, lens, adapt, spans, offs, n = _layout()
    ref = _reference(grad_dtype, wd)
    res = _run(gpu, grad_dtype, wd)
    ratio = res["ratio"].double().cpu()
    for i, (sg, o, sp) in enumerate(zip(ref["segs"], offs, spans)):
        r, sw, su = (float(x) for x in ratio[i])
        print(f"seg {i} len {lens[i]} adapt {adapt[i]}: sw {sw!r} ref {sg['sw']!r} | su {su!r} ref {sg['su']!r} "
              f"bound {sg['bound_su']:.3g} | r {r!r} ref {sg['r']!r} rel bound {sg['rel_r']:.3g}")
        assert abs(sw - sg["sw"]) <= 2e-6 * sg["sw"]
        assert abs(su - sg["su"]) <= sg["bound_su"]
        if sg["rel_r"] == 0.0:
            assert r == 1.0  # excluded from adaptation, or ||w|| = 0
        else:
            assert abs(r - sg["r"]) <= 1.01 * sg["rel_r"] * sg["r"]
        # the tile partials of the segment add up to the segment's sums (fp32 partials, fp64 here)
        t0, t1 = res["plan"].first_tile[i], res["plan"].first_tile[i + 1]
        parts = res["partials"].double().cpu().view(-1, 2)[t0:t1].sum(0)
        assert abs(float(parts[0]) - sw) <= 2 * U * sw and abs(float(parts[1]) - su) <= 2 * U * su
    assert [i for i, sg in enumerate(ref["segs"]) if sg["rel_r"] == 0.0] == [1, 8, ZERO_SEG]
    for key, err in (("w", "err_w"), ("m", "err_m"), ("v", "err_v")):
        diff = (res[key].double().cpu() - ref[key]).abs()
        worst = float((diff / (1.01 * ref[err] + 1e-300)).max())
        print(f"{key}: max |diff| {float(diff.max()):.3g}, worst diff / bound {worst:.3g}")
        assert bool((diff <= 1.01 * ref[err]).all()), key
    # alignment padding between the segments is still exactly zero, in every buffer
    pad = torch.ones(n, dtype=torch.bool)
    for o, k in zip(offs, lens):
        pad[o:o + k] = False
    assert int(pad.sum()) > 0
    for key in ("w", "m", "v", "g", "out"):
        assert int(torch.count_nonzero(res[key].cpu()[pad])) == 0, key
    assert torch.equal(res["g"].cpu(), _state(grad_dtype)[3])  # zero_grad off: the gradient is left alone
    if wd:
        assert not torch.equal(res["w"], _run(gpu, grad_dtype, 0.0)["w"])


@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16])
def test_two_runs_and_slice_by_slice_give_identical_bits(gpu, grad_dtype):
    whole = _run(gpu, grad_dtype)
    _same_bits(whole, _run(gpu, grad_dtype))
    nsegs = whole["plan"].nsegs
    _same_bits(whole, _run(gpu, grad_dtype, slices=[(0, 3), (3, 1), (4, 4), (8, nsegs - 8)]))
    _same_bits(whole, _run(gpu, grad_dtype, slices=[(i, 1) for i in reversed(range(nsegs))]))


@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16])
def test_device_scalars_override_the_host_arguments(gpu, grad_dtype):
    """Captured steps: the scalars come from the fp32 [8] device tensor; garbage host arguments change nothing."""
    coef = torch.tensor([LR, IBC1, IBC2, EPS, GSCALE, 0.01, NAN, NAN], device=gpu)
    a = _run(gpu, grad_dtype, coef=coef, host=(55.0, 7.0, 0.5, 3.0, 123.0, 9.0))
    _same_bits(a, _run(gpu, grad_dtype))
    with pytest.raises(RuntimeError):
        _run(gpu, grad_dtype, coef=coef[:4])  # Adam's [4] layout is not accepted


@pytest.mark.parametrize("device_coef", [False, True])
def test_clip_is_one_fp32_multiply_into_the_gradient_scale(gpu, device_coef):
    c = 0.37
    clip = torch.tensor([c], device=gpu)
    host_scale = float(np.float32(GSCALE) * np.float32(c))
    if device_coef:
        a = _run(gpu, coef=torch.tensor([LR, IBC1, IBC2, EPS, GSCALE, 0.01, 0.0, 0.0], device=gpu), clip=clip)
        b = _run(gpu, coef=torch.tensor([LR, IBC1, IBC2, EPS, host_scale, 0.01, 0.0, 0.0], device=gpu))
    else:
        a = _run(gpu, clip=clip)
        b = _run(gpu, host=(LR, IBC1, IBC2, EPS, host_scale, 0.01))
    _same_bits(a, b)
    assert not torch.equal(a["m"], _run(gpu)["m"])


@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16])
def test_zero_grad_clears_exactly_the_slice(gpu, grad_dtype):
    _tile, _lens, _adapt, spans, offs, n = _layout()
    res = _run(gpu, grad_dtype, slices=[(3, 3)], zero_grad=True)
    g0 = _state(grad_dtype)[3]
    inside = torch.zeros(n, dtype=torch.bool)
    inside[offs[3]:offs[5] + spans[5]] = True
    g = res["g"].cpu()
    assert int(torch.count_nonzero(g[inside])) == 0
    assert torch.equal(g[~inside], g0[~inside])
    # ... and only the slice was stepped
    w0 = _state(grad_dtype)[0]
    assert torch.equal(res["w"].cpu()[~inside], w0[~inside]) and not torch.equal(res["w"].cpu()[inside], w0[inside])
    whole = _run(gpu, grad_dtype, zero_grad=True)
    assert int(torch.count_nonzero(whole["g"])) == 0
    _same_bits(whole, _run(gpu, grad_dtype), keys=("w", "m", "v", "out", "partials", "ratio"))


@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16])
def test_output_copies(gpu, grad_dtype):
    hip = _hip()
    plain = _run(gpu, grad_dtype, out_kind=None)
    assert plain["out"] is None
    bf = _run(gpu, grad_dtype, out_kind="bf16")
    assert torch.equal(bf["out"], bf["w"].to(torch.bfloat16))
    hv = _run(gpu, grad_dtype, out_kind="halves")
    hi, lo = torch.empty_like(hv["out"]), torch.empty_like(hv["lo"])
    hip._C.split2(hv["w"].contiguous(), hi, lo)
    torch.cuda.synchronize()
    assert torch.equal(hv["out"], hi) and torch.equal(hv["lo"], lo)
    for other in (bf, hv):
        _same_bits(plain, other, keys=("w", "m", "v", "partials", "ratio"))


def test_bad_arguments_raise_without_a_launch(gpu):
    hip = _hip()
    tile, _lens, adapt, spans, offs, n = _layout()
    like = torch.zeros(1, device=gpu)
    with pytest.raises(RuntimeError):  # the last segment's tiles would end outside the buffer
        hip.lamb_plan(offs, spans, adapt, n - 64, like)
    with pytest.raises(RuntimeError):  # overlapping segments
        hip.lamb_plan([0, 64], [128, 64], [1, 1], 256, like)
    with pytest.raises(RuntimeError):  # a span that is not 64-aligned
        hip.lamb_plan([0], [63], [1], 256, like)
    plan = _plan(gpu)
    assert plan.numel == n and plan.tile == tile and plan.nsegs == len(offs)
    assert plan.ntiles == sum((sp + tile - 1) // tile for sp in spans)
    tiles = plan.tiles.cpu()
    assert int(tiles[:, 0].min()) == 0 and int((tiles[:, 0] + tiles[:, 1]).max()) == n and int(tiles[:, 1].max()) == tile

    def bufs(k=n):
        return [torch.ones(k, device=gpu) for _ in range(4)]

    def call(p, m, v, g, partials=None, ratio=None, s0=0, k=None, out=None, lo=None, coef=None):
        partials = torch.zeros(2 * plan.ntiles, device=gpu) if partials is None else partials
        ratio = torch.zeros(3 * plan.nsegs, device=gpu) if ratio is None else ratio
        hip.lamb_step(plan, s0, plan.nsegs if k is None else k, p, m, v, g, out, lo, partials, ratio, LR, IBC1, IBC2,
                      EPS, B1, B2, 1.0, 0.0, coef)

    bad = [dict(partials=torch.zeros(2 * plan.ntiles - 1, device=gpu)),  # short partials
           dict(ratio=torch.zeros(3 * plan.nsegs - 1, device=gpu)),  # short ratio buffer
           dict(s0=1, k=plan.nsegs), dict(s0=-1, k=1),  # segments outside the plan
           dict(out=torch.zeros(n - 64, dtype=torch.bfloat16, device=gpu)),
           dict(lo=torch.zeros(n, dtype=torch.bfloat16, device=gpu)),  # out_lo without out
           dict(coef=torch.zeros(8)),  # scalars not on the device
           dict(partials=torch.zeros(2 * plan.ntiles, dtype=torch.float64, device=gpu))]
    for kw in bad:
        b = bufs()
        with pytest.raises(RuntimeError):
            call(*b, **kw)
        torch.cuda.synchronize()
        assert all(bool((t == 1).all()) for t in b), kw  # nothing ran
    for k in (n - 64, n + 64):  # buffers that are not the plan's size: the tile table would not fit them
        b = bufs(k)
        with pytest.raises(RuntimeError):
            call(*b)
        torch.cuda.synchronize()
        assert all(bool((t == 1).all()) for t in b)
    b = bufs()
    with pytest.raises(RuntimeError):
        call(b[0], b[1], b[2].double(), b[3])
    with pytest.raises(RuntimeError):
        call(b[0], b[1], b[2], b[3].half())
    call(*b, s0=2, k=0)  # an empty slice is a no-op
    torch.cuda.synchronize()
    assert all(bool((t == 1).all()) for t in b)


# ------------------------------------------------------------------------------------------ trainer level
def _tiny_cfg(fp8_capable=False):
    from huggingface_sagemaker_tensorflow_distributed_amd.models import resolve_config

    cfg = resolve_config("hsd-tiny-bert")
    if fp8_capable:  # the shapes the clip tests use for the fp8 / fp32 stores
        cfg = cfg.replace(hidden_size=256, num_attention_heads=4, intermediate_size=512)
    assert cfg.hidden_dropout_prob > 0 and cfg.attention_probs_dropout_prob > 0  # dropout on
    return cfg


def _tiny_batches(cfg, gpu, n=4, b=4, s=128):
    g = torch.Generator().manual_seed(0)
    out = []
    for _ in range(n):
        am = torch.ones(b, s, dtype=torch.long)
        am[1, 70:] = 0
        out.append({"input_ids": torch.randint(5, cfg.vocab_size, (b, s), generator=g).to(gpu),
                    "attention_mask": am.to(gpu), "labels": torch.randint(0, 2, (b,), generator=g).to(gpu)})
    return out


def _trainer(gpu, cfg, optimizer="lamb", dtype="bf16", max_grad_norm=0.0, lr=2e-3, **kw):
    from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedAdam, FusedLamb
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore
    from huggingface_sagemaker_tensorflow_distributed_amd.train.trainer import Trainer

    model = build_model(cfg, seed=0).to(gpu)
    model.rng.base_seed = 5
    store = FlatParamStore(model, gpu, compute_dtype=torch.float32 if dtype == "fp32" else torch.bfloat16,
                           fp8=dtype == "fp8")
    if optimizer == "lamb":
        opt = FusedLamb(store, lr=lr, weight_decay=0.01, max_grad_norm=max_grad_norm)
    else:
        opt = FusedAdam(store, lr=lr, max_grad_norm=max_grad_norm)
    return Trainer(model, store, opt, None, gpu, **kw)


def _snapshot(tr):
    return tr.store.master.clone(), tr.optimizer.exp_avg.clone(), tr.optimizer.exp_avg_sq.clone()


def _replay_whole_buffer(tr, before, gscale):
    """ONE whole-buffer LAMB launch on the pre-step state and the step's final gradients (left in place:
    zero_grad_in_optimizer off) must give the bits the trainer's step left, however it was sliced and overlapped."""
    hip = _hip()
    st, opt = tr.store, tr.optimizer
    p0, m0, v0 = before
    # zeros: the tail of the buffer after the last segment belongs to no tile and stays the zero it always was
    out = lo = None
    if st.split_hi is not None:
        out, lo = torch.zeros_like(st.split_hi), torch.zeros_like(st.split_lo)
    elif st.compute is not st.master:
        out = torch.zeros_like(st.compute)
    plan = opt._plan
    partials = torch.zeros(2 * plan.ntiles, device=p0.device)
    ratio = torch.zeros(plan.nsegs, 3, device=p0.device)
    ibc1, ibc2 = opt._coeffs()
    clip = opt._clip_out[1:2] if opt._clip_out is not None else None
    hip.lamb_step(plan, 0, plan.nsegs, p0, m0, v0, st.grad.clone(), out, lo, partials, ratio, opt.lr, ibc1, ibc2,
                  opt.eps, opt.beta1, opt.beta2, gscale, opt.weight_decay, None, clip)
    torch.cuda.synchronize()
    assert torch.equal(p0, st.master) and torch.equal(m0, opt.exp_avg) and torch.equal(v0, opt.exp_avg_sq)
    assert torch.equal(ratio[:, 0], opt.last_trust_ratios)
    if lo is not None:
        assert torch.equal(out, st.split_hi) and torch.equal(lo, st.split_lo)
    elif out is not None:
        assert torch.equal(out, st.compute)
    for p in st.params:
        if hasattr(p, "_hsd_wt"):
            assert torch.equal(p._hsd_wt, p.detach().t())


def _replay_cpu_formula(tr, cfg, before, gscale):
    """The CPU path of FusedLamb (torch ops per segment, fp64 norms) on the same pre-step state and gradients.

    Both sides are fp32 evaluations of the same update d = lr r u: they differ by a few roundings in u (relative 1e-6
    at most here: m' = b1 m + (1 - b1) g' loses nothing at |g'| >> |m| / 10) and by the rounding of the ratio (1e-6),
    so |d_gpu - d_cpu| <= 1e-5 max|d| with room to spare, plus one ulp of w for the final rounding."""
    from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedLamb
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore

    st, opt = tr.store, tr.optimizer
    cst = FlatParamStore(build_model(cfg, seed=0), torch.device("cpu"))
    assert cst.numel == st.numel
    copt = FusedLamb(cst, lr=opt.lr, weight_decay=opt.weight_decay, max_grad_norm=opt.max_grad_norm, eps=opt.eps)
    p0, m0, v0 = (t.cpu() for t in before)
    cst.master.copy_(p0)
    copt.exp_avg.copy_(m0)
    copt.exp_avg_sq.copy_(v0)
    cst.grad.copy_(st.grad.float().cpu())
    copt.step_count = opt.step_count - 1
    copt.step(grad_scale=gscale)
    moved = float((cst.master - p0).abs().max())
    assert moved > 0
    gmax = float(cst.grad.abs().max()) * gscale
    torch.testing.assert_close(st.master.cpu(), cst.master, rtol=2.0 ** -22, atol=1e-5 * moved)
    torch.testing.assert_close(opt.exp_avg.cpu(), copt.exp_avg, rtol=1e-6, atol=1e-6 * gmax)
    torch.testing.assert_close(opt.exp_avg_sq.cpu(), copt.exp_avg_sq, rtol=1e-6, atol=1e-6 * gmax * gmax)
    torch.testing.assert_close(opt.last_trust_ratios.cpu(), copt.last_trust_ratios, rtol=1e-5, atol=0)
    if opt._clip_out is not None:
        assert opt.grad_norm() == pytest.approx(copt.grad_norm(), rel=1e-5)
        assert float(opt.last_clip_coef) == pytest.approx(float(copt.last_clip_coef), rel=1e-5)
    return copt


@pytest.mark.parametrize("overlap", ["1", "0"])
@pytest.mark.parametrize("accum", [1, 2])
def test_trainer_steps_match_whole_buffer_and_cpu_replays(gpu, monkeypatch, accum, overlap):
    """Three LAMB steps (one and two accumulation micro-steps), sliced and overlapped with the backward or not: after
    each, the store equals ONE whole-buffer launch on the step's final gradients bit for bit, and the CPU formula on the
    same gradients within rounding. This is how overlapped equals non-overlapped is shown bit for bit: two backward
    runs never produce the same gradient bits (fp32 atomics, see test_gpu_e2e.py), so both forms are compared on the
    gradients of one run."""
    monkeypatch.setenv("HSD_OPT_OVERLAP", overlap)
    monkeypatch.setenv("HSD_OPT_BUCKET_MB", "0.05")  # several slices of this small model
    monkeypatch.setenv("HSD_WT", "1")
    cfg = _tiny_cfg()
    tr = _trainer(gpu, cfg, grad_accum=accum)
    opt = tr.optimizer
    assert (tr._opt_overlap is not None) == (overlap == "1")
    if overlap == "1":
        assert len(opt._ranges) > 3 and len(opt._seg_ranges) == len(opt._ranges)
        assert sum(k for _s, k in opt._seg_ranges) == len(tr.store.segments)
    tr.zero_grad_in_optimizer = False  # the replays read the step's final gradients after the step
    batches = _tiny_batches(cfg, gpu)
    seen = []
    for step in range(3):
        before = _snapshot(tr)
        tr.train_step([batches[(step * accum + j) % 4] for j in range(accum)])
        torch.cuda.synchronize()
        _replay_whole_buffer(tr, tuple(t.clone() for t in before), 1.0 / accum)
        _replay_cpu_formula(tr, cfg, before, 1.0 / accum)
        seen.append(opt.trust_ratios())
    assert opt.step_count == 3
    names = [s.name for s in tr.store.segments]
    assert all(seen[-1][s.name] == 1.0 for s in tr.store.segments if not s.decay)
    assert any(seen[-1][n] != 1.0 for n in names)
    assert seen[0] != seen[1]


@pytest.mark.parametrize("c_mode", ["one", "half_the_norm"])
def test_lamb_with_a_global_clip_matches_the_replays(gpu, monkeypatch, c_mode):
    """max_grad_norm = 1.0 (the BERT recipe; this small model's gradient norm is under it, so the coefficient is 1),
    and half the first step's own norm (certainly clips): the hooks run the slices' sums of squares under the
    backward, step() finishes the norm and runs LAMB over the whole buffer with the device-side coefficient."""
    monkeypatch.setenv("HSD_OPT_BUCKET_MB", "0.05")
    cfg = _tiny_cfg()
    batches = _tiny_batches(cfg, gpu)
    tr = _trainer(gpu, cfg, max_grad_norm=1.0 if c_mode == "one" else float("inf"))
    st, opt = tr.store, tr.optimizer
    assert tr._opt_overlap is not None and len(opt._clip_bases) == len(opt._ranges) > 3
    tr.zero_grad_in_optimizer = False
    if c_mode != "one":
        # the first step's norm, measured with C = inf on this very trainer, which is then put back to its start
        p_init = st.master.clone()
        tr.train_step([batches[0]])
        c = 0.5 * opt.grad_norm()
        assert float(opt.last_clip_coef) == 1.0 and 0 < c < float("inf")
        st.load_master(p_init)
        opt.exp_avg.zero_()
        opt.exp_avg_sq.zero_()
        opt.step_count = tr.global_step = 0
        opt.max_grad_norm = c
    c = opt.max_grad_norm
    coefs = []
    for step in range(3):
        before = _snapshot(tr)
        tr.train_step([batches[step]])
        torch.cuda.synchronize()
        _replay_whole_buffer(tr, tuple(t.clone() for t in before), 1.0)
        _replay_cpu_formula(tr, cfg, before, 1.0)
        norm = opt.grad_norm()
        ref = float(st.grad.double().square().sum().sqrt())
        assert abs(norm - ref) <= 1e-5 * ref  # test_gpu_grad_clip.py's bound for one-trip buffers
        coefs.append(float(opt.last_clip_coef))
        want = float(np.float32(c)) / norm if norm > float(np.float32(c)) else 1.0
        assert abs(coefs[-1] - want) <= 2.0 ** -22 * want
    print("C", c, "clip coefficients", coefs)
    if c_mode != "one":
        assert coefs[0] < 0.75  # half the norm this same step had a moment ago: certainly clipped


def test_lamb_slices_on_the_engine_stream(gpu, monkeypatch):
    """Data-parallel form: each gradient bucket (whole parameters) takes its LAMB slice on the RCCL engine's stream
    right after the bucket's all-reduce (world-of-one communicator)."""
    from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model
    from huggingface_sagemaker_tensorflow_distributed_amd.ops._ext import load
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedLamb
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore, GradBucketer
    from huggingface_sagemaker_tensorflow_distributed_amd.train.trainer import Trainer

    monkeypatch.setenv("HSD_OPT_OVERLAP", "1")
    cfg = _tiny_cfg()
    model = build_model(cfg, seed=0).to(gpu)
    model.rng.base_seed = 5
    st = FlatParamStore(model, gpu, compute_dtype=torch.bfloat16)
    opt = FusedLamb(st, lr=2e-3, weight_decay=0.01)
    C = load()
    eng = C.CommEngine(0, 1, C.CommEngine.unique_id(), gpu.index, True)
    buck = GradBucketer(st, bucket_mb=0.05, engine=eng)
    tr = Trainer(model, st, opt, buck, gpu)
    assert tr._opt_overlap == "engine" and len(opt._seg_ranges) == len(buck.buckets) > 3
    tr.zero_grad_in_optimizer = False
    batches = _tiny_batches(cfg, gpu, n=2)
    for step in range(2):
        before = _snapshot(tr)
        tr.train_step([batches[step]])
        torch.cuda.synchronize()
        _replay_whole_buffer(tr, tuple(t.clone() for t in before), 1.0)
        _replay_cpu_formula(tr, cfg, before, 1.0)
    assert eng.launched_count() == len(buck.buckets)


@pytest.mark.parametrize("dtype", ["bf16", "fp32", "fp8"])
def test_lamb_steps_with_bf16_fp32_and_fp8_stores(gpu, monkeypatch, dtype):
    hip = _hip()
    monkeypatch.setenv("HSD_OPT_BUCKET_MB", "1")
    monkeypatch.setenv("HSD_WT", "1")
    cfg = _tiny_cfg(fp8_capable=True)
    batches = _tiny_batches(cfg, gpu, n=2)
    fp8 = dtype == "fp8"
    if fp8:
        hip.set_fp8(True)
    try:
        tr = _trainer(gpu, cfg, dtype=dtype)
        st, opt = tr.store, tr.optimizer
        assert tr._opt_overlap is not None and len(opt._ranges) > 1
        assert (st.split_hi is not None) == (dtype == "fp32")
        assert (st._fp8_desc is not None) == fp8
        if dtype != "fp32":
            assert len([p for p in st.params if hasattr(p, "_hsd_wt")]) == 4 * cfg.num_hidden_layers
        tr.zero_grad_in_optimizer = False
        for step in range(2):
            before = _snapshot(tr)
            tr.train_step([batches[step]])
            torch.cuda.synchronize()
            _replay_whole_buffer(tr, before, 1.0)  # also: every Wᵀ copy equals the transpose
            if fp8:  # the fp8 weight copies equal a one-pass re-quantisation of the updated master
                q, qt, si = st.fp8_w.clone(), st.fp8_wt.clone(), st.fp8_sinv.clone()
                st.refresh_fp8()
                torch.cuda.synchronize()
                assert torch.equal(q, st.fp8_w) and torch.equal(qt, st.fp8_wt) and torch.equal(si, st.fp8_sinv)
    finally:
        if fp8:
            hip.set_fp8(False)


def test_whole_step_graph_replays_the_lamb_step(gpu, monkeypatch):
    """The tolerances of test_gpu_graph.py::test_graph_replay_matches_eager (losses 2e-3, weights 1e-4 relative): the
    LAMB launches are captured with the step and read every replay's scalars (a warm-up and linear decay make each
    step's learning rate differ) from the device."""
    monkeypatch.setenv("HSD_GRAPH_FULL", "1")
    monkeypatch.setenv("HSD_OPT_BUCKET_MB", "0.05")
    cfg = _tiny_cfg()
    batches = _tiny_batches(cfg, gpu, n=3)
    res = {}
    for replay in (False, True):
        tr = _trainer(gpu, cfg, hip_graph=True, lr_schedule="linear", lr_warmup_steps=2)
        tr._graph_replay = replay
        tr.total_steps = 3
        losses, ratios = [], []
        for b in batches:
            losses.append(float(tr.train_step([b])))
            ratios.append(tr.optimizer.last_trust_ratios.clone())
        if replay:
            assert len(tr._graphs) == 1 and tr._full_graph
        assert tr.optimizer.step_count == 3
        torch.cuda.synchronize()
        res[replay] = (losses, tr.store.master.clone(), ratios)
        tr._seed.close()
    (l0, w0, r0), (l1, w1, r1) = res[False], res[True]
    print("eager", l0, "replay", l1)
    for a, b in zip(l0, l1):
        assert abs(a - b) <= 2e-3 * max(1.0, abs(a)), (l0, l1)
    rel = (w0 - w1).norm() / w0.norm()
    assert rel < 1e-4, float(rel)
    # nothing is frozen into the graph: every replayed step has its own ratios
    assert not torch.equal(r1[0], r1[1]) and not torch.equal(r1[1], r1[2])
    assert not torch.equal(r0[0], r0[1])


def test_adam_steps_before_and_after_lamb_give_identical_bits(gpu, monkeypatch):
    """The Adam path is untouched by LAMB living in the same process: an Adam trainer's steps equal the plain
    adam_step replay bit for bit before LAMB is constructed or launched and after, and Adam optimizers driven slice by
    slice over the gradients recorded from the first trainer leave the same bits before and after. (Two backward runs
    never give the same gradient bits -- fp32 atomics, see test_gpu_e2e.py -- so the comparison across runs is made on
    recorded gradients.)"""
    hip = _hip()
    monkeypatch.setenv("HSD_OPT_BUCKET_MB", "0.05")
    cfg = _tiny_cfg()
    batches = _tiny_batches(cfg, gpu)

    def trainer_steps():
        """Three Adam trainer steps, each equal to ONE adam_step on its own final gradients; returns the gradients."""
        tr = _trainer(gpu, cfg, optimizer="adam", lr=1e-3)
        st, opt = tr.store, tr.optimizer
        assert type(opt).__name__ == "FusedAdam" and opt.kind == "adam" and tr._opt_overlap is not None
        tr.zero_grad_in_optimizer = False
        grads = []
        for i in range(3):
            p0, m0, v0 = _snapshot(tr)
            tr.train_step([batches[i]])
            torch.cuda.synchronize()
            s, eps = opt._coeffs()
            out = torch.empty_like(st.compute)
            hip.adam_step(p0, m0, v0, st.grad, out, None, s, eps, opt.beta1, opt.beta2, 1.0, 0.0)
            torch.cuda.synchronize()
            assert torch.equal(p0, st.master) and torch.equal(m0, opt.exp_avg) and torch.equal(v0, opt.exp_avg_sq)
            assert torch.equal(out, st.compute)
            grads.append(st.grad.clone())
        return grads

    def sliced_adam(grads):
        """A fresh Adam optimizer stepped slice by slice (the overlap API) over recorded gradients."""
        tr = _trainer(gpu, cfg, optimizer="adam", lr=1e-3)
        st, opt = tr.store, tr.optimizer
        assert len(opt._ranges) > 3
        for g in grads:
            st.grad.copy_(g)
            opt.begin_step(grad_scale=1.0)
            for b in range(len(opt._ranges)):
                opt.step_range(b)
            opt.step(grad_scale=1.0)
        torch.cuda.synchronize()
        return (*_snapshot(tr), st.compute.clone())

    grads = trainer_steps()
    first = sliced_adam(grads)
    lamb = _trainer(gpu, cfg)
    for i in range(2):
        lamb.train_step([batches[i]])
    torch.cuda.synchronize()
    second = sliced_adam(grads)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    trainer_steps()
