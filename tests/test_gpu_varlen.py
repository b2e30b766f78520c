"""Variable-length attention kernels (csrc/kernels/attention_varlen.hip) and the packed model / trainer path
(--pack_sequences) on the GPU, vs ops/reference.py on the fp32 copy of the same inputs (same seed: the dropout bits
match).

* batch A: lengths 1, 7, 32, 33, 64, 65, 127, 128, 129, 200, 320 -- every boundary of 32-row waves, 64-key tiles and
  128-row blocks, more than one query / key block per sequence, 174 dead rows (T_real = 1106, T = 1280);
* batch B: 512, 512 -- no dead rows;
* batch C: 64 sequences of length (i % 5) + 1 -- per-sequence bookkeeping, T_real = 190 (twelve 1..5 cycles
  and 1, 2, 3, 4);
* three heads everywhere, so a swapped head / row decomposition cannot pass.
"""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from huggingface_sagemaker_tensorflow_distributed_amd import ops  # noqa: E402
from huggingface_sagemaker_tensorflow_distributed_amd.data.packing import pack_batch, position_rule  # noqa: E402
from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model, resolve_config  # noqa: E402
from huggingface_sagemaker_tensorflow_distributed_amd.ops import reference as ref  # noqa: E402

HEADS = 3
H = HEADS * 64
SEED = 777
BATCHES = {"A": [1, 7, 32, 33, 64, 65, 127, 128, 129, 200, 320], "B": [512, 512],
           "C": [(i % 5) + 1 for i in range(64)]}


def _hip():
    from huggingface_sagemaker_tensorflow_distributed_amd.ops import hip

    return hip


def _close(a, b, atol, rtol, what=""):
    """At most 0.1 % of the elements beyond tolerance (bf16 rounding flips), and NONE beyond 4x the tolerance.
    (tests/test_gpu_ops.py, verbatim)"""
    a = a.float()
    b = b.float()
    err = (a - b).abs()
    # atol is relative to the tensor's scale (bf16 outputs of long reductions), rtol per element
    tol = atol * b.abs().max().clamp_min(1e-6) + rtol * b.abs()
    bad = (err > tol).float().mean().item()
    worst = (err / tol).max().item()
    assert bad <= 1e-3, f"{what}: {bad*100:.3f}% elements out of tol, max err {err.max().item():.4g}"
    assert worst <= 4.0, f"{what}: an element is {worst:.2f}x beyond tolerance (max err {err.max().item():.4g})"


def _layout(name):
    lengths = BATCHES[name]
    cu = np.zeros(len(lengths) + 1, dtype=np.int32)
    cu[1:] = np.cumsum(lengths)
    t_real = int(cu[-1])
    return lengths, cu, t_real, -(-t_real // 256) * 256


def test_batch_layouts():
    assert _layout("A")[2:] == (1106, 1280) and _layout("B")[2:] == (1024, 1024) and _layout("C")[2:] == (190, 256)


_CASES = {}


def _case(name, p, device):
    """Inputs and the fp32 reference's output / dqkv of one batch (computed once, never modified)."""
    key = (name, p)
    c = _CASES.get(key)
    if c is None:
        lengths, cu, t_real, T = _layout(name)
        g = torch.Generator(device="cpu").manual_seed(11 + len(lengths))
        qkv = torch.randn(T, 3 * H, generator=g).to(device).bfloat16()
        dout = torch.randn(T, H, generator=g).to(device).bfloat16()
        cu_d = torch.from_numpy(cu).to(device)
        q32 = qkv.detach().float().requires_grad_()
        r = ref.attention_varlen(q32, cu_d, max(lengths), HEADS, p, SEED, p > 0)
        r.backward(dout.float())
        c = _CASES[key] = dict(qkv=qkv, dout=dout, cu=cu_d, cu_host=cu, max_seqlen=max(lengths), t_real=t_real, T=T,
                               out=r.detach(), dqkv=q32.grad.detach())
    return c


def _fwd_bwd(c, p, qkv=None):
    qkv = (c["qkv"] if qkv is None else qkv).detach().clone().requires_grad_()
    out = _hip().attention_varlen(qkv, c["cu"], c["max_seqlen"], HEADS, p, SEED)
    out.backward(c["dout"])
    torch.cuda.synchronize()
    return out.detach(), qkv.grad.detach()


# ------------------------------------------------------------------------------------------ 1. kernel vs reference
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_varlen_attention_matches_reference(gpu, name, p):
    c = _case(name, p, gpu)
    out, dqkv = _fwd_bwd(c, p)
    assert torch.isfinite(out.float()).all() and torch.isfinite(dqkv.float()).all()
    _close(out, c["out"], 2e-2, 2e-2, f"{name} out")
    for i, what in enumerate(("dq", "dk", "dv")):
        _close(dqkv[:, i * H:(i + 1) * H], c["dqkv"][:, i * H:(i + 1) * H], 3e-2, 3e-2, f"{name} {what}")


# ------------------------------------------------------------------------------------------ 2. every row written
@pytest.mark.parametrize("name", ["A", "C"])
def test_varlen_kernels_write_every_row_and_zero_the_dead_rows(gpu, name):
    C_ = _hip()._C
    p = 0.1
    c = _case(name, p, gpu)
    T, t_real, B = c["T"], c["t_real"], len(BATCHES[name])
    nan = float("nan")
    out = torch.full((T, H), nan, device=gpu, dtype=torch.bfloat16)
    lse = torch.full((HEADS * T,), nan, device=gpu)
    dqkv = torch.full((T, 3 * H), nan, device=gpu, dtype=torch.bfloat16)
    C_.attn_varlen_fwd(c["qkv"], c["cu"], out, lse, B, c["max_seqlen"], HEADS, p, SEED)
    C_.attn_varlen_bwd(c["qkv"], c["cu"], out, c["dout"], lse, dqkv, B, c["max_seqlen"], HEADS, p, SEED)
    torch.cuda.synchronize()
    assert t_real < T
    for what, t in (("out", out), ("lse2", lse.view(HEADS, T).t()), ("dqkv", dqkv)):
        assert not torch.isnan(t.float()).any(), f"{what}: a row was not written"
        assert torch.count_nonzero(t[t_real:]) == 0, f"{what}: a dead row is not zero"
    _close(out, c["out"], 2e-2, 2e-2, "out")


# ------------------------------------------------------------------------------------------ 3. sequence isolation
def test_varlen_sequences_do_not_see_each_other(gpu):
    p = 0.1
    c = _case("A", p, gpu)
    cu = c["cu_host"]
    s0, s1 = int(cu[5]), int(cu[6])
    noisy = c["qkv"].clone()
    g = torch.Generator(device="cpu").manual_seed(9)
    noisy[s0:s1] += torch.randn(s1 - s0, 3 * H, generator=g).to(gpu).bfloat16()
    out0, d0 = _fwd_bwd(c, p)
    out1, d1 = _fwd_bwd(c, p, noisy)
    keep = torch.ones(c["T"], dtype=torch.bool, device=gpu)
    keep[s0:s1] = False
    assert torch.equal(out0[keep], out1[keep]) and torch.equal(d0[keep], d1[keep])
    assert not torch.equal(out0[s0:s1], out1[s0:s1]) and not torch.equal(d0[s0:s1], d1[s0:s1])


# ------------------------------------------------------------------------------------------ 4. determinism
def test_varlen_forward_and_backward_are_bit_identical_run_to_run(gpu):
    c = _case("A", 0.1, gpu)
    out0, d0 = _fwd_bwd(c, 0.1)
    out1, d1 = _fwd_bwd(c, 0.1)
    assert torch.equal(out0, out1) and torch.equal(d0, d1)


# ------------------------------------------------------------------------------------------ 5. bias gradient
def test_varlen_backward_bias_gradient_matches_column_sums(gpu):
    """dbias: the column sums of dqkv over all T rows ADDED to what the destination held, at the bound of
    tests/test_gpu_attention_edges.py::test_attention_backward_bias_gradient_matches_column_sums."""
    C_ = _hip()._C
    p = 0.1
    c = _case("A", p, gpu)
    T, B = c["T"], len(BATCHES["A"])
    prefill = torch.randn(3 * H, generator=torch.Generator(device="cpu").manual_seed(5)).to(gpu)
    res = []
    for with_dbias in (True, False):
        out = torch.empty(T, H, device=gpu, dtype=torch.bfloat16)
        lse = torch.empty(HEADS * T, device=gpu)
        C_.attn_varlen_fwd(c["qkv"], c["cu"], out, lse, B, c["max_seqlen"], HEADS, p, SEED)
        dqkv = torch.empty_like(c["qkv"])
        db = prefill.clone() if with_dbias else None
        C_.attn_varlen_bwd(c["qkv"], c["cu"], out, c["dout"], lse, dqkv, B, c["max_seqlen"], HEADS, p, SEED, db)
        torch.cuda.synchronize()
        res.append((dqkv, db))
    (g1, db), (g0, _) = res
    _close(db - prefill, c["dqkv"].sum(0), 3e-2, 3e-2, "dbias")
    assert torch.equal(g1, g0)


# ------------------------------------------------------------------------------------------ 6 / 7. model
LENGTHS = (64, 40, 17, 2)


def _tiny(name, dropout):
    cfg = resolve_config(name).replace(hidden_size=128, num_attention_heads=2, intermediate_size=256)
    if not dropout:
        cfg = cfg.replace(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, seq_classif_dropout=0.0)
    return cfg


def _inputs(cfg, device):
    g = np.random.default_rng(0)
    ids = g.integers(5, cfg.vocab_size, size=(4, 64), dtype=np.int64)
    mask = (np.arange(64)[None, :] < np.asarray(LENGTHS)[:, None]).astype(np.int64)
    ids[mask == 0] = cfg.pad_token_id
    labels = g.integers(0, 2, size=(4,), dtype=np.int64)
    pk = pack_batch(ids, mask, labels, **position_rule(cfg))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    padded = dict(input_ids=t(ids), attention_mask=t(mask), labels=t(labels))
    packed = dict(input_ids=t(pk["input_ids"]), labels=t(labels), cu_seqlens=t(pk["cu_seqlens"]),
                  max_seqlen=pk["max_seqlen"], position_ids=t(pk["position_ids"]))
    return padded, packed


def _run(model, kw, force_torch):
    old = ops._FORCE_TORCH
    ops._FORCE_TORCH = force_torch
    try:
        model.zero_grad(set_to_none=True)
        model.rng.new_step(5)
        loss, logits = model(**kw)
        loss.backward()
        torch.cuda.synchronize()
        return (loss.detach().float(), logits.detach().float(),
                {n: p.grad.float().clone() for n, p in model.named_parameters()})
    finally:
        ops._FORCE_TORCH = old


def _assert_model_close(a, b):
    """The bounds of tests/test_gpu_e2e.py::test_model_hip_vs_reference."""
    (l1, lg1, g1), (l2, lg2, g2) = a, b
    assert torch.isfinite(l1) and torch.allclose(l1, l2, atol=2e-2, rtol=2e-2), (l1, l2)
    assert torch.allclose(lg1, lg2, atol=5e-2, rtol=5e-2)
    for n in g1:
        rel = (g1[n] - g2[n]).norm() / (g2[n].norm() + 1e-6)
        assert rel < 5e-2, f"{n}: rel grad err {rel:.3g}"


@pytest.mark.parametrize("name", ["hsd-tiny-bert", "hsd-tiny-roberta", "hsd-tiny-distilbert"])
def test_packed_model_hip_vs_packed_reference_with_dropout(gpu, name):
    cfg = _tiny(name, dropout=True)
    m = build_model(cfg, seed=0).to(gpu).bfloat16().train()
    _, packed = _inputs(cfg, gpu)
    _assert_model_close(_run(m, packed, False), _run(m, packed, True))


@pytest.mark.parametrize("name", ["hsd-tiny-bert", "hsd-tiny-roberta", "hsd-tiny-distilbert"])
def test_packed_model_hip_vs_padded_reference_without_dropout(gpu, name):
    cfg = _tiny(name, dropout=False)
    m = build_model(cfg, seed=0).to(gpu).bfloat16().train()
    padded, packed = _inputs(cfg, gpu)
    _assert_model_close(_run(m, packed, False), _run(m, padded, True))


# ------------------------------------------------------------------------------------------ 8. trainer
def _two_layer_bert_dir(tmp_path):
    cfg = {"model_type": "bert", "vocab_size": 30522, "hidden_size": 768, "num_hidden_layers": 2,
           "num_attention_heads": 12, "intermediate_size": 3072, "max_position_embeddings": 512, "type_vocab_size": 2,
           "num_labels": 2}
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    return str(tmp_path)


def _packed_batches(ds, n, bs, cfg, device):
    rule = position_rule(cfg)
    for i in range(n):
        sl = slice(bs * i, bs * (i + 1))
        pk = pack_batch(ds.input_ids[sl], ds.attention_mask[sl], ds.labels[sl], **rule)
        yield {k: (torch.from_numpy(np.ascontiguousarray(v)).to(device) if isinstance(v, np.ndarray) else v)
               for k, v in pk.items()}


def test_two_layer_bert_learns_the_marker_task_packed(gpu, tmp_path):
    """tests/test_gpu_e2e.py::test_two_layer_bert_learns_the_marker_task with --pack_sequences true: same model, data,
    steps and bound (> 95 % held-out accuracy), training and evaluation on packed batches."""
    from huggingface_sagemaker_tensorflow_distributed_amd import data as hdata
    from huggingface_sagemaker_tensorflow_distributed_amd.data.loader import BatchLoader
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import ShardSampler
    from huggingface_sagemaker_tensorflow_distributed_amd.train.runner import build
    from huggingface_sagemaker_tensorflow_distributed_amd.utils.args import build_parser

    args, _ = build_parser("train").parse_known_args(
        ["--model_name_or_path", _two_layer_bert_dir(tmp_path), "--train_batch_size", "32", "--learning_rate", "1e-4",
         "--dtype", "bf16", "--log_every", "0", "--seed", "7", "--pack_sequences", "true"])
    parts = build(args, "train")
    tr, cfg = parts["trainer"], parts["model"].cfg
    assert tr._seed is None and not tr._graph_replay  # --hip_graph auto resolves to off for packed batches
    ds = hdata.synthetic_classification(32 * 300, 128, 30522, seed=1)
    for mb in _packed_batches(ds, 300, 32, cfg, gpu):
        tr.train_step([mb])
    test = hdata.synthetic_classification(512, 128, 30522, seed=2)
    ev = tr.evaluate(BatchLoader(test, ShardSampler(512, 0, 1, shuffle=False, drop_last=False, batch_size=64), gpu,
                                 pack=True, pack_rule=position_rule(cfg)))
    assert not tr.eval_graph_active
    assert ev["sparse_categorical_accuracy"] > 0.95, ev


def test_packed_trainer_with_accumulation_clipping_and_lamb(gpu, tmp_path):
    from huggingface_sagemaker_tensorflow_distributed_amd import data as hdata
    from huggingface_sagemaker_tensorflow_distributed_amd.train.runner import build
    from huggingface_sagemaker_tensorflow_distributed_amd.utils.args import build_parser

    args, _ = build_parser("train").parse_known_args(
        ["--model_name_or_path", _two_layer_bert_dir(tmp_path), "--train_batch_size", "8", "--learning_rate", "1e-4",
         "--dtype", "bf16", "--log_every", "0", "--seed", "7", "--pack_sequences", "true", "--hip_graph", "true",
         "--gradient_accumulation_steps", "2", "--max_grad_norm", "1.0", "--optimizer", "lamb"])
    parts = build(args, "train")
    tr, cfg = parts["trainer"], parts["model"].cfg
    assert tr._seed is None and not tr._graph_replay  # an explicit --hip_graph true warns and stays eager
    ds = hdata.synthetic_classification(8 * 6, 128, 30522, seed=1)
    mbs = list(_packed_batches(ds, 6, 8, cfg, gpu))
    losses = [float(tr.train_step(mbs[2 * i:2 * i + 2]).detach()) for i in range(3)]
    torch.cuda.synchronize()
    assert all(np.isfinite(l) for l in losses), losses
    assert tr.global_step == 3 and tr.packed_real_tokens == int(ds.attention_mask.sum())


# ------------------------------------------------------------------------------------------ 9. padded path unchanged
def test_padded_step_is_unchanged_by_using_the_packed_path(gpu):
    """An existing-style padded training step (dropout on) before and after the packed path has been imported and
    used in the same process: the loss is bit-identical and the master weights agree to the padded step's own
    run-to-run noise.

    Bit-identical master weights cannot be asked of the padded step: its backward sums some gradients with fp32
    atomics (tests/test_gpu_e2e.py::test_optimizer_overlapped_with_backward_uses_final_gradients says the same), and
    four runs of this very step in one process, with no packed code touched, differed from each other in 412-418 of
    430,080 master weights by at most 4.07e-9 (119-152 weights, 1.86e-9, without dropout), the loss bit-identical.
    The bound is 4x that measured self-deviation; a different kernel or launch path moves weights by the size of an
    Adam update, 1e-4."""
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedAdam
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore
    from huggingface_sagemaker_tensorflow_distributed_amd.train.trainer import Trainer

    cfg = resolve_config("hsd-tiny-bert").replace(hidden_size=128, num_attention_heads=2, intermediate_size=256)
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(5, cfg.vocab_size, (4, 128), generator=g)
    am = torch.ones(4, 128, dtype=torch.long)
    am[1, 70:] = 0
    ids[1, 70:] = cfg.pad_token_id
    batch = {"input_ids": ids.to(gpu), "attention_mask": am.to(gpu), "labels": torch.tensor([0, 1, 1, 0], device=gpu)}

    def padded_run():
        m = build_model(cfg, seed=0).to(gpu)
        store = FlatParamStore(m, gpu, compute_dtype=torch.bfloat16)
        tr = Trainer(m, store, FusedAdam(store, lr=1e-4), None, gpu)
        loss = float(tr.train_step([batch]).detach())
        torch.cuda.synchronize()
        return loss, store.master.clone()

    l0, w0 = padded_run()
    # the packed path, in the same process: kernels, autograd function, model and trainer plumbing
    c = _case("C", 0.1, gpu)
    _fwd_bwd(c, 0.1)
    m = build_model(cfg, seed=0).to(gpu)
    store = FlatParamStore(m, gpu, compute_dtype=torch.bfloat16)
    tr = Trainer(m, store, FusedAdam(store, lr=1e-4), None, gpu, pack_sequences=True)
    pk = pack_batch(ids.numpy(), am.numpy(), np.array([0, 1, 1, 0]), **position_rule(cfg))
    mb = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(gpu) if isinstance(v, np.ndarray) else v)
          for k, v in pk.items()}
    assert np.isfinite(float(tr.train_step([mb]).detach()))
    l1, w1 = padded_run()
    dev = float((w1 - w0).abs().max())
    print(f"padded step before / after the packed path: loss {l0!r} / {l1!r}, max master deviation {dev:.3g}")
    assert l0 == l1
    assert dev <= 4 * 4.07e-9, dev
