"""--label_smoothing_factor without a GPU: the reference ops against the float64 definition, the model classes on the
CPU, and the command line.

Definition (HF ``LabelSmoother`` == ``F.cross_entropy(label_smoothing=eps)``), per row with logits z[0..C), label y:

    term = lse(z) - (1-eps)·z[y] - (eps/C)·Σ_c z[c]          loss = Σ_valid term / max(n_valid, 1)
    dz[c] = (softmax(z)[c] - (1-eps)·[c == y] - eps/C) / max(n_valid, 1)      exact 0 on ignored rows

fp32 equalities are held to rtol 1e-5 / atol 1e-6, the bound tests/test_packing.py uses for them.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from huggingface_sagemaker_tensorflow_distributed_amd import ops
from huggingface_sagemaker_tensorflow_distributed_amd.data.packing import pack_batch, position_rule
from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model, resolve_config
from huggingface_sagemaker_tensorflow_distributed_amd.ops import reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG = "--label_smoothing_factor"
RTOL, ATOL = 1e-5, 1e-6


def _formula64(z, labels, eps):
    """(loss, dz) of the definition above in float64, written out."""
    z = z.detach().double()
    R, C = z.shape
    ok = labels != -100
    n = max(int(ok.sum()), 1)
    y = labels.clamp(min=0)
    lse = torch.logsumexp(z, -1)
    term = lse - (1.0 - eps) * z[torch.arange(R), y] - eps / C * z.sum(-1)
    loss = (term * ok).sum() / n
    onehot = torch.zeros_like(z)
    onehot[torch.arange(R), y] = 1.0
    dz = (torch.exp(z - lse[:, None]) - (1.0 - eps) * onehot - eps / C) / n * ok[:, None]
    return loss, dz


def _case(R, C, seed, all_ignored=False):
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(R, C, generator=g) * 2).requires_grad_()
    labels = torch.randint(0, C, (R,), generator=g)
    labels[2::5] = -100  # about a fifth of the rows
    if all_ignored:
        labels[:] = -100
    return z, labels


def _check(loss, z, labels, eps):
    want, dz = _formula64(z, labels, eps)
    z.grad = None
    loss.backward()
    torch.testing.assert_close(loss.detach().double(), want, rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(z.grad.double(), dz, rtol=RTOL, atol=ATOL)
    assert torch.count_nonzero(z.grad[labels == -100]) == 0  # exact zeros


# ------------------------------------------------------------------------------------------ reference ops
@pytest.mark.parametrize("eps", [0.1, 0.5])
@pytest.mark.parametrize("C", [2, 3, 9])
def test_reference_losses_equal_the_float64_formula(C, eps):
    z, labels = _case(23, C, seed=C)
    _check(ref.cross_entropy(z, labels, eps), z, labels, eps)
    loss, stats = ref.seq_loss(z, labels, None, 0.5, eps)
    _check(loss, z, labels, eps)
    loss2, _ = ref.seq_loss(z, labels, "single_label_classification", label_smoothing=eps)
    assert torch.equal(loss2, loss)
    hits = int(((z.argmax(-1) == labels) & (labels != -100)).sum())
    assert stats[1].item() == hits and stats[2].item() == int((labels != -100).sum())  # hits do not depend on eps
    torch.testing.assert_close(stats[0] * stats[2], stats[3], rtol=RTOL, atol=ATOL)
    # the heads: logits = x·Wᵀ + b with gradients through x
    g = torch.Generator().manual_seed(5)
    H = 16
    x = torch.randn(23, H, generator=g)
    w, b = torch.randn(C, H, generator=g) * 0.3, torch.randn(C, generator=g)
    loss, logits, stats = ref.token_head(x, w, b, labels, 0.0, 0, True, eps)
    want, dz = _formula64(logits, labels, eps)
    torch.testing.assert_close(loss.double(), want, rtol=RTOL, atol=ATOL)
    xg = x.clone().requires_grad_()
    ref.token_head(xg, w, b, labels, 0.0, 0, True, eps)[0].backward()
    torch.testing.assert_close(xg.grad.double(), dz @ w.double(), rtol=RTOL, atol=ATOL)
    assert torch.count_nonzero(xg.grad[labels == -100]) == 0
    assert stats[2].item() == int((labels != -100).sum())


@pytest.mark.parametrize("eps", [0.1, 0.5])
def test_reference_mlm_head_smooths_over_the_real_vocabulary(eps):
    g = torch.Generator().manual_seed(7)
    T, H, V, Vp = 23, 16, 9, 12  # a padded table: C is the 9 real classes
    h = torch.randn(T, H, generator=g)
    w1, b1 = torch.randn(H, H, generator=g) * 0.2, torch.randn(H, generator=g) * 0.1
    lw, lb = torch.ones(H), torch.zeros(H)
    wemb = (torch.randn(Vp, H, generator=g) * 0.3).requires_grad_()
    bias = torch.randn(Vp, generator=g).requires_grad_()
    labels = torch.randint(0, V, (T,), generator=g)
    labels[torch.rand(T, generator=g) < 0.6] = -100
    labels[0] = 1
    loss, logits = ref.mlm_head(h, labels, w1, b1, lw, lb, 1e-5, wemb, bias, V, eps)
    sel = labels[labels != -100]
    assert logits.shape == (len(sel), V)
    want, dz = _formula64(logits, sel, eps)
    torch.testing.assert_close(loss.double(), want, rtol=RTOL, atol=ATOL)
    loss.backward()
    torch.testing.assert_close(bias.grad[:V].double(), dz.sum(0), rtol=RTOL, atol=ATOL)
    assert torch.count_nonzero(bias.grad[V:]) == 0 and torch.count_nonzero(wemb.grad[V:]) == 0  # not -eps/V


def test_all_rows_ignored_gives_zero_loss_and_zero_gradients():
    z, labels = _case(10, 3, seed=1, all_ignored=True)
    loss, stats = ref.seq_loss(z, labels, None, 0.5, 0.1)
    loss.backward()
    assert loss.item() == 0.0 and stats[2].item() == 0 and torch.count_nonzero(z.grad) == 0
    x = torch.randn(10, 8, requires_grad=True)
    loss, _, stats = ref.token_head(x, torch.randn(3, 8), torch.randn(3), labels, 0.0, 0, True, 0.1)
    loss.backward()
    assert loss.item() == 0.0 and stats[2].item() == 0 and torch.count_nonzero(x.grad) == 0
    loss, _ = ops.token_head(x, torch.randn(3, 8), torch.randn(3), labels, 0.0, 0, label_smoothing=0.1)
    assert loss.item() == 0.0


def test_eps_zero_is_bit_identical_to_a_call_without_the_keyword():
    z, labels = _case(23, 9, seed=2)
    g = torch.Generator().manual_seed(5)
    x, w, b = torch.randn(23, 16, generator=g), torch.randn(9, 16, generator=g), torch.randn(9, generator=g)

    def both(fn, *a, **k):
        outs = []
        for kw in ({}, {"label_smoothing": 0.0}):
            leaf = z.detach().clone().requires_grad_()
            xl = x.clone().requires_grad_()
            out = fn(leaf, xl, **kw)
            loss = out[0] if isinstance(out, tuple) else out
            loss.backward()
            outs.append((loss.detach(), leaf.grad, xl.grad))
        for u, v in zip(*outs):
            assert (u is None and v is None) or torch.equal(u, v)

    both(lambda zz, xx, **kw: ref.cross_entropy(zz, labels, **kw))
    both(lambda zz, xx, **kw: ref.seq_loss(zz, labels, **kw))
    both(lambda zz, xx, **kw: ref.token_head(xx, w, b, labels, 0.1, 3, **kw))
    both(lambda zz, xx, **kw: ops.cross_entropy(zz, labels, **kw))
    both(lambda zz, xx, **kw: ops.token_head(xx, w, b, labels, 0.1, 3, **kw))
    both(lambda zz, xx, **kw: ops._sum_ce(zz, labels, **kw))
    h = torch.randn(23, 2, 16, generator=g)
    w1, b1 = torch.randn(16, 16, generator=g), torch.randn(16, generator=g)
    both(lambda zz, xx, **kw: ops.cls_head(h * xx[:, None, :], w1, b1, w, b, labels, "tanh", 0.0, 0, 0.1, 4, **kw))
    mask = torch.where(labels != -100, labels, torch.full_like(labels, -100))
    both(lambda zz, xx, **kw: ref.mlm_head(xx, mask, w1, b1, torch.ones(16), torch.zeros(16), 1e-5, w, b, 9, **kw))
    both(lambda zz, xx, **kw: ops.mlm_head(xx, mask, w1, b1, torch.ones(16), torch.zeros(16), 1e-5, w, b, 9, **kw))


def test_ops_refuse_a_bad_eps_and_the_float_label_losses():
    z, labels = _case(8, 3, seed=3)
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="label_smoothing"):
            ops.cross_entropy(z, labels, label_smoothing=bad)
        with pytest.raises(ValueError, match="label_smoothing"):
            ops.token_head(torch.randn(8, 4), torch.randn(3, 4), torch.randn(3), labels, 0.0, 0, label_smoothing=bad)
    y = torch.rand(8, 3)
    for pt in ("regression", "multi_label_classification"):
        with pytest.raises(ValueError, match="label_smoothing"):
            ref.seq_loss(z, y, pt, 0.5, 0.1)
        with pytest.raises(ValueError, match="label_smoothing"):
            ops.cls_head(torch.randn(8, 1, 4), torch.randn(4, 4), torch.randn(4), torch.randn(3, 4), torch.randn(3), y,
                         "tanh", 0.0, 0, 0.0, 0, problem_type=pt, label_smoothing=0.1)
        ref.seq_loss(z, y, pt, 0.5, 0.0)  # eps = 0 is accepted everywhere


# ------------------------------------------------------------------------------------------ model level
EPS = 0.1
LENGTHS = [32, 20, 9, 2]


def _batch(cfg, task, seed=3):
    g = np.random.default_rng(seed)
    B, S = len(LENGTHS), 32
    ids = g.integers(5, cfg.vocab_size - 1, size=(B, S)).astype(np.int64)
    mask = (np.arange(S)[None, :] < np.array(LENGTHS)[:, None]).astype(np.int64)
    ids[mask == 0] = cfg.pad_token_id
    if task == "sequence-classification":
        labels = g.integers(0, cfg.num_labels, size=(B,)).astype(np.int64)
    elif task == "token-classification":
        labels = g.integers(0, cfg.num_labels, size=(B, S)).astype(np.int64)
        labels[g.random((B, S)) < 0.25] = -100
        labels[:, 0] = -100
        labels[mask == 0] = -100
    else:
        labels = np.where((g.random(ids.shape) < 0.3) & (mask != 0), ids, -100)
        labels[:, 1] = ids[:, 1]
        labels[mask == 0] = -100
    return ids, mask, labels


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def _assert_same_grads(g0, g1):
    assert set(g0) == set(g1)
    for n in g0:
        torch.testing.assert_close(g1[n], g0[n], rtol=RTOL, atol=ATOL, msg=lambda m, n=n: f"{n}: {m}")


@pytest.mark.parametrize("task", ["sequence-classification", "token-classification"])
@pytest.mark.parametrize("name", ["hsd-tiny-bert", "hsd-tiny-roberta"])
def test_model_loss_is_the_formula_on_its_logits_and_backward_matches_the_reference_recomputation(name, task):
    cfg = resolve_config(name, num_labels=3 if task == "sequence-classification" else 9)
    model = build_model(cfg, task=task, seed=1).train()  # dropout on
    assert model.label_smoothing == 0.0
    model.label_smoothing = EPS
    ids, mask, labels = _batch(cfg, task)
    t = torch.from_numpy
    kw = dict(input_ids=t(ids), attention_mask=t(mask))
    model.rng.new_step(0)
    loss, logits = model(**kw, labels=t(labels))
    C = logits.shape[-1]
    want, _ = _formula64(logits.reshape(-1, C), t(labels).reshape(-1), EPS)
    torch.testing.assert_close(loss.detach().double(), want, rtol=RTOL, atol=ATOL)
    plain, _ = _formula64(logits.reshape(-1, C), t(labels).reshape(-1), 0.0)
    assert abs(float(plain) - float(want)) > 10 * (RTOL * abs(float(want)) + ATOL)  # and not the unsmoothed loss
    loss.backward()
    g0 = _grads(model)
    # the same step with the loss recomputed by the reference ops on the label-free forward's logits
    model.zero_grad(set_to_none=True)
    model.rng.new_step(0)
    lg = model(**kw)
    torch.testing.assert_close(lg, logits, rtol=0, atol=0)  # the same dropout masks
    if task == "sequence-classification":
        loss2, _ = ref.seq_loss(lg, t(labels), None, 0.5, EPS)
    else:
        loss2 = ref.cross_entropy(lg.reshape(-1, C), t(labels).reshape(-1), EPS)
    torch.testing.assert_close(loss2, loss, rtol=RTOL, atol=ATOL)
    loss2.backward()
    _assert_same_grads(_grads(model), g0)


@pytest.mark.parametrize("masking", ["static", "dynamic"])
def test_masked_lm_model_smooths_over_the_vocabulary(masking, monkeypatch):
    cfg = resolve_config("hsd-tiny-roberta")
    model = build_model(cfg, task="masked-lm", seed=1).train()
    model.label_smoothing = EPS
    model.set_mlm_masking(masking, 0.15)
    ids, mask, labels = _batch(cfg, "masked-lm")
    t = torch.from_numpy
    seen = {}
    if masking == "dynamic":
        labels = np.where(mask != 0, 0, -100).astype(np.int64)  # maskable rows
        real = ops.mlm_head_fixed
        monkeypatch.setattr(ops, "mlm_head_fixed",
                            lambda x, mk, *a, **k: (seen.update(mask=mk), real(x, mk, *a, **k))[1])
    model.rng.new_step(0)
    loss, logits = model(t(ids), attention_mask=t(mask), labels=t(labels))
    if masking == "dynamic":
        mk = seen["mask"]
        tgt, in_ids, lab_full = mk.tgt, mk.input_ids, mk.labels.reshape(-1)
        assert int(mk.counts[0]) > 0
    else:
        lab_full = t(labels).reshape(-1)
        tgt, in_ids = lab_full[lab_full != -100], t(ids)
    V = logits.shape[-1]
    assert V == model.vocab
    want, _ = _formula64(logits, tgt, EPS)
    torch.testing.assert_close(loss.detach().double(), want, rtol=RTOL, atol=ATOL)
    loss.backward()
    g0 = _grads(model)
    # reference recomputation: every position's logits from the label-free forward, the reference CE on the targets
    model.zero_grad(set_to_none=True)
    model.rng.new_step(0)
    lg = model(in_ids, attention_mask=t(mask))
    loss2 = ref.cross_entropy(lg.reshape(-1, V), lab_full, EPS)
    torch.testing.assert_close(loss2, loss, rtol=RTOL, atol=ATOL)
    loss2.backward()
    _assert_same_grads(_grads(model), g0)


def test_packed_token_classification_step_equals_the_padded_step():
    """tests/test_packing.py's form: dropout off (the two layouts draw different masks), only the summation order
    differs."""
    cfg = resolve_config("hsd-tiny-roberta", num_labels=9).replace(hidden_dropout_prob=0.0,
                                                                   attention_probs_dropout_prob=0.0)
    if getattr(cfg, "classifier_dropout", None):
        cfg = cfg.replace(classifier_dropout=0.0)
    model = build_model(cfg, task="token-classification", seed=1).train()
    model.label_smoothing = EPS
    ids, mask, labels = _batch(cfg, "token-classification")
    t = torch.from_numpy

    def step(**kw):
        model.zero_grad(set_to_none=True)
        model.rng.new_step(0)
        loss, _ = model(**kw)
        loss.backward()
        return loss.detach(), _grads(model)

    l0, g0 = step(input_ids=t(ids), attention_mask=t(mask), labels=t(labels))
    pk = pack_batch(ids, mask, labels, **position_rule(cfg))
    l1, g1 = step(input_ids=t(pk["input_ids"]), labels=t(np.asarray(pk["labels"])), cu_seqlens=t(pk["cu_seqlens"]),
                  max_seqlen=pk["max_seqlen"], position_ids=t(pk["position_ids"]))
    torch.testing.assert_close(l1, l0, rtol=RTOL, atol=ATOL)
    _assert_same_grads(g1, g0)
    model.label_smoothing = 0.0
    plain = float(step(input_ids=t(ids), attention_mask=t(mask), labels=t(labels))[0])
    assert abs(plain - float(l0)) > 10 * (RTOL * abs(float(l0)) + ATOL)  # the smoothed loss was the one compared


# ------------------------------------------------------------------------------------------ command line
def _args(extra):
    from huggingface_sagemaker_tensorflow_distributed_amd.utils.args import build_parser

    args, _ = build_parser("train").parse_known_args(
        ["--model_name_or_path", "hsd-tiny-bert", "--train_batch_size", "8", "--log_every", "0", "--device", "cpu",
         "--dataset", "synthetic"] + extra)
    return args


def test_the_flag_parses_and_defaults_to_zero():
    assert _args([]).label_smoothing_factor == 0.0
    assert _args([FLAG, "0.1"]).label_smoothing_factor == 0.1


@pytest.mark.parametrize("extra", [
    ["--task", "question-answering", FLAG, "0.1"],
    ["--problem_type", "regression", FLAG, "0.1"],
    ["--problem_type", "multi_label_classification", "--num_labels", "3", FLAG, "0.1"],
    [FLAG, "-0.1"], [FLAG, "1.0"], [FLAG, "1.5"], [FLAG, "nan"],
    ["--task", "token-classification", FLAG, "1"], ["--task", "masked-lm", FLAG, "nan"],
])
def test_build_refuses_and_names_the_flag(extra):
    from huggingface_sagemaker_tensorflow_distributed_amd.train.runner import build

    with pytest.raises(ValueError, match=FLAG):
        build(_args(extra), "train")


@pytest.mark.parametrize("extra", [[], ["--problem_type", "single_label_classification"],
                                   ["--task", "token-classification", "--num_labels", "5"]])
def test_build_sets_the_factor_on_the_model(extra):
    from huggingface_sagemaker_tensorflow_distributed_amd.train.runner import build

    parts = build(_args(extra + [FLAG, "0.25"]), "train")
    assert parts["model"].label_smoothing == 0.25
    assert "label_smoothing" not in json.dumps(parts["model"].cfg.to_dict() if hasattr(parts["model"].cfg, "to_dict")
                                               else vars(parts["model"].cfg), default=str)


def _cli(tmp, extra, task="sequence-classification", model="hsd-tiny-bert"):
    env = dict(os.environ, SM_OUTPUT_DATA_DIR=str(tmp / "data"), SM_MODEL_DIR=str(tmp / "model"), SM_NUM_GPUS="0",
               SM_FRAMEWORK_PARAMS="{}")
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "train.py"), "--epochs", "1", "--train_batch_size", "8",
           "--eval_batch_size", "8", "--model_name_or_path", model, "--max_seq_length", "32",
           "--num_train_examples", "24", "--num_eval_examples", "16", "--device", "cpu", "--log_every", "0",
           "--dataset", "synthetic", "--task", task] + extra  # 24 / 8: three steps
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)


def _results(path):
    return dict(line.split(" = ") for line in path.read_text().splitlines())


def _without_the_clock(path):
    """train_results.txt ends in ``train_runtime = {...}``, a wall-clock reading: every other byte is compared."""
    return b"".join(ln for ln in path.read_bytes().splitlines(keepends=True) if not ln.startswith(b"train_runtime"))


def test_cli_run_writes_the_usual_files_and_records_the_factor(tmp_path):
    runs = {}
    for name, extra in (("smooth", [FLAG, "0.1"]), ("zero", [FLAG, "0"]), ("none", [])):
        d = tmp_path / name
        r = _cli(d, extra)
        assert r.returncode == 0, r.stderr[-3000:]
        runs[name] = d
    d = runs["smooth"]
    tr, ev = _results(d / "data" / "train_results.txt"), _results(d / "data" / "eval_results.txt")
    tr0 = _results(runs["none"] / "data" / "train_results.txt")
    ev0 = _results(runs["none"] / "data" / "eval_results.txt")
    assert list(tr) == list(tr0) and list(ev) == list(ev0)  # the usual format: the same keys in the same order
    assert np.isfinite(json.loads(tr["loss"])).all() and np.isfinite(float(ev["loss"]))
    assert 0.0 <= float(ev["sparse_categorical_accuracy"]) <= 1.0
    assert float(ev["loss"]) != float(ev0["loss"])  # evaluate reports the smoothed loss too
    prov = json.load(open(d / "data" / "run_provenance.json"))
    assert prov["label_smoothing_factor"] == 0.1
    for name in ("zero", "none"):
        assert "label_smoothing_factor" not in json.load(open(runs[name] / "data" / "run_provenance.json"))
    conf, conf0 = (json.load(open(runs[k] / "model" / "config.json")) for k in ("smooth", "none"))
    assert conf == conf0 and not any("smooth" in k for k in conf)  # a training argument, not a model property
    for f in ("train_results.txt", "eval_results.txt"):
        assert _without_the_clock(runs["zero"] / "data" / f) == _without_the_clock(runs["none"] / "data" / f), f


def test_cli_token_classification_metric_says_the_loss_is_smoothed(tmp_path):
    r = _cli(tmp_path, [FLAG, "0.1", "--num_labels", "5"], task="token-classification")
    assert r.returncode == 0, r.stderr[-3000:]
    prov = json.load(open(tmp_path / "data" / "run_provenance.json"))
    assert prov["label_smoothing_factor"] == 0.1 and "smoothed" in prov["metric"]
    ev = _results(tmp_path / "data" / "eval_results.txt")
    # C = 5, eps = 0.1: no smoothed loss lies below the entropy of the smoothed target,
    # 0.92·ln(1/0.92) + 0.08·ln(1/0.02) = 0.3897
    assert float(ev["loss"]) > 0.38
