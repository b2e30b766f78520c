"""--crf on the reference ops (CPU): ``reference.crf_loss`` / ``crf_decode`` against brute-force enumeration of every
tagging, a packed model step against the padded one, the flag's refusals and the checkpoint round trip."""
import itertools

import numpy as np
import pytest
import torch

from huggingface_sagemaker_tensorflow_distributed_amd.data.packing import pack_batch, position_rule
from huggingface_sagemaker_tensorflow_distributed_amd.models import (build_model, from_pretrained, resolve_config,
                                                                       save_pretrained)
from huggingface_sagemaker_tensorflow_distributed_amd.ops import reference as ref


def _inputs(C, seed):
    """Four sequences in one flat fp64 buffer: -100 gaps at both ends and inside, an empty chain, a chain of one row, a
    full chain of five rows; then two rows outside every sequence, one of them carrying a valid tag."""
    g = torch.Generator().manual_seed(seed)
    tag = lambda: int(torch.randint(C, (1,), generator=g))
    labels = [-100, tag(), tag(), -100, tag(), -100] + [-100, -100] + [tag()] + [tag() for _ in range(5)] + [0, -100]
    cu = torch.tensor([0, 6, 8, 9, 14], dtype=torch.int32)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).requires_grad_()
    return rnd(len(labels), C), torch.tensor(labels), cu, rnd(C), rnd(C), rnd(C, C)


def _brute(e, labels, cu, start, end, trans):
    """(loss, {row: best tag}) by enumerating all C^n taggings of every chain."""
    C, total, n, best = e.shape[1], 0.0, 0, {}
    for b in range(cu.numel() - 1):
        rows = [r for r in range(int(cu[b]), int(cu[b + 1])) if 0 <= int(labels[r]) < C]
        if not rows:
            continue
        score = lambda tags: (start[tags[0]] + end[tags[-1]] + sum(e[r, t] for r, t in zip(rows, tags))
                              + sum(trans[a, c] for a, c in zip(tags, tags[1:])))
        taggings = list(itertools.product(range(C), repeat=len(rows)))
        scores = torch.stack([score(t) for t in taggings])
        total = total + torch.logsumexp(scores, 0) - score([int(labels[r]) for r in rows])
        n += len(rows)
        best.update(zip(rows, taggings[int(scores.argmax())]))
    return total / max(n, 1), best


@pytest.mark.parametrize("C", [2, 3])
def test_loss_gradients_and_decode_equal_brute_force(C):
    e, labels, cu, start, end, trans = _inputs(C, seed=C)
    params = (e, start, end, trans)
    loss, stats, pred = ref.crf_loss(e, labels, cu, start, end, trans)
    want, best = _brute(e, labels, cu, start, end, trans)
    torch.testing.assert_close(loss, want, rtol=1e-12, atol=1e-12)
    for g, w in zip(torch.autograd.grad(loss, params), torch.autograd.grad(want, params)):
        torch.testing.assert_close(g, w, rtol=1e-10, atol=1e-12)
        if g.shape == e.shape:  # rows off the chain and outside every sequence: exactly zero
            assert not g[[0, 3, 5, 6, 7, 14, 15]].any()
    want_pred = torch.tensor([best.get(r, -1) for r in range(labels.numel())], dtype=torch.int32)
    assert torch.equal(pred, want_pred)
    chain = torch.tensor([r in best for r in range(labels.numel())])
    assert torch.equal(ref.crf_decode(e, chain, cu, start, end, trans), want_pred)
    assert stats[1:3].tolist() == [float((want_pred == labels).sum()), 9.0]
    torch.testing.assert_close(stats[[0, 3]].double(), torch.stack([want, want * 9]).detach(), rtol=1e-6, atol=1e-6)


def _tiny_crf(seed=1):
    cfg = resolve_config("hsd-tiny-bert", num_labels=5).replace(hidden_dropout_prob=0.0,
                                                                attention_probs_dropout_prob=0.0)
    return cfg, build_model(cfg, task="token-classification", seed=seed, use_crf=True).train()


def test_packed_model_step_equals_padded_step_fp32():
    """Dropout off, B = 4, S = 64, lengths 64 / 40 / 17 / 2, ~30 % of the real tokens unlabelled: the packed step's
    loss and every parameter gradient equal the padded step's at the bound of tests/test_packing.py."""
    cfg, model = _tiny_crf()
    g = np.random.default_rng(3)
    lengths = np.array([64, 40, 17, 2])
    mask = (np.arange(64)[None, :] < lengths[:, None]).astype(np.int64)
    ids = np.where(mask != 0, g.integers(5, cfg.vocab_size, size=(4, 64)), cfg.pad_token_id)
    labels = np.where((mask != 0) & (g.random((4, 64)) < 0.7), g.integers(0, 5, size=(4, 64)), -100)
    pk = pack_batch(ids, mask, labels, **position_rule(cfg))
    t = torch.from_numpy
    steps = []
    for kw in (dict(input_ids=t(ids), attention_mask=t(mask), labels=t(labels)),
               dict(input_ids=t(pk["input_ids"]), labels=t(np.asarray(pk["labels"])), cu_seqlens=t(pk["cu_seqlens"]),
                    max_seqlen=pk["max_seqlen"], position_ids=t(pk["position_ids"]))):
        model.zero_grad(set_to_none=True)
        model.rng.new_step(0)
        loss, _ = model(**kw)
        loss.backward()
        steps.append((loss.detach(), {n: p.grad.clone() for n, p in model.named_parameters()}, loss._hsd_stats))
    (l0, g0, s0), (l1, g1, s1) = steps
    torch.testing.assert_close(l1, l0, rtol=1e-5, atol=1e-6)
    assert s0[1:3].tolist() == s1[1:3].tolist() and s0[2] == (labels >= 0).sum()
    assert {"crf_start_bias", "crf_end_bias", "crf_transition_bias"} <= set(g0) and set(g0) == set(g1)
    for n in g0:
        torch.testing.assert_close(g1[n], g0[n], rtol=1e-5, atol=1e-6, msg=lambda m, n=n: f"{n}: {m}")


def test_refusals():
    from huggingface_sagemaker_tensorflow_distributed_amd.train import runner
    from huggingface_sagemaker_tensorflow_distributed_amd.utils.args import parse_args

    base = ["--model_name_or_path", "hsd-tiny-bert", "--device", "cpu", "--crf", "true"]
    for extra in (["--task", "sequence-classification"], ["--task", "question-answering"], ["--task", "masked-lm"],
                  ["--task", "sentence-embedding"], ["--task", "token-classification", "--label_smoothing_factor", "0.1"]):
        args, _ = parse_args(base + extra, "train")
        with pytest.raises(ValueError):
            runner.check_crf(args)
    assert runner.check_crf(parse_args(base + ["--task", "token-classification"], "train")[0]) is True
    assert runner.check_crf(parse_args(["--task", "token-classification"], "train")[0]) is False
    with pytest.raises(ValueError):
        build_model(resolve_config("hsd-tiny-bert"), task="sequence-classification", use_crf=True)
    plain = build_model(resolve_config("hsd-tiny-bert"), task="token-classification")
    assert not any(n.startswith("crf_") for n, _ in plain.named_parameters())  # flag off: nothing new


def test_save_and_load_round_trip(tmp_path, caplog):
    cfg, model = _tiny_crf()
    for n, p in model.named_parameters():
        if n.startswith("crf_"):
            assert p.abs().max() <= 0.1 and p.abs().max() > 0
    save_pretrained(model, str(tmp_path / "crf"))
    again = from_pretrained(str(tmp_path / "crf"), task="token-classification")  # config.json carries use_crf
    assert again.cfg.use_crf
    for (n0, p0), (n1, p1) in zip(model.named_parameters(), again.named_parameters()):
        assert n0 == n1 and torch.equal(p0, p1)
    ids = torch.randint(5, cfg.vocab_size, (2, 12))
    keep = torch.ones(2, 12, dtype=torch.int64)
    keep[1, 7:] = 0
    with torch.no_grad():
        tags = again.eval().decode(ids, keep)
        assert again(ids, keep).shape == (2, 12, 5)  # no labels: the emissions
    assert tags.shape == (2, 12) and (tags[1, 7:] == -1).all() and (tags[keep.bool()] >= 0).all()
    # a plain token-classification checkpoint: fresh CRF parameters and a warning
    save_pretrained(build_model(cfg.replace(use_crf=False), task="token-classification", seed=2), str(tmp_path / "plain"))
    with caplog.at_level("WARNING"):
        crf = from_pretrained(str(tmp_path / "plain"), task="token-classification", use_crf=True)
    assert crf.cfg.use_crf and "CRF" in caplog.text and crf.crf_transition_bias.abs().max() > 0
