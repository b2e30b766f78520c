"""--task question-answering on the CPU tier: the model against transformers, packed == padded, the position edge
cases, the best-span rule, the synthetic span corpus, the SQuAD reader and the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from huggingface_sagemaker_tensorflow_distributed_amd import data as hdata
from huggingface_sagemaker_tensorflow_distributed_amd import ops
from huggingface_sagemaker_tensorflow_distributed_amd.data.packing import pack_batch, position_rule, unpack_rows
from huggingface_sagemaker_tensorflow_distributed_amd.models import (build_model, from_pretrained, hf_state_dict,
                                                                     resolve_config, save_pretrained)
from huggingface_sagemaker_tensorflow_distributed_amd.ops import reference as ref
from huggingface_sagemaker_tensorflow_distributed_amd.ops import rng
from huggingface_sagemaker_tensorflow_distributed_amd.utils.args import parse_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASK = "question-answering"      # the command line's name, also taken by from_pretrained
MODEL_TASK = "span-extraction"   # build_model's key for it
NAMES = ["hsd-tiny-bert", "hsd-tiny-roberta", "hsd-tiny-distilbert"]
ARCH = {"hsd-tiny-bert": "BertForQuestionAnswering", "hsd-tiny-roberta": "RobertaForQuestionAnswering",
        "hsd-tiny-distilbert": "DistilBertForQuestionAnswering"}
t = torch.from_numpy


# ------------------------------------------------------------------------------------------ model vs transformers
def _hf_model(cfg):
    pytest.importorskip("transformers")
    from transformers import AutoConfig, AutoModelForQuestionAnswering

    d = cfg.to_hf_dict()
    hc = AutoConfig.for_model(d.pop("model_type"), **d)
    hc._attn_implementation = "eager"
    return AutoModelForQuestionAnswering.from_config(hc).eval()


def _segments(name, ids, mask=None):
    """Non-zero segment ids for BERT ([CLS] q q q [SEP] = 0, the rest = 1), none for the other families."""
    if name != "hsd-tiny-bert":
        return {}
    tt = torch.zeros_like(ids)
    tt[:, 5:] = 1
    if mask is not None:
        tt = tt * mask
    return {"token_type_ids": tt}


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_keys_and_architecture_match_hf(name):
    cfg = resolve_config(name)
    m = build_model(cfg, task=MODEL_TASK)
    ours = hf_state_dict(m)
    theirs = _hf_model(cfg).state_dict()
    assert set(ours) == set(theirs), (set(ours) ^ set(theirs))
    for k in ours:
        assert tuple(ours[k].shape) == tuple(theirs[k].shape), k
    assert m.architecture() == ARCH[name]
    assert tuple(m.qa_outputs_weight.shape) == (2, cfg.hidden_size) and tuple(m.qa_outputs_bias.shape) == (2,)
    assert m.graph_safe is True


@pytest.mark.parametrize("name", NAMES)
def test_logits_and_loss_parity_with_transformers_full_length(name):
    """Eval mode, no padding: logits at the tolerance of tests/test_token_classification.py's parity test and the
    loss equal to HF's ``.loss``."""
    cfg = resolve_config(name)
    ours = build_model(cfg, task=MODEL_TASK, seed=3).eval()
    hf = _hf_model(cfg)
    hf.load_state_dict(hf_state_dict(ours), strict=True)
    B, S = 3, 24
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(5, cfg.vocab_size, (B, S), generator=g)
    am = torch.ones(B, S, dtype=torch.long)
    pos = torch.tensor([[3, 5], [0, 0], [23, 23]])
    kw = _segments(name, ids)
    with torch.no_grad():
        loss, logits = ours(ids, attention_mask=am, labels=pos, **kw)
        out = hf(input_ids=ids, attention_mask=am, start_positions=pos[:, 0], end_positions=pos[:, 1], **kw)
        only_logits = ours(ids, attention_mask=am, **kw)
    assert tuple(logits.shape) == (B, S, 2)
    torch.testing.assert_close(logits[..., 0], out.start_logits, atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(logits[..., 1], out.end_logits, atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(loss, out.loss, atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(only_logits, logits)
    assert torch.equal(only_logits._hsd_pred, loss._hsd_pred)
    stats = loss._hsd_stats
    assert stats.shape == (8,) and float(stats[2]) == 3.0 and float(stats[4]) == 3.0 and float(stats[5]) == 3.0


@pytest.mark.parametrize("name", NAMES)
def test_padded_loss_is_ce_over_hf_logits_with_padding_at_minus_inf(name):
    """The deliberate difference from HF: padding rows take no part in the softmax."""
    cfg = resolve_config(name)
    ours = build_model(cfg, task=MODEL_TASK, seed=3).eval()
    hf = _hf_model(cfg)
    hf.load_state_dict(hf_state_dict(ours), strict=True)
    B, S = 3, 24
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(5, cfg.vocab_size, (B, S), generator=g)
    am = torch.ones(B, S, dtype=torch.long)
    am[1, 15:] = 0
    am[2, 7:] = 0
    ids[am == 0] = cfg.pad_token_id
    pos = torch.tensor([[3, 5], [14, 14], [2, 6]])
    kw = _segments(name, ids, am)
    with torch.no_grad():
        loss, logits = ours(ids, attention_mask=am, labels=pos, **kw)
        out = hf(input_ids=ids, attention_mask=am, **kw)
    real = am.bool()
    torch.testing.assert_close(logits[..., 0][real], out.start_logits[real], atol=1e-5, rtol=1e-4)
    st = out.start_logits.masked_fill(~real, float("-inf"))
    en = out.end_logits.masked_fill(~real, float("-inf"))
    want = 0.5 * (F.cross_entropy(st, pos[:, 0]) + F.cross_entropy(en, pos[:, 1]))
    torch.testing.assert_close(loss, want, atol=1e-5, rtol=1e-4)
    # and it is NOT HF's loss, whose softmax includes the padding rows
    hf_loss = 0.5 * (F.cross_entropy(out.start_logits, pos[:, 0]) + F.cross_entropy(out.end_logits, pos[:, 1]))
    assert float(hf_loss) > float(loss) + 1e-3


def test_task_names():
    """build_model's key is "span-extraction" (alias "qa"); the command line's "question-answering" is mapped by
    from_pretrained, and build_model keeps refusing that string (tests/test_token_classification.py pins it)."""
    cfg = resolve_config("hsd-tiny-bert")
    assert type(build_model(cfg, task="span-extraction")).__name__ == "TransformerForQuestionAnswering"
    assert type(build_model(cfg, task="qa")).__name__ == "TransformerForQuestionAnswering"
    assert type(from_pretrained("hsd-tiny-bert", task=TASK)).__name__ == "TransformerForQuestionAnswering"
    with pytest.raises(ValueError):
        build_model(cfg, task=TASK)


def test_head_dropout_rule_follows_hf():
    bert = resolve_config("hsd-tiny-bert").replace(hidden_dropout_prob=0.1)
    assert build_model(bert, task=MODEL_TASK).head_dropout() == 0.0
    assert build_model(resolve_config("hsd-tiny-roberta"), task=MODEL_TASK).head_dropout() == 0.0
    distil = resolve_config("hsd-tiny-distilbert")
    assert distil.qa_dropout == 0.1 and build_model(distil, task=MODEL_TASK).head_dropout() == 0.1
    assert build_model(distil.replace(qa_dropout=0.3), task=MODEL_TASK).head_dropout() == 0.3
    d = distil.replace(qa_dropout=0.25).to_hf_dict()
    assert d["qa_dropout"] == 0.25 and type(distil).from_hf_dict(d).qa_dropout == 0.25


def test_bert_draws_no_head_seed_and_distilbert_draws_one_after_the_encoder():
    """The seeds drawn in a training step are the encoder's, plus one for DistilBERT's qa_dropout and none for BERT and
    RoBERTa (whose QA heads have no dropout)."""
    pos = torch.tensor([[1, 2], [3, 3]])
    for name, extra in (("hsd-tiny-bert", 0), ("hsd-tiny-roberta", 0), ("hsd-tiny-distilbert", 1)):
        cfg = resolve_config(name)
        ids = torch.randint(5, cfg.vocab_size, (2, 16))
        m = build_model(cfg, task=MODEL_TASK, seed=0).train()
        m.rng.new_step(0)
        m.encoder(ids, torch.ones_like(ids), None, m.rng, True)
        encoder_calls = m.rng.calls
        m.rng.new_step(0)
        m(ids, attention_mask=torch.ones_like(ids), labels=pos)
        assert m.rng.calls == encoder_calls + extra, name


def test_head_dropout_site_is_the_flat_row_buffer():
    g = torch.Generator().manual_seed(0)
    h = torch.randn(37, 64, generator=g)
    w, b = torch.randn(2, 64, generator=g) * 0.1, torch.randn(2, generator=g) * 0.1
    cu = torch.tensor([0, 20, 37], dtype=torch.int32)
    pos = torch.tensor([[3, 7], [0, 16]])
    loss, logits = ops.qa_head(h, w, b, pos, cu, None, 0.1, 99, 30)
    keep = rng.keep_mask(99, (37, 64), 0.1).float() / 0.9
    want = F.linear(h * keep, w, b)
    torch.testing.assert_close(logits, want)
    ce = 0.5 * sum((F.cross_entropy(want[:20, c][None], pos[:1, c]) + F.cross_entropy(want[20:, c][None], pos[1:, c]))
                   / 2 for c in range(2))
    torch.testing.assert_close(loss, ce)
    lg, pred = ops.qa_head(h, w, b, None, cu, None, 0.1, 99, 30)
    torch.testing.assert_close(lg, want)
    assert torch.equal(pred, loss._hsd_pred)


def test_save_pretrained_loads_in_transformers(tmp_path):
    pytest.importorskip("transformers")
    from transformers import AutoModelForQuestionAnswering

    for name in NAMES:
        d = tmp_path / name
        cfg = resolve_config(name)
        ours = build_model(cfg, task=MODEL_TASK, seed=7).eval()
        save_pretrained(ours, str(d))
        assert json.load(open(d / "config.json"))["architectures"] == [ARCH[name]]
        hf = AutoModelForQuestionAnswering.from_pretrained(str(d)).eval()
        ids = torch.randint(5, cfg.vocab_size, (2, 12))
        with torch.no_grad():
            lg = ours(ids)
            out = hf(input_ids=ids)
            torch.testing.assert_close(lg[..., 0], out.start_logits, atol=1e-5, rtol=1e-4)
            torch.testing.assert_close(lg[..., 1], out.end_logits, atol=1e-5, rtol=1e-4)
            again = from_pretrained(str(d), task=TASK).eval()
            torch.testing.assert_close(again(ids), lg)


# ------------------------------------------------------------------------------------------ packed == padded
LENGTHS = [64, 40, 17, 2]
SPANS = np.array([[5, 9], [39, 39], [0, 16], [1, 1]], dtype=np.int64)  # position 0, len - 1 and a one-token span


def _padded(name, lengths, S, cfg, seed):
    g = np.random.default_rng(seed)
    ids = g.integers(5, cfg.vocab_size, size=(len(lengths), S)).astype(np.int64)
    mask = (np.arange(S)[None, :] < np.asarray(lengths)[:, None]).astype(np.int64)
    ids[mask == 0] = cfg.pad_token_id
    tt = ((np.arange(S)[None, :] >= 3) & (mask != 0)).astype(np.int64) if name == "hsd-tiny-bert" else None
    return ids, mask, tt


def _step(model, **kw):
    model.zero_grad(set_to_none=True)
    model.rng.new_step(0)
    loss, logits = model(**kw)
    loss.backward()
    grads = {n: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p))
             for n, p in model.named_parameters()}
    return loss.detach(), logits.detach(), grads, loss._hsd_stats.clone(), loss._hsd_pred.clone()


def _both_layouts(name, lengths, labels, **cfg_kw):
    cfg = resolve_config(name).replace(**cfg_kw)
    model = build_model(cfg, task=MODEL_TASK, seed=1).train()
    ids, mask, tt = _padded(name, lengths, 64, cfg, seed=3)
    kw = {"token_type_ids": t(tt)} if tt is not None else {}
    padded = _step(model, input_ids=t(ids), attention_mask=t(mask), labels=t(labels), **kw)
    pk = pack_batch(ids, mask, labels, **position_rule(cfg), span_labels=True, token_type_ids=tt)
    kw = {"token_type_ids": t(pk["token_type_ids"])} if tt is not None else {}
    packed = _step(model, input_ids=t(pk["input_ids"]), labels=t(np.asarray(pk["labels"])),
                   cu_seqlens=t(pk["cu_seqlens"]), max_seqlen=pk["max_seqlen"], position_ids=t(pk["position_ids"]),
                   **kw)
    return pk, mask, padded, packed


def _assert_same_step(pk, mask, padded, packed):
    (l0, lg0, g0, s0, p0), (l1, lg1, g1, s1, p1) = padded, packed
    torch.testing.assert_close(l1, l0, rtol=1e-5, atol=1e-6)
    back = t(unpack_rows(lg1.numpy(), pk["cu_seqlens"], 64))
    real = t(mask != 0)
    torch.testing.assert_close(back[real], lg0[real], rtol=1e-5, atol=1e-6)
    assert set(g0) == set(g1)
    for n in g0:
        torch.testing.assert_close(g1[n], g0[n], rtol=1e-5, atol=1e-6, msg=lambda m, n=n: f"{n}: {m}")
    assert torch.equal(s0[[1, 2, 4, 5, 6, 7]], s1[[1, 2, 4, 5, 6, 7]])


NO_DROPOUT = dict(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, qa_dropout=0.0)


@pytest.mark.parametrize("name", NAMES)
def test_packed_model_step_equals_padded_step_fp32(name):
    """B = 4, S = 64, lengths 64 / 40 / 17 / 2, fp32, the bound of tests/test_packing.py: loss, the logits of the real
    rows and every gradient at rtol 1e-5; BERT runs with non-zero segment ids. Dropout off (a ragged packed batch
    numbers its rows differently)."""
    pk, mask, padded, packed = _both_layouts(name, LENGTHS, SPANS, **NO_DROPOUT)
    assert pk["labels"].shape == (4, 2) and np.array_equal(pk["labels"], SPANS)
    _assert_same_step(pk, mask, padded, packed)
    if name == "hsd-tiny-bert":  # the segment ids matter: without them the loss differs
        cfg = resolve_config(name).replace(**NO_DROPOUT)
        model = build_model(cfg, task=MODEL_TASK, seed=1).train()
        ids, m, _ = _padded(name, LENGTHS, 64, cfg, seed=3)
        plain = _step(model, input_ids=t(ids), attention_mask=t(m), labels=t(SPANS))
        assert abs(float(plain[0]) - float(padded[0])) > 1e-6


def test_packed_step_equals_padded_step_with_head_dropout():
    """Full-length sequences: packed row t IS padded row b·S + i, so DistilBERT's qa_dropout draws the same mask in
    both layouts."""
    pk, mask, padded, packed = _both_layouts("hsd-tiny-distilbert", [64] * 4, SPANS, hidden_dropout_prob=0.0,
                                             attention_probs_dropout_prob=0.0, qa_dropout=0.25)
    _assert_same_step(pk, mask, padded, packed)


# ------------------------------------------------------------------------------------------ position edge cases
@pytest.mark.parametrize("packed", [False, True])
def test_all_ignored_batch_gives_zero_loss_and_zero_gradients(packed):
    labels = np.array([[-100, -100], [40, 63], [-1, 17], [2, 5]], dtype=np.int64)  # >= len, < 0, on padding rows
    pk, mask, pad, pck = _both_layouts("hsd-tiny-bert", LENGTHS, labels, **NO_DROPOUT)
    loss, _, grads, stats, _ = pck if packed else pad
    assert float(loss) == 0.0 and float(stats[2]) == 0.0 and float(stats[4]) == 0.0 and float(stats[5]) == 0.0
    for n, g in grads.items():
        assert torch.isfinite(g).all() and torch.count_nonzero(g) == 0, n


def _span_ref(logits, pos, lengths):
    """Straight-line definition: per column, CE over the real rows of each sequence with a valid position."""
    tot, cnt = [0.0, 0.0], [0, 0]
    for b, n in enumerate(lengths):
        for c in range(2):
            p = int(pos[b, c])
            if 0 <= p < n:
                x = logits[b, :n, c].double()
                tot[c] += float(torch.logsumexp(x, 0) - x[p])
                cnt[c] += 1
    return 0.5 * (tot[0] / max(cnt[0], 1) + tot[1] / max(cnt[1], 1)), cnt


@pytest.mark.parametrize("labels", [
    [[5, 64], [39, 39], [0, 16], [1, 1]],       # one label ignored (end >= len = 64)
    [[5, 9], [40, 39], [0, 16], [1, 1]],        # start == len of a shorter sequence: a padding row
    [[0, 0], [0, 39], [0, 16], [0, 1]],         # position 0 everywhere
    [[63, 63], [39, 39], [16, 16], [1, 1]],     # position len - 1
    [[-1, 9], [-100, -100], [3, 4], [2, 5]],    # negative positions; (2, 5) is past the 2-token sequence
])
def test_position_edge_cases(labels):
    labels = np.asarray(labels, dtype=np.int64)
    pk, mask, pad, pck = _both_layouts("hsd-tiny-distilbert", LENGTHS, labels, **NO_DROPOUT)
    want, cnt = _span_ref(pad[1], labels, LENGTHS)
    for loss, _, grads, stats, _ in (pad, pck):
        assert abs(float(loss) - want) < 1e-5 * max(1.0, abs(want))
        assert [int(stats[4]), int(stats[5])] == cnt
        valid = [(0 <= labels[b, 0] < n) and (0 <= labels[b, 1] < n) for b, n in enumerate(LENGTHS)]
        assert int(stats[2]) == sum(valid)
    _assert_same_step(pk, mask, pad, pck)
    # padding rows take no gradient: the padded position-embedding rows past the longest valid row stay zero
    emb = pad[2]["encoder.embeddings.word_embeddings"]
    assert torch.isfinite(emb).all()


def test_padding_rows_get_an_exactly_zero_head_gradient():
    g = torch.Generator().manual_seed(0)
    h = torch.randn(2 * 16, 32, generator=g).requires_grad_()
    w, b = (torch.randn(2, 32, generator=g) * 0.1).requires_grad_(), torch.zeros(2, requires_grad=True)
    mask = torch.ones(2, 16, dtype=torch.long)
    mask[0, 9:] = 0
    cu = torch.arange(3, dtype=torch.int32) * 16
    loss, _ = ops.qa_head(h, w, b, torch.tensor([[2, 3], [15, 15]]), cu, mask.reshape(-1), 0.0, 0, 30)
    loss.backward()
    assert torch.count_nonzero(h.grad[9:16]) == 0 and torch.count_nonzero(h.grad[:9]) > 0


# ------------------------------------------------------------------------------------------ best span
def _brute(start, end, real, mal):
    best, arg = float("-inf"), (0, 0)
    n = len(start)
    for s in range(n):
        for e in range(s, min(n, s + mal)):
            if real[s] and real[e]:
                v = float(np.float32(start[s]) + np.float32(end[e]))
                if v > best:
                    best, arg = v, (s, e)
    return arg


def test_best_span_matches_brute_force_and_never_returns_e_before_s():
    g = torch.Generator().manual_seed(4)
    lengths = [1, 2, 7, 30, 13]
    cu = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int32)
    R = int(cu[-1]) + 5  # dead rows after the last sequence
    logits = torch.randn(R, 2, generator=g).bfloat16().float()
    for mal in (1, 3, 30, 1000):
        pred = ref.span_best(logits, cu, None, mal)
        assert pred.dtype == torch.int32 and tuple(pred.shape) == (5, 2)
        for b, n in enumerate(lengths):
            x = logits[int(cu[b]):int(cu[b + 1])].numpy()
            assert tuple(pred[b].tolist()) == _brute(x[:, 0], x[:, 1], [True] * n, mal), (mal, b)
            s, e = pred[b].tolist()
            assert 0 <= s <= e < n and e - s < mal
    # the end logit peaks BEFORE the start logit's peak: the unconstrained argmaxes would give e < s
    lg = torch.zeros(10, 2)
    lg[7, 0] = 5.0
    lg[2, 1] = 5.0
    s, e = ref.span_best(lg, torch.tensor([0, 10], dtype=torch.int32), None, 30)[0].tolist()
    assert s <= e and (s, e) == (0, 2)  # 0 + 5 ties with 5 + 0 at (7, 7): the first in (s, e) order wins


def test_best_span_ties_resolve_to_the_first_pair_and_masked_rows_are_out():
    cu = torch.tensor([0, 8], dtype=torch.int32)
    lg = torch.zeros(8, 2)  # all equal: (0, 0)
    assert ref.span_best(lg, cu, None, 30)[0].tolist() == [0, 0]
    lg[3, 0] = lg[5, 0] = 1.0  # two equal starts, equal ends everywhere: (3, 3)
    assert ref.span_best(lg, cu, None, 30)[0].tolist() == [3, 3]
    lg[6, 1] = lg[4, 1] = 2.0  # first start, then the first of the two best ends
    assert ref.span_best(lg, cu, None, 30)[0].tolist() == [3, 4]
    assert ref.span_best(lg, cu, None, 1)[0].tolist() == [4, 4]  # max_answer_length 1: s == e, 0 + 2 first at row 4
    mask = torch.ones(8, dtype=torch.long)
    mask[3] = 0
    mask[4] = 0
    assert ref.span_best(lg, cu, mask, 30)[0].tolist() == [5, 6]
    assert ref.span_best(lg, cu, torch.zeros(8, dtype=torch.long), 30)[0].tolist() == [0, 0]  # no real row


def test_hits_count_exact_matches_over_sequences_with_both_labels_valid():
    cu = torch.tensor([0, 4, 8, 12], dtype=torch.int32)
    lg = torch.zeros(12, 2)
    lg[1, 0] = lg[2, 1] = 3.0     # sequence 0: best (1, 2)
    lg[4 + 0, 0] = lg[4 + 3, 1] = 3.0  # sequence 1: best (0, 3)
    lg[8 + 2, 0] = lg[8 + 2, 1] = 3.0  # sequence 2: best (2, 2)
    pos = torch.tensor([[1, 2], [0, 2], [2, 9]])  # exact; end wrong; end ignored
    loss, stats, pred = ref.span_loss(lg, pos, cu, None, 30)
    assert pred.tolist() == [[1, 2], [0, 3], [2, 2]]
    assert stats.tolist()[1:3] == [1.0, 2.0] and stats.tolist()[4:] == [3.0, 2.0, 3.0, 1.0]
    torch.testing.assert_close(stats[3], stats[0] * 2)


# ------------------------------------------------------------------------------------------ synthetic corpus
def test_synthetic_corpus_is_deterministic_and_every_label_is_inside_its_sequence():
    S, V = 32, 1024
    a = hdata.synthetic_question_answering(512, S, V, seed=5)
    b = hdata.synthetic_question_answering(512, S, V, seed=5)
    c = hdata.synthetic_question_answering(512, S, V, seed=6)
    assert np.array_equal(a.input_ids, b.input_ids) and np.array_equal(a.labels, b.labels)
    assert np.array_equal(a.token_type_ids, b.token_type_ids) and not np.array_equal(a.input_ids, c.input_ids)
    assert a.span_labels and a.labels.shape == (512, 2) and a.labels.dtype == np.int64
    table = hdata.answer_length_table(V)
    assert np.array_equal(table, hdata.answer_length_table(V)) and table.min() >= 0 and table.max() < 4
    for ds in (a, c):
        ids = ds.input_ids.astype(np.int64)
        lengths = ds.attention_mask.sum(axis=1)
        assert lengths.min() >= 12 and lengths.max() == S and len(set(lengths.tolist())) > 4
        rows = np.arange(len(ds))
        assert (ids[:, 0] == 101).all() and (ids[:, 2] == 102).all() and (ids[rows, lengths - 1] == 102).all()
        assert (ids[ds.attention_mask == 0] == 0).all()
        key = ids[:, 1]
        hits = (ids[:, 3:] == key[:, None]).sum(axis=1)
        none = (ds.labels == 0).all(axis=1)
        assert set(hits[none].tolist()) <= {0} and set(hits[~none].tolist()) == {1}  # exactly once, or not at all
        assert 0.05 < none.mean() < 0.16  # a seeded tenth (512 draws: 3 sigma is 0.04)
        s, e = ds.labels[~none, 0], ds.labels[~none, 1]
        assert (ids[rows[~none], s - 1] == key[~none]).all()  # the answer starts right after the key
        assert np.array_equal(e - s, table[ids[rows[~none], s]] % 4)
        assert (s >= 4).all() and (e <= lengths[~none] - 2).all()  # inside the context, before the final [SEP]
        tt = ds.token_type_ids
        assert (tt[:, :3] == 0).all() and (tt[ds.attention_mask == 0] == 0).all()
        assert (tt[:, 3:][ds.attention_mask[:, 3:] != 0] == 1).all()
    assert hdata.synthetic_question_answering(8, S, V, seed=0, segment_ids=False).token_type_ids is None


def test_tiny_model_learns_the_synthetic_spans_on_cpu():
    """2-layer hsd-tiny-bert (H = 64) with segment ids, vocabulary cut to 64 tokens, S = 32, batch 32, Adam lr 3e-3,
    fp32, 300 steps on CPU, sized as the token task's marker test. A model that always answers (0, 0) scores the
    no-answer tenth, about 0.10; picking a span at random scores below 0.01. The test asserts a held-out exact match
    above 0.30, which needs the key's position."""
    torch.manual_seed(0)
    V, S = 64, 32
    cfg = resolve_config("hsd-tiny-bert").replace(vocab_size=V, max_position_embeddings=S)
    model = build_model(cfg, task=MODEL_TASK, seed=0).train()
    kw = dict(cls_id=1, sep_id=2)
    tr = hdata.synthetic_question_answering(32 * 300, S, V, seed=0, **kw)
    te = hdata.synthetic_question_answering(256, S, V, seed=1, **kw)
    opt = torch.optim.Adam(model.parameters(), lr=3e-3)
    ti = lambda a: t(np.asarray(a).astype(np.int64))  # noqa: E731
    for step in range(300):
        sl = slice(32 * step, 32 * (step + 1))
        model.rng.new_step(step)
        loss, _ = model(ti(tr.input_ids[sl]), attention_mask=ti(tr.attention_mask[sl]),
                        token_type_ids=ti(tr.token_type_ids[sl]), labels=ti(tr.labels[sl]))
        opt.zero_grad()
        loss.backward()
        opt.step()
    model.eval()
    with torch.no_grad():
        loss, _ = model(ti(te.input_ids), attention_mask=ti(te.attention_mask),
                        token_type_ids=ti(te.token_type_ids), labels=ti(te.labels))
    stats = loss._hsd_stats
    acc = float(stats[1] / stats[2])
    print(f"held-out exact match {acc:.3f}, loss {float(loss):.3f}")
    assert float(stats[2]) == 256.0
    assert acc > 0.30


# ------------------------------------------------------------------------------------------ SQuAD reader
CONTEXT = ("the movie was really good and the acting was excellent but the plot was boring and i would not watch it "
           "again even if the story was the best one of the two")
SQUAD = {"version": "v2.0", "data": [{"title": "t", "paragraphs": [{"context": CONTEXT, "qas": [
    {"id": "q1", "question": "how was the acting", "answers": [{"text": "excellent", "answer_start": CONTEXT.index("excellent")}]},
    {"id": "q2", "question": "which story", "answers": [{"text": "the best one", "answer_start": CONTEXT.index("the best one")}]},
    {"id": "q3", "question": "who", "is_impossible": True, "answers": []},
]}]}]}


def test_squad_reader_windows_offsets_and_out_of_window_answers(tmp_path):
    pytest.importorskip("tokenizers")
    p = tmp_path / "train-v2.0.json"
    p.write_text(json.dumps(SQUAD))
    ex = hdata.read_squad(str(p))
    assert [e["id"] for e in ex] == ["q1", "q2", "q3"] and ex[2]["answers"] == []
    assert ex[0]["answers"] == [("excellent", CONTEXT.index("excellent"))]
    tok = hdata.load_tokenizer(None, 1024)
    S, stride = 24, 6
    tok.backend.no_truncation()
    tok.backend.no_padding()
    count = lambda text: len(tok.backend.encode(text, add_special_tokens=False).ids)  # noqa: E731
    nctx, nqs = count(CONTEXT), [count(e["question"]) for e in ex]
    enc = tok.encode_pairs([e["question"] for e in ex], [e["context"] for e in ex], S, stride)
    want = []
    for nq in nqs:
        room = S - 3 - nq  # [CLS] q [SEP] ... [SEP]: what a window holds of the context
        want.append(1 + -(-(nctx - room) // (room - stride)))  # each further window brings room - stride new tokens
    counts = np.bincount(enc["sample"], minlength=3).tolist()
    assert counts == want and enc["input_ids"].shape == (sum(want), S)
    # only the context is truncated: every window starts with the whole question
    q1 = enc["input_ids"][enc["sample"] == 0]
    nq1 = 2 + nqs[0]
    assert (q1[:, :nq1] == q1[0, :nq1]).all() and (enc["token_type_ids"][enc["sample"] == 0][:, :nq1] == 0).all()
    assert (enc["token_type_ids"][enc["sample"] == 0][:, nq1] == 1).all()
    ds = hdata.tokenize_squad(tok, ex, S, stride)
    assert ds.span_labels and ds.labels.shape == (sum(want), 2) and ds.token_type_ids.shape == ds.input_ids.shape
    found = {0: 0, 1: 0, 2: 0}
    for w in range(len(ds)):
        i = int(ds.example_index[w])
        s, e = ds.labels[w].tolist()
        if (s, e) == (0, 0):
            continue
        found[i] += 1
        text = tok.backend.decode(ds.input_ids[w, s:e + 1].tolist())
        assert text == ex[i]["answers"][0][0], (w, text)
        assert (ds.token_type_ids[w, s:e + 1] == 1).all() and ds.attention_mask[w, e] == 1
    assert found[0] >= 1 and found[1] >= 1 and found[2] == 0  # the impossible question: (0, 0) in every window
    assert found[0] < want[0] and found[1] < want[1]  # and windows without the answer carry (0, 0)
    assert hdata.tokenize_squad(tok, ex, S, stride, segment_ids=False).token_type_ids is None


# ------------------------------------------------------------------------------------------ CLI and data path
def test_flags_parse_with_their_defaults():
    a, _ = parse_args(["--task", TASK], "train")
    assert a.task == TASK and a.max_answer_length == 30 and a.doc_stride == 128
    a, _ = parse_args(["--task", TASK, "--max_answer_length", "12", "--doc_stride", "64", "--dataset", "squad"],
                      "train")
    assert a.max_answer_length == 12 and a.doc_stride == 64 and a.dataset == "squad"


def test_pack_batch_passes_span_labels_through_and_packs_segment_ids():
    ids = np.arange(1, 13).reshape(2, 6)
    mask = np.array([[1, 1, 1, 1, 0, 0], [1, 1, 1, 1, 1, 1]])
    tt = np.array([[0, 0, 1, 1, 0, 0], [0, 1, 1, 1, 1, 1]])
    spans = np.array([[2, 3], [1, 5]])
    rule = dict(pad_id=0, pos_base=0, pad_pos=0, row_multiple=8)
    with pytest.raises(ValueError):
        pack_batch(ids, mask, spans, **rule)  # the default keeps today's behaviour: [B, 2] is not [B, S]
    pk = pack_batch(ids, mask, spans, **rule, span_labels=True, token_type_ids=tt)
    assert np.array_equal(pk["labels"], spans) and pk["cu_seqlens"].tolist() == [0, 4, 10]
    assert pk["token_type_ids"].shape == (1, 16) and pk["token_type_ids"].dtype == np.int64
    assert pk["token_type_ids"][0].tolist() == [0, 0, 1, 1, 0, 1, 1, 1, 1, 1] + [0] * 6
    assert "token_type_ids" not in pack_batch(ids, mask, np.zeros(2, dtype=np.int64), **rule)
    with pytest.raises(ValueError):
        pack_batch(ids, mask, np.zeros((2, 3), dtype=np.int64), **rule, span_labels=True)


def test_loader_delivers_segment_ids_only_when_the_dataset_has_them():
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import ShardSampler

    ds = hdata.synthetic_question_answering(16, 16, 256, seed=0)
    dev = torch.device("cpu")
    for pack in (False, True):
        ld = hdata.BatchLoader(ds, ShardSampler(16, 0, 1, shuffle=False, seed=0, batch_size=8), dev, pack=pack)
        b = next(iter(ld))
        assert tuple(b["labels"].shape) == (8, 2) and b["labels"].dtype == torch.int64
        assert b["token_type_ids"].shape == b["input_ids"].shape and b["token_type_ids"].dtype == torch.int64
    plain = hdata.synthetic_classification(16, 16, 256, seed=0)
    b = next(iter(hdata.BatchLoader(plain, ShardSampler(16, 0, 1, shuffle=False, seed=0, batch_size=8), dev)))
    assert sorted(b) == ["attention_mask", "input_ids", "labels"]


def _cli(tmp, extra, model="hsd-tiny-bert"):
    env = dict(os.environ, SM_OUTPUT_DATA_DIR=str(tmp / "data"), SM_MODEL_DIR=str(tmp / "model"), SM_NUM_GPUS="0",
               SM_FRAMEWORK_PARAMS="{}")
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "train.py"), "--epochs", "1", "--train_batch_size", "8",
           "--eval_batch_size", "8", "--model_name_or_path", model, "--max_seq_length", "32",
           "--num_train_examples", "32", "--num_eval_examples", "16", "--device", "cpu", "--log_every", "0",
           "--task", TASK] + extra
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)


def _results(path):
    return dict(line.split(" = ") for line in path.read_text().splitlines())


@pytest.mark.parametrize("pack", ["false", "true"])
def test_cli_trains_on_the_synthetic_corpus(tmp_path, pack):
    r = _cli(tmp_path, ["--dataset", "synthetic", "--max_steps", "2", "--max_answer_length", "8",
                        "--pack_sequences", pack])
    assert r.returncode == 0, r.stderr[-3000:]
    prov = json.load(open(tmp_path / "data" / "run_provenance.json"))
    assert prov["task"] == TASK and prov["max_answer_length"] == 8 and prov["synthetic_data"] is True
    assert "span corpus" in prov["corpus"]
    tr, ev = _results(tmp_path / "data" / "train_results.txt"), _results(tmp_path / "data" / "eval_results.txt")
    assert np.isfinite(json.loads(tr["loss"])).all() and 0.0 <= float(ev["sparse_categorical_accuracy"]) <= 1.0
    conf = json.load(open(tmp_path / "model" / "config.json"))
    assert conf["architectures"] == ["BertForQuestionAnswering"]
    assert os.path.isfile(tmp_path / "model" / "model.safetensors")


def test_cli_reads_a_squad_directory(tmp_path):
    pytest.importorskip("tokenizers")
    d = tmp_path / "squad"
    d.mkdir()
    (d / "train-v2.0.json").write_text(json.dumps(SQUAD))
    (d / "dev-v2.0.json").write_text(json.dumps(SQUAD))
    r = _cli(tmp_path, ["--dataset", "squad", "--dataset_dir", str(d), "--doc_stride", "8"],
             model="hsd-tiny-distilbert")
    assert r.returncode == 0, r.stderr[-3000:]
    prov = json.load(open(tmp_path / "data" / "run_provenance.json"))
    assert "doc_stride 8" in prov["corpus"] and prov["synthetic_data"] is False
    assert json.load(open(tmp_path / "model" / "config.json"))["architectures"] == ["DistilBertForQuestionAnswering"]


@pytest.mark.parametrize("dataset", ["imdb", "conll", "synthetic-bigram"])
def test_cli_refuses_datasets_without_answer_spans(tmp_path, dataset):
    r = _cli(tmp_path, ["--dataset", dataset])
    assert r.returncode != 0 and "answer spans" in r.stderr


def test_cli_refuses_squad_for_the_other_tasks(tmp_path):
    env = dict(os.environ, SM_OUTPUT_DATA_DIR=str(tmp_path / "data"), SM_MODEL_DIR=str(tmp_path / "model"),
               SM_NUM_GPUS="0", SM_FRAMEWORK_PARAMS="{}")
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "train.py"), "--epochs", "1", "--model_name_or_path",
           "hsd-tiny-bert", "--device", "cpu", "--dataset", "squad", "--max_seq_length", "32"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "question-answering" in r.stderr
