"""--problem_type: regression (MSE) and multi-label (BCE-with-logits) sequence-classification heads, CPU tier (fp32).

The definition (``ops.reference.seq_loss``, ``ModelConfig.problem_type``) against Hugging Face's
``*ForSequenceClassification`` with ``config.problem_type`` set, the ignored (NaN) rows, packing, the config round
trip, the data path and the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from huggingface_sagemaker_tensorflow_distributed_amd import data as hdata
from huggingface_sagemaker_tensorflow_distributed_amd import ops
from huggingface_sagemaker_tensorflow_distributed_amd.data.loader import BatchLoader
from huggingface_sagemaker_tensorflow_distributed_amd.data.packing import pack_batch, position_rule
from huggingface_sagemaker_tensorflow_distributed_amd.models import (ModelConfig, build_model, from_pretrained,
                                                                     hf_state_dict, resolve_config, save_pretrained)
from huggingface_sagemaker_tensorflow_distributed_amd.ops import reference as ref
from huggingface_sagemaker_tensorflow_distributed_amd.parallel.sampler import ShardSampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["hsd-tiny-bert", "hsd-tiny-roberta", "hsd-tiny-distilbert"]
MSE, BCE, CE = "regression", "multi_label_classification", "single_label_classification"
CASES = [(MSE, 1), (MSE, 3), (BCE, 6)]
NAN = float("nan")


def _targets(ptype, B, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, C, generator=g) < 0.4).float() if ptype == BCE else torch.randn(B, C, generator=g)


def _inputs(cfg, B=3, S=24, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(5, cfg.vocab_size, (B, S), generator=g)
    am = torch.ones(B, S, dtype=torch.long)
    am[1, 15:] = 0
    ids[1, 15:] = cfg.pad_token_id
    return ids, am


# ------------------------------------------------------------------------------------------ HF parity
@pytest.mark.parametrize("ptype,C", CASES)
@pytest.mark.parametrize("name", NAMES)
def test_loss_and_logits_parity_with_transformers(name, ptype, C):
    pytest.importorskip("transformers")
    from transformers import AutoConfig, AutoModelForSequenceClassification

    ours = build_model(resolve_config(name, num_labels=C), seed=3, problem_type=ptype).eval()
    d = ours.cfg.to_hf_dict()
    assert d["problem_type"] == ptype
    hc = AutoConfig.for_model(d.pop("model_type"), **d)
    hc._attn_implementation = "eager"
    hf = AutoModelForSequenceClassification.from_config(hc).eval()
    assert hf.config.problem_type == ptype
    hf.load_state_dict(hf_state_dict(ours), strict=True)
    ids, am = _inputs(ours.cfg)
    y = _targets(ptype, 3, C)
    with torch.no_grad():
        loss, logits = ours(ids, attention_mask=am, labels=y)
        out = hf(input_ids=ids, attention_mask=am, labels=y)
        loss1, _ = ours(ids, attention_mask=am, labels=y[:, 0]) if C == 1 else (loss, None)  # [B] accepted when C = 1
    torch.testing.assert_close(logits, out.logits, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(loss, out.loss, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(loss1, loss, rtol=0, atol=0)
    assert loss._hsd_stats[2].item() == 3 and abs(loss._hsd_stats[3].item() - 3 * loss.item()) < 1e-5


def test_seq_loss_formulas_and_metric():
    z = torch.tensor([[2.0, -1.0, 0.5], [0.2, 0.3, -4.0], [-1.0, -2.0, -3.0], [9.0, 9.0, 9.0]])
    y = torch.tensor([[1.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [NAN, 1.0, 1.0]])
    loss, stats = ref.seq_loss(z, y, BCE)
    want = torch.nn.functional.binary_cross_entropy_with_logits(z[:3], y[:3])
    torch.testing.assert_close(loss, want)
    assert stats.tolist()[1:3] == [2.0, 3.0]  # rows 0 and 2 have every label right; row 1 misses label 1
    yr = torch.tensor([[2.4, -1.0, 0.0], [0.2, 0.3, -3.4], [-1.0, -2.0, -3.0], [NAN, 0.0, 0.0]])
    loss, stats = ref.seq_loss(z, yr, MSE, tol=0.5)
    torch.testing.assert_close(loss, torch.nn.functional.mse_loss(z[:3], yr[:3]))
    assert stats.tolist()[1:3] == [2.0, 3.0]  # row 1: |-4 + 3.4| = 0.6 > 0.5
    assert ref.seq_loss(z, yr, MSE, tol=0.7)[1][1].item() == 3.0
    # single-label: today's CE, -100 ignored
    lab = torch.tensor([0, 1, -100, 2])
    loss, stats = ref.seq_loss(z, lab, CE)
    torch.testing.assert_close(loss, torch.nn.functional.cross_entropy(z, lab, ignore_index=-100))
    assert stats.tolist()[1:3] == [2.0, 3.0]
    with pytest.raises(ValueError):
        ref.seq_loss(z, y, "ranking")


# ------------------------------------------------------------------------------------------ ignored rows
@pytest.mark.parametrize("ptype,C", CASES)
def test_nan_rows_are_ignored(ptype, C):
    m = build_model(resolve_config("hsd-tiny-bert", num_labels=C), seed=1, problem_type=ptype).eval()
    ids, am = _inputs(m.cfg, B=5)
    y = _targets(ptype, 5, C)
    keep = torch.tensor([0, 2, 3])
    sub, _ = m(ids[keep], attention_mask=am[keep], labels=y[keep])
    y2 = y.clone()
    y2[1] = NAN
    y2[4, 0] = NAN  # the FIRST label decides
    loss, logits = m(ids, attention_mask=am, labels=y2)
    torch.testing.assert_close(loss, sub, rtol=1e-5, atol=1e-6)
    assert loss._hsd_stats[2].item() == 3 and torch.isfinite(logits).all()
    m.zero_grad()
    loss.backward()
    g = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad()
    sub.backward()
    for n, p in m.named_parameters():
        torch.testing.assert_close(g[n], p.grad, rtol=1e-4, atol=1e-7, msg=lambda s, n=n: f"{n}: {s}")


@pytest.mark.parametrize("ptype,C", CASES)
def test_all_rows_ignored_gives_zero_loss_and_zero_gradients(ptype, C):
    m = build_model(resolve_config("hsd-tiny-roberta", num_labels=C), seed=1, problem_type=ptype).train()
    ids, am = _inputs(m.cfg)
    loss, _ = m(ids, attention_mask=am, labels=torch.full((3, C), NAN))
    loss.backward()
    assert loss.item() == 0.0 and loss._hsd_stats.tolist() == [0.0, 0.0, 0.0, 0.0]
    for n, p in m.named_parameters():
        assert p.grad is None or torch.count_nonzero(p.grad) == 0, n


# ------------------------------------------------------------------------------------------ packing
@pytest.mark.parametrize("ptype,C", CASES)
@pytest.mark.parametrize("name", NAMES)
def test_packed_step_equals_padded_step(name, ptype, C):
    cfg = resolve_config(name, num_labels=C).replace(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                                                     classifier_dropout=0.0, seq_classif_dropout=0.0)
    model = build_model(cfg, seed=1, problem_type=ptype).train()
    g = np.random.default_rng(3)
    lengths, S = [64, 40, 17, 2], 64
    ids = g.integers(5, cfg.vocab_size, size=(4, S)).astype(np.int64)
    mask = (np.arange(S)[None, :] < np.asarray(lengths)[:, None]).astype(np.int64)
    ids[mask == 0] = cfg.pad_token_id
    y = _targets(ptype, 4, C, seed=5).numpy()
    y[2] = np.nan
    t = torch.from_numpy

    def step(**kw):
        model.zero_grad(set_to_none=True)
        model.rng.new_step(0)
        loss, logits = model(**kw)
        loss.backward()
        return loss.detach(), logits.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}

    l0, lg0, g0 = step(input_ids=t(ids), attention_mask=t(mask), labels=t(y))
    pk = pack_batch(ids, mask, y, row_targets=True, **position_rule(cfg))
    assert pk["labels"].dtype == np.float32 and pk["labels"].shape == (4, C)
    l1, lg1, g1 = step(input_ids=t(pk["input_ids"]), labels=t(pk["labels"]), cu_seqlens=t(pk["cu_seqlens"]),
                       max_seqlen=pk["max_seqlen"], position_ids=t(pk["position_ids"]))
    torch.testing.assert_close(l1, l0, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(lg1, lg0, rtol=1e-5, atol=1e-6)
    for n in g0:
        torch.testing.assert_close(g1[n], g0[n], rtol=1e-5, atol=1e-6, msg=lambda s, n=n: f"{n}: {s}")


def test_pack_batch_does_not_take_row_targets_for_token_labels():
    ids = np.full((4, 4), 7, dtype=np.int64)
    mask = np.ones((4, 4), dtype=np.int64)
    y = np.arange(16, dtype=np.float32).reshape(4, 4)  # C == S: the shape alone cannot tell
    pk = pack_batch(ids, mask, y, row_targets=True, pad_id=0, pos_base=0, pad_pos=0)
    assert pk["labels"].shape == (4, 4) and pk["labels"].dtype == np.float32 and np.array_equal(pk["labels"], y)


# ------------------------------------------------------------------------------------------ config
def test_config_round_trip_and_refusals(tmp_path):
    assert ModelConfig().problem_type is None and "problem_type" not in ModelConfig().to_hf_dict()
    for name in NAMES:
        cfg = resolve_config(name, num_labels=4).replace(problem_type=BCE)
        d = cfg.to_hf_dict()
        assert d["problem_type"] == BCE and ModelConfig.from_hf_dict(d).problem_type == BCE
        assert ModelConfig.from_hf_dict(resolve_config(name).to_hf_dict()).problem_type is None
    with pytest.raises(ValueError):
        ModelConfig.from_hf_dict({"model_type": "bert", "problem_type": "ranking"})
    with pytest.raises(ValueError):
        build_model(resolve_config("hsd-tiny-bert"), problem_type="ranking")
    for task in ("token-classification", "span-extraction"):
        with pytest.raises(ValueError):
            build_model(resolve_config("hsd-tiny-bert"), task=task, problem_type=MSE)
    with pytest.raises(ValueError):
        build_model(resolve_config("hsd-tiny-roberta"), task="masked-lm", problem_type=MSE)
    with pytest.raises(ValueError):
        from_pretrained("hsd-tiny-bert", task="question-answering", problem_type=BCE)
    m = from_pretrained("hsd-tiny-bert", num_labels=3, problem_type=MSE)
    assert m.cfg.problem_type == MSE
    save_pretrained(m, str(tmp_path))
    assert json.load(open(tmp_path / "config.json"))["problem_type"] == MSE
    again = from_pretrained(str(tmp_path))
    assert again.cfg.problem_type == MSE and again.cfg.num_labels == 3
    assert from_pretrained(str(tmp_path), problem_type=BCE).cfg.problem_type == BCE


@pytest.mark.parametrize("ptype,C", CASES)
def test_save_pretrained_loads_in_transformers_with_the_same_loss(tmp_path, ptype, C):
    pytest.importorskip("transformers")
    from transformers import AutoModelForSequenceClassification

    ours = build_model(resolve_config("hsd-tiny-bert", num_labels=C), seed=7, problem_type=ptype).eval()
    save_pretrained(ours, str(tmp_path))
    hf = AutoModelForSequenceClassification.from_pretrained(str(tmp_path)).eval()
    assert hf.config.problem_type == ptype
    ids, am = _inputs(ours.cfg)
    y = _targets(ptype, 3, C)
    with torch.no_grad():
        loss, _ = ours(ids, attention_mask=am, labels=y)
        torch.testing.assert_close(loss, hf(input_ids=ids, attention_mask=am, labels=y).loss, rtol=1e-5, atol=1e-6)


def test_none_still_means_single_label_for_one_label():
    m = build_model(resolve_config("hsd-tiny-bert", num_labels=1), seed=2).eval()
    assert m.cfg.problem_type is None
    ids, am = _inputs(m.cfg)
    lab = torch.zeros(3, dtype=torch.long)
    loss, logits = m(ids, attention_mask=am, labels=lab)
    assert logits.shape == (3, 1) and loss.item() == 0.0  # CE over one class, not MSE
    torch.testing.assert_close(loss, torch.nn.functional.cross_entropy(logits, lab))
    # ops.cls_head: the positional signature and its behaviour without the keywords are unchanged
    h = torch.randn(3, 2, 8)
    w1, b1, w2, b2 = torch.randn(8, 8), torch.randn(8), torch.randn(2, 8), torch.randn(2)
    a, la = ops.cls_head(h, w1, b1, w2, b2, torch.tensor([0, 1, 1]), "tanh", 0.0, 0, 0.0, 0)
    b, lb = ops.cls_head(h, w1, b1, w2, b2, torch.tensor([0, 1, 1]), "tanh", 0.0, 0, 0.0, 0, problem_type=CE, tol=0.5)
    torch.testing.assert_close(a, b)
    torch.testing.assert_close(la, lb)
    assert b._hsd_stats[2].item() == 3


# ------------------------------------------------------------------------------------------ data
def test_loader_keeps_float_targets_and_pads_with_nan():
    ds = hdata.synthetic_regression(10, 16, 1024, seed=0, num_labels=3)
    assert ds.row_targets and ds.labels.dtype == np.float32 and ds.labels.shape == (10, 3)
    want = torch.from_numpy(ds.labels)
    for pack in (False, True):
        # 10 examples over 4 ranks: ranks 2 and 3 get one repeat each that only evens out the shards
        for rank, rows in ((0, [0, 4, 8]), (3, [3, 7, None])):
            sampler = ShardSampler(len(ds), rank=rank, world_size=4, drop_last=False, batch_size=3, mark_padding=True)
            (b,) = list(BatchLoader(ds, sampler, torch.device("cpu"), pack=pack))
            lab = b["labels"]
            assert lab.dtype == torch.float32 and lab.shape == (3, 3)
            for k, r in enumerate(rows):
                if r is None:
                    assert torch.isnan(lab[k]).all() and b["num_valid"] == 2
                else:
                    assert torch.equal(lab[k], want[r])
    # int labels keep their path
    ints = hdata.synthetic_classification(10, 16, 1024, seed=0)
    (b,) = list(BatchLoader(ints, ShardSampler(10, rank=3, world_size=4, drop_last=False, batch_size=3,
                                               mark_padding=True), torch.device("cpu")))
    assert b["labels"].dtype == torch.int64 and b["labels"][2].item() == -100


def test_synthetic_corpora_are_deterministic_functions_of_the_tokens():
    V, S = 1024, 32
    a = hdata.synthetic_regression(64, S, V, seed=4, num_labels=3)
    b = hdata.synthetic_regression(64, S, V, seed=4, num_labels=3)
    assert np.array_equal(a.input_ids, b.input_ids) and np.array_equal(a.labels, b.labels)
    other = hdata.synthetic_regression(64, S, V, seed=5, num_labels=3)
    assert not np.array_equal(a.input_ids, other.input_ids)
    from huggingface_sagemaker_tensorflow_distributed_amd.data.datasets import (multi_label_marker_table,
                                                                                 regression_marker_table)

    marks = regression_marker_table(V)
    assert len(set(marks.tolist())) == 16
    lengths = a.attention_mask.sum(1)
    assert lengths.min() < S and lengths.max() <= S  # ragged
    for ds in (a, other):  # one language for both splits: the targets follow from the tokens and the fixed table
        for i in range(len(ds)):
            hit = [(int(p), int(np.nonzero(marks == t)[0][0])) for p, t in enumerate(ds.input_ids[i]) if t in marks]
            assert len(hit) == 1 and 1 <= hit[0][0] < ds.attention_mask[i].sum() - 1
            j = hit[0][1]
            want = [((j * (2 * c + 1)) % 16) / 4 - 2 for c in range(3)]
            assert ds.labels[i].tolist() == want
    m = hdata.synthetic_multi_label(256, S, V, seed=4, num_labels=6)
    m2 = hdata.synthetic_multi_label(256, S, V, seed=4, num_labels=6)
    assert np.array_equal(m.input_ids, m2.input_ids) and np.array_equal(m.labels, m2.labels)
    mm = multi_label_marker_table(V, 6)
    assert len(set(mm.tolist())) == 6
    for i in range(len(m)):
        L = int(m.attention_mask[i].sum())
        present = np.array([float((m.input_ids[i, 1:L - 1] == t).sum()) for t in mm], dtype=np.float32)
        assert set(present.tolist()) <= {0.0, 1.0} and np.array_equal(present, m.labels[i])
    assert 0.15 < m.labels.mean() < 0.35  # each label present with probability 1/4
    # more labels than interior positions: the ones that find no free position are dropped, their label is 0
    tight = hdata.synthetic_multi_label(64, 8, V, seed=1, num_labels=40)
    assert (tight.labels.sum(1) <= tight.attention_mask.sum(1) - 2).all()


def test_local_files_yield_float_targets(tmp_path):
    (tmp_path / "train.csv").write_text("text,label\nhello there,0.5\nbye now,-1.25\n")
    texts, y = hdata.load_text_split(str(tmp_path), "train", None, problem_type=MSE, num_labels=1)
    assert texts == ["hello there", "bye now"] and y == [[0.5], [-1.25]]
    (tmp_path / "test.jsonl").write_text('{"text": "a", "labels": [1, 0, 1]}\n{"text": "b", "labels": [0, 0, 0]}\n')
    _, y = hdata.load_text_split(str(tmp_path), "test", None, problem_type=BCE, num_labels=3)
    assert y == [[1.0, 0.0, 1.0], [0.0, 0.0, 0.0]]
    d2 = tmp_path / "cols"
    d2.mkdir()
    (d2 / "train.csv").write_text("text,label_0,label_1\nx,1,0\ny,0,1\n")
    _, y = hdata.load_text_split(str(d2), "train", None, problem_type=BCE, num_labels=2)
    assert y == [[1.0, 0.0], [0.0, 1.0]]
    with pytest.raises(ValueError):
        hdata.load_text_split(str(d2), "train", None, problem_type=BCE, num_labels=3)
    with pytest.raises(ValueError):
        hdata.load_text_split("imdb", "train", None, problem_type=MSE, num_labels=1)


# ------------------------------------------------------------------------------------------ CLI
def _cli(tmp, extra, task="sequence-classification"):
    env = dict(os.environ, SM_OUTPUT_DATA_DIR=str(tmp / "data"), SM_MODEL_DIR=str(tmp / "model"), SM_NUM_GPUS="0",
               SM_FRAMEWORK_PARAMS="{}")
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "train.py"), "--epochs", "1", "--train_batch_size", "8",
           "--eval_batch_size", "8", "--model_name_or_path", "hsd-tiny-bert", "--max_seq_length", "32",
           "--num_train_examples", "32", "--num_eval_examples", "20", "--device", "cpu", "--log_every", "0",
           "--task", task] + extra
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)


def _results(path):
    return dict(line.split(" = ") for line in path.read_text().splitlines())


@pytest.mark.parametrize("ptype,C,extra", [(MSE, 2, ["--regression_tolerance", "0.25"]),
                                           (BCE, 5, ["--pack_sequences", "true"]), (CE, 3, [])])
def test_cli_run_per_problem_type(tmp_path, ptype, C, extra):
    r = _cli(tmp_path, ["--dataset", "synthetic", "--problem_type", ptype, "--num_labels", str(C)] + extra)
    assert r.returncode == 0, r.stderr[-3000:]
    prov = json.load(open(tmp_path / "data" / "run_provenance.json"))
    assert prov["problem_type"] == ptype and prov["num_labels"] == C and "metric" in prov
    if ptype == MSE:
        assert prov["regression_tolerance"] == 0.25 and "regression" in prov["corpus"]
    tr, ev = _results(tmp_path / "data" / "train_results.txt"), _results(tmp_path / "data" / "eval_results.txt")
    assert np.isfinite(json.loads(tr["loss"])).all() and np.isfinite(float(ev["loss"]))
    assert 0.0 <= float(ev["sparse_categorical_accuracy"]) <= 1.0
    conf = json.load(open(tmp_path / "model" / "config.json"))
    assert conf["problem_type"] == ptype and len(conf["id2label"]) == C
    assert from_pretrained(str(tmp_path / "model")).cfg.problem_type == ptype


def test_cli_refusals(tmp_path):
    r = _cli(tmp_path, ["--dataset", "synthetic", "--problem_type", MSE], task="token-classification")
    assert r.returncode != 0 and "--problem_type" in r.stderr and "sequence-classification" in r.stderr
    r = _cli(tmp_path, ["--dataset", "imdb", "--problem_type", MSE, "--num_labels", "1"])
    assert r.returncode != 0 and "one class per text" in r.stderr
    r = _cli(tmp_path, ["--dataset", "synthetic", "--problem_type", "ranking"])
    assert r.returncode != 0


# ------------------------------------------------------------------------------------------ learning
def _learn(ptype, C, steps, lr):
    from huggingface_sagemaker_tensorflow_distributed_amd.train.runner import build
    from huggingface_sagemaker_tensorflow_distributed_amd.utils.args import build_parser

    args, _ = build_parser("train").parse_known_args(
        ["--model_name_or_path", "hsd-tiny-bert", "--train_batch_size", "16", "--learning_rate", lr, "--log_every", "0",
         "--device", "cpu", "--seed", "7", "--problem_type", ptype, "--num_labels", str(C)])
    tr = build(args, "train")["trainer"]
    make = hdata.synthetic_regression if ptype == MSE else hdata.synthetic_multi_label
    ds = make(16 * steps, 32, tr.model.cfg.vocab_size, seed=1, num_labels=C)
    losses = []
    for i in range(steps):
        sl = slice(16 * i, 16 * (i + 1))
        losses.append(float(tr.train_step([{"input_ids": torch.from_numpy(ds.input_ids[sl]).long(),
                                            "attention_mask": torch.from_numpy(ds.attention_mask[sl]).long(),
                                            "labels": torch.from_numpy(ds.labels[sl])}]).detach()))
    return losses


def test_tiny_bert_learns_the_regression_corpus_on_cpu():
    """tests/test_training.py::test_tiny_bert_learns_the_marker_task_on_cpu on the regression corpus: the targets are
    uniform over 16 values in [-2, 1.75] (variance ~1.33, so predicting the mean costs ~1.33); a model that reads the
    marker gets far below a tenth of that."""
    losses = _learn(MSE, 2, 150, "2e-3")
    assert sum(losses[:10]) / 10 > 0.8 and sum(losses[-20:]) / 20 < 0.13, losses[::10]


def test_tiny_bert_learns_the_multi_label_corpus_on_cpu():
    """... and on the multi-label corpus: predicting the prior 1/4 costs H(1/4) = 0.562 nats per label; reading the
    markers gets under a third of it. (Two labels and 300 steps: a 2-layer H = 64 model finds the markers one label
    after the other.)"""
    losses = _learn(BCE, 2, 300, "3e-3")
    assert sum(losses[:10]) / 10 > 0.5 and sum(losses[-20:]) / 20 < 0.19, losses[::10]
