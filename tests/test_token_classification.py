"""--task token-classification on the CPU tier: the model against transformers, packed == padded, the all-ignored
batch, the synthetic tagging corpus, the CoNLL reader and word alignment, and the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from huggingface_sagemaker_tensorflow_distributed_amd import data as hdata
from huggingface_sagemaker_tensorflow_distributed_amd import ops
from huggingface_sagemaker_tensorflow_distributed_amd.data.packing import pack_batch, position_rule, unpack_rows
from huggingface_sagemaker_tensorflow_distributed_amd.models import (build_model, from_pretrained, hf_state_dict,
                                                                     resolve_config, save_pretrained)
from huggingface_sagemaker_tensorflow_distributed_amd.ops import reference as ref
from huggingface_sagemaker_tensorflow_distributed_amd.ops import rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASK = "token-classification"
NAMES = ["hsd-tiny-bert", "hsd-tiny-roberta", "hsd-tiny-distilbert"]


# ------------------------------------------------------------------------------------------ model vs transformers
def _hf_model(cfg):
    pytest.importorskip("transformers")
    from transformers import AutoConfig, AutoModelForTokenClassification

    d = cfg.to_hf_dict()
    hc = AutoConfig.for_model(d.pop("model_type"), **d)
    hc._attn_implementation = "eager"
    return AutoModelForTokenClassification.from_config(hc).eval()


def _token_batch(cfg, B=3, S=24, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(5, cfg.vocab_size, (B, S), generator=g)
    am = torch.ones(B, S, dtype=torch.long)
    am[1, 15:] = 0
    ids[1, 15:] = cfg.pad_token_id
    labels = torch.randint(0, cfg.num_labels, (B, S), generator=g)
    labels[torch.rand(B, S, generator=g) < 0.25] = -100
    labels[:, 0] = -100
    labels[am == 0] = -100
    return ids, am, labels


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_keys_and_architecture_match_hf(name):
    cfg = resolve_config(name, num_labels=5)
    m = build_model(cfg, task=TASK)
    ours = hf_state_dict(m)
    theirs = _hf_model(cfg).state_dict()
    assert set(ours) == set(theirs), (set(ours) ^ set(theirs))
    for k in ours:
        assert tuple(ours[k].shape) == tuple(theirs[k].shape), k
    assert m.architecture() == {"hsd-tiny-bert": "BertForTokenClassification",
                                "hsd-tiny-roberta": "RobertaForTokenClassification",
                                "hsd-tiny-distilbert": "DistilBertForTokenClassification"}[name]
    assert tuple(m.classifier_weight.shape) == (5, cfg.hidden_size) and tuple(m.classifier_bias.shape) == (5,)


@pytest.mark.parametrize("name", NAMES)
def test_logits_and_loss_parity_with_transformers(name):
    """Eval mode, labels with -100 scattered over real tokens, the first column and the padding: logits and loss at
    the tolerance of tests/test_models.py's sequence-classification parity test."""
    cfg = resolve_config(name, num_labels=5)
    ours = build_model(cfg, task=TASK, seed=3).eval()
    hf = _hf_model(cfg)
    hf.load_state_dict(hf_state_dict(ours), strict=True)
    ids, am, labels = _token_batch(cfg)
    with torch.no_grad():
        loss, logits = ours(ids, attention_mask=am, labels=labels)
        out = hf(input_ids=ids, attention_mask=am, labels=labels)
        only_logits = ours(ids, attention_mask=am)
    assert tuple(logits.shape) == (3, 24, 5)
    torch.testing.assert_close(logits, out.logits, atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(loss, out.loss, atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(only_logits, logits)
    stats = loss._hsd_stats
    assert int(stats[2]) == int(labels.ne(-100).sum())
    assert int(stats[1]) == int(((logits.argmax(-1) == labels) & labels.ne(-100)).sum())


def test_head_dropout_rule_follows_hf():
    bert = resolve_config("hsd-tiny-bert").replace(hidden_dropout_prob=0.1, classifier_dropout=None)
    assert build_model(bert, task=TASK).head_dropout() == 0.1
    assert build_model(bert.replace(classifier_dropout=0.3), task=TASK).head_dropout() == 0.3
    distil = resolve_config("hsd-tiny-distilbert").replace(hidden_dropout_prob=0.15, seq_classif_dropout=0.4)
    assert build_model(distil, task=TASK).head_dropout() == 0.15  # config.dropout, not seq_classif_dropout


def test_save_pretrained_loads_in_transformers(tmp_path):
    pytest.importorskip("transformers")
    from transformers import AutoModelForTokenClassification

    cfg = resolve_config("hsd-tiny-bert", num_labels=3)
    cfg.id2label = {"0": "O", "1": "B-PER", "2": "I-PER"}
    ours = build_model(cfg, task=TASK, seed=7).eval()
    save_pretrained(ours, str(tmp_path))
    conf = json.load(open(tmp_path / "config.json"))
    assert conf["architectures"] == ["BertForTokenClassification"]
    assert conf["id2label"] == {"0": "O", "1": "B-PER", "2": "I-PER"} and conf["label2id"]["B-PER"] == 1
    hf = AutoModelForTokenClassification.from_pretrained(str(tmp_path)).eval()
    ids = torch.randint(5, cfg.vocab_size, (2, 12))
    with torch.no_grad():
        torch.testing.assert_close(ours(ids), hf(input_ids=ids).logits, atol=1e-5, rtol=1e-4)
    again = from_pretrained(str(tmp_path), task=TASK).eval()
    with torch.no_grad():
        torch.testing.assert_close(ours(ids), again(ids))


def test_checkpoint_without_classifier_keeps_the_fresh_one(tmp_path, caplog):
    """A checkpoint without ``classifier.*`` (as a pretrained encoder is): the encoder loads, the classifier keeps its
    fresh initialisation, and the log names the newly initialised weights, as transformers does."""
    from safetensors.torch import save_file

    cfg = resolve_config("hsd-tiny-bert", num_labels=4)
    src = build_model(cfg, task=TASK, seed=11)
    sd = {k: v for k, v in hf_state_dict(src).items() if not k.startswith("classifier.")}
    os.makedirs(tmp_path / "ckpt")
    json.dump(cfg.to_hf_dict(), open(tmp_path / "ckpt" / "config.json", "w"))
    save_file(sd, str(tmp_path / "ckpt" / "model.safetensors"))
    fresh = build_model(cfg, task=TASK, seed=5)
    with caplog.at_level("INFO"):
        dst = from_pretrained(str(tmp_path / "ckpt"), task=TASK, num_labels=4, seed=5)
    assert "classifier.weight" in caplog.text and "newly initialized" in caplog.text
    torch.testing.assert_close(dst.classifier_weight, fresh.classifier_weight)
    torch.testing.assert_close(dst.encoder.layers[0].qkv_weight, src.encoder.layers[0].qkv_weight)


def test_build_model_refuses_unknown_tasks():
    with pytest.raises(ValueError):
        build_model(resolve_config("hsd-tiny-bert"), task="question-answering")


# ------------------------------------------------------------------------------------------ packed == padded
LENGTHS = [64, 40, 17, 2]


def _padded(lengths, S, cfg, seed):
    g = np.random.default_rng(seed)
    ids = g.integers(5, cfg.vocab_size, size=(len(lengths), S)).astype(np.int64)
    mask = (np.arange(S)[None, :] < np.asarray(lengths)[:, None]).astype(np.int64)
    ids[mask == 0] = cfg.pad_token_id
    labels = g.integers(0, cfg.num_labels, size=ids.shape).astype(np.int64)
    labels[g.random(ids.shape) < 0.25] = -100
    labels[:, 0] = -100
    labels[mask == 0] = -100
    return ids, mask, labels


def _step(model, **kw):
    model.zero_grad(set_to_none=True)
    model.rng.new_step(0)
    loss, logits = model(**kw)
    loss.backward()
    return loss.detach(), logits.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def _packed_and_padded(name, lengths, **cfg_kw):
    cfg = resolve_config(name, num_labels=5).replace(**cfg_kw)
    model = build_model(cfg, task=TASK, seed=1).train()
    ids, mask, labels = _padded(lengths, 64, cfg, seed=3)
    t = torch.from_numpy
    padded = _step(model, input_ids=t(ids), attention_mask=t(mask), labels=t(labels))
    pk = pack_batch(ids, mask, labels, **position_rule(cfg))
    packed = _step(model, input_ids=t(pk["input_ids"]), labels=t(np.asarray(pk["labels"])),
                   cu_seqlens=t(pk["cu_seqlens"]), max_seqlen=pk["max_seqlen"], position_ids=t(pk["position_ids"]))
    return cfg, pk, mask, padded, packed


def _assert_same_step(pk, mask, padded, packed):
    (l0, lg0, g0), (l1, lg1, g1) = padded, packed
    torch.testing.assert_close(l1, l0, rtol=1e-5, atol=1e-6)
    back = torch.from_numpy(unpack_rows(lg1.numpy(), pk["cu_seqlens"], 64))  # [B, S, L], zeros on the padding
    real = torch.from_numpy(mask != 0)
    torch.testing.assert_close(back[real], lg0[real], rtol=1e-5, atol=1e-6)
    assert set(g0) == set(g1)
    for n in g0:
        torch.testing.assert_close(g1[n], g0[n], rtol=1e-5, atol=1e-6, msg=lambda m, n=n: f"{n}: {m}")


@pytest.mark.parametrize("name", NAMES)
def test_packed_model_step_equals_padded_step_fp32(name):
    """B = 4, S = 64, lengths 64 / 40 / 17 / 2, per-token labels with scattered -100, fp32, as tests/test_packing.py:
    loss, the logits of the real rows and every gradient at rtol 1e-5. Dropout is off here because a ragged packed
    batch numbers its rows differently from the padded one, so the two draw different masks at every site (the
    full-length case below runs the head's dropout)."""
    _, pk, mask, padded, packed = _packed_and_padded(name, LENGTHS, hidden_dropout_prob=0.0,
                                                     attention_probs_dropout_prob=0.0, classifier_dropout=0.0)
    _assert_same_step(pk, mask, padded, packed)


@pytest.mark.parametrize("name", ["hsd-tiny-bert", "hsd-tiny-roberta"])
def test_packed_step_equals_padded_step_with_head_dropout(name):
    """Full-length sequences (T = B·S = 256): packed row t IS padded row b·S + i, so the head's dropout site
    ([rows, H], p = 0.25) draws the same mask in both layouts and the steps agree with dropout on. (The encoder's
    sites are numbered per layout, so its dropout stays off.)"""
    _, pk, mask, padded, packed = _packed_and_padded(name, [64, 64, 64, 64], hidden_dropout_prob=0.0,
                                                     attention_probs_dropout_prob=0.0, classifier_dropout=0.25)
    _assert_same_step(pk, mask, padded, packed)
    # and the dropout did run: the logits differ from the eval-mode logits
    cfg = resolve_config(name, num_labels=5).replace(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                                                     classifier_dropout=0.25)
    model = build_model(cfg, task=TASK, seed=1)
    ids, m, _ = _padded([64] * 4, 64, cfg, seed=3)
    with torch.no_grad():
        ev = model.eval()(torch.from_numpy(ids), attention_mask=torch.from_numpy(m))
    assert not torch.allclose(ev, padded[1], atol=1e-4)


@pytest.mark.parametrize("packed", [False, True])
def test_all_ignored_batch_gives_zero_loss_and_zero_gradients(packed):
    cfg = resolve_config("hsd-tiny-bert", num_labels=5)
    model = build_model(cfg, task=TASK, seed=1).train()
    ids, mask, labels = _padded(LENGTHS, 64, cfg, seed=3)
    labels[:] = -100
    t = torch.from_numpy
    if packed:
        pk = pack_batch(ids, mask, labels, **position_rule(cfg))
        loss, _, grads = _step(model, input_ids=t(pk["input_ids"]), labels=t(np.asarray(pk["labels"])),
                               cu_seqlens=t(pk["cu_seqlens"]), max_seqlen=pk["max_seqlen"],
                               position_ids=t(pk["position_ids"]))
    else:
        loss, _, grads = _step(model, input_ids=t(ids), attention_mask=t(mask), labels=t(labels))
    assert float(loss) == 0.0
    for n, g in grads.items():
        assert torch.isfinite(g).all() and torch.count_nonzero(g) == 0, n


def test_head_dropout_site_is_the_flat_row_buffer():
    """ops.token_head on CPU: mask = rng.keep_mask(seed, (R, H), p), one seed drawn after the encoder's."""
    g = torch.Generator().manual_seed(0)
    h = torch.randn(37, 64, generator=g)
    w, b = torch.randn(5, 64, generator=g) * 0.1, torch.randn(5, generator=g) * 0.1
    labels = torch.randint(0, 5, (37,), generator=g)
    labels[::4] = -100
    loss, logits = ops.token_head(h, w, b, labels, 0.1, 99)
    keep = rng.keep_mask(99, (37, 64), 0.1).float() / 0.9
    want = torch.nn.functional.linear(h * keep, w, b)
    torch.testing.assert_close(logits, want)
    torch.testing.assert_close(loss, torch.nn.functional.cross_entropy(want, labels, ignore_index=-100))
    loss2, logits2, stats = ref.token_head(h, w, b, labels, 0.1, 99)
    torch.testing.assert_close(loss2, loss)
    assert float(stats[2]) == float(labels.ne(-100).sum())


# ------------------------------------------------------------------------------------------ synthetic corpus
def test_synthetic_corpus_is_deterministic_and_shares_its_table():
    a = hdata.synthetic_token_classification(64, 32, 1024, seed=5, num_labels=7)
    b = hdata.synthetic_token_classification(64, 32, 1024, seed=5, num_labels=7)
    c = hdata.synthetic_token_classification(64, 32, 1024, seed=6, num_labels=7)
    assert np.array_equal(a.input_ids, b.input_ids) and np.array_equal(a.labels, b.labels)
    assert not np.array_equal(a.input_ids, c.input_ids)
    table = hdata.tag_table(1024, 7)
    assert np.array_equal(table, hdata.tag_table(1024, 7)) and table.min() >= 0 and table.max() < 7
    for ds in (a, c):  # two seeds, one language
        ids = ds.input_ids.astype(np.int64)
        want = (table[ids[:, 1:]] + table[ids[:, :-1]]) % 7
        lab = ds.labels[:, 1:]
        assert np.array_equal(lab[lab != -100], want[lab != -100])


def test_synthetic_corpus_ignores_exactly_what_is_specified():
    S = 32
    ds = hdata.synthetic_token_classification(512, S, 1024, seed=1, num_labels=9)
    lengths = ds.attention_mask.sum(axis=1)
    assert lengths.min() >= S // 4 and lengths.max() == S and len(set(lengths.tolist())) > 4  # ragged in [S/4, S]
    rows = np.arange(len(ds))
    assert (ds.input_ids[:, 0] == 101).all() and (ds.input_ids[rows, lengths - 1] == 102).all()
    assert (ds.labels[:, 0] == -100).all() and (ds.labels[rows, lengths - 1] == -100).all()
    assert (ds.labels[ds.attention_mask == 0] == -100).all() and (ds.input_ids[ds.attention_mask == 0] == 0).all()
    pos = np.arange(S)[None, :]
    real = (pos >= 1) & (pos < lengths[:, None] - 1)
    frac = float((ds.labels[real] == -100).mean())
    assert 0.22 < frac < 0.28  # a seeded ~25 % of the real tokens (about 8,700 draws: 3 sigma is 0.014)
    # scattered, not only at the tail: some ignored real token is followed by a labelled one
    ign = (ds.labels == -100) & real
    assert (ign[:, :-1] & (ds.labels[:, 1:] != -100)).any()
    assert ds.labels.max() < 9 and ds.labels[ds.labels != -100].min() >= 0


def test_tiny_model_learns_the_synthetic_tags_on_cpu():
    """2-layer hsd-tiny-bert (H = 64), vocabulary cut to 64 tokens, L = 4 tags, S = 32, batch 32, Adam lr 5e-3, fp32,
    200 steps on CPU (about 5 s). Chance is 1 / L = 0.25. Measured held-out token accuracy after the 200 steps: 0.911
    (loss 0.18); lr 1e-2 gave 0.737, and 120 steps at lr 3e-3 0.459. The test asserts > 0.60: a model that ignores the
    left neighbour cannot get there (the tag is uniform given the token alone)."""
    torch.manual_seed(0)
    L, V, S = 4, 64, 32
    cfg = resolve_config("hsd-tiny-bert", num_labels=L).replace(vocab_size=V, max_position_embeddings=S)
    model = build_model(cfg, task=TASK, seed=0).train()
    kw = dict(num_labels=L, cls_id=1, sep_id=2)
    tr = hdata.synthetic_token_classification(32 * 200, S, V, seed=0, **kw)
    te = hdata.synthetic_token_classification(256, S, V, seed=1, **kw)
    opt = torch.optim.Adam(model.parameters(), lr=5e-3)
    t = lambda a: torch.from_numpy(np.asarray(a).astype(np.int64))  # noqa: E731
    for step in range(200):
        sl = slice(32 * step, 32 * (step + 1))
        model.rng.new_step(step)
        loss, _ = model(t(tr.input_ids[sl]), attention_mask=t(tr.attention_mask[sl]), labels=t(tr.labels[sl]))
        opt.zero_grad()
        loss.backward()
        opt.step()
    model.eval()
    with torch.no_grad():
        loss, logits = model(t(te.input_ids), attention_mask=t(te.attention_mask), labels=t(te.labels))
    lab = t(te.labels)
    acc = float(((logits.argmax(-1) == lab) & lab.ne(-100)).sum()) / float(lab.ne(-100).sum())
    print(f"held-out token accuracy {acc:.3f}, loss {float(loss):.3f}")
    assert acc > 0.60


# ------------------------------------------------------------------------------------------ CoNLL
CONLL = """-DOCSTART- -X- O O

the DT B-NP O
wonderful JJ I-NP B-MISC
movie NN I-NP O

-DOCSTART- -X- O O
bad JJ B-ADJP O
plot NN B-NP B-PER
"""


def test_read_conll_sentences_docstart_and_columns(tmp_path):
    p = tmp_path / "train.txt"
    p.write_text(CONLL)
    words, tags = hdata.read_conll(str(p))
    assert words == [["the", "wonderful", "movie"], ["bad", "plot"]]
    assert tags == [["O", "B-MISC", "O"], ["O", "B-PER"]]  # first column the word, last column the tag


def test_conll_tag_list_from_labels_txt_and_from_the_data(tmp_path):
    (tmp_path / "train.txt").write_text(CONLL)
    assert hdata.conll_tag_list(str(tmp_path)) == ["B-MISC", "B-PER", "O"]  # sorted tags of the train split
    (tmp_path / "labels.txt").write_text("O\nB-PER\nI-PER\nB-MISC\n")
    assert hdata.conll_tag_list(str(tmp_path)) == ["O", "B-PER", "I-PER", "B-MISC"]


def test_conll_word_alignment_and_truncation():
    pytest.importorskip("tokenizers")
    tok = hdata.load_tokenizer(None, 1024)
    # the generated WordPiece vocabulary has "the", "movie", "bad" whole and single characters + "##" continuations,
    # so "zzq" is three pieces (z ##z ##q)
    words = [["the", "zzq", "movie"], ["bad", "zzq"]]
    tags = [["O", "B-PER", "O"], ["O", "B-PER"]]
    tag_list = ["O", "B-PER"]
    enc = tok.encode_words(words, 8)
    assert enc["word_ids"][0].tolist() == [-1, 0, 1, 1, 1, 2, -1, -1]  # [CLS] the z ##z ##q movie [SEP] [PAD]
    ds = hdata.tokenize_conll(tok, words, tags, tag_list, 8)
    assert ds.labels.shape == (2, 8) and ds.input_ids.shape == (2, 8)
    assert ds.labels[0].tolist() == [-100, 0, 1, -100, -100, 0, -100, -100]  # first piece carries the tag
    assert ds.attention_mask[0].tolist() == [1, 1, 1, 1, 1, 1, 1, 0]
    assert ds.labels[1].tolist() == [-100, 0, 1, -100, -100, -100, -100, -100]
    # truncation in the middle of a word: [CLS] the z ##z [SEP] -- the cut word keeps its first piece's tag, the
    # words beyond the cut are gone
    cut = hdata.tokenize_conll(tok, words, tags, tag_list, 5)
    assert cut.labels[0].tolist() == [-100, 0, 1, -100, -100]
    assert cut.attention_mask[0].tolist() == [1, 1, 1, 1, 1] and cut.input_ids[0, -1] == 102


# ------------------------------------------------------------------------------------------ CLI
def _cli(tmp, extra):
    env = dict(os.environ, SM_OUTPUT_DATA_DIR=str(tmp / "data"), SM_MODEL_DIR=str(tmp / "model"), SM_NUM_GPUS="0",
               SM_FRAMEWORK_PARAMS="{}")
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "train.py"), "--epochs", "1", "--train_batch_size", "8",
           "--eval_batch_size", "8", "--model_name_or_path", "hsd-tiny-bert", "--max_seq_length", "32",
           "--num_train_examples", "32", "--num_eval_examples", "16", "--device", "cpu", "--log_every", "0",
           "--task", TASK] + extra
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)


def _results(path):
    return dict(line.split(" = ") for line in path.read_text().splitlines())


def test_cli_trains_on_the_synthetic_corpus(tmp_path):
    r = _cli(tmp_path, ["--dataset", "synthetic", "--max_steps", "2", "--num_labels", "5"])
    assert r.returncode == 0, r.stderr[-3000:]
    prov = json.load(open(tmp_path / "data" / "run_provenance.json"))
    assert prov["task"] == TASK and prov["num_labels"] == 5 and prov["synthetic_data"] is True
    tr, ev = _results(tmp_path / "data" / "train_results.txt"), _results(tmp_path / "data" / "eval_results.txt")
    assert np.isfinite(json.loads(tr["loss"])).all() and 0.0 <= float(ev["sparse_categorical_accuracy"]) <= 1.0
    conf = json.load(open(tmp_path / "model" / "config.json"))
    assert conf["architectures"] == ["BertForTokenClassification"] and len(conf["id2label"]) == 5
    assert os.path.isfile(tmp_path / "model" / "model.safetensors")


def test_cli_reads_conll_and_follows_its_tag_list(tmp_path):
    pytest.importorskip("tokenizers")
    d = tmp_path / "conll"
    d.mkdir()
    (d / "train.txt").write_text(CONLL * 8)
    (d / "validation.txt").write_text(CONLL * 4)
    r = _cli(tmp_path, ["--dataset", "conll", "--dataset_dir", str(d), "--pack_sequences", "true"])
    assert r.returncode == 0, r.stderr[-3000:]
    conf = json.load(open(tmp_path / "model" / "config.json"))
    assert conf["id2label"] == {"0": "B-MISC", "1": "B-PER", "2": "O"}  # --num_labels follows the tag list
    assert json.load(open(tmp_path / "data" / "run_provenance.json"))["num_labels"] == 3


@pytest.mark.parametrize("dataset", ["imdb", "sst2"])
def test_cli_refuses_text_classification_datasets(tmp_path, dataset):
    r = _cli(tmp_path, ["--dataset", dataset])
    assert r.returncode != 0 and "per-token labels" in r.stderr
