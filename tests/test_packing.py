"""--pack_sequences on the host and on the reference ops (CPU): the packed layout (data/packing.py), the packed
attention reference and its dropout site definition, a packed model step against the padded one in fp32, and the CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from huggingface_sagemaker_tensorflow_distributed_amd.data.packing import pack_batch, position_rule, unpack_rows
from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model, resolve_config
from huggingface_sagemaker_tensorflow_distributed_amd.ops import reference as ref
from huggingface_sagemaker_tensorflow_distributed_amd.ops import rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (64, 40, 17, 2)


def _padded(lengths, S, vocab, pad_id, seed=0, lo=5):
    g = np.random.default_rng(seed)
    B = len(lengths)
    ids = g.integers(lo, vocab, size=(B, S), dtype=np.int64)
    mask = (np.arange(S)[None, :] < np.asarray(lengths)[:, None]).astype(np.int64)
    ids[mask == 0] = pad_id
    return ids, mask


# ------------------------------------------------------------------------------------------ pack_batch
def test_pack_batch_offsets_rows_and_dead_rows():
    lengths = [5, 1, 300, 64]
    ids, mask = _padded(lengths, 320, 1000, pad_id=3)
    labels = np.array([1, 0, 1, 1])
    pk = pack_batch(ids, mask, labels, pad_id=3, pos_base=0, pad_pos=0)
    cu = pk["cu_seqlens"]
    assert cu.dtype == np.int32 and cu.tolist() == [0, 5, 6, 306, 370]
    assert pk["real_tokens"] == 370 and pk["max_seqlen"] == 300
    assert isinstance(pk["real_tokens"], int) and isinstance(pk["max_seqlen"], int)
    T = pk["input_ids"].shape[1]
    assert T == 512 and T % 256 == 0 and pk["input_ids"].shape == (1, T) and pk["position_ids"].shape == (1, T)
    for b, L in enumerate(lengths):
        assert np.array_equal(pk["input_ids"][0, cu[b]:cu[b + 1]], ids[b, :L])
        assert np.array_equal(pk["position_ids"][0, cu[b]:cu[b + 1]], np.arange(L))
    assert (pk["input_ids"][0, 370:] == 3).all() and (pk["position_ids"][0, 370:] == 0).all()
    assert pk["labels"] is labels or np.array_equal(pk["labels"], labels)  # classification: unchanged [B]
    # a batch that fills its rows exactly has no dead rows; row_multiple is honoured
    pk2 = pack_batch(ids[:, :64], np.ones((4, 64), dtype=np.int64), labels, pad_id=3, pos_base=0, pad_pos=0)
    assert pk2["input_ids"].shape == (1, 256) and pk2["real_tokens"] == 256
    assert pack_batch(ids, mask, labels, pad_id=3, pos_base=0, pad_pos=0, row_multiple=64)["input_ids"].shape == (1, 384)


def test_pack_batch_mlm_labels_are_packed_with_ignored_dead_rows():
    lengths = [7, 30]
    ids, mask = _padded(lengths, 32, 100, pad_id=1)
    labels = np.where(np.random.default_rng(1).random((2, 32)) < 0.3, ids, -100)
    pk = pack_batch(ids, mask, labels, pad_id=1, pos_base=2, pad_pos=1)
    assert pk["labels"].shape == (256,)
    assert np.array_equal(pk["labels"][:7], labels[0, :7]) and np.array_equal(pk["labels"][7:37], labels[1, :30])
    assert (pk["labels"][37:] == -100).all()
    assert (pk["input_ids"][0, 37:] == 1).all() and (pk["position_ids"][0, 37:] == 1).all()


@pytest.mark.parametrize("name", ["hsd-tiny-bert", "hsd-tiny-roberta", "hsd-tiny-distilbert"])
def test_pack_batch_position_ids_match_the_embeddings_rule(name):
    cfg = resolve_config(name)
    m = build_model(cfg, seed=0)
    ids, mask = _padded(LENGTHS, 64, cfg.vocab_size, cfg.pad_token_id)
    want = m.encoder.embeddings.position_ids(torch.from_numpy(ids)).numpy()
    pk = pack_batch(ids, mask, np.zeros(4, dtype=np.int64), **position_rule(cfg))
    got = unpack_rows(pk["position_ids"][0], pk["cu_seqlens"], 64)
    valid = mask.astype(bool)
    assert np.array_equal(got[valid], want[valid])
    rule = position_rule(cfg)
    assert (pk["position_ids"][0, pk["real_tokens"]:] == rule["pad_pos"]).all()
    assert (pk["input_ids"][0, pk["real_tokens"]:] == cfg.pad_token_id).all()


def test_pack_batch_refuses_holes_and_empty_sequences():
    ids, mask = _padded([8, 8, 8], 8, 50, pad_id=0)
    hole = mask.copy()
    hole[1, 3] = 0
    with pytest.raises(ValueError, match="row 1"):
        pack_batch(ids, hole, np.zeros(3), pad_id=0, pos_base=0, pad_pos=0)
    left = mask.copy()
    left[2, 0] = 0
    with pytest.raises(ValueError, match="row 2"):
        pack_batch(ids, left, np.zeros(3), pad_id=0, pos_base=0, pad_pos=0)
    empty = mask.copy()
    empty[0] = 0
    with pytest.raises(ValueError, match="row 0"):
        pack_batch(ids, empty, np.zeros(3), pad_id=0, pos_base=0, pad_pos=0)


def test_unpack_rows_round_trip():
    ids, mask = _padded(LENGTHS, 64, 500, pad_id=0)
    pk = pack_batch(ids, mask, np.zeros(4), pad_id=0, pos_base=0, pad_pos=0)
    assert np.array_equal(unpack_rows(pk["input_ids"][0], pk["cu_seqlens"], 64), ids * mask)
    x = np.random.default_rng(0).standard_normal((pk["input_ids"].shape[1], 3, 2)).astype(np.float32)
    u = unpack_rows(x, pk["cu_seqlens"], 64)
    assert u.shape == (4, 64, 3, 2) and np.array_equal(u[1, :40], x[64:104]) and not u[1, 40:].any()


def test_batch_loader_packs_in_the_prefetch_thread():
    from huggingface_sagemaker_tensorflow_distributed_amd import data as hdata
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import ShardSampler

    ds = hdata.synthetic_classification(16, 64, 1000, seed=0)
    cfg = resolve_config("hsd-tiny-bert")
    plain = list(hdata.BatchLoader(ds, ShardSampler(16, 0, 1, shuffle=False, batch_size=8), torch.device("cpu")))
    packed = list(hdata.BatchLoader(ds, ShardSampler(16, 0, 1, shuffle=False, batch_size=8), torch.device("cpu"),
                                    pack=True, pack_rule=position_rule(cfg)))
    assert len(packed) == len(plain) == 2
    for a, b in zip(plain, packed):
        assert "attention_mask" not in b and b["cu_seqlens"].dtype == torch.int32
        assert isinstance(b["real_tokens"], int) and isinstance(b["max_seqlen"], int)
        assert b["real_tokens"] == int(a["attention_mask"].sum()) and torch.equal(a["labels"], b["labels"])
        assert torch.equal(b["input_ids"][0, :b["real_tokens"]], a["input_ids"][a["attention_mask"] != 0])


# ------------------------------------------------------------------------------------------ reference attention
HEADS = 3


def _qkv(T, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(T, 3 * HEADS * 64, generator=g)


def test_reference_varlen_equals_reference_attention_per_sequence():
    lengths = [1, 7, 33, 64, 65]
    cu = torch.tensor([0] + list(np.cumsum(lengths)), dtype=torch.int32)
    T = 256
    qkv = _qkv(T)
    out = ref.attention_varlen(qkv, cu, max(lengths), HEADS, 0.0, 0, False)
    assert out.shape == (T, HEADS * 64)
    for b, L in enumerate(lengths):
        s0 = int(cu[b])
        want = ref.attention(qkv[s0:s0 + L], None, 1, L, HEADS, 0.0, 0, False)
        assert torch.equal(out[s0:s0 + L], want), b
    assert int(cu[-1]) < T and torch.count_nonzero(out[int(cu[-1]):]) == 0


def test_reference_varlen_dropout_site_is_row_h_T_plus_t():
    """The mask is rebuilt here from rng.pair_bits for rows h*T + t and key pairs j // 2, independently of
    keep_mask's [rows, W] view: pins the site definition documented in ops/rng.py."""
    lengths = [5, 33, 18]
    cu = [0, 5, 38, 56]
    T, p, seed = 64, 0.1, 0x1234_5678_9ABC
    qkv = _qkv(T, seed=1)
    out = ref.attention_varlen(qkv, torch.tensor(cu, dtype=torch.int32), 33, HEADS, p, seed, True)
    key = rng.site_key(seed & rng.M32, (seed >> 32) & rng.M32)
    thr = rng.threshold(p)
    d = 64
    dropped = 0
    for b, L in enumerate(lengths):
        s0 = cu[b]
        x = qkv[s0:s0 + L].view(L, 3, HEADS, d).permute(1, 2, 0, 3)  # [3,h,L,d]
        pr = torch.softmax(torch.matmul(x[0], x[1].transpose(-1, -2)) / 8.0, dim=-1)
        rows = (torch.arange(HEADS).view(HEADS, 1, 1) * T + s0 + torch.arange(L).view(1, L, 1)).long()
        j = torch.arange(L).view(1, 1, L).long()
        bits = rng.pair_bits(key, rows, j // 2)
        half = torch.where(j % 2 == 0, bits & 0xFFFF, bits >> 16)
        keep = half >= thr
        dropped += int((~keep).sum())
        want = torch.matmul(pr * keep * (1.0 / (1.0 - p)), x[2]).permute(1, 0, 2).reshape(L, HEADS * d)
        torch.testing.assert_close(out[s0:s0 + L], want, rtol=1e-5, atol=1e-6)
    assert dropped > 0
    assert torch.count_nonzero(out[56:]) == 0


# ------------------------------------------------------------------------------------------ model step
def _model_inputs(cfg, mlm):
    ids, mask = _padded(LENGTHS, 64, cfg.vocab_size, cfg.pad_token_id, seed=3)
    if mlm:
        g = np.random.default_rng(4)
        labels = np.where((g.random(ids.shape) < 0.3) & (mask != 0), ids, -100)
        labels[:, 1] = ids[:, 1]  # every sequence scores at least one token
        labels[mask == 0] = -100
    else:
        labels = np.array([1, 0, 0, 1])
    return ids, mask, labels


def _step(model, **kw):
    model.zero_grad(set_to_none=True)
    model.rng.new_step(0)
    loss, _ = model(**kw)
    loss.backward()
    return loss.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def _packed_and_padded_steps(name, task):
    cfg = resolve_config(name).replace(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    if hasattr(cfg, "seq_classif_dropout"):
        cfg = cfg.replace(seq_classif_dropout=0.0)
    if getattr(cfg, "classifier_dropout", None):
        cfg = cfg.replace(classifier_dropout=0.0)
    model = build_model(cfg, task=task, seed=1).train()
    ids, mask, labels = _model_inputs(cfg, task == "masked-lm")
    t = torch.from_numpy
    padded = _step(model, input_ids=t(ids), attention_mask=t(mask), labels=t(labels))
    pk = pack_batch(ids, mask, labels, **position_rule(cfg))
    packed = _step(model, input_ids=t(pk["input_ids"]), labels=t(np.asarray(pk["labels"])),
                   cu_seqlens=t(pk["cu_seqlens"]), max_seqlen=pk["max_seqlen"], position_ids=t(pk["position_ids"]))
    return cfg, model, padded, packed


@pytest.mark.parametrize("name,task", [("hsd-tiny-bert", "sequence-classification"),
                                       ("hsd-tiny-roberta", "sequence-classification"),
                                       ("hsd-tiny-distilbert", "sequence-classification"),
                                       ("hsd-tiny-roberta", "masked-lm")])
def test_packed_model_step_equals_padded_step_fp32(name, task):
    """Dropout off, B = 4, S = 64, lengths 64 / 40 / 17 / 2: the packed step's loss and every parameter gradient equal
    the padded step's at the bound of tests/test_training.py (only the summation order differs)."""
    _, _, (l0, g0), (l1, g1) = _packed_and_padded_steps(name, task)
    torch.testing.assert_close(l1, l0, rtol=1e-5, atol=1e-6)
    assert set(g0) == set(g1)
    for n in g0:
        torch.testing.assert_close(g1[n], g0[n], rtol=1e-5, atol=1e-6, msg=lambda m, n=n: f"{n}: {m}")


def test_packed_step_leaves_the_padding_embedding_row_without_gradient():
    cfg, _, _, (_, g1) = _packed_and_padded_steps("hsd-tiny-bert", "sequence-classification")
    gw = g1["encoder.embeddings.word_embeddings"]
    assert torch.count_nonzero(gw[cfg.pad_token_id]) == 0
    assert torch.count_nonzero(gw) > 0


def test_packed_model_refuses_an_attention_mask():
    cfg = resolve_config("hsd-tiny-bert")
    model = build_model(cfg, seed=1)
    ids, mask, labels = _model_inputs(cfg, False)
    pk = pack_batch(ids, mask, labels, **position_rule(cfg))
    t = torch.from_numpy
    with pytest.raises(ValueError, match="attention_mask"):
        model(t(pk["input_ids"]), attention_mask=torch.ones(1, 256, dtype=torch.long), labels=t(labels),
              cu_seqlens=t(pk["cu_seqlens"]), max_seqlen=64, position_ids=t(pk["position_ids"]))


# ------------------------------------------------------------------------------------------ CLI
def _cli(tmp, model, extra):
    env = dict(os.environ, SM_OUTPUT_DATA_DIR=str(tmp / "data"), SM_MODEL_DIR=str(tmp / "model"), SM_NUM_GPUS="0",
               SM_FRAMEWORK_PARAMS="{}")
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "train.py"), "--epochs", "1", "--train_batch_size", "8",
           "--eval_batch_size", "8", "--model_name_or_path", model, "--max_seq_length", "64",
           "--num_train_examples", "32", "--num_eval_examples", "16", "--device", "cpu", "--log_every", "0"] + extra
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)


def _results(path):
    return dict(line.split(" = ") for line in path.read_text().splitlines())


def test_cli_pack_sequences_on_cpu_matches_the_padded_run(tmp_path):
    """scripts/train.py --pack_sequences true trains, evaluates and writes the reference's result files, and its
    metrics equal the padded run's at the model-step bound above. The tiny model is given without dropout (a
    config.json directory): with dropout the two runs draw different masks, the sites having different shapes."""
    import json

    cfg = resolve_config("hsd-tiny-bert").replace(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    mdir = tmp_path / "tiny"
    mdir.mkdir()
    (mdir / "config.json").write_text(json.dumps(cfg.to_hf_dict()))
    out = {}
    for flag in ("true", "false"):
        d = tmp_path / flag
        r = _cli(d, str(mdir), ["--pack_sequences", flag])
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        train = (d / "data" / "train_results.txt").read_text()
        assert train.startswith("loss = [") and "sparse_categorical_accuracy = [" in train and "train_runtime" in train
        ev = _results(d / "data" / "eval_results.txt")
        out[flag] = (float(ev["loss"]), float(ev["sparse_categorical_accuracy"]),
                     float(train.splitlines()[0].split("[")[1].split("]")[0]))
        assert json.loads((d / "data" / "run_provenance.json").read_text())["pack_sequences"] is (flag == "true")
        if flag == "true":
            assert "--pack_sequences: first batch holds" in r.stdout + r.stderr
    (el1, ea1, tl1), (el0, ea0, tl0) = out["true"], out["false"]
    print(f"eval loss packed {el1!r} padded {el0!r}; train loss packed {tl1!r} padded {tl0!r}")
    torch.testing.assert_close(torch.tensor(el1), torch.tensor(el0), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(torch.tensor(tl1), torch.tensor(tl0), rtol=1e-5, atol=1e-6)
    assert ea1 == ea0


def test_pack_sequences_refuses_fp8(fake_sm_env):
    from huggingface_sagemaker_tensorflow_distributed_amd.train.runner import build
    from huggingface_sagemaker_tensorflow_distributed_amd.utils.args import build_parser

    args, _ = build_parser("train").parse_known_args(
        ["--model_name_or_path", "hsd-tiny-bert", "--device", "cpu", "--pack_sequences", "true", "--dtype", "fp8"])
    with pytest.raises(ValueError, match="bf16"):
        build(args, "train")
    assert build_parser("train").parse_known_args([])[0].pack_sequences is False
