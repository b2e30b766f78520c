"""--task sentence-embedding on the CPU: the reference ops (ops/reference.py pool_normalize / contrastive_loss) against a
plain fp64 rewrite, the model padded against packed, against transformers' AutoModel, its checkpoint, and learning."""
import numpy as np
import pytest
import torch

from huggingface_sagemaker_tensorflow_distributed_amd import ops
from huggingface_sagemaker_tensorflow_distributed_amd.data.datasets import synthetic_pairs
from huggingface_sagemaker_tensorflow_distributed_amd.data.packing import pack_batch, position_rule
from huggingface_sagemaker_tensorflow_distributed_amd.models import (build_model, from_pretrained, resolve_config,
                                                                     save_pretrained)
from huggingface_sagemaker_tensorflow_distributed_amd.ops import reference as ref


def _plain_fp64(h, cu, mask, valid, scale):
    """The definition, sequence by sequence and pair by pair, in fp64 autograd."""
    es = []
    for s in range(cu.numel() - 1):
        rows = h[int(cu[s]):int(cu[s + 1])]
        w = torch.ones(rows.shape[0], dtype=h.dtype) if mask is None else mask[int(cu[s]):int(cu[s + 1])].ne(0).to(h.dtype)
        m = (rows * w[:, None]).sum(0) / max(float(w.sum()), 1.0)
        es.append(m / m.norm().clamp(min=1e-12) if float(w.sum()) > 0 else m * 0.0)
    e = torch.stack(es)
    idx = [i for i in range(valid.numel()) if int(valid[i]) != 0]
    terms = [torch.logsumexp(torch.stack([scale * e[2 * i] @ e[2 * j + 1] for j in idx]), 0) - scale * e[2 * i] @ e[2 * i + 1]
             for i in idx]
    return e, (torch.stack(terms).sum() / len(idx) if idx else e.sum() * 0.0)


@pytest.mark.parametrize("valid", [[1, 1, 0, 1], [1], [0, 0]])
def test_reference_ops_vs_plain_fp64(valid):
    """An empty sequence, a mask with a hole, an invalid pair, B = 1 (loss exactly 0) and no valid pair (loss 0)."""
    B, S, H = len(valid), 6, 16
    g = torch.Generator().manual_seed(B)
    h = torch.randn(2 * B * S + 3, H, generator=g, dtype=torch.float64)
    cu = torch.arange(2 * B + 1, dtype=torch.int32) * S
    mask = torch.ones(2 * B * S + 3, dtype=torch.long)
    mask[1] = 0            # a hole in sequence 0
    mask[S:2 * S] = 0      # sequence 1 has no live row
    valid = torch.tensor(valid, dtype=torch.int32)
    x1, x2 = h.clone().requires_grad_(), h.clone().requires_grad_()
    e_want, l_want = _plain_fp64(x1, cu, mask, valid, 20.0)
    loss, e, stats = ref.sentence_head(x2, cu, mask, valid, 20.0)
    l_want.backward()
    loss.backward()
    torch.testing.assert_close(e, e_want, rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(loss, l_want, rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(x2.grad, x1.grad, rtol=1e-10, atol=1e-14)
    assert torch.count_nonzero(e[1]) == 0 and torch.count_nonzero(x2.grad[mask == 0]) == 0
    assert stats[2].item() == float(valid.sum()) and stats[1].item() <= stats[2].item()
    if valid.sum() <= 1:
        assert loss.item() == 0.0


def _pair_batch(cfg, B, S, seed=0):
    ds = synthetic_pairs(B, S, cfg.vocab_size, seed=seed, pad_id=cfg.pad_token_id)
    labels = ds.labels.copy()
    labels[1] = -100
    return ds.input_ids.astype(np.int64), ds.attention_mask.astype(np.int64), labels


@pytest.mark.parametrize("name", ["hsd-tiny-bert", "hsd-tiny-mpnet"])
def test_packed_step_equals_padded_step(name):
    cfg = resolve_config(name).replace(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model = build_model(cfg, task="sentence-embedding", seed=0)
    B, S = 4, 16
    ids, mask, labels = _pair_batch(cfg, B, S)
    pk = pack_batch(ids.reshape(2 * B, S), mask.reshape(2 * B, S), np.zeros(2 * B, dtype=np.int64), **position_rule(cfg))
    t = torch.from_numpy
    kws = [dict(input_ids=t(ids), attention_mask=t(mask), labels=t(labels)),
           dict(input_ids=t(pk["input_ids"]), labels=t(labels), cu_seqlens=t(pk["cu_seqlens"]),
                max_seqlen=pk["max_seqlen"], position_ids=t(pk["position_ids"]))]
    out = []
    for kw in kws:
        model.zero_grad(set_to_none=True)
        loss, e = model(**kw)
        loss.backward()
        out.append((loss.detach(), e.detach(), loss._hsd_stats, [p.grad.clone() for p in model.parameters()]))
    torch.testing.assert_close(out[1][0], out[0][0], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(out[1][1], out[0][1], rtol=1e-5, atol=1e-6)
    assert out[0][2][2].item() == B - 1 and torch.equal(out[0][2][1:3], out[1][2][1:3])
    for a, b in zip(out[1][3], out[0][3]):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", ["hsd-tiny-bert", "hsd-tiny-mpnet", "hsd-tiny-roberta", "hsd-tiny-distilbert"])
def test_encode_equals_automodel_and_the_saved_directory_loads(name, tmp_path):
    transformers = pytest.importorskip("transformers")
    cfg = resolve_config(name)
    model = build_model(cfg, task="sentence-embedding", seed=1).eval()
    save_pretrained(model, str(tmp_path))
    hf = transformers.AutoModel.from_pretrained(str(tmp_path)).eval()
    assert type(hf).__name__ == model.architecture() and model.architecture().endswith("Model")
    ids, mask, _ = _pair_batch(cfg, 3, 12)
    ids, mask = torch.from_numpy(ids.reshape(6, 12)), torch.from_numpy(mask.reshape(6, 12))
    with torch.no_grad():
        hs = hf(input_ids=ids, attention_mask=mask).last_hidden_state
        m = (hs * mask[..., None]).sum(1) / mask.sum(1, keepdim=True)
        want = torch.nn.functional.normalize(m, dim=1)
        got = model.encode(ids, mask)
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-5)
    again = from_pretrained(str(tmp_path), task="sentence-embedding").eval()
    with torch.no_grad():
        assert torch.equal(again.encode(ids, mask), got)


def test_refusals():
    from huggingface_sagemaker_tensorflow_distributed_amd.train import runner
    from huggingface_sagemaker_tensorflow_distributed_amd.utils.args import parse_args

    base = ["--task", "sentence-embedding", "--model_name_or_path", "hsd-tiny-bert", "--device", "cpu"]
    for extra in (["--contrastive_scale", "0"], ["--contrastive_scale", "inf"], ["--contrastive_scale", "nan"],
                  ["--label_smoothing_factor", "0.1"], ["--problem_type", "regression"], ["--mlm_masking", "dynamic"],
                  ["--dataset", "imdb"], ["--dataset", "squad"], ["--dataset", "conll"], ["--dataset", "synthetic-bigram"]):
        args, _ = parse_args(base + extra, "train")
        with pytest.raises(ValueError):
            runner.check_sentence_embedding(args)
    args, _ = parse_args(base, "train")
    runner.check_sentence_embedding(args)
    with pytest.raises(ValueError):
        build_model(resolve_config("hsd-tiny-bert"), task="sentence-embedding", problem_type="regression")


@pytest.mark.parametrize("ext,cols", [(".tsv", ("anchor", "positive")), (".jsonl", ("sentence1", "sentence2"))])
def test_pair_files_reach_the_runner_as_side_by_side_columns(tmp_path, ext, cols):
    """--dataset pairs through the runner's dataset builder: [N, 2 S], each side tokenised on its own."""
    import json
    from huggingface_sagemaker_tensorflow_distributed_amd import data as hdata
    from huggingface_sagemaker_tensorflow_distributed_amd.train import runner
    from huggingface_sagemaker_tensorflow_distributed_amd.utils.args import parse_args

    pairs = [("a cat sat", "the cat was sitting down"), ("rain fell", "it rained"), ("good film", "a fine movie")]
    text = ("\t".join(cols) + "\n" + "".join(f"{a}\t{p}\n" for a, p in pairs) if ext == ".tsv" else
            "".join(json.dumps(dict(zip(cols, ap))) + "\n" for ap in pairs))
    for split in ("train", "test"):
        (tmp_path / (split + ext)).write_text(text)
    assert hdata.read_pairs(str(tmp_path / ("train" + ext))) == ([a for a, _ in pairs], [p for _, p in pairs])
    args, _ = parse_args(["--task", "sentence-embedding", "--model_name_or_path", "hsd-tiny-bert", "--device", "cpu",
                          "--dataset", "pairs", "--dataset_dir", str(tmp_path), "--num_train_examples", "2"], "train")
    cfg, S = resolve_config("hsd-tiny-bert"), 8
    tok = hdata.load_tokenizer(None, cfg.vocab_size)  # the offline tokenizer of the tiny configs
    tr, te = runner._datasets(args, cfg, tok, S)
    assert tr.pairs and te.pairs and tr.input_ids.shape == (2, 2 * S) and te.input_ids.shape == (3, 2 * S)
    for i, (a, p) in enumerate(pairs):
        for side, text in enumerate((a, p)):
            want = tok.encode_batch([text], S)
            assert np.array_equal(te.input_ids[i, side * S:(side + 1) * S], want["input_ids"][0])
            assert np.array_equal(te.attention_mask[i, side * S:(side + 1) * S], want["attention_mask"][0])


def test_retrieval_accuracy_rises_on_synthetic_pairs():
    """A 2-layer H = 64 BERT, B = 16 pairs (chance 1/16), 200 Adam steps on the CPU: accuracy on held-out pairs > 0.5."""
    cfg = resolve_config("hsd-tiny-bert").replace(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model = build_model(cfg, task="sentence-embedding", seed=0)
    B, S = 16, 16
    tr = synthetic_pairs(B * 200, S, cfg.vocab_size, seed=0, pad_id=cfg.pad_token_id)
    te = synthetic_pairs(B * 4, S, cfg.vocab_size, seed=1, pad_id=cfg.pad_token_id)

    def step(ds, i):
        sl = slice(i * B, (i + 1) * B)
        return model(torch.from_numpy(ds.input_ids[sl].astype(np.int64)),
                     torch.from_numpy(ds.attention_mask[sl].astype(np.int64)), labels=torch.from_numpy(ds.labels[sl]))[0]

    def accuracy():
        with torch.no_grad():
            st = sum(step(te, i)._hsd_stats for i in range(4))
        return (st[1] / st[2]).item()

    before = accuracy()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    for i in range(200):
        opt.zero_grad()
        step(tr, i).backward()
        opt.step()
    after = accuracy()
    print(f"retrieval accuracy {before:.3f} -> {after:.3f} (chance {1 / B:.3f})")
    assert after > 0.5 and after > before
