"""The last encoder layer of a sequence-classification model on its first-token rows only (ops.attn_block_cls):
CPU tier, fp32, reference ops. The pruned path computes the same function with the same dropout bits as the full
last layer, so loss, logits and every parameter gradient agree at the bound tests/test_packing.py uses for the same
kind of claim (only the summation order differs)."""
import numpy as np
import pytest
import torch

from huggingface_sagemaker_tensorflow_distributed_amd import ops
from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model, resolve_config
from huggingface_sagemaker_tensorflow_distributed_amd.ops import rng

B = 3
MASKS = ("none", "ragged", "first_key", "all_masked")


def _mask(kind, S):
    if kind == "none":
        return None
    m = np.ones((B, S), dtype=np.int64)
    m[0, max(1, S // 2):] = 0  # ragged padding
    if kind == "ragged":
        m[2, S - 1:] = 0
    elif kind == "first_key":
        m[1, 1:] = 0  # one sequence sees its first key only
    elif kind == "all_masked":
        m[1, :] = 0  # one sequence with every key masked (uniform softmax, as the reference ops define it)
    return m


def _model(name, layers, hidden, heads, dropout):
    cfg = resolve_config(name).replace(num_hidden_layers=layers, hidden_size=hidden, num_attention_heads=heads,
                                       intermediate_size=2 * hidden)
    if not dropout:
        cfg = cfg.replace(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, seq_classif_dropout=0.0,
                          classifier_dropout=0.0)
    return cfg, build_model(cfg, seed=1).train()


def _inputs(cfg, S, kind):
    g = np.random.default_rng(5)
    ids = g.integers(3, cfg.vocab_size, size=(B, S))
    mask = _mask(kind, S)
    t = torch.from_numpy
    kw = {"input_ids": t(ids), "labels": torch.tensor([1, 0, 1])}
    if mask is not None:
        kw["attention_mask"] = t(mask)
    return kw


def _step(model, monkeypatch, pruned, **kw):
    monkeypatch.setattr(ops, "CLS_ROWS_ONLY", pruned)
    model.zero_grad(set_to_none=True)
    model.rng.new_step(0)
    loss, logits = model(**kw)
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    return loss.detach(), logits.detach(), grads, model.rng.calls


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("dropout", [False, True])
@pytest.mark.parametrize("S", [2, 8])
@pytest.mark.parametrize("hidden,heads", [(64, 1), (128, 2)])
@pytest.mark.parametrize("layers", [2, 1])
@pytest.mark.parametrize("name", ["hsd-tiny-bert", "hsd-tiny-roberta", "hsd-tiny-distilbert"])
def test_pruned_step_equals_full_step_fp32(monkeypatch, name, layers, hidden, heads, S, dropout, kind):
    cfg, model = _model(name, layers, hidden, heads, dropout)
    kw = _inputs(cfg, S, kind)
    l0, y0, g0, c0 = _step(model, monkeypatch, False, **kw)
    l1, y1, g1, c1 = _step(model, monkeypatch, True, **kw)
    assert c1 == c0  # the seed counter advanced by the same amount
    torch.testing.assert_close(l1, l0, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(y1, y0, rtol=1e-5, atol=1e-6)
    assert set(g0) == set(g1)
    for n in g0:  # embeddings included
        torch.testing.assert_close(g1[n], g0[n], rtol=1e-5, atol=1e-6, msg=lambda m, n=n: f"{n}: {m}")


@pytest.mark.parametrize("layers", [2, 1])
def test_encoder_output_has_one_row_per_sequence(monkeypatch, layers):
    cfg, model = _model("hsd-tiny-bert", layers, 64, 1, True)
    kw = _inputs(cfg, 8, "ragged")
    args = (kw["input_ids"], kw["attention_mask"], None, model.rng, True)
    monkeypatch.setattr(ops, "CLS_ROWS_ONLY", True)
    assert model.encoder(*args, first_token_only=True).shape == (B, 1, 64)
    assert model.encoder(*args).shape == (B, 8, 64)  # a direct call that wants all hidden states
    monkeypatch.setattr(ops, "CLS_ROWS_ONLY", False)
    assert model.encoder(*args, first_token_only=True).shape == (B, 8, 64)


def test_odd_sequence_length_keeps_the_full_layer(monkeypatch):
    cfg, model = _model("hsd-tiny-bert", 2, 64, 1, False)
    kw = _inputs(cfg, 7, "none")
    monkeypatch.setattr(ops, "CLS_ROWS_ONLY", True)
    assert model.encoder(kw["input_ids"], None, None, model.rng, True, first_token_only=True).shape == (B, 7, 64)


def test_eval_without_labels_matches(monkeypatch):
    cfg, model = _model("hsd-tiny-roberta", 2, 64, 1, True)
    model.eval()
    kw = _inputs(cfg, 8, "ragged")
    kw.pop("labels")
    with torch.no_grad():
        monkeypatch.setattr(ops, "CLS_ROWS_ONLY", False)
        y0 = model(**kw)
        monkeypatch.setattr(ops, "CLS_ROWS_ONLY", True)
        y1 = model(**kw)
    torch.testing.assert_close(y1, y0, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("m", [2, 8, 128])
@pytest.mark.parametrize("W", [6, 64])
def test_keep_mask_row_multiplier_selects_rows_of_the_full_site(m, W):
    seed = 0x1234_5678_9ABC_DEF0
    full = rng.keep_mask(seed, (5 * m, W), 0.1)
    rows = rng.keep_mask(seed, (5, W), 0.1, row_mul=m)
    assert torch.equal(rows, full[::m])
    assert torch.equal(rng.keep_mask(seed, (5, W), 0.1, row_mul=1), rng.keep_mask(seed, (5, W), 0.1))


def test_reference_attention_cls_is_row_zero_of_reference_attention():
    from huggingface_sagemaker_tensorflow_distributed_amd.ops import reference as ref

    torch.manual_seed(0)
    Bq, S, heads = 2, 8, 2
    qkv = torch.randn(Bq * S, 3 * heads * 16)
    mb = ref.key_mask_bias(torch.tensor([[1] * 8, [1, 1, 1, 0, 0, 0, 0, 0]]))
    full = ref.attention(qkv, mb, Bq, S, heads, 0.25, 77, True).view(Bq, S, -1)[:, 0]
    torch.testing.assert_close(ref.attention_cls(qkv, mb, Bq, S, heads, 0.25, 77, True), full, rtol=1e-5, atol=1e-6)
