"""The MPNet family on the CPU: HF's bucket function, logits parity with transformers, checkpoint round trip, packed
equals padded, and what the family refuses."""
import numpy as np
import pytest
import torch

from huggingface_sagemaker_tensorflow_distributed_amd.data.packing import pack_batch, position_rule
from huggingface_sagemaker_tensorflow_distributed_amd.models import (build_model, from_pretrained, hf_state_dict,
                                                                     resolve_config, save_pretrained)
from huggingface_sagemaker_tensorflow_distributed_amd.models.encoder import relative_position_bucket

transformers = pytest.importorskip("transformers")
TABLE = "encoder.embeddings.relative_attention_table"


def test_bucket_index_equals_hf_for_every_distance_at_514():
    from transformers.models.mpnet.modeling_mpnet import MPNetEncoder

    delta = torch.arange(-513, 514)
    assert torch.equal(relative_position_bucket(delta, 32), MPNetEncoder.relative_position_bucket(delta, num_buckets=32))


def _batch(cfg, B=3, S=24):
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(5, cfg.vocab_size, (B, S), generator=g)
    am = torch.ones(B, S, dtype=torch.long)
    am[1, 15:] = 0
    ids[1, 15:] = cfg.pad_token_id
    return ids, am


def test_logits_parity_with_transformers_and_checkpoint_round_trip(tmp_path):
    from transformers import AutoModelForSequenceClassification

    cfg = resolve_config("hsd-tiny-mpnet")
    ours = build_model(cfg, seed=3).eval()
    with torch.no_grad():  # a bias of the scores' own size, so a wrong bucket or sign cannot pass
        ours.encoder.embeddings.relative_attention_table.normal_(0.0, 1.0, generator=torch.Generator().manual_seed(1))
    save_pretrained(ours, str(tmp_path))
    hf = AutoModelForSequenceClassification.from_pretrained(str(tmp_path)).eval()
    assert type(hf).__name__ == "MPNetForSequenceClassification"
    assert set(hf_state_dict(ours)) == set(hf.state_dict())
    ids, am = _batch(cfg)
    with torch.no_grad():
        want = hf(input_ids=ids, attention_mask=am).logits
        torch.testing.assert_close(ours(ids, attention_mask=am), want, atol=1e-5, rtol=1e-4)
        again = from_pretrained(str(tmp_path)).eval()
        torch.testing.assert_close(again.encoder.embeddings.relative_attention_table,
                                   ours.encoder.embeddings.relative_attention_table)
        torch.testing.assert_close(again(ids, attention_mask=am), want, atol=1e-5, rtol=1e-4)


@pytest.mark.parametrize("task", ["sequence-classification", "token-classification"])
def test_packed_step_equals_padded_step_fp32(task):
    """Dropout off, lengths 64 / 40 / 17 / 2 (tests/test_packing.py): loss and every gradient, the table's included."""
    cfg = resolve_config("hsd-tiny-mpnet").replace(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model = build_model(cfg, task=task, seed=1).train()
    g = np.random.default_rng(3)
    mask = (np.arange(64)[None, :] < np.array([64, 40, 17, 2])[:, None]).astype(np.int64)
    ids = np.where(mask != 0, g.integers(5, cfg.vocab_size, size=(4, 64)), cfg.pad_token_id)
    labels = np.array([1, 0, 0, 1]) if task == "sequence-classification" else np.where(mask != 0, ids % 2, -100)
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
        steps.append((loss.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}))
    (l0, g0), (l1, g1) = steps
    torch.testing.assert_close(l1, l0, rtol=1e-5, atol=1e-6)
    assert g0[TABLE].abs().sum() > 0
    for n in g0:
        torch.testing.assert_close(g1[n], g0[n], rtol=1e-5, atol=1e-6, msg=lambda m, n=n: f"{n}: {m}")


@pytest.mark.parametrize("flags,match", [(["--dtype", "fp8"], "fp8"), (["--task", "masked-lm"], "masked-lm")])
def test_mpnet_refuses_fp8_and_masked_lm(fake_sm_env, flags, match):
    from huggingface_sagemaker_tensorflow_distributed_amd.train.runner import build
    from huggingface_sagemaker_tensorflow_distributed_amd.utils.args import build_parser

    args, _ = build_parser("train").parse_known_args(["--model_name_or_path", "hsd-tiny-mpnet", "--device", "cpu"] + flags)
    with pytest.raises(ValueError, match=match):
        build(args, "train")
