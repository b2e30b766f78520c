"""--mlm_masking dynamic on the CPU: the mask definition (ops/rng.py "MLM mask") and its statistics, the seeds, the
capacity rule and overflow, a dynamic model step against the static step on the reference-masked batch (padded and
packed, fp32, dropout on), the synthetic-bigram corpus and the CLI."""
import json
import math

import numpy as np
import pytest
import torch

from huggingface_sagemaker_tensorflow_distributed_amd import data as hdata
from huggingface_sagemaker_tensorflow_distributed_amd.data.packing import pack_batch, position_rule
from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model, resolve_config
from huggingface_sagemaker_tensorflow_distributed_amd.ops import rng
from huggingface_sagemaker_tensorflow_distributed_amd.ops.rng import DropoutSeeds, mlm_capacity, mlm_mask_reference

V, MASK, SPECIAL, RANGE = 50265, 50264, (0, 1, 2, 50264), (3, 50265)
P = 0.15
SEEDS = (0x0123_4567_89AB_CDEF, 42, 0xFEDC_BA98_7654_3210)
NBIG = 1 << 20


def _ids(n, seed=0, lo=3, hi=V - 1):
    return torch.from_numpy(np.random.default_rng(seed).integers(lo, hi, size=n, dtype=np.int64))


_BIG = {}


def _big(seed):
    """The reference mask of 2^20 maskable tokens under ``seed``: computed once, shared, never modified."""
    if seed not in _BIG:
        ids = _ids(NBIG, seed=1)
        _BIG[seed] = (ids, mlm_mask_reference(ids, None, None, seed, P, MASK, SPECIAL, RANGE))
    return _BIG[seed]


def _within(count, n, q, what, sigmas=4.0):
    sd = math.sqrt(n * q * (1.0 - q))
    assert abs(count - n * q) <= sigmas * sd, f"{what}: {count} of {n}, expected {n * q:.1f} +- {sigmas} x {sd:.1f}"


# ------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("seed", SEEDS)
def test_reference_masker_rates_are_nominal(seed):
    ids, m = _big(seed)
    sel = m.labels != -100
    n = int(sel.sum())
    assert int(m.counts[0]) == n and int(m.counts[1]) == 0 and float(m.n_valid[0]) == n
    _within(n, NBIG, rng.threshold(P) / 65536.0, "selected share")
    out, orig = m.input_ids[sel], ids[sel]
    # the three branches, told apart by what the definition draws (w0's high half), not by the outcome: a random
    # replacement may land on the original id
    key = rng.site_key(seed & rng.M32, (seed >> 32) & rng.M32)
    t = torch.arange(NBIG, dtype=torch.int64)
    a = (rng.pair_bits(key, t, torch.zeros_like(t)) >> 16)[sel]
    is_mask, is_rand = a < 52429, (a >= 52429) & (a < 58982)
    is_keep = a >= 58982
    _within(int(is_mask.sum()), n, 52429 / 65536.0, "<mask> share")
    _within(int(is_rand.sum()), n, 6553 / 65536.0, "random share")
    _within(int(is_keep.sum()), n, 6554 / 65536.0, "unchanged share")
    assert (out[is_mask] == MASK).all() and torch.equal(out[is_keep], orig[is_keep])
    r = out[is_rand]
    lo, hi = RANGE
    assert int(r.min()) >= lo and int(r.max()) < hi
    k = hi - lo  # uniform over k ids: mean lo + (k-1)/2, variance (k^2-1)/12
    sd_mean = math.sqrt((k * k - 1) / 12.0 / r.numel())
    assert abs(float(r.double().mean()) - (lo + (k - 1) / 2.0)) <= 4.0 * sd_mean
    # labels: the original id exactly at the selected positions; every other token is untouched
    assert torch.equal(m.labels[sel], orig) and torch.equal(m.input_ids[~sel], ids[~sel])
    # the compaction: ascending positions, their ids, ranks
    pos = sel.nonzero(as_tuple=True)[0]
    assert torch.equal(m.sel[:n], pos) and torch.equal(m.tgt[:n], orig)
    assert (m.sel[n:] == 0).all() and (m.tgt[n:] == -100).all()
    assert torch.equal(m.inv[pos].long(), torch.arange(n)) and (m.inv[~sel] == -1).all()
    # neighbours are selected together at the rate of independent draws
    both = int((sel[1:] & sel[:-1]).sum())
    q = rng.threshold(P) / 65536.0
    _within(both, NBIG - 1, q * q, "adjacent pair rate")


def test_unmaskable_positions_are_never_selected():
    n = 1 << 16
    ids = _ids(n, seed=2)
    ids[::7] = 1      # pad
    ids[3::11] = 0    # bos
    ids[5::13] = 2    # eos
    ids[1::17] = MASK
    am = torch.ones(n, dtype=torch.int64)
    am[n // 2:n // 2 + 5000] = 0
    lab = torch.zeros(n, dtype=torch.int64)
    lab[1000:3000] = -100
    m = mlm_mask_reference(ids, am, lab, SEEDS[0], 1.0, MASK, SPECIAL, RANGE)  # p = 1: every maskable token
    sel = m.labels != -100
    special = (ids == 0) | (ids == 1) | (ids == 2) | (ids == MASK)
    maskable = ~special & (am != 0) & (lab != -100)
    assert torch.equal(sel, maskable) and int(m.counts[0]) == int(maskable.sum()) <= m.cap
    assert torch.equal(m.input_ids[~sel], ids[~sel])
    # a [B, S] batch is its flat buffer
    m2 = mlm_mask_reference(ids.view(64, -1), am.view(64, -1), lab.view(64, -1), SEEDS[0], 1.0, MASK, SPECIAL, RANGE)
    assert m2.input_ids.shape == (64, n // 64) and torch.equal(m2.input_ids.view(-1), m.input_ids)
    assert torch.equal(m2.sel, m.sel)


def test_mlm_seeds_vary_with_k_step_and_rank_and_leave_the_dropout_stream_alone():
    s = DropoutSeeds(7, rank=0)
    s.new_step(3)
    d0 = s.next()
    calls = s.calls
    k0, k1 = s.mlm_seed(), s.mlm_seed()
    assert s.calls == calls, "mlm_seed() must not advance the dropout call counter"
    d1 = s.next()
    s.new_step(3)
    assert (s.next(), s.mlm_seed(), s.mlm_seed(), s.next()) == (d0, k0, k1, d1)  # replayable, k restarts
    s.new_step(4)
    k_step = s.mlm_seed()
    r1 = DropoutSeeds(7, rank=1)
    r1.new_step(3)
    k_rank = r1.mlm_seed()
    assert len({k0, k1, k_step, k_rank, d0, d1}) == 6
    ids = _ids(4096, seed=3)
    masks = [mlm_mask_reference(ids, None, None, k, P, MASK, SPECIAL, RANGE).labels for k in (k0, k1, k_step, k_rank)]
    for i in range(4):
        for j in range(i):
            assert not torch.equal(masks[i], masks[j])
    again = mlm_mask_reference(ids, None, None, k0, P, MASK, SPECIAL, RANGE)
    assert torch.equal(again.labels, masks[0])
    # evaluation seeds: the batch index only
    assert s.mlm_eval_seed(5) == DropoutSeeds(7, rank=3).mlm_eval_seed(5) != s.mlm_eval_seed(6)
    assert DropoutSeeds(8).mlm_eval_seed(5) != s.mlm_eval_seed(5)


# ------------------------------------------------------------------------------------------ capacity, overflow
def test_overflow_drops_the_selections_beyond_cap():
    ids = _ids(1000, seed=4)
    full = mlm_mask_reference(ids, None, None, SEEDS[1], P, MASK, SPECIAL, RANGE)
    count = int(full.counts[0])
    assert count > 64 and int(full.counts[1]) == 0
    m = mlm_mask_reference(ids, None, None, SEEDS[1], P, MASK, SPECIAL, RANGE, cap=64)
    assert m.cap == 64 and m.sel.shape == (64,)
    assert int(m.counts[0]) == 64 and int(m.counts[1]) == count - 64 and float(m.n_valid[0]) == 64.0
    kept, dropped = full.sel[:64], full.sel[64:count]
    assert torch.equal(m.sel, kept) and torch.equal(m.tgt, full.tgt[:64])
    assert torch.equal(m.input_ids[dropped], ids[dropped]) and (m.labels[dropped] == -100).all()
    assert (m.inv[dropped] == -1).all() and torch.equal(m.inv[kept].long(), torch.arange(64))
    assert torch.equal(m.input_ids[kept], full.input_ids[kept]) and torch.equal(m.labels[kept], ids[kept])


@pytest.mark.parametrize("n,cap", [(256, 128), (1000, 256), (2048, 448), (32768, 5248)])
def test_capacity_bounds_the_selected_count(n, cap):
    assert mlm_capacity(n, P) == cap and cap % 64 == 0
    key_rows = torch.arange(n, dtype=torch.int64)
    zero = torch.zeros_like(key_rows)
    thr = rng.threshold(P)
    worst = 0
    for i in range(200):
        seed = DropoutSeeds(i).mlm_seed()
        key = rng.site_key(seed & rng.M32, (seed >> 32) & rng.M32)
        worst = max(worst, int(((rng.pair_bits(key, key_rows, zero) & 0xFFFF) < thr).sum()))
    print(f"N={n}: worst count {worst} of cap {cap}")
    assert worst <= cap
    assert mlm_capacity(1, P) == 64 and mlm_capacity(1000, 1.0) >= 1000


# ------------------------------------------------------------------------------------------ model step
LENGTHS = (64, 40, 17, 5)


def _raw_batch(cfg, seed=3):
    g = np.random.default_rng(seed)
    B, S = len(LENGTHS), 64
    ids = g.integers(3, cfg.vocab_size, size=(B, S), dtype=np.int64)
    mask = (np.arange(S)[None, :] < np.asarray(LENGTHS)[:, None]).astype(np.int64)
    ids[:, 0] = cfg.bos_token_id
    ids[np.arange(B), np.asarray(LENGTHS) - 1] = cfg.eos_token_id
    ids[mask == 0] = cfg.pad_token_id
    return ids, mask, np.where(mask != 0, 0, -100).astype(np.int64)


def _step(model, **kw):
    model.zero_grad(set_to_none=True)
    model.rng.new_step(5)
    loss, _ = model(**kw)
    loss.backward()
    return loss.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
def test_dynamic_step_equals_static_step_on_the_reference_mask_fp32(packed):
    """hsd-tiny-roberta, fp32, dropout ON: a dynamic step on raw ids equals the static step on (ids', labels') made
    by the reference masker under the same seed -- loss and every gradient at the bound of tests/test_packing.py.
    Holds only if mlm_seed() leaves the dropout seeds of the step where the static step finds them."""
    cfg = resolve_config("hsd-tiny-roberta")
    assert cfg.hidden_dropout_prob > 0
    model = build_model(cfg, task="masked-lm", seed=1).train()
    model.rng.base_seed = 11
    ids, mask, lab = _raw_batch(cfg)
    t = torch.from_numpy
    p = 0.3  # enough selections in 126 tokens
    if packed:
        pk = pack_batch(ids, mask, lab, **position_rule(cfg))
        kw = dict(input_ids=t(pk["input_ids"]), cu_seqlens=t(pk["cu_seqlens"]), max_seqlen=pk["max_seqlen"],
                  position_ids=t(pk["position_ids"]))
        raw_ids, raw_mask, raw_lab = kw.pop("input_ids"), None, t(np.asarray(pk["labels"]))
    else:
        kw = dict(attention_mask=t(mask))
        raw_ids, raw_mask, raw_lab = t(ids), t(mask), t(lab)
    model.set_mlm_masking("dynamic", p)
    assert model.graph_safe
    l1, g1 = _step(model, input_ids=raw_ids, labels=raw_lab, **kw)
    seeds = DropoutSeeds(11)
    seeds.new_step(5)
    m = mlm_mask_reference(raw_ids, raw_mask, raw_lab, seeds.mlm_seed(), p, model.mask_token_id,
                           model.mlm_special_ids(), model.mlm_rand_range())
    n = int(m.counts[0])
    assert 10 < n < m.cap and (m.input_ids != raw_ids).any()
    model.set_mlm_masking("static", p)
    assert not model.graph_safe
    l0, g0 = _step(model, input_ids=m.input_ids, labels=m.labels, **kw)
    print(f"{'packed' if packed else 'padded'}: n={n} cap={m.cap} loss dynamic {float(l1)!r} static {float(l0)!r}")
    torch.testing.assert_close(l1, l0, rtol=1e-5, atol=1e-6)
    assert set(g0) == set(g1)
    for name in g0:
        torch.testing.assert_close(g1[name], g0[name], rtol=1e-5, atol=1e-6, msg=lambda s, name=name: f"{name}: {s}")
    assert model.mlm_dropped() == 0


def test_dynamic_loss_carries_device_stats_and_nothing_maskable_gives_zero():
    cfg = resolve_config("hsd-tiny-roberta")
    model = build_model(cfg, task="masked-lm", seed=1).train()
    model.set_mlm_masking("dynamic", P)
    ids, mask, lab = _raw_batch(cfg)
    model.rng.new_step(0)
    loss, logits = model(torch.from_numpy(ids), attention_mask=torch.from_numpy(mask), labels=torch.from_numpy(lab))
    st = loss._hsd_stats
    assert st.shape == (4,) and float(st[2]) > 0 and logits.shape == (mlm_capacity(ids.size, P), cfg.vocab_size)
    torch.testing.assert_close(st[3] / st[2], loss.detach())
    model.rng.new_step(0)
    none = torch.full_like(torch.from_numpy(lab), -100)
    loss0, _ = model(torch.from_numpy(ids), attention_mask=torch.from_numpy(mask), labels=none)
    assert float(loss0.detach()) == 0.0 and float(loss0._hsd_stats[2]) == 0.0
    loss0.backward()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)


# ------------------------------------------------------------------------------------------ corpora
def test_synthetic_bigram_follows_its_successor_table_nine_times_in_ten():
    Vt = 1024
    ds = hdata.synthetic_bigram(2048, 128, Vt, seed=5)
    succ = hdata.bigram_successor(Vt)
    assert sorted(succ[3:].tolist()) == list(range(3, Vt)) and succ[:3].tolist() == [0, 1, 2]
    lengths = ds.attention_mask.sum(axis=1)
    assert lengths.min() >= 32 and lengths.max() <= 128 and len(set(lengths.tolist())) > 20
    ids = ds.input_ids.astype(np.int64)
    pos = np.arange(128)[None, :]
    inner = (pos >= 1) & (pos + 1 <= lengths[:, None] - 2)  # both x[i] and x[i+1] are corpus tokens
    a, b = ids[:, :-1][inner[:, :-1]], ids[:, 1:][inner[:, :-1]]
    assert a.size >= 100_000
    share = float((succ[a] == b).mean())
    print(f"{a.size} transitions, {share:.4f} follow succ")
    assert 0.88 <= share <= 0.92
    assert (ids[:, 0] == 0).all() and (ids[np.arange(2048), lengths - 1] == 2).all()
    assert (ids[ds.attention_mask == 0] == 1).all() and (ds.labels[ds.attention_mask == 0] == -100).all()
    assert (ds.labels[ds.attention_mask != 0] != -100).all()
    again = hdata.synthetic_bigram(2048, 128, Vt, seed=5)
    other = hdata.synthetic_bigram(2048, 128, Vt, seed=6)
    assert np.array_equal(again.input_ids, ds.input_ids) and not np.array_equal(other.input_ids, ds.input_ids)


def test_raw_synthetic_corpus_is_unmasked_and_ragged():
    ds = hdata.synthetic_mlm_raw(256, 64, 1024, seed=0)
    lengths = ds.attention_mask.sum(axis=1)
    assert lengths.min() >= 16 and len(set(lengths.tolist())) > 10
    assert not (ds.input_ids == 50264 % 1024).all(axis=1).any()
    assert (ds.labels[ds.attention_mask != 0] != -100).all() and (ds.labels[ds.attention_mask == 0] == -100).all()


# ------------------------------------------------------------------------------------------ CLI
def _args(extra):
    from huggingface_sagemaker_tensorflow_distributed_amd.utils.args import build_parser

    return build_parser("train").parse_known_args(
        ["--model_name_or_path", "hsd-tiny-roberta", "--task", "masked-lm", "--device", "cpu", "--max_seq_length", "32",
         "--num_train_examples", "16", "--num_eval_examples", "8", "--seed", "9"] + extra)[0]


def test_cli_flags_parse_and_default_to_static():
    a = _args([])
    assert a.mlm_masking == "static" and a.mlm_probability == 0.15
    b = _args(["--mlm_masking", "dynamic", "--mlm_probability", "0.2", "--dataset", "synthetic-bigram"])
    assert b.mlm_masking == "dynamic" and b.mlm_probability == 0.2 and b.dataset == "synthetic-bigram"
    with pytest.raises(SystemExit):
        _args(["--mlm_masking", "sometimes"])


def test_static_run_reads_the_corpus_synthetic_mlm_has_always_built():
    from huggingface_sagemaker_tensorflow_distributed_amd.train.runner import _datasets

    cfg = resolve_config("hsd-tiny-roberta")
    tr, te = _datasets(_args([]), cfg, None, 32)
    want_tr = hdata.synthetic_mlm(16, 32, cfg.vocab_size, seed=9)
    want_te = hdata.synthetic_mlm(8, 32, cfg.vocab_size, seed=10)
    for got, want in ((tr, want_tr), (te, want_te)):
        assert np.array_equal(got.input_ids, want.input_ids) and got.input_ids.dtype == want.input_ids.dtype
        assert np.array_equal(got.labels, want.labels) and np.array_equal(got.attention_mask, want.attention_mask)
    # dynamic: the raw variant; bigram under static masking: masked once by the reference masker
    raw, _ = _datasets(_args(["--mlm_masking", "dynamic"]), cfg, None, 32)
    assert (raw.labels[raw.attention_mask != 0] == 0).all()
    big, _ = _datasets(_args(["--dataset", "synthetic-bigram", "--mlm_probability", "0.5"]), cfg, None, 32)
    src = hdata.synthetic_bigram(16, 32, cfg.vocab_size, seed=9, pad_id=cfg.pad_token_id)
    masked = big.labels != -100
    assert masked.any() and np.array_equal(big.labels[masked], src.input_ids[masked])
    assert np.array_equal(big.input_ids[~masked], src.input_ids[~masked])
    with pytest.raises(ValueError, match="masked-lm"):
        a = _args(["--dataset", "synthetic-bigram"])
        a.task = "sequence-classification"
        _datasets(a, cfg, None, 32)


def test_cli_dynamic_run_end_to_end_and_evaluating_twice_scores_the_same_masks(tmp_path, monkeypatch):
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import ShardSampler
    from huggingface_sagemaker_tensorflow_distributed_amd.train.runner import build, run

    d, m = tmp_path / "data", tmp_path / "model"
    monkeypatch.setenv("SM_OUTPUT_DATA_DIR", str(d))
    monkeypatch.setenv("SM_MODEL_DIR", str(m))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        monkeypatch.delenv(k, raising=False)
    argv = ["--model_name_or_path", "hsd-tiny-roberta", "--task", "masked-lm", "--device", "cpu", "--max_seq_length",
            "32", "--num_train_examples", "16", "--num_eval_examples", "8", "--epochs", "1", "--train_batch_size", "4",
            "--eval_batch_size", "4", "--max_steps", "2", "--log_every", "1", "--mlm_masking", "dynamic", "--dataset",
            "synthetic-bigram", "--gradient_accumulation_steps", "2"]
    out = run(argv)
    assert out["global_step"] == 2 and math.isfinite(out["eval"]["loss"])
    prov = json.loads((d / "run_provenance.json").read_text())
    assert prov["mlm_masking"] == "dynamic" and prov["mlm_probability"] == 0.15 and "bigram" in prov["corpus"]
    # two evaluations, a training step between them (lr 0: same weights, but the step and its seeds move on)
    from huggingface_sagemaker_tensorflow_distributed_amd.utils.args import build_parser

    args = build_parser("train").parse_known_args(argv + ["--learning_rate", "0"])[0]
    parts = build(args, "train")
    trainer, model = parts["trainer"], parts["model"]
    assert model.mlm_masking == "dynamic"
    ds = hdata.synthetic_bigram(8, 32, model.cfg.vocab_size, seed=1, pad_id=model.cfg.pad_token_id)

    def loader():
        return hdata.BatchLoader(ds, ShardSampler(8, 0, 1, shuffle=False, batch_size=4, drop_last=False,
                                                  mark_padding=True), torch.device("cpu"))

    e1 = trainer.evaluate(loader())
    trainer.train_step(list(loader()))
    e2 = trainer.evaluate(loader())
    assert e1 == e2 and math.isfinite(e1["loss"])
    # and the two eval batches do not share one mask
    model.eval()
    b = next(iter(loader()))
    model.mlm_eval_index = 0
    m0 = model.mask_batch(b["input_ids"], b["attention_mask"], b["labels"])
    model.mlm_eval_index = 1
    m1 = model.mask_batch(b["input_ids"], b["attention_mask"], b["labels"])
    assert not torch.equal(m0.labels, m1.labels)
