"""``--ema_decay`` / ``--ema_warmup`` (``ema_decay=`` of FusedAdam / FusedLamb, optim/adam.py) on the CPU tier: the
reference-path formula against a per-parameter fp64 average, the warm-up rule, refused values, the off state,
checkpoints, two data-parallel ranks, the command line and the marker task."""
import json
import logging
import math
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn as nn

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CPU = torch.device("cpu")
PKG = "huggingface_sagemaker_tensorflow_distributed_amd"


class _Toy(nn.Module):
    """Five parameters of odd sizes: an embedding, a weight, a bias and a LayerNorm weight (no decay), a head."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(0)
        self.emb_weight = nn.Parameter(torch.randn(9, 7, generator=g) * 0.3)
        self.dense_weight = nn.Parameter(torch.randn(7, 13, generator=g) * 0.3)
        self.dense_bias = nn.Parameter(torch.randn(13, generator=g) * 0.1)
        self.ln_weight = nn.Parameter(1.0 + torch.randn(13, generator=g) * 0.1)
        self.head_weight = nn.Parameter(torch.randn(70, generator=g) * 0.2)


def _toy(cls_name, **kw):
    from huggingface_sagemaker_tensorflow_distributed_amd import optim
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore

    store = FlatParamStore(_Toy(), CPU)
    return store, getattr(optim, cls_name)(store, **kw)


def _fill(store, gen):
    store.grad.zero_()
    for s in store.segments:
        store.grad[s.offset:s.offset + s.numel] = torch.randn(s.numel, generator=gen)


def _warm(d, t):
    return min(d, (1.0 + t) / (10.0 + t))


# ------------------------------------------------------------------------------------------ 1. the formula
@pytest.mark.parametrize("cls_name", ["FusedAdam", "FusedLamb"])
@pytest.mark.parametrize("warmup", [False, True])
def test_cpu_average_is_the_three_operation_formula_and_tracks_fp64(cls_name, warmup):
    """After every step ``ema`` is ``e + w·(θ - e)`` in fp32, bit for bit, from the weights the step wrote, and it
    stays within a derived bound of a per-parameter fp64 average (same w = float32(1 - d_t)) of the same fp32 weight
    trajectory. One step rounds three times: the subtract errs by at most 2⁻²⁴·|θ - e|, which the product scales by w;
    the product by 2⁻²⁴·w·|θ - e|; the sum by 2⁻²⁴·|ema_new|. Earlier errors are damped by 1 - w per step."""
    d, steps = 0.9, 20
    store, opt = _toy(cls_name, lr=2e-3, weight_decay=0.01, ema_decay=d, ema_warmup=warmup)
    assert opt.ema.data_ptr() != store.master.data_ptr() and torch.equal(opt.ema, store.master)
    at = opt.ema.data_ptr()
    gen = torch.Generator().manual_seed(3)
    ref64 = store.master.double().clone()
    bound = torch.zeros(store.numel, dtype=torch.float64)
    for t in range(steps):
        _fill(store, gen)
        e = opt.ema.clone()
        opt.step(grad_scale=0.5)
        d_t = _warm(d, t) if warmup else d
        assert opt.ema_decay_at(t) == d_t
        w = torch.tensor(1.0 - d_t, dtype=torch.float32)
        assert torch.equal(opt.ema, e + w * (store.master - e))
        w64 = float(w)
        ref64 += w64 * (store.master.double() - ref64)
        diff = (store.master.double() - e.double()).abs()
        bound = bound * (1.0 - w64) + 2.0 ** -24 * (2.0 * w64 * diff * (1.0 + 2.0 ** -23) + opt.ema.double().abs())
        err = (opt.ema.double() - ref64).abs()
        assert bool((err <= bound).all()), (t, float(err.max()), float(bound.max()))
    assert opt.ema.data_ptr() == at and opt.step_count == steps
    assert not torch.equal(opt.ema, store.master)
    views = opt.ema_state()
    assert list(views) == store.names
    for s in store.segments:
        assert views[s.name].shape == torch.Size(s.shape)
        assert views[s.name].data_ptr() == opt.ema[s.offset:].data_ptr()
    # alignment padding holds zeros, as in master
    keep = torch.zeros(store.numel, dtype=torch.bool)
    for s in store.segments:
        keep[s.offset:s.offset + s.numel] = True
    assert int(torch.count_nonzero(opt.ema[~keep])) == 0


@pytest.mark.parametrize("cls_name", ["FusedAdam", "FusedLamb"])
def test_the_step_is_undisturbed_on_the_cpu(cls_name):
    """master, m, v with averaging on are the bits of the run without it; clipping and accumulation-style scales too."""
    (sa, a), (sb, b) = (_toy(cls_name, lr=2e-3, weight_decay=0.01, max_grad_norm=0.5, **kw)
                        for kw in ({}, {"ema_decay": 0.99, "ema_warmup": True}))
    for opt_store in ((sa, a), (sb, b)):
        gen = torch.Generator().manual_seed(5)
        for _ in range(4):
            _fill(opt_store[0], gen)
            opt_store[1].step(grad_scale=0.25)
    assert torch.equal(sa.master, sb.master) and torch.equal(a.exp_avg, b.exp_avg)
    assert torch.equal(a.exp_avg_sq, b.exp_avg_sq)


def test_warmup_rule():
    _, opt = _toy("FusedAdam", ema_decay=0.999, ema_warmup=True)
    assert opt.ema_decay_at(0) == 0.1 and opt.ema_decay_at(1) == 2.0 / 11.0
    assert opt.ema_decay_at(89) == 90.0 / 99.0
    # (1 + t)/(10 + t) reaches 0.999 at t = 8,990: from there on the constant
    assert opt.ema_decay_at(8989) == 8990.0 / 8999.0 < 0.999
    assert opt.ema_decay_at(8990) == 0.999 == opt.ema_decay_at(8991) == opt.ema_decay_at(10 ** 9)
    _, const = _toy("FusedLamb", ema_decay=0.999)
    assert [const.ema_decay_at(t) for t in (0, 1, 89, 8990, 10 ** 9)] == [0.999] * 5


@pytest.mark.parametrize("cls_name", ["FusedAdam", "FusedLamb"])
@pytest.mark.parametrize("bad", [-0.1, 1.0, 1.5, float("inf"), float("-inf"), float("nan")])
def test_bad_decay_is_refused_at_construction(cls_name, bad):
    with pytest.raises(ValueError, match="ema_decay"):
        _toy(cls_name, ema_decay=bad)


def test_warmup_without_a_decay_is_refused():
    with pytest.raises(ValueError, match="ema_warmup"):
        _toy("FusedAdam", ema_warmup=True)


@pytest.mark.parametrize("cls_name", ["FusedAdam", "FusedLamb"])
def test_off_allocates_nothing_and_adds_no_state(cls_name):
    store, off = _toy(cls_name, lr=1e-3)
    _, on = _toy(cls_name, lr=1e-3, ema_decay=0.5)
    assert off.ema is None and off.ema_state() is None and len(off.state_tensors()) == 2
    assert set(on.state_dict()) - set(off.state_dict()) == {"ema", "ema_decay", "ema_warmup"}
    assert len(on.state_tensors()) == 3 and on.state_tensors()[2] is on.ema
    off.reset_ema()  # nothing to do
    with pytest.raises(RuntimeError, match="ema_decay"):
        with off.ema_weights():
            pass


# ------------------------------------------------------------------------------------------ 2. the swap (CPU)
def _trainer(seed=0, lamb=False, decay=0.9, warmup=True, dropout=0.1):
    from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model, resolve_config
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedAdam, FusedLamb
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore
    from huggingface_sagemaker_tensorflow_distributed_amd.train.trainer import Trainer

    cfg = resolve_config("hsd-tiny-bert").replace(hidden_dropout_prob=dropout, attention_probs_dropout_prob=dropout)
    model = build_model(cfg, seed=seed)
    model.rng.base_seed = 7
    store = FlatParamStore(model, CPU)
    opt = (FusedLamb if lamb else FusedAdam)(store, lr=1e-3, weight_decay=0.01, ema_decay=decay, ema_warmup=warmup)
    return Trainer(model, store, opt, None, CPU)


def _batches(n, B=8, S=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        am = torch.ones(B, S, dtype=torch.long)
        am[::3, S // 2:] = 0
        out.append({"input_ids": torch.randint(5, 1024, (B, S), generator=g), "attention_mask": am,
                    "labels": torch.randint(0, 2, (B,), generator=g)})
    return out


def test_ema_weights_exchanges_contents_and_puts_them_back():
    data = _batches(4)
    tr, twin = _trainer(), _trainer()
    for t in (tr, twin):
        for b in data[:3]:
            t.train_step([b])
    opt, store = tr.optimizer, tr.store
    opt._EXCHANGE_CHUNK = 1000  # the exchange goes chunk by chunk: several chunks here, the last one short
    assert store.numel % 1000 != 0 and store.numel > 3000
    master, ema, m, v = store.master.clone(), opt.ema.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()
    at = (store.master.data_ptr(), opt.ema.data_ptr())
    raw = tr.evaluate(data[:2])
    with opt.ema_weights():
        assert (store.master.data_ptr(), opt.ema.data_ptr()) == at
        assert torch.equal(store.master, ema) and torch.equal(opt.ema, master)
        inside = tr.evaluate(data[:2])
        with pytest.raises(RuntimeError, match="ema_weights"):
            tr.train_step([data[3]])
        with pytest.raises(RuntimeError, match="ema_weights"):
            opt.step()
        with pytest.raises(RuntimeError, match="already active"):
            with opt.ema_weights():
                pass
    assert torch.equal(store.master, master) and torch.equal(opt.ema, ema)
    assert torch.equal(opt.exp_avg, m) and torch.equal(opt.exp_avg_sq, v) and opt.step_count == 3
    assert tr.evaluate(data[:2], weights="ema") == inside != raw
    assert tr.evaluate(data[:2]) == raw
    with pytest.raises(ValueError, match="weights"):
        tr.evaluate(data[:2], weights="swa")
    # an exception inside the scope still puts everything back
    with pytest.raises(KeyError):
        with opt.ema_weights():
            raise KeyError("x")
    assert torch.equal(store.master, master) and torch.equal(opt.ema, ema)
    tr.train_step([data[3]])
    twin.train_step([data[3]])
    assert torch.equal(store.master, twin.store.master) and torch.equal(opt.ema, twin.optimizer.ema)


def test_accumulation_moves_the_average_once_per_optimizer_step():
    data = _batches(4)
    tr = _trainer(warmup=True)
    e = tr.optimizer.ema.clone()
    for t in range(2):
        tr.train_step(data[2 * t:2 * t + 2])
        w = torch.tensor(1.0 - _warm(0.9, t), dtype=torch.float32)
        e = e + w * (tr.store.master - e)
        assert torch.equal(tr.optimizer.ema, e)
    assert tr.optimizer.step_count == 2


# ------------------------------------------------------------------------------------------ 3. checkpoints
@pytest.mark.parametrize("lamb", [False, True])
def test_checkpoint_resume_equals_uninterrupted_bit_for_bit(tmp_path, lamb, caplog):
    from huggingface_sagemaker_tensorflow_distributed_amd.train.callbacks import load_checkpoint, save_checkpoint

    data = _batches(4)
    ref = _trainer(lamb=lamb)
    for b in data:
        ref.train_step([b])
    a = _trainer(lamb=lamb)
    for b in data[:2]:
        a.train_step([b])
    ck = str(tmp_path / "checkpoint-1")
    save_checkpoint(ck, a, epoch=1)
    sd = torch.load(os.path.join(ck, "optimizer.pt"), map_location="cpu", weights_only=True)
    assert torch.equal(sd["ema"], a.optimizer.ema) and sd["ema_decay"] == 0.9 and sd["ema_warmup"] is True
    b = _trainer(seed=123, lamb=lamb)  # different init: everything must come from the checkpoint
    with caplog.at_level(logging.WARNING, logger=PKG):
        load_checkpoint(ck, b)
    assert not [r for r in caplog.records if "ema" in r.getMessage() or "average" in r.getMessage()]
    for x in data[2:]:
        b.train_step([x])
    assert torch.equal(b.store.master, ref.store.master) and torch.equal(b.optimizer.ema, ref.optimizer.ema)
    assert not torch.equal(b.optimizer.ema, b.store.master)


def test_resuming_without_an_average_restarts_it_and_flag_mismatches_warn(tmp_path, caplog):
    from huggingface_sagemaker_tensorflow_distributed_amd.train.callbacks import load_checkpoint, save_checkpoint

    data = _batches(2)
    off = _trainer(decay=0.0, warmup=False)
    off.train_step([data[0]])
    assert "ema" not in off.optimizer.state_dict()
    ck = str(tmp_path / "checkpoint-1")
    save_checkpoint(ck, off, epoch=1)
    on = _trainer(seed=5)
    on.train_step([data[1]])
    with caplog.at_level(logging.WARNING, logger=PKG):
        load_checkpoint(ck, on)
    msgs = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert any("restarts from the loaded weights" in m for m in msgs), msgs
    assert any("--ema_decay" in m and "win" in m for m in msgs), msgs
    assert torch.equal(on.store.master, off.store.master) and torch.equal(on.optimizer.ema, off.store.master)
    assert on.optimizer.ema_decay == 0.9 and on.optimizer.ema_warmup is True
    # other values of the flags: a warning, the current ones win, the stored average is taken
    on.train_step([data[1]])
    for kw in ({"decay": 0.5}, {"warmup": False}):
        other = _trainer(**kw)
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger=PKG):
            other.optimizer.load_state_dict(on.optimizer.state_dict())
        msgs = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
        assert any("--ema_decay" in m and "win" in m for m in msgs), msgs
        assert (other.optimizer.ema_decay, other.optimizer.ema_warmup) == (kw.get("decay", 0.9), kw.get("warmup", True))
        assert torch.equal(other.optimizer.ema, on.optimizer.ema)
    # a checkpoint with an average into an optimizer without: a warning, nothing allocated
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger=PKG):
        off.optimizer.load_state_dict(on.optimizer.state_dict())
    assert any("--ema_decay" in r.getMessage() for r in caplog.records) and off.optimizer.ema is None


# ------------------------------------------------------------------------------------------ 4. two gloo ranks
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _make_dp(seed_init, bucket_mb=0.05):
    from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model, resolve_config
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedAdam
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore, GradBucketer, backend
    from huggingface_sagemaker_tensorflow_distributed_amd.train.trainer import Trainer

    cfg = resolve_config("hsd-tiny-bert").replace(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model = build_model(cfg, seed=seed_init)
    store = FlatParamStore(model, CPU)
    opt = FusedAdam(store, lr=1e-3, weight_decay=0.01, ema_decay=0.9, ema_warmup=True)
    buck = GradBucketer(store, bucket_mb=bucket_mb) if backend.size() > 1 else None
    return model, store, opt, Trainer(model, store, opt, buck, CPU)


def _data(n, S=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(5, 1024, (n, S), generator=g)
    am = torch.ones(n, S, dtype=torch.long)
    am[::3, S // 2:] = 0
    lab = torch.randint(0, 2, (n,), generator=g)
    return ids, am, lab


def _worker_dp(rank, world, port, out_path):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "LOCAL_WORLD_SIZE": str(world), "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import backend
    from huggingface_sagemaker_tensorflow_distributed_amd.train.callbacks import BroadcastGlobalVariablesCallback

    backend.init(device="cpu")
    model, store, opt, tr = _make_dp(seed_init=100 + rank)  # the ranks start from different weights AND averages
    start = opt.ema.clone()
    BroadcastGlobalVariablesCallback(0).on_train_begin(tr)
    ids, am, lab = _data(4 * world)
    for step in range(3):
        sl = slice(rank * 4, (rank + 1) * 4)
        tr.train_step([{"input_ids": ids[sl], "attention_mask": am[sl], "labels": lab[sl]}])
    torch.save({"master": store.master.clone(), "ema": opt.ema.clone(), "start": start}, f"{out_path}.{rank}")
    backend.shutdown()


@pytest.mark.dist
def test_two_ranks_like_one_process_on_the_global_batch(tmp_path):
    """2 ranks x batch 4 == 1 process on the batch of 8 (the tolerance of test_lr_groups.py's two-rank test, which the
    average, a convex combination of those weights, inherits); the ranks agree bit for bit without a collective."""
    world = 2
    out = str(tmp_path / "dp.pt")
    mp.spawn(_worker_dp, args=(world, _port(), out), nprocs=world, join=True)
    r0, r1 = (torch.load(f"{out}.{r}") for r in range(world))
    assert not torch.equal(r0["start"], r1["start"])
    assert torch.equal(r0["master"], r1["master"]) and torch.equal(r0["ema"], r1["ema"])

    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE"):
        os.environ.pop(k, None)
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import backend

    backend.init(device="cpu")
    model, store, opt, tr = _make_dp(seed_init=100)
    ids, am, lab = _data(4 * world)
    for step in range(3):
        tr.train_step([{"input_ids": ids, "attention_mask": am, "labels": lab}])
    torch.testing.assert_close(store.master, r0["master"], atol=2e-6, rtol=1e-5)
    torch.testing.assert_close(opt.ema, r0["ema"], atol=2e-6, rtol=1e-5)
    assert not torch.equal(opt.ema, store.master)


# ------------------------------------------------------------------------------------------ 5. command line
def _build(extra):
    from huggingface_sagemaker_tensorflow_distributed_amd.train.runner import build
    from huggingface_sagemaker_tensorflow_distributed_amd.utils.args import build_parser

    args, _ = build_parser("train").parse_known_args(
        ["--model_name_or_path", "hsd-tiny-bert", "--train_batch_size", "16", "--log_every", "0", "--device", "cpu",
         "--seed", "7"] + extra)
    return build(args, "train")


@pytest.mark.parametrize("optimizer", ["adam", "adamw", "lamb"])
def test_flags_reach_the_optimizer(optimizer):
    opt = _build(["--optimizer", optimizer, "--ema_decay", "0.99", "--ema_warmup", "true"])["optimizer"]
    assert opt.ema_decay == 0.99 and opt.ema_warmup is True and torch.equal(opt.ema, opt.store.master)
    off = _build(["--optimizer", optimizer])["optimizer"]
    assert off.ema is None and off.ema_decay == 0.0 and off.ema_warmup is False


@pytest.mark.parametrize("extra", [["--ema_decay", "1"], ["--ema_decay", "-0.5"], ["--ema_decay", "nan"],
                                   ["--ema_decay", "inf"], ["--ema_warmup", "true"],
                                   ["--ema_decay", "0", "--ema_warmup", "true"]])
def test_bad_flags_are_refused_when_the_run_is_built(extra):
    with pytest.raises(ValueError, match="--ema_"):
        _build(extra)


def test_estimator_hyperparameters_carry_the_flags():
    from huggingface_sagemaker_tensorflow_distributed_amd.utils.args import build_parser, hyperparameters_to_argv

    argv = hyperparameters_to_argv({"ema_decay": 0.999, "ema_warmup": True})
    for mode in ("train", "single_node"):
        args, _ = build_parser(mode).parse_known_args(argv)
        assert args.ema_decay == 0.999 and args.ema_warmup is True
        args, _ = build_parser(mode).parse_known_args([])
        assert args.ema_decay == 0.0 and args.ema_warmup is False


def _run_train_script(tmp_path, extra):
    env = dict(os.environ, SM_OUTPUT_DATA_DIR=str(tmp_path / "data"), SM_MODEL_DIR=str(tmp_path / "model"),
               SM_NUM_GPUS="0", SM_FRAMEWORK_PARAMS="{}")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train.py"), "--model_name_or_path",
                        "hsd-tiny-bert", "--dataset", "synthetic", "--epochs", "1", "--train_batch_size", "4",
                        "--num_train_examples", "16", "--num_eval_examples", "8", "--eval_batch_size", "4",
                        "--max_seq_length", "16", "--log_every", "1", "--device", "cpu", "--learning_rate", "5e-3",
                        "--save_every_epoch", "true", "--seed", "3"] + extra,
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout + r.stderr, json.load(open(tmp_path / "data" / "run_provenance.json"))


def _safetensors(path):
    from huggingface_sagemaker_tensorflow_distributed_amd.train.callbacks import read_checkpoint

    return read_checkpoint(str(path))


def test_train_script_evaluates_and_saves_the_averaged_weights(tmp_path):
    log, info = _run_train_script(tmp_path / "on", ["--ema_decay", "0.5", "--ema_warmup", "true"])
    assert info["ema_decay"] == 0.5 and info["ema_warmup"] is True
    assert "--ema_decay 0.5 --ema_warmup true: the fused adam step keeps an fp32 average" in log
    final = _safetensors(tmp_path / "on" / "model")
    raw = _safetensors(tmp_path / "on" / "model" / "checkpoint-1")
    opt = torch.load(tmp_path / "on" / "model" / "checkpoint-1" / "optimizer.pt", map_location="cpu", weights_only=True)
    assert sorted(final) == sorted(raw) and opt["step"] == 4 and opt["ema_decay"] == 0.5
    # the same run with the flag off ends at the same raw weights: the step is undisturbed
    log_off, info_off = _run_train_script(tmp_path / "off", [])
    assert "ema_decay" not in info_off and "ema_warmup" not in info_off and "--ema_decay" not in log_off
    final_off = _safetensors(tmp_path / "off" / "model")
    opt_off = torch.load(tmp_path / "off" / "model" / "checkpoint-1" / "optimizer.pt", map_location="cpu",
                         weights_only=True)
    assert "ema" not in opt_off
    differ = 0
    for k in raw:
        assert torch.equal(raw[k], final_off[k]), k  # checkpoint-* holds the raw weights
        differ += int(not torch.equal(final[k], raw[k]))
    assert differ >= len(raw) // 2  # the saved model is the averaged one
    # ... and it is the average kept in optimizer.pt, laid out as the flat store
    from huggingface_sagemaker_tensorflow_distributed_amd.models import from_pretrained
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore

    store = FlatParamStore(from_pretrained(str(tmp_path / "on" / "model")), CPU)
    assert torch.equal(store.master, opt["ema"])
    # eval_results.txt keeps its format and holds the scores of the averaged weights
    on_txt = open(tmp_path / "on" / "data" / "eval_results.txt").read()
    off_txt = open(tmp_path / "off" / "data" / "eval_results.txt").read()
    assert [x.split("=")[0] for x in on_txt.splitlines()] == [x.split("=")[0] for x in off_txt.splitlines()]
    assert on_txt != off_txt


# ------------------------------------------------------------------------------------------ 6. learning
def test_tiny_bert_learns_the_marker_task_on_cpu_evaluated_on_the_average():
    """test_training.py's marker task (same data, 100 steps, learning rate 2e-3) with --ema_decay 0.99 --ema_warmup
    true: training is undisturbed, and the AVERAGED weights score the held-out marker data."""
    from huggingface_sagemaker_tensorflow_distributed_amd import data as hdata

    tr = _build(["--learning_rate", "2e-3", "--ema_decay", "0.99", "--ema_warmup", "true"])["trainer"]
    vocab = tr.model.cfg.vocab_size
    ds = hdata.synthetic_classification(16 * 100, 32, vocab, seed=1)
    held = hdata.synthetic_classification(64, 32, vocab, seed=2)  # the same marker tokens, other sentences

    def batch(d, i):
        sl = slice(16 * i, 16 * (i + 1))
        return {k: torch.from_numpy(v[sl]).long() for k, v in (
            ("input_ids", d.input_ids), ("attention_mask", d.attention_mask), ("labels", d.labels))}

    losses = [float(tr.train_step([batch(ds, i)]).detach()) for i in range(100)]
    assert sum(losses[:10]) / 10 > 0.5 and sum(losses[-20:]) / 20 < 0.2, losses[::10]
    held_out = [batch(held, i) for i in range(4)]
    avg = tr.evaluate(held_out, weights="ema")
    print("averaged weights:", avg, "raw weights:", tr.evaluate(held_out))
    assert math.isfinite(avg["loss"]) and avg["loss"] < 0.3 and avg["sparse_categorical_accuracy"] > 0.9, avg
    assert avg != tr.evaluate(held_out)
