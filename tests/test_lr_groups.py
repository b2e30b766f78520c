"""``--layerwise_lr_decay`` / ``--head_lr_multiplier`` (optim/groups.py, ``lr_multipliers=`` of FusedAdam / FusedLamb) on
the CPU tier: the depth map, the flags, the reference-path formulas against independent fp64 optimizers with one
parameter group per segment, checkpoints, two data-parallel ranks and the marker task."""
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


# ------------------------------------------------------------------------------------------ 1. depths and multipliers
# build_model's keys of --task sequence-classification | token-classification | question-answering | masked-lm
_TASKS = ("sequence-classification", "token-classification", "span-extraction", "masked-lm")


def _models():
    from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model, resolve_config

    for name in ("hsd-tiny-bert", "hsd-tiny-roberta", "hsd-tiny-distilbert"):
        cfg = resolve_config(name)
        for task in _TASKS:
            if task == "masked-lm" and cfg.model_type != "roberta":
                continue  # the MLM head is provided for roberta configs
            yield name, task, cfg, build_model(cfg, seed=0, task=task)


def test_every_parameter_has_one_depth_and_its_multiplier():
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import groups
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore

    D, M = 0.8, 4.0
    seen = 0
    for name, task, cfg, model in _models():
        L = cfg.num_hidden_layers
        store = FlatParamStore(model, CPU)
        mul = groups.lr_multipliers(store.names, L, D, M)
        assert sorted(mul) == sorted(store.names), (name, task)
        depths = {n: groups.param_depth(n, L) for n in store.names}
        assert set(depths.values()) == set(range(L + 2)), (name, task, depths)
        for n, d in depths.items():
            if n.startswith("encoder.embeddings."):
                assert d == 0 and mul[n] == D ** (L + 1), n
            elif n.startswith("encoder.layers."):
                i = int(n.split(".")[2])
                assert d == i + 1 and mul[n] == D ** (L - i), n
            else:
                assert not n.startswith("encoder."), n
                assert d == L + 1 and mul[n] == M, n
        assert max(v for n, v in mul.items() if depths[n] <= L) == D  # the top layer
        if task == "masked-lm":
            # the tied decoder is the word-embedding table: one parameter, one segment, depth 0
            assert sum(1 for n in store.names if "word_embeddings" in n) == 1
            assert not any("decoder" in n for n in store.names)
            assert depths["encoder.embeddings.word_embeddings"] == 0
            assert {n for n, d in depths.items() if d == L + 1} >= {"lm_bias"}
        rows = groups.depth_table(store.names, [s.numel for s in store.segments], L, D, M, 1e-3)
        assert [r[0] for r in rows] == list(range(L + 2))
        assert sum(r[4] for r in rows) == sum(s.numel for s in store.segments)
        assert rows[-1][2] == M and rows[-1][3] == pytest.approx(1e-3 * M)
        seen += 1
    assert seen == 3 * 3 + 1


def test_both_flags_at_one_is_off():
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import groups

    assert groups.lr_multipliers(["encoder.embeddings.x", "encoder.layers.0.y", "classifier_weight"], 2, 1.0, 1.0) is None
    assert groups.lr_multipliers(["classifier_weight"], 2, 1.0, 2.0) == {"classifier_weight": 2.0}
    with pytest.raises(ValueError, match="layer 5"):
        groups.param_depth("encoder.layers.5.qkv_weight", 2)
    # a decay whose power for the embeddings underflows fp32 is refused with the flag named (μ = 0 would freeze)
    with pytest.raises(ValueError, match="--layerwise_lr_decay"):
        groups.lr_multipliers(["encoder.embeddings.x", "classifier_weight"], 24, 0.01, 1.0)


@pytest.mark.parametrize("flag,value", [("--layerwise_lr_decay", "0"), ("--layerwise_lr_decay", "-0.5"),
                                        ("--layerwise_lr_decay", "1.5"), ("--layerwise_lr_decay", "nan"),
                                        ("--head_lr_multiplier", "0"), ("--head_lr_multiplier", "-1"),
                                        ("--head_lr_multiplier", "inf"), ("--head_lr_multiplier", "nan")])
def test_bad_flag_values_are_refused_with_the_flag_named(flag, value):
    with pytest.raises(ValueError, match=flag):
        _build([flag, value])


# ------------------------------------------------------------------------------------------ 2. the formulas
class _Toy(nn.Module):
    """Five parameters: an embedding, two layers' weights (one with a bias and a LayerNorm weight excluded from decay,
    flat_params._no_decay) and a head."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(0)
        self.emb_weight = nn.Parameter(torch.randn(9, 7, generator=g) * 0.3)
        self.dense_weight = nn.Parameter(torch.randn(7, 13, generator=g) * 0.3)
        self.dense_bias = nn.Parameter(torch.randn(13, generator=g) * 0.1)
        self.ln_weight = nn.Parameter(1.0 + torch.randn(13, generator=g) * 0.1)
        self.head_weight = nn.Parameter(torch.randn(70, generator=g) * 0.2)


_MU = {"emb_weight": 0.512, "dense_weight": 0.64, "dense_bias": 0.64, "ln_weight": 0.8, "head_weight": 4.0}


def _toy(cls_name, **kw):
    from huggingface_sagemaker_tensorflow_distributed_amd import optim
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore

    store = FlatParamStore(_Toy(), CPU)
    return store, getattr(optim, cls_name)(store, **kw)


def _fill(store, gen):
    store.grad.zero_()
    for s in store.segments:
        store.grad[s.offset:s.offset + s.numel] = torch.randn(s.numel, generator=gen)
    return store.grad.clone()


def _padding_is_zero(store, opt):
    keep = torch.zeros(store.numel, dtype=torch.bool)
    for s in store.segments:
        keep[s.offset:s.offset + s.numel] = True
    return all(int(torch.count_nonzero(buf[~keep])) == 0 for buf in (store.master, opt.exp_avg, opt.exp_avg_sq))


def test_cpu_fused_adamw_matches_torch_adamw_fp64_with_one_group_per_segment():
    lr, wd, gscale = 2e-3, 0.01, 0.5
    store, opt = _toy("FusedAdam", lr=lr, weight_decay=wd, eps_mode="torch", lr_multipliers=_MU)
    assert opt.lr_multipliers() == {n: float(torch.tensor(v, dtype=torch.float32)) for n, v in _MU.items()}
    params = [nn.Parameter(store.master[s.offset:s.offset + s.numel].double().clone()) for s in store.segments]
    ref = torch.optim.AdamW([{"params": [p], "lr": lr * _MU[s.name], "weight_decay": wd if s.decay else 0.0}
                             for p, s in zip(params, store.segments)], betas=(0.9, 0.999), eps=1e-8)
    g = torch.Generator().manual_seed(3)
    for _ in range(3):
        grad = _fill(store, g)
        opt.step(grad_scale=gscale)
        for p, s in zip(params, store.segments):
            p.grad = grad[s.offset:s.offset + s.numel].double() * gscale
        ref.step()
        for p, s in zip(params, store.segments):
            sl = slice(s.offset, s.offset + s.numel)
            st = ref.state[p]
            # tests/test_lamb.py's budget: fp32 against fp64, a handful of roundings (2^-24 each) per quantity per step
            # -- the multiplier adds one -- so 1e-5 relative, with floors at 1e-5 of each quantity's scale
            torch.testing.assert_close(store.master[sl].double(), p.detach(), rtol=1e-5, atol=1e-6)
            torch.testing.assert_close(opt.exp_avg[sl].double(), st["exp_avg"], rtol=1e-5, atol=1e-6)
            torch.testing.assert_close(opt.exp_avg_sq[sl].double(), st["exp_avg_sq"], rtol=1e-5, atol=1e-8)
    assert _padding_is_zero(store, opt)


def _lamb64(w, m, v, g, t, lr, b1, b2, eps, wd, adapt):
    """One LAMB step of ONE parameter in fp64 (tests/test_lamb.py's, written from the paper / TF Addons)."""
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    u = (m / (1 - b1 ** t)) / ((v / (1 - b2 ** t)).sqrt() + eps)
    r = 1.0
    if adapt:
        u = u + wd * w
        wn, un = float(w.norm()), float(u.norm())
        r = wn / un if wn > 0 and un > 0 else 1.0
    return w - lr * r * u, m, v, r


def test_cpu_fused_lamb_matches_a_per_parameter_fp64_lamb_with_its_own_rate():
    lr, wd, gscale = 2e-3, 0.01, 0.5
    store, opt = _toy("FusedLamb", lr=lr, weight_decay=wd, lr_multipliers=_MU)
    plain_store, plain = _toy("FusedLamb", lr=lr, weight_decay=wd)
    ref = {s.name: [store.master[s.offset:s.offset + s.numel].double().clone(), torch.zeros(s.numel).double(),
                    torch.zeros(s.numel).double()] for s in store.segments}
    g = torch.Generator().manual_seed(3)
    for t in (1, 2, 3):
        grad = _fill(store, g)
        if t == 1:  # the same state and gradient: the (r, Σw², Σu²) table does not depend on the multipliers
            plain_store.grad.copy_(grad)
            plain.step(grad_scale=gscale)
        opt.step(grad_scale=gscale)
        if t == 1:
            assert torch.equal(opt._ratio, plain._ratio)
            assert not torch.equal(store.master, plain_store.master)
        ratios = opt.trust_ratios()
        for s in store.segments:
            w, m, v = ref[s.name]
            w, m, v, r = _lamb64(w, m, v, grad[s.offset:s.offset + s.numel].double() * gscale, t, lr * _MU[s.name],
                                 0.9, 0.999, 1e-6, wd, s.decay)
            ref[s.name] = [w, m, v]
            sl = slice(s.offset, s.offset + s.numel)
            torch.testing.assert_close(store.master[sl].double(), w, rtol=1e-5, atol=1e-6)
            torch.testing.assert_close(opt.exp_avg[sl].double(), m, rtol=1e-5, atol=1e-6)
            torch.testing.assert_close(opt.exp_avg_sq[sl].double(), v, rtol=1e-5, atol=1e-8)
            assert ratios[s.name] == pytest.approx(r, rel=1e-5)
    assert _padding_is_zero(store, opt)


@pytest.mark.parametrize("cls_name", ["FusedAdam", "FusedLamb"])
def test_explicit_ones_equal_none_bit_for_bit(cls_name):
    st_a, a = _toy(cls_name, lr=1e-3, weight_decay=0.01, lr_multipliers={n: 1.0 for n in _MU})
    st_b, b = _toy(cls_name, lr=1e-3, weight_decay=0.01)
    st_c, c = _toy(cls_name, lr=1e-3, weight_decay=0.01, lr_multipliers=[1.0] * len(_MU))
    assert a.lr_multipliers() is None and c.lr_multipliers() is None and a._lr_mul is None  # off: no table
    assert "lr_multipliers" not in a.state_dict()
    g = torch.Generator().manual_seed(4)
    for _ in range(2):
        grad = _fill(st_a, g)
        st_b.grad.copy_(grad)
        st_c.grad.copy_(grad)
        for o in (a, b, c):
            o.step(grad_scale=0.5)
    for x, y in ((st_a.master, st_b.master), (a.exp_avg, b.exp_avg), (a.exp_avg_sq, b.exp_avg_sq),
                 (st_c.master, st_b.master)):
        assert torch.equal(x, y)


def test_multipliers_by_name_or_in_segment_order_and_their_errors():
    store, by_name = _toy("FusedAdam", lr=1e-3, lr_multipliers=_MU)
    _, in_order = _toy("FusedAdam", lr=1e-3, lr_multipliers=[_MU[n] for n in store.names])
    assert by_name.lr_multipliers() == in_order.lr_multipliers()
    table = store.block_table([_MU[n] for n in store.names])
    assert table.dtype == torch.float32 and table.numel() == store.numel // 64
    for s in store.segments:
        blocks = table[s.offset // 64:(s.offset + s.numel + 63) // 64]
        assert bool((blocks == torch.tensor(_MU[s.name], dtype=torch.float32)).all())
    used = sum((s.numel + 63) // 64 for s in store.segments)
    assert int((table == 1.0).sum()) == table.numel() - used  # the tail (and any padding block) holds 1
    with pytest.raises(ValueError, match="head_weight"):
        _toy("FusedAdam", lr_multipliers={n: v for n, v in _MU.items() if n != "head_weight"})
    with pytest.raises(ValueError, match="4 values for 5 segments"):
        _toy("FusedLamb", lr_multipliers=[1.0, 2.0, 3.0, 4.0])
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-60):  # 1e-60 rounds to 0 in fp32
        with pytest.raises(ValueError, match="finite and > 0"):
            _toy("FusedAdam", lr_multipliers=dict(_MU, emb_weight=bad))


@pytest.mark.parametrize("cls_name", ["FusedAdam", "FusedLamb"])
def test_with_clipping_norm_and_coefficient_do_not_depend_on_the_multipliers(cls_name):
    st_a, a = _toy(cls_name, lr=1e-3, weight_decay=0.01, max_grad_norm=0.5, lr_multipliers=_MU)
    st_b, b = _toy(cls_name, lr=1e-3, weight_decay=0.01, max_grad_norm=0.5)
    grad = _fill(st_a, torch.Generator().manual_seed(5))
    st_b.grad.copy_(grad)
    a.step(grad_scale=0.5)
    b.step(grad_scale=0.5)
    assert a.grad_norm() == b.grad_norm() > 0.5
    assert float(a.last_clip_coef) == float(b.last_clip_coef) < 1.0
    assert torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)  # the moments do not see μ
    assert not torch.equal(st_a.master, st_b.master)


# ------------------------------------------------------------------------------------------ 3. command line
def _build(extra):
    from huggingface_sagemaker_tensorflow_distributed_amd.train.runner import build
    from huggingface_sagemaker_tensorflow_distributed_amd.utils.args import build_parser

    args, _ = build_parser("train").parse_known_args(
        ["--model_name_or_path", "hsd-tiny-bert", "--train_batch_size", "16", "--log_every", "0", "--device", "cpu",
         "--seed", "7"] + extra)
    return build(args, "train")


@pytest.mark.parametrize("optimizer", ["adam", "adamw", "lamb"])
def test_flags_reach_the_optimizer(optimizer):
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import groups

    parts = _build(["--optimizer", optimizer, "--layerwise_lr_decay", "0.5", "--head_lr_multiplier", "4"])
    opt, store = parts["optimizer"], parts["store"]
    L = parts["model"].cfg.num_hidden_layers
    assert opt.lr_multipliers() == groups.lr_multipliers(store.names, L, 0.5, 4.0)  # powers of two: exact in fp32
    assert opt.lr_multipliers()["classifier_weight"] == 4.0
    assert opt.lr_multipliers()["encoder.embeddings.word_embeddings"] == 0.5 ** (L + 1)
    off = _build(["--optimizer", optimizer])["optimizer"]
    assert off.lr_multipliers() is None and off._lr_mul is None


def test_estimator_hyperparameters_carry_the_flags():
    from huggingface_sagemaker_tensorflow_distributed_amd.utils.args import build_parser, hyperparameters_to_argv

    argv = hyperparameters_to_argv({"layerwise_lr_decay": 0.8, "head_lr_multiplier": 4})
    for mode in ("train", "single_node"):
        args, _ = build_parser(mode).parse_known_args(argv)
        assert args.layerwise_lr_decay == 0.8 and args.head_lr_multiplier == 4.0
        args, _ = build_parser(mode).parse_known_args([])
        assert args.layerwise_lr_decay == 1.0 and args.head_lr_multiplier == 1.0


def _run_train_script(tmp_path, extra):
    env = dict(os.environ, SM_OUTPUT_DATA_DIR=str(tmp_path / "data"), SM_MODEL_DIR=str(tmp_path / "model"),
               SM_NUM_GPUS="0", SM_FRAMEWORK_PARAMS="{}")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train.py"), "--model_name_or_path",
                        "hsd-tiny-bert", "--dataset", "synthetic", "--max_steps", "2", "--epochs", "1",
                        "--train_batch_size", "4", "--num_train_examples", "8", "--num_eval_examples", "4",
                        "--max_seq_length", "16", "--log_every", "1", "--device", "cpu", "--do_eval", "False",
                        "--learning_rate", "1e-3"] + extra, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout + r.stderr, json.load(open(tmp_path / "data" / "run_provenance.json"))


def test_train_script_logs_the_table_and_writes_the_provenance(tmp_path):
    log, info = _run_train_script(tmp_path / "on", ["--layerwise_lr_decay", "0.8", "--head_lr_multiplier", "4"])
    assert info["layerwise_lr_decay"] == 0.8 and info["head_lr_multiplier"] == 4.0
    assert "--layerwise_lr_decay 0.8 --head_lr_multiplier 4: learning rate per depth" in log
    rows = {x.split()[0]: x.split() for x in log.splitlines() if x.split() and x.split()[0] in "0123"
            and len(x.split()) in (5, 6)}
    # depth, what, multiplier, learning rate (one process: world size 1), parameters
    assert rows["0"][1] == "embeddings" and float(rows["0"][2]) == pytest.approx(0.512)
    assert float(rows["0"][3]) == pytest.approx(0.512e-3)
    assert rows["2"][1:3] == ["layer", "1"] and float(rows["2"][3]) == pytest.approx(0.8)
    assert rows["3"][1] == "head" and float(rows["3"][2]) == 4.0 and float(rows["3"][3]) == pytest.approx(4e-3)
    assert int(rows["3"][4].replace(",", "")) == 64 * 64 + 64 + 2 * 64 + 2  # pooler + classifier
    log, info = _run_train_script(tmp_path / "off", [])
    assert "layerwise_lr_decay" not in info and "head_lr_multiplier" not in info
    assert "learning rate per depth" not in log


# ------------------------------------------------------------------------------------------ 4. checkpoints
def _trainer(seed=0, lamb=False, decay=0.8, head=4.0):
    from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model, resolve_config
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedAdam, FusedLamb, groups
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore
    from huggingface_sagemaker_tensorflow_distributed_amd.train.trainer import Trainer

    cfg = resolve_config("hsd-tiny-bert").replace(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    model = build_model(cfg, seed=seed)
    model.rng.base_seed = 7
    store = FlatParamStore(model, CPU)
    mul = groups.lr_multipliers(store.names, cfg.num_hidden_layers, decay, head)
    opt = (FusedLamb if lamb else FusedAdam)(store, lr=1e-3, weight_decay=0.01, lr_multipliers=mul)
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


@pytest.mark.parametrize("lamb", [False, True])
def test_checkpoint_resume_with_the_flags_equals_uninterrupted_bit_for_bit(tmp_path, lamb, caplog):
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
    assert sd["lr_multipliers"] == a.optimizer.lr_multipliers() and sd["step"] == 2
    b = _trainer(seed=123, lamb=lamb)  # different init: everything must come from the checkpoint
    with caplog.at_level(logging.WARNING, logger=PKG):
        st = load_checkpoint(ck, b)
    assert not [r for r in caplog.records if "lr_multiplier" in r.getMessage()]  # the same flags: no warning
    assert st["epoch"] == 1 and b.global_step == 2 and b.optimizer.step_count == 2
    for x in data[2:]:
        b.train_step([x])
    assert torch.equal(b.store.master, ref.store.master)
    assert torch.equal(b.optimizer.exp_avg, ref.optimizer.exp_avg)
    assert torch.equal(b.optimizer.exp_avg_sq, ref.optimizer.exp_avg_sq)


def test_resuming_with_different_flags_warns_and_the_current_flags_win(tmp_path, caplog):
    from huggingface_sagemaker_tensorflow_distributed_amd.train.callbacks import load_checkpoint, save_checkpoint

    a = _trainer()
    a.train_step(_batches(1))
    ck = str(tmp_path / "checkpoint-1")
    save_checkpoint(ck, a, epoch=1)
    for kw in ({"decay": 0.5}, {"decay": 1.0, "head": 1.0}):
        other = _trainer(**kw)
        want = other.optimizer.lr_multipliers()
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger=PKG):
            load_checkpoint(ck, other)
        msgs = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
        assert any("--layerwise_lr_decay" in m and "win" in m for m in msgs), msgs
        assert other.optimizer.lr_multipliers() == want
    # a checkpoint written with the flags off, resumed with them on
    off = _trainer(decay=1.0, head=1.0)
    off.train_step(_batches(1))
    assert "lr_multipliers" not in off.optimizer.state_dict()
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger=PKG):
        a.optimizer.load_state_dict(off.optimizer.state_dict())
    assert any("--layerwise_lr_decay" in r.getMessage() for r in caplog.records)


# ------------------------------------------------------------------------------------------ 5. two gloo ranks
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _make_dp(seed_init, bucket_mb=0.05):
    from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model, resolve_config
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedAdam, groups
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore, GradBucketer, backend
    from huggingface_sagemaker_tensorflow_distributed_amd.train.trainer import Trainer

    cfg = resolve_config("hsd-tiny-bert").replace(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model = build_model(cfg, seed=seed_init)
    store = FlatParamStore(model, CPU)
    opt = FusedAdam(store, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0,
                    lr_multipliers=groups.lr_multipliers(store.names, cfg.num_hidden_layers, 0.8, 4.0))
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
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import backend, broadcast_parameters

    backend.init(device="cpu")
    model, store, opt, tr = _make_dp(seed_init=100 + rank)
    broadcast_parameters(store)
    ids, am, lab = _data(4 * world)
    for step in range(3):
        sl = slice(rank * 4, (rank + 1) * 4)
        tr.train_step([{"input_ids": ids[sl], "attention_mask": am[sl], "labels": lab[sl]}])
    torch.save({"master": store.master.clone()}, f"{out_path}.{rank}")
    backend.shutdown()


@pytest.mark.dist
def test_two_ranks_with_multipliers_like_one_process_on_the_global_batch(tmp_path):
    """2 ranks x batch 4 == 1 process on the batch of 8, AdamW with clipping and per-layer rates (the tolerance of
    test_lamb.py::test_two_ranks_lamb_like_one_process_on_the_global_batch)."""
    world = 2
    out = str(tmp_path / "dp.pt")
    mp.spawn(_worker_dp, args=(world, _port(), out), nprocs=world, join=True)
    r0, r1 = (torch.load(f"{out}.{r}") for r in range(world))
    assert torch.equal(r0["master"], r1["master"])

    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE"):
        os.environ.pop(k, None)
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import backend

    backend.init(device="cpu")
    model, store, opt, tr = _make_dp(seed_init=100)
    before = store.master.clone()
    ids, am, lab = _data(4 * world)
    for step in range(3):
        tr.train_step([{"input_ids": ids, "attention_mask": am, "labels": lab}])
    torch.testing.assert_close(store.master, r0["master"], atol=2e-6, rtol=1e-5)
    # the rates are visible: three Adam steps move a head weight ~ 4 / 0.512 times as far as an embedding row in use
    seg = {s.name: s for s in store.segments}
    moved = (store.master - before).abs()
    head = float(moved[seg["classifier_weight"].offset:][:seg["classifier_weight"].numel].max())
    emb = seg["encoder.embeddings.position_embeddings"]
    assert head > 4.0 * float(moved[emb.offset:emb.offset + emb.numel].max())


# ------------------------------------------------------------------------------------------ 6. learning
def test_tiny_bert_learns_the_marker_task_on_cpu_with_layerwise_decay():
    """test_training.py::test_tiny_bert_learns_the_marker_task_on_cpu with --layerwise_lr_decay 0.8: same data, same 100
    steps, same learning rate, the bar test_lamb.py's learning test asks for."""
    from huggingface_sagemaker_tensorflow_distributed_amd import data as hdata

    tr = _build(["--learning_rate", "2e-3", "--layerwise_lr_decay", "0.8"])["trainer"]
    assert tr.optimizer.lr_multipliers() is not None
    vocab = tr.model.cfg.vocab_size
    ds = hdata.synthetic_classification(16 * 100, 32, vocab, seed=1)
    losses = []
    for i in range(100):
        sl = slice(16 * i, 16 * (i + 1))
        losses.append(float(tr.train_step([{k: torch.from_numpy(v[sl]).long() for k, v in (
            ("input_ids", ds.input_ids), ("attention_mask", ds.attention_mask), ("labels", ds.labels))}]).detach()))
    assert sum(losses[:10]) / 10 > 0.5 and sum(losses[-20:]) / 20 < 0.2, losses[::10]
    assert math.isfinite(losses[-1])
