"""``--optimizer lamb`` (optim/lamb.py ``FusedLamb``) on the CPU tier: the reference-path formula against an independent
per-parameter fp64 LAMB, the command line, checkpoints, two data-parallel ranks and the marker task."""
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


# ------------------------------------------------------------------------------------------ 1. the formula
class _Toy(nn.Module):
    """Four parameters: two that take decay and the trust ratio (one of them all zero), a bias and a LayerNorm weight
    that are excluded from both (flat_params._no_decay)."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(0)
        self.dense_weight = nn.Parameter(torch.randn(7, 13, generator=g) * 0.3)
        self.dense_bias = nn.Parameter(torch.randn(13, generator=g) * 0.1)
        self.ln_weight = nn.Parameter(1.0 + torch.randn(13, generator=g) * 0.1)
        self.zero_weight = nn.Parameter(torch.zeros(5, 3))


def _toy(**kw):
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedLamb
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore

    store = FlatParamStore(_Toy(), CPU)
    return store, FusedLamb(store, **kw)


def _lamb64(w, m, v, g, t, lr, b1, b2, eps, wd, adapt):
    """One LAMB step of ONE parameter in fp64, written from the paper / TF Addons, independent of optim/lamb.py."""
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    u = (m / (1 - b1 ** t)) / ((v / (1 - b2 ** t)).sqrt() + eps)
    r = 1.0
    if adapt:
        u = u + wd * w
        wn, un = float(w.norm()), float(u.norm())
        r = wn / un if wn > 0 and un > 0 else 1.0
    return w - lr * r * u, m, v, r


def test_cpu_fused_lamb_matches_a_per_parameter_fp64_lamb():
    lr, wd, gscale = 2e-3, 0.01, 0.5
    store, opt = _toy(lr=lr, weight_decay=wd)
    assert opt.eps == 1e-6 and (opt.beta1, opt.beta2) == (0.9, 0.999)
    names = {s.name: i for i, s in enumerate(store.segments)}
    assert [store.segments[names[n]].decay for n in ("dense_weight", "dense_bias", "ln_weight", "zero_weight")] == \
        [True, False, False, True]
    ref = {s.name: [store.master[s.offset:s.offset + s.numel].double().clone(), torch.zeros(s.numel).double(),
                    torch.zeros(s.numel).double()] for s in store.segments}
    g = torch.Generator().manual_seed(3)
    for t in (1, 2, 3):
        store.grad.zero_()
        for s in store.segments:
            store.grad[s.offset:s.offset + s.numel] = torch.randn(s.numel, generator=g)
        grad = store.grad.clone()
        opt.step(grad_scale=gscale)
        ratios = opt.trust_ratios()
        for s in store.segments:
            w, m, v = ref[s.name]
            w, m, v, r = _lamb64(w, m, v, grad[s.offset:s.offset + s.numel].double() * gscale, t, lr, 0.9, 0.999,
                                 1e-6, wd, s.decay)
            ref[s.name] = [w, m, v]
            sl = slice(s.offset, s.offset + s.numel)
            # fp32 against fp64: a handful of roundings (2^-24 each) per quantity per step; 1e-5 relative leaves room
            # for the cancellation in b1 m + (1 - b1) g, and the floors are 1e-5 of each quantity's scale (|w| ~ 0.3
            # and lr r |u| ~ 1e-3 .. 1; |g| ~ 1; g^2 ~ 1)
            torch.testing.assert_close(store.master[sl].double(), w, rtol=1e-5, atol=1e-6)
            torch.testing.assert_close(opt.exp_avg[sl].double(), m, rtol=1e-5, atol=1e-6)
            torch.testing.assert_close(opt.exp_avg_sq[sl].double(), v, rtol=1e-5, atol=1e-8)
            assert ratios[s.name] == pytest.approx(r, rel=1e-5)
            if not s.decay:
                assert ratios[s.name] == 1.0  # excluded from layer adaptation
        if t == 1:
            assert ratios["zero_weight"] == 1.0  # ||w|| = 0
            assert ratios["dense_weight"] != 1.0
    assert torch.equal(opt.last_trust_ratios, opt._ratio[:, 0])
    # alignment padding between the segments stayed zero everywhere
    keep = torch.zeros(store.numel, dtype=torch.bool)
    for s in store.segments:
        keep[s.offset:s.offset + s.numel] = True
    for buf in (store.master, opt.exp_avg, opt.exp_avg_sq):
        assert int(torch.count_nonzero(buf[~keep])) == 0


def test_zero_gradient_zero_state_no_decay_moves_nothing():
    store, opt = _toy(lr=1e-2, weight_decay=0.0)
    before = store.master.clone()
    store.grad.zero_()
    opt.step()
    assert torch.equal(store.master, before)  # u = 0 everywhere
    assert all(r == 1.0 for r in opt.trust_ratios().values())  # ||u|| = 0
    assert int(torch.count_nonzero(opt.exp_avg)) == 0 and int(torch.count_nonzero(opt.exp_avg_sq)) == 0


def test_nan_norm_gives_ratio_one():
    store, opt = _toy(lr=1e-2)
    store.grad.zero_()
    seg = next(s for s in store.segments if s.name == "dense_weight")
    store.grad[seg.offset] = float("nan")
    opt.step()
    assert opt.trust_ratios()["dense_weight"] == 1.0  # a NaN norm compares false


def test_lamb_with_clipping_consumes_the_clipped_gradient():
    """max_grad_norm: LAMB fed coef x g (FusedAdam's norm and coefficient) equals LAMB fed the pre-scaled gradient."""
    g = torch.Generator().manual_seed(5)
    st_a, a = _toy(lr=1e-3, weight_decay=0.01, max_grad_norm=0.5)
    st_b, b = _toy(lr=1e-3, weight_decay=0.01)
    for _ in range(2):
        grad = torch.zeros(st_a.numel)
        for s in st_a.segments:
            grad[s.offset:s.offset + s.numel] = torch.randn(s.numel, generator=g)
        norm = float(grad.double().norm()) * 0.5
        assert norm > 0.5
        st_a.grad.copy_(grad)
        a.step(grad_scale=0.5)
        assert a.grad_norm() == pytest.approx(norm, rel=1e-6)
        assert float(a.last_clip_coef) == pytest.approx(0.5 / norm, rel=1e-6)
        st_b.grad.copy_(grad * (0.5 / norm))
        b.step(grad_scale=0.5)
        torch.testing.assert_close(st_a.master, st_b.master, rtol=1e-5, atol=1e-7)


# ------------------------------------------------------------------------------------------ 2. command line
def _build(extra):
    from huggingface_sagemaker_tensorflow_distributed_amd.train.runner import build
    from huggingface_sagemaker_tensorflow_distributed_amd.utils.args import build_parser

    args, _ = build_parser("train").parse_known_args(
        ["--model_name_or_path", "hsd-tiny-bert", "--train_batch_size", "16", "--log_every", "0", "--device", "cpu",
         "--seed", "7"] + extra)
    return build(args, "train")


def test_optimizer_lamb_flag_builds_a_fused_lamb():
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedAdam, FusedLamb

    opt = _build(["--optimizer", "lamb", "--weight_decay", "0.01", "--max_grad_norm", "1.0"])["optimizer"]
    assert isinstance(opt, FusedLamb) and isinstance(opt, FusedAdam)
    assert opt.eps == 1e-6 and opt.weight_decay == 0.01 and opt.max_grad_norm == 1.0
    assert _build(["--optimizer", "lamb"])["optimizer"].weight_decay == 0.0
    assert _build(["--optimizer", "lamb", "--adam_epsilon", "1e-8"])["optimizer"].eps == 1e-8
    adam = _build(["--optimizer", "adam"])["optimizer"]
    assert type(adam) is FusedAdam and adam.eps == 1e-7


def test_train_script_logs_trust_ratio_and_grad_norm(tmp_path):
    env = dict(os.environ, SM_OUTPUT_DATA_DIR=str(tmp_path / "data"), SM_MODEL_DIR=str(tmp_path / "model"),
               SM_NUM_GPUS="0", SM_FRAMEWORK_PARAMS="{}")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train.py"), "--model_name_or_path",
                        "hsd-tiny-bert", "--dataset", "synthetic", "--optimizer", "lamb", "--weight_decay", "0.01",
                        "--max_grad_norm", "1.0", "--max_steps", "3", "--epochs", "1", "--train_batch_size", "4",
                        "--num_train_examples", "12", "--num_eval_examples", "4", "--max_seq_length", "16",
                        "--log_every", "1", "--device", "cpu", "--do_eval", "False"], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [x for x in (r.stdout + r.stderr).splitlines() if " ms/step" in x]
    assert len(lines) == 3
    assert all(" - grad_norm=" in x and " - trust_ratio=" in x for x in lines), lines


# ------------------------------------------------------------------------------------------ 3. checkpoints
def _trainer(seed=0, lamb=True):
    from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model, resolve_config
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedAdam, FusedLamb
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore
    from huggingface_sagemaker_tensorflow_distributed_amd.train.trainer import Trainer

    cfg = resolve_config("hsd-tiny-bert").replace(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    model = build_model(cfg, seed=seed)
    model.rng.base_seed = 7
    store = FlatParamStore(model, CPU)
    opt = FusedLamb(store, lr=1e-3, weight_decay=0.01) if lamb else FusedAdam(store, lr=1e-3)
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


def test_lamb_checkpoint_resume_equals_uninterrupted(tmp_path):
    """test_training.py::test_checkpoint_resume_equals_uninterrupted with LAMB (same tolerances)."""
    from huggingface_sagemaker_tensorflow_distributed_amd.train.callbacks import load_checkpoint, save_checkpoint

    data = _batches(4)
    ref = _trainer()
    for b in data:
        ref.train_step([b])
    a = _trainer()
    for b in data[:2]:
        a.train_step([b])
    ck = str(tmp_path / "checkpoint-1")
    save_checkpoint(ck, a, epoch=1)
    sd = torch.load(os.path.join(ck, "optimizer.pt"), map_location="cpu", weights_only=True)
    assert sd["kind"] == "lamb" and sd["step"] == 2
    b = _trainer(seed=123)  # different init: everything must come from the checkpoint
    st = load_checkpoint(ck, b)
    assert st["epoch"] == 1 and b.global_step == 2 and b.optimizer.step_count == 2
    for x in data[2:]:
        b.train_step([x])
    torch.testing.assert_close(b.store.master, ref.store.master, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(b.optimizer.exp_avg_sq, ref.optimizer.exp_avg_sq, rtol=1e-5, atol=1e-9)
    # a LAMB state does not load into Adam; Adam's own state (no "kind") loads into Adam as before
    adam = _trainer(lamb=False)
    with pytest.raises(ValueError, match="lamb"):
        adam.optimizer.load_state_dict(sd)
    with pytest.raises(ValueError, match="lamb"):
        load_checkpoint(ck, adam)
    adam_sd = adam.optimizer.state_dict()
    assert "kind" not in adam_sd
    adam.optimizer.load_state_dict(adam_sd)


# ------------------------------------------------------------------------------------------ 4. two gloo ranks
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _make_dp(seed_init, bucket_mb=0.05):
    from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model, resolve_config
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedLamb
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore, GradBucketer, backend
    from huggingface_sagemaker_tensorflow_distributed_amd.train.trainer import Trainer

    cfg = resolve_config("hsd-tiny-bert").replace(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model = build_model(cfg, seed=seed_init)
    store = FlatParamStore(model, CPU)
    opt = FusedLamb(store, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
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
    ratios = []
    for step in range(3):
        sl = slice(rank * 4, (rank + 1) * 4)
        tr.train_step([{"input_ids": ids[sl], "attention_mask": am[sl], "labels": lab[sl]}])
        ratios.append(opt.last_trust_ratios.clone())
    torch.save({"master": store.master.clone(), "ratios": ratios}, f"{out_path}.{rank}")
    backend.shutdown()


@pytest.mark.dist
def test_two_ranks_lamb_like_one_process_on_the_global_batch(tmp_path):
    """2 ranks x batch 4 == 1 process on the batch of 8, LAMB with clipping and decay (the tolerance of
    test_grad_clip.py::test_two_ranks_clip_like_one_process_on_the_global_batch); both ranks hold the same trust ratios
    bit for bit (every rank takes its norms over the same all-reduced buffer: no collective of LAMB's own)."""
    world = 2
    out = str(tmp_path / "dp.pt")
    mp.spawn(_worker_dp, args=(world, _port(), out), nprocs=world, join=True)
    r0, r1 = (torch.load(f"{out}.{r}") for r in range(world))
    assert all(torch.equal(a, b) for a, b in zip(r0["ratios"], r1["ratios"]))
    assert torch.equal(r0["master"], r1["master"])
    assert any(float(r.min()) != 1.0 or float(r.max()) != 1.0 for r in r0["ratios"])

    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE"):
        os.environ.pop(k, None)
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import backend

    backend.init(device="cpu")
    model, store, opt, tr = _make_dp(seed_init=100)
    ids, am, lab = _data(4 * world)
    for step in range(3):
        tr.train_step([{"input_ids": ids, "attention_mask": am, "labels": lab}])
        torch.testing.assert_close(opt.last_trust_ratios, r0["ratios"][step], rtol=1e-4, atol=0)
    torch.testing.assert_close(store.master, r0["master"], atol=2e-6, rtol=1e-5)


# ------------------------------------------------------------------------------------------ 5. learning
def test_tiny_bert_learns_the_marker_task_on_cpu_with_lamb():
    """test_training.py::test_tiny_bert_learns_the_marker_task_on_cpu with --optimizer lamb: same data, same 100
    steps, same bar. Only the learning rate differs: LAMB moves every adapted parameter by lr x its own norm per step,
    so Adam's 2e-3 (0.2 % per step) cannot leave the initial plateau in 100 steps; 3e-2 is in LAMB's usual range."""
    from huggingface_sagemaker_tensorflow_distributed_amd import data as hdata

    tr = _build(["--optimizer", "lamb", "--weight_decay", "0.01", "--learning_rate", "3e-2"])["trainer"]
    vocab = tr.model.cfg.vocab_size
    ds = hdata.synthetic_classification(16 * 100, 32, vocab, seed=1)
    losses = []
    for i in range(100):
        sl = slice(16 * i, 16 * (i + 1))
        losses.append(float(tr.train_step([{k: torch.from_numpy(v[sl]).long() for k, v in (
            ("input_ids", ds.input_ids), ("attention_mask", ds.attention_mask), ("labels", ds.labels))}]).detach()))
    assert sum(losses[:10]) / 10 > 0.5 and sum(losses[-20:]) / 20 < 0.2, losses[::10]
    assert math.isfinite(losses[-1])
