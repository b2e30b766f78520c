"""Global-norm gradient clipping (``FusedAdam(max_grad_norm=...)``, ``--max_grad_norm``) on the CPU tier: the
reference-path formula, data-parallel ranks agreeing on the coefficient, and the command-line interface."""
import json
import math
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _tiny(max_grad_norm=0.0, seed=0, lr=1e-3, weight_decay=0.0):
    from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model, resolve_config
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedAdam
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore

    cfg = resolve_config("hsd-tiny-bert").replace(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model = build_model(cfg, seed=seed)
    store = FlatParamStore(model, torch.device("cpu"))
    return model, store, FusedAdam(store, lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm)


# ------------------------------------------------------------------------------------------ 1. the CPU formula
@pytest.mark.parametrize("c_frac", [0.5, 2.0])  # C under the norm (clips) and over it (coef 1)
def test_cpu_fused_adam_clips_by_the_global_norm(c_frac):
    gscale = 1.0 / 3.0
    g = torch.Generator().manual_seed(1)
    _m, st0, _o = _tiny()
    grads = [torch.randn(st0.numel, generator=g) * s for s in (0.02, 0.5)]
    norm0 = float(grads[0].double().square().sum().sqrt()) * gscale
    c = c_frac * norm0
    _m1, st, opt = _tiny(max_grad_norm=c, weight_decay=0.01)
    _m2, st_ref, ref = _tiny(weight_decay=0.01)
    assert torch.equal(st.master, st_ref.master)
    coefs = []
    for grad in grads:
        st.grad.copy_(grad)
        opt.step(grad_scale=gscale)
        # by hand: tf.clip_by_global_norm on the averaged gradient, no epsilon
        norm = math.sqrt(float(grad.double().square().sum())) * gscale
        coef = c / norm if norm > c else 1.0
        assert opt.grad_norm() == pytest.approx(norm, rel=1e-6)
        assert float(opt.last_clip_coef) == pytest.approx(coef, rel=1e-6)
        # ... and an unclipped FusedAdam fed the pre-scaled gradient
        st_ref.grad.copy_(grad * coef)
        ref.step(grad_scale=gscale)
        # rtol 1e-6; the two sides round the gradient differently (g x (gscale x coef) against (g x coef) x gscale: a
        # few ulp), and each compared value is a SUM in which that difference can meet cancellation (theta - update,
        # b1 m + (1 - b1) g), so the absolute floor is 8 ulp (2^-21) of the term that carries it: the update (at
        # most ~lr per step), (1 - b1) |g| and (1 - b2) g^2
        gmax = float(grad.abs().max()) * gscale * coef
        torch.testing.assert_close(st.master, st_ref.master, rtol=1e-6, atol=2.0 ** -21 * opt.lr)
        torch.testing.assert_close(opt.exp_avg, ref.exp_avg, rtol=1e-6, atol=2.0 ** -21 * 0.1 * gmax)
        torch.testing.assert_close(opt.exp_avg_sq, ref.exp_avg_sq, rtol=1e-6, atol=2.0 ** -21 * 1e-3 * gmax * gmax)
        coefs.append(coef)
    # the first gradient clips only under the smaller C; the second has 25x its norm and clips under both
    assert (coefs[0] < 1.0) == (c_frac < 1.0) and coefs[1] < 1.0


def test_cpu_never_clipping_is_bit_identical_to_off_and_reports_the_norm():
    g = torch.Generator().manual_seed(2)
    _m, st_inf, opt_inf = _tiny(max_grad_norm=float("inf"))
    _m2, st_off, opt_off = _tiny()
    for _ in range(3):
        grad = torch.randn(st_off.numel, generator=g)
        for st, opt in ((st_inf, opt_inf), (st_off, opt_off)):
            st.grad.copy_(grad)
            opt.step(grad_scale=1.0 / 3.0)
        assert torch.equal(st_inf.master, st_off.master)
        assert torch.equal(opt_inf.exp_avg, opt_off.exp_avg) and torch.equal(opt_inf.exp_avg_sq, opt_off.exp_avg_sq)
        assert float(opt_inf.last_clip_coef) == 1.0
        want = float(grad.double().square().sum().sqrt()) * float(torch.tensor(1.0 / 3.0, dtype=torch.float32))
        assert opt_inf.grad_norm() == pytest.approx(want, rel=1e-6)
    assert opt_off.last_grad_norm is None
    with pytest.raises(RuntimeError):
        opt_off.grad_norm()


def test_edge_norms_and_arguments():
    _m, st, opt = _tiny(max_grad_norm=1.0)
    st.grad.zero_()
    st.grad[0] = float("inf")
    opt.step()
    assert opt.grad_norm() == float("inf") and float(opt.last_clip_coef) == 0.0  # an infinite norm gives 0
    st.grad.zero_()
    st.grad[0] = float("nan")
    opt.step()
    assert math.isnan(opt.grad_norm()) and float(opt.last_clip_coef) == 1.0  # NaN compares false: 1
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            _tiny(max_grad_norm=bad)


def test_distributed_optimizer_forwards_the_clip_interface():
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel.dist_optim import DistributedOptimizer

    _m, st, opt = _tiny(max_grad_norm=1.0)
    d = DistributedOptimizer(opt)
    st.grad.fill_(1.0)
    d.step()
    assert d.max_grad_norm == 1.0
    assert d.grad_norm() == pytest.approx(math.sqrt(st.numel), rel=1e-6)
    assert float(d.last_clip_coef) == pytest.approx(1.0 / math.sqrt(st.numel), rel=1e-6)


# ------------------------------------------------------------------------------------------ 2. two gloo ranks
CLIP_C = 0.05  # well under the first steps' gradient norm of this model (asserted: every step clips)


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _setenv(rank, world, port):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "LOCAL_WORLD_SIZE": str(world), "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})


def _make(seed_init, bucket_mb=0.05):
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import GradBucketer, backend
    from huggingface_sagemaker_tensorflow_distributed_amd.train.trainer import Trainer

    model, store, opt = _tiny(max_grad_norm=CLIP_C, seed=seed_init)
    buck = GradBucketer(store, bucket_mb=bucket_mb) if backend.size() > 1 else None
    return model, store, opt, Trainer(model, store, opt, buck, torch.device("cpu"))


def _data(n, S=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(5, 1024, (n, S), generator=g)
    am = torch.ones(n, S, dtype=torch.long)
    am[::3, S // 2:] = 0
    lab = torch.randint(0, 2, (n,), generator=g)
    return ids, am, lab


def _worker_dp(rank, world, port, out_path):
    _setenv(rank, world, port)
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import backend, broadcast_parameters

    backend.init(device="cpu")
    model, store, opt, tr = _make(seed_init=100 + rank)
    broadcast_parameters(store)
    ids, am, lab = _data(4 * world)
    coefs = []
    for step in range(3):
        sl = slice(rank * 4, (rank + 1) * 4)
        tr.train_step([{"input_ids": ids[sl], "attention_mask": am[sl], "labels": lab[sl]}])
        coefs.append((opt.grad_norm(), float(opt.last_clip_coef)))
    torch.save({"master": store.master.clone(), "coefs": coefs}, f"{out_path}.{rank}")
    backend.shutdown()


@pytest.mark.dist
def test_two_ranks_clip_like_one_process_on_the_global_batch(tmp_path):
    """2 ranks x batch 4 with clipping == 1 process on the batch of 8 with clipping (the tolerance of
    test_distributed.py::test_dp_equals_single_process_global_batch); both ranks hold the same coefficient bit for bit
    (the norm is taken over the all-reduced buffer: no collective of its own)."""
    world = 2
    out = str(tmp_path / "dp.pt")
    mp.spawn(_worker_dp, args=(world, _port(), out), nprocs=world, join=True)
    r0, r1 = (torch.load(f"{out}.{r}") for r in range(world))
    assert r0["coefs"] == r1["coefs"]
    assert all(c < 1.0 for _n, c in r0["coefs"]), r0["coefs"]
    assert torch.equal(r0["master"], r1["master"])

    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE"):
        os.environ.pop(k, None)
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import backend

    backend.init(device="cpu")
    model, store, opt, tr = _make(seed_init=100)
    ids, am, lab = _data(4 * world)
    for step in range(3):
        tr.train_step([{"input_ids": ids, "attention_mask": am, "labels": lab}])
        assert opt.grad_norm() == pytest.approx(r0["coefs"][step][0], rel=1e-4)
    torch.testing.assert_close(store.master, r0["master"], atol=2e-6, rtol=1e-5)


# ------------------------------------------------------------------------------------------ 3. command line
def test_max_grad_norm_flag_parses_and_reference_defaults_stand():
    from huggingface_sagemaker_tensorflow_distributed_amd.utils.args import build_parser

    for script in ("train", "single_node"):
        p = build_parser(script)
        assert p.parse_known_args([])[0].max_grad_norm == 0.0
        assert p.parse_known_args(["--max_grad_norm", "0"])[0].max_grad_norm == 0.0
        assert p.parse_known_args(["--max_grad_norm", "1.0"])[0].max_grad_norm == 1.0
        assert p.parse_known_args(["--max_grad_norm", "inf"])[0].max_grad_norm == float("inf")
        a = p.parse_known_args(["--max_grad_norm", "1.0"])[0]
        # the reference script's hyperparameters keep their defaults (scripts/train.py of the reference)
        assert (a.epochs, a.train_batch_size, a.eval_batch_size, a.learning_rate) == (3, 8, 4, 5e-5)
        assert a.do_train is True and a.do_eval is True


def _train_keys(path):
    return [line.split(" = ")[0] for line in open(path).read().splitlines() if " = " in line]


def test_train_script_logs_grad_norm_and_keeps_the_result_files(tmp_path):
    common = ["--model_name_or_path", "hsd-tiny-bert", "--epochs", "1", "--train_batch_size", "4",
              "--num_train_examples", "12", "--num_eval_examples", "4", "--max_seq_length", "16", "--max_steps", "3",
              "--benchmark", "True", "--warmup_steps", "0", "--log_every", "1", "--device", "cpu", "--do_eval", "False"]
    keys = {}
    for name, extra in (("clip", ["--max_grad_norm", "0.05"]), ("off", [])):
        env = dict(os.environ, SM_OUTPUT_DATA_DIR=str(tmp_path / name / "data"),
                   SM_MODEL_DIR=str(tmp_path / name / "model"), SM_NUM_GPUS="0", SM_FRAMEWORK_PARAMS="{}")
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE"):
            env.pop(k, None)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train.py"), *common, *extra], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        d = tmp_path / name / "data"
        lines = [json.loads(x) for x in (d / "metrics.jsonl").read_text().splitlines()]
        assert lines
        if name == "clip":
            assert all(math.isfinite(rec["grad_norm"]) and rec["grad_norm"] > 0 for rec in lines), lines
            assert " - grad_norm=" in r.stdout + r.stderr  # the trainer's log_every line
        else:
            assert all("grad_norm" not in rec for rec in lines)
            assert " - grad_norm=" not in r.stdout + r.stderr
        keys[name] = _train_keys(d / "train_results.txt")
    assert keys["clip"] == keys["off"] and "loss" in keys["off"]
