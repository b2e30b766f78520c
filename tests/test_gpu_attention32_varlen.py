"""fp32 variable-length attention (csrc/kernels/attention32m_varlen.hip) and --pack_sequences true --dtype fp32 on the
GPU, vs ops/reference.py on the same inputs and seed (the dropout bits match). Three heads; T rounded up to 256.

* batch A: every edge of 32-row waves, 64-key tiles, 128-row blocks and the two-stage pipeline (1 .. 5 key tiles),
  174 dead rows;  * batch C: 64 short sequences;  * batch D: 1100 rows, beyond the dense fp32 kernel's 1024.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_varlen import _inputs, _packed_batches, _run, _tiny, _two_layer_bert_dir  # noqa: E402

from huggingface_sagemaker_tensorflow_distributed_amd import ops  # noqa: E402
from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model  # noqa: E402
from huggingface_sagemaker_tensorflow_distributed_amd.ops import reference as ref  # noqa: E402

HEADS, SEED = 3, 777
H = HEADS * 64
BATCHES = {"A": [1, 7, 32, 33, 64, 65, 127, 128, 129, 200, 320], "C": [(i % 5) + 1 for i in range(64)],
           "D": [1100, 5]}
_LAYOUTS = {}


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _layout(name, device):
    """The batch's offsets and its seeded fp32 inputs (made once, never modified)."""
    if name not in _LAYOUTS:
        lengths = BATCHES[name]
        cu = np.zeros(len(lengths) + 1, dtype=np.int32)
        cu[1:] = np.cumsum(lengths)
        T = -(-int(cu[-1]) // 256) * 256
        g = torch.Generator(device="cpu").manual_seed(11 + len(lengths))
        _LAYOUTS[name] = dict(cu_host=cu, cu=torch.from_numpy(cu).to(device), t_real=int(cu[-1]), T=T, B=len(lengths),
                              max_seqlen=max(lengths), qkv=torch.randn(T, 3 * H, generator=g).to(device),
                              dout=torch.randn(T, H, generator=g).to(device))
    return _LAYOUTS[name]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("name", ["A", "C", "D"])
def test_fp32_varlen_attention_matches_reference(gpu, name, p, monkeypatch):
    """ops.attention_varlen on fp32 GPU tensors runs the HIP kernels (the reference op is made to raise) and matches
    the reference at the bounds of test_gpu_fp32.py::test_attention32_fwd_bwd, on the whole tensor and on each
    sequence's own rows."""
    from huggingface_sagemaker_tensorflow_distributed_amd.ops import hip32

    c = _layout(name, gpu)
    b = c["qkv"].clone().requires_grad_()
    r = ref.attention_varlen(b, c["cu"], c["max_seqlen"], HEADS, p, SEED, p > 0)
    r.backward(c["dout"])
    C_, ran = hip32._C, []
    real = C_.attn32m_varlen_fwd
    monkeypatch.setattr(C_, "attn32m_varlen_fwd", lambda *a: (ran.append(1), real(*a))[1])
    monkeypatch.setattr(ref, "attention_varlen", lambda *a, **k: pytest.fail("the reference op ran on the GPU path"))
    a = c["qkv"].clone().requires_grad_()
    out = ops.attention_varlen(a, c["cu"], c["max_seqlen"], HEADS, p, SEED)
    out.backward(c["dout"])
    torch.cuda.synchronize()
    assert ran == [1]
    out, r = out.detach(), r.detach()
    eo, eg = _rel(out, r), _rel(a.grad, b.grad)
    print(f"{name} p={p}: out {eo:.3g} dqkv {eg:.3g}")
    assert eo < 2e-5 and eg < 2e-4
    cu = c["cu_host"]
    worst = [max((_rel(x[cu[i]:cu[i + 1]], y[cu[i]:cu[i + 1]]), i) for i in range(c["B"]))
             for x, y in ((out, r), (a.grad, b.grad))]
    print(f"{name} p={p}: worst sequence out {worst[0]} dqkv {worst[1]}")
    assert worst[0][0] < 2e-5 and worst[1][0] < 2e-4, worst


def test_fp32_varlen_kernels_write_every_row_and_zero_the_dead_rows(gpu):
    from huggingface_sagemaker_tensorflow_distributed_amd.ops import hip32 as h

    c, p = _layout("A", gpu), 0.1
    T, B, S = c["T"], c["B"], c["max_seqlen"]
    assert c["t_real"] < T
    out, lse, dqkv = (torch.full(s, float("nan"), device=gpu) for s in ((T, H), (HEADS * T,), (T, 3 * H)))
    (qh, ql), (dh, dl) = h._split2(c["qkv"]), h._split2(c["dout"])
    h._C.attn32m_varlen_fwd(qh, ql, c["cu"], out, lse, B, S, HEADS, p, SEED)
    h._C.attn32m_varlen_bwd(qh, ql, dh, dl, c["cu"], out, c["dout"], lse, dqkv, torch.empty_like(lse), B, S, HEADS, p,
                            SEED)
    torch.cuda.synchronize()
    for what, t in (("out", out), ("lse2", lse.view(HEADS, T).t()), ("dqkv", dqkv)):
        assert not torch.isnan(t).any(), f"{what}: a row was not written"
        assert torch.count_nonzero(t[c["t_real"]:]) == 0, f"{what}: a dead row is not zero"


@pytest.mark.parametrize("where", ["sequence", "dead"])
def test_fp32_varlen_sequences_do_not_see_each_other(gpu, where):
    """Noise on one interior sequence's rows, or on the dead rows: every other sequence's out and dqkv keep their
    bits, and the noisy sequence's change."""
    c = _layout("A", gpu)
    s0, s1 = (int(c["cu_host"][5]), int(c["cu_host"][6])) if where == "sequence" else (c["t_real"], c["T"])
    noisy = c["qkv"].clone()
    noisy[s0:s1] += torch.randn(s1 - s0, 3 * H, generator=torch.Generator(device="cpu").manual_seed(9)).to(gpu)
    res = []
    for qkv in (c["qkv"], noisy):
        a = qkv.clone().requires_grad_()
        out = ops.attention_varlen(a, c["cu"], c["max_seqlen"], HEADS, 0.1, SEED)
        out.backward(c["dout"])
        res.append((out.detach(), a.grad))
    (out0, d0), (out1, d1) = res
    keep = torch.ones(c["T"], dtype=torch.bool, device=gpu)
    keep[s0:s1] = False
    assert torch.equal(out0[keep], out1[keep]) and torch.equal(d0[keep], d1[keep])
    if where == "sequence":
        assert not torch.equal(out0[s0:s1], out1[s0:s1]) and not torch.equal(d0[s0:s1], d1[s0:s1])


def test_fp32_varlen_forward_and_backward_are_bit_identical_run_to_run(gpu):
    c = _layout("A", gpu)
    res = []
    for _ in range(2):
        a = c["qkv"].clone().requires_grad_()
        out = ops.attention_varlen(a, c["cu"], c["max_seqlen"], HEADS, 0.1, SEED)
        out.backward(c["dout"])
        res.append((out.detach(), a.grad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("name", ["hsd-tiny-bert", "hsd-tiny-roberta", "hsd-tiny-distilbert"])
def test_packed_fp32_model_hip_vs_packed_reference_with_dropout(gpu, name):
    """The packed fp32 step on the kernels against the same step on the reference ops, at the bounds of
    test_gpu_fp32.py::test_fp32_bert_step_on_kernels_matches_cpu."""
    cfg = _tiny(name, dropout=True)
    m = build_model(cfg, seed=0).to(gpu).train()
    _, packed = _inputs(cfg, gpu)
    (l1, _, g1), (l2, _, g2) = _run(m, packed, False), _run(m, packed, True)
    assert torch.isfinite(l1) and abs(float(l1) - float(l2)) <= 1e-4 * abs(float(l2)), (l1, l2)
    worst = max((_rel(g1[k], g2[k]), k) for k in g2 if g2[k].norm() > 0)
    assert worst[0] < 1e-3, worst


def test_runner_accepts_packed_fp32_and_still_refuses_fp8(gpu, tmp_path):
    from huggingface_sagemaker_tensorflow_distributed_amd import data as hdata
    from huggingface_sagemaker_tensorflow_distributed_amd.train.runner import build
    from huggingface_sagemaker_tensorflow_distributed_amd.utils.args import build_parser

    def parse(dtype):
        return build_parser("train").parse_known_args(
            ["--model_name_or_path", _two_layer_bert_dir(tmp_path), "--train_batch_size", "8", "--learning_rate",
             "1e-4", "--dtype", dtype, "--log_every", "0", "--seed", "7", "--pack_sequences", "true"])[0]

    parts = build(parse("fp32"), "train")
    tr = parts["trainer"]
    assert tr._seed is None and not tr._graph_replay  # packed steps stay eager
    ds = hdata.synthetic_classification(16, 128, 30522, seed=1)
    losses = [float(tr.train_step([mb]).detach()) for mb in _packed_batches(ds, 2, 8, parts["model"].cfg, gpu)]
    assert tr.global_step == 2 and all(np.isfinite(x) for x in losses), losses
    with pytest.raises(ValueError, match="fp8"):
        build(parse("fp8"), "train")
