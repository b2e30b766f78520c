"""Per-call cost of the head-dim-32 attention kernels (csrc/kernels/attention_d32.hip) at MiniLM-L12 shape, with the
d = 64 kernels at the same B and S and half the heads (the same bytes and the same MFMA count) as yardstick, in one
process. Kernel times come from the profiler, not from this script:

    rocprofv3 --kernel-trace --stats --output-format csv -d out/attn_d32_prof -o run -- \
        python tools/attn_d32_percall.py

The script prints the bytes each d = 32 kernel has to move (from the shapes) and a device-event time per forward +
backward pair as a cross-check."""
import os
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from huggingface_sagemaker_tensorflow_distributed_amd.ops import hip  # noqa: E402

B, S, P, CALLS, WARM = 256, 128, 0.1, 25, 5


def pairs(heads, d):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(heads)
    qkv = torch.randn(B * S, 3 * heads * d, generator=g).to(dev).bfloat16().requires_grad_()
    dout = torch.randn(B * S, heads * d, generator=g).to(dev).bfloat16()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for i in range(WARM + CALLS):
        if i == WARM:
            ev[0].record()
        (hip.attention_d32 if d == 32 else hip.attention)(qkv, None, B, S, heads, P, 7).backward(dout)
        qkv.grad = None
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / CALLS


if __name__ == "__main__":
    rows, H, heads = B * S, 384, 12
    qkv_b, out_b, lse_b = rows * 3 * H * 2, rows * H * 2, B * heads * S * 4
    print(f"shape B={B} S={S} p={P}: d=32 x {heads} heads vs d=64 x {heads // 2} heads, {WARM}+{CALLS} calls each")
    print(f"bytes per call (d=32): fwd {qkv_b + out_b + lse_b}, bwd_kv {qkv_b + 2 * out_b + lse_b + 2 * out_b}, "
          f"bwd_q {qkv_b + 2 * out_b + lse_b + out_b}")
    print(f"event time per fwd+bwd pair: d=32 {pairs(12, 32):.4f} ms, d=64 {pairs(6, 64):.4f} ms")
