"""Per-call cost of the fp32 variable-length attention kernels (csrc/kernels/attention32m_varlen.hip) against the dense
fp32 kernels (attention32m.hip) on equal work: 8 sequences of 512 tokens, all full length, 16 heads, p = 0.1, in one
process. Kernel times come from the profiler, not from this script:

    rocprofv3 --kernel-trace --stats --output-format csv -d out/attn32m_varlen_prof -o run -- \
        python tools/attn32m_varlen_percall.py

The script prints a device-event time per forward + backward pair (split2 passes included) as a cross-check."""
import os
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from huggingface_sagemaker_tensorflow_distributed_amd.ops import hip32  # noqa: E402

B, S, HEADS, P, CALLS, WARM = 8, 512, 16, 0.1, 25, 5


def pairs(varlen):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(1)
    qkv = torch.randn(B * S, 3 * HEADS * 64, generator=g).to(dev).requires_grad_()
    dout = torch.randn(B * S, HEADS * 64, generator=g).to(dev)
    cu = torch.arange(0, (B + 1) * S, S, dtype=torch.int32, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for i in range(WARM + CALLS):
        if i == WARM:
            ev[0].record()
        out = hip32.attention_varlen(qkv, cu, S, HEADS, P, 7) if varlen else hip32.attention(qkv, None, B, S, HEADS, P, 7)
        out.backward(dout)
        qkv.grad = None
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / CALLS


if __name__ == "__main__":
    print(f"shape B={B} S={S} heads={HEADS} p={P}, {WARM}+{CALLS} calls each")
    print(f"event time per fwd+bwd pair: dense {pairs(False):.4f} ms, varlen {pairs(True):.4f} ms")
