"""Per-call cost of the relative-position-bias attention kernels (csrc/kernels/attention_relbias.hip) against the varlen
kernels (attention_varlen.hip: the same grid and tiling without the bias) on equal work, packed batches of full-length
sequences, p = 0.1, in one process. Kernel times come from the profiler, not from this script:

    rocprofv3 --kernel-trace --stats --output-format csv -d out/attn_relbias_prof -o run -- \
        python tools/attn_relbias_percall.py B S HEADS

The script prints a device-event time per forward + backward pair as a cross-check."""
import os
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from huggingface_sagemaker_tensorflow_distributed_amd.ops import hip  # noqa: E402

P, CALLS, WARM = 0.1, 25, 5


def pairs(B, S, heads, bias):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(1)
    qkv = torch.randn(B * S, 3 * heads * 64, generator=g).to(dev).bfloat16().requires_grad_()
    dout = torch.randn(B * S, heads * 64, generator=g).to(dev).bfloat16()
    rel = torch.randn(heads, 2 * S - 1, generator=g).to(dev).requires_grad_()
    cu = torch.arange(0, (B + 1) * S, S, dtype=torch.int32, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for i in range(WARM + CALLS):
        if i == WARM:
            ev[0].record()
        out = (hip.attention_relbias_varlen(qkv, rel, cu, S, heads, P, 7) if bias
               else hip.attention_varlen(qkv, cu, S, heads, P, 7))
        out.backward(dout)
        qkv.grad = rel.grad = None
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / CALLS


if __name__ == "__main__":
    B, S, heads = (int(a) for a in sys.argv[1:4])
    print(f"shape B={B} S={S} heads={heads} p={P}, {WARM}+{CALLS} calls each")
    print(f"event time per fwd+bwd pair: varlen {pairs(B, S, heads, False):.4f} ms, "
          f"relbias {pairs(B, S, heads, True):.4f} ms")
