"""The wide token-classification head (csrc/kernels/token_head_wide.hip) at 131,072 x 768 rows, p = 0.1, a quarter of
the labels ignored, C from the command line (default 45): 5 warm-up + 20 timed forward + backward calls, then the same
through the composed ops. Run it under the profiler for per-kernel times (profiles/token_head_wide/):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o head -- python tools/token_head_wide_profile.py 45
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from huggingface_sagemaker_tensorflow_distributed_amd import ops  # noqa: E402

dev = torch.device("cuda", 0)
R, H, p = 131072, 768, 0.1
C = int(sys.argv[1]) if len(sys.argv) > 1 else 45
g = torch.Generator().manual_seed(0)
h = torch.randn(R, H, generator=g).to(dev).bfloat16().requires_grad_()
w = (torch.randn(C, H, generator=g) * 0.05).to(dev).bfloat16().requires_grad_()
b = torch.zeros(C, device=dev, dtype=torch.bfloat16).requires_grad_()
labels = torch.randint(0, C, (R,), generator=g)
labels[torch.rand(R, generator=g) < 0.25] = -100
labels = labels.to(dev)


def step(i):
    loss, _ = ops.token_head(h, w, b, labels, p, 1234 + i)
    loss.backward()
    h.grad = None


for fused in (True, False):
    ops.TOKEN_HEAD_FUSED = fused
    for i in range(5):
        step(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(20):
        step(i)
    e1.record()
    torch.cuda.synchronize()
    print(f"token_head {'wide kernels' if fused else 'composed ops'} fwd+bwd at {R} x {H}, C={C}, p={p}: "
          f"{e0.elapsed_time(e1) / 20 * 1e3:.1f} us per call pair (device events, 20 calls)")
