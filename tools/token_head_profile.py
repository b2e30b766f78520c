"""The fused token-classification head at 131,072 x 768 rows, C = 9, p = 0.1, a quarter of the labels ignored:
5 warm-up + 20 timed forward + backward calls. Run it under the profiler for per-kernel times
(profiles/token_cls/head_kernel_stats.csv):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o head -- python tools/token_head_profile.py
"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from huggingface_sagemaker_tensorflow_distributed_amd import ops
dev = torch.device("cuda", 0)
R, H, C, p = 131072, 768, 9, 0.1
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
for i in range(5):
    step(i)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for i in range(20):
    step(i)
e1.record()
torch.cuda.synchronize()
print(f"token_head fwd+bwd at {R} x {H}, C={C}, p={p}: {e0.elapsed_time(e1) / 20 * 1e3:.1f} us per call pair (device events, 20 calls)")
