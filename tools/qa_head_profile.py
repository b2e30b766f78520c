"""The fused question-answering head at 131,072 x 768 rows (341 sequences of 384 rows plus 128 dead rows, ragged real
lengths), p = 0.1, next to the token-classification head at the same rows and C = 2: 5 warm-up + 20 timed
forward + backward calls each. Run it under the profiler for per-kernel times (profiles/qa/head_kernel_stats.csv):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o head -- python tools/qa_head_profile.py
"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from huggingface_sagemaker_tensorflow_distributed_amd import ops
dev = torch.device("cuda", 0)
R, H, S, p = 131072, 768, 384, 0.1
B = R // S
g = torch.Generator().manual_seed(0)
h = torch.randn(R, H, generator=g).to(dev).bfloat16().requires_grad_()
w = (torch.randn(2, H, generator=g) * 0.05).to(dev).bfloat16().requires_grad_()
b = torch.zeros(2, device=dev, dtype=torch.bfloat16).requires_grad_()
lengths = torch.randint(S // 4, S + 1, (B,), generator=g)
cu = torch.cat([torch.arange(B, dtype=torch.int32) * S, torch.tensor([B * S], dtype=torch.int32)]).to(dev)
mask = torch.zeros(R, dtype=torch.long)
mask[:B * S] = (torch.arange(S)[None, :] < lengths[:, None]).long().reshape(-1)
mask = mask.to(dev)
start = (torch.rand(B, generator=g) * (lengths - 4)).long()
pos = torch.stack([start, start + 3], dim=1).to(dev)
tok_labels = torch.randint(0, 2, (R,), generator=g)
tok_labels[mask.cpu() == 0] = -100
tok_labels = tok_labels.to(dev)
def qa_step(i):
    loss, _ = ops.qa_head(h, w, b, pos, cu, mask, p, 1234 + i, 30, max_seqlen=S)
    loss.backward()
    h.grad = None
def tok_step(i):
    loss, _ = ops.token_head(h, w, b, tok_labels, p, 1234 + i)
    loss.backward()
    h.grad = None
for name, step in (("qa_head", qa_step), ("token_head C=2", tok_step)):
    for i in range(5):
        step(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(20):
        step(i)
    e1.record()
    torch.cuda.synchronize()
    print(f"{name} fwd+bwd at {R} x {H}, p={p}: {e0.elapsed_time(e1) / 20 * 1e3:.1f} us per call pair (device events, 20 calls)")
