"""The CE kernels with and without label smoothing, side by side, 5 warm-up + 20 timed calls each:

  xent_kernel<true, *>                     5,248 x 50,432 bf16 logits, 50,265 real classes (the dynamic MLM head's shape)
  tok_fwd_kernel<*> / tok_bwd_kernel<false, *>   131,072 x 768 rows, C = 9, p = 0.1, a quarter of the labels ignored
  seq_fwd_kernel<*> / seq_bwd_kernel<*>     B = 1,024, H = 768, C = 2 (eps = 0 through hip.seq_head: ops.cls_head would
                                            send that head to cls_head.hip, which is timed as well)

The smoothed and the plain form are different template instantiations, so one kernel trace holds both under their own
names (profiles/label_smoothing/percall_kernel_stats.csv):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o percall -- python tools/label_smoothing_profile.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from huggingface_sagemaker_tensorflow_distributed_amd import ops
from huggingface_sagemaker_tensorflow_distributed_amd.ops import hip

dev = torch.device("cuda", 0)
EPS = 0.1
g = torch.Generator().manual_seed(0)


def timed(name, fn):
    for i in range(5):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(20):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    print(f"{name}: {e0.elapsed_time(e1) / 20 * 1e3:.1f} us per call (device events, 20 calls)", flush=True)


# xent
R, V, Vp = 5248, 50265, 50432
logits = (torch.randn(R, Vp, device=dev) * 2).bfloat16()
tgt = torch.randint(0, V, (R,), device=dev)
tgt[4800:] = -100  # the unused capacity rows
n_valid = tgt.ne(-100).sum().float().reshape(1)
dlogits = torch.empty_like(logits)
stats = torch.zeros(2, device=dev)
for eps in (0.0, EPS):
    timed(f"xent {R} x {Vp} bf16, V = {V}, eps = {eps}", lambda i: hip._C.xent(logits, tgt, dlogits, stats, n_valid, V, eps))
del logits, dlogits

# token head
R, H, C, p = 131072, 768, 9, 0.1
h = torch.randn(R, H, generator=g).to(dev).bfloat16().requires_grad_()
w = (torch.randn(C, H, generator=g) * 0.05).to(dev).bfloat16().requires_grad_()
b = torch.zeros(C, device=dev, dtype=torch.bfloat16).requires_grad_()
labels = torch.randint(0, C, (R,), generator=g)
labels[torch.rand(R, generator=g) < 0.25] = -100
labels = labels.to(dev)


def tok(i, eps):
    loss, _ = ops.token_head(h, w, b, labels, p, 1234 + i, label_smoothing=eps)
    loss.backward()
    h.grad = None


for eps in (0.0, EPS):
    timed(f"token_head fwd+bwd {R} x {H}, C = {C}, eps = {eps}", lambda i: tok(i, eps))
del h

# sequence head
B, S, H, C = 1024, 1, 768, 2
hs = torch.randn(B, S, H, generator=g).to(dev).bfloat16().requires_grad_()
mk = lambda *s, sc: (torch.randn(*s, generator=g) * sc).to(dev).bfloat16().requires_grad_()  # noqa: E731
w1, b1, w2, b2 = mk(H, H, sc=H ** -0.5), mk(H, sc=0.5), mk(C, H, sc=H ** -0.5), mk(C, sc=0.5)
lab = torch.randint(0, C, (B,), generator=g).to(dev)


def seq(i, fn, **kw):
    loss = fn(hs, w1, b1, w2, b2, lab, "tanh", 0.0, 0, 0.1, 77 + i, **kw)[0]
    loss.backward()
    hs.grad = None


timed(f"seq_head.hip fwd+bwd B = {B}, H = {H}, C = {C}, eps = 0.0", lambda i: seq(i, hip.seq_head))
timed(f"seq_head.hip fwd+bwd B = {B}, H = {H}, C = {C}, eps = {EPS}", lambda i: seq(i, ops.cls_head, label_smoothing=EPS))
timed(f"cls_head.hip fwd+bwd B = {B}, H = {H}, C = {C} (eps = 0 dispatch)", lambda i: seq(i, ops.cls_head))
