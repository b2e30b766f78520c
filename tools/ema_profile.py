"""The optimizer kernels with and without the weight average (--ema_decay), side by side, 5 warm-up + 20 timed calls
each, on the real flat store of a model (bf16 compute copy, fp32 gradients, decoupled weight decay 0.01):

  adam_kernel<false, true, 2, false, false, false, *>   one launch over the whole buffer
  lamb_stage2_kernel<true, false, false, *>             one workgroup per tile
                                                        (lamb_stage1 / lamb_ratio run too: they never see the average)

The form with ``ema`` and the one without are different template instantiations, so one kernel trace holds both under
their own names (profiles/ema/percall_<model>_kernel_stats.csv):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o percall_base -- \\
        python tools/ema_profile.py bert-base-uncased
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o percall_large -- \\
        python tools/ema_profile.py bert-large-uncased
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model, resolve_config
from huggingface_sagemaker_tensorflow_distributed_amd.ops import hip
from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedAdam, FusedLamb
from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore

name = sys.argv[1] if len(sys.argv) > 1 else "bert-base-uncased"
dev = torch.device("cuda", 0)
cfg = resolve_config(name)
store = FlatParamStore(build_model(cfg, seed=0).to(dev), dev, compute_dtype=torch.bfloat16)
adam = FusedAdam(store, lr=5e-5, weight_decay=0.01, ema_decay=0.999)
lamb = FusedLamb(store, lr=5e-5, weight_decay=0.01)
m, v, ema = adam.exp_avg, adam.exp_avg_sq, adam.ema
store.grad.normal_(0.0, 1e-3)
print(f"{name}: {store.numel:,} elements in {len(store.segments)} segments; the average is {ema.numel() * 4:,} B; "
      f"bytes per element Adam 30 -> 38 ({38 / 30:.3f}x), LAMB's two streaming stages 42 -> 50 ({50 / 42:.3f}x), its "
      f"weight update alone 14 -> 22", flush=True)


def timed(what, fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        fn()
    e1.record()
    torch.cuda.synchronize()
    print(f"{what}: {e0.elapsed_time(e1) / 20 * 1e3:.1f} us per call (device events, 20 calls)", flush=True)


def adam_call(avg):
    hip.adam_step(store.master, m, v, store.grad, store.compute, adam._decay_mask, 5e-5, 1e-7, 0.9, 0.999, 1.0,
                  5e-5 * 0.01, ema=avg, ema_omd=1.0 - 0.999)


def lamb_call(avg):
    hip.lamb_step(lamb._plan, 0, lamb._plan.nsegs, store.master, m, v, store.grad, store.compute, None, lamb._partials,
                  lamb._ratio, 5e-5, 1.0, 1.0, 1e-6, 0.9, 0.999, 1.0, 0.01, ema=avg, ema_omd=1.0 - 0.999)


for rounds in range(2):  # twice, so neither form is always the first in the run
    timed(f"adam_step {name} without ema", lambda: adam_call(None))
    timed(f"adam_step {name} with ema", lambda: adam_call(ema))
    timed(f"lamb_step (3 launches) {name} without ema", lambda: lamb_call(None))
    timed(f"lamb_step (3 launches) {name} with ema", lambda: lamb_call(ema))
