"""The optimizer kernels with and without the learning-rate multiplier table, side by side, 5 warm-up + 20 timed calls
each, on the real flat store of a model (bf16 compute copy, fp32 gradients, decoupled weight decay 0.01):

  adam_kernel<false, true, 2, false, false, *>     one launch over the whole buffer; the table is fp32 [numel / 64]
  lamb_stage2_kernel<true, false, *>               one workgroup per tile; the table is fp32 [segments]
                                                   (lamb_stage1 / lamb_ratio run too: they never see the table)

The form with the table and the one without are different template instantiations, so one kernel trace holds both under
their own names (profiles/lr_groups/percall_<model>_kernel_stats.csv):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o percall_base -- \\
        python tools/lr_groups_profile.py bert-base-uncased
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o percall_large -- \\
        python tools/lr_groups_profile.py bert-large-uncased
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model, resolve_config
from huggingface_sagemaker_tensorflow_distributed_amd.ops import hip
from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedAdam, FusedLamb, groups
from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore

name = sys.argv[1] if len(sys.argv) > 1 else "bert-base-uncased"
dev = torch.device("cuda", 0)
cfg = resolve_config(name)
store = FlatParamStore(build_model(cfg, seed=0).to(dev), dev, compute_dtype=torch.bfloat16)
mul = groups.lr_multipliers(store.names, cfg.num_hidden_layers, 0.9, 4.0)
adam = FusedAdam(store, lr=5e-5, weight_decay=0.01, lr_multipliers=mul)
lamb = FusedLamb(store, lr=5e-5, weight_decay=0.01, lr_multipliers=mul)
m, v = adam.exp_avg, adam.exp_avg_sq
store.grad.normal_(0.0, 1e-3)
print(f"{name}: {store.numel:,} elements in {len(store.segments)} segments; Adam's table {adam._lr_mul.numel() * 4:,} B "
      f"({adam._lr_mul.numel() * 4 / (30 * store.numel):.3%} of 30 B per element), LAMB's {lamb._lr_mul.numel() * 4:,} B",
      flush=True)


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


def adam_call(table):
    hip.adam_step(store.master, m, v, store.grad, store.compute, adam._decay_mask, 5e-5, 1e-7, 0.9, 0.999, 1.0,
                  5e-5 * 0.01, lr_mul=table)


def lamb_call(table):
    hip.lamb_step(lamb._plan, 0, lamb._plan.nsegs, store.master, m, v, store.grad, store.compute, None, lamb._partials,
                  lamb._ratio, 5e-5, 1.0, 1.0, 1e-6, 0.9, 0.999, 1.0, 0.01, lr_mul=table)


for rounds in range(2):  # twice, so neither form is always the first in the run
    timed(f"adam_step {name} without the table", lambda: adam_call(None))
    timed(f"adam_step {name} with the table", lambda: adam_call(adam._lr_mul))
    timed(f"lamb_step (3 launches) {name} without the table", lambda: lamb_call(None))
    timed(f"lamb_step (3 launches) {name} with the table", lambda: lamb_call(lamb._lr_mul))
