"""Learning curve of --task token-classification on the synthetic tagging corpus (data/datasets.py
synthetic_token_classification): bert-base width, 2 layers, L = 9, S = 128, B = 256, bf16 on one GPU with the fused head,
FusedAdam at a constant learning rate. Writes one JSON line per 10 steps (training loss / token accuracy of the batch)
and per 50 steps (held-out loss / token accuracy over 2,048 examples).

    python tools/token_cls_convergence.py OUT.jsonl VOCAB_SIZE STEPS LR      # profiles/token_cls: 256 600 3e-4
    python tools/token_cls_convergence.py OUT.jsonl VOCAB_SIZE STEPS LR EPS  # + --label_smoothing_factor EPS (default 0):
                                                                             # training and held-out loss are the smoothed one
"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from huggingface_sagemaker_tensorflow_distributed_amd import data as hdata
from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model, resolve_config
from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedAdam
from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore
out = sys.argv[1]
dev = torch.device("cuda", 0)
L, S, B = 9, 128, 256
V, STEPS, LR = int(sys.argv[2]), int(sys.argv[3]), float(sys.argv[4])
EPS = float(sys.argv[5]) if len(sys.argv) > 5 else 0.0
cfg = resolve_config("bert-base-uncased", num_labels=L).replace(num_hidden_layers=2, vocab_size=V)
model = build_model(cfg, task="token-classification", seed=0).to(dev)
model.label_smoothing = EPS
store = FlatParamStore(model, dev, compute_dtype=torch.bfloat16)
opt = FusedAdam(store, lr=LR)
tr = hdata.synthetic_token_classification(B * STEPS, S, V, seed=0, num_labels=L)
te = hdata.synthetic_token_classification(2048, S, V, seed=1, num_labels=L)
t = lambda a: torch.from_numpy(np.asarray(a).astype(np.int64)).to(dev)
def evaluate():
    model.eval()
    tot = torch.zeros(4, dtype=torch.float64, device=dev)
    with torch.no_grad():
        for i in range(0, len(te), 256):
            sl = slice(i, i + 256)
            loss, _ = model(t(te.input_ids[sl]), attention_mask=t(te.attention_mask[sl]), labels=t(te.labels[sl]))
            tot += loss._hsd_stats.double()
    model.train()
    return float(tot[3] / tot[2]), float(tot[1] / tot[2])
with open(out, "w") as f:
    cfgline = {"config": {"model": "bert-base-uncased, 2 layers", "vocab_size": V, "num_labels": L, "seq_len": S, "batch": B,
                          "lr": LR, "optimizer": "FusedAdam", "dtype": "bf16", "head": "fused token_head.hip", "chance": 1.0 / L}}
    if EPS:
        cfgline["config"]["label_smoothing_factor"] = EPS
    f.write(json.dumps(cfgline) + "\n")
    model.train()
    for step in range(STEPS):
        if step % 50 == 0:
            el, ea = evaluate()
            f.write(json.dumps({"step": step, "eval_loss": el, "eval_token_accuracy": ea}) + "\n"); f.flush()
        sl = slice(B * step, B * (step + 1))
        model.rng.new_step(step)
        store.zero_grad()
        loss, _ = model(t(tr.input_ids[sl]), attention_mask=t(tr.attention_mask[sl]), labels=t(tr.labels[sl]))
        loss.backward()
        opt.step(grad_scale=1.0)
        if step % 10 == 0:
            s = loss._hsd_stats.tolist()
            f.write(json.dumps({"step": step, "train_loss": s[0], "train_token_accuracy": s[1] / max(s[2], 1.0)}) + "\n")
    el, ea = evaluate()
    f.write(json.dumps({"step": STEPS, "eval_loss": el, "eval_token_accuracy": ea}) + "\n")
print(f"learning curve: held-out loss {el:.4f}, token accuracy {ea:.4f} after {STEPS} steps (chance {1.0 / L:.3f})")
