"""Learning curve of --task question-answering on the synthetic span corpus (data/datasets.py
synthetic_question_answering): bert-base width, 2 layers, segment ids, S = 128, B = 256, bf16 on one GPU with the fused
head, FusedAdam at a constant learning rate. Writes one JSON line per 10 steps (training loss / exact match of the
batch) and per 50 steps (held-out loss / exact match over 2,048 examples).

    python tools/qa_convergence.py OUT.jsonl VOCAB_SIZE STEPS LR      # profiles/qa: 256 600 3e-4
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
S, B = 128, 256
V, STEPS, LR = int(sys.argv[2]), int(sys.argv[3]), float(sys.argv[4])
cfg = resolve_config("bert-base-uncased").replace(num_hidden_layers=2, vocab_size=V)
model = build_model(cfg, task="span-extraction", seed=0).to(dev)
store = FlatParamStore(model, dev, compute_dtype=torch.bfloat16)
opt = FusedAdam(store, lr=LR)
kw = dict(cls_id=1, sep_id=2) if V <= 102 else {}
tr = hdata.synthetic_question_answering(B * STEPS, S, V, seed=0, **kw)
te = hdata.synthetic_question_answering(2048, S, V, seed=1, **kw)
t = lambda a: torch.from_numpy(np.asarray(a).astype(np.int64)).to(dev)
def run(ds, sl):
    return model(t(ds.input_ids[sl]), attention_mask=t(ds.attention_mask[sl]), token_type_ids=t(ds.token_type_ids[sl]),
                 labels=t(ds.labels[sl]))
def evaluate():
    model.eval()
    tot = torch.zeros(8, dtype=torch.float64, device=dev)
    with torch.no_grad():
        for i in range(0, len(te), 256):
            loss, _ = run(te, slice(i, i + 256))
            tot += loss._hsd_stats.double()
    model.train()
    return float(tot[3] / tot[2]), float(tot[1] / tot[2])
none = float((te.labels == 0).all(axis=1).mean())
with open(out, "w") as f:
    cfgline = {"config": {"model": "bert-base-uncased, 2 layers", "vocab_size": V, "seq_len": S, "batch": B, "lr": LR,
                          "optimizer": "FusedAdam", "dtype": "bf16", "head": "fused qa_head.hip", "max_answer_length": 30,
                          "chance": "always (0, 0) scores the no-answer share, %.3f; a random span under 0.001" % none}}
    f.write(json.dumps(cfgline) + "\n")
    model.train()
    for step in range(STEPS):
        if step % 50 == 0:
            el, ea = evaluate()
            f.write(json.dumps({"step": step, "eval_loss": el, "eval_exact_match": ea}) + "\n"); f.flush()
        model.rng.new_step(step)
        store.zero_grad()
        loss, _ = run(tr, slice(B * step, B * (step + 1)))
        loss.backward()
        opt.step(grad_scale=1.0)
        if step % 10 == 0:
            s = loss._hsd_stats.tolist()
            f.write(json.dumps({"step": step, "train_loss": s[0], "train_exact_match": s[1] / max(s[2], 1.0)}) + "\n")
    el, ea = evaluate()
    f.write(json.dumps({"step": STEPS, "eval_loss": el, "eval_exact_match": ea}) + "\n")
print(f"learning curve: held-out loss {el:.4f}, exact match {ea:.4f} after {STEPS} steps (always-(0,0) baseline {none:.3f})")
