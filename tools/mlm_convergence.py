"""Learning curve of --mlm_masking dynamic on one GPU: a RoBERTa encoder of roberta-base width with a few layers and
a small vocabulary, trained from random init on the synthetic-bigram corpus (data/datasets.py: x[i+1] = succ[x[i]]
nine times in ten), a fresh device-side mask every step. Prints one JSON line in the format of tools/convergence.py:
the loss curve (mean over 25-step windows), the held-out loss / accuracy over the dynamic evaluation masks, and
log V for scale (an i.i.d. corpus cannot get below it).

    python tools/mlm_convergence.py --steps 1000 [--dtype fp8] [--hip_graph true]"""
import argparse
import json
import math
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model_dir(layers: int, vocab: int) -> str:
    d = tempfile.mkdtemp(prefix="hsd-mlm-conv-")
    cfg = {"model_type": "roberta", "architectures": ["RobertaForMaskedLM"], "vocab_size": vocab, "hidden_size": 768,
           "num_hidden_layers": layers, "num_attention_heads": 12, "intermediate_size": 3072, "hidden_act": "gelu",
           "hidden_dropout_prob": 0.1, "attention_probs_dropout_prob": 0.1, "max_position_embeddings": 514,
           "type_vocab_size": 1, "initializer_range": 0.02, "layer_norm_eps": 1e-5, "pad_token_id": 1,
           "bos_token_id": 0, "eos_token_id": 2}
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(cfg, f)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seq_len", type=int, default=128)
    ap.add_argument("--lr", type=float, default=2e-4)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--vocab", type=int, default=1024)
    ap.add_argument("--dtype", choices=["bf16", "fp8"], default="bf16")
    ap.add_argument("--hip_graph", default="false")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    from huggingface_sagemaker_tensorflow_distributed_amd import data as hdata
    from huggingface_sagemaker_tensorflow_distributed_amd.data.loader import BatchLoader
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import ShardSampler
    from huggingface_sagemaker_tensorflow_distributed_amd.train.runner import build
    from huggingface_sagemaker_tensorflow_distributed_amd.utils.args import build_parser

    args, _ = build_parser("train").parse_known_args(
        ["--model_name_or_path", _model_dir(a.layers, a.vocab), "--task", "masked-lm", "--mlm_masking", "dynamic",
         "--dataset", "synthetic-bigram", "--train_batch_size", str(a.batch), "--max_seq_length", str(a.seq_len),
         "--learning_rate", str(a.lr), "--lr_schedule", "linear", "--lr_warmup_steps", str(a.warmup),
         "--dtype", a.dtype, "--hip_graph", a.hip_graph, "--log_every", "0", "--seed", "7"])
    parts = build(args, "train")
    tr, dev, model = parts["trainer"], parts["device"], parts["model"]
    tr.total_steps = a.steps
    pad = model.cfg.pad_token_id
    n_train = min(a.batch * a.steps, 32768)  # the corpus wraps around: every pass draws new masks
    ds = hdata.synthetic_bigram(n_train, a.seq_len, a.vocab, seed=1, pad_id=pad)
    test = hdata.synthetic_bigram(1024, a.seq_len, a.vocab, seed=2, pad_id=pad)
    curve, window = [], []
    for i in range(a.steps):
        ix = [(i * a.batch + j) % n_train for j in range(a.batch)]
        mb = {"input_ids": torch.from_numpy(ds.input_ids[ix]).long().to(dev),
              "attention_mask": torch.from_numpy(ds.attention_mask[ix]).long().to(dev),
              "labels": torch.from_numpy(ds.labels[ix]).long().to(dev)}
        window.append(tr.train_step([mb]).detach().clone())
        if len(window) == 25:
            curve.append(round(float(torch.stack(window).float().mean()), 4))
            window = []
    loader = BatchLoader(test, ShardSampler(len(test), 0, 1, shuffle=False, drop_last=False, batch_size=64), dev)
    ev = tr.evaluate(loader)
    print(json.dumps({"path": "hip", "task": "masked-lm", "mlm_masking": "dynamic", "dataset": "synthetic-bigram",
                      "dtype": a.dtype, "hip_graph": bool(tr._seed is not None), "layers": a.layers, "vocab": a.vocab,
                      "steps": a.steps, "batch": a.batch, "seq_len": a.seq_len, "lr": a.lr, "warmup": a.warmup,
                      "log_vocab": round(math.log(a.vocab), 4), "loss_curve_25": curve,
                      "eval_loss": round(ev["loss"], 4), "eval_accuracy": round(ev["sparse_categorical_accuracy"], 4),
                      "dropped_selections": model.mlm_dropped()}), flush=True)


if __name__ == "__main__":
    main()
