"""End-to-end entry logic shared by ``scripts/train.py`` and ``scripts/singe_node_train.py``.

Two batch/LR semantics, exactly as the two reference scripts differ:

* ``mode="train"`` (Horovod/SMDDP, ``scripts/train.py``): ``--train_batch_size`` is PER RANK,
  learning rate is scaled ×N (``scripts/train.py:112``), ``train_results.txt`` gets a
  ``train_runtime`` line (``:165``).
* ``mode="single_node"`` (MirroredStrategy, ``scripts/singe_node_train.py``): ``--train_batch_size``
  is the GLOBAL batch split across replicas, no LR scaling (``:78``), no runtime line (``:96-101``).

Reference fixes applied: Q3 data sharded by rank, Q4 params broadcast before
step 1, Q5 rank-0-only save + barrier, Q6 global metrics.
"""
from __future__ import annotations

import contextlib
import json
import logging
import os
import time
from typing import List, Optional, Sequence

import torch

from .. import data as hdata
from .. import ops
from ..models import from_pretrained, save_pretrained
from ..optim import FusedAdam, FusedLamb
from ..optim import groups as lr_groups
from ..parallel.ddp import resolve_compression
from ..parallel.flat_params import keep_transposed_weights
from ..parallel import FlatParamStore, GradBucketer, ShardSampler, backend, broadcast_parameters
from ..utils.args import parse_args
from ..utils.env import is_sagemaker_dp_enabled
from ..utils.logging import setup_logging
from ..utils.results_io import write_eval_results, write_train_results
from . import batch_planner
from .callbacks import FaultInjection, ModelCheckpoint, load_checkpoint, master_state_dict
from .trainer import Trainer

logger = logging.getLogger("__main__")

_DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp8": torch.bfloat16}


def _datasets(args, cfg, tokenizer, max_len: int):
    n_train = args.num_train_examples
    n_eval = args.num_eval_examples
    if getattr(args, "task", "sequence-classification") == "masked-lm":
        if args.dataset not in ("synthetic", "synthetic-bigram"):
            raise ValueError("--task masked-lm trains on --dataset synthetic or synthetic-bigram (no text corpus "
                             "offline)")
        p = float(getattr(args, "mlm_probability", 0.15))
        dynamic = getattr(args, "mlm_masking", "static") == "dynamic"
        ids = {"bos_id": cfg.bos_token_id if cfg.bos_token_id is not None else 0,
               "eos_id": cfg.eos_token_id if cfg.eos_token_id is not None else 2}
        if args.dataset == "synthetic" and not dynamic:
            # the corpus masked once as it is built: i.i.d. tokens, all full length
            tr = hdata.synthetic_mlm(n_train or 2048, max_len, cfg.vocab_size, seed=args.seed, mlm_probability=p, **ids)
            te = hdata.synthetic_mlm(n_eval or 512, max_len, cfg.vocab_size, seed=args.seed + 1, mlm_probability=p,
                                     **ids)
            return tr, te
        make = hdata.synthetic_bigram if args.dataset == "synthetic-bigram" else hdata.synthetic_mlm_raw
        tr = make(n_train or 2048, max_len, cfg.vocab_size, seed=args.seed, pad_id=cfg.pad_token_id, **ids)
        te = make(n_eval or 512, max_len, cfg.vocab_size, seed=args.seed + 1, pad_id=cfg.pad_token_id, **ids)
        if not dynamic:
            # a raw corpus under static masking: masked once, here, with the reference masker
            mask_id = 50264 % cfg.vocab_size
            special = sorted({int(cfg.pad_token_id), int(ids["bos_id"]), int(ids["eos_id"]), mask_id})
            # the model's own rule (RobertaForMaskedLM.mlm_rand_range): replacements from above pad / bos / eos
            rr = (min(1 + max(int(cfg.pad_token_id), int(ids["bos_id"]), int(ids["eos_id"])), cfg.vocab_size - 1),
                  cfg.vocab_size)
            tr = hdata.mask_dataset_static(tr, args.seed, p, mask_id, special, rr)
            te = hdata.mask_dataset_static(te, args.seed + 1, p, mask_id, special, rr)
        return tr, te
    if getattr(args, "task", "sequence-classification") == "token-classification":
        if args.dataset == "synthetic":
            kw = {"num_labels": cfg.num_labels, "pad_id": cfg.pad_token_id}
            if cfg.model_type == "roberta":
                kw.update(cls_id=cfg.bos_token_id if cfg.bos_token_id is not None else 0,
                          sep_id=cfg.eos_token_id if cfg.eos_token_id is not None else 2)
            tr = hdata.synthetic_token_classification(n_train or 2048, max_len, cfg.vocab_size, seed=args.seed, **kw)
            te = hdata.synthetic_token_classification(n_eval or 512, max_len, cfg.vocab_size, seed=args.seed + 1, **kw)
            return tr, te
        if args.dataset == "conll":
            tags = _conll_tags(args)
            out = []
            for split, n in (("train", n_train), ("test", n_eval)):
                from ..data.datasets import conll_split_path

                words, wtags = hdata.read_conll(conll_split_path(args.dataset_dir, split))
                if n:
                    words, wtags = words[:n], wtags[:n]
                out.append(hdata.tokenize_conll(tokenizer, words, wtags, tags, max_len))
            return out[0], out[1]
        raise ValueError(f"--task token-classification trains on --dataset synthetic or conll (per-token labels); "
                         f"--dataset {args.dataset} holds one label per text")
    if getattr(args, "task", "sequence-classification") == "question-answering":
        segs = cfg.model_type == "bert"  # segment ids 0 / 1 for BERT; RoBERTa and DistilBERT take none
        if args.dataset == "synthetic":
            kw = {"segment_ids": segs, "pad_id": cfg.pad_token_id}
            if cfg.model_type == "roberta":
                kw.update(cls_id=cfg.bos_token_id if cfg.bos_token_id is not None else 0,
                          sep_id=cfg.eos_token_id if cfg.eos_token_id is not None else 2)
            tr = hdata.synthetic_question_answering(n_train or 2048, max_len, cfg.vocab_size, seed=args.seed, **kw)
            te = hdata.synthetic_question_answering(n_eval or 512, max_len, cfg.vocab_size, seed=args.seed + 1, **kw)
            return tr, te
        if args.dataset == "squad":
            from ..data.datasets import squad_split_path

            if not args.dataset_dir:
                raise ValueError("--dataset squad needs --dataset_dir (train*.json and dev*.json in SQuAD format)")
            out = []
            for split, n in (("train", n_train), ("dev", n_eval)):
                ex = hdata.read_squad(squad_split_path(args.dataset_dir, split))
                if n:
                    ex = ex[:n]
                out.append(hdata.tokenize_squad(tokenizer, ex, max_len, int(getattr(args, "doc_stride", 128)),
                                                segment_ids=segs))
            return out[0], out[1]
        raise ValueError(_QA_DATASETS.format(args.dataset))
    if args.dataset == "squad":
        raise ValueError("--dataset squad holds answer spans (--task question-answering)")
    if args.dataset == "conll":
        raise ValueError("--dataset conll holds per-token tags (--task token-classification)")
    if args.dataset == "synthetic-bigram":
        raise ValueError("--dataset synthetic-bigram is a masked-lm corpus (--task masked-lm)")
    ptype = getattr(cfg, "problem_type", None)
    if ptype in ("regression", "multi_label_classification"):
        if args.dataset == "synthetic":
            make = hdata.synthetic_regression if ptype == "regression" else hdata.synthetic_multi_label
            kw = {"num_labels": cfg.num_labels, "pad_id": cfg.pad_token_id}
            if cfg.model_type == "roberta":
                kw.update(cls_id=cfg.bos_token_id if cfg.bos_token_id is not None else 0,
                          sep_id=cfg.eos_token_id if cfg.eos_token_id is not None else 2)
            return (make(n_train or 2048, max_len, cfg.vocab_size, seed=args.seed, **kw),
                    make(n_eval or 512, max_len, cfg.vocab_size, seed=args.seed + 1, **kw))
        if args.dataset in ("imdb", "sst2"):
            raise ValueError(_PTYPE_DATASETS.format(ptype, args.dataset))
        out = []
        for split, n in (("train", n_train), ("test", n_eval)):
            texts, labels = hdata.load_text_split(args.dataset, split, args.dataset_dir, problem_type=ptype,
                                                  num_labels=cfg.num_labels)
            if n:
                texts, labels = texts[:n], labels[:n]
            out.append(hdata.tokenize_dataset(tokenizer, texts, labels, max_len))
        return out[0], out[1]
    if args.dataset == "synthetic":
        tr = hdata.synthetic_classification(n_train or 2048, max_len, cfg.vocab_size, seed=args.seed,
                                            num_labels=cfg.num_labels)
        te = hdata.synthetic_classification(n_eval or 512, max_len, cfg.vocab_size, seed=args.seed + 1,
                                            num_labels=cfg.num_labels)
        return tr, te
    texts, labels = hdata.load_text_split(args.dataset, "train", args.dataset_dir)
    if n_train:
        texts, labels = texts[:n_train], labels[:n_train]
    tr = hdata.tokenize_dataset(tokenizer, texts, labels, max_len)
    texts, labels = hdata.load_text_split(args.dataset, "test", args.dataset_dir)
    if n_eval:
        texts, labels = texts[:n_eval], labels[:n_eval]
    te = hdata.tokenize_dataset(tokenizer, texts, labels, max_len)
    return tr, te


_PTYPE_DATASETS = ("--problem_type {} needs float targets: --dataset synthetic or local csv / json files "
                   "(--dataset_dir); --dataset {} holds one class per text")
_QA_DATASETS = ("--task question-answering trains on --dataset synthetic or squad (start / end positions); "
                "--dataset {} holds no answer spans")


def _label_smoothing(args, task: str, ptype) -> float:
    """``--label_smoothing_factor`` of the run, refused where no single-label cross-entropy is trained."""
    eps = float(getattr(args, "label_smoothing_factor", 0.0) or 0.0)
    if not 0.0 <= eps < 1.0:  # NaN fails both comparisons
        raise ValueError(f"--label_smoothing_factor {eps} must be in [0, 1)")
    if eps > 0.0 and task == "question-answering":
        raise ValueError("--label_smoothing_factor smooths a single-label cross-entropy; --task question-answering "
                         "trains a span loss, which it does not apply to")
    if eps > 0.0 and ptype in ("regression", "multi_label_classification"):
        raise ValueError(f"--label_smoothing_factor smooths a single-label cross-entropy; --problem_type {ptype} "
                         f"trains {'an MSE' if ptype == 'regression' else 'a BCE-with-logits'} loss")
    return eps


def _lr_group_flags(args):
    """``(--layerwise_lr_decay, --head_lr_multiplier)`` of the run, refused outside (0, 1] and finite > 0."""
    return lr_groups.validate(getattr(args, "layerwise_lr_decay", 1.0), getattr(args, "head_lr_multiplier", 1.0))


def _lr_multipliers(args, store, cfg, lr: float):
    """The run's per-parameter learning-rate multipliers ({segment name: μ}; None = both flags at 1), with the startup
    table: depth, μ, the learning rate after the world-size rule, parameters."""
    decay, head = _lr_group_flags(args)
    mul = lr_groups.lr_multipliers(store.names, cfg.num_hidden_layers, decay, head)
    if mul is not None:
        rows = lr_groups.depth_table(store.names, [sg.numel for sg in store.segments], cfg.num_hidden_layers, decay,
                                     head, lr)
        logger.info("--layerwise_lr_decay %g --head_lr_multiplier %g: learning rate per depth (base %g)\n%s", decay,
                    head, lr, lr_groups.format_table(rows))
    return mul


def _ema_flags(args):
    """``(--ema_decay, --ema_warmup)`` of the run: the decay is 0 (off) or finite in (0, 1); warm-up needs a decay."""
    d = float(getattr(args, "ema_decay", 0.0) or 0.0)
    warm = bool(getattr(args, "ema_warmup", False))
    if d != 0.0 and not (0.0 < d < 1.0):  # NaN and inf fail the comparison
        raise ValueError(f"--ema_decay {d} must be 0 (off) or finite with 0 < D < 1")
    if warm and d == 0.0:
        raise ValueError("--ema_warmup true needs --ema_decay D with 0 < D < 1")
    return d, warm


def _conll_tags(args) -> Optional[List[str]]:
    """The tag list of ``--task token-classification --dataset conll`` (read once, kept on ``args``)."""
    if getattr(args, "task", "") != "token-classification" or args.dataset != "conll":
        return None
    tags = getattr(args, "_conll_tags", None)
    if tags is None:
        if not args.dataset_dir:
            raise ValueError("--dataset conll needs --dataset_dir (train.txt and test.txt in CoNLL column format)")
        tags = args._conll_tags = hdata.conll_tag_list(args.dataset_dir)
    return tags


def _provenance(args, model, rank: int, n_train: int, n_eval: int, batch_plan=None) -> dict:
    """Say loudly when the run is not the reference's imdb fine-tune of pretrained weights: results files keep
    the reference's exact format, so the data / weights they came from go to ``run_provenance.json`` beside
    them and to a WARNING in the log."""
    weights = getattr(model, "weights_source", "random-init")
    synthetic = args.dataset in ("synthetic", "synthetic-bigram")
    info = {"dataset": args.dataset, "synthetic_data": synthetic, "weights": weights,
            "model_name_or_path": args.model_name_or_path, "num_train_examples": n_train,
            "num_eval_examples": n_eval, "train_batch_size": args.train_batch_size,
            "pack_sequences": bool(getattr(args, "pack_sequences", False))}
    if getattr(args, "task", "sequence-classification") == "masked-lm":
        dynamic = getattr(args, "mlm_masking", "static") == "dynamic"
        info["mlm_masking"] = "dynamic" if dynamic else "static"
        info["mlm_probability"] = float(getattr(args, "mlm_probability", 0.15))
        info["corpus"] = ("synthetic-bigram (first-order chain, ragged lengths)" if args.dataset == "synthetic-bigram"
                          else "synthetic i.i.d. tokens, " + ("raw, ragged lengths" if dynamic
                                                              else "masked when built, full length"))
        logger.info("masked-lm corpus: %s; --mlm_masking %s, --mlm_probability %g", info["corpus"],
                    info["mlm_masking"], info["mlm_probability"])
    if getattr(args, "task", "sequence-classification") == "token-classification":
        info["task"] = "token-classification"
        info["num_labels"] = int(model.cfg.num_labels)
        info["corpus"] = ("CoNLL column files in " + str(args.dataset_dir) if args.dataset == "conll" else
                          "synthetic tagging corpus (tag = f(token, left neighbour), ragged lengths, ~25 % of the "
                          "real tokens ignored)")
        info["metric"] = "loss and accuracy over the labelled tokens (not entity-level F1)"
        logger.info("token-classification corpus: %s; %d labels", info["corpus"], info["num_labels"])
    if getattr(args, "task", "sequence-classification") == "question-answering":
        info["task"] = "question-answering"
        info["max_answer_length"] = int(getattr(args, "max_answer_length", 30))
        info["corpus"] = ("SQuAD-format files in " + str(args.dataset_dir) + ", doc_stride "
                          + str(int(getattr(args, "doc_stride", 128))) if args.dataset == "squad" else
                          "synthetic span corpus ([CLS] key [SEP] context [SEP], the answer follows the key's one "
                          "occurrence in the context, ~10 % without an answer, ragged lengths)")
        info["metric"] = ("loss and exact match of the best (start, end) token span over the windows with both "
                          "labels valid (not text-level EM / F1)")
        logger.info("question-answering corpus: %s; max_answer_length %d", info["corpus"], info["max_answer_length"])
    ptype = getattr(model.cfg, "problem_type", None)
    if ptype is not None and getattr(args, "task", "sequence-classification") == "sequence-classification":
        info["problem_type"] = ptype
        info["num_labels"] = int(model.cfg.num_labels)
        if ptype == "regression":
            info["regression_tolerance"] = float(getattr(model, "regression_tolerance", 0.5))
            if synthetic:
                info["corpus"] = ("synthetic regression corpus (one of 16 marker tokens, index j, at a random interior "
                                  "position; y[c] = ((j(2c+1)) mod 16)/4 - 2; ragged lengths)")
            info["metric"] = ("MSE loss; accuracy = rows with |prediction - target| <= regression_tolerance on every "
                              "target (not Pearson / Spearman)")
        elif ptype == "multi_label_classification":
            if synthetic:
                info["corpus"] = ("synthetic multi-label corpus (one marker token per label, each present with "
                                  "probability 1/4 at distinct interior positions; ragged lengths)")
            info["metric"] = ("BCE-with-logits loss; accuracy = subset accuracy, rows with every label right at "
                              "threshold 0 (not F1)")
        else:
            info["metric"] = "cross-entropy loss and argmax accuracy"
        logger.info("sequence-classification problem_type %s; %d labels; %s", ptype, info["num_labels"], info["metric"])
    eps = float(getattr(model, "label_smoothing", 0.0))
    if eps > 0.0:
        info["label_smoothing_factor"] = eps
        if "metric" in info:
            info["metric"] += (f"; the loss, in training and in evaluation, is the label-smoothed cross-entropy "
                               f"(eps = {eps:g})")
        logger.info("--label_smoothing_factor %g: training and evaluation report the smoothed cross-entropy", eps)
    decay, head = _lr_group_flags(args)
    if decay != 1.0 or head != 1.0:
        info["layerwise_lr_decay"] = decay
        info["head_lr_multiplier"] = head
    ema_d, ema_warm = _ema_flags(args)
    if ema_d:
        info["ema_decay"] = ema_d
        info["ema_warmup"] = ema_warm
    if batch_plan is not None:
        info["auto_batch"] = batch_plan.as_dict()
    if synthetic or weights == "random-init":
        what = " and ".join(x for x in (("synthetic random data" if synthetic else ""),
                                         ("random-init weights" if weights == "random-init" else "")) if x)
        logger.warning("training on %s: train_results.txt / eval_results.txt are NOT comparable with the "
                       "reference's imdb fine-tune of pretrained %s (see run_provenance.json)", what,
                       args.model_name_or_path)
    if rank == 0:
        os.makedirs(args.output_data_dir, exist_ok=True)
        with open(os.path.join(args.output_data_dir, "run_provenance.json"), "w") as f:
            json.dump(info, f, indent=1)
    return info


def build(args, mode: str):
    """Construct model/store/optimizer/bucketer/trainer for ``args``. Returns a dict of parts."""
    st = backend.init(device=args.device, timeout_s=args.dist_timeout)
    dev = st.device
    world, rank = st.world_size, st.rank
    on_gpu = dev.type == "cuda"
    dtype_name = args.dtype or ("bf16" if on_gpu else "fp32")
    compute_dtype = _DTYPES[dtype_name]
    pack = bool(getattr(args, "pack_sequences", False))
    if pack and (dtype_name == "fp8" or (dtype_name == "fp32" and on_gpu)):
        raise ValueError(f"--pack_sequences true runs in bf16 on the GPU (the variable-length attention kernels are "
                         f"bf16; CPU fp32 runs the reference ops): --dtype {dtype_name} is not supported with it")
    grad_dtype = {"fp32": torch.float32, "bf16": torch.bfloat16}[args.grad_dtype or "fp32"]
    torch.manual_seed(args.seed)

    task = getattr(args, "task", "sequence-classification")
    if task == "token-classification" and args.dataset not in ("synthetic", "conll"):
        raise ValueError(f"--task token-classification trains on --dataset synthetic or conll (per-token labels); "
                         f"--dataset {args.dataset} holds one label per text")
    if task == "question-answering" and args.dataset not in ("synthetic", "squad"):
        raise ValueError(_QA_DATASETS.format(args.dataset))
    ptype = getattr(args, "problem_type", None)
    if ptype is not None and task != "sequence-classification":
        raise ValueError(f"--problem_type {ptype} is valid only with --task sequence-classification, not --task {task}")
    if ptype in ("regression", "multi_label_classification") and args.dataset in ("imdb", "sst2"):
        raise ValueError(_PTYPE_DATASETS.format(ptype, args.dataset))
    smoothing = _label_smoothing(args, task, ptype)
    _lr_group_flags(args)
    ema_d, ema_warm = _ema_flags(args)
    tags = _conll_tags(args)
    if tags is not None:
        if args.num_labels != len(tags):
            logger.info("--dataset conll: %d tags %s; --num_labels %d -> %d", len(tags), tags, args.num_labels, len(tags))
        args.num_labels = len(tags)
    model = from_pretrained(args.model_name_or_path or "bert-base-uncased", task=task, num_labels=args.num_labels,
                            seed=args.seed, problem_type=ptype)
    if task == "sequence-classification":
        tol = float(getattr(args, "regression_tolerance", 0.5))
        if not tol >= 0.0:
            raise ValueError(f"--regression_tolerance {tol} must be >= 0")
        model.regression_tolerance = tol
    model.label_smoothing = smoothing  # a training argument on the model object (never in config.json)
    if tags is not None:
        model.cfg.id2label = {str(i): t for i, t in enumerate(tags)}  # config.json id2label / label2id
    model.to(dev)
    model.rng.base_seed = args.seed
    model.rng.rank = rank
    if task == "question-answering":
        if int(getattr(args, "max_answer_length", 30)) < 1:
            raise ValueError(f"--max_answer_length {args.max_answer_length} must be at least 1")
        model.max_answer_length = int(getattr(args, "max_answer_length", 30))
    if task == "masked-lm":
        # dynamic: the model masks each batch on the device and its head has a fixed row count (--dtype fp8 takes
        # the same fp8 head GEMMs as the static head: both call the one gemm_fwd / gemm_dgrad / gemm_wgrad_ chain)
        model.set_mlm_masking(getattr(args, "mlm_masking", "static"), getattr(args, "mlm_probability", 0.15))
    # --dtype fp8: bf16 activations / master-weight copies plus fp8 (e4m3) weight copies and per-tensor
    # quantised fp8 forward + dgrad GEMMs on the HIP path (ops/hip.py set_fp8); CPU runs stay bf16.
    if dtype_name == "fp32" and on_gpu:
        logger.info("--dtype fp32 on the GPU: the reference's precision on the fp32 kernels (ops/hip32.py: split-product "
                    "MFMA GEMMs, fp32 LayerNorm / embeddings / streaming attention / head, fused fp32 Adam); "
                    "--dtype bf16 is the fast path")
    fp8 = dtype_name == "fp8" and on_gpu and ops.hip_active(dev)
    if dtype_name == "fp8" and not fp8:
        logger.warning("--dtype fp8 needs the HIP path on a GPU; computing in bf16")
    if fp8:
        ops.set_fp8(True, getattr(args, "fp8_grad_format", "e4m3"))
    tokenizer = hdata.load_tokenizer(args.model_name_or_path, model.cfg.vocab_size, model.cfg.model_max_length)
    max_len = args.max_seq_length or min(tokenizer.model_max_length, model.cfg.max_position_embeddings)
    rank_tokens = None
    if args.train_batch_size != "auto":
        rank_tokens = (int(args.train_batch_size) // (1 if mode == "train" else world)) * max_len
    store = FlatParamStore(model, dev, compute_dtype=compute_dtype, grad_dtype=grad_dtype, fp8=fp8,
                           transposed=keep_transposed_weights(rank_tokens))
    base_lr = float(args.learning_rate)
    lr = base_lr * world if mode == "train" else base_lr  # scripts/train.py:112 vs singe_node_train.py:78
    lr_mul = _lr_multipliers(args, store, model.cfg, lr)
    if args.optimizer == "lamb":
        # the learning rate keeps the Horovod x world rule above; LAMB always uses its bias-corrected form
        if args.adam_eps_mode != "keras":
            logger.info("--adam_eps_mode %s does not apply to --optimizer lamb (ignored)", args.adam_eps_mode)
        opt = FusedLamb(store, lr=lr, eps=args.adam_epsilon, weight_decay=args.weight_decay,
                        max_grad_norm=float(getattr(args, "max_grad_norm", 0.0) or 0.0), lr_multipliers=lr_mul,
                        ema_decay=ema_d, ema_warmup=ema_warm)
    else:
        opt = FusedAdam(store, lr=lr, eps=args.adam_epsilon, eps_mode=args.adam_eps_mode,
                        weight_decay=args.weight_decay if args.optimizer == "adamw" else 0.0,
                        max_grad_norm=float(getattr(args, "max_grad_norm", 0.0) or 0.0), lr_multipliers=lr_mul,
                        ema_decay=ema_d, ema_warmup=ema_warm)
    if ema_d:
        logger.info("--ema_decay %g --ema_warmup %s: the fused %s step keeps an fp32 average of the weights (%.1f MB "
                    "more on the device); the final evaluation and the saved model are those of the averaged weights",
                    ema_d, "true" if ema_warm else "false", args.optimizer, opt.ema.numel() * 4 / 2**20)
    batch_plan = None
    if args.train_batch_size == "auto":
        # sized on the device before any readiness hook / bucketer exists (the probes are plain fwd + bwd)
        batch_plan = batch_planner.plan(model, store, max_len, dev, headroom=args.auto_batch_headroom,
                                        max_tokens=args.auto_batch_max_tokens or None,
                                        compression=resolve_compression(getattr(args, "grad_compression", "none"),
                                                                        world, on_gpu, dtype_name))
        per_gpu = batch_planner.agree_min(batch_plan.per_gpu_batch, dev)
        batch_plan.per_gpu_batch = per_gpu
        args.train_batch_size = per_gpu if mode == "train" else per_gpu * world
        logger.info("--train_batch_size auto: %d per GPU (%s, %.1f MB/sequence, fixed %.2f GB, budget %.1f of "
                    "%.1f GB, capped by %s) -> train_batch_size %d", per_gpu, batch_plan.method,
                    batch_plan.per_seq_bytes / 2**20, batch_plan.fixed_bytes / 2**30, batch_plan.budget_bytes / 2**30,
                    batch_plan.total_bytes / 2**30, batch_plan.capped_by, args.train_batch_size)
    per_rank = int(args.train_batch_size) // (1 if mode == "train" else world)
    wire = resolve_compression(getattr(args, "grad_compression", "none"), world, on_gpu, dtype_name)
    if world > 1:
        logger.info("gradient wire format: %s (--grad_compression %s)", wire, getattr(args, "grad_compression", "none"))
    bucketer = GradBucketer(store, bucket_mb=args.bucket_mb, compression=wire) if world > 1 else None
    hip_graph = getattr(args, "hip_graph", False)
    if pack:
        # data-dependent shapes: auto resolves to off; an explicit true is refused (loudly) by enable_hip_graph
        hip_graph = False if hip_graph == "auto" else hip_graph
    trainer = Trainer(model, store, opt, bucketer, dev, grad_accum=args.gradient_accumulation_steps,
                      pack_sequences=pack,
                      lr_schedule=getattr(args, "lr_schedule", "constant"),
                      lr_warmup_steps=getattr(args, "lr_warmup_steps", 0),
                      check_sync=args.check_sync, log_every=args.log_every, step_watchdog=args.step_watchdog,
                      hip_graph=resolve_hip_graph(hip_graph, on_gpu, world,
                                                  per_rank * max_len, args.gradient_accumulation_steps),
                      eval_hip_graph=getattr(args, "eval_hip_graph", "auto"))
    initial_epoch = 0
    if args.resume_from:
        initial_epoch = int(load_checkpoint(args.resume_from, trainer).get("epoch", 0))
    broadcast_parameters(store, opt if args.resume_from else None)
    if not args.resume_from:
        opt.reset_ema()  # the average starts from the weights every rank now holds
    return {"initial_epoch": initial_epoch, "tokenizer": tokenizer, "max_len": max_len, "batch_plan": batch_plan,
            "model": model, "store": store, "optimizer": opt, "bucketer": bucketer, "trainer": trainer,
            "device": dev, "world": world, "rank": rank, "lr": lr, "dtype": dtype_name}


def resolve_hip_graph(flag, on_gpu: bool, world: int, tokens: int, accum: int) -> bool:
    """``--hip_graph``: True / False as given; ``auto`` = on for single-process GPU steps of one micro-step and at most
    HSD_GRAPH_AUTO_MAX_TOKENS (2,048) tokens, where the step is launch-bound and the replay wins (bert-base S = 128,
    one MI355X: B = 1 170-192 -> 254-261 seq/s, B = 8 1,314-1,422 -> 1,862-1,877, B = 16 3,042-3,077 -> 3,198-3,208;
    at B = 32 and bert-large B = 8 eager is 10-12 % faster: profiles/graph_small_batch_r5.log,
    profiles/graph_vs_eager_r5.log)."""
    if flag != "auto":
        return bool(flag)
    cap = int(os.environ.get("HSD_GRAPH_AUTO_MAX_TOKENS", "2048"))
    on = bool(on_gpu and world == 1 and int(accum) <= 1 and 0 < tokens <= cap)
    logger.info("--hip_graph auto: %s (%d tokens per step, cap %d, world %d)", "on" if on else "off", tokens, cap, world)
    return on


def run(argv: Optional[Sequence[str]] = None, mode: str = "train") -> dict:
    args, _unknown = parse_args(argv, "train" if mode == "train" else "single_node")
    env_rank = int(os.environ.get("RANK", "0"))
    setup_logging(env_rank)
    if mode == "train":
        logger.info(args)  # scripts/train.py:63
        if is_sagemaker_dp_enabled():
            logger.info("SMDDP requested via SM_FRAMEWORK_PARAMS: served by the RCCL data-parallel engine")
    parts = build(args, mode)
    model, trainer, dev = parts["model"], parts["trainer"], parts["device"]
    world, rank = parts["world"], parts["rank"]
    cfg = model.cfg

    tokenizer, max_len = parts["tokenizer"], parts["max_len"]
    train_ds, test_ds = _datasets(args, cfg, tokenizer, max_len)

    if mode == "train":
        per_rank_train = args.train_batch_size
    else:  # MirroredStrategy: global batch split over replicas
        if args.train_batch_size % world:
            raise ValueError(f"global train_batch_size {args.train_batch_size} not divisible by {world} replicas")
        per_rank_train = args.train_batch_size // world
    per_rank_eval = args.eval_batch_size if mode == "train" else max(1, args.eval_batch_size // world)
    # eval batch coalescing: evaluation has no dropout and no cross-example math (no batch statistics), so each
    # example's logits and loss do not depend on which examples share its forward, and the metrics are per-example
    # means (Keras evaluate with SUM_OVER_BATCH_SIZE over equal batches). Consecutive eval batches are therefore run
    # k at a time, up to --eval_coalesce_tokens tokens per forward: the reference's eval_batch_size 2 at S = 512
    # (launch.py:16) is 1,024-token forwards that leave most of the GPU idle. 0 = one forward per eval batch.
    coalesce = max(1, int(getattr(args, "eval_coalesce_tokens", 0) or 0) // max(1, per_rank_eval * max_len))
    per_rank_eval_fwd = per_rank_eval * coalesce
    if coalesce > 1:
        logger.info("evaluate: eval_batch_size %d per rank, %d batches per forward (%d sequences; "
                    "--eval_coalesce_tokens %d)", per_rank_eval, coalesce, per_rank_eval_fwd, args.eval_coalesce_tokens)

    pack_kw = {}
    if getattr(args, "pack_sequences", False):
        pack_kw = {"pack": True, "pack_rule": hdata.position_rule(cfg)}
    train_loader = hdata.BatchLoader(train_ds, ShardSampler(len(train_ds), rank, world, shuffle=False, seed=args.seed,
                                                             batch_size=per_rank_train), dev, **pack_kw)
    # eval scores every test example once (reference model.evaluate, scripts/train.py:170): shards padded with
    # ignored rows, the last partial batch kept
    test_loader = hdata.BatchLoader(test_ds, ShardSampler(len(test_ds), rank, world, shuffle=False, seed=args.seed,
                                                           drop_last=False, mark_padding=True,
                                                           batch_size=per_rank_eval_fwd), dev, **pack_kw)
    if pack_kw and len(train_loader):
        b0 = train_loader._host_batch(next(iter(train_loader.sampler.batches())))
        logger.info("--pack_sequences: first batch holds %d real tokens of %d padded (%.1f %% padding), packed into "
                    "%d rows", b0["real_tokens"], per_rank_train * max_len,
                    100.0 * (1.0 - b0["real_tokens"] / float(per_rank_train * max_len)), b0["input_ids"].shape[-1])
    _provenance(args, model, rank, len(train_ds), len(test_ds), parts["batch_plan"])
    out = {"args": args}
    callbacks = [FaultInjection()]
    if args.benchmark or args.profile:
        from ..obs import ProfilerCallback, ThroughputMeter

        if args.benchmark:
            callbacks.append(ThroughputMeter(args.output_data_dir, per_rank_train, max_len, warmup=args.warmup_steps,
                                             log_every=args.log_every, packed=bool(pack_kw),
                                             info={"model": args.model_name_or_path, "dtype": parts["dtype"],
                                                   "script": mode, "data": args.dataset}))
        if args.profile:
            callbacks.append(ProfilerCallback(args.output_data_dir, start=args.warmup_steps, steps=3, rank=rank))
    if args.save_every_epoch:
        callbacks.append(ModelCheckpoint(os.path.join(args.model_dir, "checkpoint-{epoch}")))

    if args.do_train:
        if mode == "train":
            logger.info("*** Train ***")
        start = time.time()
        hist = trainer.fit(train_loader, args.epochs, callbacks=callbacks, verbose=(rank == 0),
                           max_steps=args.max_steps, initial_epoch=parts["initial_epoch"])
        train_runtime = {"train_runtime": round(time.time() - start, 4)}
        if mode == "train":
            logger.info(f"train_runtime = {train_runtime}\n")
        else:
            logger.info("*** Train ***")  # singe_node_train.py logs it AFTER fit (:92)
        if rank == 0:
            write_train_results(args.output_data_dir, hist.history, train_runtime if mode == "train" else None)
        out["history"] = hist.history
        out["train_runtime"] = train_runtime

    if args.do_eval:
        logger.info("*** Evaluate ***")
        start = time.time()
        # with --ema_decay the final scores are those of the averaged weights (Keras' finalize_variable_values at the end
        # of fit); the meter's global all-reduce syncs the device
        result = trainer.evaluate(test_loader, weights="ema" if parts["optimizer"].ema is not None else None)
        eval_runtime = round(time.time() - start, 4)
        # not in eval_results.txt (the reference's writer holds the metrics only, scripts/train.py:172-179): the log line
        # and run_provenance-style JSON beside it time the reference's other measured phase, model.evaluate (:170)
        eval_speed = {"eval_runtime": eval_runtime, "eval_samples": len(test_ds),
                      "eval_samples_per_second": round(len(test_ds) / max(eval_runtime, 1e-9), 2),
                      "eval_batch_size": per_rank_eval, "eval_sequences_per_forward": per_rank_eval_fwd,
                      "eval_hip_graph": trainer.eval_graph_active}
        logger.info(f"eval_runtime = {eval_speed}")
        if rank == 0:
            write_eval_results(args.output_data_dir, result)
            with open(os.path.join(args.output_data_dir, "eval_speed.json"), "w") as f:
                json.dump(eval_speed, f, indent=1)
        out["eval"] = result
        out["eval_speed"] = eval_speed

    # Q5: rank-0-only save, then barrier
    if rank == 0:
        # with --ema_decay the saved model is the averaged one (checkpoint-* directories keep the raw weights, with the
        # average in optimizer.pt, so a resume continues both)
        averaged = parts["optimizer"].ema_weights() if parts["optimizer"].ema is not None else contextlib.nullcontext()
        with averaged:
            save_pretrained(model, args.model_dir, state_dict=master_state_dict(model, parts["store"]))
        tokenizer.save_pretrained(args.model_dir)
    backend.barrier()
    out["global_step"] = trainer.global_step
    # tear the process group down explicitly: left to interpreter exit, the c10d / gloo threads are destroyed in
    # arbitrary order and a rank can abort ("terminate called without an active exception") after a good run
    backend.shutdown()
    return out
