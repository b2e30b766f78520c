"""BERT / RoBERTa / DistilBERT models with HF-identical checkpoint names.

Stands in for ``TFAutoModelForSequenceClassification.from_pretrained(name)``
(``scripts/train.py:117``, ``scripts/singe_node_train.py:43``): an encoder, the family's
sequence-classification head with a freshly initialised classifier, logits out. The RoBERTa MLM
model serves the ``roberta-large MLM`` north-star config (BASELINE.json configs[4]).

HF layout is produced by :meth:`hf_names`; internal storage fuses Q/K/V.
"""
from __future__ import annotations

import math
from typing import Dict, Iterator, Optional, Tuple

import torch
import torch.nn as nn

from .. import ops
from ..ops.rng import DropoutSeeds
from .config import ModelConfig, check_problem_type
from .encoder import EncoderLayer, _param, layer_hf_names


class Embeddings(nn.Module):
    def __init__(self, cfg: ModelConfig):
        super().__init__()
        H = cfg.hidden_size
        self.cfg = cfg
        self.word_embeddings = _param(cfg.vocab_size, H)
        self.position_embeddings = _param(cfg.max_position_embeddings, H)
        self.token_type_embeddings = _param(cfg.type_vocab_size, H) if cfg.type_vocab_size > 0 else None
        self.ln_weight = _param(H)
        self.ln_bias = _param(H)

    def position_ids(self, input_ids: torch.Tensor) -> torch.Tensor:
        B, S = input_ids.shape
        if self.cfg.model_type == "roberta":
            # HF create_position_ids_from_input_ids: padding_idx + cumsum over non-pad tokens
            pad = self.cfg.pad_token_id
            m = input_ids.ne(pad).int()
            return (torch.cumsum(m, dim=1).type_as(m) * m).long() + pad
        return self._cached("pos", input_ids, lambda: torch.arange(S, device=input_ids.device).unsqueeze(0)
                            .expand(B, S).contiguous())

    def _cached(self, kind: str, input_ids: torch.Tensor, make):
        """Per-shape constant id tensors (arange positions, zero token types), built once instead of every step."""
        key = (kind, tuple(input_ids.shape), input_ids.device)
        cache = self.__dict__.setdefault("_id_cache", {})
        t = cache.get(key)
        if t is None:
            if len(cache) > 16:
                cache.clear()
            t = cache[key] = make()
        return t

    def forward(self, input_ids, token_type_ids, rng: DropoutSeeds, training: bool,
                q8_for: Optional[torch.Tensor] = None, position_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``q8_for``: the first encoder layer's QKV weight (fp8 path: the embedding kernel writes its fp8 operand).
        ``position_ids``: given for packed batches (data/packing.py), where a row's position is not its column."""
        c = self.cfg
        pos = self.position_ids(input_ids) if position_ids is None else position_ids
        if token_type_ids is None and self.token_type_embeddings is not None:
            token_type_ids = self._cached("type0", input_ids, lambda: torch.zeros_like(input_ids))
        p = c.hidden_dropout_prob if training else 0.0
        return ops.embed_ln(input_ids, pos, token_type_ids, self.word_embeddings, self.position_embeddings,
                            self.token_type_embeddings, self.ln_weight, self.ln_bias, c.layer_norm_eps,
                            p, rng.next() if p else 0,
                            pos_is_arange=c.model_type != "roberta" and position_ids is None, q8_for=q8_for)


class Encoder(nn.Module):
    def __init__(self, cfg: ModelConfig):
        super().__init__()
        self.cfg = cfg
        self.embeddings = Embeddings(cfg)
        self.layers = nn.ModuleList([EncoderLayer(cfg) for _ in range(cfg.num_hidden_layers)])

    def forward(self, input_ids, attention_mask, token_type_ids, rng, training, *, cu_seqlens=None, max_seqlen=None,
                position_ids=None, first_token_only=False) -> torch.Tensor:
        """Padded: ``input_ids [B, S]`` -> ``[B, S, H]``. Packed (``cu_seqlens`` given, data/packing.py):
        ``input_ids`` / ``position_ids`` ``[1, T]``, no attention mask -> ``[T, H]``.

        ``first_token_only``: the caller reads only the first-token row of each sequence (the classification heads).
        The last layer then runs everything after its attention scores on those B rows and the result is
        ``[B, 1, H]`` -- where ``ops.attn_block_cls_ok`` takes the tensors (padded batch, even S, reference ops or
        bf16 HIP ops with fp8 off) and ``HSD_CLS_ROWS_ONLY`` is not 0; otherwise, and always without the flag, all
        hidden states ``[B, S, H]``."""
        if cu_seqlens is not None:
            return self._forward_packed(input_ids, attention_mask, token_type_ids, rng, training, cu_seqlens,
                                        max_seqlen, position_ids)
        B, S = input_ids.shape
        first_qkv = self.layers[0].qkv_weight if len(self.layers) else None
        h = self.embeddings(input_ids, token_type_ids, rng, training, q8_for=first_qkv).view(B * S, -1)
        mask_bias = ops.key_mask_bias(attention_mask) if attention_mask is not None else None
        n = len(self.layers)
        prune = bool(first_token_only and n and ops.CLS_ROWS_ONLY
                     and ops.attn_block_cls_ok(h, self.layers[-1].qkv_weight, B, S, self.cfg.num_attention_heads))
        for i, layer in enumerate(self.layers):
            h = layer(h, mask_bias, B, S, rng, training, self.layers[i + 1].qkv_weight if i + 1 < n else None,
                      first_token_only=prune and i == n - 1)
        return h.view(B, 1 if prune else S, -1)

    def _forward_packed(self, input_ids, attention_mask, token_type_ids, rng, training, cu_seqlens, max_seqlen,
                        position_ids) -> torch.Tensor:
        if attention_mask is not None:
            raise ValueError("a packed batch (cu_seqlens) takes no attention_mask: the offsets say which keys a "
                             "query sees")
        if position_ids is None or not max_seqlen:
            raise ValueError("a packed batch needs position_ids and max_seqlen (data/packing.py pack_batch)")
        if input_ids.dim() != 2 or input_ids.shape[0] != 1 or position_ids.shape != input_ids.shape:
            raise ValueError(f"a packed batch holds input_ids / position_ids [1, T], got {tuple(input_ids.shape)} / "
                             f"{tuple(position_ids.shape)}")
        T = input_ids.shape[1]
        cu = cu_seqlens.to(torch.int32)
        # the embedding kernels are row-wise with explicit position ids, so any [rows, cols] view of the T tokens
        # computes the same thing; 256 columns keeps their backward's launch geometry (one block column per position
        # of a chunk of rows) at the size it was tuned for instead of T one-row blocks
        cols = 256 if T % 256 == 0 else T
        tt = token_type_ids.view(-1, cols) if token_type_ids is not None else None
        h = self.embeddings(input_ids.view(-1, cols), tt, rng, training,
                            position_ids=position_ids.view(-1, cols)).view(T, -1)
        for layer in self.layers:
            h = layer(h, None, 1, T, rng, training, None, cu_seqlens=cu, max_seqlen=int(max_seqlen))
        return h


def _init_(module: nn.Module, cfg: ModelConfig, generator: Optional[torch.Generator] = None) -> None:
    """HF ``_init_weights``: N(0, initializer_range) for matrices/embeddings, zero bias, LN = (1, 0),
    zeroed padding rows ([dep: transformers/modeling_utils.py:2375-2420])."""
    std = cfg.initializer_range
    with torch.no_grad():
        for name, p in module.named_parameters():
            leaf = name.rsplit(".", 1)[-1]
            if any(t in ("ln", "ln1", "ln2") for t in leaf.split("_")):
                if leaf.endswith("weight"):
                    p.fill_(1.0)
                else:
                    p.zero_()
            elif leaf.endswith("bias"):
                p.zero_()
            else:
                p.normal_(0.0, std, generator=generator)
        emb = getattr(module, "encoder", None)
        if emb is not None:
            e = emb.embeddings
            if 0 <= cfg.pad_token_id < e.word_embeddings.shape[0]:
                e.word_embeddings[cfg.pad_token_id].zero_()
            if cfg.model_type == "roberta" and cfg.pad_token_id < e.position_embeddings.shape[0]:
                e.position_embeddings[cfg.pad_token_id].zero_()


_FAMILY = {"bert": "Bert", "roberta": "Roberta", "distilbert": "DistilBert"}  # HF's class-name prefix per model_type


class _Base(nn.Module):
    base_prefix = None  # HF's name of the base model: cfg.model_type, unless the class fixes it
    arch_suffix = None  # HF's class name is _FAMILY[cfg.model_type] + arch_suffix
    # --label_smoothing_factor (HF TrainingArguments.label_smoothing_factor): a training argument, not a model property;
    # the runner sets it on the object, it is never written to config.json. The single-label CE heads pass it on.
    label_smoothing = 0.0

    def __init__(self, cfg: ModelConfig):
        super().__init__()
        self.cfg = cfg
        if self.base_prefix is None:
            if cfg.model_type not in _FAMILY:
                raise KeyError(cfg.model_type)
            self.base_prefix = cfg.model_type
        self.encoder = Encoder(cfg)
        self.rng = DropoutSeeds(0)

    def _encode(self, input_ids, attention_mask, token_type_ids, cu_seqlens, max_seqlen, position_ids,
                first_token_only=False):
        return self.encoder(input_ids, attention_mask, token_type_ids, self.rng, self.training, cu_seqlens=cu_seqlens,
                            max_seqlen=max_seqlen, position_ids=position_ids, first_token_only=first_token_only)

    # ----------------------------------------------------------------- HF name mapping
    def _embedding_hf_names(self) -> Iterator[Tuple[str, str, Optional[int], int]]:
        b = self.base_prefix
        yield f"{b}.embeddings.word_embeddings.weight", "encoder.embeddings.word_embeddings", None, 1
        yield f"{b}.embeddings.position_embeddings.weight", "encoder.embeddings.position_embeddings", None, 1
        if self.encoder.embeddings.token_type_embeddings is not None:
            yield f"{b}.embeddings.token_type_embeddings.weight", "encoder.embeddings.token_type_embeddings", None, 1
        yield f"{b}.embeddings.LayerNorm.weight", "encoder.embeddings.ln_weight", None, 1
        yield f"{b}.embeddings.LayerNorm.bias", "encoder.embeddings.ln_bias", None, 1

    def _layer_hf_names(self):
        distil = self.cfg.model_type == "distilbert"
        mid = "transformer" if distil else "encoder"
        for i in range(self.cfg.num_hidden_layers):
            yield from layer_hf_names(f"{self.base_prefix}.{mid}.layer.{i}.", f"encoder.layers.{i}.", distil)

    def _head_hf_names(self):
        return iter(())

    def hf_names(self) -> Iterator[Tuple[str, str, Optional[int], int]]:
        yield from self._embedding_hf_names()
        yield from self._layer_hf_names()
        yield from self._head_hf_names()

    def architecture(self) -> str:
        return _FAMILY[self.cfg.model_type] + self.arch_suffix

    def num_parameters(self) -> int:
        return sum(p.numel() for p in self.parameters())


class TransformerForSequenceClassification(_Base):
    """BertForSequenceClassification / RobertaForSequenceClassification / DistilBertForSequenceClassification.

    ``cfg.problem_type`` picks the loss as HF's ``config.problem_type`` does: ``None`` /
    ``"single_label_classification"`` cross-entropy on int labels ``[B]``; ``"multi_label_classification"``
    BCE-with-logits and ``"regression"`` MSE on fp32 labels ``[B, num_labels]`` (``ops.reference.seq_loss``). Nothing
    reads a device value on the host on any of them. ``label_smoothing`` (``--label_smoothing_factor``) smooths the
    single-label cross-entropy, in training and in evaluation; the float-label types refuse it."""

    arch_suffix = "ForSequenceClassification"

    def __init__(self, cfg: ModelConfig):
        super().__init__(cfg)
        H, L = cfg.hidden_size, cfg.num_labels
        check_problem_type(cfg.problem_type)
        self.regression_tolerance = 0.5  # --regression_tolerance: |z - y| <= this on every target scores a hit
        if cfg.model_type == "bert":
            self.pooler_weight, self.pooler_bias = _param(H, H), _param(H)
        else:  # roberta classifier.dense / distilbert pre_classifier
            self.head_dense_weight, self.head_dense_bias = _param(H, H), _param(H)
        self.classifier_weight, self.classifier_bias = _param(L, H), _param(L)

    def _head_hf_names(self):
        mt = self.cfg.model_type
        if mt == "bert":
            yield "bert.pooler.dense.weight", "pooler_weight", None, 1
            yield "bert.pooler.dense.bias", "pooler_bias", None, 1
            yield "classifier.weight", "classifier_weight", None, 1
            yield "classifier.bias", "classifier_bias", None, 1
        elif mt == "roberta":
            yield "classifier.dense.weight", "head_dense_weight", None, 1
            yield "classifier.dense.bias", "head_dense_bias", None, 1
            yield "classifier.out_proj.weight", "classifier_weight", None, 1
            yield "classifier.out_proj.bias", "classifier_bias", None, 1
        else:
            yield "pre_classifier.weight", "head_dense_weight", None, 1
            yield "pre_classifier.bias", "head_dense_bias", None, 1
            yield "classifier.weight", "classifier_weight", None, 1
            yield "classifier.bias", "classifier_bias", None, 1

    def forward(self, input_ids, attention_mask=None, token_type_ids=None, labels=None, *, cu_seqlens=None,
                max_seqlen=None, position_ids=None):
        c = self.cfg
        training = self.training
        h = self._encode(input_ids, attention_mask, token_type_ids, cu_seqlens, max_seqlen, position_ids,
                         first_token_only=cu_seqlens is None)
        if cu_seqlens is not None:
            # packed [T, H]: the first-token row of sequence b is row cu_seqlens[b]
            h = h.index_select(0, cu_seqlens[:-1].long()).unsqueeze(1)  # [B, 1, H]
        # head on the [CLS] / <s> row (ops.cls_head: one fused kernel per direction after the dense GEMM on GPUs);
        # the dropout seeds are drawn in the same order as the unfused head always drew them
        if c.model_type == "bert":
            p = (c.classifier_dropout if c.classifier_dropout is not None else c.hidden_dropout_prob) if training else 0.0
            w1, b1, act, p_in, seed_in = self.pooler_weight, self.pooler_bias, "tanh", 0.0, 0
        elif c.model_type == "roberta":
            p = (c.classifier_dropout if c.classifier_dropout is not None else c.hidden_dropout_prob) if training else 0.0
            w1, b1, act, p_in = self.head_dense_weight, self.head_dense_bias, "tanh", p
            seed_in = self.rng.next() if p else 0
        else:
            p = c.seq_classif_dropout if training else 0.0
            w1, b1, act, p_in, seed_in = self.head_dense_weight, self.head_dense_bias, "relu", 0.0, 0
        seed = self.rng.next() if p else 0
        # logits without labels, else (loss, logits)
        if c.problem_type is None:
            return ops.cls_head(h, w1, b1, self.classifier_weight, self.classifier_bias, labels, act, p_in, seed_in, p,
                                seed, label_smoothing=self.label_smoothing)
        return ops.cls_head(h, w1, b1, self.classifier_weight, self.classifier_bias, labels, act, p_in, seed_in, p, seed,
                            problem_type=c.problem_type, tol=self.regression_tolerance,
                            label_smoothing=self.label_smoothing)


class TransformerForTokenClassification(_Base):
    """BertForTokenClassification / RobertaForTokenClassification / DistilBertForTokenClassification:
    ``logits = classifier(dropout(sequence_output))`` over every row (no pooler, no dense layer), mean CE over the
    rows whose label is not -100 (NER, POS tagging, chunking); ``label_smoothing`` > 0 makes it the smoothed CE
    (target ``(1-eps)·onehot + eps/num_labels``).

    Inputs: padded ``[B, S]`` ids with ``[B, S]`` labels (logits ``[B, S, L]``), or a packed ``[1, T]`` buffer with
    ``[T]`` labels (data/packing.py; logits ``[T, L]``). The head (``ops.token_head``) draws one dropout seed after
    the encoder's; its site is the flat ``[rows, H]`` buffer. Nothing reads a device value on the host, so the
    whole step captures into a graph (``graph_safe``)."""

    graph_safe = True
    arch_suffix = "ForTokenClassification"

    def __init__(self, cfg: ModelConfig):
        super().__init__(cfg)
        self.classifier_weight, self.classifier_bias = _param(cfg.num_labels, cfg.hidden_size), _param(cfg.num_labels)

    def _head_hf_names(self):
        yield "classifier.weight", "classifier_weight", None, 1
        yield "classifier.bias", "classifier_bias", None, 1

    def head_dropout(self) -> float:
        c = self.cfg
        if c.model_type == "distilbert":
            return c.hidden_dropout_prob  # HF DistilBertForTokenClassification: nn.Dropout(config.dropout)
        return c.classifier_dropout if c.classifier_dropout is not None else c.hidden_dropout_prob

    def forward(self, input_ids, attention_mask=None, token_type_ids=None, labels=None, *, cu_seqlens=None,
                max_seqlen=None, position_ids=None):
        h = self._encode(input_ids, attention_mask, token_type_ids, cu_seqlens, max_seqlen, position_ids)
        H = h.shape[-1]
        p = self.head_dropout() if self.training else 0.0
        seed = self.rng.next() if p else 0
        out = ops.token_head(h.reshape(-1, H), self.classifier_weight, self.classifier_bias, labels, p, seed,
                             label_smoothing=self.label_smoothing)
        shape = tuple(h.shape[:-1]) + (self.cfg.num_labels,)  # [B, S, L] padded, [T, L] packed
        if labels is None:
            return out.view(shape)
        loss, logits = out
        return loss, logits.view(shape)


class TransformerForQuestionAnswering(_Base):
    """BertForQuestionAnswering / RobertaForQuestionAnswering / DistilBertForQuestionAnswering (extractive, SQuAD-style):
    ``logits = qa_outputs(dropout(sequence_output))`` over every row, column 0 the start logit and column 1 the end
    logit, and per column a cross-entropy over the positions of each sequence (``ops.qa_head``).

    Inputs: padded ``[B, S]`` ids with mask (and ``token_type_ids`` for BERT), or a packed ``[1, T]`` buffer with
    ``cu_seqlens`` (data/packing.py); either way ``labels [B, 2]`` int64 = (start, end) token indices relative to the
    sequence's first token, so an example carries the same numbers padded or packed. Logits ``[B, S, 2]`` / ``[T, 2]``.
    A position ``< 0``, ``>= len`` or on a masked row is ignored.

    Unlike HF the softmax of a sequence runs over its REAL rows only (docs/PARITY.md): a padding row gets an exactly
    zero gradient and the packed step equals the padded one, as for every other task. On a batch without padding the
    loss is HF's. BERT and RoBERTa have no head dropout (no seed is drawn); DistilBERT uses ``qa_dropout``, its seed
    drawn after the encoder's, on the flat ``[rows, H]`` buffer. ``loss._hsd_pred`` holds the best span per sequence
    (``max_answer_length``), ``loss._hsd_stats`` the exact-match counts. Nothing reads a device value on the host
    (``graph_safe``)."""

    graph_safe = True
    arch_suffix = "ForQuestionAnswering"
    max_answer_length = 30

    def __init__(self, cfg: ModelConfig):
        super().__init__(cfg)
        self.qa_outputs_weight, self.qa_outputs_bias = _param(2, cfg.hidden_size), _param(2)

    def _head_hf_names(self):
        yield "qa_outputs.weight", "qa_outputs_weight", None, 1
        yield "qa_outputs.bias", "qa_outputs_bias", None, 1

    def head_dropout(self) -> float:
        return self.cfg.qa_dropout if self.cfg.model_type == "distilbert" else 0.0

    def _offsets(self, input_ids) -> torch.Tensor:
        B, S = input_ids.shape
        return self.encoder.embeddings._cached(
            "cu", input_ids, lambda: torch.arange(B + 1, device=input_ids.device, dtype=torch.int32) * S)

    def forward(self, input_ids, attention_mask=None, token_type_ids=None, labels=None, *, cu_seqlens=None,
                max_seqlen=None, position_ids=None):
        h = self._encode(input_ids, attention_mask, token_type_ids, cu_seqlens, max_seqlen, position_ids)
        H = h.shape[-1]
        p = self.head_dropout() if self.training else 0.0
        seed = self.rng.next() if p else 0
        if cu_seqlens is not None:
            cu, row_mask, longest = cu_seqlens, None, int(max_seqlen)
        else:
            cu, longest = self._offsets(input_ids), int(input_ids.shape[1])
            row_mask = attention_mask.reshape(-1) if attention_mask is not None else None
        out = ops.qa_head(h.reshape(-1, H), self.qa_outputs_weight, self.qa_outputs_bias, labels, cu, row_mask, p, seed,
                          self.max_answer_length, max_seqlen=longest)
        shape = tuple(h.shape[:-1]) + (2,)  # [B, S, 2] padded, [T, 2] packed
        if labels is None:
            logits, pred = out
            logits = logits.view(shape)
            logits._hsd_pred = pred
            return logits
        loss, logits = out
        return loss, logits.view(shape)


class RobertaForMaskedLM(_Base):
    """RoBERTa MLM (decoder tied to the word embeddings), for the roberta-large pretraining config."""

    base_prefix = "roberta"

    # --mlm_masking: "static" = the batch arrives masked (labels -100 off the masked positions) and the head gathers
    # the masked rows with a data-dependent size; "dynamic" = the batch arrives raw, forward() draws a fresh
    # 80 / 10 / 10 mask on the device every call (ops.mlm_mask) and the head runs on a fixed number of rows
    mlm_masking = "static"
    mlm_probability = 0.15
    mlm_eval_index = 0  # the evaluation loop's batch index (Trainer.evaluate): eval masks depend on nothing else

    @property
    def graph_safe(self) -> bool:
        """Static masking: the masked-token gather has a data-dependent size (no HIP-graph capture). Dynamic masking
        reads no device value on the host."""
        return self.mlm_masking == "dynamic"

    eval_graph_safe = False  # dynamic eval masks take a host seed per batch, which a replayed graph would freeze

    # The decoder's vocabulary dimension (tied word embeddings, lm_head.bias) is padded to a multiple of this many
    # rows: 50265 -> 50432 for RoBERTa, so every GEMM of the head (logits forward, its dgrad and the tied-embedding
    # weight gradient) tiles on the hand-written MFMA kernels. The padding rows stay exactly zero (zero init, zero
    # gradient), the loss and the returned logits cover the real vocabulary only, and checkpoints keep HF's shapes
    # (models/hf_io.py slices on save, zero-pads on load).
    VOCAB_PAD = 256

    def __init__(self, cfg: ModelConfig):
        super().__init__(cfg)
        H = cfg.hidden_size
        self.vocab = cfg.vocab_size
        self.vocab_padded = -(-cfg.vocab_size // self.VOCAB_PAD) * self.VOCAB_PAD
        if self.vocab_padded != self.vocab:
            self.encoder.embeddings.word_embeddings = _param(self.vocab_padded, H)
        self.lm_dense_weight, self.lm_dense_bias = _param(H, H), _param(H)
        self.lm_ln_weight, self.lm_ln_bias = _param(H), _param(H)
        self.lm_bias = _param(self.vocab_padded)

    def padded_rows(self):
        """Internal parameter -> its HF row count (the rows beyond it are the zero vocabulary padding)."""
        return {"encoder.embeddings.word_embeddings": self.vocab, "lm_bias": self.vocab}

    @torch.no_grad()
    def zero_padding_rows(self) -> None:
        self.encoder.embeddings.word_embeddings[self.vocab:].zero_()
        self.lm_bias[self.vocab:].zero_()

    def architecture(self) -> str:
        return "RobertaForMaskedLM"

    def _head_hf_names(self):
        yield "lm_head.dense.weight", "lm_dense_weight", None, 1
        yield "lm_head.dense.bias", "lm_dense_bias", None, 1
        yield "lm_head.layer_norm.weight", "lm_ln_weight", None, 1
        yield "lm_head.layer_norm.bias", "lm_ln_bias", None, 1
        yield "lm_head.bias", "lm_bias", None, 1

    def set_mlm_masking(self, mode: str, probability: float = 0.15) -> None:
        if mode not in ("static", "dynamic"):
            raise ValueError(f"mlm_masking {mode!r}")
        if not 0.0 < float(probability) <= 1.0:
            raise ValueError(f"mlm_probability {probability!r}")
        self.mlm_masking, self.mlm_probability = mode, float(probability)

    @property
    def mask_token_id(self) -> int:
        # RoBERTa's <mask> is the last id of its 50,265-token vocabulary; smaller test vocabularies fold it the way
        # data/datasets.py synthetic_mlm does
        return 50264 % self.vocab

    def mlm_special_ids(self):
        c = self.cfg
        ids = [c.pad_token_id, c.bos_token_id, c.eos_token_id, self.mask_token_id]
        return sorted({int(i) for i in ids if i is not None})

    def mlm_rand_range(self):
        """Random replacements are drawn from the ids above pad / bos / eos."""
        c = self.cfg
        lo = 1 + max(int(i) for i in (c.pad_token_id, c.bos_token_id, c.eos_token_id) if i is not None)
        return (min(lo, self.vocab - 1), self.vocab)

    def mask_batch(self, input_ids, attention_mask, labels, cap=None):
        """The dynamic mask of one batch (padded ``[B, S]`` or packed ``[1, T]`` ids; ``labels``: -100 marks rows that
        must stay unmasked). Training draws ``rng.mlm_seed()`` (a new one per call since ``rng.new_step``) and folds
        the device step seed in; evaluation draws ``rng.mlm_eval_seed(mlm_eval_index)``."""
        seed = self.rng.mlm_seed() if self.training else self.rng.mlm_eval_seed(self.mlm_eval_index)
        m = ops.mlm_mask(input_ids, attention_mask, labels, seed, self.mlm_probability, self.mask_token_id,
                         self.mlm_special_ids(), self.mlm_rand_range(), cap=cap, use_step_seed=self.training)
        if self.training:
            # selections dropped for want of head capacity, summed on the device; read where the trainer logs
            tot = self.__dict__.get("_mlm_dropped")
            if tot is None or tot.device != m.counts.device:
                tot = self.__dict__["_mlm_dropped"] = torch.zeros((), dtype=torch.int64, device=m.counts.device)
            tot.add_(m.counts[1])
        return m

    def mlm_dropped(self) -> int:
        """Selections dropped so far because a batch selected more than ``cap`` positions (reads the device)."""
        tot = self.__dict__.get("_mlm_dropped")
        return int(tot) if tot is not None else 0

    def forward(self, input_ids, attention_mask=None, token_type_ids=None, labels=None, *, cu_seqlens=None,
                max_seqlen=None, position_ids=None):
        c = self.cfg
        mask = None
        if labels is not None and self.mlm_masking == "dynamic":
            mask = self.mask_batch(input_ids, attention_mask, labels)
            input_ids = mask.input_ids
        h = self._encode(input_ids, attention_mask, token_type_ids, cu_seqlens, max_seqlen, position_ids)
        if cu_seqlens is not None:
            h = h.unsqueeze(0)  # packed [T, H] -> [1, T, H]; labels are the packed [T]
        B, S, H = h.shape
        x = h.view(B * S, H)
        wemb = self.encoder.embeddings.word_embeddings
        if mask is not None:
            # fixed-capacity head: the rows the device compacted, no host read (graph-safe)
            return ops.mlm_head_fixed(x, mask, self.lm_dense_weight, self.lm_dense_bias, self.lm_ln_weight,
                                      self.lm_ln_bias, c.layer_norm_eps, wemb, self.lm_bias, self.vocab,
                                      label_smoothing=self.label_smoothing)
        if labels is not None:
            # only masked positions feed the (large-vocab) decoder: dense + GELU -> LN -> tied decoder -> CE
            loss, logits = ops.mlm_head(x, labels.view(-1), self.lm_dense_weight, self.lm_dense_bias, self.lm_ln_weight,
                                        self.lm_ln_bias, c.layer_norm_eps, wemb, self.lm_bias, self.vocab,
                                        label_smoothing=self.label_smoothing)
            return loss, logits
        x = ops.linear_gelu(x, self.lm_dense_weight, self.lm_dense_bias)
        x = ops.layer_norm(x, self.lm_ln_weight, self.lm_ln_bias, c.layer_norm_eps)
        logits = ops.linear(x, wemb[:self.vocab], self.lm_bias[:self.vocab])
        return logits.view(B, S, -1)


def build_model(cfg: ModelConfig, task: str = "sequence-classification", seed: Optional[int] = 0,
                problem_type: Optional[str] = None) -> _Base:
    """``problem_type``: sets ``cfg.problem_type`` of a sequence-classification model (models/config.py); any other
    task refuses it."""
    if problem_type is not None:
        if task not in ("sequence-classification", "seq-cls"):
            raise ValueError(f"problem_type={problem_type!r} is for task sequence-classification, not {task!r}")
        cfg = cfg.replace(problem_type=check_problem_type(problem_type))
    if task in ("sequence-classification", "seq-cls"):
        m = TransformerForSequenceClassification(cfg)
    elif task in ("masked-lm", "mlm"):
        if cfg.model_type != "roberta":
            raise ValueError("masked-lm is provided for roberta configs")
        m = RobertaForMaskedLM(cfg)
    elif task in ("token-classification", "token-cls"):
        m = TransformerForTokenClassification(cfg)
    elif task in ("span-extraction", "qa"):
        # --task question-answering (models/hf_io.py from_pretrained maps the flag's name to this key). build_model
        # itself keeps refusing the string "question-answering", which tests/test_token_classification.py pins as its
        # example of a task this function does not know.
        m = TransformerForQuestionAnswering(cfg)
    else:
        raise ValueError(task)
    g = None
    if seed is not None:
        g = torch.Generator()
        g.manual_seed(int(seed))
    _init_(m, cfg, g)
    if hasattr(m, "zero_padding_rows"):
        m.zero_padding_rows()
    return m
