"""Padding-free batches (``--pack_sequences``): the host side.

The reference pads every example to ``max_seq_length`` (``scripts/train.py:74-100``) and so do
``tokenization.encode_batch`` / ``datasets``. A padded key is masked and the loss reads only the first-token row
(or the masked-LM positions), so a padding row influences no valid row and receives a zero gradient: dropping
it changes neither loss nor gradients. :func:`pack_batch` drops them on the host: the ``B`` sequences of a batch
go back to back into one ``[T]`` buffer, sequence ``b`` in rows ``cu_seqlens[b] .. cu_seqlens[b+1]-1``, and the
whole step runs on ``T`` rows (``ops.attention_varlen`` walks the buffer by those offsets).

``T`` is the real token count rounded up to ``row_multiple`` (256): the weight-gradient GEMMs need a token
dimension that is a multiple of 64 (csrc/kernels/gemm_plan.h), 256 keeps whole 256-row NT tiles, and it bounds
the number of distinct shapes the GEMM planner and the caching allocator see. The rows past the last sequence
are *dead*: they belong to no sequence, hold the padding token, and every kernel output for them is zero.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np


def pack_batch(input_ids: np.ndarray, attention_mask: np.ndarray, labels: np.ndarray, *, pad_id: int, pos_base: int,
               pad_pos: int, row_multiple: int = 256, token_type_ids: Optional[np.ndarray] = None,
               span_labels: bool = False, row_targets: bool = False) -> Dict[str, object]:
    """Pack a right-padded ``[B, S]`` batch.

    ``position_ids[t] = pos_base + i`` for the ``i``-th token of its sequence (BERT / DistilBERT: ``pos_base = 0``,
    ``pad_pos = 0``; RoBERTa: ``pos_base = pad_token_id + 1``, ``pad_pos = pad_token_id``, what
    ``Embeddings.position_ids`` yields for a prefix mask). ``labels``: ``[B]`` (classification, returned as is) or
    ``[B, S]`` (masked LM, packed to ``[T]`` with -100 on the dead rows). ``span_labels=True``: ``labels`` are the
    ``[B, 2]`` (start, end) positions of question answering, relative to the sequence's first token and so the same
    numbers packed: returned as they are. ``row_targets=True``: ``labels`` are the fp32 ``[B, C]`` row targets of
    ``--problem_type`` regression / multi-label (one row per sequence, never ``[B, S]`` token labels, whatever
    ``C`` is): returned as they are. ``token_type_ids [B, S]``, when given, are packed to ``[1, T]`` (0 on the
    dead rows) and returned under that key.

    Returns ``input_ids [1, T]``, ``position_ids [1, T]`` (int64), ``cu_seqlens [B+1]`` (int32), ``labels`` and the
    host ints ``max_seqlen`` and ``real_tokens``.
    """
    ids = np.asarray(input_ids)
    mask = np.asarray(attention_mask)
    if ids.ndim != 2 or mask.shape != ids.shape:
        raise ValueError(f"pack_batch: input_ids {ids.shape} and attention_mask {mask.shape} must both be [B, S]")
    B, S = ids.shape
    valid = mask != 0
    lengths = valid.sum(axis=1).astype(np.int64)
    prefix = np.arange(S)[None, :] < lengths[:, None]
    bad = np.nonzero((lengths < 1) | (valid != prefix).any(axis=1))[0]
    if bad.size:
        b = int(bad[0])
        why = "is empty" if lengths[b] < 1 else "is not a right-padded prefix of ones"
        raise ValueError(f"pack_batch: attention_mask row {b} {why}")
    cu = np.zeros(B + 1, dtype=np.int32)
    cu[1:] = np.cumsum(lengths)
    t_real = int(cu[B])
    m = int(row_multiple)
    T = -(-t_real // m) * m
    out_ids = np.full(T, pad_id, dtype=np.int64)
    out_ids[:t_real] = ids[prefix]  # row-major: sequence by sequence, tokens in order
    pos = np.full(T, pad_pos, dtype=np.int64)
    pos[:t_real] = (np.broadcast_to(np.arange(S, dtype=np.int64), (B, S)) + pos_base)[prefix]
    lab = np.asarray(labels)
    if span_labels:
        if lab.shape != (B, 2):
            raise ValueError(f"pack_batch: span labels {lab.shape} must be [B, 2] = {(B, 2)}")
    elif row_targets:
        if lab.ndim != 2 or lab.shape[0] != B:
            raise ValueError(f"pack_batch: row targets {lab.shape} must be [B, C] with B = {B}")
    elif lab.ndim == 2:
        if lab.shape != ids.shape:
            raise ValueError(f"pack_batch: per-token labels {lab.shape} do not match input_ids {ids.shape}")
        packed = np.full(T, -100, dtype=np.int64)
        packed[:t_real] = lab[prefix]
        lab = packed
    out = {"input_ids": out_ids[None, :], "position_ids": pos[None, :], "cu_seqlens": cu, "labels": lab,
           "max_seqlen": int(lengths.max()), "real_tokens": t_real}
    if token_type_ids is not None:
        tt = np.asarray(token_type_ids)
        if tt.shape != ids.shape:
            raise ValueError(f"pack_batch: token_type_ids {tt.shape} do not match input_ids {ids.shape}")
        packed_tt = np.zeros(T, dtype=np.int64)
        packed_tt[:t_real] = tt[prefix]
        out["token_type_ids"] = packed_tt[None, :]
    return out


def unpack_rows(x: np.ndarray, cu_seqlens: np.ndarray, S: int) -> np.ndarray:
    """Packed rows ``x [T, ...]`` back to the padded ``[B, S, ...]`` layout, zero-filled (tests)."""
    x = np.asarray(x)
    cu = np.asarray(cu_seqlens).astype(np.int64)
    B = cu.shape[0] - 1
    out = np.zeros((B, S) + x.shape[1:], dtype=x.dtype)
    for b in range(B):
        n = int(cu[b + 1] - cu[b])
        out[b, :n] = x[cu[b]:cu[b + 1]]
    return out


def position_rule(cfg) -> Dict[str, int]:
    """``pad_id`` / ``pos_base`` / ``pad_pos`` of a model config (models/config.py) for :func:`pack_batch`."""
    pad = int(cfg.pad_token_id)
    if cfg.model_type == "roberta":
        return {"pad_id": pad, "pos_base": pad + 1, "pad_pos": pad}
    return {"pad_id": pad, "pos_base": 0, "pad_pos": 0}
