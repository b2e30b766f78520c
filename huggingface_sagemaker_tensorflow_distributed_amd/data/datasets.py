"""Datasets: synthetic (default, no network) and local IMDB / SST-2 text.

Reference data path (``scripts/train.py:71-100``): ``load_dataset("imdb")``, tokenize with
``truncation=True``, pad every example to exactly ``tokenizer.model_max_length`` (512), keep
``input_ids``/``attention_mask``/``label`` — ``token_type_ids`` are never fed.

Offline here, so:

* ``synthetic``: a learnable binary task of the same tensor shapes. Label 1 sequences contain a
  "positive" marker token at a random position, label 0 sequences a "negative" one; real-length
  variation comes from a padded tail (or full length for throughput runs, which matches IMDB at
  S=128: almost every review is longer than 128 tokens and is truncated to full length).
* ``imdb`` / ``sst2`` / a path: read from a local directory (HF ``save_to_disk`` dir, parquet,
  csv/tsv, jsonl, or the raw ``aclImdb/{train,test}/{pos,neg}/*.txt`` tree).
"""
from __future__ import annotations

import glob
import json
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

POS_MARK = 2204  # "good" in bert-base-uncased's vocab
NEG_MARK = 2919  # "bad"


@dataclass
class ArrayDataset:
    input_ids: np.ndarray        # [N, S] int32
    attention_mask: np.ndarray   # [N, S] int8
    labels: np.ndarray           # [N] int64 (or [N, S] for MLM / token classification, [N, 2] for question answering)
    token_type_ids: Optional[np.ndarray] = None  # [N, S] segment ids (question answering with BERT), else None
    span_labels: bool = False    # labels are [N, 2] (start, end) token positions, not one label per row
    row_targets: bool = False    # labels are fp32 [N, C] row targets (--problem_type regression / multi-label)

    def __len__(self) -> int:
        return int(self.input_ids.shape[0])

    @property
    def seq_len(self) -> int:
        return int(self.input_ids.shape[1])


def synthetic_classification(num_examples: int, seq_len: int, vocab_size: int, seed: int = 0,
                             full_length: bool = False, num_labels: int = 2, cls_id: int = 101, sep_id: int = 102,
                             pad_id: int = 0) -> ArrayDataset:
    rng = np.random.default_rng(seed)
    lo = 1000 if vocab_size > 4000 else 4
    ids = rng.integers(lo, vocab_size, size=(num_examples, seq_len), dtype=np.int64)
    labels = rng.integers(0, num_labels, size=(num_examples,), dtype=np.int64)
    if full_length:
        lengths = np.full(num_examples, seq_len)
    else:
        lengths = rng.integers(max(4, seq_len // 4), seq_len + 1, size=num_examples)
    marks = np.array([POS_MARK, NEG_MARK] + [NEG_MARK + 1 + i for i in range(num_labels - 2)]) % vocab_size
    for i in range(num_examples):
        L = int(lengths[i])
        ids[i, 0] = cls_id % vocab_size
        ids[i, L - 1] = sep_id % vocab_size
        pos = int(rng.integers(1, max(2, L - 1)))
        ids[i, pos] = marks[labels[i]]
        ids[i, L:] = pad_id
    mask = (np.arange(seq_len)[None, :] < lengths[:, None]).astype(np.int8)
    return ArrayDataset(ids.astype(np.int32), mask, labels)


def regression_marker_table(vocab_size: int) -> np.ndarray:
    """The 16 marker token ids of the synthetic regression corpus: distinct, a function of ``vocab_size`` and a
    constant only, so the train and eval splits share them (as :func:`tag_table`)."""
    lo = 1000 if vocab_size > 4000 else 4
    return lo + np.random.default_rng([0x5E67, int(vocab_size)]).permutation(vocab_size - lo)[:16].astype(np.int64)


def multi_label_marker_table(vocab_size: int, num_labels: int) -> np.ndarray:
    """The marker token id of every label of the synthetic multi-label corpus (distinct; shared by the splits)."""
    lo = 1000 if vocab_size > 4000 else 4
    if num_labels > vocab_size - lo:
        raise ValueError(f"{num_labels} labels need as many marker ids; the vocabulary has {vocab_size - lo}")
    return lo + np.random.default_rng([0x3B17, int(vocab_size), int(num_labels)]).permutation(
        vocab_size - lo)[:num_labels].astype(np.int64)


def _marker_free_ids(rng, shape, vocab_size: int, markers: np.ndarray) -> np.ndarray:
    """Uniform filler tokens that are none of ``markers`` (a hit is moved to the next free id)."""
    lo = 1000 if vocab_size > 4000 else 4
    ids = rng.integers(lo, vocab_size, size=shape, dtype=np.int64)
    taken = np.zeros(vocab_size, dtype=bool)
    taken[markers] = True
    free = np.nonzero(~taken[lo:])[0] + lo
    hit = taken[ids]
    ids[hit] = free[ids[hit] % free.size]
    return ids


def synthetic_regression(num_examples: int, seq_len: int, vocab_size: int, seed: int = 0, num_labels: int = 1,
                         full_length: bool = False, cls_id: int = 101, sep_id: int = 102,
                         pad_id: int = 0) -> ArrayDataset:
    """``--problem_type regression --dataset synthetic``: one marker token, drawn from 16 fixed ids
    (:func:`regression_marker_table`) with index ``j``, at a random interior position of a ragged ``[CLS] … [SEP]``
    row; target ``y[c] = ((j·(2c+1)) mod 16) / 4 - 2``. ``labels`` fp32 ``[N, C]``."""
    rng = np.random.default_rng(seed)
    marks = regression_marker_table(vocab_size)
    ids = _marker_free_ids(rng, (num_examples, seq_len), vocab_size, marks)
    lengths = _ragged_lengths(rng, num_examples, seq_len, full_length)
    j = rng.integers(0, 16, size=num_examples)
    pos = 1 + (rng.integers(0, 1 << 30, size=num_examples) % np.maximum(lengths - 2, 1))
    ids[np.arange(num_examples), pos] = marks[j]
    mask = _frame(ids, lengths, cls_id % vocab_size, sep_id % vocab_size, pad_id)
    c = np.arange(num_labels)[None, :]
    y = ((j[:, None] * (2 * c + 1)) % 16) / 4.0 - 2.0
    return ArrayDataset(ids.astype(np.int32), mask, y.astype(np.float32), row_targets=True)


def synthetic_multi_label(num_examples: int, seq_len: int, vocab_size: int, seed: int = 0, num_labels: int = 6,
                          full_length: bool = False, cls_id: int = 101, sep_id: int = 102,
                          pad_id: int = 0) -> ArrayDataset:
    """``--problem_type multi_label_classification --dataset synthetic``: label ``c`` has its own marker id
    (:func:`multi_label_marker_table`) and is present independently with probability 1/4; the markers of a row go
    to distinct interior positions, and one that finds no free position is dropped (its label is 0). ``labels`` fp32
    ``[N, C]`` of 0 / 1."""
    rng = np.random.default_rng(seed)
    marks = multi_label_marker_table(vocab_size, num_labels)
    ids = _marker_free_ids(rng, (num_examples, seq_len), vocab_size, marks)
    lengths = _ragged_lengths(rng, num_examples, seq_len, full_length)
    want = rng.random((num_examples, num_labels)) < 0.25
    y = np.zeros((num_examples, num_labels), dtype=np.float32)
    for i in range(num_examples):
        interior = rng.permutation(np.arange(1, max(int(lengths[i]) - 1, 1)))
        cs = np.nonzero(want[i])[0][:interior.size]
        ids[i, interior[:cs.size]] = marks[cs]
        y[i, cs] = 1.0
    mask = _frame(ids, lengths, cls_id % vocab_size, sep_id % vocab_size, pad_id)
    return ArrayDataset(ids.astype(np.int32), mask, y, row_targets=True)


def synthetic_mlm(num_examples: int, seq_len: int, vocab_size: int, seed: int = 0, mask_id: int = 50264,
                  mlm_probability: float = 0.15, bos_id: int = 0, eos_id: int = 2) -> ArrayDataset:
    rng = np.random.default_rng(seed)
    ids = rng.integers(3, vocab_size, size=(num_examples, seq_len), dtype=np.int64)
    ids[:, 0] = bos_id
    ids[:, -1] = eos_id
    labels = np.full_like(ids, -100)
    sel = rng.random(ids.shape) < mlm_probability
    sel[:, 0] = sel[:, -1] = False
    labels[sel] = ids[sel]
    ids[sel] = mask_id % vocab_size
    return ArrayDataset(ids.astype(np.int32), np.ones_like(ids, dtype=np.int8), labels)


def _ragged_lengths(rng, num_examples: int, seq_len: int, full_length: bool) -> np.ndarray:
    if full_length:
        return np.full(num_examples, seq_len)
    return rng.integers(max(4, seq_len // 4), seq_len + 1, size=num_examples)  # as synthetic_classification


def _frame(ids: np.ndarray, lengths: np.ndarray, bos_id: int, eos_id: int, pad_id: int) -> np.ndarray:
    """<s> first, </s> last, padding after: the right-padded layout of every dataset here; returns the mask."""
    seq_len = ids.shape[1]
    rows = np.arange(ids.shape[0])
    ids[:, 0] = bos_id
    ids[rows, lengths - 1] = eos_id
    mask = np.arange(seq_len)[None, :] < lengths[:, None]
    ids[~mask] = pad_id
    return mask.astype(np.int8)


def synthetic_mlm_raw(num_examples: int, seq_len: int, vocab_size: int, seed: int = 0, bos_id: int = 0, eos_id: int = 2,
                      pad_id: int = 1, full_length: bool = False) -> ArrayDataset:
    """The unmasked variant of :func:`synthetic_mlm` for ``--mlm_masking dynamic``: i.i.d. uniform tokens (nothing to
    learn: the loss stays near log V), lengths uniform in ``[S/4, S]`` so ``--pack_sequences`` has padding to drop.
    ``labels`` is a placeholder: 0 on real tokens (the device masker reads only ``!= -100``), -100 on the padding."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(3, vocab_size, size=(num_examples, seq_len), dtype=np.int64)
    mask = _frame(ids, _ragged_lengths(rng, num_examples, seq_len, full_length), bos_id, eos_id, pad_id)
    labels = np.where(mask != 0, 0, -100).astype(np.int64)
    return ArrayDataset(ids.astype(np.int32), mask, labels)


def bigram_successor(vocab_size: int, seed: int = 0, lo: int = 3) -> np.ndarray:
    """``succ [V]``: a fixed random permutation of ``[lo, V)`` (identity below ``lo``), the ``synthetic-bigram``
    corpus' transition table; a function of ``(vocab_size, lo)`` and a constant only, so the training and the
    evaluation corpus share it whatever their seeds."""
    del seed  # one table per vocabulary: the corpus seed picks the sequences, not the language
    succ = np.arange(vocab_size, dtype=np.int64)
    succ[lo:] = lo + np.random.default_rng(0x5EED_B16A).permutation(vocab_size - lo)
    return succ


def synthetic_bigram(num_examples: int, seq_len: int, vocab_size: int, seed: int = 0, bos_id: int = 0, eos_id: int = 2,
                     pad_id: int = 1, follow: float = 0.9, full_length: bool = False) -> ArrayDataset:
    """``--dataset synthetic-bigram`` (masked-lm): a corpus with something to learn. ``x[i+1] = succ[x[i]]`` with
    probability ``follow``, uniform over ``[3, V)`` otherwise (:func:`bigram_successor`), so a masked token is
    predictable from its neighbours and the MLM loss can fall far below log V. Unmasked, ragged lengths, placeholder
    labels: the layout of :func:`synthetic_mlm_raw`."""
    rng = np.random.default_rng(seed)
    lo = 3
    succ = bigram_successor(vocab_size, lo=lo)
    fresh = rng.integers(lo, vocab_size, size=(num_examples, seq_len), dtype=np.int64)
    keep = rng.random((num_examples, seq_len)) < follow
    ids = fresh.copy()
    for i in range(2, seq_len):  # column by column: position 0 is <s>, the chain starts fresh at 1
        ids[:, i] = np.where(keep[:, i], succ[ids[:, i - 1]], fresh[:, i])
    mask = _frame(ids, _ragged_lengths(rng, num_examples, seq_len, full_length), bos_id, eos_id, pad_id)
    labels = np.where(mask != 0, 0, -100).astype(np.int64)
    return ArrayDataset(ids.astype(np.int32), mask, labels)


def tag_table(vocab_size: int, num_labels: int) -> np.ndarray:
    """``table [V]`` of the synthetic tagging corpus: a fixed random map token id -> ``[0, L)``, a function of
    ``(vocab_size, num_labels)`` and a constant only, so the train and eval splits share one language."""
    return np.random.default_rng([0x7A65, int(vocab_size), int(num_labels)]).integers(
        0, num_labels, size=vocab_size, dtype=np.int64)


def synthetic_token_classification(num_examples: int, seq_len: int, vocab_size: int, seed: int = 0,
                                   num_labels: int = 9, full_length: bool = False, ignore_fraction: float = 0.25,
                                   cls_id: int = 101, sep_id: int = 102, pad_id: int = 0) -> ArrayDataset:
    """``--task token-classification --dataset synthetic``: a learnable tagging corpus in the ``[CLS] … [SEP]`` layout
    of :func:`synthetic_classification`, lengths ragged in ``[S/4, S]``. ``tag[i] = (table[x[i]] + table[x[i-1]]) % L``
    (:func:`tag_table`; ``x[i-1]`` of the first real token is ``[CLS]``), so a token's tag depends on its left
    neighbour. ``labels [N, S]``: -100 on ``[CLS]``, ``[SEP]``, the padding and a seeded ``ignore_fraction`` of the
    real tokens (they stand in for word-continuation pieces: ignored rows are scattered, not only at the tail)."""
    rng = np.random.default_rng(seed)
    lo = 1000 if vocab_size > 4000 else 4
    ids = rng.integers(lo, vocab_size, size=(num_examples, seq_len), dtype=np.int64)
    lengths = _ragged_lengths(rng, num_examples, seq_len, full_length)
    drop = rng.random((num_examples, seq_len)) < ignore_fraction
    mask = _frame(ids, lengths, cls_id % vocab_size, sep_id % vocab_size, pad_id)
    table = tag_table(vocab_size, num_labels)
    tags = np.zeros_like(ids)
    tags[:, 1:] = (table[ids[:, 1:]] + table[ids[:, :-1]]) % num_labels
    pos = np.arange(seq_len)[None, :]
    real = (pos >= 1) & (pos < (lengths[:, None] - 1))
    labels = np.where(real & ~drop, tags, -100).astype(np.int64)
    return ArrayDataset(ids.astype(np.int32), mask, labels)


# ------------------------------------------------------------------------------------------ question answering
def answer_length_table(vocab_size: int) -> np.ndarray:
    """``table [V]`` of the synthetic question-answering corpus: a fixed random map token id -> ``[0, 4)``, a function
    of ``vocab_size`` and a constant only (the train and eval splits share it)."""
    return np.random.default_rng([0x51AD, int(vocab_size)]).integers(0, 4, size=vocab_size, dtype=np.int64)


def synthetic_question_answering(num_examples: int, seq_len: int, vocab_size: int, seed: int = 0,
                                 full_length: bool = False, segment_ids: bool = True, no_answer_fraction: float = 0.1,
                                 cls_id: int = 101, sep_id: int = 102, pad_id: int = 0) -> ArrayDataset:
    """``--task question-answering --dataset synthetic``: a learnable span corpus in the layout
    ``[CLS] q [SEP] context [SEP]``, lengths uniform in ``[S/4, S]`` (at least 12). The question ``q`` is ONE key token
    and the context holds it exactly once (keys and context tokens come from disjoint id ranges); the answer starts at
    the token after it and runs for ``1 + table[x[start]] % 4`` tokens (:func:`answer_length_table`). A seeded
    ``no_answer_fraction`` of the examples has no key in its context and the label ``(0, 0)`` (the ``[CLS]`` span of
    SQuAD v2). ``labels [N, 2]`` = (start, end) token indices; ``token_type_ids`` 0 on ``[CLS] q [SEP]`` and the
    padding, 1 on ``context [SEP]`` (``segment_ids=False``: none, for RoBERTa / DistilBERT)."""
    if seq_len < 12:
        raise ValueError(f"synthetic_question_answering needs seq_len >= 12, got {seq_len}")
    rng = np.random.default_rng(seed)
    lo = 1000 if vocab_size > 4000 else 4
    nkeys = max(1, (vocab_size - lo) // 4)
    ids = rng.integers(lo + nkeys, vocab_size, size=(num_examples, seq_len), dtype=np.int64)  # context tokens
    if full_length:
        lengths = np.full(num_examples, seq_len)
    else:
        lengths = rng.integers(max(12, seq_len // 4), seq_len + 1, size=num_examples)
    keys = rng.integers(lo, lo + nkeys, size=num_examples, dtype=np.int64)
    special = [cls_id % vocab_size, sep_id % vocab_size, pad_id]  # a key that is [SEP] would occur twice
    spare = [k for k in range(lo, lo + nkeys) if k not in special]
    if not spare:
        raise ValueError(f"synthetic_question_answering: vocab_size {vocab_size} leaves no key token")
    keys[np.isin(keys, special)] = spare[0]
    no_answer = rng.random(num_examples) < no_answer_fraction
    # the key sits at k in [3, len - 6]: the answer (at most 4 tokens from k + 1) ends before the final [SEP]
    where = 3 + (rng.random(num_examples) * (lengths - 8)).astype(np.int64)
    table = answer_length_table(vocab_size)
    labels = np.zeros((num_examples, 2), dtype=np.int64)
    rows = np.arange(num_examples)
    ids[:, 0] = cls_id % vocab_size
    ids[:, 1] = keys
    ids[:, 2] = sep_id % vocab_size
    ids[rows, lengths - 1] = sep_id % vocab_size
    has = ~no_answer
    ids[rows[has], where[has]] = keys[has]
    start = where + 1
    end = start + table[ids[rows, start]] % 4
    labels[has, 0] = start[has]
    labels[has, 1] = end[has]
    pos = np.arange(seq_len)[None, :]
    mask = pos < lengths[:, None]
    ids[~mask] = pad_id
    tt = ((pos >= 3) & mask).astype(np.int8) if segment_ids else None
    return ArrayDataset(ids.astype(np.int32), mask.astype(np.int8), labels, token_type_ids=tt, span_labels=True)


def read_squad(path: str) -> List[Dict[str, object]]:
    """SQuAD-format JSON (v1.1 or v2 layout: ``data[].paragraphs[].{context, qas[]}``) -> one dict per question:
    ``question``, ``context``, ``answers`` = list of ``(text, answer_start)`` (empty for a v2 ``is_impossible``
    question) and ``id``."""
    with open(path, encoding="utf-8") as f:
        doc = json.load(f)
    out: List[Dict[str, object]] = []
    for article in doc["data"]:
        for para in article["paragraphs"]:
            ctx = para["context"]
            for qa in para["qas"]:
                ans = [] if qa.get("is_impossible", False) else [(a["text"], int(a["answer_start"]))
                                                                 for a in qa.get("answers", [])]
                out.append({"id": qa.get("id", str(len(out))), "question": qa["question"].strip(), "context": ctx,
                            "answers": ans})
    return out


def squad_split_path(dataset_dir: str, split: str) -> str:
    pats = ["train*.json"] if split == "train" else ["dev*.json", "validation*.json", "test*.json"]
    for pat in pats:
        hits = sorted(glob.glob(os.path.join(dataset_dir or "", pat)))
        if hits:
            return hits[0]
    raise FileNotFoundError(f"--dataset squad: none of {pats} in --dataset_dir {dataset_dir!r}")


def tokenize_squad(tokenizer, examples: List[Dict[str, object]], max_length: int, doc_stride: int = 128,
                   segment_ids: bool = True, chunk: int = 256) -> ArrayDataset:
    """Questions and contexts -> windows of ``max_length`` tokens (``Tokenizer.encode_pairs``: only the context is
    truncated, a long context yields overlapping windows ``doc_stride`` tokens apart). ``labels [N, 2]``: the token
    positions, within the window, of the first answer's first and last character; ``(0, 0)`` for a window that does
    not hold the whole answer and for a question without one. ``example_index [N]`` (an attribute of the result) maps
    a window to its question."""
    ids, mask, tts, labels, owner = [], [], [], [], []
    for i in range(0, len(examples), chunk):
        part = examples[i:i + chunk]
        enc = tokenizer.encode_pairs([e["question"] for e in part], [e["context"] for e in part], max_length,
                                     doc_stride)
        off, sid = enc["offsets"], enc["sequence_ids"]
        lab = np.zeros((off.shape[0], 2), dtype=np.int64)
        for w in range(off.shape[0]):
            ans = part[int(enc["sample"][w])]["answers"]
            if not ans:
                continue
            text, a0 = ans[0]
            a1 = a0 + len(text)
            ctx = sid[w] == 1
            s = np.nonzero(ctx & (off[w, :, 0] <= a0) & (a0 < off[w, :, 1]))[0]
            e = np.nonzero(ctx & (off[w, :, 0] < a1) & (a1 <= off[w, :, 1]))[0]
            if s.size and e.size and s[0] <= e[-1]:
                lab[w] = (s[0], e[-1])
        ids.append(enc["input_ids"])
        mask.append(enc["attention_mask"])
        tts.append(enc["token_type_ids"])
        labels.append(lab)
        owner.append(enc["sample"] + i)
    ds = ArrayDataset(np.concatenate(ids), np.concatenate(mask), np.concatenate(labels),
                      token_type_ids=np.concatenate(tts).astype(np.int8) if segment_ids else None, span_labels=True)
    ds.example_index = np.concatenate(owner)
    return ds


# ------------------------------------------------------------------------------------------ CoNLL column files
def read_conll(path: str) -> Tuple[List[List[str]], List[List[str]]]:
    """CoNLL column format: one token per line, first column the word, last column the tag; a blank line ends a
    sentence; ``-DOCSTART-`` lines are skipped. Returns (sentences of words, sentences of tags)."""
    words: List[List[str]] = []
    tags: List[List[str]] = []
    w: List[str] = []
    t: List[str] = []
    with open(path, encoding="utf-8") as f:
        for line in f:
            cols = line.split()
            if not cols:
                if w:
                    words.append(w)
                    tags.append(t)
                    w, t = [], []
                continue
            if cols[0] == "-DOCSTART-":
                continue
            if len(cols) < 2:
                raise ValueError(f"{path}: a token line needs a word and a tag, got {line!r}")
            w.append(cols[0])
            t.append(cols[-1])
    if w:
        words.append(w)
        tags.append(t)
    return words, tags


def conll_split_path(dataset_dir: str, split: str) -> str:
    names = ["train.txt"] if split == "train" else ["test.txt", "validation.txt", "dev.txt"]
    for n in names:
        p = os.path.join(dataset_dir or "", n)
        if os.path.isfile(p):
            return p
    raise FileNotFoundError(f"--dataset conll: none of {names} in --dataset_dir {dataset_dir!r}")


def conll_tag_list(dataset_dir: str) -> List[str]:
    """``labels.txt`` (one tag per line) if present, else the sorted tags of the train split."""
    p = os.path.join(dataset_dir or "", "labels.txt")
    if os.path.isfile(p):
        with open(p, encoding="utf-8") as f:
            tags = [l.strip() for l in f if l.strip()]
    else:
        tags = sorted({t for sent in read_conll(conll_split_path(dataset_dir, "train"))[1] for t in sent})
    if len(tags) < 2:
        raise ValueError(f"--dataset conll: {len(tags)} tag(s) in {dataset_dir!r}")
    return tags


def tokenize_conll(tokenizer, words: List[List[str]], tags: List[List[str]], tag_list: List[str],
                   max_length: int, chunk: int = 1000) -> ArrayDataset:
    """Pre-tokenised sentences -> ``ArrayDataset`` with ``labels [N, S]``: a word's first piece carries its tag; its
    other pieces, the special tokens and the padding carry -100. Truncated and padded to ``max_length``."""
    tag_id = {t: i for i, t in enumerate(tag_list)}
    ids, mask, labels = [], [], []
    for i in range(0, len(words), chunk):
        enc = tokenizer.encode_words(words[i:i + chunk], max_length)
        ids.append(enc["input_ids"])
        mask.append(enc["attention_mask"])
        wid = enc["word_ids"]  # [n, S] int64, -1 on special tokens and padding
        lab = np.full(wid.shape, -100, dtype=np.int64)
        for r in range(wid.shape[0]):
            sent = tags[i + r]
            prev = -1
            for c in range(wid.shape[1]):
                k = int(wid[r, c])
                if k >= 0 and k != prev:
                    if sent[k] not in tag_id:
                        raise ValueError(f"tag {sent[k]!r} is not in the tag list {tag_list}")
                    lab[r, c] = tag_id[sent[k]]
                if k >= 0:
                    prev = k
        labels.append(lab)
    return ArrayDataset(np.concatenate(ids), np.concatenate(mask), np.concatenate(labels))


def mask_dataset_static(ds: ArrayDataset, seed: int, mlm_probability: float, mask_id: int, special_ids,
                        rand_range) -> ArrayDataset:
    """Mask a raw corpus ONCE with the reference masker (ops/rng.py mlm_mask_reference), one call per example with
    the example's index in the seed: ``--mlm_masking static`` on a raw corpus (``synthetic-bigram``)."""
    import torch

    from ..ops.rng import DropoutSeeds, mlm_mask_reference

    seeds = DropoutSeeds(seed)
    ids = np.array(ds.input_ids, dtype=np.int64)
    labels = np.full_like(ids, -100)
    for i in range(ids.shape[0]):
        m = mlm_mask_reference(torch.from_numpy(ids[i]), torch.from_numpy(ds.attention_mask[i].astype(np.int64)),
                               torch.from_numpy(ds.labels[i]), seeds.mlm_eval_seed(i), mlm_probability, mask_id,
                               special_ids, rand_range, cap=ids.shape[1])
        ids[i] = m.input_ids.numpy()
        labels[i] = m.labels.numpy()
    return ArrayDataset(ids.astype(np.int32), ds.attention_mask, labels)


# ------------------------------------------------------------------------------------------ text
def _row_targets(t: dict, problem_type: str, num_labels: int, path: str) -> List[List[float]]:
    """The float targets of a csv / json table: regression reads a float ``label`` (or ``label_0..label_{C-1}``);
    multi-label a ``labels`` list per row or ``label_0..label_{C-1}`` columns."""
    cols = [f"label_{c}" for c in range(num_labels)]
    if all(c in t for c in cols):
        rows = [[float(t[c][i]) for c in cols] for i in range(len(t[cols[0]]))]
    elif problem_type == "multi_label_classification" and "labels" in t:
        rows = [[float(v) for v in (json.loads(x) if isinstance(x, str) else x)] for x in t["labels"]]
    elif problem_type == "regression" and "label" in t:
        rows = [[float(x)] for x in t["label"]]
    else:
        want = "a float label column" if problem_type == "regression" else "a labels list"
        raise ValueError(f"{path}: --problem_type {problem_type} reads {want} or label_0..label_{num_labels - 1} columns")
    bad = [i for i, r in enumerate(rows) if len(r) != num_labels]
    if bad:
        raise ValueError(f"{path}: row {bad[0]} has {len(rows[bad[0]])} targets, --num_labels is {num_labels}")
    return rows


def _read_table(path: str, problem_type: Optional[str] = None, num_labels: int = 2) -> Tuple[List[str], list]:
    ext = os.path.splitext(path)[1].lower()
    if ext == ".parquet":
        import pyarrow.parquet as pq

        t = pq.read_table(path).to_pydict()
    elif ext in (".jsonl", ".json"):
        rows = [json.loads(l) for l in open(path) if l.strip()]
        t = {k: [r[k] for r in rows] for k in rows[0]}
    elif ext in (".csv", ".tsv"):
        import pandas as pd

        t = pd.read_csv(path, sep="\t" if ext == ".tsv" else ",").to_dict(orient="list")
    else:
        raise ValueError(f"unsupported dataset file {path}")
    text_key = "text" if "text" in t else "sentence"
    if problem_type in ("regression", "multi_label_classification"):
        return [str(x) for x in t[text_key]], _row_targets(t, problem_type, num_labels, path)
    return [str(x) for x in t[text_key]], [int(x) for x in t["label"]]


def load_text_split(name_or_path: str, split: str, dataset_dir: Optional[str] = None,
                    problem_type: Optional[str] = None, num_labels: int = 2) -> Tuple[List[str], list]:
    """``split`` in {"train", "test"}; SST-2's ``validation`` serves as its test split. ``problem_type`` regression /
    multi_label_classification: csv / tsv / json files yield float targets (``_row_targets``; rows of ``num_labels``
    floats) instead of int labels; the other layouts hold one class per text and are refused."""
    floats = problem_type in ("regression", "multi_label_classification")
    if floats and name_or_path in ("imdb", "sst2"):
        raise ValueError(f"--dataset {name_or_path} holds one class per text, not the float targets of "
                         f"--problem_type {problem_type}")
    roots = [p for p in (name_or_path, dataset_dir, os.path.join(dataset_dir or "", name_or_path)) if p]
    for root in roots:
        if not os.path.exists(root):
            continue
        if os.path.isfile(root):
            return _read_table(root, problem_type, num_labels)
        # HF datasets save_to_disk
        if not floats and os.path.isfile(os.path.join(root, "dataset_dict.json")):
            from datasets import load_from_disk

            dd = load_from_disk(root)
            sp = split if split in dd else ("validation" if split == "test" and "validation" in dd else split)
            d = dd[sp]
            key = "text" if "text" in d.column_names else "sentence"
            return list(d[key]), list(d["label"])
        cands = []
        for sp in ([split] if split == "train" else [split, "validation", "dev"]):
            cands += sorted(glob.glob(os.path.join(root, f"{sp}*.parquet")))
            cands += sorted(glob.glob(os.path.join(root, "*", f"{sp}*.parquet")))
            for ext in ("jsonl", "csv", "tsv"):
                cands += sorted(glob.glob(os.path.join(root, f"{sp}*.{ext}")))
        if cands:
            texts, labels = [], []
            for c in cands:
                t, l = _read_table(c, problem_type, num_labels)
                texts += t
                labels += l
            return texts, labels
        raw = os.path.join(root, split)
        if not floats and os.path.isdir(os.path.join(raw, "pos")):  # aclImdb layout
            texts, labels = [], []
            for lab, sub in ((0, "neg"), (1, "pos")):
                for f in sorted(glob.glob(os.path.join(raw, sub, "*.txt"))):
                    texts.append(open(f, encoding="utf-8").read())
                    labels.append(lab)
            return texts, labels
    raise FileNotFoundError(f"dataset {name_or_path!r} split {split!r} not found locally "
                            f"(no network: pass --dataset_dir or use --dataset synthetic)")


def tokenize_dataset(tokenizer, texts: List[str], labels: List[int], max_length: int,
                     chunk: int = 1000) -> ArrayDataset:
    ids, mask = [], []
    for i in range(0, len(texts), chunk):  # the reference maps in 1000-row batches
        enc = tokenizer.encode_batch(texts[i:i + chunk], max_length)
        ids.append(enc["input_ids"])
        mask.append(enc["attention_mask"])
    if len(labels) and isinstance(labels[0], (list, tuple, np.ndarray)):  # float row targets (--problem_type)
        return ArrayDataset(np.concatenate(ids), np.concatenate(mask), np.asarray(labels, dtype=np.float32),
                            row_targets=True)
    return ArrayDataset(np.concatenate(ids), np.concatenate(mask), np.asarray(labels, dtype=np.int64))
