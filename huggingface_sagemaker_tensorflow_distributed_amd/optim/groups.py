"""Per-parameter learning-rate multipliers from the command line (``--layerwise_lr_decay``, ``--head_lr_multiplier``).

Layer-wise learning-rate decay (ELECTRA, BEiT, "Revisiting Few-sample BERT Fine-tuning"): the head trains at the full
rate and each encoder layer below it at a geometrically smaller one. With ``L = num_hidden_layers``:

* ``encoder.embeddings.*`` has depth 0, ``encoder.layers.i.*`` depth ``i + 1``, everything else (pooler,
  ``head_dense_*``, ``classifier_*``, ``qa_outputs_*``, ``lm_dense_*``, ``lm_ln_*``, ``lm_bias``) is the head, depth
  ``L + 1``.
* ``μ = D^(L + 1 - depth)`` for the embeddings and the encoder layers: the top layer gets ``D``, the embeddings
  ``D^(L+1)``. This is the BEiT / timm convention; ELECTRA's puts the head one step further away (depth ``L + 2``),
  so every encoder exponent is one larger there: the top layer gets ``D²``.
* ``μ = M`` for the head (a larger rate for the freshly initialised head).
* A tied weight is one parameter and has one depth: RoBERTa's MLM decoder is the word-embedding table, depth 0.

``μ`` is computed in Python floats; the optimizers round it to fp32 once (:class:`FusedAdam`'s ``lr_multipliers``). Pure
Python: nothing here touches a device.
"""
from __future__ import annotations

import math
import re
from typing import Dict, Iterable, List, Optional, Tuple

_LAYER = re.compile(r"^encoder\.layers\.(\d+)\.")
_FP32_MIN_NORMAL, _FP32_MAX = 2.0 ** -126, (2.0 - 2.0 ** -23) * 2.0 ** 127


def validate(decay, head_mul) -> Tuple[float, float]:
    """The two flags as floats, refused outside ``0 < D <= 1`` and finite ``M > 0`` (NaN fails every comparison)."""
    d = float(1.0 if decay is None else decay)
    m = float(1.0 if head_mul is None else head_mul)
    if not 0.0 < d <= 1.0:
        raise ValueError(f"--layerwise_lr_decay {d} must be in (0, 1] (1 = off; freezing layers is not supported)")
    if not (0.0 < m and math.isfinite(m)):
        raise ValueError(f"--head_lr_multiplier {m} must be finite and > 0 (1 = off)")
    return d, m


def param_depth(name: str, num_hidden_layers: int) -> int:
    """Depth of the parameter ``name``: 0 embeddings, ``i + 1`` encoder layer ``i``, ``L + 1`` the head."""
    L = int(num_hidden_layers)
    if name.startswith("encoder.embeddings."):
        return 0
    m = _LAYER.match(name)
    if m is not None:
        i = int(m.group(1))
        if not 0 <= i < L:
            raise ValueError(f"parameter {name!r}: layer {i} outside a model of {L} layers")
        return i + 1
    if name.startswith("encoder."):
        raise ValueError(f"parameter {name!r}: an encoder parameter that is neither an embedding nor in a layer")
    return L + 1


def depth_multiplier(depth: int, num_hidden_layers: int, decay: float, head_mul: float) -> float:
    L = int(num_hidden_layers)
    return float(head_mul) if depth == L + 1 else float(decay) ** (L + 1 - depth)


def lr_multipliers(names: Iterable[str], num_hidden_layers: int, decay: float = 1.0,
                   head_mul: float = 1.0) -> Optional[Dict[str, float]]:
    """``{parameter name: μ}`` for ``names`` (a store's segment names), or None when both flags are at 1 (off)."""
    d, m = validate(decay, head_mul)
    if d == 1.0 and m == 1.0:
        return None
    mul = {n: depth_multiplier(param_depth(n, num_hidden_layers), num_hidden_layers, d, m) for n in names}
    for n, mu in mul.items():
        if not _FP32_MIN_NORMAL <= mu <= _FP32_MAX:  # the optimizers keep μ in fp32, where it must stay > 0 and finite
            raise ValueError(f"--layerwise_lr_decay {d} / --head_lr_multiplier {m}: the multiplier {mu:g} of {n!r} "
                             f"is outside fp32's normal range")
    return mul


def depth_table(names: Iterable[str], numels: Iterable[int], num_hidden_layers: int, decay: float, head_mul: float,
                lr: float) -> List[Tuple[int, str, float, float, int]]:
    """Rows ``(depth, what, μ, lr·μ, parameters)`` by depth, for the startup log."""
    L = int(num_hidden_layers)
    count: Dict[int, int] = {}
    for n, k in zip(names, numels):
        dep = param_depth(n, L)
        count[dep] = count.get(dep, 0) + int(k)
    rows = []
    for dep in sorted(count):
        what = "embeddings" if dep == 0 else ("head" if dep == L + 1 else f"layer {dep - 1}")
        mu = depth_multiplier(dep, L, decay, head_mul)
        rows.append((dep, what, mu, float(lr) * mu, count[dep]))
    return rows


def format_table(rows) -> str:
    lines = [f"{'depth':>5}  {'parameters of':<13}  {'multiplier':>12}  {'learning rate':>13}  {'parameters':>12}"]
    for dep, what, mu, eff, k in rows:
        lines.append(f"{dep:>5}  {what:<13}  {mu:>12.6g}  {eff:>13.6g}  {k:>12,}")
    return "\n".join(lines)
