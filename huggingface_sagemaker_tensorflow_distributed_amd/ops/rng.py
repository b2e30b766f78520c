"""Counter-based dropout RNG shared bit-for-bit by the torch reference path and the HIP kernels.

Why counter-based: dropout masks are never stored; the backward kernels regenerate the mask of
element ``e`` from ``(seed, e)``. The reference's TF dropout draws from a
stateful Philox stream; we need the same *distribution* (Bernoulli keep with prob ``1-p``, scale
``1/(1-p)``) and determinism between forward and backward, not TF's exact bit stream.

Definition (mirrored in ``csrc/kernels/common.h``, dropout mask section). A dropout site of shape ``[..., W]`` is
viewed as ``[rows, W]``; element ``(r, c)`` belongs to column pair ``cp = c // 2`` of row ``r``:

* the site's 64-bit seed is mixed once into a 32-bit key ``k = mix32(seed_lo ^ mix32(seed_hi))``
  (``mix32`` = lowbias32, Wellons);
* the row word ``R(r) = mix32(r ^ k)`` (one full hash per ROW: kernels hold it in a register across the row);
* the column word ``C(cp) = clmul32(cp, 0x6D2B79F5)`` (carry-less product: GF(2)-linear, so kernels fold their
  lane / tile offsets into one register with XORs and every register offset is a compile-time constant);
* the pair's bits ``h = y ^ (y >> 16)`` with ``y = (R(r) ^ C(cp)) * 0x9E3779B1 mod 2^32``;
* column ``2cp`` keeps iff ``(h & 0xFFFF) >= thr``; column ``2cp+1`` keeps iff ``(h >> 16) >= thr``;
  ``thr = round(p * 65536)``.

Attention sites. Padded attention (``ops.attention``): probability element (batch ``b``, head ``h``, query ``i``,
key ``j``) is row ``(b*heads + h)*S + i``, column ``j``. Packed attention (``ops.attention_varlen``,
``--pack_sequences``): element (head ``h``, packed query row ``t``, key ``j`` counted within ``t``'s own sequence) is
row ``h*T + t``, column ``j``, with ``T`` the packed row count. ``keep(r, c)`` above does not depend on the row
width, so sequences of any (odd) length need no special case; the reference builds the mask at width
``max_seqlen`` and slices it. The backward regenerates the bits: no keep-mask buffer.

Per element pair a kernel spends one XOR, one multiply and one XOR (round 4: two lowbias32 multiplies, three
xor-shifts and the pair arithmetic per pair). Statistics: ``tests/test_rng.py`` (keep rate over 1e8 draws, neighbour
correlations, 2x2 block patterns), ``tools/rng_quality.py`` (the candidate screen).

MLM mask (``--mlm_masking dynamic``; mirrored in ``csrc/kernels/mlm_mask.hip``, :func:`mlm_mask_reference` is the torch
side). A batch is a flat buffer of ``N`` token ids: ``[B*S]`` when padded, the ``[T]`` rows of a packed batch otherwise.
With the 64-bit mask seed ``s`` (``DropoutSeeds.mlm_seed()``; a kernel XORs the process-wide device step seed into
its two words first, exactly as ``resolve_seed`` does for dropout) and ``key = site_key(s)``, flat index ``t`` draws
``w0 = pair_bits(key, row=t, cp=0)`` and ``w1 = pair_bits(key, row=t, cp=1)``:

* ``maskable(t)``: ``attention_mask[t] == 1`` (no mask for packed batches), ``id[t]`` is none of the special ids (up
  to 8: pad, bos/cls, eos/sep, mask) and the incoming ``labels[t] != -100`` (the loader marks shard-padding rows and
  packing's dead rows that way);
* ``selected(t)``: ``maskable(t)`` and ``(w0 & 0xFFFF) < round(p * 65536)``;
* replacement, with ``a = w0 >> 16``: ``a < 52429`` (``round(0.8 * 65536)``) -> ``mask_id``; ``a < 58982``
  (``round(0.9 * 65536)``) -> ``rand_lo + ((w1 * (rand_hi - rand_lo)) >> 32)`` (a 64-bit product); otherwise the token
  stays as it is;
* ``labels_out[t]`` is the original id where selected, -100 elsewhere.

The selected positions are compacted in ascending ``t`` into fixed-capacity buffers ``sel[cap]`` / ``tgt[cap]``
(``sel = 0``, ``tgt = -100`` from rank ``n`` on), ``inv[t]`` is the rank of ``t`` or -1, and
``cap = mlm_capacity(N, p)`` is a 5 sigma bound on the selected count computed from the shape alone. A selection of
rank ``>= cap`` is dropped: id unchanged, label -100, ``inv = -1``, counted in ``counts[1]``.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch

M32 = 0xFFFFFFFF
_C1 = 0x7FEB352D
_C2 = 0x846CA68B
DROP_C = 0x6D2B79F5
DROP_M = 0x9E3779B1


def _mul32(x: torch.Tensor, c: int) -> torch.Tensor:
    # (x * c) mod 2^32 without signed int64 overflow: split c into 16-bit halves.
    lo = c & 0xFFFF
    hi = c >> 16
    return (x * lo + (((x * hi) & 0xFFFF) << 16)) & M32


def mix32(x: torch.Tensor) -> torch.Tensor:
    x = x ^ (x >> 16)
    x = _mul32(x, _C1)
    x = x ^ (x >> 15)
    x = _mul32(x, _C2)
    x = x ^ (x >> 16)
    return x


def mix32_int(x: int) -> int:
    x &= M32
    x ^= x >> 16
    x = (x * _C1) & M32
    x ^= x >> 15
    x = (x * _C2) & M32
    x ^= x >> 16
    return x


def site_key(seed_lo: int, seed_hi: int) -> int:
    """32-bit key of a dropout site (``common.h::dropout_key``)."""
    return mix32_int((seed_lo & M32) ^ mix32_int(seed_hi & M32))


def drop_col(cp: torch.Tensor) -> torch.Tensor:
    """``C(cp)``: carry-less product of the column-pair index with DROP_C, mod 2^32."""
    out = torch.zeros_like(cp)
    for i in range(32):
        if (DROP_C >> i) & 1:
            out = out ^ ((cp << i) & M32)
    return out


def drop_col_int(cp: int) -> int:
    o = 0
    for i in range(32):
        if (DROP_C >> i) & 1:
            o ^= (cp << i) & M32
    return o


def drop_fin(x: torch.Tensor) -> torch.Tensor:
    y = _mul32(x, DROP_M)
    return y ^ (y >> 16)


def threshold(p: float) -> int:
    return int(round(p * 65536.0))


def pair_bits(key: int, rows: torch.Tensor, cps: torch.Tensor) -> torch.Tensor:
    """32 mask bits of column pair ``cps`` of row ``rows`` (int64 tensors, broadcast) for site key ``key``."""
    return drop_fin(mix32((rows & M32) ^ key) ^ drop_col(cps & M32))


def keep_mask(seed: int, shape, p: float, device=None, row_mul: int = 1) -> torch.Tensor:
    """Boolean keep mask of a dropout site of ``shape`` (a tuple / torch.Size; the last dimension is the row width W)
    with 64-bit ``seed``. ``row_mul``: row ``r`` of ``shape`` is row ``r * row_mul`` of the site (the first-token rows
    ``[B, W]`` of a ``[B * S, W]`` site: ``row_mul = S``; ``common.h`` ``DropoutParams::row_mul``)."""
    if isinstance(shape, int):
        raise TypeError("keep_mask: pass the site's shape (its last dimension is the mask's row width), not numel")
    shape = tuple(int(d) for d in shape)
    W = shape[-1] if shape else 1
    numel = 1
    for d in shape:
        numel *= d
    rows = numel // W if W else 0
    key = site_key(seed & M32, (seed >> 32) & M32)
    r = (torch.arange(rows, dtype=torch.int64, device=device) * int(row_mul)).unsqueeze(1)
    cp = torch.arange((W + 1) // 2, dtype=torch.int64, device=device).unsqueeze(0)
    h = pair_bits(key, r, cp)
    bits = torch.stack([h & 0xFFFF, h >> 16], dim=2).reshape(rows, -1)[:, :W]
    return (bits >= threshold(p)).reshape(shape)


class DropoutSeeds:
    """Hands out one 64-bit seed per dropout call site per step.

    Seeds are derived deterministically from ``(base_seed, step, call_index)`` so a replayed step
    (e.g. re-running forward for a check) regenerates identical masks, and data-parallel ranks can
    choose to share or decorrelate masks (``rank`` is mixed in by default, like independent TF
    replicas).
    """

    def __init__(self, base_seed: int = 0, rank: int = 0):
        self.base_seed = int(base_seed)
        self.rank = int(rank)
        self.step = 0
        self.calls = 0
        self.mlm_calls = 0

    def new_step(self, step: int | None = None) -> None:
        self.step = self.step + 1 if step is None else int(step)
        self.calls = 0
        self.mlm_calls = 0

    def mlm_seed(self) -> int:
        """The 64-bit seed of the next MLM masking call of this step, from ``(base_seed, step, rank, k)`` with ``k``
        the number of masking calls since :meth:`new_step` (each accumulation micro-batch masks once). A stream of
        its own: ``calls`` does not advance, so a dynamic step draws the dropout seeds of the static step."""
        a = mix32_int(self.base_seed ^ 0x3C6EF372)
        b = mix32_int(a ^ (self.step * 0x85EBCA6B + self.rank * 0xC2B2AE35))
        c = mix32_int(b ^ (self.mlm_calls * 0x27D4EB2F + 0x2F0B4A57))
        d = mix32_int(c ^ a ^ 0x7ED55D16)
        self.mlm_calls += 1
        return (c << 32) | d

    def mlm_eval_seed(self, index: int) -> int:
        """The mask seed of batch ``index`` of an evaluation: ``(base_seed, a constant, index)`` only, so every
        ``evaluate()`` scores the same masks whatever was trained in between."""
        a = mix32_int(self.base_seed ^ 0x1B873593)
        c = mix32_int(a ^ (int(index) * 0x27D4EB2F + 0x52DCE729))
        d = mix32_int(c ^ a ^ 0x38495AB5)
        return (c << 32) | d

    def next(self) -> int:
        a = mix32_int(self.base_seed ^ 0x9E3779B9)
        b = mix32_int(a ^ (self.step * 0x85EBCA6B + self.rank * 0xC2B2AE35))
        c = mix32_int(b ^ (self.calls * 0x27D4EB2F + 0x165667B1))
        d = mix32_int(c ^ a ^ 0x5BD1E995)
        self.calls += 1
        return (c << 32) | d


# ------------------------------------------------------------------------------------------ MLM mask
MLM_MASK_SHARE = 52429  # round(0.8 * 65536): a selected token becomes <mask>
MLM_RAND_SHARE = 58982  # round(0.9 * 65536): ... or, up to here, a random token; beyond, it stays


def mlm_capacity(n_tokens: int, p: float) -> int:
    """Rows of the fixed-capacity MLM head for ``n_tokens`` tokens masked with probability ``p``: the mean plus five
    standard deviations of the selected count (exceeded about 3e-7 of the time when every token is maskable), rounded
    up to whole 64-row GEMM tiles, at least 64. A function of the shape alone: no device value is read."""
    n, p = int(n_tokens), float(p)
    return max(64, 64 * int(math.ceil((n * p + 5.0 * math.sqrt(n * p * (1.0 - p)) + 1.0) / 64.0)))


@dataclass
class MlmMask:
    """What :func:`mlm_mask_reference` / ``ops.mlm_mask`` return (module docstring, "MLM mask")."""
    input_ids: torch.Tensor   # int64, the input's shape: the masked ids
    labels: torch.Tensor      # int64, the input's shape: the original id where selected, else -100
    sel: torch.Tensor         # int64 [cap]: the selected flat positions in ascending order, 0 from rank n on
    tgt: torch.Tensor         # int64 [cap]: their original ids, -100 from rank n on
    inv: torch.Tensor         # int32 [N]: the rank of a selected position, else -1
    counts: torch.Tensor      # int32 [2]: n (<= cap) and the selections dropped for want of capacity
    n_valid: torch.Tensor     # fp32 [1]: n
    cap: int


def mlm_mask_reference(input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor],
                       labels_in: Optional[torch.Tensor], seed: int, p: float, mask_id: int,
                       special_ids: Sequence[int], rand_range: Tuple[int, int], cap: Optional[int] = None,
                       step_seed: Optional[Tuple[int, int]] = None) -> MlmMask:
    """The MLM mask in torch, bit for bit what ``csrc/kernels/mlm_mask.hip`` computes: the CPU path of
    ``ops.mlm_mask`` and the kernels' test oracle. ``step_seed``: the two 32-bit words of the device step seed
    (``train/graph.py step_seed``) the kernels XOR into ``seed`` when one is set."""
    ids = input_ids.reshape(-1).long()
    N = ids.numel()
    dev = ids.device
    special_ids = [int(s) for s in special_ids]
    if len(special_ids) > 8:
        raise ValueError("mlm_mask: at most 8 special ids")
    rand_lo, rand_hi = int(rand_range[0]), int(rand_range[1])
    if not 0 <= rand_lo < rand_hi or rand_hi - rand_lo >= 1 << 31:
        raise ValueError(f"mlm_mask: rand_range {rand_range}")
    cap = mlm_capacity(N, p) if cap is None else int(cap)
    lo, hi = seed & M32, (seed >> 32) & M32
    if step_seed is not None:
        lo, hi = lo ^ (int(step_seed[0]) & M32), hi ^ (int(step_seed[1]) & M32)
    key = site_key(lo, hi)
    t = torch.arange(N, dtype=torch.int64, device=dev)
    w0 = pair_bits(key, t, torch.zeros_like(t))
    w1 = pair_bits(key, t, torch.ones_like(t))
    ok = torch.ones(N, dtype=torch.bool, device=dev)
    if attention_mask is not None:
        ok &= attention_mask.reshape(-1) != 0
    if labels_in is not None:
        ok &= labels_in.reshape(-1) != -100
    for s in special_ids:
        ok &= ids != s
    selected = ok & ((w0 & 0xFFFF) < threshold(p))
    rank = torch.cumsum(selected.to(torch.int64), 0) - 1
    total = int(selected.sum())
    take = selected & (rank < cap)
    n = min(total, cap)
    a = w0 >> 16
    rnd = rand_lo + ((w1 * (rand_hi - rand_lo)) >> 32)
    out = torch.where(a < MLM_MASK_SHARE, torch.full_like(ids, int(mask_id)), torch.where(a < MLM_RAND_SHARE, rnd, ids))
    out = torch.where(take, out, ids)
    labels = torch.where(take, ids, torch.full_like(ids, -100))
    pos = take.nonzero(as_tuple=True)[0]
    sel = torch.zeros(cap, dtype=torch.int64, device=dev)
    tgt = torch.full((cap,), -100, dtype=torch.int64, device=dev)
    sel[:n] = pos
    tgt[:n] = ids[pos]
    inv = torch.where(take, rank, torch.full_like(rank, -1)).to(torch.int32)
    counts = torch.tensor([n, total - n], dtype=torch.int32, device=dev)
    n_valid = torch.tensor([float(n)], dtype=torch.float32, device=dev)
    return MlmMask(out.view(input_ids.shape), labels.view(input_ids.shape), sel, tgt, inv, counts, n_valid, cap)
