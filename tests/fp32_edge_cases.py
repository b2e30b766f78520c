"""Case tables, launch-geometry formulas, fp64 references and fp32 error bounds shared by tests/test_gpu_fp32_edges.py
(GPU: every fp32 step kernel of csrc/kernels/fp32.hip, and split2 of attention32m.hip, inside guarded buffers) and
tests/test_fp32_edge_references.py (no GPU: the references against ops/reference.py and fp32 autograd, the geometry
properties of every table row). Plain torch, device agnostic; nothing here touches the extension.

U = 2^-24 is the fp32 unit roundoff. The bounds are first order in U, with the second-order terms either written out
or covered by the factor SECOND = 1 + 2^-10 (every relative perturbation multiplied here is below 2^-10).
"""
import math

import torch

U = 2.0 ** -24
SECOND = 1.0 + 2.0 ** -10
MATH_MARGIN = 8.0  # device libm vs host libm: 8 x the host's worst measured ratio (module docstring of the GPU file)


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ launch geometry
def ew_blocks(n):
    """fp32.hip ew_blocks: blocks of 256 threads for n element groups."""
    return min(2048, max(1, ceil_div(n, 256)))


def split3_geometry(R, C):
    """(V, cvn, groups, stride) of launch_split3 / split3_kernel."""
    V = 8 if C % 8 == 0 else 4
    cvn = C // V
    groups = R * cvn
    return V, cvn, groups, ew_blocks(groups) * 256


def ew4_geometry(rows, W):
    """(W4, groups, stride) of epi32_kernel / dropout32_kernel on [rows][W]."""
    groups = rows * W // 4
    return W // 4, groups, ew_blocks(groups) * 256


def split2_geometry(n):
    """(groups, stride) of launch_split2 (attention32m.hip): at most 4096 blocks."""
    n4 = n // 4
    return n4, min(ceil_div(n4, 256), 4096) * 256


def colsum32_geometry(M, N):
    """(path, gx, grid y, rows per block) of launch_colsum32."""
    if N % 4 == 0:
        gx = ceil_div(N, 256)
        gy = max(1, min(min(1024, 2048 // gx), ceil_div(M, 256)))
        path = "vector"
    else:
        gx = ceil_div(N, 64)
        gy = max(1, min(1024, 2048 // gx))
        path = "scalar"
    rpb = ceil_div(M, gy)
    return path, gx, ceil_div(M, rpb), rpb


def ln32_nj(H):
    return 1 if H <= 256 else 2 if H <= 512 else 4


def ln32_bwd_geometry(R):
    """(rows per wave, waves with rows, waves launched) of launch_ln32_bwd."""
    rpw = max(1, (R + 1023) // 1024)
    waves = ceil_div(R, rpw)
    return rpw, waves, 4 * ceil_div(waves, 4)


# ------------------------------------------------------------------------------------------------ case tables
# split3 / split3_dual: (R, C, why)
SPLIT_SMALL = [
    (1, 8, "V = 8, one group"),
    (3, 8, "V = 8, cvn = 1: every group is a row"),
    (1, 40, "V = 8, cvn = 5, one row"),
    (3, 40, "V = 8, cvn = 5"),
    (1, 4, "V = 4, one group"),
    (3, 4, "V = 4, cvn = 1"),
    (1, 12, "V = 4, cvn = 3, one row"),
    (3, 12, "V = 4, cvn = 3"),
]
SPLIT_SECOND_TRIP = [
    (110000, 40, "V = 8 second trip, stride % cvn = 3: the column wrap"),
    (180000, 12, "V = 4 second trip, stride % cvn = 2"),
]
SPLIT_WIDE_ROW = (2, 8 * 600000, "a row wider than the grid: sr == 0, three trips")
SPLIT2_N = 4 * (4096 * 256 + 37)

# epi32 / dropout32 second trip
EW_SECOND_TRIP = (180000, 12)
EPI_SHAPES = [(1, 4), (3, 12), (5, 260)]
DROPOUT_SHAPES = [(1, 4), (7, 12), (2, 3, 20)]

COLSUM_VECTOR_M = [1, 3, 13, 16, 17, 255, 256, 257]
COLSUM_VECTOR_N = [4, 260]
COLSUM_LONG_M = [4097, 4100]  # 4097 = 17 x 241: odd blocks, none short; 4100: 17 blocks of 242, the last one 228 rows
COLSUM_SCALAR_N = [1, 63, 65, 130]
COLSUM_SCALAR_M = [1, 5, 1000]

LN_H = [4, 252, 256, 260, 512, 516, 768, 1020, 1024]
LN_R = [1, 3, 5]
LN_BWD_LONG = [(1025, 260), (2049, 516)]  # (R, H)

GATHER_H = [4, 260, 772, 1028]
SCATTER_H = [1, 63, 65, 768]
EMBED_R = [1, 5]

CLS_C = [1, 2, 8]
CLS_H = [2, 126, 128, 130, 768]
CLS_R = [1, 5]

ATTN_S = [2, 34, 62, 66]
ATTN_B, ATTN_HEADS = 2, 3
# "soft": a finite additive bias (-2.5) on every third key of sequence 0; the only case in which the bias value itself,
# and so its log2(e) factor, reaches the result (a -inf-like bias is clamped to -1e30 whatever its scale)
ATTN_MASKS = ["none", "tail", "full", "soft"]


# ------------------------------------------------------------------------------------------------ inputs
def wide_range_input(shape, seed, device):
    """fp32 values of magnitude 2^-100 .. 2^100 (24 random significand bits) with +0 and -0 sprinkled in. Subnormal
    results are outside the split's contract: |x| >= 2^-100 keeps x - hi (>= 2^-123 when not 0) a normal number."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    n = 1
    for d in shape:
        n *= d
    # a 1 Mi pattern tiled over large tensors (generated on the CPU so every device sees the same values)
    m = min(n, 1 << 20)
    e = torch.randint(-100, 100, (m,), generator=g)
    mant = 1.0 + torch.rand(m, generator=g, dtype=torch.float64)
    sign = torch.randint(0, 2, (m,), generator=g).double() * 2 - 1
    v = (sign * torch.ldexp(mant, e.to(torch.int32))).float()
    z = torch.randint(0, 16, (m,), generator=g)
    v = torch.where(z == 0, torch.zeros_like(v), v)
    v = torch.where(z == 1, -torch.zeros_like(v), v)
    v = v.to(device)
    if n > m:
        # 2^20 + 1 .. : an odd period so that no row or group stride lines up with the pattern
        v = torch.cat([v, v[:1]]).repeat(ceil_div(n, m + 1))[:n]
    return v.view(shape).contiguous()


def bits(t):
    """The raw bits of a float tensor (so that -0 != +0 and NaN == NaN)."""
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


# ------------------------------------------------------------------------------------------------ references
def split_halves(x):
    """hi = bf16(x), lo = bf16(x - hi): the bit-exact halves of an fp32 tensor."""
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    return hi, lo


def split3_ref(x, pat, rows):
    """Three blocks of x [R][C], block b = lo if (pat >> b) & 1 else hi, side by side ([R][3C]) or stacked ([3R][C])."""
    hi, lo = split_halves(x)
    blocks = [lo if (pat >> b) & 1 else hi for b in range(3)]
    return torch.cat(blocks, 0 if rows else 1).contiguous()


def gelu64(x):
    x = x.double()
    return 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5)))


def dgelu64(x):
    x = x.double()
    return 0.5 * (1.0 + torch.erf(x * math.sqrt(0.5))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu32_host(v):
    """epi32 kind 1's expression in fp32 on the host."""
    v = v.float().cpu()
    return 0.5 * v * (1.0 + torch.erf(v * 0.70710678118654752))


def dgelu32_host(v, x):
    """epi32 kind 4's expression in fp32 on the host."""
    v, x = v.float().cpu(), x.float().cpu()
    cdf = 0.5 * (1.0 + torch.erf(x * 0.70710678118654752))
    return v * (cdf + x * 0.3989422804014327 * torch.exp(-0.5 * x * x))


def gelu_unit(x):
    """Error unit of 0.5 x (1 + erf(x / sqrt 2)) in fp32: the roundings of erf and of 1 + erf are absolute (0.5 |x| U
    each), the products relative to the result."""
    return U * (x.double().abs() + gelu64(x).abs())


def dgelu_unit(v, x):
    """Error unit of v (Phi(x) + x phi(x)) in fp32: absolute roundings of size U inside the bracket, relative ones
    of the products."""
    return U * v.double().abs() * (1.0 + dgelu64(x).abs())


def host_ratio(host32, ref64, unit):
    """Worst |host fp32 evaluation - fp64| / unit over the elements with a non-zero unit (where the unit is 0 the
    result is determined exactly and compared with bound 0)."""
    err = (host32.double().cpu() - ref64.cpu()).abs()
    unit = unit.cpu()
    nz = unit > 0
    assert bool((err[~nz] == 0).all())
    return float((err[nz] / unit[nz]).max()) if bool(nz.any()) else 0.0


def ln_fwd_ref(x, g, b, eps):
    """fp64 LayerNorm of the fp32 rows x -> (out, mean, rstd, per-element bounds of the three) for a two-pass fp32
    kernel that sums in any grouping:
      mean:  (H - 1) U sum|x| / H for the sum, U |mean| for the division                              -> bm
      d = x - mean_computed: |d - D| <= bm + U (|D| + bm)                                            -> bd
      var:   sum over the row of bd (2 |D| + bd) / H, plus (H + 1) U relative (squares, sum, division) -> bv
      rstd:  rsqrt at var + eps -/+ (bv + U (var + eps)), plus `rsqrt_allow` U rstd for the call         -> br
      out = ((d rstd) g) + b: |g| (rstd bd + |D| br + bd br) + 3 U |xhat g| + U |out|, times SECOND.
    The rsqrt allowance is added by the caller (it is measured there)."""
    x64, g64, b64 = x.double(), g.double(), b.double()
    H = x.shape[1]
    mean = x64.mean(1)
    D = x64 - mean[:, None]
    var = (D * D).mean(1)
    rstd = (var + eps).rsqrt()
    out = D * rstd[:, None] * g64 + b64
    bm = U * ((H - 1) * x64.abs().sum(1) / H + mean.abs())
    bd = bm[:, None] + U * (D.abs() + bm[:, None])
    bv = (bd * (2 * D.abs() + bd)).sum(1) / H
    bv = bv + (H + 1) * U * (var + bv) + U * (var + eps)
    lo = (var + eps - bv).clamp_min(0.0).rsqrt()  # inf where the bound reaches 0: no upper limit on rstd there
    hi = (var + eps + bv).rsqrt()
    br = torch.maximum(lo - rstd, rstd - hi)
    return out, mean, rstd, dict(mean=bm, d=bd, rstd=br, D=D)


def ln_out_bound(ref_out, rstd, br, bd, D, g):
    g64 = g.double().abs()
    xh = (D * rstd[:, None]).abs()
    b = g64 * (rstd[:, None] * bd + D.abs() * br[:, None] + bd * br[:, None]) + 3 * U * xh * g64 + U * ref_out.abs()
    return b * SECOND


def ln_bwd_ref(dy, x, mean, rstd, g):
    """fp64 LayerNorm backward from the fp32 inputs (mean and rstd are inputs here) -> (dx, dgamma terms, dbeta terms,
    bound of dx). With A1 = mean|dy g| and A2 = mean|dy g xhat| over the row:
      xhat = (x - mean) rstd: 2 U |xhat|;  dy g: U |dy g|
      s1 = mean(dy g):       (H + 1) U A1;   s2 = mean(dy g xhat): (H + 4) U A2
      dx = rstd (dy g - s1 - xhat s2): rstd (2 U (|dy g| + |s1|) + bs1 + |xhat| bs2 + 4 U |xhat s2| + 2 U |inner|)
    dgamma / dbeta terms are returned per row ([R][H]); their sums are bounded by the caller."""
    dy64, x64, g64 = dy.double(), x.double(), g.double()
    H = x.shape[1]
    mu, rs = mean.double()[:, None], rstd.double()[:, None]
    xh = (x64 - mu) * rs
    dyg = dy64 * g64
    s1 = dyg.mean(1, keepdim=True)
    s2 = (dyg * xh).mean(1, keepdim=True)
    inner = dyg - s1 - xh * s2
    dx = rs * inner
    bs1 = (H + 1) * U * dyg.abs().mean(1, keepdim=True)
    bs2 = (H + 4) * U * (dyg * xh).abs().mean(1, keepdim=True)
    bdx = rs.abs() * (2 * U * (dyg.abs() + s1.abs()) + bs1 + xh.abs() * bs2 + 4 * U * (xh * s2).abs()
                      + 2 * U * inner.abs()) * SECOND
    return dx, dy64 * xh, dy64, bdx


def attention64(qkv, mask, B, S, heads, p, seed, keep_mask):
    """Plain fp64 softmax attention on qkv [B S][3 heads 64] (q | k | v) with an additive key mask [B][S] or None and
    the dropout keep mask of ops/rng.py (row (b heads + h) S + i, column j). Returns (out [B S][H], lse2 [B heads S]
    in the log2 domain, and the pieces the bounds need)."""
    d = 64
    H = heads * d
    x = qkv.double().view(B, S, 3, heads, d).permute(2, 0, 3, 1, 4)  # [3][B][h][S][d]
    q, k, v = x[0], x[1], x[2]
    s = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(d)
    if mask is not None:
        s = s + mask.double().view(B, 1, 1, S)
    pr = torch.softmax(s, dim=-1)
    lse2 = torch.logsumexp(s, dim=-1) * math.log2(math.e)
    ks = torch.ones_like(pr)
    if p > 0:
        ks = keep_mask(seed, (B * heads * S, S), p, device=qkv.device).view(B, heads, S, S).double()
        ks = ks * float(torch.tensor(1.0 / (1.0 - p), dtype=torch.float32))  # the kernels' fp32 scale
    o = torch.matmul(pr * ks, v)
    out = o.permute(0, 2, 1, 3).reshape(B * S, H)
    return out, lse2.reshape(B * heads * S), dict(q=q, k=k, v=v, s=s, pr=pr, ks=ks, o=o)


def attn_masks(kind, B, S, device):
    """(additive fp32 mask [B][S] or None, boolean key-kept [B][S]) of the mask cases: no mask; sequence 1 with its
    last S // 3 + 1 keys masked (at least one key stays); sequence 1 fully masked; a finite bias on some keys."""
    kept = torch.ones(B, S, dtype=torch.bool, device=device)
    if kind == "none":
        return None, kept
    if kind == "soft":
        mask = torch.zeros(B, S, device=device)
        mask[0, ::3] = -2.5
        return mask, kept
    if kind == "tail":
        kept[1, S - min(S - 1, S // 3 + 1):] = False
    else:
        kept[1, :] = False
    mask = (~kept).float() * torch.finfo(torch.float32).min
    return mask, kept


def cls_forward64(pre, W2, b2, act, keep, scale):
    """fp64 head: t = act(pre) keep scale, logits = t W2^T + b2."""
    a = torch.tanh(pre) if act == 0 else torch.relu(pre)
    t = a * keep * scale
    return t, t @ W2.t() + b2


def ce_rows64(logits, labels):
    """Per-row cross-entropy in fp64."""
    return torch.logsumexp(logits, 1) - logits.gather(1, labels[:, None])[:, 0]


def ce_rows32_host(logits32, labels):
    """cls32_fwd_kernel's expression in fp32 on the host: logf(sum expf(lg - mx)) + mx - lg[y]."""
    lg = logits32.float().cpu()
    lab = labels.cpu()
    mx = lg.max(1).values
    se = torch.zeros_like(mx)
    for c in range(lg.shape[1]):
        se = se + torch.exp(lg[:, c] - mx)
    return torch.log(se) + mx - lg.gather(1, lab[:, None])[:, 0]


def ce_unit(logits, labels):
    """Error unit of one row's cross-entropy: C exponentials in [0, 1] summed (absolute U each, the sum is >= 1 so the
    logarithm turns them into absolute errors of the same size), the logarithm itself, and the two additions."""
    lg = logits.double()
    C = lg.shape[1]
    mx = lg.max(1).values
    ly = lg.gather(1, labels[:, None])[:, 0]
    return U * (C + torch.logsumexp(lg - mx[:, None], 1).abs() + mx.abs() + ly.abs() + 1.0)


def dlogits64(logits, labels, g):
    lg = logits.double()
    onehot = torch.zeros_like(lg).scatter_(1, labels[:, None], 1.0)
    return (torch.softmax(lg, 1) - onehot) * g, onehot


def dlogits32_host(logits32, labels, dloss32, R):
    """cls32_bwd_kernel's expression in fp32 on the host."""
    lg = logits32.float().cpu()
    lab = labels.cpu()
    mx = lg.max(1, keepdim=True).values
    e = torch.exp(lg - mx)
    se = torch.zeros_like(mx)
    for c in range(lg.shape[1]):
        se = se + e[:, c:c + 1]
    onehot = torch.zeros_like(lg).scatter_(1, lab[:, None], 1.0)
    g = dloss32.float().cpu() / float(R)
    return (e / se - onehot) * g


def dlogits_unit(logits, labels, g):
    """Error unit of (softmax - onehot) g: the exponential's argument rounding is relative to |lg - mx|, the sum, the
    division, the subtraction and the product are relative to the values they produce."""
    lg = logits.double()
    pr = torch.softmax(lg, 1)
    onehot = torch.zeros_like(lg).scatter_(1, labels[:, None], 1.0)
    mx = lg.max(1, keepdim=True).values
    C = lg.shape[1]
    return U * abs(g) * (pr * (C + 2.0 + (lg - mx).abs()) + (pr - onehot).abs())


# ------------------------------------------------------------------------------------------------ guarded buffers
class Guard:
    """A contiguous tensor inside a larger 1-D allocation, PAD elements (>= 128 bytes, so the slice starts 16-byte
    aligned) in from either end. Pure outputs (init None) are pre-filled with NaN and must hold none afterwards;
    accumulate-into targets start from `init` between guards of a known value. check() requires both guards to be
    unchanged bit for bit."""
    PAD = 64
    KNOWN = 7.25

    def __init__(self, shape, dtype, device, init=None):
        shape = tuple(shape)
        n = 1
        for d in shape:
            n *= d
        self.pure = init is None
        self.buf = torch.full((n + 2 * self.PAD,), float("nan") if self.pure else self.KNOWN, dtype=dtype,
                              device=device)
        self.t = self.buf[self.PAD:self.PAD + n].view(shape)
        if init is not None:
            self.t.copy_(init)
        self.n = n
        self.before = (bits(self.buf[:self.PAD]).clone(), bits(self.buf[self.PAD + n:]).clone())
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == 0

    def check(self, what):
        lo, hi = bits(self.buf[:self.PAD]), bits(self.buf[self.PAD + self.n:])
        assert torch.equal(lo, self.before[0]), f"{what}: written below the output"
        assert torch.equal(hi, self.before[1]), f"{what}: written beyond the output"
        if self.pure:
            bad = int(torch.isnan(self.t.float()).sum())
            assert bad == 0, f"{what}: {bad} elements never written (or NaN)"
        return self.t


# ------------------------------------------------------------------------------------------------ attention bounds
LOG2E = math.log2(math.e)
LN2 = math.log(2.0)


def _attn_scores2(pc, mask, kept, B, S):
    """Log2-domain pieces of the streaming kernels: s2 = log2(e) (q.k / 8 + finite mask) over the kept keys (a fully
    masked sequence computes -1e30 for every key, exactly: treated as s2 = 0 with every key kept), the magnitude sum A
    of each score's 64 products, and the per-score bound
      bs = U (66 A + 2 |mb| + |s2|): q sl2 rounded, 64 fused multiply-adds, the mask's product and its addition."""
    q, k = pc["q"], pc["k"]
    full = ~kept.any(1)  # [B]
    eff_kept = (kept | full[:, None]).view(B, 1, 1, S)
    qk = torch.matmul(q, k.transpose(-1, -2)) / 8.0
    mb = torch.zeros(B, 1, 1, S, dtype=torch.float64, device=q.device)
    if mask is not None:
        mb = torch.where(kept, mask.double(), torch.zeros_like(mask.double())).view(B, 1, 1, S) * LOG2E
    s2 = qk * LOG2E + mb
    A = torch.matmul(q.abs(), k.abs().transpose(-1, -2)) / 8.0 * LOG2E
    fullv = full.view(B, 1, 1, 1)
    s2 = torch.where(fullv, torch.zeros_like(s2), s2)
    bs = torch.where(fullv, torch.zeros_like(s2), U * (66 * A + 2 * mb.abs() + s2.abs()))
    neg = torch.full_like(s2, -float("inf"))
    m = torch.where(eff_kept, s2, neg).max(-1, keepdim=True).values
    lo = torch.where(eff_kept, s2, -neg).min(-1, keepdim=True).values
    bs_max = torch.where(eff_kept, bs, torch.zeros_like(bs)).max(-1, keepdim=True).values
    return s2, bs, bs_max, m, m - lo, eff_kept, full


def attn_fwd_bounds(pc, mask, kept, B, S, heads, a_exp, a_log):
    """Per-element bounds of out [B S][H] and lse [B heads S] for attn32_fwd_kernel (online softmax over chunks of 4
    keys). With m the row maximum, `range` the spread of the kept scores and n_c = S / 4 + 1 chunks, each weight
    2^(s - m) carries the relative error
      rho = ln2 (2 bs_max + U (2 (m - s) + range)) + n_c (a_exp + 2) U
    (the score and the running maximum it is compared with, the roundings of s - m and of the rescale exponents, whose
    sum telescopes to at most the range, one exp2f and one product per chunk). Then
      out = N / l:  sum_k W |v| (rho + (S + 2) U) + |out| sum_k P (rho + S U) + 2 U |out|
      lse = m + log2 l: bs_max + (n_c (a_exp + 2) + S + 2 ln2 range) U / ln2 + a_log U max(1, |log2 l|) + U |lse|."""
    s2, bs, bs_max, m, rng, eff_kept, full = _attn_scores2(pc, mask, kept, B, S)
    nc = S / 4 + 1
    rho = LN2 * (2 * bs_max + U * (2 * (m - s2).abs() + rng)) + nc * (a_exp + 2) * U
    P, W, v, o = pc["pr"], pc["pr"] * pc["ks"], pc["v"], pc["o"]
    bN = torch.matmul(W * (rho + (S + 2) * U), v.abs())
    bl = (P * (rho + S * U)).sum(-1, keepdim=True)
    bo = (bN + o.abs() * bl + 2 * U * o.abs()) * SECOND
    l2 = torch.where(eff_kept, torch.exp2(s2 - m), torch.zeros_like(s2)).sum(-1, keepdim=True).log2()
    lse = m + l2
    blse = bs_max + (nc * (a_exp + 2) + S + 2 * LN2 * rng) * U / LN2 + a_log * U * l2.abs().clamp_min(1.0) + U * lse.abs()
    H = heads * 64
    return bo.permute(0, 2, 1, 3).reshape(B * S, H), (blse * SECOND).reshape(B * heads * S), full


def attn_bwd_bounds(pc, mask, kept, dout, lse_in, B, S, heads, a_exp):
    """Per-element bound of dqkv [B S][3 H] for attn32_bwd (delta, dQ, dV, dK passes) given the fp32 inputs o and lse
    (each within U of the exact value, a fully masked sequence's lse being the kernels' -1e30):
      p = exp2f(s - lse): rho' = ln2 (bs + U |lse| + U |s - lse|) + a_exp U   (2 U where every key is masked: p = 1, 1 / S)
      dP = dO.v: 65 U sum|dO v|;  delta = dO.O: 66 U sum|dO O|
      ds = p (keep dP - delta): |ds| (rho' + 2 U) + P (keep bdP + bdelta + U (|keep dP| + |delta|))
      dq = sum_k ds k / 8, dk = sum_q ds q / 8: the ds bounds through |k|, |q| plus (S + 5) U of the magnitude sums
      dv = sum_q p keep dO: P keep |dO| (rho' + (S + 2) U)."""
    s2, bs, bs_max, m, rng, eff_kept, full = _attn_scores2(pc, mask, kept, B, S)
    q, k, v, P, ks = pc["q"], pc["k"], pc["v"], pc["pr"], pc["ks"]
    dO = dout.double().view(B, S, heads, 64).permute(0, 2, 1, 3)
    lse = lse_in.double().view(B, heads, S, 1)
    fullv = full.view(B, 1, 1, 1)
    rho = LN2 * (bs + U * lse.abs() + U * (s2 - lse).abs()) + a_exp * U
    rho = torch.where(fullv, torch.full_like(rho, 2 * U), rho)
    dP = torch.matmul(dO, v.transpose(-1, -2))
    bdp = 65 * U * torch.matmul(dO.abs(), v.abs().transpose(-1, -2))
    delta = (dO * pc["o"]).sum(-1, keepdim=True)
    bdel = 66 * U * (dO * pc["o"]).abs().sum(-1, keepdim=True)
    ds = P * (ks * dP - delta)
    bds = ds.abs() * (rho + 2 * U) + P * (ks * bdp + bdel + U * ((ks * dP).abs() + delta.abs()))
    bdq = (torch.matmul(bds, k.abs()) + (S + 5) * U * torch.matmul(ds.abs(), k.abs())) / 8.0
    bdk = (torch.matmul(bds.transpose(-1, -2), q.abs()) + (S + 5) * U * torch.matmul(ds.abs().transpose(-1, -2), q.abs())) / 8.0
    bdv = torch.matmul((P * ks * (rho + (S + 2) * U)).transpose(-1, -2), dO.abs())
    b = torch.stack([bdq, bdk, bdv]) * SECOND  # [3][B][h][S][d]
    return b.permute(1, 3, 0, 2, 4).reshape(B * S, 3 * heads * 64)
