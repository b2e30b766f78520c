"""The case table of tests/test_gpu_gemm_edges.py (GPU: every case against an fp64 reference inside guarded buffers) and
tests/test_gemm_edge_table.py (no GPU: every case against the launch planner, csrc/kernels/gemm_plan.h, at 256 CUs).

One row per case; every row names the kernel it is there for (``kernel``, ``targs``: the template arguments the planner
must choose under the row's knobs) and, for K-split rows, the slabs it claims (``splits`` launched, ``kps`` K elements
per slab). The shapes are the smallest at which each path can still go wrong: M at 1 and around the 128 / 256-row
tiles, main loops of one, two, three and five K-tiles, uneven K-split remainders, grids that are no multiple of the 8
XCDs, and one strided row per kernel family (leading dimensions 8 elements -- 16 fp8 bytes -- past the row).

``mode`` "exact": small-integer operands (``ra`` / ``rb`` / ``rbias`` / ``raux`` / ``rc0``: the closed ranges), every
product and partial sum an integer below 2^24, so fp32 accumulation is exact in any order and the output must equal the
rounded fp64 reference bit for bit. ``mode`` "bounded": randn operands against the per-element bound of
tests/test_gpu_gemm.py::_check (the erf / exp epilogues)."""

STORE, BIAS, BIAS_GELU, DROP_RES, RES, DGELU, F32_ATOMIC, F32_SLAB, GELU_D, MUL, RDOT = range(11)
EPI_NAME = {STORE: "store", BIAS: "bias", BIAS_GELU: "gelu", DROP_RES: "dropres", RES: "res", DGELU: "dgelu",
            F32_ATOMIC: "atomic", F32_SLAB: "slab", GELU_D: "gelud", MUL: "mul", RDOT: "rdot"}
BOUNDED = (BIAS_GELU, DGELU, GELU_D)
HAS_BIAS = (BIAS, BIAS_GELU, DROP_RES, GELU_D)
HAS_AUX = (DROP_RES, RES, DGELU, MUL, RDOT)
TWO_OUT = (BIAS_GELU, GELU_D)

EXACT_LIMIT = 2 ** 24

CASES = []


def _add(family, entry, kernel, targs, la, lb, epi, M, N, K, *, splits=1, exp=None, knobs=None, dbias=False, p=0.0,
         strided=False, launches=1, tag="", **extra):
    c = dict(family=family, entry=entry, kernel=kernel, targs=list(targs), la=la, lb=lb, epi=epi, M=M, N=N, K=K,
             req_splits=splits, splits=(exp or (1, K))[0], kps=(exp or (1, K))[1], knobs=dict(knobs or {}),
             dbias=dbias, p=p, strided=strided, launches=launches, accumulate=False, fa=0, q8=False, rd_seq=0,
             ra=3, rb=3, rbias=4, raux=3, rc0=5)
    c["mode"] = "bounded" if epi in BOUNDED else "exact"
    c.update(extra)
    bits = [family, EPI_NAME[epi] + ("+db" if dbias else "") + (f"+p{p}" if epi == DROP_RES else ""),
            f"{M}x{N}x{K}", f"l{la}{lb}"]
    if splits != 1:
        bits.append(f"s{splits}")
    if strided:
        bits.append("strided")
    if tag:
        bits.append(tag)
    c["id"] = "-".join(bits)
    CASES.append(c)
    return c


def _ceil(a, b):
    return -(-a // b)


# ---------------------------------------------------------------- gemm2_kernel: 256-row tiles, one pass
def _g2(M, N, K, epi, *, lb=0, bn=256, sync=4, **kw):
    return _add("g2", "gemm2", "gemm2_kernel", [0, lb, epi, bn, sync, 0], 0, lb, epi, M, N, K,
                knobs={"HSD_G2_SMALL": 0, "HSD_G2_SYNC": sync}, grid=_ceil(M, 256) * (N // bn),
                tag=f"sync{sync}", **kw)


# every schedule at one, two and three K-tiles (pipeline prologue and drain); M, N and the epilogue rotate
_G2_MN = [(1, 192, 192), (255, 256, 256), (257, 384, 192), (300, 512, 256)]
_G2_EPI = [dict(epi=STORE), dict(epi=BIAS), dict(epi=DROP_RES, p=0.5), dict(epi=RES), dict(epi=MUL)]
_i = 0
for _sync in (0, 1, 2, 4, 5, 6, 7):
    for _K in (64, 128, 192):
        _M, _N, _bn = _G2_MN[_i % 4]
        _g2(_M, _N, _K, bn=_bn, sync=_sync, **_G2_EPI[_i % 5])
        _i += 1
# five K-tiles, every epilogue, the fused column sums at an M edge, k-strided B (lb 1), grids of 3 and 6 workgroups
_g2(300, 384, 320, BIAS, bn=192)
_g2(257, 512, 320, RES)
_g2(255, 192, 320, DROP_RES, bn=192, p=0.0)
_g2(1, 256, 320, DROP_RES, p=0.5)
_g2(300, 256, 320, MUL, dbias=True)
_g2(257, 512, 64, MUL, dbias=True)
_g2(300, 256, 320, DGELU, dbias=True)
_g2(1, 192, 128, DGELU, bn=192)
_g2(257, 384, 320, BIAS_GELU, bn=192)
_g2(255, 512, 64, GELU_D)
_g2(257, 256, 192, STORE, lb=1)
_g2(300, 256, 64, RES, lb=1)
_g2(1, 256, 320, MUL, lb=1, dbias=True)
_g2(255, 256, 128, DGELU, lb=1)
_g2(600, 256, 128, BIAS)
_g2(600, 512, 192, STORE)
_g2(300, 384, 192, DROP_RES, bn=192, p=0.5, strided=True)
_g2(257, 256, 128, RES, lb=1, strided=True)
_g2(300, 256, 64, MUL, dbias=True, strided=True)


# ---------------------------------------------------------------- gemm2s_kernel: 128 x 128 tiles, one pass
def _g2s(M, N, K, epi, *, lb=0, stages=3, kw=2, **kwargs):
    return _add("g2s", "gemm2", "gemm2s_kernel", [0, lb, epi, stages, kw, 0], 0, lb, epi, M, N, K,
                knobs={"HSD_G2_SMALL": 1, "HSD_G2S_STAGES": stages, "HSD_G2S_KW": kw},
                grid=_ceil(M, 128) * (N // 128), tag=f"st{stages}kw{kw}", **kwargs)


# every (stages, waves) pair at one, two, three and five K-tiles: fewer K-tiles than stages, KW 2 on one K-tile
_G2S_MN = [(1, 256), (127, 384), (129, 256), (257, 384)]
_G2S_EPI = [dict(epi=BIAS), dict(epi=STORE), dict(epi=RES), dict(epi=DROP_RES, p=0.5), dict(epi=MUL),
            dict(epi=BIAS_GELU), dict(epi=GELU_D), dict(epi=DGELU)]
_i = 0
for _st, _kw in ((2, 1), (3, 1), (3, 2), (4, 1)):
    for _K in (64, 128, 192, 320):
        _M, _N = _G2S_MN[(_i + _i // 4) % 4]
        _g2s(_M, _N, _K, stages=_st, kw=_kw, **_G2S_EPI[_i % 8])
        _i += 1
_g2s(129, 256, 320, MUL, dbias=True)
_g2s(257, 256, 64, DGELU, dbias=True, stages=2, kw=1)
_g2s(127, 256, 128, DROP_RES, p=0.0, stages=4, kw=1)
_g2s(129, 128, 192, STORE, lb=1)
_g2s(1, 128, 64, RES, lb=1, stages=2, kw=1)
_g2s(257, 128, 320, MUL, lb=1, stages=3, kw=1)
_g2s(257, 384, 192, DROP_RES, p=0.5, strided=True)
_g2s(129, 128, 128, RES, lb=1, strided=True, stages=2, kw=1)


# ---------------------------------------------------------------- split-K NT: fp32 slabs + splitk_epi_kernel
def _splitk(M, N, K, splits, exp, epi, *, small, lb=0, **kwargs):
    knobs = {"HSD_G2_SMALL": int(small)}
    if small:
        tiles = _ceil(M, 128) * (N // 128)
        targs, kernel = [0, lb, F32_SLAB, 3, 2, 0], "gemm2s_kernel"
    else:
        tiles = _ceil(M, 256) * _ceil(N, 256)
        targs, kernel = [0, lb, F32_SLAB, 256, 4, 0], "gemm2_kernel"
    return _add("splitk", "gemm2", kernel, targs, 0, lb, epi, M, N, K, splits=splits, exp=exp, knobs=knobs,
                grid=tiles * exp[0], launches=2, second=("splitk_epi_kernel", [epi]),
                tag="small" if small else "big", **kwargs)


# K 320 / 3: slabs of 128, 128 and one K-tile; K 192 / 2: 128 + 64; K 320 / 4: three slabs launched, not four
_SK = [(320, 3, (3, 128)), (192, 2, (2, 128)), (320, 4, (3, 128))]
_SK_EPI = [dict(epi=STORE), dict(epi=BIAS), dict(epi=BIAS_GELU), dict(epi=DROP_RES, p=0.5), dict(epi=RES),
           dict(epi=DGELU), dict(epi=GELU_D), dict(epi=MUL), dict(epi=DROP_RES, p=0.0)]
_SK_M = [1, 33, 129, 300]
for _i, _e in enumerate(_SK_EPI):
    _K, _s, _exp = _SK[_i % 3]
    _splitk(_SK_M[_i % 4], (192, 256, 384)[(_i + _i // 3) % 3], _K, _s, _exp, small=False, **_e)
    _K, _s, _exp = _SK[(_i + 1) % 3]
    _splitk(_SK_M[(_i + 1) % 4], (256, 384)[_i % 2], _K, _s, _exp, small=True, **_e)
_splitk(300, 256, 320, 3, (3, 128), MUL, small=False, dbias=True)
_splitk(300, 256, 192, 2, (2, 128), MUL, small=True, dbias=True)
_splitk(300, 256, 320, 4, (3, 128), DGELU, small=False, dbias=True)
_splitk(300, 256, 320, 3, (3, 128), DGELU, small=True, dbias=True)
_splitk(129, 256, 192, 2, (2, 128), RES, small=False, lb=1)
_splitk(33, 384, 320, 3, (3, 128), BIAS, small=True, lb=1)
_splitk(300, 384, 320, 3, (3, 128), DROP_RES, small=False, p=0.5, strided=True)
_splitk(129, 256, 320, 4, (3, 128), MUL, small=True, dbias=True, strided=True)


# ---------------------------------------------------------------- gemm2pk_kernel: persistent NT, default knobs
def _pk(M, N, K, epi, *, bn=256, **kwargs):
    return _add("pk", "gemm2", "gemm2pk_kernel", [epi, bn], 0, 0, epi, M, N, K, grid=256, **kwargs)


# 257 tiles on a grid of 256 (the extra tile is one row), BN 192, and 129 x 2 tiles at two K-tiles
_pk(65537, 256, 64, BIAS)
_pk(65537, 256, 64, DROP_RES, p=0.5)
_pk(65537, 256, 64, MUL, dbias=True, ra=1, rb=1, raux=1)  # 65,537 rows of column sums stay below 2^24
_pk(65537, 192, 64, BIAS, bn=192)
_pk(32769, 512, 128, DROP_RES, p=0.5)
_pk(32769, 512, 128, MUL, dbias=True, ra=1, rb=1, raux=1, strided=True)


# ---------------------------------------------------------------- E2_STORE_RDOT: the attention backward's delta rows
def _rdot(B, S, K, path, *, lb=0, splits=1, exp=None, **kwargs):
    M, N = B * S, 256
    if path == "big":
        kernel, targs, knobs = "gemm2_kernel", [0, lb, RDOT, 256, 4, 0], {"HSD_G2_SMALL": 0}
        grid = _ceil(M, 256)
    elif path == "small":
        kernel, targs, knobs = "gemm2s_kernel", [0, lb, RDOT, 3, 2, 0], {"HSD_G2_SMALL": 1}
        grid = _ceil(M, 128) * 2
    elif path == "splitk-big":
        kernel, targs, knobs = "gemm2_kernel", [0, lb, F32_SLAB, 256, 4, 0], {"HSD_G2_SMALL": 0}
        grid = _ceil(M, 256) * exp[0]
    else:
        kernel, targs, knobs = "gemm2s_kernel", [0, lb, F32_SLAB, 3, 2, 0], {"HSD_G2_SMALL": 1}
        grid = _ceil(M, 128) * 2 * exp[0]
    two = path.startswith("splitk")
    return _add("rdot", "gemm2", kernel, targs, 0, lb, RDOT, M, N, K, splits=splits, exp=exp, knobs=knobs, grid=grid,
                rd_seq=S, launches=2 if two else 1, second=("splitk_epi_kernel", [RDOT]) if two else None,
                tag=f"{B}x{S}-{path}", **kwargs)


# 2 x 200 and 3 x 80 rows: a sequence boundary and the M edge inside one 256-row tile
_rdot(2, 200, 64, "big")
_rdot(3, 80, 64, "big", lb=1)
_rdot(3, 80, 64, "small")
_rdot(2, 200, 64, "small", lb=1)
_rdot(2, 200, 192, "splitk-big", splits=3, exp=(3, 64))
_rdot(3, 80, 192, "splitk-small", splits=3, exp=(3, 64), lb=1)
_rdot(2, 200, 64, "big", strided=True)


# ---------------------------------------------------------------- TT weight gradient (la = lb = 1): C += Aᵀ·B in fp32
def _tt(M, N, K, epi, splits, exp, *, small_tt, atomic=None, main_epi=None, **kwargs):
    knobs = {"HSD_G2_SMALL_TT": int(small_tt)}
    if atomic is not None:
        knobs["HSD_G2_TT_ATOMIC"] = int(atomic)
    small = bool(small_tt) and epi == F32_SLAB
    me = main_epi if main_epi is not None else epi
    if small:
        kern, targs, tiles = "gemm2s_kernel", [1, 1, me, 3, 2, 0], _ceil(M, 128) * (N // 128)
    else:
        kern, targs, tiles = "gemm2_kernel", [1, 1, me, 256, 4, 0], _ceil(M, 256) * (N // 256)
    two = exp[0] > 1 and me == F32_SLAB
    return _add("tt", "gemm2", kern, targs, 1, 1, epi, M, N, K, splits=splits, exp=exp, knobs=knobs,
                grid=tiles * exp[0], launches=2 if two else 1, second=("slab_reduce_kernel", []) if two else None,
                ws_numel=exp[0] * M * N if two else 0, tag="small" if small_tt else "big", **kwargs)


# 128 x 128 tiles: one split in place; 3 slabs of 128 + 128 + 64; automatic: 2 slabs of 192 + 128; 3 asked for at one
# K-tile: one slab, so in place
_tt(8, 128, 64, F32_SLAB, 1, (1, 64), small_tt=1)
_tt(136, 128, 320, F32_SLAB, 3, (3, 128), small_tt=1)
_tt(264, 256, 320, F32_SLAB, 0, (2, 192), small_tt=1)
_tt(264, 128, 64, F32_SLAB, 3, (1, 64), small_tt=1)
_tt(136, 256, 64, F32_SLAB, 1, (1, 64), small_tt=1, strided=True)
# 256-row tiles: one split in place or through atomics, slabs, automatic splits, the atomic epilogue split over K
_tt(8, 256, 64, F32_SLAB, 1, (1, 64), small_tt=0, atomic=0)
_tt(136, 256, 320, F32_SLAB, 1, (1, 320), small_tt=0, atomic=1, main_epi=F32_ATOMIC)
_tt(264, 256, 320, F32_SLAB, 3, (3, 128), small_tt=0)
_tt(136, 256, 320, F32_SLAB, 0, (2, 192), small_tt=0)
_tt(264, 256, 320, F32_ATOMIC, 3, (3, 128), small_tt=0)
_tt(8, 256, 64, F32_ATOMIC, 1, (1, 64), small_tt=1)
_tt(264, 256, 64, F32_SLAB, 1, (1, 64), small_tt=0, atomic=0, strided=True)
_tt(136, 256, 320, F32_SLAB, 3, (3, 128), small_tt=0, strided=True)


# ---------------------------------------------------------------- fp32-output NT (gemm2_f32nt): contiguous operands
def _f32nt(M, K, lb, exp, *, force=None):
    knobs = {"HSD_G2_SYNC": 4}
    if force is not None:
        knobs["HSD_F32NT_SPLITS"] = force
    two = exp[0] > 1
    return _add("f32nt", "gemm2", "gemm2_kernel", [0, lb, F32_SLAB, 256, 4, 0], 0, lb, F32_SLAB, M, 256, K, splits=0,
                exp=exp, knobs=knobs, grid=_ceil(M, 256) * exp[0], launches=2 if two else 1,
                second=("slab_reduce_kernel", []) if two else None, tag=f"f{force}" if force else "")


_f32nt(1, 64, 0, (1, 64))
_f32nt(257, 64, 1, (1, 64))
_f32nt(257, 1088, 0, (2, 576))  # automatic: two uneven slabs, 576 + 512
_f32nt(1, 1088, 1, (2, 576))
_f32nt(257, 320, 0, (3, 128), force=3)
_f32nt(1, 320, 1, (3, 128), force=3)


# ---------------------------------------------------------------- segmented K (gemm2_seg): C = Σ_s A_s · B_s, K = 3 · Kseg
def _seg(la, lb, M, N, Kseg, exp, *, accumulate=False, kernel="gemm2s_kernel", knobs=None, **kwargs):
    if kernel == "gemm2s_kernel":
        targs, tiles = [la, lb, F32_SLAB, 3, 2, 1], _ceil(M, 128) * (N // 128)
    else:
        targs, tiles = [la, lb, F32_SLAB, 256, 4, 1], _ceil(M, 256) * (N // 256)
    two = exp[0] > 1
    bits = [k.replace("HSD_", "").lower() + str(v) for k, v in (knobs or {}).items()]
    return _add("seg", "gemm2_seg", kernel, targs, la, lb, F32_SLAB, M, N, Kseg, splits=0, exp=exp, knobs=knobs,
                grid=tiles * exp[0], launches=2 if two else 1, second=("slab_reduce_kernel", []) if two else None,
                accumulate=accumulate, tag="-".join(bits + (["acc"] if accumulate else [])), **kwargs)


_BIG = "gemm2_kernel"
# NT forward / dgrad: 128-tile kernel (default) and 256-row tiles (HSD_SEG_NT_SMALL=0), written or accumulated
_seg(0, 0, 129, 256, 64, (1, 192))
_seg(0, 1, 257, 256, 320, (1, 960), accumulate=True)
_seg(0, 0, 257, 256, 320, (1, 960), accumulate=True, strided=True)
_seg(0, 1, 129, 256, 64, (1, 192))
_seg(0, 0, 257, 256, 64, (1, 192), kernel=_BIG, knobs={"HSD_SEG_NT_SMALL": 0}, accumulate=True)
_seg(0, 1, 129, 256, 320, (1, 960), kernel=_BIG, knobs={"HSD_SEG_NT_SMALL": 0})
_seg(0, 1, 257, 256, 64, (1, 192), kernel=_BIG, knobs={"HSD_SEG_NT_SMALL": 0}, strided=True)
# two K-splits of 512 + 448: the boundary falls inside the second segment [320, 640)
_seg(0, 0, 129, 256, 320, (2, 512), kernel=_BIG, knobs={"HSD_SEG_NT_SMALL": 0, "HSD_F32NT_SPLITS": 2})
_seg(0, 1, 257, 256, 320, (2, 512), kernel=_BIG, knobs={"HSD_SEG_NT_SMALL": 0, "HSD_F32NT_SPLITS": 2},
     accumulate=True)
# TT weight gradient: 128-tile kernel (one split in place; 7 asked for over 15 K-tiles: 5 slabs of 192), 256-row tiles
_seg(1, 1, 136, 128, 64, (1, 192), accumulate=True)
_seg(1, 1, 264, 256, 320, (5, 192), accumulate=True)
_seg(1, 1, 136, 256, 320, (5, 192), accumulate=True, strided=True)
_seg(1, 1, 264, 256, 64, (1, 192), kernel=_BIG, knobs={"HSD_G2_SMALL_TT": 0}, accumulate=True)
_seg(1, 1, 136, 256, 320, (5, 192), kernel=_BIG, knobs={"HSD_G2_SMALL_TT": 0}, accumulate=True)


# ---------------------------------------------------------------- fp8 gemm8pk_kernel (K in bytes; K-tiles of 128)
def _g8(M, N, K, epi, *, fa=0, bn=256, q8=False, **kwargs):
    return _add("g8", "gemm8", "gemm8pk_kernel", [epi, bn, fa, 0, int(q8)], 0, 0, epi, M, N, K, exp=(1, K // 2), fa=fa,
                q8=q8, grid=_ceil(M, 256) * (N // bn), ra=4, rb=4, tag=f"fa{fa}" + ("-q8" if q8 else ""), **kwargs)


_g8(1, 192, 128, STORE, bn=192)
_g8(255, 256, 256, BIAS, fa=1)
_g8(257, 384, 384, RES, bn=192)
_g8(300, 256, 128, DROP_RES, p=0.5, fa=1)
_g8(1, 384, 256, DROP_RES, p=0.0, bn=192)
_g8(255, 192, 384, MUL, bn=192, fa=1)
_g8(300, 256, 384, MUL, dbias=True)
_g8(257, 256, 128, MUL, dbias=True, fa=1)
_g8(300, 256, 256, RDOT, rd_seq=100, fa=1)
_g8(257, 384, 256, BIAS_GELU, bn=192)
_g8(300, 256, 128, DGELU, dbias=True, fa=1)
_g8(1, 192, 384, DGELU, bn=192)
_g8(255, 256, 256, GELU_D)
_g8(300, 256, 256, MUL, q8=True, fa=1)
_g8(300, 384, 256, BIAS, bn=192, strided=True)
_g8(257, 256, 128, MUL, dbias=True, strided=True)


# ---------------------------------------------------------------- fp8 gemm8tt_kernel (T tokens in K-tiles of 128)
def _g8tt(M, N, T, splits, exp, *, fdy=0, **kwargs):
    return _add("g8tt", "gemm8_wgrad", "gemm8tt_kernel", [fdy, 0], 1, 1, F32_SLAB, M, N, T, splits=splits, exp=exp,
                fa=fdy, grid=(M // 256) * (N // 256) * exp[0], launches=2, second=("slab_reduce_kernel", []),
                ws_numel=exp[0] * M * N, ra=4, rb=4, tag=f"fdy{fdy}", **kwargs)


_g8tt(256, 256, 128, 1, (1, 128))
_g8tt(256, 512, 128, 3, (1, 128), fdy=1)
_g8tt(256, 512, 384, 1, (1, 384))
_g8tt(256, 256, 384, 3, (3, 128), fdy=1)
_g8tt(256, 256, 640, 1, (1, 640), fdy=1)
_g8tt(256, 512, 640, 3, (3, 256))  # slabs of 256, 256 and 128
_g8tt(256, 256, 640, 3, (3, 256), fdy=1, strided=True)


# ---------------------------------------------------------------- gemm.hip, the fallback (no planner: launch_gemm picks
# the register-staged kernel for K % 64 != 0 or M / N < 128)
def _fb(M, N, K, la, lb, epi, *, splits=1, **kwargs):
    return _add("gemm", "gemm", "gemm_kernel", [la, lb, epi], la, lb, epi, M, N, K, splits=splits,
                exp=(splits, 0), **kwargs)


for _M, _N, _K in ((8, 8, 8), (136, 8, 72), (120, 264, 200)):
    _fb(_M, _N, _K, 0, 0, STORE)
    _fb(_M, _N, _K, 0, 0, BIAS)
    _fb(_M, _N, _K, 0, 0, DROP_RES, p=0.5)
    _fb(_M, _N, _K, 0, 1, STORE)
    _fb(_M, _N, _K, 0, 1, RES)
    for _la, _lb, _s in ((1, 1, 1), (0, 0, 3), (0, 1, 1), (1, 1, 3)):
        _fb(_M, _N, _K, _la, _lb, F32_ATOMIC, splits=_s)
_fb(120, 264, 200, 0, 0, BIAS, strided=True)
_fb(136, 8, 72, 1, 1, F32_ATOMIC, splits=3, strided=True)


def exact_bounds(c):
    """Worst-case magnitudes of an exact case from its value ranges: every intermediate the kernel holds in fp32 --
    a K-sum of products (x the fp8 dequantisation scale 2), the epilogue's sum or product, a fused column sum over M
    rows, a 64-column row dot -- must stay below 2^24 (integers that size are exact in fp32, in any order)."""
    K = 3 * c["K"] if c["family"] == "seg" else c["K"]
    acc = K * c["ra"] * c["rb"] * (2 if c["family"] in ("g8", "g8tt") else 1)
    epi = c["epi"]
    out = acc
    if epi in HAS_BIAS:
        out = acc + c["rbias"]
    if epi == DROP_RES:
        out = 2 * out + c["raux"]
    elif epi == RES:
        out = out + c["raux"]
    elif epi == MUL:
        out = out * c["raux"]
    elif epi in (F32_ATOMIC, F32_SLAB):
        out = acc + c["rc0"]
    worst = {"acc": acc, "out": out}
    if c["dbias"]:
        worst["dbias"] = c["M"] * out + c["rc0"]
    if epi == RDOT:
        worst["rd"] = 64 * acc * c["raux"]
    return worst


BY_ID = {c["id"]: c for c in CASES}
