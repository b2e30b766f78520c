"""The MFMA GEMMs (gemm2.hip, gemm8, gemm.hip) at tile, K-split and stride edges against an fp64 reference.

One case table (tests/gemm_edge_cases.py; tests/test_gemm_edge_table.py checks it against the planner without a GPU).
Every case
* asserts through ``_C.gemm_plan`` that the kernel it is there for is what runs (it fails, never skips, otherwise);
* "exact" cases: small-integer operands, so every product and partial sum is an integer below 2^24 and fp32
  accumulation is exact in any order and under any K-split -- the output must equal the fp64 product, rounded where
  gemm_common.h documents a rounding (bf16(acc + bias), the epilogue, one bf16 rounding), bit for bit. The test checks
  that precondition on the operands it drew (|A| @ |B| and the bias / aux / C0 terms in fp64);
* "bounded" cases (erf / exp epilogues): randn operands against fp64 within test_gpu_gemm.py::_check's per-element bound;
* guards: every output (C, C2, dbias, rd, the caller's slab workspace, the fp8 copy) is a view inside a larger
  allocation filled with a NaN bit pattern, rows before and after it (and, strided cases, columns between its rows);
  the guards must come back bit-identical. Every input is a view inside a NaN-filled allocation, so a read past its
  logical extent that reaches a stored element shows as NaN. Nothing here relies on a fault."""
import math
import zlib

import pytest
import torch

import gemm_edge_cases as T
from test_gemm_edge_table import check_plan, plan_of
from test_gpu_gemm import _check, _gelu_grad  # the per-element bound of the existing GEMM tests

pytestmark = pytest.mark.gpu

LIMIT = float(T.EXACT_LIMIT)
SENTINEL = {torch.bfloat16: (torch.int16, 0x7FC1), torch.float32: (torch.int32, 0x7FC00001),
            torch.uint8: (torch.uint8, 0x7F)}  # NaN in bf16, fp32, e4m3 and e5m2
F8 = (torch.float8_e4m3fn, torch.float8_e5m2)
SA, SB = 4.0, 0.5  # fp8 dequantisation scales: powers of two, sa · sb = 2


def _C():
    from huggingface_sagemaker_tensorflow_distributed_amd.ops import hip

    return hip._C


class Guarded:
    """A [rows, cols] view (leading dimension cols + pad) with `g` guard rows before and after it, the whole allocation
    filled with the dtype's NaN bit pattern."""

    def __init__(self, rows, cols, dtype, dev, pad=0, g=2):
        it, self.sent = SENTINEL[dtype]
        self.raw = torch.full((rows + 2 * g, cols + pad), self.sent, dtype=it, device=dev)
        self.t = self.raw.view(dtype)[g:g + rows, :cols]
        self.outside = torch.ones(self.raw.shape, dtype=torch.bool, device=dev)
        self.outside[g:g + rows, :cols] = False

    def put(self, data):
        self.t.copy_(data)
        return self

    def intact(self):
        return bool((self.raw[self.outside] == self.sent).all())


def _vec(n, dtype, dev):
    return Guarded(1, n, dtype, dev)


def _rb(x):
    """fp64 -> bf16 (round to nearest even, as pack_bf2) -> fp64; exact cases hold fp32-exact values, so the fp32 step
    rounds nothing."""
    return x.float().bfloat16().double()


def _gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


class Run:
    """One case: operands and guarded buffers (prepare), the launch, and the checks."""

    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        self.gen = torch.Generator(device=dev)
        self.seed = zlib.crc32(c["id"].encode())
        self.gen.manual_seed(self.seed)
        self.exact = c["mode"] == "exact"
        self.bufs = {}
        self.fp8 = c["family"] in ("g8", "g8tt")
        self.pad = (16 if self.fp8 else 8) if c["strided"] else 0
        if c["epi"] in (T.F32_ATOMIC, T.F32_SLAB):
            self._prepare_f32()
        else:
            self._prepare_bf16()

    # ---- operands
    def _ints(self, shape, r, nonzero=False):
        v = torch.randint(-r, r + 1, shape, generator=self.gen, device=self.dev).double()
        return torch.where(v == 0, torch.ones_like(v), v) if nonzero else v

    def _randn(self, shape, scale=1.0):
        return torch.randn(shape, generator=self.gen, device=self.dev) * scale

    def _operand(self, name, shape, r, scale, fmt=None, pad=None):
        """A bf16 (or fp8, format `fmt`) operand inside a NaN-filled allocation; returns the stored values in fp64."""
        v = self._ints(shape, r) if self.exact else self._randn(shape, scale)
        pad = self.pad if pad is None else pad
        if fmt is None:
            q = v.float().bfloat16()
            self.bufs[name] = Guarded(shape[0], shape[1], torch.bfloat16, self.dev, pad).put(q)
            return q.double()
        q = v.float().to(F8[fmt])
        self.bufs[name] = Guarded(shape[0], shape[1], torch.uint8, self.dev, pad).put(q.view(torch.uint8))
        return q.double()

    def _vector(self, name, n, r, dtype=torch.bfloat16, nonzero=False):
        v = self._ints((n,), r, nonzero) if self.exact else self._randn((n,))
        q = v.float().to(dtype)
        self.bufs[name] = _vec(n, dtype, self.dev).put(q.view(1, n))
        return q.double()

    def t(self, name):
        b = self.bufs.get(name)
        return None if b is None else b.t

    def v(self, name):
        b = self.bufs.get(name)
        return None if b is None else b.t[0]

    # ---- bf16-output GEMMs: C = epilogue(A · Bᵀ)
    def _prepare_bf16(self):
        c, dev = self.c, self.dev
        M, N, K, epi = c["M"], c["N"], c["K"], c["epi"]
        fa = c["fa"] if self.fp8 else None
        a = self._operand("A", (M, K) if c["la"] == 0 else (K, M), c["ra"], 1.0, fa)
        b = self._operand("B", (N, K) if c["lb"] == 0 else (K, N), c["rb"], 0.1 if not self.fp8 else 0.5,
                          0 if self.fp8 else None)
        a = a if c["la"] == 0 else a.t()
        b = b.t() if c["lb"] == 0 else b
        dq = SA * SB if self.fp8 else 1.0
        self.acc = (a @ b) * dq
        self.absacc = (a.abs() @ b.abs()) * dq
        self.bias = self._vector("bias", N, c["rbias"]) if epi in T.HAS_BIAS else None
        self.aux = None
        if epi in T.HAS_AUX:
            self.aux = self._operand("aux", (M, N), c["raux"], 1.0)
        self.bufs["C"] = Guarded(M, N, torch.bfloat16, dev, 0 if c["q8"] else self.pad)
        if epi in T.TWO_OUT:
            self.bufs["C2"] = Guarded(M, N, torch.bfloat16, dev, self.pad)
        self.db0 = self._vector("dbias", N, c["rc0"], torch.float32, nonzero=True) if c["dbias"] else None
        if epi == T.RDOT:
            self.bufs["rd"] = _vec(M * (N // 64), torch.float32, dev)
        if c["q8"]:
            self.bufs["q8"] = Guarded(M, N, torch.uint8, dev)
            self.q8_amax = torch.tensor([300.0], device=dev)
            self.q8_sinv = torch.zeros(1, device=dev)
            self.q8_track = torch.zeros(1, device=dev)
        if self.fp8:
            self.sa, self.sb = torch.tensor([SA], device=dev), torch.tensor([SB], device=dev)
        self.keep = None
        if epi == T.DROP_RES and c["p"] > 0:
            from huggingface_sagemaker_tensorflow_distributed_amd.ops.reference import keep_mask

            self.keep = keep_mask(self.seed, (M, N), c["p"], device=dev).double() * (1.0 / (1.0 - c["p"]))

    # ---- fp32-output GEMMs: C (+)= A · B
    def _prepare_f32(self):
        c, dev = self.c, self.dev
        M, N, K, fam = c["M"], c["N"], c["K"], c["family"]
        nseg = 3 if fam == "seg" else 1
        self.acc = torch.zeros(M, N, dtype=torch.float64, device=dev)
        self.absacc = torch.zeros_like(self.acc)
        for s in range(nseg):
            sfx = str(s) if fam == "seg" else ""
            a = self._operand("A" + sfx, (M, K) if c["la"] == 0 else (K, M), c["ra"], 1.0, c["fa"] if self.fp8 else None)
            b = self._operand("B" + sfx, (N, K) if c["lb"] == 0 else (K, N), c["rb"], 1.0, 0 if self.fp8 else None)
            a = a if c["la"] == 0 else a.t()
            b = b.t() if c["lb"] == 0 else b
            self.acc += a @ b
            self.absacc += a.abs() @ b.abs()
        if self.fp8:
            self.acc *= SA * SB
            self.absacc *= SA * SB
            self.sa, self.sb = torch.tensor([SA], device=dev), torch.tensor([SB], device=dev)
        # C += ... (weight gradients, atomics, `accumulate`): integers; C = ...: the NaN fill, every element is written
        self.adds = c["la"] == 1 or c["epi"] == T.F32_ATOMIC or c["accumulate"]
        cpad = self.pad // 2 if self.fp8 else self.pad
        if fam in ("seg", "f32nt"):
            cpad = 0  # their bindings take a contiguous C
        self.bufs["C"] = Guarded(M, N, torch.float32, dev, cpad)
        self.c0 = None
        if self.adds:
            self.c0 = self._ints((M, N), c["rc0"])
            self.bufs["C"].put(self.c0.float())
        if c.get("ws_numel", 0):
            self.bufs["ws"] = _vec(c["ws_numel"], torch.float32, dev)

    # ---- launch
    def launch(self, C_):
        c = self.c
        fam, epi = c["family"], c["epi"]
        if fam == "gemm":
            C_.gemm(self.t("A"), self.t("B"), self.t("C"), c["la"], c["lb"], epi, self.v("bias"), self.t("aux"),
                    self.t("C2"), c["p"], self.seed, c["req_splits"])
        elif fam == "g8":
            kw = {}
            if c["q8"]:
                kw = dict(q8=self.t("q8"), q8_amax=self.q8_amax, q8_sinv=self.q8_sinv, q8_track=self.q8_track, q8fmt=0)
            C_.gemm8(self.t("A"), c["fa"], self.sa, self.t("B"), 0, self.sb, self.t("C"), epi, self.v("bias"),
                     self.t("aux"), self.t("C2"), c["p"], self.seed, self.v("dbias"), rd=self.v("rd"),
                     rd_seq=c["rd_seq"], **kw)
        elif fam == "g8tt":
            C_.gemm8_wgrad(0, self.t("A"), c["fa"], self.sa, self.t("B"), 0, self.sb, self.t("C"), c["req_splits"],
                           self.v("ws"))
        elif fam == "f32nt":
            C_.gemm2_f32nt(self.t("A"), self.t("B"), self.t("C"), c["lb"])
        elif fam == "seg":
            C_.gemm2_seg([self.t("A0"), self.t("A1"), self.t("A2")], [self.t("B0"), self.t("B1"), self.t("B2")],
                         self.t("C"), c["la"], c["lb"], c["accumulate"])
        else:
            C_.gemm2(self.t("A"), self.t("B"), self.t("C"), c["la"], c["lb"], epi, self.v("bias"), self.t("aux"),
                     self.t("C2"), c["p"], self.seed, c["req_splits"], self.v("ws"), self.v("dbias"), self.v("rd"),
                     c["rd_seq"])

    # ---- checks
    def verify(self, C_):
        torch.cuda.synchronize()
        if self.c["epi"] in (T.F32_ATOMIC, T.F32_SLAB):
            self._verify_f32()
        elif self.exact:
            self._verify_exact(C_)
        else:
            self._verify_bounded()
        broken = [k for k, b in self.bufs.items() if not b.intact()]
        assert not broken, f"guard elements overwritten around {broken}"

    def _verify_f32(self):
        bound = self.absacc + (self.c0.abs() if self.adds else 0.0)
        assert float(bound.max()) < LIMIT  # the exactness precondition, on the operands drawn
        ref = self.acc + (self.c0 if self.adds else 0.0)
        out = self.t("C").double()
        assert torch.equal(out, ref), _diff(out, ref)

    def _verify_exact(self, C_):
        c = self.c
        epi, M, N = c["epi"], c["M"], c["N"]
        y = self.acc + (self.bias if self.bias is not None else 0.0)
        bound = self.absacc + (self.bias.abs() if self.bias is not None else 0.0)
        if epi == T.DROP_RES:
            scale = self.keep if self.keep is not None else 1.0
            ref = _rb(_rb(y) * scale + self.aux)
            bound = 2.0 * bound + self.aux.abs()
        elif epi == T.RES:
            ref = _rb(_rb(y) + self.aux)
            bound = bound + self.aux.abs()
        elif epi == T.MUL:
            ref = _rb(_rb(y) * self.aux)
            bound = bound * self.aux.abs()
        else:  # STORE, BIAS, STORE_RDOT
            ref = _rb(y)
        assert float(bound.max()) < LIMIT  # the exactness precondition, on the operands drawn
        out = self.t("C")
        assert torch.equal(out, ref.float().bfloat16()), _diff(out.double(), ref)
        if c["dbias"]:
            assert float((ref.abs().sum(0) + self.db0.abs()).max()) < LIMIT
            want = self.db0 + ref.sum(0)  # rows below M only: the reference has no others
            assert torch.equal(self.v("dbias").double(), want), _diff(self.v("dbias").double(), want)
        if epi == T.RDOT:
            S, heads = c["rd_seq"], N // 64
            assert float((ref.abs() * self.aux.abs()).view(M, heads, 64).sum(-1).max()) < LIMIT
            want = (ref * self.aux).view(M // S, S, heads, 64).sum(-1).permute(0, 2, 1).reshape(-1)
            assert torch.equal(self.v("rd").double(), want), _diff(self.v("rd").double(), want)
        if c["q8"]:
            # the fp8 copy == the standalone quantiser on the kernel's own bf16 output at the same amax
            dev = self.dev
            q_ref = torch.empty(M, N, dtype=torch.uint8, device=dev)
            sinv_ref, track_ref = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
            C_.fp8_quant(out, self.q8_amax, q_ref, sinv_ref, 0, False, track_ref)
            torch.cuda.synchronize()
            assert torch.equal(self.t("q8"), q_ref), int((self.t("q8") != q_ref).sum())
            assert torch.equal(self.q8_sinv, sinv_ref)
            assert float(self.q8_track) == float(out.float().abs().max()) == float(track_ref)

    def _verify_bounded(self):
        c = self.c
        epi = c["epi"]
        am = self.absacc
        C = self.t("C")
        if epi == T.BIAS_GELU:
            y = self.acc + self.bias
            _check(C, y, acc=am)
            g = _gelu64(y)
            _check(self.t("C2"), g, mag=2 * y.abs() + g.abs(), acc=2 * am)
        elif epi == T.DGELU:
            gg = _gelu_grad(self.aux)
            r = _rb(self.acc) * gg
            _check(C, r, mag=2 * self.acc.abs() * gg.abs() + r.abs(), acc=2 * am)
            if c["dbias"]:
                # the fp64 column sums of the kernel's own bf16 output (rows below M: it has no others) + the pre-fill
                want = self.db0 + C.double().sum(0)
                _check(self.v("dbias"), want, acc=self.db0.abs() + C.double().abs().sum(0), fp32=True)
        else:  # GELU_D: C = gelu'(y), C2 = gelu(y), y = bf16(acc + bias)
            y = _rb(self.acc + self.bias)
            g, d = _gelu64(y), _gelu_grad(y)
            _check(self.t("C2"), g, mag=2 * y.abs() + g.abs(), acc=2 * am)
            _check(C, d, mag=y.abs() + d.abs(), acc=am)


def _diff(out, ref):
    bad = out != ref
    i = int(bad.flatten().nonzero()[0])
    cols = ref.shape[-1]
    return (f"{int(bad.sum())} of {bad.numel()} elements differ; first at row {i // cols} column {i % cols}: "
            f"out {out.flatten()[i].item()} ref {ref.flatten()[i].item()}")


def _assert_kernel(C_, c, dev):
    """The planner, at this device's CU count, runs the kernel the case is there for."""
    if c["entry"] == "gemm":
        return
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    check_plan(c, plan_of(C_, c, cus=cus))


def _set_knobs(c, monkeypatch):
    for k, v in c["knobs"].items():
        monkeypatch.setenv(k, str(v))


@pytest.mark.parametrize("c", T.CASES, ids=[c["id"] for c in T.CASES])
def test_gemm_edge_case(gpu, monkeypatch, c):
    C_ = _C()
    _set_knobs(c, monkeypatch)
    _assert_kernel(C_, c, gpu)
    run = Run(c, gpu)
    run.launch(C_)
    run.verify(C_)


def test_persistent_tile_queue_is_reset_between_launches(gpu, monkeypatch):
    """Two persistent launches with different tile counts (257 and 258 tiles on 256 workgroups, then the first again)
    back to back on one stream, no synchronisation between them: each starts from a zeroed tile queue, so all three are
    exact."""
    C_ = _C()
    cases = [T.BY_ID["pk-bias-65537x256x64-l00"], T.BY_ID["pk-dropres+p0.5-32769x512x128-l00"],
             T.BY_ID["pk-mul+db-65537x256x64-l00"]]
    runs = []
    for c in cases:
        assert not c["knobs"]
        _assert_kernel(C_, c, gpu)
        runs.append(Run(c, gpu))
    torch.cuda.synchronize()
    for r in runs:
        r.launch(C_)
    for r in runs:
        r.verify(C_)
