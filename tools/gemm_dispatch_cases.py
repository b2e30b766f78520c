"""The GEMM dispatch table: every branch of the gemm2 / gemm8 launch policy, one case each.

CASES is the table (tests/test_gemm_plan.py compares ``_C.gemm_plan`` with the kernel trace recorded for each case).
The tool runs every case through the real entry points on seeded, CPU-generated inputs:

    python tools/gemm_dispatch_cases.py --hash   [--out FILE]   sha256 of every deterministic output, one JSON line
    python tools/gemm_dispatch_cases.py --launch                launches only, a marker kernel (gelu_fwd on 64
                                                                elements) before each case:
        rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/gemm_dispatch_cases.py --launch
    python tools/gemm_dispatch_cases.py --parse-trace CSV --out JSON
                                                                the ordered (kernel, template arguments, grid,
                                                                workgroup) list per case from such a trace

It uses only bindings that every revision since the fp8 weight gradient has, so it runs unchanged in an older tree.
"""
from __future__ import annotations

import argparse
import csv
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# epilogues (csrc/kernels/gemm_plan.h enum Epi2)
STORE, BIAS, BIAS_GELU, BIAS_DROP_RES, RES, DGELU, F32_ATOMIC, F32_SLAB, BIAS_GELU_D, MUL, STORE_RDOT = range(11)


def _c(entry, branch, M, N, K, la=0, lb=0, epi=STORE, splits=0, dbias=False, knobs=None, accumulate=False, q8=False,
       tag=""):
    name = f"{entry}_{la}{lb}_e{epi}_{M}x{N}x{K}_s{splits}"
    if dbias:
        name += "_dbias"
    if accumulate:
        name += "_acc"
    if q8:
        name += "_q8"
    for k, v in sorted((knobs or {}).items()):
        name += f"_{k}={v}"
    return dict(id=name + tag, branch=branch, entry=entry, la=la, lb=lb, epi=epi, M=M, N=N, K=K, splits=splits,
                dbias=dbias, knobs=dict(knobs or {}), accumulate=accumulate, q8=q8)


def _cases():
    c = []
    # ---- NT, bf16 output -------------------------------------------------------------------------------------------
    c.append(_c("gemm2", "128-tile, one split, 256 workgroups: 3 stages, 8 waves", 4096, 1024, 128, epi=BIAS))
    c.append(_c("gemm2", "128-tile, 512 workgroups: 2 stages", 4096, 2048, 128, epi=BIAS_GELU_D))
    c.append(_c("gemm2", "128-tile split-K, 6 splits, plus splitk_epi", 128, 768, 768, epi=BIAS_DROP_RES))
    c.append(_c("gemm2", "128-tile split-K, k-strided B", 128, 768, 768, lb=1, epi=STORE))
    c.append(_c("gemm2", "one-shot 256-row tile, BN 192, 256 tiles", 16384, 768, 128, epi=BIAS))
    c.append(_c("gemm2", "one-shot, BN 256", 16384, 1024, 128, epi=RES))
    c.append(_c("gemm2", "one-shot, k-strided B (256 wide)", 16384, 1024, 128, lb=1, epi=STORE))
    c.append(_c("gemm2", "persistent, BN 192", 32768, 768, 128, epi=BIAS_GELU))
    c.append(_c("gemm2", "persistent, BN 256", 32768, 1024, 128, epi=STORE))
    c.append(_c("gemm2", "k-strided B is never persistent", 32768, 1024, 128, lb=1, epi=STORE))
    c.append(_c("gemm2", "256-tile split-K, 2 splits, layout (0,0) only", 256, 192, 1024, epi=STORE))
    c.append(_c("gemm2", "unsupported: 192 columns with k-strided B", 256, 192, 1024, lb=1, epi=STORE))
    c.append(_c("gemm2", "long K, 32 splits", 256, 256, 16384, epi=DGELU))
    c.append(_c("gemm2", "long K, 32 splits, k-strided B", 256, 256, 16384, lb=1, epi=MUL))
    c.append(_c("gemm2", "unsupported shape", 200, 136, 128, epi=STORE))
    c.append(_c("gemm2", "fused dbias forces BN 256 (persistent)", 32768, 768, 128, epi=DGELU, dbias=True))
    c.append(_c("gemm2", "fused dbias forces BN 256 (one-shot)", 16384, 768, 128, epi=MUL, dbias=True))
    c.append(_c("gemm2", "row dots force BN 256", 16384, 768, 128, epi=STORE_RDOT))
    c.append(_c("gemm2", "row dots on the 128-tile kernel", 4096, 1024, 128, epi=STORE_RDOT))
    c.append(_c("gemm2", "requested splits on the 128-tile kernel", 4096, 1024, 256, epi=BIAS, splits=2))
    c.append(_c("gemm2", "one requested split", 128, 768, 768, epi=STORE, splits=1))
    # ---- TT weight gradient (K = tokens) ---------------------------------------------------------------------------
    c.append(_c("gemm2", "small-step minimum-grid plan, 11 splits", 768, 768, 4096, la=1, lb=1, epi=F32_SLAB))
    c.append(_c("gemm2", "small-step plan, 2 splits", 768, 768, 256, la=1, lb=1, epi=F32_SLAB))
    c.append(_c("gemm2", "cost model, 16 splits", 1024, 1024, 16384, la=1, lb=1, epi=F32_SLAB))
    c.append(_c("gemm2", "cost model, 7 splits", 768, 3072, 131072, la=1, lb=1, epi=F32_SLAB))
    c.append(_c("gemm2", "one split, in-place accumulate", 256, 256, 64, la=1, lb=1, epi=F32_SLAB))
    c.append(_c("gemm2", "the tied-decoder one-split case", 50432, 1024, 4928, la=1, lb=1, epi=F32_SLAB, splits=1))
    c.append(_c("gemm2", "cost model, one split on 256-row tiles, in place", 4096, 4096, 16384, la=1, lb=1,
                epi=F32_SLAB))
    c.append(_c("gemm2", "atomics, automatic splits", 768, 768, 4096, la=1, lb=1, epi=F32_ATOMIC))
    c.append(_c("gemm2", "atomics, one split", 256, 256, 64, la=1, lb=1, epi=F32_ATOMIC))
    c.append(_c("gemm2", "requested splits on the planned tile", 1024, 1024, 16384, la=1, lb=1, epi=F32_SLAB, splits=4))
    # ---- fp32-output NT --------------------------------------------------------------------------------------------
    c.append(_c("f32nt", "fp32 NT, split over K", 4096, 1024, 3072, epi=F32_SLAB))
    c.append(_c("f32nt", "fp32 NT, split over K, k-strided B", 4096, 1024, 3072, lb=1, epi=F32_SLAB))
    c.append(_c("f32nt", "fp32 NT, one pass", 16384, 1024, 256, epi=F32_SLAB))
    # ---- segmented fp32 (K = Kseg) ---------------------------------------------------------------------------------
    for acc in (False, True):
        c.append(_c("seg", "128-tile, no slabs", 4096, 1024, 1024, epi=F32_SLAB, accumulate=acc))
        c.append(_c("seg", "slabs plus reduce", 4096, 1024, 4096, epi=F32_SLAB, accumulate=acc))
    c.append(_c("seg", "one split on 256-row tiles", 16384, 1024, 64, lb=1, epi=F32_SLAB, accumulate=True))
    for la, lb in ((0, 0), (0, 1), (1, 1)):
        c.append(_c("seg", "the three layouts", 128, 768, 768, la=la, lb=lb, epi=F32_SLAB))
    c.append(_c("seg", "TT on 256-row tiles, slabs", 1024, 1024, 8192, la=1, lb=1, epi=F32_SLAB))
    c.append(_c("seg", "TT, one split", 256, 256, 64, la=1, lb=1, epi=F32_SLAB, knobs={"HSD_G2_SMALL_TT": 0}))
    # ---- fp8 -------------------------------------------------------------------------------------------------------
    c.append(_c("gemm8", "fp8 NT, BN 256", 4096, 1024, 256, epi=BIAS))
    c.append(_c("gemm8", "fp8 NT, BN 192", 16384, 768, 256, epi=BIAS))
    c.append(_c("gemm8", "fp8 NT, BN 256, q8 copy", 4096, 1024, 256, epi=BIAS_GELU_D, q8=True))
    c.append(_c("gemm8", "fp8 NT, BN 192, q8 copy", 16384, 768, 256, epi=MUL, q8=True))
    c.append(_c("gemm8", "fp8 NT, fused dbias forces BN 256", 16384, 768, 256, epi=DGELU, dbias=True))
    c.append(_c("gemm8", "fp8 NT, row dots force BN 256", 16384, 768, 256, epi=STORE_RDOT))
    c.append(_c("gemm8_wgrad", "fp8 weight gradient, automatic (16 slabs)", 1024, 1024, 32768))
    c.append(_c("gemm8_wgrad", "fp8 weight gradient, 2 requested", 1024, 1024, 32768, splits=2))
    c.append(_c("gemm8_wgrad", "fp8 weight gradient, one slab", 256, 256, 128))
    # ---- knob rows, each on a shape whose plan it changes ----------------------------------------------------------
    k = lambda name, v, branch, *a, **kw: c.append(_c(*((a[0], f"{name}={v}: {branch}") + a[1:]), knobs={name: v}, **kw))
    k("HSD_G2_SMALL", 0, "256-row tiles where 128 would be picked", "gemm2", 4096, 1024, 128, epi=BIAS)
    k("HSD_G2_SMALL", 1, "128 tiles where 256 would be picked", "gemm2", 16384, 1024, 128, epi=RES)
    k("HSD_G2_SPLITK", 1, "no split", "gemm2", 128, 768, 768, epi=BIAS_DROP_RES)
    k("HSD_G2_SPLITK", 3, "3 splits", "gemm2", 128, 768, 768, epi=BIAS_DROP_RES)
    k("HSD_G2_PERSIST", 0, "one-shot where persistent would be picked", "gemm2", 32768, 1024, 128, epi=STORE)
    k("HSD_G2S_STAGES", 2, "2 stages at 256 workgroups", "gemm2", 4096, 1024, 128, epi=BIAS)
    k("HSD_G2S_STAGES", 4, "4 stages", "gemm2", 4096, 1024, 128, epi=BIAS)
    k("HSD_G2S_KW", 1, "3 stages, 4 waves", "gemm2", 4096, 1024, 128, epi=BIAS)
    k("HSD_G2_SMALL_TT", 0, "256-row tiles", "gemm2", 768, 768, 16384, la=1, lb=1, epi=F32_SLAB)
    k("HSD_G2_SMALL_TT", 1, "128 tiles", "gemm2", 1024, 1024, 16384, la=1, lb=1, epi=F32_SLAB)
    k("HSD_WGRAD_MIN_GRID", 0, "the cost model at a small step", "gemm2", 768, 768, 4096, la=1, lb=1, epi=F32_SLAB)
    k("HSD_G2_TT_ATOMIC", 1, "atomics at one split", "gemm2", 4096, 4096, 16384, la=1, lb=1, epi=F32_SLAB)
    k("HSD_F32NT_SPLITS", 1, "one pass", "f32nt", 4096, 1024, 3072, epi=F32_SLAB)
    k("HSD_F32NT_SPLITS", 1, "segmented, one pass on 256-row tiles", "seg", 4096, 1024, 4096, epi=F32_SLAB)
    k("HSD_SEG_NT_SMALL", 0, "slabs where 128 tiles would be picked", "seg", 4096, 1024, 1024, epi=F32_SLAB)
    k("HSD_G2_SYNC", 1, "one barrier per K-tile", "gemm2", 16384, 1024, 128, epi=RES)
    ids = [x["id"] for x in c]
    assert len(set(ids)) == len(ids), "duplicate case id"
    return c


CASES = _cases()
KNOBS = sorted({k for c in CASES for k in c["knobs"]})


# ---- running the cases ------------------------------------------------------------------------------------------------
class _Data:
    """Seeded CPU values, tiled to any size (the large weight-gradient operands would take seconds of randn each)."""

    def __init__(self, torch, dev):
        self.torch, self.dev = torch, dev
        g = torch.Generator(device="cpu").manual_seed(1234)
        self.base = torch.randn(1 << 20, generator=g) * 0.5
        self.bits = torch.randint(0, 0x70, (1 << 20,), generator=g, dtype=torch.int32)  # finite e4m3 / e5m2
        self.sign = torch.randint(0, 2, (1 << 20,), generator=g, dtype=torch.int32) * 0x80
        self.n = 0

    def _tile(self, src, numel):
        self.n += 1
        off = (self.n * 7919) % 4096
        reps = (numel + off + src.numel() - 1) // src.numel()
        return src.repeat(reps)[off:off + numel]

    def bf16(self, *shape):
        t = self.torch
        return self._tile(self.base, int(t.Size(shape).numel())).to(t.bfloat16).view(*shape).to(self.dev)

    def fp8(self, *shape):
        t = self.torch
        n = int(t.Size(shape).numel())
        return (self._tile(self.bits, n) | self._tile(self.sign, n)).to(t.uint8).view(*shape).to(self.dev)


def set_knobs(_C, knobs):
    for k in KNOBS:
        os.environ.pop(k, None)
    for k, v in knobs.items():
        os.environ[k] = str(v)
    _C.refresh_env()


def run_case(torch, _C, d, c):
    """Launch one case; returns {name: tensor} of its outputs, or None if the shape is unsupported."""
    dev, f32 = d.dev, torch.float32
    la, lb, epi, M, N, K, sp = c["la"], c["lb"], c["epi"], c["M"], c["N"], c["K"], c["splits"]
    e = c["entry"]
    if e in ("gemm2", "f32nt"):
        if not _C.gemm2_supported(la, lb, epi, M, N, K):
            return None
        A = d.bf16(M, K) if la == 0 else d.bf16(K, M)
        B = d.bf16(N, K) if lb == 0 else d.bf16(K, N)
        if e == "f32nt":
            C = torch.zeros(M, N, dtype=f32, device=dev)
            _C.gemm2_f32nt(A, B, C, lb)
            return {"C": C}
        out = {}
        if la == 1:
            C = torch.zeros(M, N, dtype=f32, device=dev)
            ws = None
            if epi == F32_SLAB:
                n = sp if sp > 0 else _C.gemm2_splits(M, N, K)
                ws = torch.empty(n * M * N, dtype=f32, device=dev)
            _C.gemm2(A, B, C, 1, 1, epi, None, None, None, 0.0, 0, sp, ws, None)
            return {"C": C}
        C = torch.zeros(M, N, dtype=torch.bfloat16, device=dev)
        bias = d.bf16(N) if epi in (BIAS, BIAS_GELU, BIAS_DROP_RES, BIAS_GELU_D) else None
        aux = d.bf16(M, N) if epi in (BIAS_DROP_RES, RES, DGELU, MUL, STORE_RDOT) else None
        C2 = torch.zeros_like(C) if epi in (BIAS_GELU, BIAS_GELU_D) else None
        db = torch.zeros(N, dtype=f32, device=dev) if c["dbias"] else None
        rd = torch.zeros(M * (N // 64), dtype=f32, device=dev) if epi == STORE_RDOT else None
        p = 0.1 if epi == BIAS_DROP_RES else 0.0
        _C.gemm2(A, B, C, 0, lb, epi, bias, aux, C2, p, 77, sp, None, db, rd, 128 if rd is not None else 0)
        out["C"] = C
        for name, t in (("C2", C2), ("dbias", db), ("rd", rd)):
            if t is not None:
                out[name] = t
        return out
    if e == "seg":
        if not _C.gemm2_seg_supported(la, lb, M, N, K):
            return None
        A = [d.bf16(M, K) if la == 0 else d.bf16(K, M) for _ in range(3)]
        B = [d.bf16(N, K) if lb == 0 else d.bf16(K, N) for _ in range(3)]
        C = d.bf16(M, N).float() if (c["accumulate"] or la == 1) else torch.zeros(M, N, dtype=f32, device=dev)
        _C.gemm2_seg(A, B, C, la, lb, c["accumulate"])
        return {"C": C}
    one = lambda v: torch.full((1,), v, dtype=f32, device=dev)
    if e == "gemm8":
        if not _C.gemm8_supported(epi, M, N, K):
            return None
        A, B = d.fp8(M, K), d.fp8(N, K)
        C = torch.zeros(M, N, dtype=torch.bfloat16, device=dev)
        bias = d.bf16(N) if epi in (BIAS, BIAS_GELU, BIAS_DROP_RES, BIAS_GELU_D) else None
        aux = d.bf16(M, N) if epi in (BIAS_DROP_RES, RES, DGELU, MUL, STORE_RDOT) else None
        C2 = torch.zeros_like(C) if epi in (BIAS_GELU, BIAS_GELU_D) else None
        db = torch.zeros(N, dtype=f32, device=dev) if c["dbias"] else None
        rd = torch.zeros(M * (N // 64), dtype=f32, device=dev) if epi == STORE_RDOT else None
        kw = {}
        q8 = None
        if c["q8"]:
            q8 = torch.zeros(M, N, dtype=torch.uint8, device=dev)
            kw = dict(q8=q8, q8_amax=one(64.0), q8_sinv=one(0.0), q8_track=one(0.0), q8fmt=0)
        _C.gemm8(A, 0, one(2.0 ** -8), B, 0, one(2.0 ** -8), C, epi, bias=bias, aux=aux, C2=C2, p=0.0, seed=0, dbias=db,
                 rd=rd, rd_seq=128 if rd is not None else 0, **kw)
        out = {"C": C}
        for name, t in (("C2", C2), ("dbias", db), ("rd", rd), ("q8", q8)):
            if t is not None:
                out[name] = t
        return out
    if e == "gemm8_wgrad":
        if not _C.gemm8_wgrad_supported(M, N, K):
            return None
        dy, x = d.fp8(K, M), d.fp8(K, N)
        C = torch.zeros(M, N, dtype=f32, device=dev)
        ws = torch.empty(_C.gemm8_wgrad_ws_numel(M, N, K, sp), dtype=f32, device=dev)
        _C.gemm8_wgrad(0, dy, 0, one(2.0 ** -8), x, 0, one(2.0 ** -8), C, sp, ws)
        return {"C": C}
    raise ValueError(e)


def _sha(torch, t):
    b = t.detach().cpu().contiguous()
    if b.dtype == torch.bfloat16:
        b = b.view(torch.int16)
    return hashlib.sha256(b.numpy().tobytes()).hexdigest()


def run_all(mode, out_path=None, dump_dir=None, only=None):
    import torch

    from huggingface_sagemaker_tensorflow_distributed_amd.ops import _ext

    _C = _ext.load()
    dev = torch.device("cuda", 0)
    marker = torch.zeros(64, dtype=torch.bfloat16, device=dev)
    result = {}
    for c in CASES:
        if only and c["id"] not in only:
            continue
        d = _Data(torch, dev)
        set_knobs(_C, c["knobs"])
        if mode == "launch":
            torch.cuda.synchronize()
            _C.gelu_fwd(marker, marker)
        outs = run_case(torch, _C, d, c)
        torch.cuda.synchronize()
        if mode == "hash":
            result[c["id"]] = None if outs is None else {k: _sha(torch, v) for k, v in outs.items()}
            if dump_dir and outs is not None and c["id"] in (only or ()):
                os.makedirs(dump_dir, exist_ok=True)
                for k, v in outs.items():
                    torch.save(v.cpu(), os.path.join(dump_dir, f"{c['id']}.{k}.pt"))
        del outs, d
    set_knobs(_C, {})
    if mode == "launch":
        _C.gelu_fwd(marker, marker)
        torch.cuda.synchronize()
        return
    text = json.dumps(result, sort_keys=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")
    print(text)


# ---- reading a kernel trace --------------------------------------------------------------------------------------------
_GEMM_KERNELS = ("gemm2_kernel", "gemm2pk_kernel", "gemm2s_kernel", "gemm8pk_kernel", "gemm8tt_kernel",
                 "slab_reduce_kernel", "splitk_epi_kernel")


def normalise(name):
    """'void hsd::g2::gemm2_kernel<0, 1, 7, 256, 4, false>(hsd::G2Params)' -> ('gemm2_kernel', [0, 1, 7, 256, 4, 0])"""
    m = re.search(r"(\w+)(?:<([^>]*)>)?\s*\(", name)
    if not m:
        m = re.search(r"(\w+)(?:<([^>]*)>)?", name)
    base, targs = m.group(1), []
    for a in (m.group(2) or "").split(","):
        a = a.strip()
        if not a:
            continue
        a = re.sub(r"^\([^)]*\)", "", a)  # '(hsd::Epi2)1' -> '1'
        targs.append(1 if a == "true" else 0 if a == "false" else int(a))
    return base, targs


def parse_trace(path):
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    key = "Dispatch_Id" if rows and "Dispatch_Id" in rows[0] else "Start_Timestamp"
    rows.sort(key=lambda r: int(r[key]))
    per_case, cur = [], None
    for r in rows:
        base, targs = normalise(r["Kernel_Name"])
        if "gelu_fwd" in base:
            cur = []
            per_case.append(cur)
            continue
        if cur is None or base not in _GEMM_KERNELS:
            continue
        wg, grid = 1, 1
        for ax in "XYZ":
            w = int(r["Workgroup_Size_" + ax])
            wg *= w
            grid *= int(r["Grid_Size_" + ax]) // w
        cur.append({"kernel": base, "targs": targs, "grid": grid, "wg": wg})
    per_case.pop()  # the closing marker
    assert len(per_case) == len(CASES), (len(per_case), len(CASES))
    return {c["id"]: launches for c, launches in zip(CASES, per_case)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hash", action="store_true")
    ap.add_argument("--launch", action="store_true")
    ap.add_argument("--parse-trace")
    ap.add_argument("--out")
    ap.add_argument("--dump", help="with --hash and --only: save the listed cases' outputs here (torch.save)")
    ap.add_argument("--only", nargs="*")
    a = ap.parse_args()
    if a.parse_trace:
        text = json.dumps(parse_trace(a.parse_trace), indent=1, sort_keys=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text + "\n")
        else:
            print(text)
    elif a.launch:
        run_all("launch", only=a.only)
    else:
        run_all("hash", a.out, a.dump, a.only)


if __name__ == "__main__":
    main()
