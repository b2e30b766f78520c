"""The GEMM edge-case table (tests/gemm_edge_cases.py) against the launch planner (csrc/kernels/gemm_plan.h, through
``_C.gemm_plan`` at 256 CUs): under each case's knobs the planner must pick the kernel and the template arguments the
case is there for, launch the K-slabs it claims, and the case's value ranges must keep every fp32 intermediate exact. A
policy change in the planner then breaks the table here instead of quietly moving GPU cases onto another kernel.
Needs the built extension, no GPU."""
import importlib

import pytest

import gemm_edge_cases as T

CASES = T.CASES
PLANNED = [c for c in CASES if c["entry"] != "gemm"]


@pytest.fixture(scope="module")
def C():
    try:
        return importlib.import_module("huggingface_sagemaker_tensorflow_distributed_amd._C")
    except ImportError:
        pytest.skip("native extension not built")


def plan_of(C, c, cus=256):
    """The planner's answer for a case (the caller has set the case's knobs)."""
    return C.gemm_plan(c["entry"], c["la"], c["lb"], c["epi"], c["M"], c["N"], c["K"], splits=c["req_splits"],
                       dbias=c["dbias"], accumulate=c["accumulate"], q8=c["q8"], fa=c["fa"], cus=cus)


def check_plan(c, pl):
    """`pl` runs the kernel the case names, with its template arguments, grid and K-slabs."""
    assert pl["supported"], c["id"]
    ls = pl["launches"]
    assert len(ls) == c["launches"], [l["kernel"] for l in ls]
    assert (ls[0]["kernel"], list(ls[0]["targs"])) == (c["kernel"], c["targs"])
    assert ls[0]["grid"] == c["grid"]
    if c["launches"] == 2:
        assert (ls[1]["kernel"], list(ls[1]["targs"])) == (c["second"][0], list(c["second"][1]))
    assert (pl["splits"], pl["kps"]) == (c["splits"], c["kps"])
    if "ws_numel" in c:
        assert pl["ws_numel"] == c["ws_numel"]


def test_table_is_well_formed():
    ids = [c["id"] for c in CASES]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    fams = {c["family"] for c in CASES}
    assert fams == {"g2", "g2s", "splitk", "pk", "rdot", "tt", "f32nt", "seg", "g8", "g8tt", "gemm"}
    for fam in fams - {"f32nt"}:  # gemm2_f32nt takes contiguous operands only
        assert any(c["strided"] for c in CASES if c["family"] == fam), fam
    # the axes the table is there for
    g2 = [c for c in CASES if c["family"] == "g2"]
    assert {(c["targs"][4], c["K"] // 64) for c in g2} >= {(s, k) for s in (0, 1, 2, 4, 5, 6, 7) for k in (1, 2, 3)}
    assert {c["M"] for c in g2} >= {1, 255, 257, 300} and {c["grid"] for c in g2} >= {1, 2, 3, 4, 6}
    g2s = [c for c in CASES if c["family"] == "g2s"]
    assert {(c["targs"][3], c["targs"][4], c["K"]) for c in g2s} >= {
        (s, w, k) for s, w in ((2, 1), (3, 1), (3, 2), (4, 1)) for k in (64, 128, 192, 320)}
    assert {c["M"] for c in g2s} >= {1, 127, 129, 257}
    sk = [c for c in CASES if c["family"] == "splitk"]
    for kern in ("gemm2_kernel", "gemm2s_kernel"):
        assert {c["epi"] for c in sk if c["kernel"] == kern} >= {0, 1, 2, 3, 4, 5, 8, 9}
        assert {(c["K"], c["req_splits"]) for c in sk if c["kernel"] == kern} >= {(320, 3), (192, 2), (320, 4)}


@pytest.mark.parametrize("c", PLANNED, ids=[c["id"] for c in PLANNED])
def test_case_runs_the_kernel_it_names(C, c, monkeypatch):
    for k, v in c["knobs"].items():
        monkeypatch.setenv(k, str(v))
    pl = plan_of(C, c)
    check_plan(c, pl)
    K, bk = c["K"] * (3 if c["family"] == "seg" else 1), 128 if c["family"] == "g8tt" else 64
    if c["family"] == "g8":
        assert c["kps"] * 2 == K and K % 128 == 0
    else:
        # the slabs cover K, the last one is not empty, every slab is whole K-tiles
        assert c["kps"] % bk == 0 and (c["splits"] - 1) * c["kps"] < K <= c["splits"] * c["kps"]
    if c["req_splits"] > 1 and c["family"] in ("splitk", "tt", "f32nt", "g8tt") and c["splits"] > 1:
        assert K - (c["splits"] - 1) * c["kps"] <= c["kps"]


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_exact_cases_stay_below_2_pow_24(c):
    if c["mode"] != "exact":
        assert c["epi"] in T.BOUNDED
        return
    assert c["epi"] not in T.BOUNDED
    for what, v in T.exact_bounds(c).items():
        assert v < T.EXACT_LIMIT, (what, v)
    if c["family"] in ("g8", "g8tt"):
        assert max(c["ra"], c["rb"]) <= 8  # e4m3 and e5m2 both hold the integers -8 .. 8
