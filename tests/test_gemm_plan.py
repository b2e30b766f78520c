"""The GEMM launch policy as a policy (csrc/kernels/gemm_plan.h): for every case of the dispatch table
(tools/gemm_dispatch_cases.py CASES: one case per branch, each naming the branch it is there for) ``_C.gemm_plan`` must
list exactly the kernels -- base name, template arguments, grid, workgroup size, in order -- that the commit before the
planner launched for that case. tests/data/gemm_dispatch_parent.json holds those lists, read from a rocprofv3 kernel
trace of that commit on an MI355X (256 CUs); it is a record of the old code, not output of the code under test.
Needs the built extension, no GPU."""
import importlib
import importlib.util
import json
import os

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _load_cases():
    spec = importlib.util.spec_from_file_location("gemm_dispatch_cases",
                                                  os.path.join(ROOT, "tools", "gemm_dispatch_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_T = _load_cases()
CASES = _T.CASES
with open(os.path.join(ROOT, "tests", "data", "gemm_dispatch_parent.json")) as _f:
    PARENT = json.load(_f)

GL_SLABS_ASSIGN = 3  # gemm_plan.h GemmLanding: this and above land through workspace slabs


@pytest.fixture(scope="module")
def C():
    try:
        return importlib.import_module("huggingface_sagemaker_tensorflow_distributed_amd._C")
    except ImportError:
        pytest.skip("native extension not built")


def _plan(C, c):
    e = c["entry"]
    if e in ("gemm2", "f32nt"):
        return C.gemm_plan("gemm2", c["la"], c["lb"], c["epi"], c["M"], c["N"], c["K"], splits=c["splits"],
                           dbias=c["dbias"])
    if e == "seg":
        return C.gemm_plan("gemm2_seg", c["la"], c["lb"], c["epi"], c["M"], c["N"], c["K"], accumulate=c["accumulate"])
    if e == "gemm8":
        return C.gemm_plan("gemm8", 0, 0, c["epi"], c["M"], c["N"], c["K"], dbias=c["dbias"], q8=c["q8"])
    return C.gemm_plan("gemm8_wgrad", 1, 1, c["epi"], c["M"], c["N"], c["K"], splits=c["splits"])


def _k_split(K, splits, bk=64):
    kps = -(-K // max(splits, 1))
    kps = -(-kps // bk) * bk
    return kps, -(-K // kps)


def test_table_and_fixture_cover_the_same_cases():
    assert sorted(PARENT) == sorted(c["id"] for c in CASES)
    assert all(c["branch"] for c in CASES)
    # every knob of the policy has a row
    assert set(_T.KNOBS) >= {"HSD_G2_SMALL", "HSD_G2_SPLITK", "HSD_G2_PERSIST", "HSD_G2S_STAGES", "HSD_G2S_KW",
                             "HSD_G2_SMALL_TT", "HSD_WGRAD_MIN_GRID", "HSD_G2_TT_ATOMIC", "HSD_F32NT_SPLITS",
                             "HSD_SEG_NT_SMALL", "HSD_G2_SYNC"}


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_plan_matches_parent_dispatch(C, c, monkeypatch):
    for k, v in c["knobs"].items():
        monkeypatch.setenv(k, str(v))
    pl = _plan(C, c)
    want = PARENT[c["id"]]
    got = [dict(kernel=l["kernel"], targs=list(l["targs"]), grid=l["grid"], wg=l["wg"]) for l in pl["launches"]]
    assert got == want, c["branch"]
    assert pl["supported"] == bool(want)

    # the workspace holds every slab the kernels write
    M, N, K, e = c["M"], c["N"], c["K"], c["entry"]
    if pl["landing"] >= GL_SLABS_ASSIGN:
        assert pl["ws_numel"] >= pl["splits"] * M * N
        assert len(got) == 2 and got[0]["grid"] % pl["splits"] == 0
    else:
        assert pl["ws_numel"] == 0 and len(got) <= 1

    # the thin wrappers read the same plan
    if e in ("gemm2", "f32nt") and not c["dbias"]:
        assert C.gemm2_supported(c["la"], c["lb"], c["epi"], M, N, K) == pl["supported"]
    if e == "gemm2" and c["la"] == 1 and pl["supported"]:
        ok, sp, ws = C.gemm2_wgrad_plan(M, N, K)
        assert sp == C.gemm2_splits(M, N, K)
        if c["splits"] == 0:
            assert (pl["kps"], pl["splits"]) == _k_split(K, sp)
            if c["epi"] == _T.F32_SLAB:
                assert ok and ws == pl["ws_numel"]
    if e == "gemm2" and c["la"] == 0 and c["splits"] == 0 and pl["supported"]:
        sp = C.gemm2_nt_splits(M, N, K)
        assert (sp > 1) == (pl["landing"] >= GL_SLABS_ASSIGN)
        if sp > 1:
            assert (pl["kps"], pl["splits"]) == _k_split(K, sp)
    if e == "seg":
        assert C.gemm2_seg_supported(c["la"], c["lb"], M, N, K) == pl["supported"]
    if e == "gemm8":
        assert C.gemm8_supported(c["epi"], M, N, K) == pl["supported"]
    if e == "gemm8_wgrad":
        assert C.gemm8_wgrad_supported(M, N, K) == pl["supported"]
        assert C.gemm8_wgrad_ws_numel(M, N, K, c["splits"]) == pl["ws_numel"]
        if c["splits"] > 0:
            assert (pl["kps"], pl["splits"]) == _k_split(K, c["splits"], 128)
