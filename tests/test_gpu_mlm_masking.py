"""--mlm_masking dynamic on the GPU: the masking / compaction kernels bit for bit against the torch reference
(ops/rng.py mlm_mask_reference), the row-scatter kernel, the fixed-capacity head against the static head with the fp32
CPU model as the yardstick, and HIP-graph capture (no host sync) with fresh masks per replay."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V, MASK, SPECIAL, RANGE = 50265, 50264, (0, 1, 2, 50264), (3, 50265)
SEED = 0x5EED_0F_A_9A55_C0DE
FIELDS = ("input_ids", "labels", "sel", "tgt", "inv", "counts", "n_valid")


def _ops():
    from huggingface_sagemaker_tensorflow_distributed_amd import ops

    return ops


def _rng():
    from huggingface_sagemaker_tensorflow_distributed_amd.ops import rng

    return rng


def _block():
    from huggingface_sagemaker_tensorflow_distributed_amd.ops import hip

    return int(hip._C.mlm_mask_block())


def _flat_case(n, seed=0):
    """ids with a sprinkling of special tokens, and incoming labels with ignored stretches."""
    g = np.random.default_rng(seed)
    ids = g.integers(3, V - 1, size=n, dtype=np.int64)
    ids[g.random(n) < 0.05] = 1
    ids[g.random(n) < 0.02] = MASK
    lab = np.zeros(n, dtype=np.int64)
    lab[g.random(n) < 0.1] = -100
    return torch.from_numpy(ids), torch.from_numpy(lab)


def _check(got, want, what=""):
    assert got.cap == want.cap, what
    for f in FIELDS:
        a, b = getattr(got, f).cpu(), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, f, a.dtype, b.dtype, a.shape, b.shape)
        assert torch.equal(a, b), f"{what} {f}: {int((a != b).sum())} of {a.numel()} differ"


def _both(gpu, ids, am, lab, p=0.15, cap=None, step_seed=None, seed=SEED):
    d = lambda t: None if t is None else t.to(gpu)  # noqa: E731
    got = _ops().mlm_mask(d(ids), d(am), d(lab), seed, p, MASK, SPECIAL, RANGE, cap=cap)
    want = _rng().mlm_mask_reference(ids, am, lab, seed, p, MASK, SPECIAL, RANGE, cap=cap, step_seed=step_seed)
    return got, want


# ------------------------------------------------------------------------------------------ mask + compaction
def test_mask_kernels_equal_the_reference_bit_for_bit_at_edge_sizes(gpu):
    bs = _block()
    for n in (1, 63, 64, 65, bs - 1, bs, bs + 1, 3 * bs + 5):
        ids, lab = _flat_case(n, seed=n)
        for p in (0.15, 0.5):
            got, want = _both(gpu, ids, None, lab, p=p)
            _check(got, want, f"N={n} p={p}")
            again, _ = _both(gpu, ids, None, lab, p=p)
            _check(again, want, f"N={n} p={p} second run")
    # many blocks: the cross-block prefix
    n = 40 * bs + 17
    ids, lab = _flat_case(n, seed=7)
    got, want = _both(gpu, ids, None, lab)
    assert int(want.counts[0]) > 1000
    _check(got, want, f"N={n}")


def test_mask_kernels_on_a_ragged_padded_batch_and_a_packed_buffer(gpu):
    g = np.random.default_rng(11)
    B, S = 4, 128
    lengths = np.array([128, 77, 5, 64])
    ids = g.integers(3, V - 1, size=(B, S), dtype=np.int64)
    am = (np.arange(S)[None, :] < lengths[:, None]).astype(np.int64)
    ids[:, 0] = 0
    ids[np.arange(B), lengths - 1] = 2
    ids[am == 0] = 1
    lab = np.where(am != 0, 0, -100)
    t = torch.from_numpy
    got, want = _both(gpu, t(ids), t(am), t(lab), p=0.3)
    assert got.input_ids.shape == (B, S) and got.labels.shape == (B, S)
    sel = want.labels != -100
    assert int(sel.sum()) > 20 and not sel[t(am) == 0].any() and not sel[:, 0].any()
    _check(got, want, "padded [4, 128]")
    # packed: [1, T = 512] rows, no attention mask, dead rows marked by the labels
    from huggingface_sagemaker_tensorflow_distributed_amd.data.packing import pack_batch

    pk = pack_batch(ids, am, lab, pad_id=1, pos_base=2, pad_pos=1, row_multiple=512)
    pids, plab = t(pk["input_ids"]), t(np.asarray(pk["labels"]))
    assert pids.shape == (1, 512) and int((plab == -100).sum()) == 512 - int(lengths.sum())
    got, want = _both(gpu, pids, None, plab, p=0.3)
    assert not (want.labels.view(-1) != -100)[int(lengths.sum()):].any()
    _check(got, want, "packed [T = 512]")


def test_mask_kernels_nothing_maskable_overflow_and_the_device_step_seed(gpu):
    from huggingface_sagemaker_tensorflow_distributed_amd.train.graph import DeviceStepSeed, step_seed

    n = 1000
    ids, lab = _flat_case(n, seed=3)
    # nothing maskable: n = 0, every buffer at its fill value
    got, want = _both(gpu, ids, torch.zeros(n, dtype=torch.int64), lab)
    assert int(want.counts[0]) == 0 and (want.tgt == -100).all()
    _check(got, want, "nothing maskable")
    # p = 1 with a capacity below N: the selections from rank cap on are dropped
    got, want = _both(gpu, ids, None, lab, p=1.0, cap=192)
    assert int(want.counts[0]) == 192 and int(want.counts[1]) > 500
    _check(got, want, "overflow")
    dropped = (want.labels == -100) & (lab != -100) & (ids > 2) & (ids != MASK)
    assert int(dropped.sum()) == int(want.counts[1]) and torch.equal(got.input_ids.cpu()[dropped], ids[dropped])
    # the device step seed, set (XORed in, as for dropout) and unset again
    plain, want_plain = _both(gpu, ids, None, lab)
    ds = DeviceStepSeed(gpu, 5, 0)
    try:
        ds.set_step(3)
        got, want = _both(gpu, ids, None, lab, step_seed=step_seed(5, 0, 3))
        _check(got, want, "device step seed set")
        assert not torch.equal(want.labels, want_plain.labels)
        off = _ops().mlm_mask(ids.to(gpu), None, lab.to(gpu), SEED, 0.15, MASK, SPECIAL, RANGE, use_step_seed=False)
        _check(off, want_plain, "device step seed set but not used (evaluation)")
    finally:
        ds.close()
    after, _ = _both(gpu, ids, None, lab)
    _check(after, want_plain, "device step seed unset")
    _check(plain, want_plain, "no device step seed")


# ------------------------------------------------------------------------------------------ row scatter
@pytest.mark.parametrize("H", [64, 1024])
def test_row_scatter_equals_index_copy_on_a_zeroed_buffer(gpu, H):
    from huggingface_sagemaker_tensorflow_distributed_amd.ops import hip

    g = torch.Generator().manual_seed(H)
    cap = 64
    dx = torch.randn(cap, H, generator=g).bfloat16().to(gpu)
    for N in (1, 65, 1000):
        full = min(cap, N)
        for n in (0, full, full // 2):
            pos = torch.randperm(N, generator=g)[:n].sort().values
            inv = torch.full((N,), -1, dtype=torch.int32)
            inv[pos] = torch.arange(n, dtype=torch.int32)
            want = torch.zeros(N, H, dtype=torch.bfloat16, device=gpu)
            want.index_copy_(0, pos.to(gpu), dx[:n])
            got = torch.full((N, H), float("nan"), dtype=torch.bfloat16, device=gpu)  # every row must be written
            hip._C.mlm_scatter_rows(dx, inv.to(gpu), got)
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (H, N, n)


# ------------------------------------------------------------------------------------------ fixed-capacity head
def _models(gpu, layers=2):
    from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model, resolve_config
    from huggingface_sagemaker_tensorflow_distributed_amd.parallel import FlatParamStore

    cfg = resolve_config("roberta-base").replace(num_hidden_layers=layers)
    m = build_model(cfg, task="masked-lm", seed=0).to(gpu)
    m.rng.base_seed = 5
    store = FlatParamStore(m, gpu, compute_dtype=torch.bfloat16)
    return cfg, m, store


def _raw(cfg, B, S, seed, lengths=None):
    g = np.random.default_rng(seed)
    ids = g.integers(3, cfg.vocab_size - 1, size=(B, S), dtype=np.int64)
    lengths = np.full(B, S) if lengths is None else np.asarray(lengths)
    am = (np.arange(S)[None, :] < lengths[:, None]).astype(np.int64)
    ids[:, 0] = cfg.bos_token_id
    ids[np.arange(B), lengths - 1] = cfg.eos_token_id
    ids[am == 0] = cfg.pad_token_id
    t = torch.from_numpy
    return t(ids), t(am), t(np.where(am != 0, 0, -100))


HEAD = ("lm_dense_weight", "lm_dense_bias", "lm_ln_weight", "lm_ln_bias", "lm_bias")


def test_fixed_capacity_head_is_as_close_to_fp32_as_the_static_head(gpu):
    """roberta-base cut to 2 layers, B = 4, S = 128, bf16, dropout on (the masks are shared bit for bit with the CPU).
    The static head and the fixed-capacity head run on the same (ids', labels'); each is compared with the fp32 CPU
    model's loss and head gradients, and the dynamic path's error may be at most 1.5 x the static path's (the factor
    only because cap and ceil(n / 64) * 64 rows may plan their GEMMs differently).

    Measured on one MI355X (this test's printout, profiles/mlm_dynamic/head_vs_static.log; n = 64, cap = 128): loss
    error 7.92e-5 static / 8.01e-5 dynamic; relative gradient errors equal to four digits in both paths: dense weight
    7.735e-3, dense bias 5.071e-3, LN weight 7.901e-3, LN bias 2.479e-3, decoder bias 6.272e-5."""
    from huggingface_sagemaker_tensorflow_distributed_amd.models import build_model
    from huggingface_sagemaker_tensorflow_distributed_amd.ops.rng import DropoutSeeds, mlm_mask_reference

    cfg, m, store = _models(gpu)
    ids, am, lab = _raw(cfg, 4, 128, seed=21, lengths=[128, 128, 90, 128])
    seeds = DropoutSeeds(5)
    seeds.new_step(0)
    mk = mlm_mask_reference(ids, am, lab, seeds.mlm_seed(), 0.15, m.mask_token_id, m.mlm_special_ids(),
                            m.mlm_rand_range())
    n = int(mk.counts[0])
    assert 40 < n < mk.cap

    cpu = build_model(cfg, task="masked-lm", seed=0).train()
    cpu.rng.base_seed = 5
    cpu.rng.new_step(0)
    l_ref, _ = cpu(mk.input_ids, attention_mask=am, labels=mk.labels)
    l_ref.backward()
    g_ref = {k: dict(cpu.named_parameters())[k].grad.clone() for k in HEAD}

    def gpu_step(mode, x, y):
        m.set_mlm_masking(mode, 0.15)
        m.train()
        m.rng.new_step(0)
        store.zero_grad()
        loss, logits = m(x.to(gpu), attention_mask=am.to(gpu), labels=y.to(gpu))
        assert getattr(loss, "_hsd_correct", None) is not None, "the fused HIP head did not run"
        loss.backward()
        torch.cuda.synchronize()
        params = dict(m.named_parameters())
        return float(loss), {k: params[k].main_grad.float().cpu().clone() for k in HEAD}, logits, loss

    l_st, g_st, lg_st, _ = gpu_step("static", mk.input_ids, mk.labels)
    l_dy, g_dy, lg_dy, loss_dy = gpu_step("dynamic", ids, lab)
    assert lg_st.shape == (n, cfg.vocab_size) and lg_dy.shape == (mk.cap, cfg.vocab_size)
    st = loss_dy._hsd_stats.cpu()
    assert float(st[2]) == n and abs(float(st[3]) / n - l_dy) <= 1e-6 * max(1.0, abs(l_dy))
    assert m.mlm_dropped() == 0

    err = {"loss": (abs(l_st - float(l_ref)), abs(l_dy - float(l_ref)))}
    for k in HEAD:
        ref_n = float(g_ref[k].norm())
        err[k] = (float((g_st[k] - g_ref[k]).norm()) / ref_n, float((g_dy[k] - g_ref[k]).norm()) / ref_n)
    for k, (e_st, e_dy) in err.items():
        print(f"{k}: static error {e_st:.4e}  dynamic error {e_dy:.4e}  (n={n}, cap={mk.cap})")
    for k, (e_st, e_dy) in err.items():
        assert e_dy <= 1.5 * e_st, f"{k}: dynamic {e_dy:.4e} > 1.5 x static {e_st:.4e}"


def test_nothing_maskable_gives_a_zero_loss_and_finite_zero_head_gradients(gpu):
    cfg, m, store = _models(gpu, layers=1)
    ids, am, lab = _raw(cfg, 2, 128, seed=22)
    m.set_mlm_masking("dynamic", 0.15)
    m.train()
    m.rng.new_step(0)
    store.zero_grad()
    loss, _ = m(ids.to(gpu), attention_mask=am.to(gpu), labels=torch.full_like(lab, -100).to(gpu))
    loss.backward()
    torch.cuda.synchronize()
    assert float(loss) == 0.0 and float(loss._hsd_stats[2]) == 0.0
    assert torch.isfinite(store.grad).all() and torch.count_nonzero(store.grad) == 0


# ------------------------------------------------------------------------------------------ graphs
def test_mask_and_head_capture_into_a_graph_and_replay_with_fresh_masks(gpu):
    """ops.mlm_mask + the fixed-capacity head inside torch.cuda.graph: the capture succeeding shows that nothing
    synchronises; each replay under a new device step seed equals the eager result for that seed."""
    from huggingface_sagemaker_tensorflow_distributed_amd.train.graph import DeviceStepSeed, step_seed

    ops, rng = _ops(), _rng()
    torch.manual_seed(3)
    N, H, Vp = 512, 256, 50432
    mkp = lambda *s, sc=0.05: (torch.randn(*s, device=gpu) * sc).bfloat16()  # noqa: E731
    h = torch.randn(N, H, device=gpu).bfloat16()
    w1, b1, lw, lb = mkp(H, H), mkp(H), (1 + 0.1 * torch.randn(H, device=gpu)).bfloat16(), mkp(H)
    wemb, bias = mkp(Vp, H), mkp(Vp)
    wemb[V:] = 0
    bias[V:] = 0
    ids, lab = _flat_case(N, seed=5)
    ids_d, lab_d = ids.to(gpu), lab.to(gpu)

    def run():
        mk = ops.mlm_mask(ids_d, None, lab_d, SEED, 0.15, MASK, SPECIAL, RANGE)
        loss, _ = ops.mlm_head_fixed(h, mk, w1, b1, lw, lb, 1e-5, wemb, bias, V)
        return mk, loss

    ds = DeviceStepSeed(gpu, 9, 0)
    try:
        with torch.no_grad():
            ds.set_step(0)
            s = torch.cuda.Stream(device=gpu)
            s.wait_stream(torch.cuda.current_stream(gpu))
            with torch.cuda.stream(s):
                run()
            torch.cuda.current_stream(gpu).wait_stream(s)
            torch.cuda.synchronize(gpu)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                mk_g, loss_g = run()
            seen = []
            for step in (1, 2):
                ds.set_step(step)
                graph.replay()
                torch.cuda.synchronize(gpu)
                replay = {f: getattr(mk_g, f).cpu().clone() for f in FIELDS}
                loss_replay = float(loss_g)
                mk_e, loss_e = run()
                want = rng.mlm_mask_reference(ids, None, lab, SEED, 0.15, MASK, SPECIAL, RANGE,
                                              step_seed=step_seed(9, 0, step))
                for f in FIELDS:
                    assert torch.equal(replay[f], getattr(want, f)), (step, f)
                    assert torch.equal(replay[f], getattr(mk_e, f).cpu()), (step, f)
                assert abs(loss_replay - float(loss_e)) <= 1e-5 * abs(float(loss_e)), (loss_replay, float(loss_e))
                assert loss_replay > 0
                seen.append(replay["labels"])
            assert not torch.equal(seen[0], seen[1])
    finally:
        ds.close()


def test_trainer_whole_step_graph_matches_eager_in_dynamic_mode(gpu):
    """Three whole-step optimizer steps of a dynamic-masking MLM trainer, replayed from the captured graph against
    the same steps run eagerly with graph-mode seeding: the bounds of tests/test_gpu_graph.py."""
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedAdam
    from huggingface_sagemaker_tensorflow_distributed_amd.train.trainer import Trainer

    res = {}
    for replay in (False, True):
        cfg, m, store = _models(gpu)
        m.set_mlm_masking("dynamic", 0.15)
        assert m.graph_safe
        opt = FusedAdam(store, lr=1e-4)
        tr = Trainer(m, store, opt, None, gpu, hip_graph=True)
        assert tr._seed is not None, "--hip_graph must accept the dynamic-masking MLM model"
        tr._graph_replay = replay
        batches = []
        for i in range(3):
            ids, am, lab = _raw(cfg, 8, 128, seed=30 + i, lengths=[128, 128, 128, 100, 128, 128, 64, 128])
            batches.append({"input_ids": ids.to(gpu), "attention_mask": am.to(gpu), "labels": lab.to(gpu)})
        try:
            losses = [float(tr.train_step([b])) for b in batches]
            if replay:
                assert len(tr._graphs) == 1 and tr._full_graph
            torch.cuda.synchronize()
            res[replay] = (losses, tr.store.master.clone(), m.mlm_dropped())
        finally:
            tr._seed.close()
    (l0, w0, d0), (l1, w1, d1) = res[False], res[True]
    print(f"eager losses {l0}  replayed losses {l1}")
    for a, b in zip(l0, l1):
        assert abs(a - b) <= 2e-3 * max(1.0, abs(a)), (l0, l1)
    rel = (w0 - w1).norm() / w0.norm()
    assert rel < 1e-4, float(rel)
    assert len({round(x, 6) for x in l1}) == 3
    assert d0 == 0 and d1 == 0


def test_static_mode_still_refuses_hip_graph(gpu):
    from huggingface_sagemaker_tensorflow_distributed_amd.optim import FusedAdam
    from huggingface_sagemaker_tensorflow_distributed_amd.train.trainer import Trainer

    cfg, m, store = _models(gpu, layers=1)
    assert m.mlm_masking == "static" and not m.graph_safe
    tr = Trainer(m, store, FusedAdam(store, lr=1e-4), None, gpu, hip_graph=True)
    assert tr._seed is None
