"""GPU: the epoch loop (libgnnmp K21, epoch_loop.py).  gnn_epoch_keep_best against its numpy mirror over the
scripted runs of epoch_loop_cases.py; EpochLoop's device bookkeeping against the host bookkeeping for every
block size; the capture warm-up; and train_gnn.main with ``epoch_block``."""
import json

import numpy as np
import pytest
import torch

import epoch_loop_cases as ec
from elliptic_gnn_project_amd import epoch_loop

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------- kernel against mirror
GUARD = 16  # bytes of 0xA5 kept on both sides of every destination


def _device_entry(host_bytes, offset, device):
    """(the tensor handed to the kernel, its whole storage): ``offset`` bytes into a guarded allocation."""
    nb = host_bytes.size
    base = torch.full((GUARD + offset + nb + GUARD,), 0xA5, dtype=torch.uint8, device=device)
    view = base[GUARD + offset:GUARD + offset + nb]
    view.copy_(torch.from_numpy(host_bytes.copy()))
    return view, base


def _run_kernel_case(device, patience, max_epochs, script, sizes, offset):
    """Every launch of ``script`` on the device and on the mirror; all state compared after every launch."""
    # GUARD is a multiple of 16 and torch's allocations are 256-byte aligned: offset 0 takes the 16-byte
    # path, offset 4 (a view one f32 into its storage) the 4-byte path
    src = [_device_entry(s.view(np.uint8), offset, device) for s in ec.sources(0, sizes)]
    dst = [_device_entry(d, offset, device) for d in ec.blank(sizes)]
    if sizes is ec.SIZES and offset == 0:  # the int64 entry as an int64 tensor
        j = ec.INT64_ENTRY
        t = torch.zeros(1, dtype=torch.int64, device=device)
        src[j] = (t, t)
    for (v, _) in src + dst:
        assert v.numel() == 0 or v.data_ptr() % 16 == (offset % 16 if v.dtype == torch.uint8 else 0)
    kb = epoch_loop.KeepBest([v for v, _ in src], [v for v, _ in dst], patience, max_epochs, torch.device(device))
    ap_d = torch.zeros(1, dtype=torch.float64, device=device)
    st_d = torch.zeros(1, dtype=torch.int32, device=device)
    loss_d = torch.zeros(1, dtype=torch.float32, device=device)

    state = epoch_loop.initial_state()
    loss_log, ap_log = np.zeros(max_epochs, np.float32), np.zeros(max_epochs, np.float64)
    m_dst = ec.blank(sizes)
    for i, (ap, st, loss) in enumerate(script):
        h_src = ec.sources(i, sizes)
        for (v, _), h in zip(src, h_src):
            if v.numel():
                v.copy_(torch.from_numpy(h).view(v.dtype) if v.dtype == torch.int64 else torch.from_numpy(h.view(np.uint8)))
        ap_d.fill_(ap)
        st_d.fill_(st)
        loss_d.fill_(loss)
        kb.launch(ap_d, st_d, loss_d)
        epoch_loop.host_keep_best(state, ap, st, loss, h_src, m_dst, patience, max_epochs, loss_log, ap_log)
        g_state, g_loss, g_ap = kb.read()
        assert g_state.tobytes() == state.tobytes(), f"launch {i}: state {g_state} != {state}"
        assert g_loss.tobytes() == loss_log.tobytes() and g_ap.tobytes() == ap_log.tobytes(), f"launch {i}: logs"
        for j, ((v, base), m) in enumerate(zip(dst, m_dst)):
            got = base.cpu().numpy()
            lo = GUARD + offset
            assert got[lo:lo + m.size].tobytes() == m.tobytes(), f"launch {i}: entry {j} ({m.size} bytes)"
            assert (got[:lo] == 0xA5).all() and (got[lo + m.size:] == 0xA5).all(), f"launch {i}: entry {j} guard"
    return state


@pytest.mark.parametrize("offset", [0, 4], ids=["aligned16", "one_element_in"])
@pytest.mark.parametrize("name", list(ec.CASES))
def test_kernel_matches_mirror(device, name, offset):
    patience, max_epochs, script = ec.CASES[name]
    want = ec.main_loop(patience, max_epochs, script)
    state = _run_kernel_case(device, patience, max_epochs, script, ec.SIZES, offset)
    assert int(state["stop_epoch"]) == want["stop_epoch"] < len(script)  # the script launched past the stop


@pytest.mark.parametrize("offset", [0, 4], ids=["aligned16", "one_element_in"])
@pytest.mark.parametrize("entries", [1, 64])
def test_kernel_table_sizes(device, entries, offset):
    """Tables of 1 and of GNN_EPOCH_MAX_TENSORS entries (sizes cycling through every bytes % 16, nothing, and
    one entry past a block's chunk)."""
    cycle = (20, 4, 0, 8, 16, 12, 16384 + 4, 32)
    sizes = tuple(cycle[j % len(cycle)] for j in range(entries))
    patience, max_epochs, script = ec.CASES["tie"]
    _run_kernel_case(device, patience, max_epochs, script, sizes, offset)


def test_keep_best_refuses_what_the_kernel_cannot_copy(device):
    a = torch.zeros(6, dtype=torch.float32, device=device)
    with pytest.raises(ValueError):
        epoch_loop.KeepBest([a], [a[:5].clone()], 1, 2)
    with pytest.raises(ValueError):
        epoch_loop.KeepBest([a.view(2, 3).t()], [a.clone().view(3, 2)], 1, 2)
    with pytest.raises(ValueError):
        epoch_loop.KeepBest([torch.zeros(6, dtype=torch.uint8, device=device)], [torch.zeros(6, dtype=torch.uint8, device=device)], 1, 2)
    with pytest.raises(ValueError, match="64"):
        epoch_loop.KeepBest([a] * 65, [a.clone() for _ in range(65)], 1, 2)


# ----------------------------------------------------------------------------- EpochLoop
# The synthetic labels carry little signal, so the validation AP stops rising within a few epochs at any seed.
# The seeds below were picked from a probe of six (lr 0.02): under ``patience=1`` the host-bookkeeping reference
# stops at epoch 5 (sage), 2 (gcn, gat) and 3 (sage_resbn) — past epoch 1, before epoch 30 and inside a block of 4.
ARCH_CFG = {
    "sage": dict(arch="sage", dropout=0.5, seed=1),
    "gcn": dict(arch="gcn", seed=7),
    "gat": dict(arch="gat", seed=7),
    "sage_resbn": dict(arch="sage_resbn", layers=3, time_embed_dim=2, time_embed_type="learned", use_time_scalar=False,
                       time_loss_weighting="sqrt", seed=11),
}
# ends on max_epochs / ends on patience in the middle of a block
SETTINGS = {"max_epochs": dict(max_epochs=3, patience=50), "patience": dict(max_epochs=30, patience=1)}
SEED = 7  # train_gnn.main's runs below


def _cfg(arch, **kw):
    base = dict(hidden_dim=32, layers=2, heads=4, dropout=0.2, lr=0.02, weight_decay=1e-4, grad_clip=1.0, amp=False,
                symmetrize_edges=True, use_time_scalar=True, train_window_k=10, seed=SEED,
                synthetic=dict(num_nodes=8000, num_edges=12000, seed=5))
    base.update(ARCH_CFG[arch])
    base.update(kw)
    return base


_DATA = {}


def _data(cfg, device):
    """The graph as train_gnn.main prepares it, once per input layout."""
    from elliptic_gnn_project_amd.dataset_elliptic import prepare_inputs, synthetic_elliptic
    from elliptic_gnn_project_amd.planes import register_input

    key = bool(cfg["use_time_scalar"])
    if key not in _DATA:
        full = prepare_inputs(synthetic_elliptic(**cfg["synthetic"]), cfg)
        data = full.to(device)
        register_input(data.x)
        _DATA[key] = (full, data)
    return _DATA[key]


def _train(device, cfg, block, bookkeeping="device", warmup=3):
    """One run from a fresh model under cfg's seed, set up as train_gnn.main sets a run up."""
    from elliptic_gnn_project_amd import train_gnn as T

    full, data = _data(cfg, device)
    T.set_seed(cfg["seed"])
    model = T.build_model(cfg["arch"], data.x.size(1), cfg).to(device)
    opt = T.make_optimizer(model, cfg, device, False)
    cw = T.class_weight(full.y[full.train_mask])
    t_train = full.timestep[full.train_mask]
    loss_fn = T._make_loss_fn(cfg, cw, model, int(t_train.min()), int(t_train.max()))
    loop = epoch_loop.EpochLoop(model, data, data.edge_index, opt, loss_fn, cfg, device, n_train=int(full.n_train),
                                val_mask=data.val_mask, patience=cfg["patience"], max_epochs=cfg["max_epochs"],
                                warmup=warmup)
    res = loop.run(block=block, bookkeeping=bookkeeping)
    res["model_state"] = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return res


_REF = {}


def _reference(device, arch, setting):
    """The host-bookkeeping run of (arch, setting), computed once."""
    key = (arch, setting)
    if key not in _REF:
        _REF[key] = _train(device, _cfg(arch, **SETTINGS[setting]), 1, "host")
    return _REF[key]


def _assert_same_run(a, b):
    assert np.float64(a["best_val"]).tobytes() == np.float64(b["best_val"]).tobytes()
    assert a["best_epoch"] == b["best_epoch"] and a["epochs"] == b["epochs"]
    assert a["loss_log"].dtype == b["loss_log"].dtype == np.float32 and a["ap_log"].dtype == b["ap_log"].dtype == np.float64
    assert a["loss_log"].tobytes() == b["loss_log"].tobytes(), (a["loss_log"], b["loss_log"])
    assert a["ap_log"].tobytes() == b["ap_log"].tobytes(), (a["ap_log"], b["ap_log"])
    for name in ("best_state", "model_state"):  # the kept copies, and what the model was left with
        assert list(a[name]) == list(b[name])
        for k in a[name]:
            assert a[name][k].dtype == b[name][k].dtype and torch.equal(a[name][k], b[name][k]), (name, k)


@pytest.mark.parametrize("block", ["1", "4", "max_epochs+5"])
@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("arch", list(ARCH_CFG))
def test_block_size_invariance(device, arch, setting, block):
    cfg = _cfg(arch, **SETTINGS[setting])
    ref = _reference(device, arch, setting)
    print(f"{arch}/{setting}: host reference ran {ref['epochs']} epochs, best {ref['best_val']:.6f} at {ref['best_epoch']}")
    assert ref["best_epoch"] >= 1 and np.isfinite(ref["loss_log"]).all()
    if setting == "patience":  # the reference itself must stop on patience, inside the run
        assert 1 < ref["epochs"] < 30, "choose a seed / learning rate at which the reference stops early"
        assert ref["epochs"] % 4 != 0, "... and inside a block of 4, not at its end"
    else:
        assert ref["epochs"] == 3
    K = cfg["max_epochs"] + 5 if block == "max_epochs+5" else int(block)
    _assert_same_run(_train(device, cfg, K), ref)


def test_warmup_leaves_no_trace(device):
    cfg = _cfg("sage", **SETTINGS["max_epochs"])
    one, three = _train(device, cfg, 4, warmup=1), _train(device, cfg, 4, warmup=3)
    _assert_same_run(one, three)
    _assert_same_run(three, _reference(device, "sage", "max_epochs"))


def test_eager_tail_is_the_captured_epoch(device):
    """``capture_eval=False`` (the evaluation forward, the AP and the bookkeeping launched eagerly after each
    replayed train step) computes what the fully captured epoch computes."""
    from elliptic_gnn_project_amd import train_gnn as T

    cfg = _cfg("sage", **SETTINGS["max_epochs"])
    full, data = _data(cfg, device)
    T.set_seed(cfg["seed"])
    model = T.build_model(cfg["arch"], data.x.size(1), cfg).to(device)
    opt = T.make_optimizer(model, cfg, device, False)
    t_train = full.timestep[full.train_mask]
    loss_fn = T._make_loss_fn(cfg, T.class_weight(full.y[full.train_mask]), model, int(t_train.min()), int(t_train.max()))
    loop = epoch_loop.EpochLoop(model, data, data.edge_index, opt, loss_fn, cfg, device, n_train=int(full.n_train),
                                val_mask=data.val_mask, patience=cfg["patience"], max_epochs=cfg["max_epochs"],
                                capture_eval=False)
    res = loop.run(block=2)
    res["model_state"] = {k: v.detach().clone() for k, v in model.state_dict().items()}
    _assert_same_run(res, _reference(device, "sage", "max_epochs"))


# ----------------------------------------------------------------------------- train_gnn.main
def _main_cfg(tmp_path, name, **kw):
    base = dict(run_name=name, output_root=str(tmp_path), arch="sage", hidden_dim=32, layers=2, dropout=0.2, lr=0.005,
                weight_decay=1e-4, max_epochs=12, patience=3, grad_clip=1.0, amp=False, symmetrize_edges=True,
                use_time_scalar=True, train_window_k=10, calibrate_temperature=True, topk=50, seed=SEED,
                synthetic=dict(num_nodes=8000, num_edges=12000, seed=5))
    base.update(kw)
    return base


FILES = ("training_log.csv", "metrics.json", "scores_val.npy", "scores_test.npy")


def _assert_same_files(a, b):
    for f in FILES:
        assert (a / f).read_bytes() == (b / f).read_bytes(), f
    sa, sb = torch.load(a / "best.ckpt", weights_only=True), torch.load(b / "best.ckpt", weights_only=True)
    assert list(sa) == list(sb)
    for k in sa:
        assert sa[k].dtype == sb[k].dtype and torch.equal(sa[k], sb[k]), k


def test_main_with_the_key(device, tmp_path, capsys):
    from elliptic_gnn_project_amd.train_gnn import main

    runs = {}
    for K in (1, 7):
        m = main(_main_cfg(tmp_path, f"k{K}", epoch_block=K))
        out = capsys.readouterr().out
        assert "[LOOP]" not in out and "Epoch    1 | loss" in out
        runs[K] = (tmp_path / "gnn" / f"k{K}", m)
    _assert_same_files(runs[1][0], runs[7][0])
    log = (runs[7][0] / "training_log.csv").read_text().strip().splitlines()
    assert log[0] == "epoch,train_loss,val_pr_auc" and 2 <= len(log) - 1 <= 12
    assert [int(r.split(",")[0]) for r in log[1:]] == list(range(1, len(log)))
    best = max(float(r.split(",")[2]) for r in log[1:])
    m = json.loads((runs[7][0] / "metrics.json").read_text())
    assert f"{m['best_val_pr_auc']:.6f}" == f"{best:.6f}" and m["best_val_pr_auc"] == runs[7][1]["best_val_pr_auc"]
    assert "test_pr_auc_by_time" in m


def test_main_with_the_key_under_the_fused_amp_step(device, tmp_path):
    """``amp: true`` on the fp32 fused SAGENet is the fused step with ClipAdam's skip of a non-finite update
    (train_gnn.amp_is_exact): capture-safe, and the same run as ``amp: false``."""
    from elliptic_gnn_project_amd.train_gnn import main

    for amp in (False, True):
        main(_main_cfg(tmp_path, f"amp_{amp}", epoch_block=3, amp=amp, max_epochs=5))
    _assert_same_files(tmp_path / "gnn" / "amp_False", tmp_path / "gnn" / "amp_True")
    assert len((tmp_path / "gnn" / "amp_True" / "training_log.csv").read_text().strip().splitlines()) >= 3


def test_main_without_dropout_is_the_key_absent_run(device, tmp_path):
    """``dropout: 0``: no mask is drawn, so the captured stream and the eager loop with ``device_metrics`` train
    the same model — the same kernels on the same operands in the same order (DESIGN §4 "Epoch loop")."""
    from elliptic_gnn_project_amd.train_gnn import main

    main(_main_cfg(tmp_path, "absent", dropout=0.0, device_metrics=True))
    main(_main_cfg(tmp_path, "keyed", dropout=0.0, epoch_block=5))
    _assert_same_files(tmp_path / "gnn" / "absent", tmp_path / "gnn" / "keyed")


def test_main_ignores_the_key_for_a_step_that_cannot_be_captured(device, tmp_path, capsys):
    """A focal loss with gamma < 1 keeps the torch loss (not the fused CE): one ``[LOOP] ... ignored`` line and
    the files of the key-absent run."""
    from elliptic_gnn_project_amd.train_gnn import main

    extra = dict(focal_loss=True, focal_gamma=0.5, max_epochs=3)
    main(_main_cfg(tmp_path, "absent", **extra))
    out_absent = capsys.readouterr().out
    main(_main_cfg(tmp_path, "keyed", epoch_block=4, **extra))
    out_keyed = capsys.readouterr().out
    lines = [ln for ln in out_keyed.splitlines() if ln.startswith("[LOOP]")]
    assert len(lines) == 1 and lines[0].startswith("[LOOP] epoch_block ignored: ") and "loss" in lines[0]
    assert "[LOOP]" not in out_absent
    assert [ln for ln in out_keyed.splitlines() if not ln.startswith("[LOOP]")] == out_absent.splitlines()
    _assert_same_files(tmp_path / "gnn" / "absent", tmp_path / "gnn" / "keyed")
