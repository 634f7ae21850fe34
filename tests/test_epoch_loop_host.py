"""CPU side of the epoch loop (libgnnmp K21, epoch_loop.py): the numpy mirror of gnn_epoch_keep_best against a
literal transcription of train_gnn.main's loop, the additive ABI check, the entry point's host validation,
and train_gnn.main with ``epoch_block`` where the key cannot apply.  No device calls."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import epoch_loop_cases as ec
from elliptic_gnn_project_amd import _lib, epoch_loop, train_gnn

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "gnnmp.h"
LIB = ROOT / "elliptic_gnn_project_amd" / "libgnnmp.so"
K21 = ("gnn_epoch_keep_best",)


# ----------------------------------------------------------------------------- the mirror
def run_mirror(patience, max_epochs, script, sizes=ec.SIZES):
    state = epoch_loop.initial_state()
    loss_log = np.zeros(max_epochs, dtype=np.float32)
    ap_log = np.zeros(max_epochs, dtype=np.float64)
    dsts = ec.blank(sizes)
    snaps = []
    for i, (ap, st, loss) in enumerate(script):
        epoch_loop.host_keep_best(state, ap, st, loss, ec.sources(i, sizes), dsts, patience, max_epochs, loss_log, ap_log)
        snaps.append((state.tobytes(), loss_log.tobytes(), ap_log.tobytes(), b"".join(d.tobytes() for d in dsts)))
    return state, loss_log, ap_log, dsts, snaps


@pytest.mark.parametrize("name", list(ec.CASES))
def test_mirror_is_mains_loop(name):
    patience, max_epochs, script = ec.CASES[name]
    want = ec.main_loop(patience, max_epochs, script)
    state, loss_log, ap_log, dsts, snaps = run_mirror(patience, max_epochs, script)
    assert len(script) > want["stop_epoch"], "the script launches past the stop"
    for k in ("epoch", "bad", "best_epoch", "stop_epoch", "status"):
        assert int(state[k]) == want[k], k
    assert int(state["reserved"]) == 0
    assert np.float64(state["best_val"]).tobytes() == np.float64(want["best_val"]).tobytes()
    assert loss_log.tobytes() == want["loss_log"].tobytes() and ap_log.tobytes() == want["ap_log"].tobytes()
    for j, (d, w) in enumerate(zip(dsts, want["dsts"])):
        assert d.tobytes() == w.tobytes(), f"entry {j}"
    # the launches after the stop, with other sources and inputs that would win: nothing moves
    stop = want["stop_epoch"]
    for later in snaps[stop:]:
        assert later == snaps[stop - 1]


def test_mirror_case_table_covers_the_rule():
    ends = {n: ec.main_loop(*ec.CASES[n]) for n in ec.CASES}
    assert ends["rising"]["best_epoch"] == ends["rising"]["stop_epoch"] == 5
    assert ends["tie"]["best_epoch"] == 3 and ends["tie"]["stop_epoch"] == 6
    assert ends["nan"]["best_epoch"] == 3 and ends["nan"]["stop_epoch"] == 5 and ends["nan"]["best_val"] == 0.4
    assert ends["first_below"]["best_epoch"] == 3 and ends["never_best"]["best_epoch"] == 0
    assert ends["never_best"]["best_val"] == -1.0 and ends["never_best"]["stop_epoch"] == 2
    assert ends["patience_exact"]["stop_epoch"] == 3 and ends["patience_exact"]["bad"] == 2
    assert ends["patience_zero"]["stop_epoch"] == 1 and ends["patience_zero"]["best_epoch"] == 1
    assert ends["max_improves_last"]["stop_epoch"] == ends["max_improves_last"]["best_epoch"] == 3
    assert ends["status_at_3"]["stop_epoch"] == 3 and ends["status_at_3"]["status"] == 1
    assert ends["status_at_3"]["best_epoch"] == 2


def test_mirror_refuses_bad_arguments():
    st, ll, al = epoch_loop.initial_state(), np.zeros(2, np.float32), np.zeros(2, np.float64)
    a = [np.zeros(2, np.float32)]
    with pytest.raises(ValueError):
        epoch_loop.host_keep_best(st, 0.5, 0, 1.0, a, [np.zeros(3, np.float32)], 1, 2, ll, al)
    with pytest.raises(ValueError):
        epoch_loop.host_keep_best(st, 0.5, 0, 1.0, a * 65, a * 65, 1, 2, ll, al)
    with pytest.raises(ValueError):
        epoch_loop.host_keep_best(st, 0.5, 0, 1.0, a, a, -1, 2, ll, al)
    assert epoch_loop.STATE_BYTES == ctypes.sizeof(_lib.GnnEpochState) == 32
    assert [n for n, _ in _lib.GnnEpochState._fields_] == list(epoch_loop.STATE_DTYPE.names)
    for name in epoch_loop.STATE_DTYPE.names:
        assert epoch_loop.STATE_DTYPE.fields[name][1] == getattr(_lib.GnnEpochState, name).offset, name


# ----------------------------------------------------------------------------- ABI
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_k21_is_additive_to_abi_32(lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert int(re.search(r"#define GNNMP_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == lib.gnn_abi_version() == 32
    exported = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], capture_output=True, text=True, check=True).stdout
    for fn in K21:
        proto = re.search(r"gnn_status\s+%s\s*\((.*?)\)\s*;" % fn, text, re.S)
        assert proto, fn
        nargs = len([a for a in proto.group(1).split(",") if a.strip()])
        assert fn in _lib.SIGNATURES and len(_lib.SIGNATURES[fn][1]) == nargs, fn
        assert f" T {fn}\n" in exported, fn
    for name, value in (("GNN_EPOCH_MAX_TENSORS", _lib.EPOCH_MAX_TENSORS), ("GNN_EPOCH_CHUNK_BYTES", _lib.EPOCH_CHUNK_BYTES)):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value, name
    # the structs, field by field in the header's order
    for cname, cls in (("gnn_epoch_tensor", _lib.GnnEpochTensor), ("gnn_epoch_table", _lib.GnnEpochTable),
                       ("gnn_epoch_state", _lib.GnnEpochState)):
        body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % cname, text).group(1)
        names = [re.search(r"(\w+)\s*(\[\w+\])?$", d.strip()).group(1) for d in body.split(";") if d.strip()]
        assert names == [n for n, _ in cls._fields_], cname
    assert ctypes.sizeof(_lib.GnnEpochTensor) == 24 and ctypes.sizeof(_lib.GnnEpochTable) == 8 + 24 * 64
    assert (ROOT / "elliptic_gnn_project_amd" / "csrc" / "epoch.hip").exists()
    assert re.search(r"^SRCS :=.*\bepoch\.hip\b", (ROOT / "elliptic_gnn_project_amd" / "csrc" / "Makefile").read_text(), re.M)


def test_k21_entry_point_validates_on_the_host(lib):
    """Bad arguments are refused before any launch (no GPU needed: the pointers are never dereferenced)."""
    one, INVALID = ctypes.c_void_p(1 << 20), 1

    def table(n=1, src=1 << 20, dst=1 << 21, nbytes=16):
        t = _lib.GnnEpochTable()
        t.num_tensors = n
        for j in range(max(0, min(n, _lib.EPOCH_MAX_TENSORS))):
            t.tensors[j].src, t.tensors[j].dst, t.tensors[j].bytes = src, dst, nbytes
        return t

    def call(ap=one, st=one, loss=one, tab=None, patience=1, max_epochs=2, state=one, ll=one, al=one):
        tab = table() if tab is None else tab
        return lib.gnn_epoch_keep_best(ap, st, loss, ctypes.byref(tab) if tab is not False else None, patience,
                                       max_epochs, state, ll, al, None)

    for bad in (dict(ap=None), dict(st=None), dict(loss=None), dict(tab=False), dict(state=None), dict(ll=None),
                dict(al=None), dict(patience=-1), dict(max_epochs=0), dict(tab=table(n=-1)), dict(tab=table(n=65)),
                dict(tab=table(nbytes=-4)), dict(tab=table(nbytes=6)), dict(tab=table(src=None)), dict(tab=table(dst=None)),
                dict(tab=table(src=(1 << 20) + 2)), dict(tab=table(dst=(1 << 21) + 1))):
        assert call(**bad) == INVALID, bad
        assert b"gnn_epoch_keep_best" in lib.gnn_last_error()


# ----------------------------------------------------------------------------- train_gnn.main where the key cannot apply
def small_cfg(tmp_path, name, **kw):
    """test_baselines_host.small_cfg's graph (1,500 nodes, 2,000 edges, 12 features) under train_gnn.main's keys."""
    cfg = dict(run_name=name, seed=1, arch="sage", hidden_dim=16, layers=2, dropout=0.2, lr=0.01, weight_decay=1e-4,
               max_epochs=6, patience=3, grad_clip=1.0, amp=False, symmetrize_edges=True, use_time_scalar=True,
               train_window_k=10, calibrate_temperature=True, topk=20, device="cpu", output_root=str(tmp_path),
               graph_file=str(tmp_path / "no_such_graph.npz"),
               synthetic=dict(num_nodes=1500, num_edges=2000, num_feats=12, seed=5, num_illicit=150, num_licit=900))
    cfg.update(kw)
    return cfg


def _tree(root):
    """Every file under ``root`` with its bytes (without the optional TensorBoard directory: its file names carry
    the time)."""
    return sorted((str(p.relative_to(root)), p.read_bytes() if p.is_file() else None) for p in root.rglob("*")
                  if "tb" not in p.relative_to(root).parts)


def test_main_on_cpu_is_the_key_absent_run(tmp_path, capsys):
    """``device: cpu`` with ``epoch_block: 4`` is the key-absent run.  train_gnn.main has no CPU path — get_device
    refuses ``device: cpu`` and GraphPlan refuses host tensors: the kernels are the product — so on this side
    the key-absent run is the RuntimeError of get_device and what the run directory holds by then; the keyed
    run must be that, byte for byte.  The ``[LOOP] ... ignored`` line and the byte-equal files of a run that
    does train are checked where main runs: test_gpu_epoch_loop.py (``mini_batch``, a loss outside the fused
    CE).  The reason main would print off the GPU is checked below."""
    errs = {}
    for name, extra in (("absent", {}), ("keyed", dict(epoch_block=4))):
        cfg = small_cfg(tmp_path / name, "run", **extra)
        with pytest.raises(RuntimeError) as exc:
            train_gnn.main(cfg)
        errs[name] = str(exc.value)
        assert "[LOOP]" not in capsys.readouterr().out  # nothing to ignore yet: the run ends before the loop
    assert errs["absent"] == errs["keyed"] and "device='cpu'" in errs["absent"]
    assert _tree(tmp_path / "absent") == _tree(tmp_path / "keyed") and _tree(tmp_path / "absent")
    why = epoch_loop.ignored_reason(torch.device("cpu"), False, None, None, False, None)
    assert why == "the device is not a CUDA device"
    assert epoch_loop.ignored_reason("cpu", True, None, None, True, 5) == why  # the device is looked at first


def test_main_refuses_the_key_across_ranks(tmp_path, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(NotImplementedError, match="epoch_block"):
        train_gnn.main(small_cfg(tmp_path, "ranks", epoch_block=4, world_size=2))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="epoch_block"):
        train_gnn.main(small_cfg(tmp_path, "ranks_env", epoch_block=2))
    with pytest.raises(ValueError, match="epoch_block"):
        train_gnn.main(small_cfg(tmp_path, "negative", epoch_block=-1))
    assert not (tmp_path / "gnn").exists(), "refused before the run directory is made"


def test_capture_unsafe_reasons():
    """What makes main ignore the key on the GPU: another optimizer, a loss the fused CE does not cover, AMP's
    GradScaler form."""
    from elliptic_gnn_project_amd.train_ops import ClipAdam

    p = [torch.nn.Parameter(torch.zeros(3))]
    adam, clip, clip_amp = torch.optim.Adam(p), ClipAdam(p, lr=0.1), ClipAdam(p, lr=0.1, skip_nonfinite=True)

    class Loss:
        fusable = True

    class Torch:
        fusable = False

    assert epoch_loop.capture_unsafe_reason(clip, Loss, False, 10) is None
    assert epoch_loop.capture_unsafe_reason(clip_amp, Loss, True, 10) is None
    assert "ClipAdam" in epoch_loop.capture_unsafe_reason(adam, Loss, False, 10)
    assert "loss" in epoch_loop.capture_unsafe_reason(clip, Torch, False, 10)
    assert "loss" in epoch_loop.capture_unsafe_reason(clip, Loss, False, None)
    assert "amp" in epoch_loop.capture_unsafe_reason(clip, Loss, True, 10)
    cuda = torch.device("cuda", 0)  # (a name only: nothing is allocated)
    assert epoch_loop.ignored_reason(cuda, True, clip, Loss, False, 10).startswith("mini_batch")
    assert epoch_loop.ignored_reason(cuda, False, clip, Loss, False, 10) is None
    assert "ClipAdam" in epoch_loop.ignored_reason(cuda, False, adam, Loss, False, 10)
    with pytest.raises(ValueError, match="64"):
        epoch_loop.KeepBest([torch.zeros(1)] * 65, [torch.zeros(1)] * 65, 1, 2)
