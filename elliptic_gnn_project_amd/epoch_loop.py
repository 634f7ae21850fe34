"""Whole runs from captured epochs: train_gnn.main's epoch loop with its best-state and early-stopping
bookkeeping on the device (libgnnmp K21, csrc/epoch.hip), so that a block of epochs is enqueued — replayed
from one HIP graph — without a host decision between them.

* ``host_keep_best``: the numpy mirror of ``gnn_epoch_keep_best`` (include/gnnmp.h), bit-equal in every
  state word, both logs and every destination byte; the kernel's test oracle.
* ``KeepBest``: the device state block, the two logs and the (src, dst, bytes) table of one run.
* ``EpochLoop``: one epoch = train_epoch(sync=False) -> eval_split_device -> rank_metrics.average_precision
  over the validation mask -> gnn_epoch_keep_best, captured by train_gnn.CapturedStep; ``run(block=K)``
  replays K epochs, then reads the state block and the logs in one transfer.

The rule of one launch is the loop of train_gnn.main:

    if stop_epoch != 0 (or epoch >= max_epochs): return          # frozen: nothing is read or written
    e = epoch + 1; epoch = e; loss_log[e-1] = loss; ap_log[e-1] = ap
    if ap_status != 0:  status |= ap_status; stop_epoch = e       # the host raises, as check_status does
    else:
        if ap > best_val: best_val = ap; bad = 0; best_epoch = e; copy every src -> dst
        else:             bad += 1                                # a tie or a NaN AP is "not better"
        if bad >= patience or e == max_epochs: stop_epoch = e

Under capture the fused layers draw their dropout masks from a device counter (fused.dropout_seeds), not
from the host's per-step seeds: a run through EpochLoop is a reproducible stream of its own — the same
seed gives the same bytes whatever the block size — and not the bytes of train_gnn.main's eager loop.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib

STATE_DTYPE = np.dtype([("epoch", "<i4"), ("bad", "<i4"), ("best_epoch", "<i4"), ("stop_epoch", "<i4"),
                        ("status", "<i4"), ("reserved", "<i4"), ("best_val", "<f8")])
STATE_BYTES = STATE_DTYPE.itemsize  # 32 = sizeof(gnn_epoch_state)


def initial_state() -> np.ndarray:
    """The state block a run starts from: all zero, best_val = -1.0 (train_gnn.main's ``best_val``)."""
    s = np.zeros((), dtype=STATE_DTYPE)
    s["best_val"] = -1.0
    return s


# ----------------------------------------------------------------------------- host mirror
def host_keep_best(state: np.ndarray, ap, ap_status, loss, srcs: Sequence[np.ndarray], dsts: Sequence[np.ndarray],
                   patience: int, max_epochs: int, loss_log: np.ndarray, ap_log: np.ndarray) -> None:
    """One ``gnn_epoch_keep_best`` launch on host arrays, in place: ``state`` a 0-d STATE_DTYPE array,
    ``loss_log`` f32 [max_epochs], ``ap_log`` f64 [max_epochs], ``srcs`` / ``dsts`` arrays of equal byte
    sizes (copied as bytes)."""
    if len(srcs) != len(dsts) or len(srcs) > _lib.EPOCH_MAX_TENSORS:
        raise ValueError(f"host_keep_best: {len(srcs)} sources, {len(dsts)} destinations "
                         f"(at most {_lib.EPOCH_MAX_TENSORS})")
    if patience < 0 or max_epochs < 1:
        raise ValueError("host_keep_best: patience < 0 or max_epochs < 1")
    if int(state["stop_epoch"]) != 0 or int(state["epoch"]) >= max_epochs:
        return
    e = int(state["epoch"]) + 1
    ap = np.float64(ap)
    state["epoch"] = e
    loss_log[e - 1] = np.float32(loss)
    ap_log[e - 1] = ap
    if int(ap_status) != 0:
        state["status"] = int(state["status"]) | int(ap_status)
        state["stop_epoch"] = e
        return
    if ap > state["best_val"]:  # (False for a NaN)
        state["best_val"] = ap
        state["bad"] = 0
        state["best_epoch"] = e
        for s, d in zip(srcs, dsts):
            sb, db = _bytes_view(s), _bytes_view(d)
            if sb.size != db.size or sb.size % 4:
                raise ValueError("host_keep_best: an entry's sizes differ or are no multiple of 4 bytes")
            db[:] = sb
    else:
        state["bad"] = int(state["bad"]) + 1
    if int(state["bad"]) >= patience or e == max_epochs:
        state["stop_epoch"] = e


def _bytes_view(a: np.ndarray) -> np.ndarray:
    if not a.flags.c_contiguous:
        raise ValueError("host_keep_best: entries are contiguous arrays")
    return a.reshape(-1).view(np.uint8)


# ----------------------------------------------------------------------------- device
class KeepBest:
    """The device side of one run: a state block, the two logs (one buffer: a single transfer reads all
    three) and the table of ``srcs`` -> ``dsts`` (contiguous CUDA tensors of pairwise equal byte sizes,
    multiples of 4)."""

    def __init__(self, srcs: Sequence[torch.Tensor], dsts: Sequence[torch.Tensor], patience: int, max_epochs: int,
                 device: Optional[torch.device] = None):
        if len(srcs) != len(dsts):
            raise ValueError(f"KeepBest: {len(srcs)} sources for {len(dsts)} destinations")
        if len(srcs) > _lib.EPOCH_MAX_TENSORS:
            raise ValueError(f"KeepBest: {len(srcs)} state tensors; gnn_epoch_keep_best takes at most "
                             f"{_lib.EPOCH_MAX_TENSORS} (GNN_EPOCH_MAX_TENSORS)")
        if int(patience) < 0 or int(max_epochs) < 1:
            raise ValueError("KeepBest: patience < 0 or max_epochs < 1")
        _lib.load()
        self.patience, self.max_epochs = int(patience), int(max_epochs)
        self.srcs, self.dsts = list(srcs), list(dsts)  # held: the table keeps their addresses
        self.table = _lib.GnnEpochTable()
        self.table.num_tensors = len(self.srcs)
        for j, (s, d) in enumerate(zip(self.srcs, self.dsts)):
            nb = s.numel() * s.element_size()
            if not (s.is_cuda and d.is_cuda and s.is_contiguous() and d.is_contiguous()):
                raise ValueError("KeepBest: entries are contiguous CUDA tensors")
            if nb != d.numel() * d.element_size() or nb % 4:
                raise ValueError("KeepBest: an entry's sizes differ or are no multiple of 4 bytes")
            t = self.table.tensors[j]
            t.src, t.dst, t.bytes = (s.data_ptr(), d.data_ptr(), nb) if nb else (None, None, 0)
        if device is None:
            device = self.srcs[0].device if self.srcs else torch.device("cuda", torch.cuda.current_device())
        self.device = device
        M = self.max_epochs
        self.buf = torch.zeros(STATE_BYTES + 12 * M, dtype=torch.uint8, device=device)
        self.ap_log = self.buf[STATE_BYTES:STATE_BYTES + 8 * M].view(torch.float64)
        self.loss_log = self.buf[STATE_BYTES + 8 * M:].view(torch.float32)
        self.reset()

    def reset(self) -> None:
        """The start of a run (a host-to-device copy: not for use between the epochs of a block)."""
        host = np.zeros(self.buf.numel(), dtype=np.uint8)
        host[:STATE_BYTES] = np.frombuffer(initial_state().tobytes(), dtype=np.uint8)
        self.buf.copy_(torch.from_numpy(host))

    def launch(self, ap: torch.Tensor, ap_status: torch.Tensor, loss: torch.Tensor) -> None:
        """One epoch's bookkeeping from the device scalars ``ap`` (f64), ``ap_status`` (int32) and ``loss``
        (f32), read when the launch runs; no host synchronisation, capturable."""
        if ap.dtype != torch.float64 or ap_status.dtype != torch.int32 or loss.dtype != torch.float32:
            raise ValueError("KeepBest.launch: ap is f64, ap_status int32, loss f32")
        if not (ap.is_cuda and ap_status.is_cuda and loss.is_cuda and ap.numel() and ap_status.numel() and loss.numel()):
            raise ValueError("KeepBest.launch: ap, ap_status and loss are device scalars")
        with torch.cuda.device(self.device):
            _lib.call("gnn_epoch_keep_best", ap.data_ptr(), ap_status.data_ptr(), loss.data_ptr(),
                      ctypes.byref(self.table), self.patience, self.max_epochs, self.buf.data_ptr(),
                      self.loss_log.data_ptr(), self.ap_log.data_ptr(), _lib.stream_handle(self.device))

    def read(self):
        """(state, loss_log, ap_log) as host arrays — ONE device-to-host transfer (it synchronises)."""
        host = self.buf.cpu().numpy()
        M = self.max_epochs
        state = host[:STATE_BYTES].view(STATE_DTYPE)[0].copy()
        ap_log = host[STATE_BYTES:STATE_BYTES + 8 * M].view(np.float64).copy()
        loss_log = host[STATE_BYTES + 8 * M:].view(np.float32).copy()
        return state, loss_log, ap_log


def capture_unsafe_reason(optimizer, loss_fn, use_amp: bool, denom) -> Optional[str]:
    """Why train_epoch's step with these pieces cannot be captured (None: it can): the optimizer's state
    must advance on the device (ClipAdam), the loss must be the fused CE (no torch fallback that indexes
    rows on the host) and AMP must be off or ClipAdam's exact form (no GradScaler bookkeeping)."""
    from .train_ops import ClipAdam

    if not isinstance(optimizer, ClipAdam):
        return f"the optimizer is {type(optimizer).__name__}, not ClipAdam"
    if not getattr(loss_fn, "fusable", False) or denom is None:
        return "the loss is not the fused masked cross entropy"
    if use_amp and not getattr(optimizer, "skip_nonfinite", False):
        return "amp without the fused (exact) AMP step"
    return None


def ignored_reason(device, mini_batch: bool, optimizer, loss_fn, use_amp: bool, denom) -> Optional[str]:
    """Why train_gnn.main runs its own loop although ``epoch_block`` is set (None: the key applies)."""
    if torch.device(device).type != "cuda":
        return "the device is not a CUDA device"
    if mini_batch:
        return "mini_batch runs keep the host loop"
    return capture_unsafe_reason(optimizer, loss_fn, use_amp, denom)


class EpochLoop:
    """train_gnn.main's full-batch epoch loop as replays of one captured epoch.

    ``warmup``: the eager epochs CapturedStep runs before capturing.  They leave no trace: parameters,
    buffers, ClipAdam's state, the dropout counter, torch's CPU generator and the state block are put back
    in place afterwards (the graph holds their addresses), and the B images are rebuilt from the restored
    weights (CapturedStep._refresh_preps).  ``capture_eval`` false captures the train step alone and
    launches the evaluation forward, the AP and the bookkeeping eagerly after each replay — still without
    a host synchronisation inside a block.

    ``run(block=K)``: K epochs are enqueued, then the state block and the logs cross to the host in one
    transfer; the ``training_log.csv`` rows (``logger``) and the progress lines (``verbose``) of the epochs
    that ran are written, and the loop ends when ``stop_epoch`` is set.  Status bits raise what
    rank_metrics.check_status raises.  At the end the best copies are loaded into the model in place.
    ``bookkeeping="host"``: the same captured epoch, loss and AP read every epoch and main's four Python
    lines applied to ``state_dict()`` clones — the reference the device bookkeeping is tested against.
    """

    def __init__(self, model, data, edge_index, optimizer, loss_fn, cfg: Dict, device, *, n_train: int, val_mask,
                 patience: int, max_epochs: int, use_amp: bool = False, scaler=None, warmup: int = 3,
                 capture_eval: bool = True, logger=None, verbose: bool = False):
        from . import fused, rank_metrics
        from .train_gnn import CapturedStep, eval_split_device, train_epoch

        why = capture_unsafe_reason(optimizer, loss_fn, use_amp, n_train)
        if why is not None:
            raise ValueError(f"EpochLoop: the step is not capture-safe: {why}")
        if int(warmup) < 1:
            raise ValueError("EpochLoop: warmup >= 1 (the eager epoch before a capture builds plans and workspaces)")
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("EpochLoop runs on a CUDA device")
        self.model, self.logger, self.verbose = model, logger, verbose
        self.patience, self.max_epochs = int(patience), int(max_epochs)
        if scaler is None:
            scaler = torch.amp.GradScaler(device=device.type, enabled=use_amp)
        self.state_keys = list(model.state_dict().keys())
        srcs = [v.detach() for v in model.state_dict().values()]
        if len(srcs) > _lib.EPOCH_MAX_TENSORS:
            raise ValueError(f"epoch_block: the model has {len(srcs)} state tensors; the device bookkeeping keeps "
                             f"at most {_lib.EPOCH_MAX_TENSORS} (GNN_EPOCH_MAX_TENSORS)")
        self.best = [torch.empty_like(s, memory_format=torch.contiguous_format) for s in srcs]
        self.keep = KeepBest(srcs, self.best, self.patience, self.max_epochs, device)
        vm = val_mask.to(device)
        keep = self.keep

        def step():
            return train_epoch(model, data, edge_index, optimizer, loss_fn, scaler, use_amp, cfg, device, sync=False,
                               denom=n_train)

        def tail(loss):
            y_all, p_all, _ = eval_split_device(model, data, edge_index)
            ap, st = rank_metrics.average_precision(p_all, y_all, vm, check=False, return_status=True)
            keep.launch(ap.view(1), st.view(1), loss.view(1))
            return loss, ap, st

        def epoch():
            return tail(step())

        # --- what the warm-up epochs change, cloned before them
        ctr = fused._graph_seed_counter(data.x.device)  # (the key the forwards look it up by)
        ctr.fill_(fused.seed_counter_start())  # the run's stream starts from the seed, whatever ran before
        rng = torch.get_rng_state()
        tensors = [p.detach() for p in model.parameters()] + [b.detach() for b in model.buffers()] + [ctr]
        saved = [t.clone() for t in tensors]
        opt_before = {id(t): t.clone() for t in _optimizer_tensors(optimizer)}
        self._tail = None if capture_eval else tail
        self.step = CapturedStep(epoch if capture_eval else step, warmup=int(warmup), defer_loss=True)
        # --- and put back in place: the graph holds these addresses
        with torch.no_grad():
            for t, s in zip(tensors, saved):
                t.copy_(s)
            for t in _optimizer_tensors(optimizer):  # (state the warm-up created started from zero)
                s = opt_before.get(id(t))
                if s is not None:
                    t.copy_(s)
                else:
                    t.zero_()
        torch.set_rng_state(rng)
        keep.reset()
        self.epochs_enqueued = 0

    # ------------------------------------------------------------------ one epoch, no host sync
    def _enqueue(self):
        out = self.step()
        if self._tail is not None:
            with torch.no_grad():
                out = self._tail(out)
        self.epochs_enqueued += 1
        return out

    def run(self, block: int = 1, bookkeeping: str = "device") -> Dict:
        if int(block) < 1:
            raise ValueError("EpochLoop.run: block >= 1")
        if bookkeeping not in ("device", "host"):
            raise ValueError(f"EpochLoop.run: bookkeeping={bookkeeping!r}")
        if self.epochs_enqueued:
            raise RuntimeError("EpochLoop.run: one run per EpochLoop (its state block has advanced)")
        if bookkeeping == "host":
            return self._run_host()
        from . import rank_metrics

        done, best_seen = 0, -1.0
        while True:
            for _ in range(int(block)):
                self._enqueue()
            state, loss_log, ap_log = self.keep.read()
            ran = int(state["epoch"])
            bad_status = int(state["status"]) != 0
            # main raises before it logs the epoch whose AP carried status bits
            for e in range(done + 1, ran + 1 - (1 if bad_status else 0)):
                loss, ap = float(loss_log[e - 1]), float(ap_log[e - 1])
                if ap > best_seen:
                    best_seen = ap
                self._report(e, loss, ap, best_seen)
            done = ran
            if bad_status:
                rank_metrics.check_status(torch.tensor([int(state["status"])], dtype=torch.int32))
                raise RuntimeError(f"rank_metrics: status word {int(state['status'])}")
            if int(state["stop_epoch"]) != 0:
                break
        if int(state["bad"]) >= self.patience and self.verbose:
            print("Early stopping.")
        best_epoch = int(state["best_epoch"])
        if best_epoch > 0:
            self._load(self.best)
        return dict(best_val=float(state["best_val"]), best_epoch=best_epoch, epochs=ran,
                    loss_log=loss_log[:ran].copy(), ap_log=ap_log[:ran].copy(),
                    best_state=self._named(self.best) if best_epoch > 0 else None)

    def _run_host(self) -> Dict:
        """train_gnn.main's loop over the captured epoch: one transfer [AP, status, loss] per epoch."""
        from . import rank_metrics

        best_val, best_state, bad, best_epoch = -1.0, None, 0, 0
        losses: List[float] = []
        aps: List[float] = []
        for epoch in range(1, self.max_epochs + 1):
            loss_dev, ap_dev, st_dev = self._enqueue()
            row = torch.cat([ap_dev.view(1), st_dev.view(1).to(torch.float64), loss_dev.view(1).to(torch.float64)]).cpu()
            if int(row[1]) != 0:
                rank_metrics.check_status(st_dev)
            pr_val, loss = float(row[0]), float(row[2])
            losses.append(loss)
            aps.append(pr_val)
            if pr_val > best_val:
                best_val, bad, best_epoch = pr_val, 0, epoch
                best_state = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
            else:
                bad += 1
            self._report(epoch, loss, pr_val, best_val)
            if bad >= self.patience:
                if self.verbose:
                    print("Early stopping.")
                break
        if best_state is not None:
            self._load([best_state[k] for k in self.state_keys])
        return dict(best_val=best_val, best_epoch=best_epoch, epochs=len(losses),
                    loss_log=np.asarray(losses, dtype=np.float32), ap_log=np.asarray(aps, dtype=np.float64),
                    best_state=best_state)

    # ------------------------------------------------------------------ helpers
    def _report(self, epoch: int, loss: float, ap: float, best: float) -> None:
        if self.logger is not None:
            self.logger.log_epoch(epoch, loss, ap)
        if self.verbose and (epoch % 10 == 0 or epoch == 1):
            print(f"Epoch {epoch:4d} | loss {loss:.4f} | val PR-AUC(illicit) {ap:.4f} (best {best:.4f})")

    def _named(self, tensors) -> Dict[str, torch.Tensor]:
        return {k: t.detach().clone() for k, t in zip(self.state_keys, tensors)}

    @torch.no_grad()
    def _load(self, tensors) -> None:
        """The best copies into the model's own tensors (in place: the graph and ClipAdam hold them)."""
        for dst, src in zip(self.model.state_dict().values(), tensors):
            dst.copy_(src)


def _optimizer_tensors(optimizer) -> List[torch.Tensor]:
    """Every device tensor ClipAdam's launches advance: the moments, the groups' step counters, the
    workspace (its counter word) and the norm it reports."""
    out: List[torch.Tensor] = []
    for st in optimizer.state.values():
        out += [v for k, v in sorted(st.items()) if isinstance(v, torch.Tensor) and k != "step"]
    for g in optimizer.param_groups:
        if isinstance(g.get("step_t"), torch.Tensor):
            out.append(g["step_t"])
    for name in ("_ws", "last_norm"):
        t = getattr(optimizer, name, None)
        if isinstance(t, torch.Tensor):
            out.append(t)
    return out
