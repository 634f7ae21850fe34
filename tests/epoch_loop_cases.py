"""Scripted runs of the epoch loop's bookkeeping (libgnnmp K21), shared by test_epoch_loop_host.py (the numpy
mirror against a literal transcription of train_gnn.main's loop) and test_gpu_epoch_loop.py (the kernel
against the mirror).

A case is (patience, max_epochs, [(ap, ap_status, loss), ...]): one tuple per launch, the launches after the
stop included — their inputs would change the state if the run were not frozen.  The sources of launch i
(0-based) are ``sources(i)``: every launch sees other bytes.
"""
import numpy as np

NAN = float("nan")

CASES = {
    # a strictly rising AP: every epoch is the best one; ends on max_epochs
    "rising": (2, 5, [(0.1, 0, 1.0), (0.2, 0, 0.9), (0.3, 0, 0.8), (0.4, 0, 0.7), (0.5, 0, 0.6),
                      (0.9, 0, 0.1), (0.95, 0, 0.05)]),
    # a tie with the best is "not better"
    "tie": (3, 10, [(0.5, 0, 1.0), (0.5, 0, 0.9), (0.6, 0, 0.8), (0.6, 0, 0.7), (0.6, 0, 0.6), (0.6, 0, 0.5),
                    (0.99, 0, 0.4), (0.999, 0, 0.3)]),
    # a NaN AP is "not better" and does not poison best_val
    "nan": (2, 8, [(0.3, 0, 1.0), (NAN, 0, NAN), (0.4, 0, 0.8), (NAN, 0, 0.7), (NAN, 0, 0.6), (0.9, 0, 0.5),
                   (0.95, 0, 0.4)]),
    # a first AP of -1.0 or below never beats the initial -1.0
    "first_below": (5, 4, [(-1.0, 0, 1.0), (-2.0, 0, 0.9), (0.2, 0, 0.8), (0.1, 0, 0.7), (0.9, 0, 0.6), (0.95, 0, 0.5)]),
    # ... and a run that never beats it ends without a best epoch
    "never_best": (2, 9, [(-1.0, 0, 1.0), (-1.0, 0, 0.9), (0.5, 0, 0.8), (0.6, 0, 0.7)]),
    # patience reached exactly
    "patience_exact": (2, 10, [(0.5, 0, 1.0), (0.4, 0, 0.9), (0.3, 0, 0.8), (0.9, 0, 0.7), (0.95, 0, 0.6)]),
    # patience 0: the first epoch ends the run, and is still the best one
    "patience_zero": (0, 10, [(0.5, 0, 1.0), (0.9, 0, 0.9), (0.95, 0, 0.8)]),
    # max_epochs reached with an improvement on the last epoch
    "max_improves_last": (5, 3, [(0.1, 0, 1.0), (0.05, 0, 0.9), (0.3, 0, 0.8), (0.9, 0, 0.7), (0.95, 0, 0.6)]),
    # a status bit at epoch 3: the run ends there, the state of epoch 2 stays the best
    "status_at_3": (5, 6, [(0.1, 0, 1.0), (0.2, 0, 0.9), (0.9, 1, 0.8), (0.95, 0, 0.7), (0.99, 4, 0.6)]),
}

# entry sizes in bytes: 4 .. 20 (every bytes % 16), a span of blocks with a ragged tail, nothing, an int64
RAGGED = 4 * (64 * 1024 + 3)
SIZES = (4, 8, 12, 16, 20, RAGGED, 0, 8)
INT64_ENTRY = 7  # the entry that is one int64 (num_batches_tracked)


def sources(launch, sizes=SIZES):
    """The source arrays of 0-based ``launch``: f32 entries (an int64 one at INT64_ENTRY), other bytes every launch."""
    out = []
    for j, nb in enumerate(sizes):
        if sizes is SIZES and j == INT64_ENTRY:
            out.append(np.array([(launch + 1) * (1 << 40) + 12345], dtype=np.int64))
        else:
            n = nb // 4
            out.append(((np.arange(n, dtype=np.float64) * 0.37 + 17.0 * (launch + 1) + j) % 1013.0).astype(np.float32))
    return out


def blank(sizes=SIZES):
    """The destinations before a run: a byte pattern no source holds."""
    return [np.full(nb, 0xA5, dtype=np.uint8) for nb in sizes]


class _Status(Exception):
    pass


def main_loop(patience, max_epochs, script, sizes=SIZES):
    """train_gnn.main's loop, transcribed: epoch e trains (``sources(e - 1)`` is the state dict after it),
    evaluates (script[e - 1]), then the four lines.  Returns what the device state block, the logs and the
    destinations must hold when the loop ends (a status word raises in main: the run ends at that epoch)."""
    best_val, best_state, bad = -1.0, None, 0
    best_epoch = stop_epoch = status = epoch = 0
    loss_log = np.zeros(max_epochs, dtype=np.float32)
    ap_log = np.zeros(max_epochs, dtype=np.float64)
    try:
        for epoch in range(1, max_epochs + 1):
            pr_val, st, loss = script[epoch - 1]
            state_dict = sources(epoch - 1, sizes)
            loss_log[epoch - 1], ap_log[epoch - 1] = loss, pr_val
            if st != 0:
                raise _Status(st)
            if pr_val > best_val:
                best_val, bad = pr_val, 0
                best_state = [v.copy() for v in state_dict]
                best_epoch = epoch
            else:
                bad += 1
            if bad >= patience:
                break
    except _Status as exc:
        status = exc.args[0]
    stop_epoch = epoch
    dsts = blank(sizes) if best_state is None else [v.view(np.uint8).copy() for v in best_state]
    return dict(epoch=epoch, bad=bad, best_epoch=best_epoch, stop_epoch=stop_epoch, status=status, best_val=best_val,
                loss_log=loss_log, ap_log=ap_log, dsts=dsts)
