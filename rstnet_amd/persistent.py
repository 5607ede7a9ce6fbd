"""Health of the persistent frame launches (csrc/persist.h).  A launch whose workgroups are not all resident (device shared with other
work) times out and is repaired in-stream by its one-workgroup twin: outputs stay right, but a repaired frame costs >= 0.1 s.  Every
launcher's status words are registered here; `persistent_poll` reads their repair counters WITHOUT synchronising (async copy into
pinned memory, evaluated on the next poll) and retires the persistent path on a device that had to repair -- sessions then
re-capture their frame graphs on the launch-per-op chain (`persistent_epoch` changes).  Callers go through `ops.`, which re-exports this."""
import os
import warnings
import weakref
from collections import defaultdict
from types import SimpleNamespace
from typing import Optional

import torch

PERSISTENT_MAX_REPAIRS = 0          # repairs tolerated per device before the launch-per-op chain takes over


class _Health:
    """What the registry knows about one device."""
    def __init__(self):
        self.status = []          # weakrefs of the registered status tensors (int32 [4])
        self.retired = None       # reason string once the persistent path is retired
        self.epoch = 0            # bumped when the persistent path is retired or given back
        self.pending = None       # (event, [pinned int32 [4] copies]) requested by the last poll
        self.seen = 0             # repairs counted by the last completed read


_health = defaultdict(_Health)      # torch.device -> _Health


def _clears(field: str) -> SimpleNamespace:
    def clear() -> None:
        for h in _health.values():
            setattr(h, field, None)
    return SimpleNamespace(clear=clear)


# The registry's former dicts, as far as callers written against them reset it: the fixtures of the GPU tests of earlier revisions, which
# must keep passing on this library, clear the first two and zero the tensors behind the third.  New code uses `persistent_rearm`.
_persist_off, _persist_pending = _clears("retired"), _clears("pending")
_persist_status = SimpleNamespace(values=lambda: [h.status for h in _health.values()])


def new_persistent_status(device) -> torch.Tensor:
    """The 4 status words of a persistent launcher (time-out codes in flight | frames repaired | OR of repaired codes | reserved),
    registered for `persistent_poll`."""
    device = torch.device(device)
    st = torch.zeros(4, device=device, dtype=torch.int32)
    _health[device].status.append(weakref.ref(st))
    return st


def persistent_epoch(device) -> int:
    return _health[torch.device(device)].epoch


def persistent_retired(device) -> Optional[str]:
    """Why `persistent_poll` retired the persistent launches of `device`, None while it has them."""
    return _health[torch.device(device)].retired


def persistent_repairs(device, synchronize: bool = True) -> int:
    """Frames / codec steps of `device` that the repair launches had to recompute so far.  ``synchronize=True`` reads the device words
    now (a device-to-host copy: waits for the stream); ``False`` returns the count seen by the last completed `persistent_poll` copy
    without touching the device (0 before the first one)."""
    h = _health[torch.device(device)]
    if not synchronize:
        if h.pending is not None and h.pending[0].query():
            h.seen = int(sum(int(c[1]) for c in h.pending[1]))
        return h.seen
    h.seen = int(sum(int(t[1].item()) for t in (r() for r in h.status) if t is not None))
    return h.seen


def persistent_rearm(device) -> None:
    """Gives `device` its persistent frame launches back after `persistent_poll` retired them (e.g. the process that shared the GPU
    has gone): clears the repair counters, bumps the epoch so that sessions re-capture their graphs.  The in-stream repair launch
    keeps every frame correct either way; this is about speed only.

    Call it with NO frame in flight on `device`: the status words are shared with captured graphs and per-session streams, and a
    repair launch's atomics racing with the reset would lose or mis-count a repair.  The whole device is therefore drained first
    (every stream, not only the current one), and the counters are zeroed on a quiet device."""
    device = torch.device(device)
    h = _health[device]
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    for r in h.status:
        t = r()
        if t is not None:
            t.zero_()
    h.pending, h.seen = None, 0
    if h.retired is not None:
        h.retired = None
        h.epoch += 1


def _judge(device, h: _Health, n: int) -> bool:
    """Retires the persistent path of `device` when `n` repairs are more than it tolerates; whether it did."""
    if n <= PERSISTENT_MAX_REPAIRS:
        return False
    if h.retired is None:
        h.retired = f"{n} frame(s) needed the one-workgroup repair launch (hand-offs timed out: not all workgroups were resident)"
        h.epoch += 1
        warnings.warn(f"rstnet_amd: persistent frame launches retired on {device}: {h.retired}; the launch-per-op chain takes over "
                      "(outputs were repaired in-stream, nothing wrong left the device)", RuntimeWarning)
    return True


def persistent_poll(device, synchronize: bool = False) -> None:
    """Looks at the repair counters of `device` (the copy requested by the PREVIOUS call unless `synchronize`), retires the persistent
    path beyond PERSISTENT_MAX_REPAIRS repairs and requests the next copy.  Cheap enough for once every few dozen frames; never
    called inside a graph capture."""
    device = torch.device(device)
    h = _health[device]
    if device.type != "cuda" or h.retired is not None or torch.cuda.is_current_stream_capturing():
        return
    if synchronize:
        _judge(device, h, persistent_repairs(device))
        return
    if h.pending is not None:
        if not h.pending[0].query():
            return
        n, h.pending = persistent_repairs(device, synchronize=False), None
        if _judge(device, h, n):
            return
    alive = [t for t in (r() for r in h.status) if t is not None]
    h.status = [r for r in h.status if r() is not None]
    if not alive:
        return
    with torch.cuda.device(device):
        copies = [torch.empty(4, dtype=torch.int32).pin_memory() for _ in alive]
        for c, t in zip(copies, alive):
            c.copy_(t, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
    h.pending = (ev, copies)


def depth_frame_enabled(device=None) -> bool:
    """RST_DEPTH_FRAME=0 keeps the launch-per-op depth phase / codec transformer layers (A/B measurements, or a device known to be
    shared with other work); a device whose persistent launches needed repairs is retired automatically (`persistent_poll`)."""
    if os.environ.get("RST_DEPTH_FRAME", "1") in ("0", ""):
        return False
    return device is None or persistent_retired(device) is None
