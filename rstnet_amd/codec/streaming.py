"""Streaming-state protocol of the codec / LM modules.

Same surface as the reference's ``StreamingModule`` family (``modules/streaming.py:33-194`` of the
MimiCodec tokenizer copy): ``streaming(batch_size)`` context manager, ``streaming_forever``,
``reset_streaming``, ``get_streaming_state`` / ``set_streaming_state``, ``set_streaming_propagate`` and the
``is_streaming`` flag.  States are small dataclasses whose tensors live on the module's device and are handed
to the stateless C ABI as plain pointers.
"""
from __future__ import annotations

import abc
from contextlib import contextmanager
from dataclasses import dataclass
from typing import Any, Callable, Dict, Generic, List, Optional, Sequence, TypeVar

import torch
from torch import nn

State = TypeVar("State")


def check_rows(rows: Sequence[int], batch_size: int) -> List[int]:
    """The streams of a ``reset_streams(rows)`` call as a sorted list of distinct ints; ``ValueError`` for a row outside the batch."""
    out = sorted({int(r) for r in rows})
    bad = [r for r in out if not 0 <= r < batch_size]
    if bad:
        raise ValueError(f"reset_streams: rows {bad} are outside the batch of {batch_size} streams")
    return out


def reset_stream_rows(module: nn.Module, rows: Sequence[int]) -> None:
    """Streams ``rows`` of every live streaming state under ``module`` go back to what a new session holds (the state's ``reset_rows``:
    history rows zeroed or flagged for re-seeding, positions to 0), in place and eagerly: tensors keep their addresses, so a captured
    frame that points at them stays valid and sees the new rows on its next replay.  The other streams' bytes are not touched."""
    for m in module.modules():
        if isinstance(m, StreamingModule) and m._streaming_state is not None:
            fn = getattr(m._streaming_state, "reset_rows", None)
            if fn is not None:
                fn(rows)


class StreamingModule(abc.ABC, nn.Module, Generic[State]):
    def __init__(self) -> None:
        super().__init__()
        self._streaming_state: Optional[State] = None
        self._streaming_propagate: bool = True
        # the live session keeps one position / history seed per stream (``streaming(batch_size, per_stream=True)``): any row can then be
        # reset between two steps while the others go on (``reset_stream_rows``); read by ``_init_streaming_state``
        self._streaming_per_stream: bool = False

    @property
    def is_streaming(self) -> bool:
        return self._streaming_state is not None

    def set_streaming_propagate(self, streaming_propagate: bool) -> None:
        self._streaming_propagate = streaming_propagate

    def _apply_named_streaming(self, fn: Callable[[str, "StreamingModule"], None]) -> None:
        """Depth-first walk over this module and its streaming descendants.  A module whose
        ``_streaming_propagate`` is False is skipped together with its subtree -- except at the root, where only
        the root itself is skipped and its children are still visited (the reference relies on this for the depth
        transformer, ``modules/streaming.py:67-84``)."""
        def visit(prefix: str, module: nn.Module) -> None:
            if isinstance(module, StreamingModule):
                if not module._streaming_propagate:
                    return
                fn(prefix, module)
            for name, child in module.named_children():
                visit(f"{prefix}.{name}", child)

        if self._streaming_propagate:
            fn("", self)
        for name, child in self.named_children():
            visit(name, child)

    @abc.abstractmethod
    def _init_streaming_state(self, batch_size: int) -> State:
        ...

    def _start_streaming(self, batch_size: int, per_stream: bool = False) -> None:
        def start(_: str, m: "StreamingModule") -> None:
            m._streaming_per_stream = bool(per_stream)
            m._streaming_state = m._init_streaming_state(batch_size)
        try:
            self._apply_named_streaming(start)
        except Exception:
            self._stop_streaming()      # (a module that does not serve the session's mode refuses it: leave nothing half open)
            raise

    def _stop_streaming(self) -> None:
        def stop(_: str, m: "StreamingModule") -> None:
            m._streaming_state = None
            m._streaming_per_stream = False
        self._apply_named_streaming(stop)

    def streaming_forever(self, batch_size: int, per_stream: bool = False) -> None:
        self._start_streaming(batch_size, per_stream)

    @contextmanager
    def streaming(self, batch_size: int, per_stream: bool = False):
        """``per_stream``: every stateful module keeps one position per stream instead of one for the batch, so that single streams can
        be reset while the session runs (``MimiCodec.reset_streams``, ``LMGen.reset_streams``); off, nothing changes."""
        self._start_streaming(batch_size, per_stream)
        try:
            yield
        finally:
            self._stop_streaming()

    def reset_streaming(self) -> None:
        def reset(name: str, m: "StreamingModule") -> None:
            if m._streaming_state is None:
                raise ValueError(f"Trying to reset streaming, but {name} wasn't streaming.")
            m._streaming_state.reset()
        self._apply_named_streaming(reset)

    def get_streaming_state(self) -> Dict[str, Any]:
        out: Dict[str, Any] = {}

        def collect(name: str, m: "StreamingModule") -> None:
            out[name] = m._streaming_state
        self._apply_named_streaming(collect)
        return out

    def set_streaming_state(self, state: Dict[str, Any]) -> None:
        pending = dict(state)

        def assign(name: str, m: "StreamingModule") -> None:
            if name not in pending:
                raise RuntimeError(f"Expected to find a streaming state for {name}.")
            m._streaming_state = pending.pop(name)
        self._apply_named_streaming(assign)
        if pending:
            raise RuntimeError(f"Some states were not consumed: {list(pending.keys())}")


@dataclass
class _NullState:
    def reset(self) -> None:
        pass


class StreamingContainer(StreamingModule[_NullState]):
    def _init_streaming_state(self, batch_size: int) -> _NullState:
        return _NullState()


@dataclass
class _StreamingAddState:
    previous_x: Optional[torch.Tensor] = None
    previous_y: Optional[torch.Tensor] = None

    def reset(self) -> None:
        self.previous_x = None
        self.previous_y = None

    def reset_rows(self, rows) -> None:
        for t in (self.previous_x, self.previous_y):
            if t is not None and t.numel():
                raise RuntimeError("StreamingAdd holds back a surplus: its streams cannot be reset one by one")


class StreamingAdd(StreamingModule[_StreamingAddState]):
    """``x + y`` on ``[B, C, T]`` tensors; when streaming, holds back the surplus of the longer operand
    (``modules/streaming.py:162-194``).  Inside the SEANet residual blocks the addition is fused into the
    epilogue of the 1x1 convolution, where both operands always have the same length."""

    def _init_streaming_state(self, batch_size: int) -> _StreamingAddState:
        return _StreamingAddState()

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        state = self._streaming_state
        if state is None:
            return x + y
        if state.previous_x is not None:
            x = torch.cat([state.previous_x, x], dim=-1)
        if state.previous_y is not None:
            y = torch.cat([state.previous_y, y], dim=-1)
        n = min(x.shape[-1], y.shape[-1])
        state.previous_x, state.previous_y = x[..., n:], y[..., n:]
        return x[..., :n] + y[..., :n]
