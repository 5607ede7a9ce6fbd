"""``_PackedCache``: the one way a module keeps a kernel-side form of its parameters (repacked, stacked, cast, pointer tables)."""
from __future__ import annotations

from typing import Any, Optional, Tuple

import torch


class _PackedCache:
    """Device-side repacked weights, rebuilt when the parameters they derive from change."""

    def __init__(self) -> None:
        self._key: Optional[Tuple] = None
        self._val: Any = None

    def get(self, params, build):
        key = tuple((p.data_ptr(), p._version, p.device) if p is not None else None for p in params)
        if key != self._key:
            with torch.no_grad():
                self._val = build()
            self._key = key
        return self._val

    def clear(self) -> None:
        self._key, self._val = None, None
