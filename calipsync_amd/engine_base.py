"""What the ctypes engines over a packed-weight handle share (HubertEngine, PFLDEngine, S3FDEngine): the create / load
sequence, the grow-only workspace and the end of the handle.  ``unet.Model`` is an ``nn.Module`` with a lifecycle of its
own and stays outside."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib


class _PackedEngine:
    _destroy = ""        # the casync_*_destroy symbol of the subclass's handle

    _h = None
    _ws: Optional[torch.Tensor] = None

    def _create(self, device, create_name: str, *create_args) -> None:
        """casync_<...>_create*(device index, *create_args, &handle) on `device`."""
        self._lib = _lib.load()
        self.device = torch.device(device)
        h = C.c_void_p()
        _lib.check(getattr(self._lib, create_name)(self.device.index or 0, *create_args, C.byref(h)), create_name)
        self._h = h

    def _load_host(self, load_name: str, buf: np.ndarray) -> None:
        _lib.check(getattr(self._lib, load_name)(self._h, buf.ctypes.data, buf.size), load_name)

    def _open(self, device, create_name: str, create_args, load_name: str, buf: np.ndarray) -> None:
        self._create(device, create_name, *create_args)
        self._load_host(load_name, buf)

    def _grow_workspace(self, need_bytes: int) -> torch.Tensor:
        """The engine's own fp32 workspace tensor, reallocated only when a call needs more than it holds."""
        if self._ws is None or self._ws.numel() * 4 < need_bytes:
            self._ws = torch.empty((need_bytes + 3) // 4, dtype=torch.float32, device=self.device)
        return self._ws

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            getattr(self._lib, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
