"""The one staging buffer of a `build`: named sections of host tables laid out back to back, uploaded in one transfer."""
from __future__ import annotations

import ctypes
from typing import Dict, Tuple

import numpy as np
import torch


class Staging:
    """`add` lays contiguous arrays out at aligned offsets and `write` copies them into a byte buffer: the host side, which needs no
    GPU.  `upload` makes the one pinned buffer and its one non-blocking transfer; `ptr` and `view` then address the device copy."""
    MIN_BYTES = 16                  # an empty layout still uploads a buffer

    def __init__(self):
        self.sections: Dict[str, Tuple[int, np.ndarray]] = {}          # name -> (byte offset, contiguous array)
        self._end = 0

    def add(self, name: str, array: np.ndarray, align: int = 16) -> None:
        a = np.ascontiguousarray(array)
        offset = -(-self._end // align) * align
        self.sections[name] = (offset, a)
        self._end = offset + a.nbytes

    @property
    def nbytes(self) -> int:
        return max(self._end, self.MIN_BYTES)

    def write(self, out: np.ndarray) -> None:
        """Every section's bytes into `out`, a uint8 array of at least `nbytes`."""
        for offset, a in self.sections.values():
            out[offset:offset + a.nbytes] = a.reshape(-1).view(np.uint8)

    def upload(self, device: torch.device) -> None:
        self._pinned = torch.empty(self.nbytes, dtype=torch.uint8, pin_memory=True)     # (the source lives as long as its copy)
        self.write(self._pinned.numpy())
        self.device_bytes = self._pinned.to(device, non_blocking=True)

    def ptr(self, name: str, byte_offset: int = 0) -> ctypes.c_void_p:
        return ctypes.c_void_p(self.device_bytes.data_ptr() + self.sections[name][0] + byte_offset)

    def view(self, name: str, dtype: torch.dtype, shape) -> torch.Tensor:
        offset, a = self.sections[name]
        return self.device_bytes[offset:offset + a.nbytes].view(dtype).view(shape)
