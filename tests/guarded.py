"""Guarded buffers for the buffer-contract tests (include/vfmreg.h: "the caller owns every buffer").

A ``GuardedBuffer`` is one uint8 tensor laid out as ``[guard G | body | guard G]``.  ``.t`` is a typed, shaped view of the body that
can be handed to the ``vfmreg.ops`` wrappers or passed as ``.t.data_ptr()`` to the C ABI.  Both guards hold a seeded random byte
pattern; ``intact()`` tells whether they still do and ``damage()`` names the first byte that differs, by its offset from the body's
edge.  A write one padded tile past the end of a buffer lands in a guard -- mapped memory that belongs to the test -- instead of in
whatever the caching allocator put next to it, where it would go unnoticed.

The guards can also be POISONED (``poison_guards``): filled with a value that a kernel which reads past the end of an input would
turn into a different answer (NaN for floating-point data, a valid index for index arrays).  Poison values never become far
addresses.  G is a multiple of 512 bytes, so the body keeps the alignment of a normal allocation, and it defaults to 2 MiB -- more
than any one-tile overrun (128 rows x 768 fp32 = 384 KiB).
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch

GUARD_BYTES = 2 << 20
GUARD_ALIGN = 512


_PATTERNS = {}


def _pattern(guard: int, seed: int, device: torch.device) -> torch.Tensor:
    """The seeded random bytes of both guards (2 x guard), made once per (guard, seed, device) and never written."""
    key = (guard, seed, str(device))
    if key not in _PATTERNS:
        g = torch.Generator().manual_seed(seed)
        _PATTERNS[key] = torch.randint(0, 256, (2 * guard,), dtype=torch.uint8, generator=g).to(device)
    return _PATTERNS[key]


class GuardCheck:
    """Result of ``GuardedBuffer.intact()``: truthy when intact; ``str()`` says where a guard was written."""

    def __init__(self, damage: Optional[str]):
        self.damage = damage

    def __bool__(self) -> bool:
        return self.damage is None

    def __repr__(self) -> str:
        return "intact" if self.damage is None else self.damage


class GuardedBuffer:
    def __init__(self, shape: Sequence[int] | int, dtype: torch.dtype, device="cuda", guard: int = GUARD_BYTES, seed: int = 0,
                 pin_memory: bool = False):
        if guard <= 0 or guard % GUARD_ALIGN:
            raise ValueError(f"guard must be a positive multiple of {GUARD_ALIGN} bytes")
        self.shape = (int(shape),) if isinstance(shape, (int, np.integer)) else tuple(int(s) for s in shape)
        self.dtype = dtype
        self.itemsize = torch.empty((), dtype=dtype).element_size()
        self.nbytes = math.prod(self.shape) * self.itemsize
        self.guard = int(guard)
        self.device = torch.device(device)
        self.raw = torch.empty(2 * self.guard + self.nbytes, dtype=torch.uint8, device=self.device,
                               pin_memory=pin_memory and self.device.type == "cpu")
        self._pattern = _pattern(self.guard, int(seed), self.device)
        self.restore_guards()
        self.body = self.raw[self.guard:self.guard + self.nbytes]
        self.t = self.body.view(dtype).view(self.shape)

    # ------------------------------------------------------------------------------------------------------------ guards
    @property
    def front(self) -> torch.Tensor:
        return self.raw[:self.guard]

    @property
    def back(self) -> torch.Tensor:
        return self.raw[self.guard + self.nbytes:]

    def restore_guards(self) -> None:
        """Both guards back to the seeded random pattern."""
        self._expect = self._pattern
        self.raw[:self.guard] = self._pattern[:self.guard]
        self.raw[self.raw.numel() - self.guard:] = self._pattern[self.guard:]

    def poison_guards(self, kind: str) -> None:
        """Fill both guards with poison: ``"nan"`` (a quiet NaN of the body's floating-point type), ``"zero"`` (bytes 0x00: the
        value 0, a valid index), ``"ff"`` (bytes 0xFF).  ``intact()`` then checks for the poison."""
        if kind == "nan":
            if not self.dtype.is_floating_point:
                raise ValueError("NaN poison needs a floating-point body")
            val = torch.full((self.guard // self.itemsize,), float("nan"), dtype=self.dtype, device=self.device).view(torch.uint8)
        elif kind in ("zero", "ff"):
            val = torch.full((self.guard,), 0 if kind == "zero" else 0xFF, dtype=torch.uint8, device=self.device)
        else:
            raise ValueError(f"unknown poison {kind!r}")
        self._expect = torch.cat([val, val])
        self.raw[:self.guard] = val
        self.raw[self.raw.numel() - self.guard:] = val

    def damage(self) -> Optional[str]:
        """None if both guards hold what they were given; otherwise where the first differing byte of each damaged guard is,
        as an offset from the body's edge (-1 = the byte just before the body, +0 = the byte just after it)."""
        msgs = []
        exp = self._expect
        f = torch.nonzero(self.front != exp[:self.guard])
        if f.numel():
            i = int(f[-1])   # the byte nearest to the body: where an overrun from below starts
            msgs.append(f"front guard differs at offset {i - self.guard} (and {f.numel() - 1} more bytes)")
        b = torch.nonzero(self.back != exp[self.guard:])
        if b.numel():
            j = int(b[0])
            msgs.append(f"back guard differs at offset +{j} past the body (and {b.numel() - 1} more bytes)")
        return "; ".join(msgs) or None

    def intact(self) -> "GuardCheck":
        """Truthy iff both guards are intact; otherwise falsy, and its text names the first differing byte (``damage()``)."""
        return GuardCheck(self.damage())

    # ------------------------------------------------------------------------------------------------------------ body
    def fill_bytes(self, value: int) -> "GuardedBuffer":
        """Every body byte = value: 0x00 (0 / 0.0) or 0xFF (-1 for integers, a NaN for floating-point types)."""
        self.body.fill_(int(value))
        return self

    def fill_nan(self) -> "GuardedBuffer":
        self.t.fill_(float("nan"))
        return self

    def set(self, data) -> "GuardedBuffer":
        src = torch.as_tensor(np.ascontiguousarray(data)) if not isinstance(data, torch.Tensor) else data
        self.t.copy_(src.reshape(self.shape).to(self.dtype))
        return self

    def body_bytes(self) -> np.ndarray:
        return self.body.cpu().numpy().copy()

    def numpy(self) -> np.ndarray:
        return self.t.cpu().numpy().copy()

    def ptr(self) -> int:
        return self.t.data_ptr()
