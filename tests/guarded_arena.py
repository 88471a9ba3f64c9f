"""A guarded arena for memory-contract tests: one ``torch.uint8`` tensor out
of which named regions are carved at a requested alignment (and offset from
it), every region with at least 64 KiB of ``0xA5`` in front of it and behind
it.  64 KiB is twice the largest single-workgroup output in the library (1024
nodes of 32 B), so a pass that writes a workgroup's worth past its slot lands
in memory the test owns, and ``check_guards`` names where.

A plain module (imported by tests/test_gpu_ws_contract.py and by the CPU
self-test tests/test_guarded_arena.py); it works on any torch device.
"""
from __future__ import annotations

import torch

GUARD = 64 * 1024
FILL = 0xA5


def _up(x: int, a: int) -> int:
    return -(-x // a) * a


class GuardedArena:
    """``GuardedArena(device, [(name, nbytes, align, shift), ...])`` lays the
    regions out in order; ``region(name, nbytes, align, shift)`` carves one more
    out of what ``capacity`` left.  Everything outside the regions is guard."""

    def __init__(self, device, regions=(), capacity: int = 0):
        need = GUARD + capacity
        for _name, nbytes, align, shift in regions:
            need += GUARD + align + shift + nbytes
        self.buf = torch.full((need,), FILL, dtype=torch.uint8, device=device)
        self.base = self.buf.data_ptr()
        self._cursor = 0                # everything below is regions and their guards
        self._regions = {}              # name -> (front_lo, lo, hi, back_hi)
        self._snaps = {}
        for name, nbytes, align, shift in regions:
            self.region(name, nbytes, align, shift)

    def region(self, name: str, nbytes: int, align: int = 256, shift: int = 0) -> torch.Tensor:
        """A view of ``nbytes`` bytes whose address is ``shift`` past a multiple of ``align``."""
        if name in self._regions:
            raise ValueError(f"region {name!r} exists")
        if align <= 0 or not 0 <= shift:
            raise ValueError("align > 0 and shift >= 0")
        lo = _up(self.base + self._cursor + GUARD, align) + shift - self.base
        hi = lo + nbytes
        if hi + GUARD > self.buf.numel():
            raise ValueError(f"arena exhausted by region {name!r}: {hi + GUARD} > {self.buf.numel()}")
        self._regions[name] = (self._cursor, lo, hi, hi + GUARD)
        self._cursor = hi  # the guard behind this region is (part of) the one in front of the next
        assert (self.base + lo - shift) % align == 0
        return self.buf[lo:hi]

    def view(self, name: str) -> torch.Tensor:
        _f, lo, hi, _b = self._regions[name]
        return self.buf[lo:hi]

    def ptr(self, name: str) -> int:
        return self.base + self._regions[name][1]

    def poison(self, name: str, byte: int) -> None:
        self.view(name).fill_(byte)

    def assert_poison(self, name: str, byte: int, lo: int = 0, hi: int = None, what: str = "") -> None:
        """Bytes [lo, hi) of a region still hold the poison ``byte``."""
        v = self.view(name)[lo:hi]
        bad = v != byte
        if bool(bad.any()):
            idx = torch.nonzero(bad).flatten()
            first, last = int(idx[0]), int(idx[-1])
            raise AssertionError(f"{what}region {name!r}: poison 0x{byte:02X} overwritten at offset {lo + first}, "
                                 f"{last - first + 1} bytes to the last damaged one ({int(idx.numel())} differ)")

    def check_guards(self, what: str = "") -> None:
        """Every guard byte is intact; else the region, the side, the first
        damaged offset (counted away from the region) and the damaged length."""
        for name, (flo, lo, hi, bhi) in self._regions.items():
            for side, a, b in (("front", flo, lo), ("back", hi, bhi)):
                bad = self.buf[a:b] != FILL
                if not bool(bad.any()):
                    continue
                idx = torch.nonzero(bad).flatten()
                first, last = int(idx[0]), int(idx[-1])
                # front: bytes before the region's start; back: bytes past its end
                dist = (lo - a - 1 - last) if side == "front" else first
                raise AssertionError(
                    f"{what}guard damaged: region {name!r}, {side} guard, first damaged byte {dist} bytes "
                    f"{'before the start' if side == 'front' else 'past the end'} of the region, damaged length "
                    f"{last - first + 1} ({int(idx.numel())} bytes differ from 0x{FILL:02X})")

    def snapshot(self, name: str) -> None:
        self._snaps[name] = self.view(name).clone()

    def assert_unchanged(self, name: str, what: str = "") -> None:
        if not torch.equal(self.view(name), self._snaps[name]):
            idx = torch.nonzero(self.view(name) != self._snaps[name]).flatten()
            raise AssertionError(f"{what}region {name!r} changed: first at offset {int(idx[0])}, "
                                 f"{int(idx.numel())} bytes differ from the snapshot")
