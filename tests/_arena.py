"""A guard-band arena for memory-contract tests (tests/test_gpu_memory_contract.py; held on the CPU by tests/test_arena_cpu.py).

One allocation per case holds every pointer argument of a call.  The allocation is filled from the host with a word pattern that
depends on the position (word i = 0x9E3779B9 (i + 1) mod 2^32: no legitimate output reproduces it by chance) or with all-ones
words (a read one word past a row then meets the worst carry input, not the zeros of fresh memory).  place() puts an operand
between two guards of max(4096 bytes, 4 rows of that operand) at one of two alignment classes:

  aligned   the address is a multiple of 256;
  natural   the address is a multiple of the element size and of nothing coarser below 16 bytes: = 4 (mod 16) for 4-byte
            elements, = 8 (mod 16) for 8-byte elements, = 1 (mod 16) — an odd address — for bytes.

check(expected) reads the whole allocation back once and compares it with the host shadow in which only the regions named in
`expected` are replaced by the expected values: one comparison for "the outputs are right", "the guards are intact" and "the
inputs are unchanged".  A mismatch reports the first differing word, its offset and the region or guard it lies in.

The memory behind the arena is a backend: DeviceBackend goes through the C ABI's own allocator and copies (pai_malloc,
pai_memcpy_h2d / _d2h); HostBackend is a numpy buffer standing in for the device, for the CPU test of this file's own logic."""
from __future__ import annotations

import ctypes as C

import numpy as np

GOLDEN = 0x9E3779B9
GUARD_MIN = 4096
ALIGNED = "aligned"
NATURAL = "natural"
ALIGNS = (ALIGNED, NATURAL)
FILLERS = ("pattern", "ones")


def filler_words(kind: str, nwords: int) -> np.ndarray:
    if kind == "ones":
        return np.full(nwords, 0xFFFFFFFF, dtype=np.uint32)
    assert kind == "pattern"
    return ((np.arange(1, nwords + 1, dtype=np.uint64) * GOLDEN) & 0xFFFFFFFF).astype(np.uint32)


def natural_residue(itemsize: int) -> int:
    """the address modulo 16 of the `natural` class for an element of `itemsize` bytes"""
    return {1: 1, 4: 4, 8: 8}[itemsize]


class HostBackend:
    """a numpy buffer standing in for the device; `base` is the address the arena believes it has (a multiple of 256)"""

    def __init__(self, base: int = 0x7F0000010000):
        self.base, self.buf = base, None

    def alloc(self, nbytes: int) -> int:
        self.buf = np.zeros(nbytes, dtype=np.uint8)
        return self.base

    def write(self, data: np.ndarray) -> None:
        self.buf[:] = data

    def read(self) -> np.ndarray:
        return self.buf.copy()

    def free(self) -> None:
        self.buf = None


class DeviceBackend:
    def __init__(self, device: int = 0):
        from pailliercryptolib_python_amd import _native

        self.native, self.lib, self.device, self.ptr, self.nbytes = _native, _native.load(), device, None, 0

    def alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self.native.check(self.lib.pai_malloc(self.device, nbytes, C.byref(p)))
        self.ptr, self.nbytes = p, nbytes
        return p.value

    def write(self, data: np.ndarray) -> None:
        self.native.check(self.lib.pai_memcpy_h2d(self.device, self.ptr, data.ctypes.data_as(C.c_void_p), self.nbytes, None))

    def read(self) -> np.ndarray:
        out = np.empty(self.nbytes, dtype=np.uint8)
        self.native.check(self.lib.pai_memcpy_d2h(self.device, out.ctypes.data_as(C.c_void_p), self.ptr, self.nbytes, None))
        return out

    def free(self) -> None:
        if self.ptr:
            self.lib.pai_free(self.device, self.ptr)
            self.ptr = None


class Region:
    def __init__(self, arena, name, offset, shape, dtype, guard, host):
        self.arena, self.name, self.offset, self.shape, self.dtype, self.guard, self.host = arena, name, offset, shape, dtype, guard, host
        self.nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        self.row_bytes = (shape[-1] if len(shape) > 1 else 1) * dtype.itemsize

    @property
    def address(self) -> int:
        assert self.arena.base is not None, "commit() the arena before taking a pointer"
        return self.arena.base + self.offset

    @property
    def ptr(self) -> C.c_void_p:
        return C.c_void_p(self.address)

    def at(self, row: int) -> C.c_void_p:
        """the pointer to row `row` of the region"""
        assert 0 <= row * self.row_bytes < max(self.nbytes, 1)
        return C.c_void_p(self.address + row * self.row_bytes)


class Arena:
    def __init__(self, filler: str = "pattern", backend=None):
        self.filler = filler
        self.backend = backend if backend is not None else DeviceBackend()
        self.regions: list[Region] = []
        self.cursor = 0
        self.base = None
        self.shadow = None

    def place(self, name, host=None, shape=None, dtype=np.uint32, align=ALIGNED, row_bytes=None) -> Region:
        """Reserves a region for `host` (an array: its contents are uploaded) or for `shape` x `dtype` (it keeps the filler) and
        returns it; pointers exist after commit()."""
        assert self.base is None, "place() after commit()"
        assert all(r.name != name for r in self.regions), name
        if host is not None:
            host = np.ascontiguousarray(host)
            shape, dtype = host.shape, host.dtype
        shape, dtype = tuple(int(s) for s in (shape if hasattr(shape, "__len__") else (shape,))), np.dtype(dtype)
        item = dtype.itemsize
        rb = row_bytes if row_bytes is not None else (shape[-1] if len(shape) > 1 else 1) * item
        guard = max(GUARD_MIN, 4 * rb)
        start = self.cursor + guard
        start = (start + 255) // 256 * 256
        if align == NATURAL:
            start += natural_residue(item)
        else:
            assert align == ALIGNED, align
        r = Region(self, name, start, shape, dtype, guard, host)
        self.cursor = start + r.nbytes + guard
        self.regions.append(r)
        return r

    def commit(self) -> None:
        total = (self.cursor + 255) // 256 * 256 + 256
        self.base = self.backend.alloc(total)
        assert self.base % 256 == 0, "the allocator's base is expected to be 256-byte aligned"
        self.shadow = filler_words(self.filler, total // 4).view(np.uint8).copy()
        for r in self.regions:
            if r.host is not None and r.nbytes:
                self.shadow[r.offset:r.offset + r.nbytes] = r.host.reshape(-1).view(np.uint8)
        self.backend.write(self.shadow)

    def where(self, off: int) -> str:
        """the name of the region or guard byte offset `off` lies in"""
        for r in self.regions:
            if r.offset <= off < r.offset + r.nbytes:
                return f"region '{r.name}'"
        best = None
        for r in self.regions:
            if r.offset - r.guard <= off < r.offset:
                d, nm = r.offset - off, f"guard before '{r.name}'"
            elif r.offset + r.nbytes <= off < r.offset + r.nbytes + r.guard:
                d, nm = off - (r.offset + r.nbytes) + 1, f"guard after '{r.name}'"
            else:
                continue
            if best is None or d < best[0]:
                best = (d, nm)
        return best[1] if best else "padding between guards"

    def check(self, expected: dict) -> None:
        """`expected`: region name -> array of the region's shape and element size (the outputs the call documents).  Raises
        AssertionError naming the first byte that differs from the shadow."""
        want = self.shadow.copy()
        for name, val in expected.items():
            r = next(x for x in self.regions if x.name == name)
            v = np.ascontiguousarray(val)
            assert v.dtype.itemsize == r.dtype.itemsize and v.size * v.dtype.itemsize == r.nbytes, (name, v.shape, v.dtype, r.shape, r.dtype)
            want[r.offset:r.offset + r.nbytes] = v.reshape(-1).view(np.uint8)
        got = self.backend.read()
        bad = np.flatnonzero(got != want)
        if bad.size == 0:
            return
        off = int(bad[0])
        w = off // 4 * 4
        gw, ww = (int(x[w:w + 4].view(np.uint32)[0]) for x in (got, want))
        where = self.where(off)
        rel = ""
        for r in self.regions:
            if where == f"region '{r.name}'":
                i = off - r.offset
                rel = f" (row {i // r.row_bytes}, byte {i % r.row_bytes} of the row)"
        raise AssertionError(f"arena[{self.filler}]: word at byte offset {w} is 0x{gw:08x}, expected 0x{ww:08x}, in {where}{rel}; "
                             f"{bad.size} bytes differ, the last at offset {int(bad[-1])} in {self.where(int(bad[-1]))}")

    def free(self) -> None:
        self.backend.free()
