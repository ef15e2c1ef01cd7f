"""Helpers of the stream-contract tests (include/paillier_hip.h, conventions block: asynchronous on `stream`, users of one
handle's scratch chained across streams, any mix of threads and streams safe).  DESIGN.md, "stream contract", has the method.

Streams are NON-BLOCKING ones (hipStreamCreateWithFlags, the kind torch hands out): the null stream does not wait for them and
they do not wait for it, so work the library queues on the wrong stream is not serialised into place by accident.

The blocker is a long, side-effect-free piece of stream work issued through the library itself: pai_modexp_var on a pai_modulus
handle of its own (its own ScratchOrder: no scratch shared with the handle under test), 4096-bit odd modulus, full-width
exponents.  Behind it, a late operand's true values are copied into place by pai_buf_slice on the same stream; until then the
operand buffer holds a VALID BUT DIFFERENT operand of the same shape (by default the true rows rotated by one), and outputs hold
a sentinel.  Whatever the library runs elsewhere than behind the blocker on that stream reads the filler or the sentinel, and the
bits differ — wrong bits, never an out-of-range access: only value operands arrive late, everything a kernel uses as an index,
offset, count or plan is resident from the start.

`Resident` and `Late` are the two placements a runner of tests/_fuzz_ext_run.py or a row of tests/_stream_cases.py is written
against.  Nothing here loads the library at import."""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np

HIP_STREAM_NON_BLOCKING = 1
HIP_SUCCESS = 0
HIP_ERROR_NOT_READY = 600
PAI_E_HIP = -3
MAX_STREAMS = 3                          # user streams per test: the machines run with 4 hardware queues
SENTINEL_BYTE = 0xA5
BLOCKER_BITS = 4096
BLOCKER_ROWS = 256                       # profiles/r24/stream_contract.json: the blocker's duration against the longest enqueue

_hip = None


def hip():
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipStreamQuery.argtypes = [C.c_void_p]
        _hip.hipStreamSynchronize.argtypes = [C.c_void_p]
        _hip.hipStreamDestroy.argtypes = [C.c_void_p]
    return _hip


_pool = []


@contextlib.contextmanager
def streams(count=1):
    """`count` non-blocking streams from a pool of at most MAX_STREAMS that lives as long as the process; drained on exit.

    They are not destroyed after a test: the key handles and the calling thread's staging ring are cached across tests and keep
    events that were last recorded on these streams, and include/paillier_hip.h (conventions) asks that such a stream stays alive
    while those events can still be waited for."""
    assert 1 <= count <= MAX_STREAMS
    while len(_pool) < count:
        s = C.c_void_p()
        if hip().hipStreamCreateWithFlags(C.byref(s), HIP_STREAM_NON_BLOCKING) != HIP_SUCCESS:
            stop("hipStreamCreateWithFlags failed")
        _pool.append(s)
    try:
        yield _pool[:count]
    finally:
        for s in _pool[:count]:
            sync(s)


def stop(what):
    """a HIP runtime error (a fault among them) ends the session: nothing more is started on a device that has reported one"""
    import pytest

    pytest.exit(f"{what}: nothing more is started on the GPU", returncode=3)


def check(rc):
    """_native.check, except that PAI_E_HIP ends the session"""
    from pailliercryptolib_python_amd import _native

    if rc == PAI_E_HIP:
        stop(f"PAI_E_HIP: {_native.load().pai_last_error().decode()}")
    _native.check(rc)


def running(stream):
    """work queued on `stream` has not completed"""
    rc = hip().hipStreamQuery(stream)
    if rc not in (HIP_SUCCESS, HIP_ERROR_NOT_READY):
        stop(f"hipStreamQuery returned {rc}")
    return rc == HIP_ERROR_NOT_READY


def sync(stream):
    rc = hip().hipStreamSynchronize(stream)
    if rc != HIP_SUCCESS:
        stop(f"hipStreamSynchronize returned {rc}")


def device_sync():
    rc = hip().hipDeviceSynchronize()
    if rc != HIP_SUCCESS:
        stop(f"hipDeviceSynchronize returned {rc}")


def sentinel(shape, dtype=np.uint32):
    dtype = np.dtype(dtype)
    return np.frombuffer(bytes([SENTINEL_BYTE]) * (int(np.prod(shape)) * dtype.itemsize), dtype=dtype).reshape(shape).copy()


class Blocker:
    """blocker(stream) enqueues `rows` full-width exponentiations modulo a 4096-bit odd number and returns"""

    def __init__(self, rows=BLOCKER_ROWS, seed=4096):
        import random

        from pailliercryptolib_python_amd import _native
        from tests._util import DevArray, host_ptr, ints_to_limbs

        self.lib, self.rows, self.words = _native.load(), rows, BLOCKER_BITS // 32
        rng = random.Random(seed)
        self.M = rng.getrandbits(BLOCKER_BITS) | (1 << (BLOCKER_BITS - 1)) | 1
        self.base = [rng.randrange(2, self.M) for _ in range(rows)]
        self.expo = [rng.getrandbits(BLOCKER_BITS) | (1 << (BLOCKER_BITS - 1)) for _ in range(rows)]
        self.handle = C.c_void_p()
        check(self.lib.pai_modulus_create(host_ptr(ints_to_limbs([self.M], self.words)), self.words, 0, C.byref(self.handle)))
        self.d_base, self.d_expo = DevArray(ints_to_limbs(self.base, self.words)), DevArray(ints_to_limbs(self.expo, self.words))
        self.d_out = DevArray(shape=(rows, self.words))
        self._check = check

    def __call__(self, stream):
        self._check(self.lib.pai_modexp_var(self.handle, self.d_base.ptr, 0, self.d_expo.ptr, self.words, BLOCKER_BITS, 0, self.rows,
                                            self.d_out.ptr, stream))

    def check(self):
        """its output against CPython's pow (bulk through the C oracle, which tests/_util.pow_many spot-checks against pow)"""
        from tests._util import limbs_to_ints, pow_many

        with streams(1) as (s,):
            self(s)
            got = np.empty((self.rows, self.words), dtype=np.uint32)
            self._check(self.lib.pai_memcpy_d2h(0, got.ctypes.data_as(C.c_void_p), self.d_out.ptr, got.nbytes, s))
        assert limbs_to_ints(got) == pow_many(self.base, self.expo, self.M), "the blocker's own result is wrong"

    def close(self):
        if self.handle:
            device_sync()
            self.lib.pai_modulus_destroy(self.handle)
            self.handle = None


class Resident:
    """every operand uploaded before the call, every call on the null stream: what the suite did before.  Outputs are filled with
    the sentinel before every call (issue), so that a call which writes nothing cannot pass on what an earlier one left there"""
    stream = None

    def __init__(self):
        self.outs = []

    def value(self, host, filler=None):
        from tests._util import DevArray

        return DevArray(np.ascontiguousarray(host))

    resident = value

    def out(self, shape, dtype=np.uint32):
        from tests._util import DevArray

        host = sentinel(shape, dtype)
        d = DevArray(host)
        self.outs.append((d, host))
        return d

    def issue(self):
        from pailliercryptolib_python_amd import _native

        for d, host in self.outs:
            if host.nbytes:
                check(_native.load().pai_memcpy_h2d(0, d.ptr, host.ctypes.data_as(C.c_void_p), host.nbytes, None))

    def issued(self, syncs=False):
        pass

    def read(self, d):
        return d.get()


class Late:
    """Operands whose true values exist only behind a blocker on one non-blocking stream.

    value(host)    a late operand: the buffer holds `filler` (default: the rows rotated by one; it must differ from `host`) until
                   issue() queues the copy of the true values behind the blocker
    resident(host) an operand that is in place from the start (indices, offsets, counts, plans, caller-zeroed flag words)
    out(shape)     an output, filled with the sentinel
    issue()        drains the stream, puts fillers, sentinels and resident words back, then queues blocker + copies and asserts
                   that the stream is running: call it right before the entry point
    issued(syncs)  right after the entry point returned: unless the call is one that synchronises, the stream must still be running —
                   the call returned while its inputs did not exist yet
    read(d)        the buffer read back on the stream (pai_memcpy_d2h synchronises that stream only); an output must not hold a
                   sentinel row any more"""

    def __init__(self, stream, blocker, delayed=True):
        from pailliercryptolib_python_amd import _native

        self.stream, self.blocker, self.delayed = stream, blocker, delayed      # not delayed: every operand resident, the calls on `stream`
        self.lib, self._check = _native.load(), check
        self.lates, self.outs, self.fixed = [], [], []
        self.issues = 0

    def value(self, host, filler=None):
        from tests._util import DevArray

        host = np.ascontiguousarray(host)
        if not self.delayed:
            return self.resident(host)
        if filler is None:
            filler = np.roll(host, 1, axis=0)
        filler = np.ascontiguousarray(filler, dtype=host.dtype)
        assert filler.shape == host.shape
        if np.array_equal(filler, host) or host.nbytes % 4:
            return self.resident(host)               # one row, or equal rows: no other valid operand to stand in (the caller counts `lates`)
        op, staging = DevArray(filler), DevArray(host)
        self.lates.append((op, staging, filler))
        return op

    def resident(self, host):
        from tests._util import DevArray

        host = np.ascontiguousarray(host)
        d = DevArray(host)
        self.fixed.append((d, host.copy()))
        return d

    def out(self, shape, dtype=np.uint32):
        from tests._util import DevArray

        host = sentinel(shape, dtype)
        d = DevArray(host)
        self.outs.append((d, host))
        return d

    def _h2d(self, d, host):
        if host.nbytes:
            self._check(self.lib.pai_memcpy_h2d(0, d.ptr, host.ctypes.data_as(C.c_void_p), host.nbytes, None))

    def restore(self):
        sync(self.stream)
        for op, _, filler in self.lates:
            self._h2d(op, filler)
        for d, host in self.outs + self.fixed:
            self._h2d(d, host)
        device_sync()

    def arrive(self):
        for op, staging, filler in self.lates:
            self._check(self.lib.pai_buf_slice(0, staging.ptr, filler.nbytes // 4, 0, 1, 1, op.ptr, self.stream))

    def issue(self):
        self.restore()
        self.blocker(self.stream)
        self.arrive()
        assert running(self.stream), "the blocker ended before the call was issued (blocker too short)"
        self.issues += 1

    def issued(self, syncs=False):
        if not syncs:
            assert running(self.stream), "blocker too short / call synchronised: the stream was idle when the call returned"

    def read(self, d):
        got = np.empty(d.shape, dtype=d.dtype)
        if d.nbytes:
            self._check(self.lib.pai_memcpy_d2h(0, got.ctypes.data_as(C.c_void_p), d.ptr, d.nbytes, self.stream))
        else:
            sync(self.stream)
        for o, host in self.outs:
            if o is d and d.nbytes:
                rows = got.reshape(got.shape[0], -1).view(np.uint8)
                assert not (rows == SENTINEL_BYTE).all(axis=1).any(), "an output row still holds the sentinel"
        return got
