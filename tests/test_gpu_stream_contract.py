"""GPU: every entry point with a `stream` argument, held to the stream contract of include/paillier_hip.h (conventions block):
asynchronous on that stream, users of one handle's scratch on different streams chained with an event, any mix of threads and
streams on one handle safe.  DESIGN.md, "stream contract", describes the method; tests/_streams.py has the helpers and
tests/_stream_cases.py the table (tests/test_stream_contract_cpu.py holds it to the header by name).

A. late inputs: behind a blocker on a NON-BLOCKING stream the true operands are copied into place by the stream itself; the call is
   issued while the stream is still running (asserted) and, unless it is one that synchronises, returns while it is still running
   (asserted): its inputs did not exist yet.  Outputs are read on that stream and compared bit for bit; no sentinel row survives.
   Anything the library queues on the null stream or on another stream reads the fillers or the sentinel.
B. chaining: X behind the blocker on s1, a second scratch user Y of the same handle on s2 with resident inputs; Y must not complete
   while X is still queued (stream queries, s2 then s1), both results exact; then with the roles swapped.
C. the staging rings wrap while their readers are still queued: 40 pai_ct_mul_host / pai_ct_add_aligned_host calls (32 slots), 8
   pai_modexp_fixed calls on two streams (4 slots, one device exponent buffer), two pai_threshold_combine calls with different theta.
D. three threads with a stream each on one public / private handle pair, 8 counted rounds of six calls.
E. the public API on a torch side stream, against the committed transcripts.

The kernel timers synchronise, so nothing here runs with the profile on; the routes are forced with the knobs the suite already uses
and are asserted where those knobs are tested (tests/test_gpu_path_edges.py, tests/test_gpu_fuzz_ext.py).

Measured on one MI355X (profiles/r24/stream_contract.json): see the README there for the blocker's duration, the longest enqueue
and the wall time of every test."""
import contextlib
import ctypes as C
import threading
import time

import numpy as np
import pytest

from pailliercryptolib_python_amd import _native
from tests import _fuzz_ext as fz
from tests import _fuzz_ext_run as fr
from tests import _stream_cases as sc
from tests._streams import Blocker, Late, check, device_sync, running, stop, streams, sync
from tests._util import disable, tune

pytestmark = pytest.mark.gpu

KNOB_VARS = ("PAI_LATENCY_MAX", "PAI_LAT_ADD_MAX", "PAI_TUNE", "PAI_DISABLE", "PAI_POW2_DIGIT_MIN")
POLL_LIMIT_S = 60.0                                   # a query loop that has not ended by then fails (it ends when the blocker does)


@pytest.fixture(scope="module")
def blocker():
    b = Blocker()
    b.check()
    yield b
    b.close()


@pytest.fixture(scope="module", autouse=True)
def handles_released():
    yield
    device_sync()
    sc.release_keyshares(fr._HANDLES.values())
    fr.release_handles()


def set_env(monkeypatch, env):
    for v in KNOB_VARS:
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def rows_of(h, row):
    """257 rows only where a 256-row tile exists: the digit engine's keys (wider keys: one ragged 64-row tile, and exponents of
    twice the length on the host's side of the comparison)"""
    return row.N if h.key.bits <= 2048 else sc.N_TILE


def warm(st, call):
    """once on the null stream at the same shape: lazy table builds and scratch growth synchronise the device and would drain the
    blocker (the operands are the fillers: valid ones)"""
    saved, st.stream = st.stream, None
    try:
        check(call())
        device_sync()
    finally:
        st.stream = saved


def compare(st, expected, what):
    for i, (d, want) in enumerate(expected):
        got = st.read(d)
        want = np.ascontiguousarray(want).astype(got.dtype, copy=False).reshape(got.shape)
        bad = np.nonzero((got != want).reshape(got.shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, f"{what}: output {i}: {bad.size} of {got.shape[0]} rows differ, first row {int(bad[0])}"


def with_knobs_of(monkeypatch):
    @contextlib.contextmanager
    def with_knobs(run):
        with monkeypatch.context() as mp:
            for name, value in run["tune"].items():
                tune(mp, name, value)
            for name in run["disable"]:
                disable(mp, name)
            yield
    return with_knobs


# ---- A. late inputs on a non-blocking stream ---------------------------------------------------------------------------------------------
def a_cases():
    seen, out = set(), []
    for row in sc.TABLE:
        if row.family:
            for bits in row.bits:
                if (row.family, bits) not in seen:
                    seen.add((row.family, bits))
                    out.append(pytest.param("family:" + row.family, "lat", bits, id=f"{row.family}-{bits}"))
            continue
        for variant in row.variants:
            for bits in row.bits:
                out.append(pytest.param(row.name, variant, bits, id=f"{row.name}-{variant}-{bits}"))
    return out


@pytest.mark.parametrize("name,variant,bits", a_cases())
def test_late_inputs(name, variant, bits, blocker, monkeypatch):
    h = fr.handle(bits)
    with streams(1) as (s,):
        st = Late(s, blocker)
        if name.startswith("family:"):
            family = name.split(":")[1]
            row = next(r for r in sc.TABLE if r.family == family)
            set_env(monkeypatch, sc.env_of(row, variant))
            lib = _native.load()
            check(lib.pai_profile_enable(1))                 # the warm-up is the ordinary runner: null stream, kernels asserted
            try:
                fr.run_round(family, fz.class_of(bits), fz.SEED, row.rnd, with_knobs_of(monkeypatch), set(), bits=bits)
            finally:
                check(lib.pai_profile_enable(0))
            device_sync()
            checks = fr.run_round(family, fz.class_of(bits), fz.SEED, row.rnd, with_knobs_of(monkeypatch), set(), stream=st, bits=bits)
            assert checks and st.issues and st.lates, (checks, st.issues, len(st.lates))
            return
        row = sc.BY_NAME[name]
        set_env(monkeypatch, sc.env_of(row, variant))
        call, expected = row.build(h, st, rows_of(h, row))
        warm(st, call)
        st.issue()
        check(call())
        st.issued(row.syncs)
        compare(st, expected, f"{name} [{variant}] at {bits} bits")


# ---- B. chaining across streams ----------------------------------------------------------------------------------------------------------
SK_CALLS = {"pai_decrypt", "pai_recover_r", "pai_encrypt_crt", "pai_obfuscate_crt"}
MODULUS_CALLS = {"pai_modexp_fixed", "pai_modexp_var"}
CRT_CALLS = {"pai_encrypt_crt", "pai_obfuscate_crt"}


def partner_of(name, key):
    """a second scratch user of the SAME handle: pai_ct_mul on the public handle (pai_ct_prod for pai_ct_mul itself), pai_decrypt on the
    private one (pai_recover_r for pai_decrypt itself), the other exponentiation on a pai_modulus.  The CRT calls own private-handle
    scratch only where they are served; elsewhere they ARE the public call (include/paillier_hip.h) and pair with pai_ct_mul"""
    if name in MODULUS_CALLS:
        return "pai_modexp_var" if name == "pai_modexp_fixed" else "pai_modexp_fixed"
    if name in CRT_CALLS and not fz.crt_served(key):
        return "pai_ct_mul"
    if name in SK_CALLS:
        return "pai_recover_r" if name == "pai_decrypt" else "pai_decrypt"
    return "pai_ct_prod" if name == "pai_ct_mul" else "pai_ct_mul"


def b_cases():
    """every chained (row, variant) on the 2048-bit key, and on one key of every further class where the dispatcher routes by class"""
    out = []
    for row in sc.TABLE:
        for variant in row.variants:
            if sc.chained_in(row, variant):
                for bits in sorted(row.bits, key=lambda b: (b != 2048, b)):
                    out.append(pytest.param(row.name, variant, bits, id=f"{row.name}-{variant}-{bits}"))
    return out


def ordered(s_first, s_second, what):
    """the later call (on s_second) must not complete while the earlier one (on s_first) is still queued: queries s_second, THEN s_first"""
    t0 = time.monotonic()
    while True:
        second_runs, first_runs = running(s_second), running(s_first)
        if not second_runs:
            assert not first_runs, f"{what}: the later call completed while the earlier one was still queued behind the blocker: not chained"
            return
        if not first_runs:
            return
        assert time.monotonic() - t0 < POLL_LIMIT_S, f"{what}: neither stream completed"


def chain(h, blocker, first, second, what):
    with streams(2) as (s1, s2):
        st1, st2 = Late(s1, blocker), Late(s2, None, delayed=False)
        c1, e1 = first.build(h, st1, rows_of(h, first))
        c2, e2 = second.build(h, st2, rows_of(h, second))
        warm(st1, c1)
        warm(st2, c2)
        st2.restore()
        st1.issue()
        check(c1())
        st1.issued(first.syncs)
        check(c2())
        ordered(s1, s2, what)
        compare(st1, e1, what + ": the earlier call")
        compare(st2, e2, what + ": the later call")


@pytest.mark.parametrize("name,variant,bits", b_cases())
def test_chained_across_streams(name, variant, bits, blocker, monkeypatch):
    h = fr.handle(bits)
    x, y = sc.BY_NAME[name], sc.BY_NAME[partner_of(name, h.key)]
    assert y.chained is True and y.build is not None
    env = sc.env_of(x._replace(tune={**(y.tune or {}), **(x.tune or {})}), variant)
    set_env(monkeypatch, env)
    chain(h, blocker, x, y, f"{x.name} then {y.name} [{variant}]")
    chain(h, blocker, y, x, f"{y.name} then {x.name} [{variant}]")


# ---- C. the staging rings wrap while their readers are still queued ----------------------------------------------------------------------
def test_host_stage_ring_wraps_behind_a_blocker(blocker, monkeypatch):
    """40 pai_ct_mul_host and 40 pai_ct_add_aligned_host calls behind ONE blocker each: more stagings than HostStageRing has slots
    (32), the caller's host buffer overwritten after every call.  The 33rd call may wait on the host until the blocker has run —
    that is the contract at work; a slot reused earlier gives a queued kernel another call's exponents."""
    from tests._util import pow_many

    set_env(monkeypatch, sc.env_of(sc.BY_NAME["pai_ct_mul_host"], "lat"))
    h = fr.handle(2048)
    nk, M, N, CALLS = h.nk, h.key.nsq, sc.N_TILE, 40
    _, a = sc.ciph(h, N, 70)
    _, b = sc.ciph(h, N, 71)
    es = [sc.expos(N, 53, 700 + i) for i in range(CALLS)]
    ds = [sc.deltas(N, 800 + i) for i in range(CALLS)]
    for which in ("mul", "aligned"):
        with streams(1) as (s,):
            st = Late(s, blocker)
            da, db = st.value(sc.L(a, nk.cw)), st.value(sc.L(b, nk.cw))
            outs = [st.out((N, nk.cw)) for _ in range(CALLS)]
            e_h, d_h = sc.L(es[0], 2), ds[0].copy()

            def call(i):
                if which == "mul":
                    np.copyto(e_h, sc.L(es[i], 2))
                    rc = nk.lib.pai_ct_mul_host(nk.pk, da.ptr, sc.host_ptr(e_h), 2, 53, 0, N, outs[i].ptr, st.stream)
                    e_h[:] = 0xFFFFFFFF                                  # the caller's buffer is free when the call returns
                else:
                    np.copyto(d_h, ds[i])
                    rc = nk.lib.pai_ct_add_aligned_host(nk.pk, da.ptr, db.ptr, 0, sc.host_ptr(d_h), N, outs[i].ptr, st.stream)
                    d_h[:] = 40
                return rc
            warm(st, lambda: call(0))
            st.issue()
            for i in range(CALLS):
                check(call(i))
                if i == 0:
                    st.issued()
            for i in range(CALLS):
                want = pow_many(a, es[i], M) if which == "mul" else sc.aligned(a, b, ds[i], M)
                compare(st, [(outs[i], sc.L(want, nk.cw))], f"{which} call {i} of {CALLS}")


def test_pinned_ring_and_exponent_buffer_of_modexp_fixed(blocker, monkeypatch):
    """8 pai_modexp_fixed calls with different exponents on one pai_modulus, alternating between two streams, the first behind a
    blocker: more than PinnedRing has slots (4), and every call rewrites the handle's one device exponent buffer — which must not
    reach a kernel that is still queued"""
    set_env(monkeypatch, {})
    h = fr.handle(2048)
    nk, M, N, CALLS = h.nk, h.key.nsq, sc.N_TILE, 8
    _, a = sc.ciph(h, N, 72)
    es = [(1 << 52) + 0x1234567 * (i + 1) for i in range(CALLS)]
    m = sc.modulus(h)
    with streams(2) as (s1, s2):
        st = Late(s1, blocker)
        da = st.value(sc.L(a, nk.cw))
        outs = [st.out((N, nk.cw)) for _ in range(CALLS)]
        e_h = sc.L([es[0]], 2)

        def call(i, stream):
            np.copyto(e_h, sc.L([es[i]], 2))
            rc = nk.lib.pai_modexp_fixed(m, da.ptr, sc.host_ptr(e_h), 2, N, outs[i].ptr, stream)
            e_h[:] = 0xFFFFFFFF
            return rc
        warm(st, lambda: call(0, st.stream))
        st.issue()
        for i in range(CALLS):
            check(call(i, s1 if i % 2 == 0 else s2))
            if i == 0:
                st.issued()
        sync(s2)
        for i in range(CALLS):
            compare(st, [(outs[i], sc.L([pow(x, es[i], M) for x in a], nk.cw))], f"pai_modexp_fixed call {i}")


@pytest.mark.parametrize("route", ["fused", "composition"])
def test_two_combines_with_different_theta_behind_one_blocker(route, blocker, monkeypatch):
    """pai_threshold_combine stages theta and the coefficients at its start and reads them in its last kernel: two calls with
    different theta (and different share sets) back to back behind one blocker, on both routes"""
    env = sc.env_of(sc.BY_NAME["pai_threshold_combine"], "lat")
    if route == "composition":
        env["PAI_DISABLE"] = "tcombine"
    set_env(monkeypatch, env)
    h = fr.handle(2048)
    nk, n, N = h.nk, h.key.n, sc.N_LANES
    with streams(1) as (s,):
        st = Late(s, blocker)
        calls = []
        for subset, scale in (((1, 2, 4), 1), ((2, 3, 5), 3)):
            m, parts, mu, neg, theta = sc.combine_operands(h, N, subset, 42)
            dparts = [st.value(sc.L(p, nk.cw)) for p in parts]
            out, fl = st.out((N, nk.nw)), st.resident(np.zeros(1, np.int32))
            mu_h, neg_h, th_h = sc.L(mu, 1), np.asarray(neg, dtype=np.int32), sc.L([theta * scale % n], nk.nw)
            ptrs = (C.c_void_p * 3)(*[p.ptr.value for p in dparts])
            calls.append(((lambda ptrs=ptrs, mu_h=mu_h, neg_h=neg_h, th_h=th_h, out=out, fl=fl: nk.lib.pai_threshold_combine(
                nk.pk, ptrs, 3, sc.host_ptr(mu_h), sc.host_ptr(neg_h), 1, sc.host_ptr(th_h), N, out.ptr, fl.ptr, None, st.stream)),
                [(out, sc.L([x * scale % n for x in m], nk.nw)), (fl, np.zeros(1, np.int32))]))
        for call, _ in calls:
            warm(st, call)
        st.issue()
        for call, _ in calls:
            check(call())
        st.issued()
        for i, (_, expected) in enumerate(calls):
            compare(st, expected, f"combine {i} [{route}]")


# ---- D. threads ------------------------------------------------------------------------------------------------------------------------------
THREAD_CALLS = ("pai_ct_mul", "pai_decrypt", "pai_ct_prod", "pai_sha256_rows", "pai_encrypt_crt", "pai_threshold_combine")
THREAD_ROUNDS = 8
JOIN_TIMEOUT_S = 120.0


def test_three_threads_share_one_handle_pair(monkeypatch):
    """ctypes releases the GIL, so the calls of the three threads overlap: each thread has a stream and inputs of its own and runs
    8 counted rounds of the six calls on ONE public / private handle pair; every output is exact.  A thread that has not ended by
    its join timeout ends the session: nothing more is started on the GPU."""
    env = {"PAI_TUNE": "fb_digit_wbits=6,crtenc_min=0,tcomb_min=0"}
    set_env(monkeypatch, env)
    h = fr.handle(2048)
    with streams(3) as ss:
        plans = []
        for t, s in enumerate(ss):
            st = Late(s, None, delayed=False)
            with sc.salted(f"thread{t}"):
                built = [sc.BY_NAME[name].build(h, st, sc.N_TILE + 5 * t) for name in THREAD_CALLS]
            plans.append((st, built))
        for st, built in plans:                        # lazy tables and scratch growth happen here, on one thread
            for call, _ in built:
                warm(st, call)
        for st, _ in plans:
            st.restore()
        errors = []

        def body(t):
            try:
                for _ in range(THREAD_ROUNDS):
                    for name, (call, _) in zip(THREAD_CALLS, plans[t][1]):
                        rc = call()
                        if rc:
                            raise AssertionError(f"thread {t}: {name} returned {rc}: {_native.load().pai_last_error().decode()}")
                rc = _native.load().pai_stream_sync(0, plans[t][0].stream)      # before the thread's pinned staging ring goes with the thread
                if rc:
                    raise AssertionError(f"thread {t}: pai_stream_sync returned {rc}")
            except BaseException as e:                 # noqa: BLE001 - handed to the main thread
                errors.append(e)
        threads = [threading.Thread(target=body, args=(t,), daemon=True) for t in range(3)]
        for th in threads:
            th.start()
        for th in threads:
            th.join(JOIN_TIMEOUT_S)
        alive = [i for i, th in enumerate(threads) if th.is_alive()]
        if alive:                                      # the stuck thread may hold a handle's mutex: the session ends here
            stop(f"threads {alive} still running after {JOIN_TIMEOUT_S} s (a deadlock between the handles' locks?)")
        assert not errors, errors
        for t, (st, built) in enumerate(plans):
            for name, (_, expected) in zip(THREAD_CALLS, built):
                compare(st, expected, f"thread {t}: {name}")


# ---- E. the public API on a torch side stream ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [1024, 2048])
def test_public_api_on_a_torch_side_stream(bits, blocker, monkeypatch):
    """tests/_transcripts.py's programs through the public classes inside `with torch.cuda.stream(...)`: engine.py hands torch's
    current stream to every call, so the whole library runs on a non-blocking stream, behind a blocker issued on that stream's raw
    handle at the head of each program — HostOperand's "next call only" rule and the host-computed exponents under a delayed stream."""
    import torch

    from tests import _transcripts as T
    from tests.test_gpu_transcripts import GOLD, ApiBackend

    assert bits in T.KEY_BITS
    set_env(monkeypatch, {})
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        B = ApiBackend(bits)
        for name in sorted(T.PROGRAMS):
            torch.cuda.synchronize()
            raw = C.c_void_p(side.cuda_stream)
            blocker(raw)
            assert running(raw), "the blocker ended before the program began (blocker too short)"
            got = T.run_program(name, B)
            want = GOLD["keys"][str(bits)][name]
            assert set(got) == set(want)
            for k in want:
                assert got[k]["expo"] == want[k]["expo"], (name, k, "exponents")
                assert got[k]["ct"] == want[k]["ct"], (name, k, "ciphertext bits")
                assert got[k]["dec"] == want[k]["dec"], (name, k, "decoded values")
    torch.cuda.synchronize()
