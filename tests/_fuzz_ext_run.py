"""The device half of the differential fuzz for the extension entry points: runs the cases of tests/_fuzz_ext.py through the raw
C ABI (NativeKey, DevArray) and compares every row with the case's expectation.  Shared by tests/test_gpu_fuzz_ext.py (knobs
through monkeypatch) and tools/fuzz_ext_gpu.py (knobs through the environment): `with_knobs(run)` is the caller's context
manager that sets one entry of a case's `runs` and restores the environment on exit.

A mismatch raises AssertionError with the reproducer line of tests/_fuzz_ext.reproducer.  What ran is recorded per call as
"kernel:path" (pai_profile_last / pai_profile_last_path) in the caller's coverage set; the multi-level calls add
"k_segprod:levels>=2" / "k_segscan:carry" when more than one launch of the kernel was recorded.  The profile gives k_smexp no
path, so the sparse family's "[digit pairs]" / "[lane groups]" labels are INFERRED from the handle the call ran on (the default
handle of a key the digit engine serves, or one created under PAI_DISABLE=padic), not read from the library."""
from __future__ import annotations

import ctypes as C
import gc
import json
from pathlib import Path

import numpy as np

from oracle import paillier_oracle as orc
from pailliercryptolib_python_amd import _native
from tests import _fuzz_ext as fz
from tests import _streams
from tests._util import DevArray, host_ptr, ints_to_limbs, limbs_to_ints

ROOT = Path(__file__).resolve().parents[1]
FIXTURE_BITS = (1024, 2048, 3072, 4096)
DJN_X = (1 << 70) + 12345


def oracle_key(bits):
    """the committed fixture primes at 1024 / 2048 / 3072 / 4096 bits, the native generator seeded with `bits` elsewhere; DJN"""
    if bits in FIXTURE_BITS:
        fx = json.loads((ROOT / "tests" / "golden" / "fixture_keys.json").read_text())
        if str(bits) in fx:
            return orc.make_key(int(fx[str(bits)]["p"], 16), int(fx[str(bits)]["q"], 16), djn_x=DJN_X, bits=bits)
        assert bits == 2048
        return orc.make_key(orc.BENCH_P, orc.BENCH_Q, djn_x=DJN_X, bits=2048)
    p, q = _native.keygen(bits, True, seed=bits)
    return orc.make_key(p, q, djn_x=DJN_X, bits=bits)


class Handle:
    """one key with its raw-ABI handles: `nk` as the library chooses, `nk_off` created under PAI_DISABLE=padic (lane groups
    where the digit engine would serve; on demand)"""

    def __init__(self, bits):
        from tests.test_gpu_paillier_abi import NativeKey

        self._NativeKey = NativeKey
        self.key = oracle_key(bits)
        self.nk = NativeKey(self.key)
        self.nk_off = None
        rb = C.c_int(0)
        _native.check(self.nk.lib.pai_pubkey_mont_bits(self.nk.pk, C.byref(rb)))
        self.R = pow(2, rb.value, self.key.nsq)

    def padic_off(self, with_knobs):
        if self.nk_off is None:
            with with_knobs(fz.knobs(disable=["padic"])):
                self.nk_off = self._NativeKey(self.key)
        return self.nk_off


_HANDLES = {}


def handle(bits):
    if bits not in _HANDLES:
        _HANDLES[bits] = Handle(bits)
    return _HANDLES[bits]


def release_handles():
    _HANDLES.clear()
    gc.collect()


def ran(lib):
    from tests.test_gpu_paillier_abi import _last_kernels

    buf = C.create_string_buffer(64)
    out = []
    for i, nm in enumerate(_last_kernels(lib)):
        _native.check(lib.pai_profile_last_path(i, buf, 64))
        out.append(f"{nm}:{buf.value.decode()}")
    return out


def has(names, kernel):
    return any(n.split(":")[0] == kernel or n.split(":")[0].startswith(kernel + "(") for n in names)


class Checker:
    def __init__(self, case, seed, cov, profiled=True):
        self.c, self.seed, self.cov, self.checks, self.profiled = case, seed, cov, 0, profiled

    def ran(self, lib, label=""):
        names = ran(lib)
        self.cov.update(n + label for n in names)
        return names

    def rows(self, run, what, got, want, skip=()):
        self.checks += 1
        if len(got) != len(want):
            raise AssertionError(fz.reproducer(self.c, self.seed, run, what + " (row count)", len(got), len(got), len(want)))
        for i, (g, w) in enumerate(zip(got, want)):
            if g != w and i not in skip:
                raise AssertionError(fz.reproducer(self.c, self.seed, run, what, i, g, w))

    def that(self, ok, run, what, got=None, want=None):
        if what.startswith("kernels") and not self.profiled:
            return                                   # the kernel timers synchronise: a delayed stream runs without the profile
        self.checks += 1
        if not ok:
            raise AssertionError(fz.reproducer(self.c, self.seed, run, what, "-", got, want))


def tagged(h, vals, tag):
    f = pow(h.R, tag, h.key.nsq)
    return [v * f % h.key.nsq for v in vals]


def placement(stream):
    """`stream` of a runner: None — resident operands, the null stream; or a tests/_streams.Late — value operands arrive behind its
    blocker, the calls go to its stream"""
    return _streams.Resident() if stream is None else stream


def dev(nk, vals, words=None, st=None):
    """a value operand: rows of residues or exponents"""
    return (st or _streams.Resident()).value(ints_to_limbs(vals, words or nk.cw))


def opt(arr, st=None):
    """an operand the kernels index with (rows, offsets, shifts, steps, signs): resident on every placement"""
    return None if arr is None else (st or _streams.Resident()).resident(arr)


def ptr(d):
    return None if d is None else d.ptr


def status(nk, clear=1, stream=None):
    st = C.c_int(-1)
    _native.check(nk.lib.pai_pubkey_status(nk.pk, C.byref(st), clear, stream))
    return st.value


# ---- the families ------------------------------------------------------------------------------------------------------------------
def run_segprod(h, c, ck, with_knobs, stream=None):
    nk, lib, st = h.nk, h.nk.lib, placement(stream)
    dct = dev(nk, tagged(h, c["cts"], c["tag"]), st=st)
    drows, dshift, doff = opt(c["rows"], st), opt(c["shift"], st), st.resident(c["offsets"])
    out = st.out((c["S"], nk.cw))
    for run in c["runs"]:
        with with_knobs(run):
            st.issue()
            _native.check(lib.pai_ct_segment_prod(nk.pk, dct.ptr, c["N"], c["tag"], ptr(drows), ptr(dshift), doff.ptr, c["S"], out.ptr, st.stream))
            st.issued(syncs=True)
            names = ck.ran(lib)
            ck.rows(run, "pai_ct_segment_prod", limbs_to_ints(st.read(out)), c["want"])
            ck.that(set(names) == {"k_segprod:"}, run, "kernels", names)
            if len(names) >= 2:
                ck.cov.add("k_segprod:levels>=2")
            sw = status(nk, stream=st.stream)
            ck.that(sw == c["status_bit"], run, "status word", sw, c["status_bit"])


def run_scan(h, c, ck, with_knobs, stream=None):
    nk, lib, M, st = h.nk, h.nk.lib, h.key.nsq, placement(stream)
    dct = dev(nk, tagged(h, c["cts"], c["tag"]), st=st)
    draise, dstep = opt(c["raise"], st), opt(c["step"], st)
    out = st.out((c["N"], nk.cw))
    want = tagged(h, c["want"], c["dom_out"])
    for run in c["runs"]:
        with with_knobs(run):
            st.issue()
            _native.check(lib.pai_ct_scan(nk.pk, dct.ptr, c["N"], c["tag"], c["dom_out"], c["seg_len"], c["reverse"], ptr(draise), ptr(dstep),
                                          out.ptr, st.stream))
            st.issued()
            names = ck.ran(lib)
            ck.rows(run, "pai_ct_scan", limbs_to_ints(st.read(out)), want)
            ck.that(set(names) == {"k_segscan:"}, run, "kernels", names)
            if len(names) >= 2:
                ck.cov.add("k_segscan:carry")
            sw = status(nk, stream=st.stream)
            ck.that(sw == c["status_bit"], run, "status word", sw, c["status_bit"])


def run_smexp(h, c, ck, with_knobs, stream=None):
    st = placement(stream)
    handles = [("", h.nk)]
    if c["second_handle_padic_off"]:
        handles.append(("[PAI_DISABLE=padic handle]", h.padic_off(with_knobs)))
    for label, nk in handles:
        lib = nk.lib
        dbase, dinv = dev(nk, c["base"], st=st), (dev(nk, c["inv"], st=st) if c["inv"] is not None else None)
        didx, de = st.resident(c["bidx"]), dev(nk, c["e"], c["e_words"], st=st)
        dsign, doff = opt(c["sign"], st), st.resident(c["offsets"])
        out = st.out((c["S"], nk.cw))
        digit = fz.digit_served(h.key.n.bit_length()) and not label
        for run in c["runs"]:
            with with_knobs(run):
                st.issue()
                _native.check(lib.pai_ct_sparse_multiexp(nk.pk, dbase.ptr, ptr(dinv), c["N"], didx.ptr, de.ptr, c["e_words"], c["ebits"], ptr(dsign),
                                                         c["T"], doff.ptr, c["S"], out.ptr, st.stream))
                st.issued(syncs=True)
                names = ck.ran(lib, "[digit pairs]" if digit else "[lane groups]")          # inferred from the handle (module docstring)
                ck.rows(run, "pai_ct_sparse_multiexp" + label, limbs_to_ints(st.read(out)), c["want"])
                ck.that(has(names, "k_smexp"), run, "kernels" + label, names)
                sw = status(nk, stream=st.stream)
                ck.that(sw == c["status_bit"], run, "status word" + label, sw, c["status_bit"])


def run_pack(h, c, ck, with_knobs, stream=None):
    nk, lib, st = h.nk, h.nk.lib, placement(stream)
    N, b, k, N2, step, count = c["N"], c["slot_bits"], c["slots"], c["N_step"], c["step_bits"], c["count"]
    dct = dev(nk, tagged(h, c["cts"], c["tag"]), st=st)
    out = st.out((len(c["want"]), nk.cw))
    out2 = st.out((len(c["want_step"]), nk.cw))
    digit = fz.digit_served(h.key.n.bit_length()) and c["tag"] == 0
    for run in c["runs"]:
        with with_knobs(run):
            fused = digit and not run["disable"]
            for what, call, o, want in (
                    (f"pai_ct_pack({b}, {k})", lambda: lib.pai_ct_pack(nk.pk, dct.ptr, N, c["tag"], b, k, out.ptr, st.stream), out, c["want"]),
                    (f"pai_ct_pack_step({b}, {k})", lambda: lib.pai_ct_pack_step(nk.pk, dct.ptr, N, c["tag"], b, k, out.ptr, st.stream), out, c["want"]),
                    (f"pai_ct_pack_step({step}, {count})", lambda: lib.pai_ct_pack_step(nk.pk, dct.ptr, N2, c["tag"], step, count, out2.ptr, st.stream),
                     out2, c["want_step"])):
                st.issue()
                _native.check(call())
                st.issued(syncs=not fused)                 # the level driver reads its sizes back; one chain per lane is asynchronous
                names = ck.ran(lib)
                ck.rows(run, what, limbs_to_ints(st.read(o)), want)
                ck.that(has(names, "k_ct_pack_padic") == fused and (fused or set(names) == {"k_segprod:"}), run, "kernels of " + what, names)


def run_open(h, c, ck, with_knobs, stream=None):
    nk, lib, st = h.nk, h.nk.lib, placement(stream)
    N = c["N"]
    dct, outr = dev(nk, c["cts"], st=st), st.out((N, nk.nw))
    st.issue()
    _native.check(lib.pai_recover_r(nk.sk, dct.ptr, N, outr.ptr, st.stream))
    st.issued()
    names = ck.ran(lib)
    ck.rows("-", "pai_recover_r", limbs_to_ints(st.read(outr)), c["want_r"])
    ck.that(has(names, "k_rrec_a") and has(names, "k_rrec_b"), "-", "kernels of pai_recover_r", names)
    S = len(c["want_lhs"])
    fct, fm, fr = dev(nk, c["fold_ct"], st=st), dev(nk, c["fold_m"], nk.nw, st=st), dev(nk, c["fold_r"], nk.nw, st=st)
    fe = dev(nk, c["e"], c["e_words"], st=st)
    lhs, rhs = st.out((S, nk.cw)), st.out((S, nk.cw))
    for run in c["runs"]:
        with with_knobs(run):
            flag = st.resident(np.zeros(1, dtype=np.int32))
            st.issue()
            _native.check(lib.pai_opening_fold(nk.pk, fct.ptr, fm.ptr, fr.ptr, N, fe.ptr, c["e_words"], c["ebits"], c["seg_len"], lhs.ptr, rhs.ptr,
                                               flag.ptr, st.stream))
            st.issued(syncs=True)
            names = ck.ran(lib)
            ck.rows(run, "pai_opening_fold lhs", limbs_to_ints(st.read(lhs)), c["want_lhs"])
            ck.rows(run, "pai_opening_fold rhs", limbs_to_ints(st.read(rhs)), c["want_rhs"])
            got = int(st.read(flag)[0])
            ck.that(got & 1 == c["want_flag"], run, "pai_opening_fold flag", got, c["want_flag"])
            fused = fz.digit_served(h.key.n.bit_length()) and not run["disable"]
            ck.that(has(names, "k_open_fold") == fused, run, "kernels of pai_opening_fold", names)


def run_crtenc(h, c, ck, with_knobs, stream=None):
    nk, lib, st = h.nk, h.nk.lib, placement(stream)
    N = c["N"]
    dm, dr = dev(nk, c["m"], nk.nw, st=st), dev(nk, c["r"], nk.rw, st=st)
    out = st.out((N, nk.cw))
    for run in c["runs"]:                                  # the served route first: a handle's first call decides its CRT constants
        with with_knobs(run):
            st.issue()
            _native.check(lib.pai_encrypt_crt(nk.sk, dm.ptr, dr.ptr, N, out.ptr, st.stream))
            st.issued()
            names = ck.ran(lib)
            ck.rows(run, "pai_encrypt_crt", limbs_to_ints(st.read(out)), c["want_enc"])
            lift = c["served"] and not run["disable"]
            ck.that(has(names, "k_crt_lift") == lift and (lift or has(names, "k_encrypt")), run, "kernels of pai_encrypt_crt", names)
            ct = dev(nk, c["cts"], st=st)
            st.issue()
            _native.check(lib.pai_obfuscate_crt(nk.sk, ct.ptr, dr.ptr, N, st.stream))
            st.issued()
            names = ck.ran(lib)
            ck.rows(run, "pai_obfuscate_crt", limbs_to_ints(st.read(ct)), c["want_obf"])
            ck.that(has(names, "k_crt_lift") == lift and (lift or has(names, "k_encrypt")), run, "kernels of pai_obfuscate_crt", names)


def run_tpart(h, c, ck, with_knobs, stream=None):
    nk, lib, st = h.nk, h.nk.lib, placement(stream)
    N = c["N"]
    dct = dev(nk, c["cts"], st=st)
    out = st.out((N, nk.cw))
    for run in c["runs"]:
        with with_knobs(run):
            for E, want in zip(c["E"], c["want"]):
                ew = (E.bit_length() + 31) // 32
                sh = C.c_void_p()
                _native.check(lib.pai_keyshare_create(nk.pk, host_ptr(ints_to_limbs([E], ew)), ew, C.byref(sh)))
                try:
                    st.issue()
                    _native.check(lib.pai_partial_decrypt(sh, dct.ptr, N, out.ptr, st.stream))
                    st.issued()
                    names = ck.ran(lib)
                    got = limbs_to_ints(st.read(out))
                finally:
                    lib.pai_keyshare_destroy(sh)
                what = f"pai_partial_decrypt E of {E.bit_length()} bits, {bin(E).count('1')} set"
                ck.rows(run, what, got, want)
                ck.that(has(names, "k_pow_padic") == c["digit_route"], run, "kernels of " + what, names)
                if not c["digit_route"] and E.bit_length() > 64:
                    ck.that(has(names, "k_ctmul"), run, "kernels of " + what, names)


def run_tcomb(h, c, ck, with_knobs, stream=None):
    nk, lib, st = h.nk, h.nk.lib, placement(stream)
    N, t = c["N"], c["t"]
    mu = ints_to_limbs(c["mu"], c["mu_words"])
    neg = np.asarray(c["neg"], dtype=np.int32)
    theta = ints_to_limbs([c["theta"]], nk.nw)
    digit = fz.digit_served(h.key.n.bit_length())
    m = st.out((N, nk.nw))

    def combine(parts):
        ptrs = (C.c_void_p * t)(*[p.ptr.value for p in parts])
        flag, rowflag = st.resident(np.zeros(1, dtype=np.int32)), st.resident(np.zeros(N, dtype=np.int32))
        st.issue()
        _native.check(lib.pai_threshold_combine(nk.pk, ptrs, t, host_ptr(mu), host_ptr(neg), c["mu_words"], host_ptr(theta), N, m.ptr, flag.ptr,
                                                rowflag.ptr, st.stream))
        st.issued()
        _native.check(lib.pai_stream_sync(0, st.stream))
        return limbs_to_ints(st.read(m)), int(st.read(flag)[0]), st.read(rowflag).tolist()

    parts = [dev(nk, p, st=st) for p in c["parts"]]
    poisoned = None
    if c["poison"] is not None:
        j, i, v = c["poison"]
        bad = list(c["parts"][j])
        bad[i] = v
        poisoned = parts[:j] + [dev(nk, bad, st=st)] + parts[j + 1:]
    seen = []
    for run in c["runs"]:
        with with_knobs(run):
            got, fl, rf = combine(parts)
            names = ck.ran(lib)
            ck.rows(run, "pai_threshold_combine d_rowflag", rf, c["want_rowflag"])
            ck.that(fl == int(any(c["want_rowflag"])), run, "pai_threshold_combine flag", fl, int(any(c["want_rowflag"])))
            ck.rows(run, "pai_threshold_combine d_m", got, c["want"], skip={i for i, f in enumerate(c["want_rowflag"]) if f})
            fused = digit and not run["disable"]
            ck.that(has(names, "k_tfinish") and has(names, "k_tcomb_padic") == fused, run, "kernels of pai_threshold_combine", names)
            seen.append(got)
            if poisoned is not None:
                _, fl, _ = combine(poisoned)
                ck.that(fl & 2 == 2, run, "pai_threshold_combine flag bit 1 (a part of the negative side that is no unit)", fl, 2)
    ck.rows(c["runs"][1], "pai_threshold_combine: the two routes differ", seen[1], seen[0])


RUNNERS = {"segprod": run_segprod, "scan": run_scan, "smexp": run_smexp, "pack": run_pack, "open": run_open, "crtenc": run_crtenc,
           "tpart": run_tpart, "tcomb": run_tcomb}


def run_round(family, cls, seed, rnd, with_knobs, cov, stream=None, bits=None):
    """one round of one family on the key of its class for that round (or on the key of `bits` bits); `stream`: None, or the
    tests/_streams.Late placement the value operands arrive through (no kernel timers then: they synchronise, so the kernel-name
    comparisons are left to the null-stream run).  Returns the number of comparisons made"""
    h = handle(bits or fz.key_bits_for(cls, rnd))
    c = fz.case(family, h.key, seed, rnd)
    ck = Checker(c, seed, cov, profiled=stream is None)
    RUNNERS[family](h, c, ck, with_knobs, stream)
    return ck.checks
