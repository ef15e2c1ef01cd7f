"""GPU: every entry point that writes device memory, held to the memory contract of include/paillier_hip.h (conventions block):
alignment of the C type and no more, no write outside the documented outputs, no write into an input, exact aliasing where a
call promises it and PAI_E_INVALID — nothing launched — for every other overlap.

Every pointer argument of a case lives in a guard-band arena (tests/_arena.py; its own logic is held by tests/test_arena_cpu.py):
one allocation per case, filled with a position-dependent word pattern or with all-ones words, every operand between two guards
of max(4096 bytes, 4 rows).  After the call and a synchronisation the whole arena is compared with the host shadow in which only
the documented outputs are replaced by their expectations.  Every case runs with all operands `aligned` (256 bytes) and with all
operands `natural` (4 mod 16 for words, 8 mod 16 for doubles / int64, an odd address for bytes), under both fillers.
Expectations are CPython integers and the C oracle (tests/_util.pow_many, djn_encrypt_many; the models of the segment, scan,
packed and quantiser tests) — never a second run of the library.

Keys (module-scoped handles, DJN, fixed x): the 2048-bit bench key (rows of 64 / 128 words), seeded_key(3072) (96 / 192 words,
lane-group pairs), and the two limit keys on which a row offset alone breaks 16-byte alignment: hi-nl36 (n of 521 bits, rows of
17 / 34 words, wider than their geometry) and hi-nl112 (n of 1623 bits, rows of 51 / 102 words, digit engine).  Batches: N = 1,
and one full plus one ragged tile of the path that runs — 70 at the 64-element tiles, 37 at the 32-element tiles of the 3072-bit
key, 257 on hi-nl36, whose lane-group geometry (36 x 1) has 256 elements per workgroup, and 257 wherever a call runs on the digit
engine (one element per lane, tiles of 256): encryption, obfuscation, raw encryption, ct * pt fresh and in place, pai_ct_pow2 and
pai_decrypt on the 2048-bit key and hi-nl112, and 258 output rows of pai_ct_pack / pai_ct_pack_step there.

Paths are forced with the suite's knobs (PAI_LATENCY_MAX, PAI_LAT_ADD_MAX, PAI_TUNE, PAI_DISABLE) and what ran is read back
(pai_profile_last / pai_profile_last_path) and recorded per key; the last test prints it and requires the families of FAMILIES.
Hand-downs (pp -> rl -> window where a key has no four-wave or minus-one context; no most-significant-limb-first product on the
limit keys; pair4 only where n fits the 4-lane geometries) are recorded as what ran and printed as HANDDOWN lines."""
import ctypes as C
import json
import math
import random
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import paillier_oracle as orc
from pailliercryptolib_python_amd import _native, fixedpoint
from tests._arena import ALIGNS, FILLERS, Arena
from tests._util import chacha_block, djn_encrypt_many, djn_obfuscate_many, host_ptr, ints_to_limbs, model_pack, pow_many, tune
from tests._util import disable as knob_disable
from tests.test_gpu_aggregate_limits import want_segprod
from tests.test_gpu_cumsum import want_chain
from tests.test_gpu_extreme_keys import Key, ciphertexts, decrypt_many, plain, rand_r
from tests.test_gpu_packed_rows import want_stepped
from tests.test_gpu_padic_kara_mul import MODES
from tests.test_gpu_paillier_abi import NativeKey, _last_kernels
from tests.test_limit_keys_cpu import load_limit_keys
from tests.test_packed_linear_cpu import quantize_model

pytestmark = pytest.mark.gpu

PAI_E_INVALID = -1
KEY_IDS = ["k2048", "k3072", "hi-nl36", "hi-nl112"]
TILE = {"k2048": 70, "k3072": 37, "hi-nl36": 257, "hi-nl112": 70}
RAN = {}                       # (key, operation) -> {"kernel:path"}
UNPROFILED = {"codec", "buffers", "modarith", "ct_mul_untimed"}       # calls without a kernel timer: pai_profile_last still holds an earlier call's entries
HANDDOWN = set()
VISITED = set()
# what the last test requires to have run on SOME key (on the 2048-bit key: at least the list of tests/test_gpu_extreme_keys.py)
FAMILIES = {
    "encrypt": {f"k_encrypt(djn):{x}" for x in ("padic", "pair", "lane_group", "pair4", "lat_tree_m1", "lat_tree", "lat_chain")},
    "decrypt": {f"k_dec_a:{x}" for x in ("pp", "rl", "window", "pair4", "padic", "padic_kara_mul", "padic_kara", "padic_rowwise", "wide", "lane_group")},
    "ct_mul": {f"k_ctmul:{x}" for x in ("pp", "rl", "window", "pair4", "padic", "pair", "lane_group")},
    "ct_add": {"k_modmul_msb:lane_group", "k_modmul:lane_group", "k_modmul:lat", "k_add_aligned:lane_group", "k_pow2:lane_group", "k_pow2:lat", "k_pow2:padic"},
    "aggregate": {"k_addn:", "k_segprod:", "k_segscan:", "k_invert:"},
}


def make_key(ident):
    if ident == "k2048":
        return Key(ident, "bench", 1024, orc.BENCH_P, orc.BENCH_Q)
    if ident == "k3072":
        fx = json.loads((Path(__file__).parent / "golden" / "fixture_keys.json").read_text())["3072"]
        return Key(ident, "seeded", 1536, int(fx["p"], 16), int(fx["q"], 16))
    _, kind, _, _, pb, p, q = next(e for e in load_limit_keys() if e[0] == ident)
    return Key(ident, kind, pb, p, q)


@pytest.fixture(scope="module", params=KEY_IDS)
def mk(request):
    lib = _native.load()
    _native.check(lib.pai_profile_enable(1))
    k = make_key(request.param)
    k.T = TILE[k.ident]
    rb = C.c_int(0)
    _native.check(lib.pai_pubkey_mont_bits(k.nk.pk, C.byref(rb)))
    k.R = pow(2, rb.value, k.key.nsq)
    nb = k.key.n.bit_length()
    k.thr = "padic" if 700 <= nb <= 1024 or 1400 <= nb <= 2068 else ("pair" if nb > 2048 else "lane_group")
    VISITED.add(k.ident)
    yield k
    _native.check(lib.pai_profile_enable(0))


def ran(k, op):
    lib = k.nk.lib
    buf = C.create_string_buffer(64)
    out = []
    for i, nm in enumerate(_last_kernels(lib)):
        _native.check(lib.pai_profile_last_path(i, buf, 64))
        out.append(f"{nm}:{buf.value.decode()}")
    RAN.setdefault((k.ident, op), set()).update(out)
    return out


def sweep(k, op, build, allowed=None):
    """build(P) places the operands of one case through P(name, host=None, shape=..., dtype=...) and returns (call, expected):
    `call` runs the library once the arena is committed and returns its status, `expected` maps the output regions to their
    values.  Runs under both alignment classes and both fillers; returns what ran."""
    lib = k.nk.lib
    paths = None
    for al in ALIGNS:
        for fill in FILLERS:
            ar = Arena(fill)
            try:
                call, expected = build(lambda name, host=None, **kw: ar.place(name, host, align=al, **kw))
                ar.commit()
                _native.check(call())
                paths = ran(k, op) if op not in UNPROFILED else []
                _native.check(lib.pai_stream_sync(0, None))
                try:
                    ar.check(expected)
                except AssertionError as e:
                    raise AssertionError(f"{op} on {k.ident}, operands {al}, ran {paths}: {e}") from None
                if allowed is not None:
                    assert paths and paths[0].split(":")[1] in allowed, (op, k.ident, paths, allowed)
            finally:
                ar.free()
    return paths


def refused(k, op, build, message):
    """the call returns PAI_E_INVALID with `message` in pai_last_error() and leaves the arena as it was"""
    lib = k.nk.lib
    for al in ALIGNS:
        ar = Arena("pattern")
        try:
            call = build(lambda name, host=None, **kw: ar.place(name, host, align=al, **kw))
            ar.commit()
            rc = call()
            msg = lib.pai_last_error().decode()
            assert rc == PAI_E_INVALID and message in msg, (op, k.ident, al, rc, msg)
            _native.check(lib.pai_stream_sync(0, None))
            ar.check({})
        finally:
            ar.free()


def L(vals, words):
    return ints_to_limbs(vals, words)


def sizes(k, throughput=False):
    """N = 1 and one full plus one ragged tile: k.T on the lane-group and latency kernels; 257 where the call runs on the digit engine,
    whose kernels (k_encrypt_padic, k_ctmul_padic, k_ct_pack_padic) walk tiles of 256 elements, one per lane"""
    return (1, 257 if throughput and k.thr == "padic" else k.T)


def knobs_default(monkeypatch):
    for v in ("PAI_LATENCY_MAX", "PAI_LAT_ADD_MAX", "PAI_TUNE", "PAI_DISABLE"):
        monkeypatch.delenv(v, raising=False)


# ---- encryption and decryption ----------------------------------------------------------------------------------------------------
def test_encrypt_obfuscate_raw(mk, monkeypatch):
    """pai_raw_encrypt, pai_encrypt (DJN) and pai_obfuscate (in place by definition) on the throughput engine of the key, the three
    small-batch chains and, where n fits the 4-lane geometries, the mid-size digit-pair kernel"""
    k, nk, key = mk, mk.nk, mk.key
    lib = nk.lib
    N = max(sizes(k, True))
    m, r = plain(k, N, 1), rand_r(k, N, 2)
    want = djn_encrypt_many(key, m, r)
    assert want[:2] == [orc.encrypt(key, x, rr) for x, rr in zip(m[:2], r[:2])]
    want2 = djn_obfuscate_many(key, want, r)
    raw = [orc.raw_encrypt(x, key.n) for x in m]
    mid = 2 * k.b in (1024, 2048)
    cfgs = [("0", None, None, False, {k.thr}), ("100000", "100000", False, False, {"lat_tree_m1", "lat_tree"}),
            ("100000", "100000", True, False, {"lat_tree"}), ("100000", "0", False, False, {"lat_chain"})]
    if mid:
        cfgs.append(("100000", None, None, True, {"pair4"}))
    else:
        HANDDOWN.add(f"{k.ident}: no mid-size digit-pair kernel (pair4) for encryption, decryption and ct * pt: n does not fit the 4-lane geometries")
    for switch, tree, no_m1, use_mid, allowed in cfgs:
        monkeypatch.setenv("PAI_LATENCY_MAX", switch)
        tune(monkeypatch, "lat_enc_tree", tree)
        knob_disable(monkeypatch, "lat_enc_m1", bool(no_m1))
        tune(monkeypatch, "enc_mid_min", 0 if use_mid else None)
        tune(monkeypatch, "enc_mid_max", 1 << 30 if use_mid else None)
        for n in sizes(k, switch == "0"):
            def enc(P, n=n):
                dm, dr, ct = P("m", L(m[:n], nk.nw)), P("r", L(r[:n], nk.rw)), P("ct", shape=(n, nk.cw))
                return (lambda: lib.pai_encrypt(nk.pk, dm.ptr, dr.ptr, n, ct.ptr, None)), {"ct": L(want[:n], nk.cw)}

            def obf(P, n=n):
                dr, ct = P("r", L(r[:n], nk.rw)), P("ct", L(want[:n], nk.cw))
                return (lambda: lib.pai_obfuscate(nk.pk, ct.ptr, dr.ptr, n, None)), {"ct": L(want2[:n], nk.cw)}
            got = sweep(k, "encrypt", enc, allowed)
            if allowed == {"lat_tree_m1", "lat_tree"} and got[0].endswith(":lat_tree"):
                HANDDOWN.add(f"{k.ident}: pai_encrypt lat_tree_m1 -> lat_tree (no minus-one context)")
            sweep(k, "encrypt", obf, allowed)
    knobs_default(monkeypatch)
    for lat_add, allowed in (("0", {"padic" if k.thr == "padic" else "lane_group"}), ("4096", {"lat"})):
        monkeypatch.setenv("PAI_LAT_ADD_MAX", lat_add)
        for n in sizes(k, lat_add == "0"):
            def rawenc(P, n=n):
                dm, ct = P("m", L(m[:n], nk.nw)), P("ct", shape=(n, nk.cw))
                return (lambda: lib.pai_raw_encrypt(nk.pk, dm.ptr, n, ct.ptr, None)), {"ct": L(raw[:n], nk.cw)}
            sweep(k, "encrypt", rawenc, allowed)


def test_standard_scheme_2048(monkeypatch):
    """pai_encrypt and pai_obfuscate with the obfuscator r^n (the power goes through the handle's scratch, then k_encrypt modes 3 / 4)"""
    lib = _native.load()
    _native.check(lib.pai_profile_enable(1))
    key = orc.make_key(orc.BENCH_P, orc.BENCH_Q, djn_x=None, bits=2048)
    nk = NativeKey(key)
    k = SimpleNamespace(ident="k2048-std", nk=nk, key=key)
    N = 70
    m = plain(k, N, 21)
    r = [x or 1 for x in ([1, key.n - 1, 2] + [random.Random(5).randrange(1, key.n) for _ in range(N)])[:N]]
    obf = pow_many(r, key.n, key.nsq)
    want = [(1 + x * key.n) % key.nsq * o % key.nsq for x, o in zip(m, obf)]
    assert want[1] == orc.encrypt(key, m[1], r[1])
    want2 = [c * o % key.nsq for c, o in zip(want, obf)]
    for n in (1, N):
        def enc(P, n=n):
            dm, dr, ct = P("m", L(m[:n], nk.nw)), P("r", L(r[:n], nk.nw)), P("ct", shape=(n, nk.cw))
            return (lambda: lib.pai_encrypt(nk.pk, dm.ptr, dr.ptr, n, ct.ptr, None)), {"ct": L(want[:n], nk.cw)}

        def ob(P, n=n):
            dr, ct = P("r", L(r[:n], nk.nw)), P("ct", L(want[:n], nk.cw))
            return (lambda: lib.pai_obfuscate(nk.pk, ct.ptr, dr.ptr, n, None)), {"ct": L(want2[:n], nk.cw)}
        sweep(k, "encrypt_std", enc)
        sweep(k, "encrypt_std", ob)
    _native.check(lib.pai_profile_enable(0))


def test_decrypt_and_recover(mk, monkeypatch):
    """pai_decrypt on the throughput engine (257: the 256-element tiles of the one-element-per-lane kernels), the four-wave, wave-pair
    and window kernels and the mid-size stage A; pai_recover_r on openings built from known r"""
    k, nk, key = mk, mk.nk, mk.key
    lib = nk.lib
    cts = ciphertexts(k, 257, 3, units=True)
    want = decrypt_many(k, cts)
    assert want[:2] == [orc.decrypt_crt(key, c) for c in cts[:2]]

    def dec(n):
        def build(P):
            ct, out = P("ct", L(cts[:n], nk.cw)), P("m", shape=(n, nk.nw))
            return (lambda: lib.pai_decrypt(nk.sk, ct.ptr, n, out.ptr, None)), {"m": L(want[:n], nk.nw)}
        return build
    monkeypatch.setenv("PAI_LATENCY_MAX", "0")
    tune(monkeypatch, "dec_mid_max", 0)
    kara = 676 < k.b <= 1024                                 # 36-limb primes: the three MODES of tests/test_gpu_padic_kara_mul.py
    for mode in (MODES if kara else ["padic"]):
        for name in ("padic_kara_mul", "padic_kara"):
            knob_disable(monkeypatch, name, kara and name in MODES[mode])
        for n in (1, 257):
            sweep(k, "decrypt", dec(n))
    knob_disable(monkeypatch, "padic_kara_mul", False)
    knob_disable(monkeypatch, "padic_kara", False)
    tune(monkeypatch, "dec_mid_max", None)
    monkeypatch.setenv("PAI_LATENCY_MAX", "100000")
    for pp, rl, allowed in (("100000", "100000", {"pp", "rl", "window"}), ("0", "100000", {"rl", "window"}), ("0", "0", {"window"})):
        tune(monkeypatch, "lat_pp", pp)
        tune(monkeypatch, "lat_rl", rl)
        for n in (1, 70):
            got = sweep(k, "decrypt", dec(n), allowed)
            want_path = "pp" if pp != "0" else ("rl" if rl != "0" else "window")
            if got[0].split(":")[1] != want_path:
                HANDDOWN.add(f"{k.ident}: pai_decrypt {want_path} -> {got[0].split(':')[1]}")
    if 2 * k.b in (1024, 2048):
        tune(monkeypatch, "dec_mid_min", 0)
        tune(monkeypatch, "dec_mid_max", 1 << 30)
        sweep(k, "decrypt", dec(70), {"pair4"})
    knobs_default(monkeypatch)
    N = 70
    rs = [x or 1 for x in ([1, key.n - 1, 2, key.n - 2] + plain(k, N, 31))[:N] if math.gcd(x or 1, key.n) == 1][:N]
    N = len(rs)
    ms = plain(k, N, 32)
    op = pow_many(rs, key.n, key.nsq)
    cts2 = [(1 + m * key.n) % key.nsq * o % key.nsq for m, o in zip(ms, op)]
    for n in (1, N):
        def rec(P, n=n):
            ct, out = P("ct", L(cts2[:n], nk.cw)), P("r", shape=(n, nk.nw))
            return (lambda: lib.pai_recover_r(nk.sk, ct.ptr, n, out.ptr, None)), {"r": L(rs[:n], nk.nw)}
        sweep(k, "recover", rec)


def test_fallback_engines_2048(monkeypatch):
    """Handles of the 2048-bit key created with the digit engines left out (PAI_DISABLE=padic,pair, then wide as well): DJN
    encryption, ct * pt (fresh and in place) and decryption on the wide / lane-group kernels that serve every size"""
    lib = _native.load()
    _native.check(lib.pai_profile_enable(1))
    key = orc.make_key(orc.BENCH_P, orc.BENCH_Q, djn_x=(1 << 70) + 12345, bits=2048)
    k = SimpleNamespace(ident="k2048", key=key, consts=orc.crt_constants(key), b=1024)
    monkeypatch.setenv("PAI_LATENCY_MAX", "0")
    N = 70
    m, r = plain(k, N, 11), rand_r(k, N, 12)
    want = djn_encrypt_many(key, m, r)
    e = [0, 1, (1 << 53) - 1, 1 << 52] + [random.Random(5).getrandbits(53) for _ in range(N - 4)]
    want_mul = pow_many(want, e, key.nsq)
    for off in ("padic,pair", "padic,pair,wide"):
        monkeypatch.setenv("PAI_DISABLE", off)
        nk = k.nk = NativeKey(key)
        for n in (1, N):
            def enc(P, n=n):
                dm, dr, ct = P("m", L(m[:n], nk.nw)), P("r", L(r[:n], nk.rw)), P("ct", shape=(n, nk.cw))
                return (lambda: lib.pai_encrypt(nk.pk, dm.ptr, dr.ptr, n, ct.ptr, None)), {"ct": L(want[:n], nk.cw)}
            sweep(k, "encrypt", enc, {"lane_group"})
            for alias in (None, "ct"):
                def mul(P, n=n, alias=alias):
                    dc, de = P("ct", L(want[:n], nk.cw)), P("e", L(e[:n], 2))
                    out = dc if alias else P("out", shape=(n, nk.cw))
                    return (lambda: lib.pai_ct_mul(nk.pk, dc.ptr, de.ptr, 2, 53, 0, n, out.ptr, None)), {alias or "out": L(want_mul[:n], nk.cw)}
                sweep(k, "ct_mul", mul, {"lane_group"})

            def dec(P, n=n):
                ct, out = P("ct", L(want[:n], nk.cw)), P("m", shape=(n, nk.nw))
                return (lambda: lib.pai_decrypt(nk.sk, ct.ptr, n, out.ptr, None)), {"m": L(m[:n], nk.nw)}
            sweep(k, "decrypt", dec, {"wide", "lane_group"} if off == "padic,pair" else {"lane_group"})
        del nk, k.nk
    _native.check(lib.pai_profile_enable(0))


def test_crt_encrypt(mk, monkeypatch):
    """pai_encrypt_crt / pai_obfuscate_crt with the hand-over edge at 0: served where the encryption digit engine takes the primes,
    the public call elsewhere — the same bits either way"""
    k, nk, key = mk, mk.nk, mk.key
    lib = nk.lib
    N = 70
    m, r = plain(k, N, 41), rand_r(k, N, 42)
    want = djn_encrypt_many(key, m, r)
    want2 = djn_obfuscate_many(key, want, r)
    tune(monkeypatch, "crtenc_min", 0)
    for n in (1, N):
        def enc(P, n=n):
            dm, dr, ct = P("m", L(m[:n], nk.nw)), P("r", L(r[:n], nk.rw)), P("ct", shape=(n, nk.cw))
            return (lambda: lib.pai_encrypt_crt(nk.sk, dm.ptr, dr.ptr, n, ct.ptr, None)), {"ct": L(want[:n], nk.cw)}

        def obf(P, n=n):
            dr, ct = P("r", L(r[:n], nk.rw)), P("ct", L(want[:n], nk.cw))
            return (lambda: lib.pai_obfuscate_crt(nk.sk, ct.ptr, dr.ptr, n, None)), {"ct": L(want2[:n], nk.cw)}
        got = sweep(k, "encrypt_crt", enc)
        sweep(k, "encrypt_crt", obf)
    if not any(p.startswith("k_crt_lift") for p in got):
        HANDDOWN.add(f"{k.ident}: pai_encrypt_crt -> the public call ({got})")


def test_opening_fold(mk, monkeypatch):
    """pai_opening_fold: 7 rows in segments of 3 (a ragged last segment), 40-bit coefficients; S rows on each side, the flag word
    stays as the caller zeroed it; both routes"""
    k, nk, key = mk, mk.nk, mk.key
    lib = nk.lib
    n_, M = key.n, key.nsq
    N, seg, ew, eb = 7, 3, 2, 40
    rng = random.Random(7)
    rs = [rng.randrange(1, n_) for _ in range(N)]
    ms = plain(k, N, 51)
    cts = [(1 + m * n_) % M * pow(r, n_, M) % M for m, r in zip(ms, rs)]
    es = [0, 1, (1 << eb) - 1] + [rng.getrandbits(eb) for _ in range(N - 3)]
    lhs, rhs = [], []
    for s in range(0, N, seg):
        a, Ms, Bs = 1, 0, 1
        for i in range(s, min(N, s + seg)):
            a = a * pow(cts[i], es[i], M) % M
            Ms = (Ms + es[i] * ms[i]) % n_
            Bs = Bs * pow(rs[i], es[i], n_) % n_
        lhs.append(a)
        rhs.append((1 + n_ * Ms) % M * pow(Bs, n_, M) % M)
    assert lhs == rhs
    S = len(lhs)
    for off in (False, True):
        knob_disable(monkeypatch, "open_fold", off)

        def build(P):
            ct, dm, dr, de = P("ct", L(cts, nk.cw)), P("m", L(ms, nk.nw)), P("r", L(rs, nk.nw)), P("e", L(es, ew))
            dl, dh, fl = P("lhs", shape=(S, nk.cw)), P("rhs", shape=(S, nk.cw)), P("flag", np.zeros(1, np.int32))
            return (lambda: lib.pai_opening_fold(nk.pk, ct.ptr, dm.ptr, dr.ptr, N, de.ptr, ew, eb, seg, dl.ptr, dh.ptr, fl.ptr, None)), \
                {"lhs": L(lhs, nk.cw), "rhs": L(rhs, nk.cw)}
        sweep(k, "opening_fold", build)


# ---- ciphertext arithmetic --------------------------------------------------------------------------------------------------------
def add_operands(k, n):
    key = k.key
    a, b = ciphertexts(k, n, 7), list(reversed(ciphertexts(k, max(n, 10), 8)))[:n]
    if n > 6:
        b[1], b[3], b[6] = key.nsq - 1, key.n + 1, key.nsq - 1
    return a, b


def test_ct_add_family(mk, monkeypatch):
    """pai_ct_add (most-significant-limb-first product and Montgomery products), pai_ct_mont_mul, pai_ct_add_aligned / _host / _dom,
    pai_ct_pow2 / _hint and pai_ct_add_plain on lane groups and on the latency geometry; the output fresh, exactly d_a, and exactly
    d_b; a broadcast addend with a fresh output and, at N = 1, as the output"""
    k, nk, key = mk, mk.nk, mk.key
    lib = nk.lib
    M, W = key.nsq, nk.cw
    Ri = pow(k.R, -1, M)
    has_msb = None
    for lat_add, geo in (("0", "lane_group"), ("4096", "lat")):
        monkeypatch.setenv("PAI_LAT_ADD_MAX", lat_add)
        for n in sizes(k):
            a, b = add_operands(k, n)
            rng = np.random.default_rng(n)
            delta = rng.integers(-3, 9, n).astype(np.int32)
            delta[:6] = [0, 1, -3, 8, -1, 7][:n]
            prod = [x * y % M for x, y in zip(a, b)]
            prod_b = [x * b[0] % M for x in a]
            want_al = [x * pow(y, 1 << int(d), M) % M if d > 0 else pow(x, 1 << int(-d), M) * y % M for x, y, d in zip(a, b, delta)]
            want_alb = [x * pow(b[0], 1 << int(d), M) % M if d > 0 else pow(x, 1 << int(-d), M) * b[0] % M for x, d in zip(a, delta)]
            want_p2 = [pow(x, 1 << int(d), M) if d > 0 else x for x, d in zip(a, delta)]
            mpl = plain(k, n, 9)
            want_pl = [x * (1 + m * key.n) % M for x, m in zip(a, mpl)]

            def binary(fn, want, alias, bcast=0, extra=None):
                def build(P):
                    da = P("a", L(a, W))
                    db = P("b", L(b[:1] if bcast else b, W))
                    out = {"a": da, "b": db}.get(alias) or P("out", shape=(n, W))
                    ex = extra(P) if extra else ()
                    return (lambda: fn(da, db, bcast, out, *ex)), {alias or "out": L(want, W)}
                return build
            forms = [(None, 0), ("a", 0), ("b", 0), (None, 1), ("a", 1)] + ([("b", 1)] if n == 1 else [])
            for no_msb in (False, True):
                knob_disable(monkeypatch, "add_msb", no_msb)
                for alias, bc in forms:
                    got = sweep(k, "ct_add", binary(lambda da, db, bc_, out: lib.pai_ct_add(nk.pk, da.ptr, db.ptr, bc_, n, out.ptr, None),
                                                    prod_b if bc else prod, alias, bc))
                    if geo == "lane_group" and not no_msb and not bc and n > 1:
                        has_msb = got == ["k_modmul_msb:lane_group"]
                    assert got[0].split(":")[1].startswith(geo), (k.ident, got)
            knob_disable(monkeypatch, "add_msb", False)
            for alias, bc in forms:
                sweep(k, "ct_add", binary(lambda da, db, bc_, out: lib.pai_ct_mont_mul(nk.pk, da.ptr, db.ptr, bc_, n, out.ptr, None),
                                          [x * Ri % M for x in (prod_b if bc else prod)], alias, bc), {geo})
                sweep(k, "ct_add", binary(lambda da, db, bc_, out, dd: lib.pai_ct_add_aligned(nk.pk, da.ptr, db.ptr, bc_, dd.ptr, n, out.ptr, None),
                                          want_alb if bc else want_al, alias, bc, lambda P: (P("delta", delta),)))
            hd = np.ascontiguousarray(delta)
            sweep(k, "ct_add", binary(lambda da, db, bc_, out: lib.pai_ct_add_aligned_host(nk.pk, da.ptr, db.ptr, bc_, host_ptr(hd), n, out.ptr, None),
                                      want_al, "b"))
            # buffers that share the tag 1: the entry constant R^(2 - 1) = R, the result at tag 1
            t1 = lambda v: [x * k.R % M for x in v]

            def dom(P):
                da, db, dd, de, out = P("a", L(t1(a), W)), P("b", L(t1(b), W)), P("delta", delta), P("entry", L([k.R], W)), P("out", shape=(n, W))
                return (lambda: lib.pai_ct_add_aligned_dom(nk.pk, da.ptr, db.ptr, 0, dd.ptr, n, out.ptr, de.ptr, None)), {"out": L(t1(want_al), W)}
            sweep(k, "ct_add", dom)
            for hint in (False, True):
                def p2(P):
                    dc, dd = P("ct", L(a, W)), P("delta", delta)
                    if hint:
                        return (lambda: lib.pai_ct_pow2_hint(nk.pk, dc.ptr, dd.ptr, 0, n, 8, None)), {"ct": L(want_p2, W)}
                    return (lambda: lib.pai_ct_pow2(nk.pk, dc.ptr, dd.ptr, 0, n, None)), {"ct": L(want_p2, W)}
                sweep(k, "ct_add", p2, {geo})
            for alias in (None, "ct"):
                def pl(P):
                    dc, dm = P("ct", L(a, W)), P("m", L(mpl, nk.nw))
                    out = dc if alias else P("out", shape=(n, W))
                    return (lambda: lib.pai_ct_add_plain(nk.pk, dc.ptr, dm.ptr, n, out.ptr, None)), {alias or "out": L(want_pl, W)}
                sweep(k, "add_plain", pl)
    if k.thr == "padic":
        # pai_ct_pow2 / _hint on the digit engine (PAI_POW2_DIGIT_MIN; a largest shift of 8 .. 62): k_pow2_expo writes the one-bit exponents
        # to the handle's scratch, k_ctmul_padic runs in place on d_ct — 257 rows: one full and one ragged 256-element tile
        knobs_default(monkeypatch)
        monkeypatch.setenv("PAI_POW2_DIGIT_MIN", "1")
        n = 257
        a = ciphertexts(k, n, 7)
        delta = np.random.default_rng(n).integers(-3, 9, n).astype(np.int32)
        delta[:6] = [0, 1, -3, 8, -1, 7]
        want_p2 = pow_many(a, [1 << int(d) if d > 0 else 1 for d in delta], M)
        for hint in (False, True):
            def p2d(P):
                dc, dd = P("ct", L(a, W)), P("delta", delta)
                if hint:
                    return (lambda: lib.pai_ct_pow2_hint(nk.pk, dc.ptr, dd.ptr, 0, n, 8, None)), {"ct": L(want_p2, W)}
                return (lambda: lib.pai_ct_pow2(nk.pk, dc.ptr, dd.ptr, 0, n, None)), {"ct": L(want_p2, W)}
            sweep(k, "ct_add", p2d, {"padic"})
        monkeypatch.delenv("PAI_POW2_DIGIT_MIN")
    else:
        HANDDOWN.add(f"{k.ident}: pai_ct_pow2 has no digit-engine path (n not served by the digit engine): k_pow2 on lane groups / latency geometry")
    if not has_msb:
        HANDDOWN.add(f"{k.ident}: pai_ct_add without the most-significant-limb-first product (no msb context): k_modmul serves")


def test_ct_addn_aliasing(mk):
    """pai_ct_addn with 5 operands: the output fresh and exactly the first, a middle and the last operand, with and without raises"""
    k, nk, key = mk, mk.nk, mk.key
    lib = nk.lib
    M, W, K = key.nsq, nk.cw, 5
    for n in sizes(k):
        ops = [ciphertexts(k, n, 60 + j, units=True) for j in range(K)]
        rng = np.random.default_rng(3)
        raises = [None, rng.integers(0, 4, n).astype(np.int32), None, rng.integers(0, 3, n).astype(np.int32), None]
        for with_raise in (False, True):
            want = []
            for i in range(n):
                acc = 1
                for j in range(K):
                    s = int(raises[j][i]) if with_raise and raises[j] is not None else 0
                    acc = acc * pow(ops[j][i], 1 << s, M) % M
                want.append(acc)
            for alias in (None, 0, 2, 4):
                def build(P):
                    regs = [P(f"op{j}", L(ops[j], W)) for j in range(K)]
                    rz = [P(f"raise{j}", raises[j]) if with_raise and raises[j] is not None else None for j in range(K)]
                    out = regs[alias] if alias is not None else P("out", shape=(n, W))

                    def call():                              # the pointers exist once the arena is committed
                        hp = (C.c_void_p * K)(*[r.ptr for r in regs])
                        hr = (C.c_void_p * K)(*[r.ptr if r is not None else None for r in rz])
                        return lib.pai_ct_addn(nk.pk, hp, hr if with_raise else None, K, 0, 0, 0, n, out.ptr, None)
                    return call, {out.name: L(want, W)}
                sweep(k, "aggregate", build)


@pytest.mark.parametrize("part", ["throughput", "small_batch"])
def test_ct_mul(mk, part, monkeypatch):
    """pai_ct_mul / pai_ct_mul_host with 53-bit exponents, one full-width batch and (once per key) 7-bit exponents on every path of
    the dispatcher, per element and broadcast (the full-width batch: per element), into a fresh output and in place"""
    k, nk, key = mk, mk.nk, mk.key
    lib = nk.lib
    M, W = key.nsq, nk.cw
    nb = 2 * k.b
    cfgs = [("0", None, None, False, False, {k.thr})]
    if k.thr == "pair":
        cfgs.append(("0", None, None, True, False, {"lane_group"}))
    cfgs += [("100000", "100000", "100000", False, False, {"pp", "rl", "window"}), ("100000", "0", "100000", False, False, {"rl", "window"}),
             ("100000", "0", "0", False, False, {"window"})]
    if nb <= 2068:
        cfgs.append(("100000", None, None, False, True, {"pair4"} if k.ident == "k2048" else None))
    wants = {}
    cfgs = [c for c in cfgs if (c[0] == "0") == (part == "throughput")]
    for ci, (switch, pp, rl, no_pair, mid, allowed) in enumerate(cfgs):
        first = part == "throughput" and ci == 0             # the key's own throughput engine
        monkeypatch.setenv("PAI_LATENCY_MAX", switch)
        tune(monkeypatch, "lat_mul_pp", pp)
        tune(monkeypatch, "lat_mul_rl", rl)
        knob_disable(monkeypatch, "pair_ctmul", no_pair)
        tune(monkeypatch, "ctmul_mid_min", 0 if mid else None)
        tune(monkeypatch, "ctmul_mid_max", 1 << 30 if mid else None)
        for n in sizes(k, first):
            c = ciphertexts(k, n, 5)
            # 53 bits everywhere; one full-width batch on every path (the four-wave kernel takes short exponents only: the dispatcher
            # hands a wide one down, which `allowed` admits); 7 bits once per key: at 8 bits and below the dispatcher skips the latency
            # and window kernels, and where the digit engine does not serve n it launches k_modexp_var, which has no timer
            for ebits in (53,) + ((nb,) if n > 1 else ()) + ((7,) if first else ()):
                # a full-width batch on the small-batch kernels (one integer per wavefront or per workgroup): 5 rows, more than one workgroup
                m_ = 5 if ebits == nb and switch != "0" and not mid else n
                cc = c[:m_]
                rng = random.Random(ebits)
                e = ([0, 1, (1 << ebits) - 1, 1 << (ebits - 1)] + [rng.getrandbits(ebits) for _ in range(m_)])[:m_]
                if m_ == 1:
                    e = [(1 << ebits) - 1]
                ew = (ebits + 31) // 32
                if (m_, ebits) not in wants:                 # the reference once per shape, shared by every path
                    wants[(m_, ebits)] = (pow_many(cc, e, M), pow_many(cc, e[-1], M))
                want, want_b = wants[(m_, ebits)]
                for bcast, alias in ((0, None), (0, "ct")) + (((1, None), (1, "ct")) if ebits != nb else ()):
                    def build(P):
                        dc, de = P("ct", L(cc, W)), P("e", L(e[-1:] if bcast else e, ew))
                        out = dc if alias else P("out", shape=(m_, W))
                        return (lambda: lib.pai_ct_mul(nk.pk, dc.ptr, de.ptr, ew, ebits, bcast, m_, out.ptr, None)), \
                            {alias or "out": L(want_b if bcast else want, W)}
                    if ebits == 7:
                        sweep(k, "ct_mul" if k.thr == "padic" else "ct_mul_untimed", build, {"padic"} if k.thr == "padic" else None)
                    else:
                        got = sweep(k, "ct_mul", build, allowed)
                if ebits != 53:
                    continue
                if allowed is None and got[0] != "k_ctmul:pair4":
                    HANDDOWN.add(f"{k.ident}: pai_ct_mul pair4 -> {got[0].split(':')[1]}")
                if allowed is not None and len(allowed) > 1:
                    asked = "pp" if pp != "0" else "rl"
                    if got[0].split(":")[1] != asked:
                        HANDDOWN.add(f"{k.ident}: pai_ct_mul {asked} -> {got[0].split(':')[1]}")
                if m_ * ew * 4 <= 4096:
                    he = L(e, ew)

                    def host(P):
                        dc = P("ct", L(cc, W))
                        return (lambda: lib.pai_ct_mul_host(nk.pk, dc.ptr, host_ptr(he), ew, ebits, 0, m_, dc.ptr, None)), {"ct": L(want, W)}
                    sweep(k, "ct_mul", host, allowed)


def test_invert_prod_multiexp(mk, monkeypatch):
    """pai_ct_invert / _async / _flag (one level, and a tree forced with invert_chunk), fresh and in place; pai_ct_prod in 1 and 7
    groups; pai_ct_multiexp with and without signs"""
    k, nk, key = mk, mk.nk, mk.key
    lib = nk.lib
    M, W = key.nsq, nk.cw
    u = ciphertexts(k, 70, 9, units=True)
    inv = [pow(x, -1, M) for x in u]
    for chunk in (None, 8):
        tune(monkeypatch, "invert_chunk", chunk)
        for n in (1, 70):
            for alias in (None, "ct"):
                for form in ("sync", "async", "flag"):
                    def build(P):
                        dc = P("ct", L(u[:n], W))
                        out = dc if alias else P("out", shape=(n, W))
                        ex = {alias or "out": L(inv[:n], W)}
                        if form == "flag":
                            fl = P("flag", np.zeros(1, np.int32))
                            return (lambda: lib.pai_ct_invert_flag(nk.pk, dc.ptr, n, out.ptr, fl.ptr, None)), ex
                        fn = lib.pai_ct_invert if form == "sync" else lib.pai_ct_invert_async
                        return (lambda: fn(nk.pk, dc.ptr, n, out.ptr, None)), ex
                    sweep(k, "aggregate", build)
    tune(monkeypatch, "invert_chunk", None)
    st = C.c_int(-1)
    _native.check(lib.pai_pubkey_status(nk.pk, C.byref(st), 1, None))
    assert st.value & 1 == 0
    a = ciphertexts(k, 70, 10, units=True)
    for groups in (1, 7):
        want = []
        for g in range(groups):
            acc = 1
            for l in range(70 // groups):
                acc = acc * a[l * groups + g] % M
            want.append(acc)

        def prod(P):
            dc, out = P("ct", L(a, W)), P("out", shape=(groups, W))
            return (lambda: lib.pai_ct_prod(nk.pk, dc.ptr, 70, groups, out.ptr, None)), {"out": L(want, W)}
        sweep(k, "aggregate", prod)
    R_, K_, Mc, ew = 2, 5, 3, 2
    base = u[3:3 + R_ * K_]
    binv = [pow(x, -1, M) for x in base]
    rng = random.Random(k.b)
    e = [[[rng.getrandbits(53) for _ in range(Mc)] for _ in range(K_)] for _ in range(R_)]
    e[0][0][0], e[0][1][0], e[1][0][1], e[1][1][1] = 0, 1, (1 << 53) - 1, 1 << 52
    sign = np.array([[(l + j) % 2 for j in range(Mc)] for l in range(K_)], dtype=np.uint8)
    e_l = np.array([[[[e[r][l][j] & 0xFFFFFFFF, e[r][l][j] >> 32] for j in range(Mc)] for l in range(K_)] for r in range(R_)], dtype=np.uint32)
    for signed in (True, False):
        want = []
        for r in range(R_):
            for j in range(Mc):
                acc = 1
                for l in range(K_):
                    acc = acc * pow(binv[r * K_ + l] if signed and sign[l, j] else base[r * K_ + l], e[r][l][j], M) % M
                want.append(acc)

        def mexp(P):
            dc, de, out = P("ct", L(base, W)), P("e", e_l.reshape(-1, ew)), P("out", shape=(R_ * Mc, W))
            di, ds = (P("inv", L(binv, W)), P("sign", sign.reshape(-1))) if signed else (None, None)
            return (lambda: lib.pai_ct_multiexp(nk.pk, dc.ptr, di.ptr if di else None, R_, K_, Mc, de.ptr, ew, 53, ds.ptr if ds else None,
                                                out.ptr, None)), {"out": L(want, W)}
        sweep(k, "multiexp", mexp)


def test_segment_scan_sparse_pack(mk, monkeypatch):
    """pai_ct_segment_prod (an empty and a one-member segment, gathered rows, shifts), pai_ct_scan (both directions, runs of 5),
    pai_ct_sparse_multiexp (an empty segment, signs), pai_ct_pack and pai_ct_pack_step with a ragged last group, on the chain
    levels and, where the digit engine serves the key, one chain per lane"""
    k, nk, key = mk, mk.nk, mk.key
    lib = nk.lib
    M, W = key.nsq, nk.cw
    N = 70
    cts = ciphertexts(k, N, 70, units=True)
    rng = np.random.default_rng(11)
    offs = np.array([0, 0, 1, 3, 20, 70, 75], dtype=np.int64)                   # empty, one member, 2, 17, 50, 5 (gather with repeats)
    rows = np.concatenate([np.arange(N), rng.integers(0, N, 5)]).astype(np.uint32)
    shift = rng.integers(0, 4, len(rows)).astype(np.int32)
    S = len(offs) - 1
    want = want_segprod(cts, rows, shift, offs, M)
    tagged = [c * k.R % M for c in cts]                                         # the same rows at domain tag 1: the same outputs
    for chunk, tag in ((None, 0), (3, 0), (None, 1), (3, 1)):
        tune(monkeypatch, "segprod_chunk", chunk)

        def seg(P):
            dc, dr, ds, do, out = P("ct", L(tagged if tag else cts, W)), P("rows", rows), P("shift", shift), P("offsets", offs), P("out", shape=(S, W))
            return (lambda: lib.pai_ct_segment_prod(nk.pk, dc.ptr, N, tag, dr.ptr, ds.ptr, do.ptr, S, out.ptr, None)), {"out": L(want, W)}
        sweep(k, "aggregate", seg)
    tune(monkeypatch, "segprod_chunk", None)
    raise_, step = rng.integers(0, 3, N).astype(np.int32), rng.integers(0, 3, N).astype(np.int32)
    for reverse in (0, 1):
        want_s = want_chain(cts, raise_, step, 5, bool(reverse), M)
        for chunk, tag in ((None, 0), (2, 0), (2, 1)):
            tune(monkeypatch, "scan_chunk", chunk)

            def scan(P):
                dc, dr, ds, out = P("ct", L(tagged if tag else cts, W)), P("raise", raise_), P("step", step), P("out", shape=(N, W))
                return (lambda: lib.pai_ct_scan(nk.pk, dc.ptr, N, tag, 0, 5, reverse, dr.ptr, ds.ptr, out.ptr, None)), {"out": L(want_s, W)}
            sweep(k, "aggregate", scan)
    tune(monkeypatch, "scan_chunk", None)
    # sparse: 12 bases, 30 terms in 5 segments (the second empty, the third of one term)
    NB, T_ = 12, 30
    sb = cts[:NB]
    sinv = [pow(x, -1, M) for x in sb]
    tb = rng.integers(0, NB, T_).astype(np.int32)
    te = [int(x) for x in rng.integers(0, 1 << 53, T_)]
    te[0], te[1] = 0, (1 << 53) - 1
    tsg = rng.integers(0, 2, T_).astype(np.uint8)
    soff = np.array([0, 4, 4, 5, 17, 30], dtype=np.int64)
    want_sp = []
    for s in range(len(soff) - 1):
        acc = 1
        for t in range(int(soff[s]), int(soff[s + 1])):
            acc = acc * pow(sinv[tb[t]] if tsg[t] else sb[tb[t]], te[t], M) % M
        want_sp.append(acc)
    for no_padic_chunk in (None, 4):
        tune(monkeypatch, "smexp_chunk", no_padic_chunk)

        def sparse(P):
            dc, di, db, de, ds, do = P("ct", L(sb, W)), P("inv", L(sinv, W)), P("base", tb), P("e", L(te, 2)), P("sign", tsg), P("offsets", soff)
            out = P("out", shape=(len(soff) - 1, W))
            return (lambda: lib.pai_ct_sparse_multiexp(nk.pk, dc.ptr, di.ptr, NB, db.ptr, de.ptr, 2, 53, ds.ptr, T_, do.ptr, len(soff) - 1,
                                                       out.ptr, None)), {"out": L(want_sp, W)}
        sweep(k, "sparse", sparse)
    tune(monkeypatch, "smexp_chunk", None)
    # packing: 16-bit slots, 3 per row: 70 rows -> 24 output rows, the last of one member; repacking in steps of 48 bits, 4 per row
    nbits = key.n.bit_length()
    for disable_padic in (True, False):
        knob_disable(monkeypatch, "pack_padic", disable_padic)
        tune(monkeypatch, "pack_padic_min", None if disable_padic else 0)
        # one chain per lane on the digit engine: 258 output rows, one full and one ragged 256-lane tile (772 = 3 * 257 + 1, 1029 = 4 * 257 + 1)
        big = not disable_padic and k.thr == "padic"
        for step_bits, count, fn, tag in ((16, 3, "pack", 0), (48, 4, "step", 0)) + (((16, 3, "pack", 1), (48, 4, "step", 1)) if disable_padic else ()):
            assert step_bits * count <= nbits - 2
            Np = (772 if count == 3 else 1029) if big else N
            pool = ciphertexts(k, Np, 70, units=True) if big else cts
            want_p = want_stepped(pool, step_bits, count, M)
            G = len(want_p)
            assert Np % count != 0 and G == -(-Np // count) and (G == 258 or not big)
            rows_in = [c * k.R % M for c in pool] if tag else pool

            def pack(P):
                dc, out = P("ct", L(rows_in, W)), P("out", shape=(G, W))
                f = lib.pai_ct_pack if fn == "pack" else lib.pai_ct_pack_step
                return (lambda: f(nk.pk, dc.ptr, Np, tag, step_bits, count, out.ptr, None)), {"out": L(want_p, W)}
            got = sweep(k, "pack", pack, {""} if big else None)
            assert not big or "k_ct_pack_padic:" in got, (k.ident, got)
            if not disable_padic and "k_ct_pack_padic:" not in got:
                HANDDOWN.add(f"{k.ident}: pai_ct_pack above the hand-over -> the k_segprod levels (n not served by the digit engine)")


# ---- codec ------------------------------------------------------------------------------------------------------------------------
def test_codec(mk):
    """pai_fp_encode_f64 / _i64 / _at, pai_fp_decode_i64, pai_fp_pack, pai_fp_unpack (16-bit and 80-bit slots) on 257 elements: one
    full and one ragged 256-element workgroup; grouped outputs with a ragged last row"""
    k, nk, key = mk, mk.nk, mk.key
    lib = nk.lib
    n_, nw = key.n, nk.nw
    max_int = n_ // 3 - 1
    rng = np.random.default_rng(5)
    for N in (1, 257):
        xf = rng.uniform(-1e6, 1e6, N)
        xf[0] = -0.75
        xi = rng.integers(-(1 << 62), 1 << 62, N).astype(np.int64)
        xi[0] = -1
        for x, fn in ((xf, lib.pai_fp_encode_f64), (xi, lib.pai_fp_encode_i64)):
            enc = [orc.fp_encode(float(v) if x.dtype.kind == "f" else int(v), n_, max_int) for v in x]

            def build(P):
                dx, dm, de = P("x", x), P("m", shape=(N, nw)), P("expo", shape=(N,), dtype=np.int32)
                return (lambda: fn(nk.pk, dx.ptr, N, dm.ptr, de.ptr, None)), \
                    {"m": L([e[0] for e in enc], nw), "expo": np.array([e[1] for e in enc], dtype=np.int32)}
            sweep(k, "codec", build)
        tg = np.array([0, 5, 40][:N] + [int(v) for v in rng.integers(0, 41, max(0, N - 3))], dtype=np.int32)
        for bc in (0, 1):
            t_of = (lambda i: int(tg[0 if bc else i]))
            want_r = [(int(v) << t_of(i)) % n_ for i, v in enumerate(xi)]
            want_e = np.array([t_of(i) for i in range(N)], dtype=np.int32)

            def at(P):
                dx, dt, dm, de = P("x", xi), P("target", tg[:1] if bc else tg), P("m", shape=(N, nw)), P("expo", shape=(N,), dtype=np.int32)
                return (lambda: lib.pai_fp_encode_at(nk.pk, dx.ptr, 0, N, dt.ptr, bc, dm.ptr, de.ptr, None)), {"m": L(want_r, nw), "expo": want_e}
            sweep(k, "codec", at)
        # doubles: the oracle's encodings brought to their targets by the host codec's rule (fixedpoint.align_encoded, as
        # tests/test_gpu_codec_keys.py::test_encode_at): targets 3 below to 40 above each element's own exponent
        encf = [orc.fp_encode(float(v), n_, max_int) for v in xf]
        ef = np.array([e[1] for e in encf], dtype=np.int32)
        tgf = (ef + rng.integers(-3, 41, N)).astype(np.int32)
        for bc in (0, 1):
            tt = np.full(N, tgf[0], dtype=np.int32) if bc else tgf
            wr, we = fixedpoint.align_encoded(L([e[0] for e in encf], nw), ef, tt, n_, max_int)

            def atf(P):
                dx, dt, dm, de = P("x", xf), P("target", tt[:1] if bc else tt), P("m", shape=(N, nw)), P("expo", shape=(N,), dtype=np.int32)
                return (lambda: lib.pai_fp_encode_at(nk.pk, dx.ptr, 1, N, dt.ptr, bc, dm.ptr, de.ptr, None)), \
                    {"m": np.ascontiguousarray(wr, dtype=np.uint32), "expo": np.asarray(we, dtype=np.int32)}
            sweep(k, "codec", atf)
        mant = [int(v) for v in xi]

        def dec(P):
            dm, do, df = P("m", L([v % n_ for v in mant], nw)), P("mant", shape=(N,), dtype=np.int64), P("flag", shape=(N,), dtype=np.int32)
            return (lambda: lib.pai_fp_decode_i64(nk.pk, dm.ptr, N, do.ptr, df.ptr, None)), \
                {"mant": np.array(mant, dtype=np.int64), "flag": np.zeros(N, np.int32)}
        sweep(k, "codec", dec)
        for b, slots in ((16, 3), (80, 2)):
            v = 14
            ms = [int(x) for x in rng.integers(-(1 << v) + 1, 1 << v, N)]
            rows = model_pack(ms, b, slots, n_)
            G = len(rows)
            xs = np.array(ms, dtype=np.int64)

            for is_f64 in (0, 1):                            # integer-valued doubles: rint(x 2^0) is the same mantissa
                def pack(P, is_f64=is_f64):
                    dx, dm, fl = P("x", xs.astype(np.float64) if is_f64 else xs), P("m", shape=(G, nw)), P("flag", np.zeros(1, np.int32))
                    return (lambda: lib.pai_fp_pack(nk.pk, dx.ptr, is_f64, N, 0, v, b, slots, dm.ptr, fl.ptr, None)), {"m": L(rows, nw)}
                sweep(k, "codec", pack)
            full = ms + [0] * (G * slots - N)
            if b <= 64:
                want_u = np.array(full, dtype=np.int64)
            else:
                want_u = np.array([[x & ((1 << 64) - 1), x >> 64] for x in full], dtype=object)
                want_u = np.array([[int(lo) - (1 << 64) if lo >= 1 << 63 else int(lo), int(hi)] for lo, hi in want_u], dtype=np.int64)

            def unpack(P):
                dm, do, df = P("m", L(rows, nw)), P("out", shape=want_u.shape, dtype=np.int64), P("flag", shape=(G,), dtype=np.int32)
                return (lambda: lib.pai_fp_unpack(nk.pk, dm.ptr, G, b, slots, do.ptr, df.ptr, None)), {"out": want_u, "flag": np.zeros(G, np.int32)}
            sweep(k, "codec", unpack)


def test_quantize(mk):
    """pai_fp_quantize: column sums of a [67][5] matrix at unit and non-unit strides (the X and X.T views), segment sums of a [67]
    vector with an empty segment; words of 1, 2 and 4 per weight — the 8-byte and 16-byte stores and their word-wise fallback"""
    k, nk = mk, mk.nk
    lib = nk.lib
    rng = np.random.default_rng(9)
    K_, M_ = 67, 5
    for ew, wb in ((1, 20), (2, 40), (4, 40)):
        x = rng.integers(-(1 << wb) + 1, 1 << wb, (K_, M_)).astype(np.int64)
        x[:, 2] = 0
        words, sign, sums = quantize_model(x, 0, ew)
        want_sum = np.array([[s & ((1 << 64) - 1), s >> 64] for s in sums], dtype=np.uint64)
        for transposed, is_f64 in ((False, 0), (True, 0), (False, 1), (True, 1)):    # doubles: integer-valued, the same weights
            xs = np.ascontiguousarray(x.T) if transposed else x
            xs = xs.astype(np.float64) if is_f64 else xs
            sk, sm = (1, K_) if transposed else (M_, 1)

            def col(P):
                dx, de, ds = P("x", xs), P("e", shape=(K_ * M_, ew)), P("sign", shape=(K_ * M_,), dtype=np.uint8)
                du, fl = P("sum", shape=(M_, 2), dtype=np.uint64), P("flag", np.zeros(1, np.int32))
                return (lambda: lib.pai_fp_quantize(nk.pk, dx.ptr, is_f64, K_, M_, sk, sm, 0, wb, None, 0, de.ptr, ew, ds.ptr, du.ptr, fl.ptr, None)), \
                    {"e": words.reshape(K_ * M_, ew), "sign": sign.reshape(-1), "sum": want_sum}
            sweep(k, "quantize", col)
        v = np.ascontiguousarray(x[:, 0])
        offs = np.array([0, 0, 10, 11, 60], dtype=np.int64)
        words1, sign1, sums1 = quantize_model(v, 0, ew, offsets=offs.tolist())
        want1 = np.array([[s & ((1 << 64) - 1), s >> 64] for s in sums1], dtype=np.uint64)

        def segs(P):
            dx, do, de, ds = P("x", v), P("offsets", offs), P("e", shape=(K_, ew)), P("sign", shape=(K_,), dtype=np.uint8)
            du, fl = P("sum", shape=(len(offs) - 1, 2), dtype=np.uint64), P("flag", np.zeros(1, np.int32))
            return (lambda: lib.pai_fp_quantize(nk.pk, dx.ptr, 0, K_, 1, 1, 1, 0, wb, do.ptr, len(offs) - 1, de.ptr, ew, ds.ptr, du.ptr, fl.ptr,
                                                None)), {"e": words1.reshape(K_, ew), "sign": sign1.reshape(-1), "sum": want1}
        sweep(k, "quantize", segs)


# ---- buffers, randomness, generic arithmetic ----------------------------------------------------------------------------------------
def test_draw_r_and_buffers(mk):
    """pai_draw_r against RFC 8439's block function; pai_buf_slice (steps 1 and 3), pai_buf_rotate (both signs); pai_gather and
    pai_scatter with three shards on device 0"""
    k, nk, key = mk, mk.nk, mk.key
    lib = nk.lib
    rw, W = nk.rw, nk.cw
    key8 = np.arange(1, 9, dtype=np.uint32) * 0x01020305
    nonce = np.array([7, 8, 9], dtype=np.uint32)
    for N in (1, 70):
        total = N * rw
        stream = []
        for blk in range((total + 15) // 16):
            stream += chacha_block([int(v) for v in key8], (5 + blk) & 0xFFFFFFFF, [int(v) for v in nonce])
        want = np.array(stream[:total], dtype=np.uint32).reshape(N, rw)
        top_word, top = (key.randbits - 1) // 32, key.randbits - 32 * ((key.randbits - 1) // 32)
        want[:, top_word] &= 0xFFFFFFFF if top >= 32 else (1 << top) - 1
        want[:, top_word + 1:] = 0

        def draw(P):
            dr = P("r", shape=(N, rw))
            return (lambda: lib.pai_draw_r(nk.pk, host_ptr(key8), host_ptr(nonce), 5, N, dr.ptr, None)), {"r": want}
        sweep(k, "buffers", draw)
    N = 70
    src = L(ciphertexts(k, N, 90), W)
    for start, count, step in ((0, N, 1), (3, 22, 3), (69, 1, 1)):
        def sl(P):
            ds, out = P("src", src), P("out", shape=(count, W))
            return (lambda: lib.pai_buf_slice(0, ds.ptr, W, start, count, step, out.ptr, None)), {"out": src[start:start + count * step:step]}
        sweep(k, "buffers", sl)
    for sh in (0, 1, -3, 75):
        def rot(P):
            ds, out = P("src", src), P("out", shape=(N, W))
            return (lambda: lib.pai_buf_rotate(0, ds.ptr, W, N, sh, out.ptr, None)), {"out": np.roll(src, -sh, axis=0)}
        sweep(k, "buffers", rot)
    cnt = [30, 0, 40]
    devs = (C.c_int32 * 3)(0, 0, 0)
    rows = (C.c_size_t * 3)(*cnt)
    parts = [src[:30], src[:0], src[30:]]

    def gather(P):
        regs = [P(f"shard{i}", parts[i]) if cnt[i] else None for i in range(3)]
        out = P("out", shape=(N, W))
        return (lambda: lib.pai_gather(3, devs, (C.c_void_p * 3)(*[r.ptr if r else None for r in regs]), rows, W, 0, out.ptr)), {"out": src}
    sweep(k, "buffers", gather)

    def scatter(P):
        regs = [P(f"shard{i}", shape=(cnt[i], W)) if cnt[i] else None for i in range(3)]
        din = P("in", src)
        return (lambda: lib.pai_scatter(3, devs, (C.c_void_p * 3)(*[r.ptr if r else None for r in regs]), rows, W, 0, din.ptr)), \
            {"shard0": parts[0], "shard2": parts[2]}
    sweep(k, "buffers", scatter)


@pytest.mark.parametrize("which", ["m2048", "m521"])
def test_generic_modular_arithmetic(which):
    """pai_modmul (fresh, exactly d_a, exactly d_b, broadcast), pai_modexp_fixed and pai_modexp_var on one modulus of 2048 bits (rows of
    64 words) and one of 521 bits (rows of 17 words: every second row is off the 16-byte grid even in an aligned batch)"""
    lib = _native.load()
    _native.check(lib.pai_profile_enable(1))
    Mod = orc.BENCH_P * orc.BENCH_Q if which == "m2048" else next(e for e in load_limit_keys() if e[0] == "hi-nl36")[5] * \
        next(e for e in load_limit_keys() if e[0] == "hi-nl36")[6]
    W = (Mod.bit_length() + 31) // 32
    h = C.c_void_p()
    _native.check(lib.pai_modulus_create(host_ptr(L([Mod], W)), W, 0, C.byref(h)))
    K = SimpleNamespace(ident=which, nk=SimpleNamespace(lib=lib))                   # what sweep() needs of a key
    try:
        rng = random.Random(3)
        for n in (1, 257 if which == "m521" else 70):
            a = ([0, 1, Mod - 1] + [rng.randrange(Mod) for _ in range(n)])[:n]
            b = ([Mod - 1, Mod - 1, Mod - 1] + [rng.randrange(Mod) for _ in range(n)])[:n]
            for alias, bc in [(None, 0), ("a", 0), ("b", 0), (None, 1)] + ([("b", 1)] if n == 1 else []):
                want = [x * (b[0] if bc else y) % Mod for x, y in zip(a, b)]

                def mm(P):
                    da, db = P("a", L(a, W)), P("b", L(b[:1] if bc else b, W))
                    out = {"a": da, "b": db}.get(alias) or P("out", shape=(n, W))
                    return (lambda: lib.pai_modmul(h, da.ptr, db.ptr, bc, n, out.ptr, None)), {alias or "out": L(want, W)}
                sweep(K, "modarith", mm)
            ef = (1 << 53) - 3
            he = L([ef], 2)

            def fixed(P):
                da, out = P("base", L(a, W)), P("out", shape=(n, W))
                return (lambda: lib.pai_modexp_fixed(h, da.ptr, host_ptr(he), 2, n, out.ptr, None)), {"out": L(pow_many(a, ef, Mod), W)}
            sweep(K, "modarith", fixed)
            for ebits in (7, 53) + ((Mod.bit_length(),) if n > 1 else ()):
                e = ([0, 1, (1 << ebits) - 1] + [rng.getrandbits(ebits) for _ in range(n)])[:n]
                ew = (ebits + 31) // 32

                def var(P):
                    da, de, out = P("base", L(a, W)), P("e", L(e, ew)), P("out", shape=(n, W))
                    return (lambda: lib.pai_modexp_var(h, da.ptr, 0, de.ptr, ew, ebits, 0, n, out.ptr, None)), {"out": L(pow_many(a, e, Mod), W)}
                sweep(K, "modarith", var)
                if ebits == 53:
                    def var_bb(P):                                   # one base for every exponent
                        da, de, out = P("base", L(a[-1:], W)), P("e", L(e, ew)), P("out", shape=(n, W))
                        return (lambda: lib.pai_modexp_var(h, da.ptr, 1, de.ptr, ew, ebits, 0, n, out.ptr, None)), \
                            {"out": L(pow_many([a[-1]] * n, e, Mod), W)}

                    def var_eb(P):                                   # one exponent for every base
                        da, de, out = P("base", L(a, W)), P("e", L(e[-1:], ew)), P("out", shape=(n, W))
                        return (lambda: lib.pai_modexp_var(h, da.ptr, 0, de.ptr, ew, ebits, 1, n, out.ptr, None)), \
                            {"out": L(pow_many(a, e[-1], Mod), W)}
                    sweep(K, "modarith", var_bb)
                    sweep(K, "modarith", var_eb)
    finally:
        lib.pai_modulus_destroy(h)
        _native.check(lib.pai_profile_enable(0))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_overlaps_are_refused(mk):
    """Every overlap the header forbids: PAI_E_INVALID, the message, and an arena no call has touched"""
    k, nk, key = mk, mk.nk, mk.key
    lib = nk.lib
    W, N = nk.cw, 6
    a, b = ciphertexts(k, N + 1, 7, units=True), ciphertexts(k, N + 1, 8, units=True)
    delta = np.array([0, 1, -1, 2, 0, 3], dtype=np.int32)
    e = L([5] * N, 1)

    def two(fn):
        """(a, b, shifted): output one row into a; the broadcast row as row 0 of the output; output one row into b"""
        def at_a(P):
            da, db = P("a", L(a, W)), P("b", L(b, W))
            return lambda: fn(da.ptr, db.ptr, 0, da.at(1))
        def bcast(P):
            da, db = P("a", L(a, W)), P("b", L(b, W))
            return lambda: fn(da.ptr, db.ptr, 1, db.ptr)
        def at_b(P):
            da, db = P("a", L(a, W)), P("b", L(b, W))
            return lambda: fn(da.ptr, db.ptr, 0, db.at(1))
        return ((at_a, "d_out overlaps d_a"), (bcast, "d_out overlaps the broadcast row d_b"), (at_b, "d_out overlaps d_b"))
    hdelta = host_ptr(delta)
    for name, fn in (("pai_ct_add", lambda pa, pb, bc, out: lib.pai_ct_add(nk.pk, pa, pb, bc, N, out, None)),
                     ("pai_ct_mont_mul", lambda pa, pb, bc, out: lib.pai_ct_mont_mul(nk.pk, pa, pb, bc, N, out, None)),
                     ("pai_ct_add_aligned_host", lambda pa, pb, bc, out: lib.pai_ct_add_aligned_host(nk.pk, pa, pb, bc, hdelta, N, out, None))):
        for build, msg in two(fn):
            refused(k, name, build, msg)
    for dom in (False, True):
        for shape in ("a", "bcast", "b"):
            def build(P):
                da, db, dl, de = P("a", L(a, W)), P("b", L(b, W)), P("delta", delta), P("entry", L([k.R], W))
                bc = 1 if shape == "bcast" else 0
                out = lambda: da.at(1) if shape == "a" else (db.ptr if shape == "bcast" else db.at(1))
                if dom:
                    return lambda: lib.pai_ct_add_aligned_dom(nk.pk, da.ptr, db.ptr, bc, dl.ptr, N, out(), de.ptr, None)
                return lambda: lib.pai_ct_add_aligned(nk.pk, da.ptr, db.ptr, bc, dl.ptr, N, out(), None)
            refused(k, "pai_ct_add_aligned", build, {"a": "d_out overlaps d_a", "bcast": "d_out overlaps the broadcast row d_b", "b": "d_out overlaps d_b"}[shape])

    def addn(P):
        regs = [P(f"op{j}", L(a if j % 2 else b, W)) for j in range(3)]
        return lambda: lib.pai_ct_addn(nk.pk, (C.c_void_p * 3)(*[r.ptr for r in regs]), None, 3, 0, 0, 0, N, regs[1].at(1), None)
    refused(k, "pai_ct_addn", addn, "pai_ct_addn: d_out overlaps an operand")
    for fn in (lib.pai_ct_invert, lib.pai_ct_invert_async):
        def inv(P, fn=fn):
            da = P("ct", L(a, W))
            return lambda: fn(nk.pk, da.ptr, N, da.at(1), None)
        refused(k, "pai_ct_invert", inv, "ct_invert: d_out overlaps d_ct")

    def invf(P):
        da, fl = P("ct", L(a, W)), P("flag", np.zeros(1, np.int32))
        return lambda: lib.pai_ct_invert_flag(nk.pk, da.at(1), N, da.ptr, fl.ptr, None)
    refused(k, "pai_ct_invert_flag", invf, "ct_invert: d_out overlaps d_ct")

    def addpl(P):
        da, dm = P("ct", L(a, W)), P("m", L(plain(k, N, 1), nk.nw))
        return lambda: lib.pai_ct_add_plain(nk.pk, da.ptr, dm.ptr, N, da.at(1), None)
    refused(k, "pai_ct_add_plain", addpl, "pai_ct_add_plain: d_out overlaps d_ct")

    def mul(P):
        da, de = P("ct", L(a, W)), P("e", e)
        return lambda: lib.pai_ct_mul(nk.pk, da.at(1), de.ptr, 1, 3, 0, N, da.ptr, None)
    refused(k, "pai_ct_mul", mul, "pai_ct_mul: d_out overlaps d_ct")

    def mul_host(P):                                     # the host-exponent form refuses before it stages anything
        da = P("ct", L(a, W))
        return lambda: lib.pai_ct_mul_host(nk.pk, da.at(1), host_ptr(e), 1, 3, 0, N, da.ptr, None)
    refused(k, "pai_ct_mul_host", mul_host, "pai_ct_mul: d_out overlaps d_ct")

    def addpl_m(P):                                     # 2 N plaintext rows are as long as N ciphertext rows: the output on top of them
        da, dm = P("ct", L(a, W)), P("m", L(plain(k, 2 * N, 1), nk.nw))
        return lambda: lib.pai_ct_add_plain(nk.pk, da.ptr, dm.ptr, N, dm.ptr, None)
    refused(k, "pai_ct_add_plain", addpl_m, "pai_ct_add_plain: d_out overlaps d_m")

    def mul_e(P):                                        # one-word exponents in front of a buffer that holds the whole output
        da, de = P("ct", L(a, W)), P("e", np.full((N * W, 1), 5, dtype=np.uint32))
        return lambda: lib.pai_ct_mul(nk.pk, da.ptr, de.ptr, 1, 3, 0, N, de.ptr, None)
    refused(k, "pai_ct_mul", mul_e, "pai_ct_mul: d_out overlaps d_e")
    for same in (True, False):
        def scan(P, same=same):
            da = P("ct", L(a, W))
            return lambda: lib.pai_ct_scan(nk.pk, da.ptr, N, 0, 0, 3, 0, None, None, da.ptr if same else da.at(1), None)
        refused(k, "pai_ct_scan", scan, "pai_ct_scan: d_out must not alias d_ct")
    for step in (False, True):
        for where in (0, 5):
            def pack(P, step=step, where=where):
                da = P("ct", L(a, W))
                f = lib.pai_ct_pack_step if step else lib.pai_ct_pack
                return lambda: f(nk.pk, da.ptr, N, 0, 16, 3, da.at(where), None)            # 2 output rows over rows 0-1 / 5-6 of the input
            refused(k, "pai_ct_pack", pack, "pai_ct_pack: d_out must not alias d_ct")

    def sl(P):
        da = P("src", L(a, W))
        return lambda: lib.pai_buf_slice(0, da.ptr, W, 1, 3, 2, da.at(4), None)             # reads rows 1, 3, 5; writes rows 4, 5, 6
    refused(k, "pai_buf_slice", sl, "pai_buf_slice: d_out overlaps the rows it reads")
    for where in (0, 3):
        def rot(P, where=where):
            da = P("src", L(a, W))
            return lambda: lib.pai_buf_rotate(0, da.ptr, W, 4, 1, da.at(where), None)
        refused(k, "pai_buf_rotate", rot, "pai_buf_rotate: d_out overlaps d_src")


def test_modmul_overlaps_are_refused():
    lib = _native.load()
    Mod = orc.BENCH_P
    W = (Mod.bit_length() + 31) // 32
    h = C.c_void_p()
    _native.check(lib.pai_modulus_create(host_ptr(L([Mod], W)), W, 0, C.byref(h)))
    K = SimpleNamespace(ident="m1024", nk=SimpleNamespace(lib=lib))
    vals = [Mod - 1 - i for i in range(5)]
    try:
        for shape, msg in (("a", "d_out overlaps d_a"), ("bcast", "d_out overlaps the broadcast row d_b"), ("b", "d_out overlaps d_b")):
            def build(P):
                da, db = P("a", L(vals, W)), P("b", L(vals, W))
                out = lambda: da.at(1) if shape == "a" else (db.ptr if shape == "bcast" else db.at(1))
                return lambda: lib.pai_modmul(h, da.ptr, db.ptr, 1 if shape == "bcast" else 0, 4, out(), None)
            refused(K, "pai_modmul", build, msg)
    finally:
        lib.pai_modulus_destroy(h)


# ---- what ran -----------------------------------------------------------------------------------------------------------------------
def test_every_family_ran_on_some_key():
    """Prints, per key and operation, the kernel and path families that ran, and the hand-downs; requires FAMILIES when every key ran."""
    for (ident, op), names in sorted(RAN.items()):
        print(f"COVERAGE {ident} {op}: {' '.join(sorted(names))}")
    for h in sorted(HANDDOWN):
        print(f"HANDDOWN {h}")
    if VISITED != set(KEY_IDS):
        pytest.skip(f"coverage not asserted: {len(VISITED)} of {len(KEY_IDS)} keys ran (a selection of the file)")
    for op, need in FAMILIES.items():
        seen = set().union(*(v for (_, o), v in RAN.items() if o == op))
        assert need <= seen, (op, sorted(need - seen))
    seen2048 = {op: set().union(*(v for (i, o), v in RAN.items() if o == op and i == "k2048")) for op in FAMILIES}
    # the 2048-bit key: what the last test of tests/test_gpu_extreme_keys.py requires of 1024-bit primes (its `pair` families need n
    # above 2048 bits: FAMILIES, on the 3072-bit key)
    assert {f"k_dec_a:{x}" for x in ("pp", "rl", "window", "pair4", "padic_kara_mul", "padic_kara", "padic_rowwise", "wide", "lane_group")} \
        <= seen2048["decrypt"], sorted(seen2048["decrypt"])
    assert {f"k_ctmul:{x}" for x in ("pp", "rl", "window", "pair4", "padic", "lane_group")} <= seen2048["ct_mul"], sorted(seen2048["ct_mul"])
    assert {f"k_encrypt(djn):{x}" for x in ("padic", "lane_group", "pair4", "lat_tree_m1", "lat_tree", "lat_chain")} <= seen2048["encrypt"], \
        sorted(seen2048["encrypt"])
    assert {"k_modmul_msb:lane_group", "k_modmul:lane_group", "k_modmul:lat", "k_add_aligned:lane_group", "k_pow2:lane_group", "k_pow2:lat", "k_pow2:padic"} \
        <= seen2048["ct_add"], sorted(seen2048["ct_add"])
