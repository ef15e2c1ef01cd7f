"""GPU: the data-format kernels (csrc/kernels_codec.hpp: k_fp_encode_f64, k_fp_encode_i64, k_fp_encode_at, k_fp_decode_i64;
csrc/kernels_pack.hpp: k_fp_pack, k_fp_unpack) on the 27 structured keys of tests/golden/extreme_keys.json and the 15 limit keys of
tests/golden/limit_keys.json, every comparison bit-exact against the oracle's codec (oracle.paillier_oracle.fp_encode / fp_decode),
fixedpoint.align_encoded and the Python-int model of the packed format (tests/_util.py).

Why these keys: the kernels write a negative mantissa as n - m with a hand-rolled borrow and compare rows against n word by word.
On a random modulus no word is 0 or all ones, so a borrow never ripples past word 2 and every comparison is decided in the top
word.  The families `ones`, `zeros` and `half` have n mod 2^64 below 2^26 and 8 to 64 zero words directly above word 1: every
negative float mantissa (at least 2^52) borrows across the whole zero run.  `ones_zeros` at 1536 / 2048 bits has 92 / 124 all-ones
words (the carry of r + B in unpack), and the limit keys have bits(n) = 521, 695, ..., 4175 — no multiple of 32 — for the
`mbits + dist <= bits(n) - 2` bound of k_fp_encode_at and the `k b <= bits(n) - 2` bound of the packed layout on a partial top
word.  tests/test_codec_keys_cpu.py holds these properties of the fixtures and of the inputs built here (codec_inputs) without a GPU.

One module-scoped handle per key; a key that cannot be created fails its tests.  The last test requires all 42 keys when the whole
file ran."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import paillier_oracle as orc
from pailliercryptolib_python_amd import _native
from pailliercryptolib_python_amd import fixedpoint as fp
from tests._util import DevArray, ints_to_limbs, limbs_to_ints, model_bias, model_max_slots, model_pack, model_unpack
from tests.test_extreme_keys_cpu import load_extreme_keys
from tests.test_gpu_codec import EDGE
from tests.test_limit_keys_cpu import load_limit_keys

pytestmark = pytest.mark.gpu

# (id, family or kind, prime bits, p, q): the 15 limit keys, then the 27 structured keys
ALL_KEYS = [(e[0], e[1], e[4], e[5], e[6]) for e in load_limit_keys()] + list(load_extreme_keys())
IDS = [e[0] for e in ALL_KEYS]
SLOT_BITS = (8, 29, 64, 65, 128)
AT_SHIFTS = (0, 1, 31, 32, 33)
AT_BCAST = (60, 2**31 - 1, -(2**31))
M32 = (1 << 32) - 1
VISITED = set()


def first_upper_word(n):
    """the index z >= 2 of the first non-zero 32-bit word of n above word 1"""
    z = 2
    while (n >> (32 * z)) & M32 == 0:
        z += 1
    return z


def zero_words_above_word_1(n):
    return first_upper_word(n) - 2


def float_inputs(rng):
    special = [s * math.ldexp(float(m), e - 52) for e in (-300, 0, 300) for m in (2**52, 2**53 - 1, 2**52 + 1) for s in (1, -1)]
    seeded = np.ldexp(rng.uniform(-1, 1, 200), rng.integers(-600, 1000, 200))
    return np.concatenate([np.array(EDGE), np.array(special), seeded])


def int_inputs(rng, n):
    vals = [0, 1, -1, 2**53, -(2**53), 2**63 - 1, -(2**63 - 1), -(2**63)]
    vals += [int(v) for v in rng.integers(-(2**63), 2**63 - 1, 150, dtype=np.int64)] + [int(v) for v in rng.integers(-1000, 1000, 50)]
    for L in (n % (1 << 64), n % (1 << 32)):                # the three values around the first borrow of n - |x|
        if L < 1 << 63:
            vals += [-(L - 1), -L, -(L + 1)]
    return np.array(vals, dtype=np.int64)


def decode_expect(r, n, max_int):
    """(flag, mantissa or None): flag 0 exactly when r < n and the centred value m has |m| < 2^63"""
    if r >= n:
        return 1, None
    m = r if r <= n // 2 else r - n
    if abs(m) >= 1 << 63:
        return 1, None
    assert orc.fp_decode(r, 0, n, max_int) == m
    return 0, m


def decode_rows(n, nw, max_int):
    full = 1 << (32 * nw)
    z = first_upper_word(n)
    rows = [m % n for m in (1, 2, 2**53, 2**63 - 1)] + [-m % n for m in (1, 2, 2**53, 2**63 - 1)]
    rows += [m % n for m in (2**63, 2**64 + 5, max_int, max_int + 1)] + [-m % n for m in (2**63, 2**64 + 5, max_int, max_int + 1)]
    rows += [n // 2]
    rows += [r for r in (n, n + 1, n + (1 << (32 * z))) if r < full] + [full - 1]                  # rows >= n
    rows += [n - (1 << 64), n - (1 << (32 * z))]                                                   # n - 2^(32 j): flag 1
    # (beyond the list of the issue: the same two with a low word of the difference set, so that only the upper words of n - r decide)
    rows += [n - (1 << 64) - 1, n - (1 << (32 * z)) - 1]
    return rows


def magnitudes(x, is_f64):
    """|mantissa| of every input as the encoders form it (0 for tiny floats and for -2^63)"""
    out = []
    for v in x:
        if is_f64:
            v = float(v)
            out.append(0 if abs(v) < 1e-200 else int(abs(math.frexp(v)[0]) * (1 << 53)))
        else:
            v = int(v)
            out.append(0 if v == -(2**63) else abs(v))
    return out


def at_targets(x, is_f64, enc, nbits, z):
    mags = magnitudes(x, is_f64)
    mb = np.array([m.bit_length() for m in mags], dtype=np.int64)
    ex0 = np.array([e for _, e in enc], dtype=np.int64)
    L = len(mags)
    dists = [np.full(L, d, dtype=np.int64) for d in AT_SHIFTS + (32 * (z - 1), 32 * z, 32 * (z + 1))]
    dists += [nbits - 2 - mb, nbits - 1 - mb, np.full(L, -5, dtype=np.int64)]
    bound_block = len(dists) - 3                            # index of the `mbits + d = bits(n) - 2` block; the next one is one more
    tg = np.concatenate([ex0 + d for d in dists])
    assert tg.min() >= -(2**31) and tg.max() < 2**31
    return mags, len(dists), bound_block, tg.astype(np.int32)


def pack_cases(n, nw):
    """per slot width b and slot count k: the pack calls [(E, v, raw int64 inputs, mantissas, model rows)] and the unpack rows
    [(row, claimed flag)]"""
    nbits = n.bit_length()
    full = 1 << (32 * nw)
    out = []
    for b in SLOT_BITS:
        kmax = model_max_slots(nbits, b)
        v = b - 1
        for k in sorted({1, 2, kmax}):
            assert 1 <= k and k * b <= nbits - 2
            H = (1 << min(v, 63)) - 1
            pats = [[-H] * k, [H] * k, ([-H, H] * k)[:k], [-1] * k, [0] * k, [0] * (k - 1) + [-1], [-1] + [0] * (k - 1),
                    [-1] * (k - 1) + [H]]
            flat = [m for p in pats for m in p]
            calls = []
            for E in sorted({0, max(0, v - 63)}):
                for raw in (flat + [-1], flat[:k], (flat[:k] + flat[3 * k:4 * k] + [H])):       # N = 8 k + 1, N = k, N = 2 k + 1
                    ms = [r << E for r in raw]
                    calls.append((E, v, raw, ms, model_pack(ms, b, k, n)))
            B = model_bias(b, k)
            lo, hi = -(1 << (b - 1)), (1 << (b - 1)) - 1
            unpack = [(r, 0) for c in calls for r in c[4]]
            unpack += [(r, 0) for r in model_pack([lo] * k + [hi] * k + ([lo, hi] * k)[:k], b, k, n)]     # the true extremes of a slot
            unpack += [((1 << (k * b)) - B, 1), (n, 2), (n - B - 1, 1)]
            unpack += [(n + 1, 2)] if n + 1 < full else []
            unpack += [(full - 1, 2), ((-B) % n, 0), ((-B) % n - 1, 1)]
            out.append(dict(b=b, k=k, calls=calls, unpack=unpack))
    return out


def codec_inputs(key):
    """Every input of this module and its expected value, from the oracle / the model alone; deterministic per key."""
    n, nbits, max_int = key.n, key.n.bit_length(), key.n // 3 - 1
    nw = (key.bits + 31) // 32
    z = first_upper_word(n)
    rng = np.random.default_rng(n % (1 << 61))
    ci = dict(n=n, nw=nw, z=z)
    ci["xf"] = float_inputs(rng)
    ci["xi"] = int_inputs(rng, n)
    ci["want_f"] = [orc.fp_encode(float(v), n, max_int) for v in ci["xf"]]
    ci["want_i"] = [orc.fp_encode(int(v), n, max_int) for v in ci["xi"]]
    ci["dec_rows"] = decode_rows(n, nw, max_int)
    ci["dec_want"] = [decode_expect(r, n, max_int) for r in ci["dec_rows"]]
    for tag, x, is_f64, enc in (("f", ci["xf"], True, ci["want_f"]), ("i", ci["xi"], False, ci["want_i"])):
        mags, blocks, bound_block, tg = at_targets(x, is_f64, enc, nbits, z)
        res0 = ints_to_limbs([r for r, _ in enc], nw)
        ex0 = np.array([e for _, e in enc], dtype=np.int32)
        want_r, want_e = fp.align_encoded(np.tile(res0, (blocks, 1)), np.tile(ex0, blocks), tg, n, max_int)
        bcast = [fp.align_encoded(res0, ex0, np.array([t], dtype=np.int64), n, max_int) for t in AT_BCAST]
        ci["at_" + tag] = dict(x=np.tile(x, blocks), targets=tg, want_r=want_r, want_e=want_e, bcast=bcast, L=len(mags), mags=mags,
                               bound_block=bound_block, ex0=ex0)
    ci["pack"] = pack_cases(n, nw)
    return ci


class CodecKey:
    def __init__(self, ident, family, b, p, q):
        from tests.test_gpu_extreme_keys import Key

        self.ident = ident
        self.k = Key(ident, family, b, p, q)
        self.nk, self.key = self.k.nk, self.k.key
        self.ci = codec_inputs(self.key)
        assert self.ci["nw"] == self.nk.nw


@pytest.fixture(scope="module", params=ALL_KEYS, ids=IDS)
def ck(request):
    k = CodecKey(*request.param)
    VISITED.add(k.ident)
    return k


def test_encoders(ck):
    """pai_fp_encode_f64 / pai_fp_encode_i64 -> orc.fp_encode(v, n, n // 3 - 1)"""
    nk, ci = ck.nk, ck.ci
    for x, want, fn in ((ci["xf"], ci["want_f"], nk.lib.pai_fp_encode_f64), (ci["xi"], ci["want_i"], nk.lib.pai_fp_encode_i64)):
        N = x.shape[0]
        dx, dm, de = DevArray(x), DevArray(shape=(N, nk.nw)), DevArray(shape=(N,), dtype=np.int32)
        _native.check(fn(nk.pk, dx.ptr, N, dm.ptr, de.ptr, None))
        got = limbs_to_ints(dm.get())
        bad = [(i, x[i]) for i in range(N) if got[i] != want[i][0]]
        assert not bad, (ck.ident, x.dtype, bad[:5])
        assert de.get().tolist() == [w[1] for w in want], (ck.ident, x.dtype)


def test_decoder(ck):
    """pai_fp_decode_i64: flag 0 exactly when r < n and |m| < 2^63, then the mantissa is the oracle's"""
    nk, ci = ck.nk, ck.ci
    rows, want = ci["dec_rows"], ci["dec_want"]
    N = len(rows)
    dm = DevArray(ints_to_limbs(rows, nk.nw))
    dmant, dflag = DevArray(shape=(N,), dtype=np.int64), DevArray(shape=(N,), dtype=np.int32)
    _native.check(nk.lib.pai_fp_decode_i64(nk.pk, dm.ptr, N, dmant.ptr, dflag.ptr, None))
    mant, flag = dmant.get().tolist(), dflag.get().tolist()
    assert flag == [f for f, _ in want], (ck.ident, [i for i in range(N) if flag[i] != want[i][0]])
    assert [m for m, (f, _) in zip(mant, want) if f == 0] == [m for f, m in want if f == 0], ck.ident


@pytest.mark.parametrize("kind", ["f", "i"])
def test_encode_at(ck, kind):
    """pai_fp_encode_at -> fixedpoint.align_encoded of the oracle's encodings: per-element targets at every distance of the list,
    and the three broadcast targets"""
    nk, at = ck.nk, ck.ci["at_" + kind]
    is_f64 = 1 if kind == "f" else 0
    x, tg, L = at["x"], at["targets"], at["L"]
    N = x.shape[0]
    dx, dt = DevArray(x), DevArray(tg)
    dm, de = DevArray(shape=(N, nk.nw)), DevArray(shape=(N,), dtype=np.int32)
    _native.check(nk.lib.pai_fp_encode_at(nk.pk, dx.ptr, is_f64, N, dt.ptr, 0, dm.ptr, de.ptr, None))
    got_e, got_r = de.get(), dm.get()
    bad = [(i // L, i % L, x[i], int(tg[i])) for i in np.nonzero(got_e != at["want_e"])[0][:5]]
    assert not bad, (ck.ident, kind, "exponents (block, input, value, target)", bad)
    bad = [(i // L, i % L, x[i], int(tg[i])) for i in np.nonzero((got_r != at["want_r"]).any(axis=1))[0][:5]]
    assert not bad, (ck.ident, kind, "residues (block, input, value, target)", bad)
    dm1, de1 = DevArray(shape=(L, nk.nw)), DevArray(shape=(L,), dtype=np.int32)
    for t, (want_r, want_e) in zip(AT_BCAST, at["bcast"]):
        dt1 = DevArray(np.array([t], dtype=np.int32))
        _native.check(nk.lib.pai_fp_encode_at(nk.pk, dx.ptr, is_f64, L, dt1.ptr, 1, dm1.ptr, de1.ptr, None))
        assert de1.get().tolist() == want_e.tolist(), (ck.ident, kind, "broadcast", t)
        assert np.array_equal(dm1.get(), want_r), (ck.ident, kind, "broadcast", t)


def unpacked(out, b, count):
    o = out.get()
    if b <= 64:
        return [int(v) for v in o[:count]]
    return [(int(hi) << 64) + int(lo) for lo, hi in zip(np.ascontiguousarray(o[:count, 0]).view(np.uint64), o[:count, 1])]


def test_pack_and_unpack(ck):
    """pai_fp_pack -> model_pack, pai_fp_unpack of those rows -> the mantissas with flag 0, and pai_fp_unpack's flags (and the
    mantissas where the flag is 0) on the rows around 2^(k b), n and the bias -> model_unpack"""
    nk, n = ck.nk, ck.key.n
    for case in ck.ci["pack"]:
        b, k = case["b"], case["k"]
        for E, v, raw, ms, want in case["calls"]:
            N, G = len(raw), len(want)
            dx, dm, dflag = DevArray(np.array(raw, dtype=np.int64)), DevArray(shape=(G, nk.nw)), DevArray(np.zeros(1, dtype=np.int32))
            _native.check(nk.lib.pai_fp_pack(nk.pk, dx.ptr, 0, N, E, v, b, k, dm.ptr, dflag.ptr, None))
            assert int(dflag.get()[0]) == 0, (ck.ident, b, k, E, N)
            got = limbs_to_ints(dm.get())
            assert got == want, (ck.ident, b, k, E, N, [g for g in range(G) if got[g] != want[g]])
            do = DevArray(shape=(G * k, 2) if b > 64 else (G * k,), dtype=np.int64)
            df = DevArray(shape=(G,), dtype=np.int32)
            _native.check(nk.lib.pai_fp_unpack(nk.pk, dm.ptr, G, b, k, do.ptr, df.ptr, None))
            back = unpacked(do, b, G * k)
            assert df.get().tolist() == [0] * G and back[:N] == ms and not any(back[N:]), (ck.ident, b, k, E, N)
        rows = [r for r, _ in case["unpack"]]
        G = len(rows)
        dm = DevArray(ints_to_limbs(rows, nk.nw))
        do = DevArray(shape=(G * k, 2) if b > 64 else (G * k,), dtype=np.int64)
        df = DevArray(shape=(G,), dtype=np.int32)
        _native.check(nk.lib.pai_fp_unpack(nk.pk, dm.ptr, G, b, k, do.ptr, df.ptr, None))
        flags, back = df.get().tolist(), unpacked(do, b, G * k)
        model = [model_unpack(r, b, k, n) for r in rows]
        assert flags == [f for f, _ in model], (ck.ident, b, k, [g for g in range(G) if flags[g] != model[g][0]])
        for g, (f, ms) in enumerate(model):
            if f == 0:
                assert back[g * k:(g + 1) * k] == ms, (ck.ident, b, k, g)
    st = C.c_int(-1)
    _native.check(nk.lib.pai_pubkey_status(nk.pk, C.byref(st), 0, None))
    assert st.value == 0


def test_codec_ran_on_every_key():
    """All 42 keys when the whole file ran; a selection of keys only prints."""
    print(f"COVERAGE codec and packing kernels: {len(VISITED)} keys")
    if VISITED != set(IDS):
        print(f"COVERAGE not asserted: {len(VISITED)} of {len(IDS)} keys ran")
        return
    assert len(VISITED) == 42
