"""GPU: packed ciphertexts — pai_fp_pack / pai_fp_unpack / pai_ct_pack and the PaillierPackedNumber API, every check exact.

The expectations come from the Python-int model of the format below (include/paillier_hip.h, "packed ciphertexts"), from
CPython / the C oracle's modular exponentiation on the ciphertexts (tests/_util.pow_many) and from oracle.paillier_oracle
decryption — never from the code under test.

pai_ct_pack has two routes: the level driver of pai_ct_segment_prod (route A, every key size) and, for keys up to 2048 bits and
batches of at least pack_padic_min_rows output rows (csrc/path_ranges.hpp; op 4 of pai_path_edges), one chain per lane on digit
pairs (route B, k_ct_pack_padic).  The tests force each route (PAI_DISABLE=pack_padic / PAI_TUNE pack_padic_min=0), check which
kernels ran (pai_profile_last), stand on both sides of the hand-over read from the library, and force short chunks
(PAI_TUNE segprod_chunk) so that k-member chains cross the driver's levels."""
import ctypes
from fractions import Fraction
import json
from pathlib import Path
import pickle

import numpy as np
import pytest
import torch

from oracle import paillier_oracle as orc
from pailliercryptolib_python_amd import PaillierPackedNumber, PaillierPrivateKey, PaillierPublicKey, _native, engine
from pailliercryptolib_python_amd.bindings import ipclCipherText, ipclPublicKey
from pailliercryptolib_python_amd.paillier import PaillierEncryptedNumber

from ._util import disable, model_bias, model_max_slots, model_pack, model_unpack, pow_many, rand_below, tune

pytestmark = pytest.mark.gpu

SLOT_BITS = (8, 29, 32, 53, 64, 65, 100, 128)
_KEYS = {}


def keypair(bits):
    if bits not in _KEYS:
        fx = json.loads((Path(__file__).parent / "golden" / "fixture_keys.json").read_text())[str(bits)]
        key = orc.make_key(int(fx["p"], 16), int(fx["q"], 16), djn_x=(1 << 70) + 12345, bits=bits)
        pk = PaillierPublicKey(ipclPublicKey(key.n, bits, True, hs=key.hs, randbits=key.randbits))
        _KEYS[bits] = (key, pk, PaillierPrivateKey(pk, key.p, key.q))
    return _KEYS[bits]


# ---- the model of the format (Python ints only): model_max_slots, model_bias, model_pack and model_unpack live in tests/_util.py ----
def model_mantissa(x, E):
    """rint(x 2^E), ties to even, exactly (Fraction.__round__ rounds half to even); ints: x << E"""
    return round(Fraction(x) * Fraction(2) ** E) if isinstance(x, float) else int(x) << E


def model_add_bits(va, vb, b):
    v = max(va, vb) + 1
    if v + 1 > b:
        raise OverflowError
    return v


def model_mul_bits(v, c, b):
    v += abs(c).bit_length()
    if v + 1 > b:
        raise OverflowError
    return v


# ---- helpers ------------------------------------------------------------------------------------------------------------------
def dev(a, h):
    return torch.from_numpy(np.ascontiguousarray(a)).to(h.device)


def rows_of(t):
    return engine.words_to_ints(engine.to_host_words(t))


def unpacked_ints(out, b):
    o = out.cpu().numpy()
    if b <= 64:
        return [int(v) for v in o]
    return [(int(hi) << 64) + int(lo) for lo, hi in zip(np.ascontiguousarray(o[:, 0]).view(np.uint64), o[:, 1])]


def slot_counts(nb, b):
    kmax = model_max_slots(nb, b)
    return sorted({k for k in (1, 2, 7, kmax) if k <= kmax})


def signed_mantissas(rng, N, v):
    lim = (1 << v) - 1
    out = [lim, -lim, 0] + [int.from_bytes(rng.bytes(17), "little") % (2 * lim + 1) - lim for _ in range(N)]
    return [out[int(i)] for i in rng.permutation(len(out))[:N]]


def call_status(h):
    """the handle's sticky status word (pai_pubkey_status), left in place"""
    v = ctypes.c_int(-1)
    _native.check(h.lib.pai_pubkey_status(h.h, ctypes.byref(v), 0, None))
    return v.value


# ---- pai_fp_pack / pai_fp_unpack ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [1024, 2048, 3072])
def test_fp_pack_rows_equal_the_model_and_unpack_inverts_them(bits):
    key, pk, _ = keypair(bits)
    h = pk.pubkey.handle
    n, nb = key.n, key.n.bit_length()
    rng = np.random.default_rng(bits)
    for b in SLOT_BITS:
        v = b - 1                                          # full value_bits
        for k in slot_counts(nb, b):
            for N in sorted({1, max(1, k - 1), k, k + 1, 3 * k + 2}):
                # integer inputs: 63-bit magnitudes shifted up to the full width of the slot
                E = max(0, v - 63)
                raw = signed_mantissas(rng, N, min(v, 63))
                ms = [m << E for m in raw]
                rows, flag = h.fp_pack(dev(np.array(raw, dtype=np.int64), h), E, v, b, k)
                assert int(flag.item()) == 0
                want = model_pack(ms, b, k, n)
                assert rows_of(rows) == want, (bits, b, k, N, "int")
                out, fl = h.fp_unpack(rows, b, k)
                got = unpacked_ints(out, b)
                assert fl.cpu().tolist() == [0] * len(want) and got[:N] == ms and not any(got[N:]), (bits, b, k, N)
                # float inputs: half-to-even ties, the largest double mantissas the slot takes, zeros, subnormals
                E = int(rng.integers(-5, min(v, 60) + 1))
                xs = []
                for _ in range(N):
                    c = int(rng.integers(0, 5))
                    x = [(float(rng.integers(-1000, 1000)) + 0.5) * 2.0 ** -E,
                         float(rng.uniform(-1, 1)) * 2.0 ** (min(v, 52) - E - 1),
                         float((1 << min(v, 53)) - 1) * 2.0 ** -E * (1 if rng.integers(0, 2) else -1),
                         0.0, 5e-324 * float(rng.integers(1, 5))][c]
                    xs.append(x if abs(model_mantissa(x, E)) < 1 << v else 0.0)
                ms = [model_mantissa(x, E) for x in xs]
                rows, flag = h.fp_pack(dev(np.array(xs, dtype=np.float64), h), E, v, b, k)
                assert int(flag.item()) == 0
                assert rows_of(rows) == model_pack(ms, b, k, n), (bits, b, k, N, E, "float")
                assert unpacked_ints(h.fp_unpack(rows, b, k)[0], b)[:N] == ms


def test_fp_pack_negative_rows_and_ties():
    key, pk, _ = keypair(2048)
    h = pk.pubkey.handle
    # the sign of P_g is that of its highest non-zero slot: rows [.., -1], [-1, 0, 0] and [5, 0, -0.0]
    x = np.array([7.0, 3.0, -1.0, -1.0, 0.0, 0.0, 5.0, 0.0, -0.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5])
    ms = [model_mantissa(float(t), 0) for t in x]
    assert ms[9:] == [0, 2, 2, 0, -2, -2]                 # round half to even
    rows, flag = h.fp_pack(dev(x, h), 0, 7, 8, 3)
    want = model_pack(ms, 8, 3, key.n)
    assert int(flag.item()) == 0 and rows_of(rows) == want
    assert want[0] > key.n // 2 and want[1] > key.n // 2 and want[2] == 5


def test_fp_pack_flags():
    _, pk, _ = keypair(2048)
    h = pk.pubkey.handle
    f = lambda a, E, v, b, k: int(h.fp_pack(dev(a, h), E, v, b, k)[1].item())
    assert f(np.array([1.0, 1023.0, -1023.0]), 0, 10, 32, 3) == 0
    assert f(np.array([1.0, 1024.0, 2.0]), 0, 10, 32, 3) == 1
    assert f(np.array([1.0, -1023.5, 2.0]), 0, 10, 32, 3) == 1            # rint(-1023.5) = -1024
    assert f(np.array([1.0, 1023.4999, 2.0]), 0, 10, 32, 3) == 0
    assert f(np.array([1.0, np.nan, 2.0]), 0, 10, 32, 3) & 2
    assert f(np.array([-np.inf]), 0, 10, 32, 3) & 2
    assert f(np.array([1e300]), 900, 127, 128, 1) == 1
    assert f(np.array([1, 1 << 62], dtype=np.int64), 70, 127, 128, 2) == 1
    assert f(np.array([1, 1 << 56], dtype=np.int64), 70, 127, 128, 2) == 0
    assert f(np.array([127, -127, 128], dtype=np.int64), 0, 7, 8, 2) == 1
    assert call_status(h) == 0


@pytest.mark.parametrize("bits", [1024, 2048, 3072])
def test_fp_unpack_of_model_residues_and_flags(bits):
    key, pk, _ = keypair(bits)
    h = pk.pubkey.handle
    n, nb = key.n, key.n.bit_length()
    for b in SLOT_BITS:
        k = model_max_slots(nb, b)
        lo, hi = -(1 << (b - 1)), (1 << (b - 1)) - 1
        good = model_pack([lo] * k + [hi] * k + ([lo, hi] * k)[:k] + [-1] * k + [0] * k, b, k, n)
        bad = [(1 << (k * b)) - model_bias(b, k), n, (n - model_bias(b, k) - 1) % n, n + 1, (1 << (32 * h.n_words)) - 1]
        rows = good[:2] + [bad[0], good[2], bad[1], bad[2], good[3], bad[3], bad[4], good[4]]
        out, fl = h.fp_unpack(engine.to_device_words(engine.ints_to_words(rows, h.n_words), h.device), b, k)
        got = unpacked_ints(out, b)
        for g, r in enumerate(rows):
            f, ms = model_unpack(r, b, k, n)
            assert int(fl[g]) == f, (bits, b, g)
            if f == 0:
                assert got[g * k:(g + 1) * k] == ms, (bits, b, g)
        assert fl.cpu().tolist() == [0, 0, 1, 0, 2, 1, 0, 2, 2, 0]


def test_bad_layouts_are_invalid_and_launch_nothing():
    _, pk, _ = keypair(2048)
    h = pk.pubkey.handle
    x = dev(np.ones(8), h)
    ct = h.empty_ct(8)
    m = h.empty_pt(1)
    for b, k in ((7, 1), (129, 1), (64, 32), (8, 256), (64, 0)):
        if k >= 1:
            with pytest.raises(_native.NativeError) as e:
                h.fp_pack(x, 0, 5, b, k)
            assert e.value.code == _native.PAI_E_INVALID
            with pytest.raises(_native.NativeError) as e:
                h.fp_unpack(m, b, k)
            assert e.value.code == _native.PAI_E_INVALID
            with pytest.raises(_native.NativeError) as e:
                h.ct_pack(ct, b, k)
            assert e.value.code == _native.PAI_E_INVALID
        else:
            out = h.empty_ct(8)
            rc = h.lib.pai_ct_pack(h.h, ct.data_ptr(), 8, 0, b, k, out.data_ptr(), None)
            assert rc == _native.PAI_E_INVALID
    with pytest.raises(_native.NativeError):
        h.fp_pack(x, 0, 64, 64, 2)                         # value_bits + 1 > slot_bits
    assert call_status(h) == 0


# ---- pai_ct_pack ----------------------------------------------------------------------------------------------------------------
def want_packed(cts, b, k, nsq):
    """prod_j ct_(g k + j)^(2^(b j)) mod n^2 per output row, the powers through tests/_util.pow_many"""
    pw = pow_many(cts, [1 << (b * (i % k)) for i in range(len(cts))], nsq)
    out = []
    for g in range(0, len(cts), k):
        acc = 1
        for v in pw[g:g + k]:
            acc = acc * v % nsq
        out.append(acc)
    return out


def pack_rows(h, t, b, k, tag=0):
    return rows_of(h.ct_pack(t, b, k, tag=tag))


def pack_rows_and_kernels(h, t, b, k):
    """(rows, names of the kernels the call launched)"""
    engine.profile_enable(True)
    try:
        rows = rows_of(h.ct_pack(t, b, k))
        return rows, set(engine.profile_last())
    finally:
        engine.profile_enable(False)


def pack_edges(h):
    cnt = ctypes.c_int(0)
    buf = (ctypes.c_size_t * 8)()
    _native.check(h.lib.pai_path_edges(h.h, 4, buf, 8, ctypes.byref(cnt)))
    return [int(buf[i]) for i in range(min(cnt.value, 8))]


@pytest.mark.parametrize("bits,b,big", [(1024, 32, 2500), (2048, 64, 3000), (2048, 8, 600), (2048, 100, 0), (3072, 53, 1500),
                                        (4096, 128, 0)])
def test_ct_pack_equals_the_product_of_powers(bits, b, big, monkeypatch):
    key, pk, _ = keypair(bits)
    h = pk.pubkey.handle
    nb = key.n.bit_length()
    rng = np.random.default_rng(bits + b)
    ks = slot_counts(nb, b) if bits < 4096 else [model_max_slots(nb, b)]
    for k in ks:
        sizes = sorted({1, max(1, k - 1), k, k + 1} | ({big} if big and k == ks[-1] else set()))
        if bits == 4096:
            sizes = [k + 1]
        for N in sizes:
            cts = rand_below(rng, key.nsq, N)
            t = engine.to_device_words(engine.ints_to_words(cts, h.ct_words), h.device)
            want = want_packed(cts, b, k, key.nsq)
            got = pack_rows(h, t, b, k)
            assert got == want, (bits, b, k, N)
            if bits <= 2048:                               # both routes forced: identical rows from two engines
                tune(monkeypatch, "pack_padic_min", 0)
                rows_b, kern_b = pack_rows_and_kernels(h, t, b, k)
                disable(monkeypatch, "pack_padic")
                rows_a, kern_a = pack_rows_and_kernels(h, t, b, k)
                disable(monkeypatch, "pack_padic", False)
                tune(monkeypatch, "pack_padic_min", None)
                assert rows_b == want and rows_a == want, (bits, b, k, N)
                assert "k_ct_pack_padic" in kern_b and "k_segprod" not in kern_b, kern_b
                assert "k_segprod" in kern_a and "k_ct_pack_padic" not in kern_a, kern_a
            if N <= k + 1 or N == big:
                for tag in (1, -1):                        # rows at a lazy domain tag: x R^tag in, the wire form out
                    assert pack_rows(h, h.ct_retag(t, 0, tag), b, k, tag=tag) == want, (bits, b, k, N, tag)
            if N == big or (N == k + 1 and k > 2):
                for chunk in (1, 2, 3):                    # k-member chains cut into chunks: every level of the driver
                    tune(monkeypatch, "segprod_chunk", chunk)
                    assert pack_rows(h, t, b, k) == want, (bits, b, k, N, chunk)
                tune(monkeypatch, "segprod_chunk", None)
    assert call_status(h) == 0


@pytest.mark.parametrize("bits", [1024, 2048])
def test_ct_pack_on_both_sides_of_the_route_hand_over(bits, monkeypatch):
    """the default dispatch at G = E and G = E + 1 output rows, E read from the library: the k_segprod levels below, digit pairs above"""
    key, pk, _ = keypair(bits)
    h = pk.pubkey.handle
    edges = pack_edges(h)
    assert len(edges) == 1 and edges[0] >= 1
    E, b, k = edges[0], 64, 2
    rng = np.random.default_rng(bits + 77)
    cts = rand_below(rng, key.nsq, (E + 1) * k)
    t = engine.to_device_words(engine.ints_to_words(cts, h.ct_words), h.device)
    want = want_packed(cts, b, k, key.nsq)
    below, kern_below = pack_rows_and_kernels(h, t[:E * k - 1].contiguous(), b, k)      # E rows, the last one ragged
    above, kern_above = pack_rows_and_kernels(h, t, b, k)                               # E + 1 rows
    assert above == want and below[:-1] == want[:E - 1] and below[-1] == cts[E * k - 2]
    assert "k_segprod" in kern_below and "k_ct_pack_padic" not in kern_below, kern_below
    assert "k_ct_pack_padic" in kern_above and "k_segprod" not in kern_above, kern_above
    disable(monkeypatch, "pack_padic")
    assert pack_rows(h, t, b, k) == want
    disable(monkeypatch, "pack_padic", False)
    tune(monkeypatch, "pack_padic_min", 5)                   # the knob moves the edge
    assert pack_edges(h) == [4]
    assert call_status(h) == 0


# ---- the public API, 2048 bits --------------------------------------------------------------------------------------------------
def test_encrypt_packed_round_trip_and_oracle_plaintext():
    key, pk, sk = keypair(2048)
    rng = np.random.default_rng(5)
    for b, v, E, N in ((64, 40, 30, 1000), (100, 99, 46, 45), (8, 7, 3, 700), (65, 53, 20, 130)):
        x = rng.uniform(-1, 1, N) * 2.0 ** (min(v, 52) - E - 1)
        x[:3] = [0.0, (2.0 ** min(v, 53) - 1) * 2.0 ** -E, -(2.0 ** min(v, 53) - 1) * 2.0 ** -E]
        ms = [model_mantissa(float(t), E) for t in x]
        p = pk.encrypt_packed(x, exponent=E, value_bits=v, slot_bits=b)
        k = model_max_slots(2048, b)
        assert isinstance(p, PaillierPackedNumber) and len(p) == N and (p.slot_bits, p.slots, p.exponent, p.value_bits) == (b, k, E, v)
        assert p.ciphertext().getSize() == -(-N // k)
        assert sk.decrypt_packed_mantissas(p) == ms
        assert np.array_equal(sk.decrypt_packed(p), np.array([float(Fraction(m) / Fraction(2) ** E) for m in ms]))
        # the oracle decrypts one packed ciphertext to the model's P_g
        want = model_pack(ms, b, k, key.n)
        g = len(want) // 2
        assert orc.decrypt_crt(key, int(p.ciphertext().getTexts()[g])) == want[g]
    # integers, raw encryption: the ciphertext bits are 1 + P_g n
    xi = rng.integers(-1000, 1000, 77)
    p = pk.encrypt_packed(xi, exponent=2, value_bits=12, slot_bits=16, slots=5, apply_obfuscator=False)
    ms = [int(t) << 2 for t in xi]
    assert [int(c) for c in p.ciphertext().getTexts()] == [orc.raw_encrypt(r, key.n) for r in model_pack(ms, 16, 5, key.n)]
    assert sk.decrypt_packed_mantissas(p) == ms
    assert sk.decrypt_packed(pk.encrypt_packed([], exponent=0, value_bits=5, slot_bits=8)).shape == (0,)


def test_pack_of_mixed_exponents_decrypts_like_the_elements():
    key, pk, sk = keypair(2048)
    rng = np.random.default_rng(6)
    N = 500
    # floats with mixed exponents; the mantissas aligned to the largest exponent keep the 53 significant bits of their doubles
    # (trailing zeros only), so the float comparison is exact equality
    x = rng.integers(-(1 << 10), 1 << 10, N).astype(np.float64) * 2.0 ** rng.integers(-8, 1, N)
    x[:4] = [0.0, 1.0, -1.0, 2.0 ** -8]
    enc = pk.encrypt(x)
    E = max(enc.exponent())
    assert len(set(enc.exponent())) > 3
    ms = [model_mantissa(float(t), E) for t in x]
    v = max(abs(m) for m in ms).bit_length()
    assert v <= 79
    b = 80
    p = enc.pack(slot_bits=b, value_bits=v)
    assert p.exponent == E and len(p) == N and p.slots == model_max_slots(2048, b)
    assert sk.decrypt_packed_mantissas(p) == ms
    ref = np.asarray(sk.decrypt(enc), dtype=np.float64)
    assert np.array_equal(sk.decrypt_packed(p), ref) and np.array_equal(ref, x)
    # a larger common exponent, few slots; the ciphertext bits against CPython
    p2 = enc[:10].pack(slot_bits=100, value_bits=v + 5, exponent=E + 5, slots=3)
    assert sk.decrypt_packed_mantissas(p2) == [m << 5 for m in ms[:10]]
    cts = [pow(int(c), 1 << (E + 5 - e), key.nsq) for c, e in zip(enc[:10].ciphertextBN(), enc.exponent()[:10])]
    assert [int(c) for c in p2.ciphertext().getTexts()] == want_packed(cts, 100, 3, key.nsq)
    with pytest.raises(ValueError):
        enc.pack(slot_bits=b, value_bits=v, exponent=E - 1)


def test_arithmetic_chain_and_headroom():
    key, pk, sk = keypair(2048)
    h = pk.pubkey.handle
    rng = np.random.default_rng(7)
    N, b, E = 300, 64, 16
    xp = rng.uniform(-100, 100, N)
    xp[0] = 99.5
    xq = rng.uniform(-100, 100, N)
    arr = rng.uniform(-1000, 1000, N)
    mp, mq, ma = ([model_mantissa(float(t), E) for t in a] for a in (xp, xq, arr))
    p = pk.encrypt_packed(xp, exponent=E, value_bits=24, slot_bits=b)
    q = pk.encrypt_packed(xq, exponent=E, value_bits=24, slot_bits=b)
    r = (p + q) * (-3) + arr
    va = max(abs(m) for m in ma).bit_length()
    assert r.value_bits == model_add_bits(model_mul_bits(model_add_bits(24, 24, b), -3, b), va, b)
    want = [(a + c) * -3 + d for a, c, d in zip(mp, mq, ma)]
    assert sk.decrypt_packed_mantissas(r) == want
    assert sk.decrypt_packed_mantissas(arr + p) == [a + d for a, d in zip(mp, ma)]
    assert sk.decrypt_packed_mantissas(p - q) == [a - c for a, c in zip(mp, mq)]
    assert sk.decrypt_packed_mantissas(p - arr) == [a - d for a, d in zip(mp, ma)]
    assert sk.decrypt_packed_mantissas(np.int64(5) * p) == [5 * a for a in mp]
    assert sk.decrypt_packed_mantissas(p * 0) == [0] * N
    assert sk.decrypt_packed_mantissas(PaillierPackedNumber.add_many([p, q, p])) == [2 * a + c for a, c in zip(mp, mq)]
    ints = rng.integers(-50, 50, N)
    assert sk.decrypt_packed_mantissas(p + ints) == [a + (int(t) << E) for a, t in zip(mp, ints)]
    # the ciphertext of p + q is the product of the rows
    cp, cq = ([int(c) for c in z.ciphertext().getTexts()] for z in (p, q))
    assert [int(c) for c in (p + q).ciphertext().getTexts()] == [a * c % key.nsq for a, c in zip(cp, cq)]
    # errors raise before any kernel and leave the handle's status word clear
    with pytest.raises(OverflowError):
        p * (1 << 39)
    with pytest.raises(OverflowError):
        pk.encrypt_packed(xp, exponent=E, value_bits=62, slot_bits=b) + q * 2 + q + q
    with pytest.raises(ValueError):
        pk.encrypt_packed(xp, exponent=E, value_bits=22, slot_bits=b)         # |m| reaches 99.5 * 2^16 > 2^22
    with pytest.raises(ValueError):
        pk.encrypt_packed(np.array([1.0, np.nan]), exponent=E, value_bits=24, slot_bits=b)
    with pytest.raises(ValueError):
        p + pk.encrypt_packed(xq, exponent=E + 1, value_bits=24, slot_bits=b)
    with pytest.raises(TypeError):
        p * 2.5
    assert call_status(h) == 0
    h.check_status(force=True)
    # a plaintext outside the packed range (what a broken value_bits promise produces) is an OverflowError at decryption
    zone = PaillierPackedNumber(pk, ipclCipherText(pk.pubkey, [orc.raw_encrypt(1 << 2045, key.n)]), slot_bits=8, slots=255,
                                exponent=0, value_bits=7, length=255)
    with pytest.raises(OverflowError):
        sk.decrypt_packed(zone)
    with pytest.raises(OverflowError):
        sk.decrypt_packed_mantissas(zone)
    assert call_status(h) == 0


def test_segment_sum_then_pack():
    key, pk, sk = keypair(2048)
    rng = np.random.default_rng(8)
    N, K = 4000, 37
    x = rng.integers(-(1 << 16), 1 << 16, N).astype(np.float64) / 256.0
    ids = rng.integers(0, K, N)
    enc = pk.encrypt(x)
    seg = enc.segment_sum(ids, K)
    E = max(seg.exponent())
    sums = [sum(Fraction(float(t)) for t in x[ids == s]) for s in range(K)]
    want = [int(s * Fraction(2) ** E) for s in sums]
    assert all(Fraction(w) == s * Fraction(2) ** E for w, s in zip(want, sums))
    v = max(1, max(abs(w) for w in want).bit_length())
    p = seg.pack(slot_bits=100, value_bits=v)
    assert p.ciphertext().getSize() == 2 and sk.decrypt_packed_mantissas(p) == want
    assert np.array_equal(sk.decrypt_packed(p), np.array([float(s) for s in sums]))
    # integers (exponent 0) in 64-bit slots: the int64 side of pai_fp_unpack
    xi = rng.integers(-(1 << 40), 1 << 40, N)
    segi = pk.encrypt(xi).segment_sum(ids, K)
    wi = [int(xi[ids == s].sum()) for s in range(K)]
    pi = segi.pack(slot_bits=64, value_bits=max(abs(w) for w in wi).bit_length())
    assert pi.exponent == 0 and pi.slots == 31 and pi.ciphertext().getSize() == 2
    assert sk.decrypt_packed_mantissas(pi) == wi and np.array_equal(sk.decrypt_packed(pi), np.array(wi, dtype=np.float64))


def test_pickle_and_obfuscator():
    key, pk, sk = keypair(2048)
    x = np.arange(-40, 40, dtype=np.float64) / 8
    p = pk.encrypt_packed(x, exponent=3, value_bits=10, slot_bits=16)
    q = pickle.loads(pickle.dumps(p))
    assert (len(q), q.slot_bits, q.slots, q.exponent, q.value_bits) == (len(p), 16, p.slots, 3, 10)
    assert [int(c) for c in q.ciphertext().getTexts()] == [int(c) for c in p.ciphertext().getTexts()]
    assert np.array_equal(sk.decrypt_packed(q), x)
    before = [int(c) for c in q.ciphertext().getTexts()]
    q.apply_obfuscator()
    assert [int(c) for c in q.ciphertext().getTexts()] != before
    assert np.array_equal(sk.decrypt_packed(q), x)
