"""GPU: ciphertext openings — pai_recover_r (csrc/kernels_recover.hpp: k_rrec_a, k_rrec_b), PaillierPrivateKey.recover_randomness /
open and PaillierPublicKey.verify_opening.

Every expectation is a CPython integer (tests/test_recover_cpu.py: pow on the half-width primes plus Garner; on three elements per
case also the full-width pow(c mod n, n^-1 mod lcm(p - 1, q - 1), n)); for DJN ciphertexts with known r' also pow(h, r', n), h the
opening of hs.  The profile is on: every served call must show k_rrec_a and k_rrec_b, the refused one must show nothing."""
import math
import pickle

import numpy as np
import pytest

from oracle import paillier_oracle as orc
from pailliercryptolib_python_amd import PaillierOpening, PaillierPrivateKey, PaillierPublicKey, _native, engine
from pailliercryptolib_python_amd.bindings import ipclPublicKey
from tests._util import DevArray, ints_to_limbs, limbs_to_ints, tune
from tests.test_gpu_crt_encrypt import keys
from tests.test_gpu_paillier_abi import NativeKey
from tests.test_recover_cpu import all_keys, expect_r, expect_r_full, reencrypt

pytestmark = pytest.mark.gpu

SIZES = (1024, 1536, 2048, 2112, 3072, 4096, 4128)       # primes on 36 x 1 up to 2048 bits, on 36 x 2 above
DJN_X = 0xABCDEF1234567                                   # the x of tests.test_gpu_keysizes.make: hs = (-x^2)^n mod n^2


@pytest.fixture(autouse=True)
def profiled():
    engine.profile_enable(True)
    yield
    engine.profile_enable(False)


def served():
    prof = engine.profile_last()
    assert "k_rrec_a" in prof and "k_rrec_b" in prof, prof


def recover(pk, sk, cts):
    """pai_recover_r on ciphertexts given as ints, through the word-level binding"""
    h = pk.pubkey.handle
    got = sk.prikey.recover_r_words(engine.to_device_words(engine.ints_to_words(cts, h.ct_words), h.device))
    served()
    return engine.words_to_ints(engine.to_host_words(got))


def check_full_width(key, cts, got, idx=(0, 1, -1)):
    for i in sorted({i % len(cts) for i in idx}):         # (three elements where the batch has them)
        if math.gcd(cts[i], key.n) == 1:
            assert got[i] == expect_r_full(key.p, key.q, cts[i])


@pytest.mark.parametrize("bits", SIZES)
def test_key_sizes(bits):
    key, pk, sk = keys(bits)
    N = 37 if bits <= 2048 else 9
    vals = [float(v) for v in np.random.default_rng(bits).uniform(-1000, 1000, N)]
    r = orc.synth_r_limbs(bits + 3, N, key.randbits)
    en = pk.encrypt(vals, r=r)
    cts = [int(c) for c in en.ciphertextBN()]
    got = sk.recover_randomness(en)
    served()
    assert got == [expect_r(key.p, key.q, c) for c in cts]
    h = (-DJN_X * DJN_X) % key.n
    assert reencrypt(key.n, 0, h) == key.hs
    assert got == [pow(h, rr, key.n) for rr in orc.limbs_to_ints(r)]
    check_full_width(key, cts, got)
    assert all(reencrypt(key.n, m, rr) == c for m, rr, c in zip(sk.raw_decrypt(en)[:3], got[:3], cts[:3]))


_POOL = {}


def pool(bits):
    """2 E + 1 random residues modulo n^2 and their expectation, once per key size (E = elements per workgroup)"""
    if bits not in _POOL:
        key, _, _ = keys(bits)
        E = 256 if bits <= 2048 else 128
        rng = np.random.default_rng(bits + 17)
        cts = [int.from_bytes(rng.bytes(bits // 4 + 8), "little") % key.nsq for _ in range(2 * E + 1)]
        _POOL[bits] = (E, cts, [expect_r(key.p, key.q, c) for c in cts])
    return _POOL[bits]


@pytest.mark.parametrize("bits", (2048, 3072))
@pytest.mark.parametrize("shape", ("1", "E-1", "E", "E+1", "2E+1:grid1"))
def test_shapes(bits, shape, monkeypatch):
    key, pk, sk = keys(bits)
    assert pk.pubkey.handle.n_words * 32 == bits
    E, cts, want = pool(bits)
    N = {"1": 1, "E-1": E - 1, "E": E, "E+1": E + 1, "2E+1:grid1": 2 * E + 1}[shape]
    if shape.endswith("grid1"):
        tune(monkeypatch, "rrec_grid", 1)                 # one workgroup per prime walks three tiles, the last one ragged
    off = len(cts) - N                                    # (every shape ends on the pool's last row)
    got = recover(pk, sk, cts[off:])
    assert got == want[off:], (bits, shape)
    check_full_width(key, cts[off:], got)


def crt(p, q, ap, aq):
    return ap + p * ((aq - ap) * pow(p, -1, q) % q)


@pytest.mark.parametrize("bits", (2048, 3072))
def test_corner_rows(bits):
    key, pk, sk = keys(bits)
    n, nsq, p, q = key.n, key.nsq, key.p, key.q
    assert p < q
    m = int.from_bytes(np.random.default_rng(bits).bytes(bits // 8), "little") % n
    rows = {
        "one": (1, 1),
        "minus one": (nsq - 1, n - 1),
        "g": (1 + n, 1),
        "raw encryption": ((1 + m * n) % nsq, 1),
        "2^n": (pow(2, n, nsq), 2),                       # r_p = r_q = 2: the lift's difference is 0
        "r_q - r_p > 0": (crt(p, q, 1, q - 1), crt(p, q, 1, q - 1)),         # (-1)^(odd exponent) = -1 modulo q
        "r_q - r_p < 0": (crt(p, q, p - 1, 1), crt(p, q, p - 1, 1)),
        "non-unit p k": (p * (nsq // p - 12345), None),
        "non-unit q k": (q * 6789, None),
    }
    cts = [c for c, _ in rows.values()]
    got = recover(pk, sk, cts)
    for (name, (c, r)), g in zip(rows.items(), got):
        assert g == expect_r(p, q, c), name
        assert 0 <= g < n
        if r is not None:
            assert g == r, name
            assert g == expect_r_full(p, q, c), name
    assert got[-2] % p == 0 and got[-2] % q != 0          # the call succeeds and gives r == 0 modulo the prime that divides the row
    assert got[-1] % q == 0 and got[-1] % p != 0


def standard_pair(bits):
    key, _, _ = keys(bits)
    pk = PaillierPublicKey(ipclPublicKey(key.n, bits, False))
    return key, pk, PaillierPrivateKey(pk, key.p, key.q)


_STD = {}


@pytest.mark.parametrize("scheme", ("djn", "standard"))
def test_closure_through_the_public_api(scheme):
    bits = 2048
    if scheme == "djn":
        key, pk, sk = keys(bits)
    else:
        if bits not in _STD:
            _STD[bits] = standard_pair(bits)
        key, pk, sk = _STD[bits]
    rng = np.random.default_rng(5)
    N = 12
    a = pk.encrypt([float(v) for v in rng.uniform(-1000, 1000, N)])
    b = pk.encrypt([int(v) for v in rng.integers(-1000, 1000, N)])
    assert a.exponent() != b.exponent()                  # mixed exponents: the sum aligns them
    ids = np.arange(N) % 3
    cases = {
        "fresh": a,
        "a + b": a + b,
        "a * 3.5": a * 3.5,
        "a - b": a - b,
        "segment_sum": a.segment_sum(ids, 3),
        "cumsum": a.cumsum(),
    }
    for name, x in cases.items():
        op = sk.open(x)
        served()
        assert isinstance(op, PaillierOpening) and len(op) == len(x)
        ok = pk.verify_opening(x, op)
        assert ok.dtype == bool and ok.shape == (len(x),) and ok.all(), name
        assert op.decode() == sk.decrypt(x), name
        assert op.raw() == sk.raw_decrypt(x) and op.randomness() == sk.recover_randomness(x), name
        cts = [int(c) for c in x.ciphertextBN()]
        ms, rs = op.raw(), op.randomness()
        ms, rs = (ms, rs) if len(x) > 1 else ([ms], [rs])
        assert all(reencrypt(key.n, m, r) == c for m, r, c in list(zip(ms, rs, cts))[:3]), name
    # packed rows: the opening of each row as a pair of int lists
    pkd = pk.encrypt_packed(np.arange(40, dtype=np.float64) - 7.5, exponent=8, value_bits=24, slot_bits=64)
    r = sk.recover_randomness(pkd)
    served()
    r = r if isinstance(r, list) else [r]
    m = [int(v) for v in sk.prikey.decrypt(pkd.ciphertext()).getTexts()]
    assert len(r) == pkd.rows == len(m)
    assert pk.verify_opening(pkd, (m, r)).all()
    summed = pkd + pkd
    m2 = [int(v) for v in sk.prikey.decrypt(summed.ciphertext()).getTexts()]
    r2 = sk.recover_randomness(summed)
    r2 = r2 if isinstance(r2, list) else [r2]
    assert pk.verify_opening(summed, (m2, r2)).all()
    assert not pk.verify_opening(summed, (m, r)).any()


def test_negatives():
    key, pk, sk = keys(2048)
    n = key.n
    N = 6
    x = pk.encrypt([float(v) for v in np.random.default_rng(9).uniform(-5, 5, N)])
    op = sk.open(x)
    m, r = op.raw(), op.randomness()
    assert pk.verify_opening(x, (m, r)).all()

    def only(i, got):
        want = np.ones(N, dtype=bool)
        want[i] = False
        assert got.tolist() == want.tolist(), (i, got)

    for i, bit in ((0, 0), (2, 1000), (5, n.bit_length() - 2)):
        r2 = list(r)
        r2[i] ^= 1 << bit
        if 0 < r2[i] < n:
            assert math.gcd(r2[i], n) == 1
        only(i, pk.verify_opening(x, (m, r2)))
    for i in (1, 4):
        m2 = list(m)
        m2[i] += 1
        only(i, pk.verify_opening(x, (m2, r)))
    for i, (dm, rr) in enumerate([(0, 0), (0, n), (n - m[2], r[2]), (0, r[3] + n), (n, r[4]), (0, 1 << (32 * len(m) * 100))]):
        m2, r2 = list(m), list(r)
        m2[i] += dm                                       # i == 2: m_i = n exactly; i == 4: m_i + n
        r2[i] = rr
        only(i, pk.verify_opening(x, (m2, r2)))           # False, never an exception
    # the same through an opening whose device rows were tampered with, and one with a wrong exponent
    h = pk.pubkey.handle
    bad_r = list(r)
    bad_r[3] = n                                          # fits the row, is not a residue
    t = PaillierOpening(pk, engine.to_device_words(engine.ints_to_words(m, h.n_words), h.device),
                        engine.to_device_words(engine.ints_to_words(bad_r, h.n_words), h.device), x.exponent(), N)
    only(3, pk.verify_opening(x, t))
    expo = x.exponent()
    expo[1] += 1
    t = PaillierOpening(pk, *op._words(h.device), expo, N)
    only(1, pk.verify_opening(x, t))
    with pytest.raises(ValueError):
        pk.verify_opening(x, (m[:-1], r[:-1]))
    with pytest.raises(ValueError):
        pk.verify_opening(x, (m, r + [1]))
    with pytest.raises(ValueError):
        pk.verify_opening(x[0:3], op)
    other_key, other_pk, other_sk = keys(1536)
    with pytest.raises(ValueError):
        other_sk.recover_randomness(x)
    with pytest.raises(ValueError):
        other_sk.open(x)


ALL_KEYS = all_keys()


@pytest.mark.parametrize("ident,p,q", ALL_KEYS, ids=[e[0] for e in ALL_KEYS])
def test_every_structured_and_limit_key_is_served(ident, p, q):
    """all 42 (tests/test_recover_cpu.py holds the count and gcd(n, (p - 1)(q - 1)) = 1): five DJN ciphertexts each"""
    bits = 2 * max(p.bit_length(), q.bit_length())
    djn = orc.make_key(p, q, djn_x=DJN_X, bits=bits)
    nk = NativeKey(orc.make_key(p, q, djn_x=None, bits=bits))
    rng = np.random.default_rng(p % (1 << 32))
    ms = [0, djn.n - 1] + [int.from_bytes(rng.bytes(bits // 8 + 8), "little") % djn.n for _ in range(3)]
    rs = [1, (1 << djn.randbits) - 1] + orc.limbs_to_ints(orc.synth_r_limbs(bits, 3, djn.randbits))
    cts = [orc.encrypt(djn, m, r) for m, r in zip(ms, rs)]
    ct, out = DevArray(ints_to_limbs(cts, nk.cw)), DevArray(shape=(5, nk.nw))
    _native.check(nk.lib.pai_recover_r(nk.sk, ct.ptr, 5, out.ptr, None))
    served()
    got = limbs_to_ints(out.get())
    assert got == [expect_r(p, q, c) for c in cts], ident
    h = (-DJN_X * DJN_X) % djn.n
    assert got == [pow(h, r, djn.n) for r in rs], ident
    assert got[2] == expect_r_full(p, q, cts[2]), ident
    del nk


# A key with p | q - 1: gcd(n, (p - 1)(q - 1)) = p, r -> r^n is no bijection modulo q and n has no inverse modulo q - 1.
# Found by: p = orc.seeded_prime(500, 20261019); k = 2048; repeat k += 2, q = k p + 1 until q has 512 bits and is prime (k = 2608).
# (q = k p + 1 with an even k >= 2 is wider than p: two primes of exactly 512 bits cannot have p | q - 1.  p has 500 bits.)
P_DIV = 0xe847b5d4c16d2f034158c99d4db3ef52bd6e73033195e674fabe8438f25c088d6ab791086cede25ed1a8d762feed5bd08422da056114d40b2ed0e579ab7d7
Q_DIV = 0x93e5a8c6772884ef129b885f28799161ae9d533b089271bc7ba74e30425099720af2e1585d5b77225f7e812408512175c42230d16cd043031ecf021c7830de51


def test_key_without_unique_openings_is_refused():
    assert (Q_DIV - 1) % P_DIV == 0 and (Q_DIV - 1) // P_DIV == 2608 and Q_DIV.bit_length() == 512 and P_DIV.bit_length() == 500
    assert orc.is_probable_prime(P_DIV) and orc.is_probable_prime(Q_DIV)
    key = orc.make_key(P_DIV, Q_DIV, djn_x=DJN_X, bits=1024)
    pk = PaillierPublicKey(ipclPublicKey(key.n, 1024, True, hs=key.hs, randbits=key.randbits))
    sk = PaillierPrivateKey(pk, P_DIV, Q_DIV)                            # pai_privkey_create accepts the key ...
    vals = [1.5, -2.25, 1000.0]
    x = pk.encrypt(vals)
    assert sk.decrypt(x) == vals                                         # ... and it decrypts
    for _ in range(2):                                                   # refused on the first call and on every later one
        with pytest.raises(_native.NativeError) as ei:
            sk.recover_randomness(x)
        assert ei.value.code == _native.PAI_E_INVALID and "coprime" in str(ei.value)
        assert engine.profile_last() == {}                               # nothing was launched
    with pytest.raises(_native.NativeError):
        sk.open(x)
    assert sk.decrypt(x) == vals


def test_private_handle_may_be_destroyed_after_its_public_handle():
    """A garbage collector destroys the two handles of a key in either order (the objects of the test above die in a reference
    cycle with the caught exception).  pai_privkey_destroy frees its own memory on the device it recorded at creation and does not
    look at the public handle: no HIP error is left behind for the caller's next call to report."""
    import torch

    key, _, _ = keys(1024)
    nk = NativeKey(orc.make_key(key.p, key.q, djn_x=None, bits=1024))
    ct, out = DevArray(ints_to_limbs([1 + key.n, pow(2, key.n, key.nsq)], nk.cw)), DevArray(shape=(2, nk.nw))
    _native.check(nk.lib.pai_recover_r(nk.sk, ct.ptr, 2, out.ptr, None))
    assert limbs_to_ints(out.get()) == [1, 2]
    nk.lib.pai_pubkey_destroy(nk.pk)
    nk.lib.pai_privkey_destroy(nk.sk)
    nk.pk = nk.sk = None                                                 # (NativeKey.__del__ then destroys NULL handles: no-ops)
    torch.cuda.synchronize()
    assert int(torch.ones(4, device="cuda").sum()) == 4


def test_pickling():
    key, pk, sk = keys(2048)
    x = pk.encrypt([0.5, -3.0, 7.25, 1e6])
    op = sk.open(x)
    blob = pickle.dumps(op)
    op2 = pickle.loads(blob)
    assert isinstance(op2._m, np.ndarray) and isinstance(op2._r, np.ndarray)          # host words
    assert len(op2) == len(op) and op2.raw() == op.raw() and op2.randomness() == op.randomness()
    assert op2.exponent() == x.exponent()
    assert [int(v) for v in sk.prikey.recover_r(x.ciphertext()).getTexts()] == op.randomness()      # the container-level binding
    assert op2.decode() == sk.decrypt(x)
    assert pk.verify_opening(x, op2).all()
    assert pk.verify_opening(pickle.loads(pickle.dumps(x)), pickle.loads(blob)).all()
