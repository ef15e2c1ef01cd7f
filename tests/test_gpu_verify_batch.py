"""GPU: batch verification of openings — pai_opening_fold (csrc/dispatch_open_fold.hpp, kernels_open_fold.hpp: k_open_fold) and
PaillierPublicKey.verify_openings.

Every expectation is a CPython integer: tests/test_verify_batch_cpu.py's fold_expect (pow only).  Where a case has more than eight
segments the right-hand sides come from the left-hand ones — the rows are valid openings, for which the CPU file proves
lhs == rhs — so that no test spends its time in CPython's pow(B, n, n^2); cases with invalid rows always take the full model.
The profile is on: the fused route must show k_open_fold, the composition route must not."""
import pickle
import random

import numpy as np
import pytest

from oracle import paillier_oracle as orc
from pailliercryptolib_python_amd import PaillierEncryptedNumber, PaillierOpening, _native, engine
from pailliercryptolib_python_amd.bindings import ipclCipherText
from tests._util import DevArray, disable, ints_to_limbs, limbs_to_ints, tune
from tests.test_extreme_keys_cpu import load_extreme_keys
from tests.test_gpu_crt_encrypt import keys
from tests.test_gpu_paillier_abi import NativeKey
from tests.test_recover_cpu import reencrypt
from tests.test_verify_batch_cpu import fold_expect

pytestmark = pytest.mark.gpu

KERNEL = "k_open_fold"
FUSED = (1024, 2048)
COMPOSED = (2112, 3072)


@pytest.fixture(autouse=True)
def profiled():
    engine.profile_enable(True)
    yield
    engine.profile_enable(False)


def derived_openings(n, count, rng, base=6):
    """`count` valid openings (ct, m, r) from `base` re-encryptions: products of small powers of two of them —
    ct_a^x ct_b^y opens to (x m_a + y m_b mod n, r_a^x r_b^y mod n)."""
    nsq = n * n
    bm = [rng.randrange(n) for _ in range(base)]
    br = [rng.randrange(1, n) for _ in range(base)]
    bc = [reencrypt(n, m, r) for m, r in zip(bm, br)]
    cts, ms, rs = [], [], []
    for _ in range(count):
        a, b = rng.sample(range(base), 2)
        x, y = rng.randrange(1, 8), rng.randrange(0, 8)
        cts.append(pow(bc[a], x, nsq) * pow(bc[b], y, nsq) % nsq)
        ms.append((x * bm[a] + y * bm[b]) % n)
        rs.append(pow(br[a], x, n) * pow(br[b], y, n) % n)
    return cts, ms, rs


_POOL = {}


def pool(bits):
    """513 valid openings per key size, built once"""
    if bits not in _POOL:
        key, _, _ = keys(bits)
        _POOL[bits] = derived_openings(key.n, 513, random.Random(bits + 16))
        c, m, r = _POOL[bits]
        assert all(reencrypt(key.n, m[i], r[i]) == c[i] for i in (0, 512))
    return _POOL[bits]


def coefficients(rng, count, ebits):
    es = [rng.getrandbits(ebits) for _ in range(count)]
    es[0] |= 1 << (ebits - 1)                              # the top window is used
    return es


def fold(pk, cts, ms, rs, es, ew, ebits, L):
    """pai_opening_fold on Python ints through the engine binding -> (lhs, rhs, flag) as ints"""
    h = pk.pubkey.handle
    up = lambda vals, words: engine.to_device_words(engine.ints_to_words(vals, words), h.device)
    lhs, rhs, flag = h.opening_fold(up(cts, h.ct_words), up(ms, h.n_words), up(rs, h.n_words), up(es, ew), ebits, L)
    back = lambda t: engine.words_to_ints(engine.to_host_words(t))
    return back(lhs), back(rhs), int(flag.item())


def expect_valid(n, cts, ms, rs, es, L):
    """(lhs, rhs) for VALID openings: the full model up to eight segments, the left-hand sides alone beyond"""
    if -(-len(cts) // L) <= 8:
        lhs, rhs, unit = fold_expect(n, cts, ms, rs, es, L)
        assert unit and lhs == rhs
        return lhs, rhs
    nsq = n * n
    lhs = []
    for s0 in range(0, len(cts), L):
        A = 1
        for c, e in zip(cts[s0:s0 + L], es[s0:s0 + L]):
            A = A * pow(c, e, nsq) % nsq
        lhs.append(A)
    return lhs, lhs


# (name, N, seg_len (None: N, -5: N + 5), coefficient bits, coefficient words, PAI_TUNE entries)
CASES = [
    ("one", 1, 1, 32, 1, {}),
    ("255-L3", 255, 3, 64, 2, {}),
    ("256-L64", 256, 64, 128, 4, {}),
    ("256-33bits", 256, 3, 33, 2, {}),                     # a window straddles the coefficient words
    ("257-chunk1", 257, None, 128, 4, {"open_chunk": 1}),
    ("257-chunk2", 257, -5, 64, 2, {"open_chunk": 2}),
    ("257-chunk3", 257, 1, 32, 1, {"open_chunk": 3}),
    ("257-chunk3-L64", 257, 64, 128, 4, {"open_chunk": 3}),
    ("513-grid1", 513, 64, 128, 4, {"open_chunk": 1, "open_grid": 1}),      # one workgroup walks three tiles, the last one ragged
]


def run_case(bits, case, monkeypatch):
    name, N, L, ebits, ew, knobs = case
    key, pk, _ = keys(bits)
    for k, v in knobs.items():
        tune(monkeypatch, k, v)
    L = N if L is None else (N + 5 if L == -5 else L)
    cts, ms, rs = (v[513 - N:] for v in pool(bits))        # every shape ends on the pool's last row
    es = coefficients(random.Random(N * 1000 + ebits), N, ebits)
    got = fold(pk, cts, ms, rs, es, ew, ebits, L)
    return key, (cts, ms, rs, es, L), got


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("bits", FUSED + COMPOSED)
def test_fold_against_the_model(bits, case, monkeypatch):
    key, (cts, ms, rs, es, L), (lhs, rhs, flag) = run_case(bits, case, monkeypatch)
    assert (KERNEL in engine.profile_last()) == (bits in FUSED), engine.profile_last()
    want_l, want_r = expect_valid(key.n, cts, ms, rs, es, L)
    assert lhs == want_l and rhs == want_r and flag == 0, (bits, case[0])


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_composition_route_gives_the_same_bits(case, monkeypatch):
    bits = 2048
    key, (cts, ms, rs, es, L), fused = run_case(bits, case, monkeypatch)
    assert KERNEL in engine.profile_last()
    disable(monkeypatch, "open_fold")
    _, pk, _ = keys(bits)
    composed = fold(pk, cts, ms, rs, es, case[4], case[3], L)
    assert KERNEL not in engine.profile_last() and "k_smexp" in engine.profile_last()
    assert composed == fused
    want_l, want_r = expect_valid(key.n, cts, ms, rs, es, L)
    assert composed[0] == want_l and composed[1] == want_r


@pytest.mark.parametrize("bits", (2048, 3072))
def test_row_blocks(bits, monkeypatch):
    """A call too large for one pass is cut into row blocks on segment boundaries by halving (here forced: at most 50 rows per
    block): 9 segments of 16 rows — tried as 9, then 5 — run as three blocks of 3 segments, the last one holding the ragged
    segment of one row.  The sides are the model's for the undivided call, and the unit flag of one block is the call's."""
    key, pk, _ = keys(bits)
    n, N, L = key.n, 129, 16
    cts, ms, rs = (list(v[513 - N:]) for v in pool(bits))
    es = [e | 1 for e in coefficients(random.Random(bits + 7), N, 64)]
    tune(monkeypatch, "open_block_rows", 50)
    cut = fold(pk, cts, ms, rs, es, 2, 64, L)
    assert (KERNEL in engine.profile_last()) == (bits in FUSED)
    want = fold_expect(n, cts, ms, rs, es, L)
    assert len(want[0]) == 9 and want[2] and want[0] == want[1]
    assert cut == (want[0], want[1], 0)
    # r_j = p in the second block: its flag bit is the call's; only that row's segment changes
    rs[60], cts[60] = key.p, reencrypt(n, ms[60], key.p)
    lhs, rhs, flag = fold(pk, cts, ms, rs, es, 2, 64, L)
    s, nsq = 60 // L, n * n
    A = B = 1
    M = 0
    for c, m, r, e in zip(cts[s * L:(s + 1) * L], ms[s * L:(s + 1) * L], rs[s * L:(s + 1) * L], es[s * L:(s + 1) * L]):
        A, B, M = A * pow(c, e, nsq) % nsq, B * pow(r, e, n) % n, (M + e * m) % n
    assert B % key.p == 0 and flag & 1 == 1
    assert lhs == want[0][:s] + [A] + want[0][s + 1:] and rhs == want[1][:s] + [(1 + n * M) * pow(B, n, nsq) % nsq] + want[1][s + 1:]


def test_argument_checks():
    _, pk, _ = keys(2048)
    h = pk.pubkey.handle
    cts, ms, rs = (v[:4] for v in pool(2048))
    up = lambda vals, words: engine.to_device_words(engine.ints_to_words(vals, words), h.device)
    ct, m, r = up(cts, h.ct_words), up(ms, h.n_words), up(rs, h.n_words)
    for ew, ebits, L in ((9, 32, 1), (1, 0, 1), (1, 33, 1), (2, 65, 1), (2, 32, 0)):
        with pytest.raises(_native.NativeError) as ei:
            h.opening_fold(ct, m, r, up([1, 2, 3, 4], ew), ebits, L)
        assert ei.value.code == _native.PAI_E_INVALID, (ew, ebits, L)
    lhs, rhs, flag = h.opening_fold(ct[:0], m[:0], r[:0], up([], 1), 32, 3)              # an empty batch: no segments
    assert lhs.shape[0] == rhs.shape[0] == 0 and int(flag.item()) == 0


@pytest.mark.parametrize("bits", (2048, 3072))
def test_corner_rows(bits, monkeypatch):
    key, pk, sk = keys(bits)
    n, p = key.n, key.p
    lam = 128
    tune(monkeypatch, "open_chunk", 2)
    # ciphertexts of the API: a sum, a scalar product, a packed row — opened by the key owner
    rng = np.random.default_rng(bits)
    a = pk.encrypt([float(v) for v in rng.uniform(-100, 100, 2)])
    b = pk.encrypt([int(v) for v in rng.integers(-100, 100, 2)])
    pkd = pk.encrypt_packed(np.arange(40, dtype=np.float64) - 7.5, exponent=8, value_bits=24, slot_bits=64)
    cts, ms, rs = [], [], []
    for x in (a + b, a * 3.5):
        op = sk.open(x)
        cts += [int(c) for c in x.ciphertextBN()]
        ms += op.raw()
        rs += op.randomness()
    r_p = sk.recover_randomness(pkd)
    r_p = r_p if isinstance(r_p, list) else [r_p]
    cts += engine.words_to_ints(engine.to_host_words(pkd.ciphertext().words))[:1]
    ms += [int(v) for v in sk.prikey.decrypt(pkd.ciphertext()).getTexts()][:1]
    rs += r_p[:1]
    # every corner plaintext with every corner randomness
    for m in (0, 1, n - 1):
        for r in (1, 2, n - 1):
            cts.append(reencrypt(n, m, r))
            ms.append(m)
            rs.append(r)
    N = len(cts)
    assert N == 14
    corner_e = [0, 1, (1 << lam) - 1, 1 << (lam - 1)]
    es = [corner_e[i % 4] for i in range(N)]
    es[4] = es[5] = 0                                      # chunk (4, 5) of segment 1: all coefficients 0
    L = 4
    lhs, rhs, flag = fold(pk, cts, ms, rs, es, 4, lam, L)
    assert (KERNEL in engine.profile_last()) == (bits <= 2048)
    want = fold_expect(n, cts, ms, rs, es, L)
    assert want[2] and want[0] == want[1]
    assert lhs == want[0] and rhs == want[1] and flag == 0
    # all coefficients 0: every product is 1
    lhs, rhs, flag = fold(pk, cts, ms, rs, [0] * N, 4, lam, L)
    assert lhs == rhs == [1] * 4 and flag == 0
    # a wrong plaintext: the sides differ in that segment only, as the model says
    wrong = list(ms)
    wrong[6] = (wrong[6] + 5) % n
    lhs, rhs, flag = fold(pk, cts, wrong, rs, es, 4, lam, L)
    want = fold_expect(n, cts, wrong, rs, es, L)
    assert lhs == want[0] and rhs == want[1] and flag == 0
    assert [x == y for x, y in zip(lhs, rhs)] == [True, False, True, True]
    # r_j = p: the unit flag
    rs2, cts2 = list(rs), list(cts)
    rs2[9] = p
    cts2[9] = reencrypt(n, ms[9], p)
    es2 = [e | 1 for e in es]
    lhs, rhs, flag = fold(pk, cts2, ms, rs2, es2, 4, lam, L)
    want = fold_expect(n, cts2, ms, rs2, es2, L)
    assert not want[2] and flag & 1 == 1
    assert lhs == want[0] and rhs == want[1]


STRUCTURED = [e for e in load_extreme_keys() if (e[1], e[2]) in (("ones", 1024), ("n0_one", 1024), ("zeros", 512))]


@pytest.mark.parametrize("ident,family,prime_bits,p,q", STRUCTURED, ids=[e[0] for e in STRUCTURED])
def test_structured_keys(ident, family, prime_bits, p, q):
    """three keys the digit engine serves, among them all-ones limbs of n and n0inv = 1: N = 37 rows, 128-bit coefficients"""
    assert len(STRUCTURED) == 3
    bits = 2 * prime_bits
    nk = NativeKey(orc.make_key(p, q, djn_x=None, bits=bits))
    n = p * q
    rng = random.Random(prime_bits + len(family))
    cts, ms, rs = derived_openings(n, 37, rng, base=4)
    es = coefficients(rng, 37, 128)
    L, S = 8, 5
    lhs, rhs = DevArray(shape=(S, nk.cw)), DevArray(shape=(S, nk.cw))
    flag = DevArray(np.zeros((1, 1), dtype=np.uint32))
    ct, m, r, e = (DevArray(ints_to_limbs(v, w)) for v, w in ((cts, nk.cw), (ms, nk.nw), (rs, nk.nw), (es, 4)))
    _native.check(nk.lib.pai_opening_fold(nk.pk, ct.ptr, m.ptr, r.ptr, 37, e.ptr, 4, 128, L, lhs.ptr, rhs.ptr, flag.ptr, None))
    assert KERNEL in engine.profile_last()
    want = fold_expect(n, cts, ms, rs, es, L)
    assert want[2] and limbs_to_ints(lhs.get()) == want[0] and limbs_to_ints(rhs.get()) == want[1], ident
    assert int(flag.get()[0, 0]) == 0
    del nk


# ---- PaillierPublicKey.verify_openings --------------------------------------------------------------------------------------------
def same_as_single(pk, x, opening, **kw):
    got = pk.verify_openings(x, opening, **kw)
    want = pk.verify_opening(x, opening)
    assert got.dtype == bool and got.shape == want.shape and got.tolist() == want.tolist(), (got, want)
    return got


@pytest.mark.parametrize("bits", (2048, 3072))
def test_api(bits):
    key, pk, sk = keys(bits)
    n = key.n
    N = 70
    vals = [float(v) for v in np.random.default_rng(bits + 1).uniform(-50, 50, N)]
    x = pk.encrypt(vals)
    op = sk.open(x)
    m, r = op.raw(), op.randomness()
    assert pk.verify_openings(x, op).all()
    assert (KERNEL in engine.profile_last()) == (bits <= 2048)
    assert same_as_single(pk, x, op).all()
    assert same_as_single(pk, x, (m, r), segment=64).all()                   # a pair of int lists, a ragged second segment
    assert same_as_single(pk, x, pickle.loads(pickle.dumps(op)), security_bits=64).all()
    one = pk.encrypt([1.5])
    op1 = sk.open(one)
    assert same_as_single(pk, one, (op1.raw(), op1.randomness())).tolist() == [True]      # single ints

    def only(i, got):
        want = np.ones(N, dtype=bool)
        want[list(i)] = False
        assert got.tolist() == want.tolist(), (i, got)

    # a failing segment of 64 with one bad element: exactly one False
    m2 = list(m)
    m2[17] = (m2[17] + 1) % n
    only([17], same_as_single(pk, x, (m2, r), segment=64))
    only([17], same_as_single(pk, x, (m2, r)))
    r2 = list(r)
    r2[66] += 1
    assert r2[66] < n
    only([66], same_as_single(pk, x, (m, r2), segment=64))
    # tampered ciphertexts: a fresh encryption of the same values has the same plaintexts and exponents, other ciphertexts
    y = pk.encrypt(vals)
    assert not same_as_single(pk, y, op, segment=64).any()
    # out-of-range values are False, never an exception
    m3, r3 = list(m), list(r)
    m3[0] = n
    r3[1] = 0
    r3[2] = r[2] + n
    m3[3] = m[3] + n
    r3[4] = 1 << (32 * len(m) * 100)
    only(range(5), same_as_single(pk, x, (m3, r3), segment=64))
    # a ciphertext row that is not a canonical residue (1 + n^2 for the ciphertext 1 = Enc(0, 1))
    cts = [int(c) for c in x.ciphertextBN()]
    z = PaillierEncryptedNumber(pk, ipclCipherText(pk.pubkey, [1 + n * n] + cts[1:]), x.exponent(), N)
    only([0], same_as_single(pk, z, ([0] + m[1:], [1] + r[1:]), segment=64))
    zc = PaillierEncryptedNumber(pk, ipclCipherText(pk.pubkey, [1] + cts[1:]), x.exponent(), N)
    assert same_as_single(pk, zc, ([0] + m[1:], [1] + r[1:]), segment=64).all()
    # exponents are compared, lengths and keys checked, as verify_opening does
    expo = x.exponent()
    expo[5] += 1
    only([5], same_as_single(pk, x, PaillierOpening(pk, *op._words(pk.pubkey.handle.device), expo, N)))
    with pytest.raises(ValueError):
        pk.verify_openings(x, (m[:-1], r[:-1]))
    with pytest.raises(ValueError):
        pk.verify_openings(x[0:3], op)
    with pytest.raises(ValueError):
        pk.verify_openings(x, op, security_bits=31)
    with pytest.raises(ValueError):
        pk.verify_openings(x, op, segment=0)
    with pytest.raises(TypeError):
        pk.verify_openings(x, 5)


@pytest.mark.parametrize("bits", (2048, 3072))
def test_negated_randomness_follows_the_parity(bits):
    """(m, n - r) is NOT pinned by the batch test: it passes exactly when the coefficients of those elements sum to an even number
    (tests/test_verify_batch_cpu.py); verify_opening says False.  A failing segment is checked row by row."""
    key, pk, sk = keys(bits)
    n = key.n
    N = 12
    x = pk.encrypt([float(v) for v in range(N)])
    op = sk.open(x)
    m, r = op.raw(), op.randomness()
    cts = [int(c) for c in x.ciphertextBN()]
    rng = random.Random(bits)
    seen = set()
    for J in ((3,), (1, 7), (0, 4, 9), (2, 3, 5, 11)):
        neg = [n - v if i in J else v for i, v in enumerate(r)]
        single = pk.verify_opening(x, (m, neg))
        assert single.tolist() == [i not in J for i in range(N)]
        for want_even in (True, False):
            es = [rng.getrandbits(32) for _ in range(N)]
            if (sum(es[i] for i in J) % 2 == 0) != want_even:
                es[J[0]] ^= 1
            lhs, rhs, unit = fold_expect(n, cts, m, neg, es, N)
            assert unit and (lhs == rhs) == want_even
            got = pk.verify_openings(x, (m, neg), security_bits=32, segment=N, _coefficients=es)
            assert got.tolist() == ([True] * N if want_even else single.tolist())
            seen.add(want_even)
    assert seen == {True, False}


@pytest.mark.parametrize("bits", (2048, 3072))
def test_packed_rows(bits):
    key, pk, sk = keys(bits)
    pkd = pk.encrypt_packed(np.arange(200, dtype=np.float64) - 7.5, exponent=8, value_bits=24, slot_bits=64)
    r = sk.recover_randomness(pkd)
    r = r if isinstance(r, list) else [r]
    m = [int(v) for v in sk.prikey.decrypt(pkd.ciphertext()).getTexts()]
    assert len(m) == pkd.rows >= 2
    assert pk.verify_openings(pkd, (m, r)).all()
    assert (KERNEL in engine.profile_last()) == (bits <= 2048)
    assert same_as_single(pk, pkd, (m, r)).all()
    summed = pkd + pkd
    assert not same_as_single(pk, summed, (m, r), segment=2).any()
