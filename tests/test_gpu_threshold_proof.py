"""GPU: verifiable threshold decryption — pai_sha256_rows / pai_sha256_expand (csrc/kernels_sha256.hpp, dispatch_transcript.hpp)
against hashlib, and PaillierKeyShare.partial_decrypt(prove=True) / PaillierPublicKey.verify_partial / verified_parts against the
integer model of pailliercryptolib_python_amd/threshold.py (prove_int, verify_int), bit for bit.

The hash kernels see every padding case (message length mod 64 = 52 fits the length, 56 and 60 spill a block, 0 adds a whole block),
part boundaries inside a block, one row to several tiles of rows under one workgroup, and both alignment classes of tests/_arena.py
(the 16-byte loads serve only aligned parts whose rows keep the 16-byte grid; everything else goes word by word).  The protocol's oracle takes the
DEVICE's partial decryptions as its data (they are held to CPython by tests/test_gpu_threshold.py): what is compared is the proof."""
import ctypes as C
import hashlib
import json
import pickle
import struct
from pathlib import Path

import numpy as np
import pytest

from oracle import paillier_oracle as orc
from pailliercryptolib_python_amd import (PaillierDecryptionProof, PaillierPrivateKey, PaillierPublicKey, PaillierVerificationKey, _native,
                                          engine)
from pailliercryptolib_python_amd import threshold as th
from pailliercryptolib_python_amd.bindings import ipclPublicKey
from tests._arena import ALIGNS, FILLERS, Arena
from tests._util import host_ptr, tune
from tests.test_gpu_crt_encrypt import keys

pytestmark = pytest.mark.gpu

ROWS, EXPAND = "k_sha256_rows", "k_sha256_expand"
PAI_E_INVALID = -1
_SAFE = {}


@pytest.fixture(autouse=True)
def profiled():
    engine.profile_enable(True)
    yield
    engine.profile_enable(False)


def safe_key():
    """(key, pk, sk) of the 1024-bit safe-prime key of tests/golden/safe_prime_keys.json"""
    if not _SAFE:
        fx = next(k for k in json.loads((Path(__file__).parent / "golden" / "safe_prime_keys.json").read_text()) if k["name"] == "k1024")
        p, q = int(fx["p"], 16), int(fx["q"], 16)
        key = orc.make_key(p, q, djn_x=0xABCDEF1234567, bits=1024)
        pk = PaillierPublicKey(ipclPublicKey(key.n, 1024, True, hs=key.hs, randbits=key.randbits))
        _SAFE["k"] = (key, pk, PaillierPrivateKey(pk, p, q))
    return _SAFE["k"]


def key_of(bits):
    return safe_key() if bits == 1024 else keys(bits)


def handle():
    return keys(2048)[1].pubkey.handle


def digests(mats):
    """hashlib over the rows of the host matrices side by side, as uint32 [N, 8]"""
    n = mats[0].shape[0]
    out = b"".join(hashlib.sha256(b"".join(m[j].tobytes() for m in mats)).digest() for j in range(n))
    return np.frombuffer(out, dtype=np.uint32).reshape(n, 8)


def random_mats(widths, n, seed, fill=None):
    rng = np.random.default_rng(seed)
    if fill is not None:
        return [np.full((n, w), fill, dtype=np.uint32) for w in widths]
    return [rng.integers(0, 1 << 32, size=(n, w), dtype=np.uint64).astype(np.uint32) for w in widths]


def run_rows(h, mats):
    got = h.sha256_rows([engine.to_device_words(m, h.device) for m in mats])
    assert list(engine.profile_last()) == [ROWS]
    return engine.to_host_words(got)


# ---- pai_sha256_rows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("words", (1, 13, 14, 15, 16, 17, 29, 30, 31, 32, 128))
def test_rows_every_padding_case(words):
    h = handle()
    for n in (1, 65):
        mats = random_mats((words,), n, 100 * words + n)
        assert np.array_equal(run_rows(h, mats), digests(mats)), (words, n)
    for fill in (0, 0xFFFFFFFF):
        mats = random_mats((words,), 3, 0, fill)
        assert np.array_equal(run_rows(h, mats), digests(mats)), (words, fill)


@pytest.mark.parametrize("widths", ((64, 64), (128, 128), (20, 7, 37), (16, 3, 32), (4, 4, 4, 4), (4096,), (1, 1, 1, 13)))
def test_rows_parts(widths):
    """K = 1 .. 4; unequal widths put part boundaries inside a block, and widths that are no multiple of 4 take rows off the
    16-byte grid"""
    h = handle()
    n = 7 if max(widths) > 1000 else 70
    mats = random_mats(widths, n, sum(widths))
    assert np.array_equal(run_rows(h, mats), digests(mats)), widths


@pytest.mark.parametrize("n", (1, 63, 64, 65, 300))
def test_rows_counts_and_the_tile_loop(n, monkeypatch):
    h = handle()
    mats = random_mats((128, 128), n, n)
    want = digests(mats)
    assert np.array_equal(run_rows(h, mats), want), n
    tune(monkeypatch, "sha_grid", 1)                              # one workgroup walks the tiles, the last one ragged
    assert np.array_equal(run_rows(h, mats), want), n


def arena_sweep(build):
    """build(place) -> (call, expected); both alignment classes, both fillers; the whole arena is compared after the call"""
    lib = _native.load()
    for al in ALIGNS:
        for fill in FILLERS:
            ar = Arena(fill)
            try:
                call, expected = build(lambda name, host=None, **kw: ar.place(name, host, align=al, **kw))
                ar.commit()
                rc = call()
                _native.check(lib.pai_stream_sync(0, None))
                if expected is None:
                    assert rc == PAI_E_INVALID, rc
                    ar.check({})                                  # refused: nothing written
                else:
                    _native.check(rc)
                    ar.check(expected)
            finally:
                ar.free()


@pytest.mark.parametrize("widths,n", (((128, 128), 67), ((17,), 5), ((64, 6, 64), 300)))
def test_rows_memory_contract(widths, n):
    h = handle()
    mats = random_mats(widths, n, 5 * n)
    wd = np.asarray(widths, dtype=np.int32)

    def call_on(regs, out, k=None, wd_=wd, rows=n):
        def call():
            ptrs = (C.c_void_p * 4)(*([r.address for r in regs] + [regs[0].address] * (4 - len(regs))))
            return h.lib.pai_sha256_rows(h.h, ptrs, host_ptr(wd_), len(regs) if k is None else k, rows, out.ptr, None)
        return call

    def served(P):
        regs = [P(f"part{i}", m) for i, m in enumerate(mats)]
        return call_on(regs, P("digest", shape=(n, 8))), {"digest": digests(mats)}

    arena_sweep(served)
    assert list(engine.profile_last()) == [ROWS]

    def refused(**kw):
        def build(P):
            regs = [P(f"part{i}", m) for i, m in enumerate(mats)]
            return call_on(regs, P("digest", shape=(n, 8)), **kw), None
        return build

    bad_w = wd.copy()
    bad_w[-1] = 0
    wide_w = wd.copy()
    wide_w[0] = 4097
    for kw in (dict(k=0), dict(k=5), dict(wd_=bad_w), dict(wd_=wide_w), dict(rows=1 << 31)):
        arena_sweep(refused(**kw))

    def overlapping(P):
        regs = [P(f"part{i}", m) for i, m in enumerate(mats)]
        return call_on(regs, regs[-1]), None

    arena_sweep(overlapping)

    def nothing(P):                                               # N = 0: a no-op
        regs = [P(f"part{i}", m) for i, m in enumerate(mats)]
        return call_on(regs, P("digest", shape=(n, 8)), rows=0), {}

    arena_sweep(nothing)


# ---- pai_sha256_expand --------------------------------------------------------------------------------------------------------------------
def expand_want(seed, tag, first, n, bits):
    ew = (bits + 31) // 32
    rows = []
    for j in range(n):
        d = hashlib.sha256(seed + tag + struct.pack("<Q", (first + j) % (1 << 64))).digest()
        rows.append(int.from_bytes(d[:4 * ew], "little") & ((1 << bits) - 1))
    return engine.ints_to_words(rows, ew)


@pytest.mark.parametrize("bits", (32, 100, 128, 256))
@pytest.mark.parametrize("n", (1, 65, 300))
def test_expand(bits, n, monkeypatch):
    h = handle()
    seed = hashlib.sha256(b"seed %d %d" % (bits, n)).digest()
    for tag, first in ((b"pai-rho", 0), (b"", 12345678901234), (b"fifteen-bytes-15", 7)):
        tag = tag[:15]
        got = engine.to_host_words(h.sha256_expand(seed, tag, first, n, bits))
        assert list(engine.profile_last()) == [EXPAND]
        assert np.array_equal(got, expand_want(seed, tag, first, n, bits)), (bits, n, tag)
    tune(monkeypatch, "sha_grid", 1)
    got = engine.to_host_words(h.sha256_expand(seed, b"pai-rho", 3, n, bits))
    assert np.array_equal(got, expand_want(seed, b"pai-rho", 3, n, bits))


def test_expand_carry_and_refusals():
    h = handle()
    seed = bytes(range(32))
    for first in ((1 << 32) - 3, (1 << 64) - 3):                  # the carry into the high word; the wrap modulo 2^64
        got = engine.to_host_words(h.sha256_expand(seed, b"pai-rho", first, 8, 128))
        assert np.array_equal(got, expand_want(seed, b"pai-rho", first, 8, 128)), first
    assert [int(x) for x in engine.words_to_ints(engine.to_host_words(h.sha256_expand(seed, b"pai-rho", 0, 5, 128)))] == th.rho(seed, 5)
    want = expand_want(seed, b"t", 0, 4, 128)
    for al in ALIGNS:
        ar = Arena("pattern")
        try:
            out = ar.place("e", shape=(4, 4), align=al)
            ar.commit()

            def call(tag_len=1, bits=128, ew=4, rows=4):
                return h.lib.pai_sha256_expand(h.h, seed, b"t" * 16, tag_len, 0, rows, bits, out.ptr, ew, None)

            for rc in (call(tag_len=16), call(tag_len=-1), call(bits=31), call(bits=257, ew=9), call(ew=3), call(rows=1 << 31)):
                assert rc == PAI_E_INVALID
            assert call(rows=0) == 0
            _native.check(h.lib.pai_stream_sync(0, None))
            ar.check({})
            _native.check(call())
            _native.check(h.lib.pai_stream_sync(0, None))
            ar.check({"e": want})
        finally:
            ar.free()


# ---- the protocol -------------------------------------------------------------------------------------------------------------------------
def container(pk, N, seed, packed=False):
    vals = [float(v) for v in np.random.default_rng(seed).integers(-1000, 1000, N)]
    if packed:
        return pk.encrypt_packed(vals, exponent=0, value_bits=16, slot_bits=32)
    return pk.encrypt(vals)


def rows_of(x):
    return engine.words_to_ints(engine.to_host_words(x.ciphertext().words))


def model_args(pk, vk, index):
    h = pk.pubkey.handle
    return (vk.n, h.key_bits, vk.parties, vk.threshold, index, vk.v, vk.values[index - 1])


@pytest.mark.parametrize("bits", (1024, 2048, 3072))
@pytest.mark.parametrize("N", (1, 5, 300))
def test_proof_is_the_integer_models(bits, N, monkeypatch):
    key, pk, sk = key_of(bits)
    tune(monkeypatch, "smexp_chunk", 64)                          # N = 300: several chunks and the segment combine
    shares = sk.share(3, 2, seed=bits, verifiable=True)
    assert [s.exponent() for s in shares] == [s.exponent() for s in sk.share(3, 2, seed=bits)]
    vk = shares[0].verification_key
    assert isinstance(vk, PaillierVerificationKey) and all(s.verification_key is vk for s in shares)
    assert vk.safe_primes == (bits == 1024) and vk.small_order_factor == th.small_order_factor(key.p, key.q)
    D, nsq = 6, key.n * key.n
    assert vk.values[1] == pow(vk.v, shares[1].exponent() // 2, nsq) and len(vk.values) == 3
    x = container(pk, N, bits + N)
    sh = shares[1]
    nonce = th.SeededRng(bits + N)(1 << th.nonce_bits(key.n, 3))
    part = sh.partial_decrypt(x, prove=True, _nonce=nonce)
    assert isinstance(part.proof, PaillierDecryptionProof)
    cts, prt = rows_of(x), engine.words_to_ints(part.host_words())
    want = th.prove_int(*model_args(pk, vk, 2)[:5], sh.exponent() // (2 * D), vk.v, vk.values[1], cts, prt, nonce)
    assert tuple(part.proof) == want
    assert pk.verify_partial(x, part, vk) is True
    if N == 5:
        assert th.verify_int(*model_args(pk, vk, 2), cts, prt, part.proof)
        fresh = sh.partial_decrypt(x, prove=True)                     # a nonce of its own
        assert fresh.proof != part.proof and pk.verify_partial(x, fresh, vk)
        assert th.verify_int(*model_args(pk, vk, 2), cts, prt, fresh.proof)
        assert sh.partial_decrypt(x).proof is None


@pytest.mark.parametrize("bits", (1024, 2048))
def test_rejections_through_the_api(bits):
    key, pk, sk = key_of(bits)
    shares = sk.share(3, 2, seed=bits + 1, verifiable=True)
    vk = shares[0].verification_key
    h = pk.pubkey.handle
    nsq = key.n * key.n
    x = container(pk, 6, bits)
    cts = rows_of(x)
    part = pickle.loads(pickle.dumps(shares[1].partial_decrypt(x, prove=True)))
    assert isinstance(part._t, np.ndarray) and pk.verify_partial(x, part, vk)
    prt = engine.words_to_ints(part.host_words())

    def variant(rows=None, proof=part.proof, index=2):
        p = pickle.loads(pickle.dumps(part))
        if rows is not None:
            p._t = engine.ints_to_words(rows, h.ct_words)
        p.proof, p.index = proof, index
        return p

    def both(p, cts_=cts, x_=x):
        got = pk.verify_partial(x_, p, vk)
        assert got == th.verify_int(*model_args(pk, vk, p.index), cts_, engine.words_to_ints(p.host_words()), p.proof)
        return got

    other = shares[2].partial_decrypt(x, prove=True)
    shifted = list(prt)
    shifted[3] = shifted[3] * pow(1 + key.n, 9, nsq) % nsq
    swapped = [prt[1], prt[0]] + prt[2:]
    a, b, z = part.proof
    B = th.nonce_bits(key.n, 3)
    assert both(other)                                            # honest under its own index ..
    assert not both(variant(rows=engine.words_to_ints(other.host_words())))            # .. and not under share 2's proof
    assert not both(variant(rows=engine.words_to_ints(other.host_words()), proof=other.proof))
    assert not both(variant(rows=shifted))
    assert not both(variant(rows=swapped))
    assert not both(variant(index=1))
    assert not both(variant(proof=PaillierDecryptionProof(a, b, z + (1 << (B + 1)))))
    assert not both(variant(proof=PaillierDecryptionProof(0, b, z)))
    assert not both(variant(proof=PaillierDecryptionProof(a, nsq, z)))
    assert not both(variant(rows=[prt[0] + nsq] + prt[1:]))
    # a cheater who proves over what it sends is caught by the relation, not by the transcript
    forged = variant(rows=shifted)
    forged.proof = PaillierDecryptionProof(*th.prove_int(*model_args(pk, vk, 2)[:5], shares[1].exponent() // 12, vk.v, vk.values[1], cts,
                                                         shifted, 12345))
    assert not both(forged)
    # a replay on another container; a negated row
    y = x + x
    assert not both(variant(rows=engine.words_to_ints(shares[1].partial_decrypt(y).host_words())), cts_=rows_of(y), x_=y)
    neg = [nsq - prt[0]] + prt[1:]
    negated = variant(rows=neg)
    negated.proof = PaillierDecryptionProof(*th.prove_int(*model_args(pk, vk, 2)[:5], shares[1].exponent() // 12, vk.v, vk.values[1], cts,
                                                          neg, 99))
    assert both(negated)
    assert pk.combine([shares[0].partial_decrypt(x), negated]) == sk.decrypt(x)
    # what is False without a look at the rows, and what raises
    assert not pk.verify_partial(x, variant(proof=None), vk)
    assert not pk.verify_partial(x[:5], part, vk)
    assert not pk.verify_partial(x, part, PaillierVerificationKey(vk.n, 3, 3, vk.v, vk.values))
    assert not pk.verify_partial(x, part, None)
    other_key = key_of(3072 if bits == 2048 else 2048)
    assert not other_key[1].verify_partial(other_key[1].encrypt([1.0] * 6), part, vk)
    with pytest.raises(ValueError, match="another key"):
        pk.verify_partial(other_key[1].encrypt([1.0] * 6), part, vk)
    with pytest.raises(TypeError):
        pk.verify_partial([1, 2, 3], part, vk)
    with pytest.raises(ValueError, match="verifiable"):
        sk.share(3, 2, seed=1)[0].partial_decrypt(x, prove=True)
    big = pickle.loads(pickle.dumps(x))
    w = big.ciphertext().words
    w[2] = engine.to_device_words(engine.ints_to_words([cts[2] + nsq], h.ct_words), w.device)[0]
    with pytest.raises(ValueError, match="residue"):
        pk.verify_partial(big, part, vk)
    with pytest.raises(ValueError, match="residue"):
        shares[1].partial_decrypt(big, prove=True)


def test_packed_container():
    key, pk, sk = key_of(2048)
    shares = sk.share(5, 3, seed=77, verifiable=True)
    vk = shares[0].verification_key
    packed = container(pk, 40, 3, packed=True)
    parts = [s.partial_decrypt(packed, prove=True) for s in shares[:3]]
    assert all(pk.verify_partial(packed, p, vk) for p in parts) and parts[0].packing is not None
    good, rejected = pk.verified_parts(packed, pickle.loads(pickle.dumps(parts)), vk)
    assert len(good) == 3 and rejected == []
    assert np.array_equal(pk.combine_packed(good), sk.decrypt_packed(packed))
    plain = container(pk, packed.ciphertext().words.shape[0], 4)
    assert not pk.verify_partial(plain, parts[0], vk)             # the shape of another container


def test_verified_parts():
    key, pk, sk = key_of(2048)
    shares = sk.share(5, 3, seed=5, verifiable=True)
    vk = shares[0].verification_key
    h = pk.pubkey.handle
    x = container(pk, 9, 31)
    parts = [s.partial_decrypt(x, prove=True) for s in shares]

    def tamper(p):
        rows = engine.words_to_ints(p.host_words())
        rows[4] = rows[4] * (1 + 3 * key.n) % (key.n * key.n)
        p._t = engine.to_device_words(engine.ints_to_words(rows, h.ct_words), h.device)

    tamper(parts[1])
    assert pk.combine_raw(parts[:3]) != sk.raw_decrypt(x)         # unverified: the wrong plaintext goes through
    good, rejected = pk.verified_parts(x, parts, vk)
    assert [p.index for p in good] == [1, 3, 4, 5] and rejected == [2]
    assert pk.combine(good) == sk.decrypt(x)
    tamper(parts[0])
    tamper(parts[4])
    good, rejected = pk.verified_parts(x, parts, vk)
    assert [p.index for p in good] == [3, 4] and rejected == [1, 2, 5]
    with pytest.raises(ValueError, match="threshold"):
        pk.combine(good)
