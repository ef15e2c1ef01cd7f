"""GPU: owner-side CRT encryption (csrc/dispatch_encrypt_crt.hpp) — PaillierPrivateKey.encrypt / encrypt_packed / apply_obfuscator
and the word-level ipclPrivateKey.encrypt_words / obfuscate_words_ return the bits of the public route for the same r.  Every case
profiles the call and asserts that the lift kernel ran where the route is expected and did NOT run where a fallback is: a silent
fallback cannot pass.  Tables are pinned to 6-bit windows and the route is forced with crtenc_min = 0."""
import numpy as np
import pytest
import torch

from oracle import paillier_oracle as orc
from pailliercryptolib_python_amd import PaillierPrivateKey, PaillierPublicKey, engine
from pailliercryptolib_python_amd.bindings import ipclPublicKey
from tests._util import disable, djn_obfuscate_many, tune
from tests.test_extreme_keys_cpu import load_extreme_keys
from tests.test_gpu_keysizes import make

pytestmark = pytest.mark.gpu

LIFT = "k_crt_lift"
SIZES = (1536, 2048, 3072, 4096, 4128)
_KEYS = {}


def keys(bits):
    if bits not in _KEYS:
        _KEYS[bits] = make(bits)
    return _KEYS[bits]


@pytest.fixture(autouse=True)
def forced(monkeypatch):
    tune(monkeypatch, "fb_digit_wbits", 6)
    tune(monkeypatch, "crtenc_min", 0)
    engine.profile_enable(True)
    yield
    engine.profile_enable(False)


def ran_lift():
    return LIFT in engine.profile_last()


def dev(h, ints, words):
    return engine.to_device_words(engine.ints_to_words(ints, words), h.device)


def ints(t):
    return engine.words_to_ints(engine.to_host_words(t))


@pytest.mark.parametrize("bits", SIZES)
def test_bits_against_oracle(bits):
    key, pk, sk = keys(bits)
    N = 37 if bits <= 2560 else 9
    vals = [float(v) for v in np.random.default_rng(bits).uniform(-1000, 1000, N)]
    r = orc.synth_r_limbs(bits, N, key.randbits)
    en = sk.encrypt(vals, r=r)
    assert ran_lift()
    want_ct, want_e = orc.api_encrypt(key, vals, orc.limbs_to_ints(r))
    assert [int(c) for c in en.ciphertextBN()] == want_ct and en.exponent() == want_e
    assert en.public_key == pk
    assert sk.decrypt(en) == vals


@pytest.mark.parametrize("bits", SIZES)
def test_shapes_against_public_route(bits):
    key, pk, sk = keys(bits)
    h = pk.pubkey.handle
    rng = np.random.default_rng(bits + 1)
    for N in (1, 63, 64, 65, 130):
        m = dev(h, [int.from_bytes(rng.bytes(bits // 8 + 8), "little") % key.n for _ in range(N)], h.n_words)
        r = engine.to_device_words(orc.synth_r_limbs(bits + N, N, key.randbits), h.device)
        got = sk.prikey.encrypt_words(m, r)
        assert ran_lift()
        assert torch.equal(got, pk.pubkey.encrypt_words(m, True, r)), N
        assert not ran_lift()


@pytest.mark.parametrize("bits", SIZES)
def test_corner_operands(bits):
    key, pk, sk = keys(bits)
    h = pk.pubkey.handle
    n, p, q = key.n, min(key.p, key.q), max(key.p, key.q)
    ms = [0, 1, n - 1, p, q, (n - 1) // p * p]               # s | m: the per-prime residue of the message factor is 1
    rs = [0, 1, (1 << key.randbits) - 1]
    mm = [m for m in ms for _ in rs]
    rr = [r for _ in ms for r in rs]
    m, r = dev(h, mm, h.n_words), dev(h, rr, h.r_words)
    got = sk.prikey.encrypt_words(m, r)
    assert ran_lift()
    assert torch.equal(got, pk.pubkey.encrypt_words(m, True, r))
    gi = ints(got)
    assert gi[0] == 1                                       # m = 0, r = 0: ct = 1, c_q - c_p = 0 in the lift
    for i in (1, 5, 9):                                     # (0, 1), (1, 2^randbits - 1), (p, 0)
        assert gi[i] == orc.encrypt(key, mm[i], rr[i])


def test_extreme_keys():
    served = skipped = 0
    for ident, family, b, p, q in load_extreme_keys():
        key = orc.make_key(p, q, djn_x=0xABCDEF1234567, bits=2 * b)
        pk = PaillierPublicKey(ipclPublicKey(key.n, 2 * b, True, hs=key.hs, randbits=key.randbits))
        sk = PaillierPrivateKey(pk, p, q)
        h = pk.pubkey.handle
        rng = np.random.default_rng(b)
        mm = [0, key.n - 1] + [int.from_bytes(rng.bytes(b // 4 + 8), "little") % key.n for _ in range(3)]
        rr = [(1 << key.randbits) - 1, 1] + orc.limbs_to_ints(orc.synth_r_limbs(b, 3, key.randbits))
        got = sk.prikey.encrypt_words(dev(h, mm, h.n_words), dev(h, rr, h.r_words))
        if not ran_lift():
            skipped += 1
            assert b in (512, 676), ident                   # primes outside 700..1024 / 1400..2068 bits: the public route
        else:
            served += 1
        assert ints(got) == [orc.encrypt(key, m, r) for m, r in zip(mm, rr)], ident
    print(f"extreme keys: {served} served by the CRT route, {skipped} skipped as not served")
    assert served > 0


@pytest.mark.parametrize("bits", (2048, 3072))
def test_apply_obfuscator(bits):
    key, pk, sk = keys(bits)
    N = 9
    vals = [float(v) for v in np.random.default_rng(5).uniform(-10, 10, N)]
    r0, r1 = orc.synth_r_limbs(1, N, key.randbits), orc.synth_r_limbs(2, N, key.randbits)
    en = pk.encrypt(vals, r=r0)
    before = [int(c) for c in en.ciphertextBN()]
    sk.apply_obfuscator(en, r=engine.to_device_words(r1, pk.pubkey.handle.device))
    assert ran_lift()
    assert [int(c) for c in en.ciphertextBN()] == djn_obfuscate_many(key, before, orc.limbs_to_ints(r1))
    assert sk.decrypt(en) == vals
    pkd = pk.encrypt_packed(np.arange(N, dtype=np.float64), exponent=8, value_bits=24, slot_bits=64)
    G = pkd.rows
    before = [int(c) for c in pkd.ciphertext().getTexts()]
    sk.apply_obfuscator(pkd, r=engine.to_device_words(r1[:G], pk.pubkey.handle.device))
    assert ran_lift()
    assert [int(c) for c in pkd.ciphertext().getTexts()] == djn_obfuscate_many(key, before, orc.limbs_to_ints(r1[:G]))


@pytest.mark.parametrize("bits", (2048, 3072))
def test_encrypt_packed(bits):
    key, pk, sk = keys(bits)
    x = np.random.default_rng(9).uniform(-100, 100, 70)
    kw = dict(exponent=10, value_bits=30, slot_bits=64)
    G = pk.encrypt_packed(x, apply_obfuscator=False, **kw).rows
    r = engine.to_device_words(orc.synth_r_limbs(3, G, key.randbits), pk.pubkey.handle.device)
    a = sk.encrypt_packed(x, r=r, **kw)
    assert ran_lift()
    b = pk.encrypt_packed(x, r=r, **kw)
    assert [int(c) for c in a.ciphertext().getTexts()] == [int(c) for c in b.ciphertext().getTexts()]
    assert np.array_equal(sk.decrypt_packed(a), sk.decrypt_packed(b))
    assert np.allclose(sk.decrypt_packed(a), x, atol=2.0 ** -10)


def test_fallbacks(monkeypatch):
    def same_no_lift(key, pk, sk, N=9):
        h = pk.pubkey.handle
        m = dev(h, list(range(N)), h.n_words)
        rr = orc.synth_r_limbs(N, N, key.randbits) if key.randbits else engine.ints_to_words(list(range(2, N + 2)), h.r_words)
        r = engine.to_device_words(rr, h.device)
        got = sk.prikey.encrypt_words(m, r)
        assert not ran_lift()
        assert torch.equal(got, pk.pubkey.encrypt_words(m, True, r))

    same_no_lift(*make(512))                                  # 256-bit primes: no digit-engine instantiation
    key = keys(2048)[0]
    std = orc.make_key(key.p, key.q, bits=2048)               # standard scheme
    pk_std = PaillierPublicKey(ipclPublicKey(std.n, 2048, False))
    same_no_lift(std, pk_std, PaillierPrivateKey(pk_std, key.p, key.q))
    disable(monkeypatch, "crtenc")
    same_no_lift(*keys(2048))
    disable(monkeypatch, "crtenc", False)
    tune(monkeypatch, "crtenc_min", 100)
    same_no_lift(*keys(2048))                                 # N = 9 below the hand-over edge
    tune(monkeypatch, "crtenc_min", 0)
    h = keys(2048)[1].pubkey.handle
    m, r = dev(h, [5], h.n_words), engine.to_device_words(orc.synth_r_limbs(1, 1, key.randbits), h.device)
    keys(2048)[2].prikey.encrypt_words(m, r)
    assert ran_lift()                                         # ... and the route is back once the knobs are


def test_tables_trim_and_eviction(monkeypatch):
    ka, pka, ska = keys(2048)
    kb, pkb, skb = keys(1536)

    def enc(key, pk, sk):
        h = pk.pubkey.handle
        m = dev(h, [3, key.n - 2, 77], h.n_words)
        r = engine.to_device_words(orc.synth_r_limbs(4, 3, key.randbits), h.device)
        got = sk.prikey.encrypt_words(m, r)
        assert ran_lift()
        return ints(got), [orc.encrypt(key, a, b) for a, b in zip([3, key.n - 2, 77], orc.limbs_to_ints(orc.synth_r_limbs(4, 3, key.randbits)))]

    got, want = enc(ka, pka, ska)
    assert got == want and ska.prikey.handle.crt_table_info()["bytes"] > 0
    pka.pubkey.handle.trim()
    assert ska.prikey.handle.crt_table_info()["bytes"] == 0
    got2, _ = enc(ka, pka, ska)                               # rebuilt: the same bits
    assert got2 == want and ska.prikey.handle.crt_table_info()["bytes"] > 0
    pka.pubkey.handle.trim()
    pkb.pubkey.handle.trim()
    monkeypatch.setenv("PAI_FB_CACHE_MB", "8")                # 6 MB (2048 bits) + 4.5 MB (1536 bits) of 6-bit tables do not fit together
    for key, pk, sk in ((ka, pka, ska), (kb, pkb, skb), (ka, pka, ska)):
        got, want = enc(key, pk, sk)
        assert got == want
    assert skb.prikey.handle.crt_table_info()["bytes"] == 0   # B's tables went when A's came back


def test_interplay():
    key, pk, sk = keys(2048)
    a, b = [1.5, -2.25, 100.0], [0.5, 4.0, -7.0]
    ea = sk.encrypt(a)
    assert ran_lift()
    s = ea + pk.encrypt(b)
    assert np.allclose(sk.decrypt(s), np.add(a, b))
