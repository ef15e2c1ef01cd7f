"""GPU: PaillierEncryptedNumber.cumsum (pai_ct_scan / k_segscan) bit for bit against CPython's pow on the ciphertexts, against
sum() on slices, with forced chunk lengths (the three-phase levels), on lazily tagged inputs, through its consumers (+, pack,
pickling), through the raw C ABI, and at full size through decryption."""
import json
import pickle
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import paillier_oracle as orc
from pailliercryptolib_python_amd import PaillierPrivateKey, PaillierPublicKey, engine, fixedpoint
from pailliercryptolib_python_amd.bindings import ipclCipherText, ipclPublicKey
from pailliercryptolib_python_amd.paillier import PaillierEncryptedNumber

from ._util import rand_below, tune

pytestmark = pytest.mark.gpu

_KEYS = {}


def keypair(bits):
    if bits not in _KEYS:
        fx = json.loads((Path(__file__).parent / "golden" / "fixture_keys.json").read_text())[str(bits)]
        key = orc.make_key(int(fx["p"], 16), int(fx["q"], 16), djn_x=(1 << 70) + 12345, bits=bits)
        pk = PaillierPublicKey(ipclPublicKey(key.n, bits, True, hs=key.hs, randbits=key.randbits))
        _KEYS[bits] = (key, pk, PaillierPrivateKey(pk, key.p, key.q))
    return _KEYS[bits]


def random_container(pk, key, n, expo, seed):
    """n random residues modulo n^2 as ciphertexts (the product is what is checked), with the given exponents."""
    cts = rand_below(np.random.default_rng(seed), key.nsq, n)
    return PaillierEncryptedNumber(pk, ipclCipherText(pk.pubkey, cts), expo, n), cts


def mixed_expo(n, seed):
    """exponents of floats, negatives and integers mixed"""
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.standard_normal(n // 3) * 100, -rng.random(n // 3), rng.integers(-50, 50, n - 2 * (n // 3)).astype(float)])
    rng.shuffle(x)
    _, expo = fixedpoint.float64_mantissas(x)
    return np.asarray(expo, dtype=np.int32)


def want_chain(cts, raise_, step, L, reverse, nsq):
    """pai_ct_scan's definition with CPython's pow: acc_i = acc_prev^(2^step_i) * ct_i^(2^raise_i) along each run"""
    N = len(cts)
    out = [None] * N
    for base in range(0, N, L):
        acc = None
        for p in range(L):
            i = base + (L - 1 - p if reverse else p)
            v = pow(cts[i], 1 << int(raise_[i]), nsq)
            acc = v if p == 0 else pow(acc, 1 << int(step[i]), nsq) * v % nsq
            out[i] = acc
    return out


def want_cumsum(cts, expo, L, reverse, nsq):
    """out[i] = prod_j ct_j^(2^(E_i - e_j)) over the prefix of i, E_i its largest exponent: walked as a chain (the residue is the
    same), and recomputed from the formula itself on a spread of elements"""
    N = len(cts)
    E = np.zeros(N, dtype=np.int64)
    for base in range(0, N, L):
        run = np.asarray(expo[base:base + L], dtype=np.int64)
        E[base:base + L] = np.maximum.accumulate(run[::-1])[::-1] if reverse else np.maximum.accumulate(run)
    step = np.zeros(N, dtype=np.int64)
    prev = np.arange(N) + (1 if reverse else -1)
    inner = np.arange(N) % L != (L - 1 if reverse else 0)
    step[inner] = E[inner] - E[prev[inner]]
    out = want_chain(cts, E - np.asarray(expo, dtype=np.int64), step, L, reverse, nsq)
    for i in sorted({int(v) for v in np.linspace(0, N - 1, 5)}):
        a = i - i % L
        acc = 1
        for j in (range(i, a + L) if reverse else range(a, i + 1)):
            acc = acc * pow(cts[j], 1 << int(E[i] - expo[j]), nsq) % nsq
        assert out[i] == acc
    return out, [int(e) for e in E]


@pytest.mark.parametrize("bits", [1024, 2048, 3072, 4096])
def test_cumsum_bit_exact(bits):
    key, pk, _ = keypair(bits)
    n = 602                                                          # 7 * 86
    expo = mixed_expo(n, bits)
    assert len(set(expo.tolist())) > 3
    x, cts = random_container(pk, key, n, expo, bits + 1)
    for L in (1, 7, n):
        for reverse in (False, True):
            got = x.cumsum(L, reverse=reverse)
            want, want_e = want_cumsum(cts, expo, L, reverse, key.nsq)
            assert len(got) == n
            assert got.exponent() == want_e, (L, reverse)
            assert [int(c) for c in got.ciphertextBN()] == want, (L, reverse)
    one = x.cumsum()                                                 # None: one run of n
    assert [int(c) for c in one.ciphertextBN()] == want_cumsum(cts, expo, n, False, key.nsq)[0]


def test_cumsum_matches_sum_of_slices():
    key, pk, _ = keypair(2048)
    n, L = 1500, 300
    x, _ = random_container(pk, key, n, mixed_expo(n, 8), 9)
    fwd, rev = x.cumsum(L), x.cumsum(L, reverse=True)
    for i in (0, 1, 2, 57, 299, 300, 301, 777, 1199, 1200, 1498, 1499):
        a = i - i % L
        ref = x[a:i + 1].sum()
        assert int(fwd.ciphertextBN(i)) == int(ref.ciphertextBN(0)) and fwd.exponent(i) == ref.exponent(0)
        ref = x[i:a + L].sum()
        assert int(rev.ciphertextBN(i)) == int(ref.ciphertextBN(0)) and rev.exponent(i) == ref.exponent(0)
    # not re-randomised: a run's first element is the input element itself
    assert int(fwd.ciphertextBN(300)) == int(x.ciphertextBN(300)) and int(rev.ciphertextBN(299)) == int(x.ciphertextBN(299))


@pytest.mark.parametrize("chunk", [1, 2, 3, 5])
def test_forced_chunks_match_default(monkeypatch, chunk):
    key, pk, _ = keypair(2048)
    n = 1001                                                         # one run: at chunk 2 the totals are scanned over nine levels
    expo = mixed_expo(n, 11)
    x, cts = random_container(pk, key, n, expo, 12)
    for reverse in (False, True):
        tune(monkeypatch, "scan_chunk", None)
        base = x.cumsum(reverse=reverse)
        tune(monkeypatch, "scan_chunk", chunk)
        got = x.cumsum(reverse=reverse)
        want, want_e = want_cumsum(cts, expo, n, reverse, key.nsq)
        assert [int(c) for c in got.ciphertextBN()] == [int(c) for c in base.ciphertextBN()]
        assert got.exponent() == base.exponent() == want_e
        assert [int(c) for c in got.ciphertextBN()] == want
    # several runs, chunked (143 = 11 * 13 is no multiple of the chunk: ragged last chunks)
    tune(monkeypatch, "scan_chunk", chunk)
    got = x.cumsum(143)
    assert [int(c) for c in got.ciphertextBN()] == want_cumsum(cts, expo, 143, False, key.nsq)[0]


def test_lazy_tag_inputs():
    key, pk, _ = keypair(2048)
    n, L = 1 << 14, 64                                 # beyond the small-batch range, where a + b returns the wire form at once
    expo = mixed_expo(n, 14)
    a, _ = random_container(pk, key, n, expo, 15)
    b, _ = random_container(pk, key, n, expo, 16)
    lazy = a + b
    assert lazy.ciphertext()._raw()[1] != 0            # the sum is held at a domain tag (no wire-form copy)
    wire_cts = [int(c) * int(d) % key.nsq for c, d in zip(a.ciphertextBN(), b.ciphertextBN())]
    got = lazy.cumsum(L)
    assert got.ciphertext()._raw()[1] == 1             # the result is held at tag 1 ...
    want, want_e = want_cumsum(wire_cts, expo, L, False, key.nsq)
    assert [int(c) for c in got.ciphertextBN()] == want and got.exponent() == want_e       # ... and read in the wire form


def test_output_consumers_see_the_wire_form():
    key, pk, sk = keypair(2048)
    n, L = 96, 32
    expo = mixed_expo(n, 17)
    x, cts = random_container(pk, key, n, expo, 18)
    want, want_e = want_cumsum(cts, expo, L, False, key.nsq)

    def wire():
        return PaillierEncryptedNumber(pk, ipclCipherText(pk.pubkey, want), want_e, n)

    y, _ = random_container(pk, key, n, expo, 19)
    c = x.cumsum(L)
    assert c.ciphertext()._raw()[1] == 1
    s, ref = c + y, wire() + y                         # + on the tagged result
    assert [int(v) for v in s.ciphertextBN()] == [int(v) for v in ref.ciphertextBN()] and s.exponent() == ref.exponent()
    c = x.cumsum(L)
    q = pickle.loads(pickle.dumps(c))                  # pickling
    assert [int(v) for v in q.ciphertextBN()] == want and q.exponent() == want_e
    c = x.cumsum(L)
    E = max(want_e)
    p, pref = c.pack(slot_bits=64, value_bits=60, exponent=E), wire().pack(slot_bits=64, value_bits=60, exponent=E)
    assert [int(v) for v in p.ciphertext().getTexts()] == [int(v) for v in pref.ciphertext().getTexts()]
    c = x.cumsum(L)
    sl = c[5:9]                                        # a slice keeps the tag and resolves it when read
    assert [int(v) for v in sl.ciphertextBN()] == want[5:9]
    # decryption of a tagged result: real ciphertexts
    v = np.arange(-20, 20, dtype=np.float64)
    assert np.array_equal(np.asarray(sk.decrypt(pk.encrypt(v).cumsum(8)), dtype=np.float64), np.cumsum(v.reshape(-1, 8), axis=1).reshape(-1))


def dev_words(h, ints):
    return engine.to_device_words(engine.ints_to_words(ints, h.ct_words), h.device)


def test_raw_abi_arbitrary_counts_tags_and_guards(monkeypatch):
    key, pk, _ = keypair(1024)
    h = pk.pubkey.handle
    nsq = key.nsq
    rng = np.random.default_rng(23)
    n, L = 120, 40
    cts = rand_below(rng, nsq, n)
    raise_ = rng.integers(0, 4, n).astype(np.int32)
    step = rng.integers(0, 4, n).astype(np.int32)
    assert ((raise_ != 0) & (step != 0)).any()
    d_raise, d_step = torch.from_numpy(raise_).to(h.device), torch.from_numpy(step).to(h.device)
    ct = dev_words(h, cts)
    # R mod n^2 from the library's own Montgomery product: mont_mul(a, 1) = a R^-1
    rinv = engine.words_to_ints(engine.to_host_words(h.ct_mont_mul(dev_words(h, [1]), dev_words(h, [1]))))[0]
    R = pow(rinv, -1, nsq)
    for chunk in (None, 3):
        tune(monkeypatch, "scan_chunk", chunk)
        for reverse in (False, True):
            want = want_chain(cts, raise_, step, L, reverse, nsq)
            for tag in (0, 1, -2):
                tagged = dev_words(h, [c * pow(R, tag, nsq) % nsq for c in cts])
                for dom in (0, 1):
                    out = h.ct_scan(tagged, L, tag=tag, dom_out=dom, reverse=reverse, raise_=d_raise, step=d_step)
                    got = engine.words_to_ints(engine.to_host_words(out))
                    assert got == [w * pow(R, dom, nsq) % nsq for w in want], (chunk, reverse, tag, dom)
    tune(monkeypatch, "scan_chunk", None)
    # no counts at all: plain prefix products
    got = engine.words_to_ints(engine.to_host_words(h.ct_scan(ct, L, tag=0, dom_out=0)))
    assert got == want_chain(cts, np.zeros(n, int), np.zeros(n, int), L, False, nsq)
    # seg_len that does not divide N
    with pytest.raises(engine._native.NativeError) as ei:
        h.ct_scan(ct, 7)
    assert ei.value.code == engine._native.PAI_E_INVALID
    with pytest.raises(engine._native.NativeError):
        h.ct_scan(ct, 0)
    # negative counts are taken as 0 and set bit 4 of the status word
    h.check_status(force=True)
    bad_r, bad_s = raise_.copy(), step.copy()
    bad_r[5], bad_s[50] = -2, -1
    out = h.ct_scan(ct, L, tag=0, dom_out=0, raise_=torch.from_numpy(bad_r).to(h.device), step=torch.from_numpy(bad_s).to(h.device))
    ok_r, ok_s = np.maximum(bad_r, 0), np.maximum(bad_s, 0)
    assert engine.words_to_ints(engine.to_host_words(out)) == want_chain(cts, ok_r, ok_s, L, False, nsq)
    with pytest.raises(engine._native.NativeError, match="ct_scan"):
        h.check_status(force=True)
    h.check_status(force=True)                                       # read and cleared: nothing pending any more
    # the step of a run's first row is never applied; a negative value there is still counted (bit 4), a positive one is not
    want = want_chain(cts, raise_, step, L, False, nsq)
    for garbage, flagged in ((-9, True), (1 << 20, False)):
        first_s = step.copy()
        first_s[0] = garbage
        out = h.ct_scan(ct, L, tag=0, dom_out=0, raise_=d_raise, step=torch.from_numpy(first_s).to(h.device))
        assert engine.words_to_ints(engine.to_host_words(out)) == want, garbage
        if flagged:
            with pytest.raises(engine._native.NativeError, match="ct_scan"):
                h.check_status(force=True)
        h.check_status(force=True)


@pytest.mark.parametrize("L", [256, 65536])
def test_full_size_decrypts_to_numpy_cumsum(L):
    key, pk, sk = keypair(2048)
    n = 65536
    rng = np.random.default_rng(29)
    xi = rng.integers(-(1 << 20), 1 << 20, n).astype(np.float64)
    xf = rng.integers(-(1 << 20), 1 << 20, n).astype(np.float64) / 1024.0       # multiples of 2^-10: the sums are exact in float64
    for x in (xi, xf):
        enc = pk.encrypt(x)
        for reverse in (False, True):
            got = np.asarray(sk.decrypt(enc.cumsum(L, reverse=reverse)), dtype=np.float64)
            runs = x.reshape(-1, L)
            want = np.cumsum(runs[:, ::-1], axis=1)[:, ::-1] if reverse else np.cumsum(runs, axis=1)
            assert np.array_equal(got, want.reshape(-1)), (L, reverse)


def test_pipeline_segment_sum_cumsum_pack():
    key, pk, sk = keypair(2048)
    rng = np.random.default_rng(31)
    n, F, K = 4000, 3, 32
    g = rng.integers(-(1 << 16), 1 << 16, n).astype(np.float64) / 256.0
    ids = rng.integers(0, K, (n, F))
    h = pk.encrypt(g).segment_sum(ids, K)
    c = h.cumsum(K)
    hist = np.stack([np.bincount(ids[:, f], weights=g, minlength=K) for f in range(F)])
    want = np.cumsum(hist, axis=1).reshape(-1)                       # exact: multiples of 2^-8 far below 2^53
    E = max(c.exponent())
    ints = [int(Fraction(float(w)) * Fraction(2) ** E) for w in want]
    assert all(Fraction(m) == Fraction(float(w)) * Fraction(2) ** E for m, w in zip(ints, want))
    # a float's exponent leaves room for its 53 significant bits, so the aligned mantissas pass 64 bits: 100-bit slots
    p = c.pack(slot_bits=100, value_bits=max(1, max(abs(w) for w in ints).bit_length()))
    assert sk.decrypt_packed_mantissas(p) == ints
    assert np.array_equal(sk.decrypt_packed(p), want)
    assert np.array_equal(np.asarray(sk.decrypt(c), dtype=np.float64), want)


def test_argument_errors_and_empty_container():
    key, pk, _ = keypair(1024)
    x, _ = random_container(pk, key, 12, np.zeros(12, np.int32), 1)
    for bad in (5, 24, 0, -3):
        with pytest.raises(ValueError):
            x.cumsum(bad)
    for bad in (2.0, True, "3"):
        with pytest.raises(TypeError):
            x.cumsum(bad)
    e, _ = random_container(pk, key, 0, np.zeros(0, np.int32), 2)
    for L in (None, 4):
        got = e.cumsum(L)
        assert isinstance(got, PaillierEncryptedNumber) and len(got) == 0 and got.exponent() == []
