"""GPU: PaillierEncryptedNumber.segment_sum (pai_ct_segment_prod / k_segprod) bit for bit against CPython's pow on the
ciphertexts, against sum() on slices, with forced chunk lengths (the multi-level path), on lazily tagged inputs, and at full
size through decryption."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import paillier_oracle as orc
from pailliercryptolib_python_amd import PaillierPrivateKey, PaillierPublicKey, engine
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


def want_segments(cts, expo, ids, K, nsq):
    ids = np.asarray(ids).reshape(len(cts), -1)
    N, F = ids.shape
    emin = int(min(expo)) if N else 0
    out, ex = [], []
    for f in range(F):
        for b in range(K):
            mem = np.nonzero(ids[:, f] == b)[0]
            if len(mem) == 0:
                out.append(1)
                ex.append(emin)
                continue
            E = int(max(expo[i] for i in mem))
            acc = 1
            for i in mem:
                acc = acc * pow(cts[i], 1 << (E - int(expo[i])), nsq) % nsq
            out.append(acc)
            ex.append(E)
    return out, ex


def mixed_case(n, F, K, seed):
    """ids with dropped pairs and empty segments; exponents of floats, negatives and integers mixed"""
    rng = np.random.default_rng(seed)
    ids = rng.integers(-1, K - 2, (n, F))                           # ids K-2, K-1 never occur
    x = np.concatenate([rng.standard_normal(n // 3) * 100, -rng.random(n // 3), rng.integers(-50, 50, n - 2 * (n // 3)).astype(float)])
    from pailliercryptolib_python_amd import fixedpoint
    _, expo = fixedpoint.float64_mantissas(x)
    return ids, np.asarray(expo, dtype=np.int32)


@pytest.mark.parametrize("bits", [1024, 2048, 3072, 4096])
def test_segment_sum_bit_exact(bits):
    key, pk, _ = keypair(bits)
    n, F, K = 2000, 3, 11
    ids, expo = mixed_case(n, F, K, bits)
    x, cts = random_container(pk, key, n, expo, bits + 1)
    got = x.segment_sum(torch.from_numpy(ids).cuda(), K)
    want, want_e = want_segments(cts, expo, ids, K, key.nsq)
    assert len(got) == F * K
    assert got.exponent() == want_e
    assert [int(c) for c in got.ciphertextBN()] == want


def test_segment_sum_matches_sum_of_slices():
    key, pk, _ = keypair(2048)
    n, K = 1500, 6
    rng = np.random.default_rng(7)
    ids = np.sort(rng.integers(0, K, n))
    _, expo = mixed_case(n, 1, K, 8)
    x, _ = random_container(pk, key, n, expo, 9)
    got = x.segment_sum(ids, K)
    bounds = np.searchsorted(ids, np.arange(K + 1))
    for s in range(K):
        a, b = int(bounds[s]), int(bounds[s + 1])
        if a == b:
            continue
        ref = x[a:b].sum()
        assert int(got.ciphertextBN(s)) == int(ref.ciphertextBN(0)) and got.exponent(s) == ref.exponent(0)


@pytest.mark.parametrize("chunk", [1, 2, 3])
def test_forced_chunks_match_default(monkeypatch, chunk):
    key, pk, _ = keypair(2048)
    n, F, K = 1200, 2, 5
    rng = np.random.default_rng(10)
    ids = np.where(rng.random((n, F)) < 0.9, 1, rng.integers(-1, K, (n, F)))      # one segment per feature holds 90 % of the rows
    _, expo = mixed_case(n, 1, K, 11)
    x, cts = random_container(pk, key, n, expo, 12)
    base = x.segment_sum(ids, K)
    tune(monkeypatch, "segprod_chunk", chunk)
    got = x.segment_sum(ids, K)
    assert [int(c) for c in got.ciphertextBN()] == [int(c) for c in base.ciphertextBN()]
    assert got.exponent() == base.exponent()
    if chunk == 2:
        want, want_e = want_segments(cts, expo, ids, K, key.nsq)
        assert [int(c) for c in got.ciphertextBN()] == want and got.exponent() == want_e


def test_lazy_tag_inputs():
    key, pk, _ = keypair(2048)
    n, K = 1 << 14, 4                                  # beyond the small-batch range, where a + b returns the wire form at once
    rng = np.random.default_rng(13)
    _, expo = mixed_case(n, 1, K, 14)
    a, _ = random_container(pk, key, n, expo, 15)
    b, _ = random_container(pk, key, n, expo, 16)
    lazy = a + b
    assert lazy.ciphertext()._raw()[1] != 0            # the sum is held at a domain tag (no wire-form copy)
    ids = rng.integers(-1, K, n)
    got = lazy.segment_sum(ids, K)
    wire = PaillierEncryptedNumber(pk, ipclCipherText(pk.pubkey, [int(c) for c in lazy.ciphertextBN()]), lazy._expo, n)
    ref = wire.segment_sum(ids, K)
    assert [int(c) for c in got.ciphertextBN()] == [int(c) for c in ref.ciphertextBN()] and got.exponent() == ref.exponent()


def test_bad_rows_and_negative_shifts_are_guarded():
    """pai_ct_segment_prod with a member row >= N and a negative shift (input the Python plan never produces): the kernel skips
    the row, takes the shift as 0, sets bit 2 of the handle's status word, and the other members give their product."""
    key, pk, _ = keypair(1024)
    h = pk.pubkey.handle
    h.check_status(force=True)                                       # a clean status word before the call
    _, cts = random_container(pk, key, 3, np.zeros(3, np.int32), 21)
    ct = engine.to_device_words(engine.ints_to_words(cts, h.ct_words), h.device)
    dev = h.device
    rows = torch.tensor([0, 7, 1, 2, 1 << 30, 2], dtype=torch.int64).to(torch.int32).to(dev)
    shift = torch.tensor([0, 0, -3, 1, 0, 0], dtype=torch.int32, device=dev)
    offsets = torch.tensor([0, 4, 6], dtype=torch.int64, device=dev)
    out = h.ct_segment_prod(ct, rows, shift, offsets)
    got = engine.words_to_ints(engine.to_host_words(out))
    nsq = key.nsq
    # segment 0: ct0, (row 7 skipped), ct1 with its shift -3 taken as 0, then ct2 after one squaring; segment 1: ct2 alone
    assert got == [pow(cts[0] * cts[1] % nsq, 2, nsq) * cts[2] % nsq, cts[2]]
    with pytest.raises(engine._native.NativeError, match="ct_segment_prod"):
        h.check_status(force=True)
    h.check_status(force=True)                                       # read and cleared: nothing pending any more


@pytest.mark.parametrize("chunk", [None, 2])
def test_bad_rows_and_negative_shifts_across_levels(monkeypatch, chunk):
    """The guarded input in a chain that is cut into chunks (found by tests/test_gpu_fuzz_ext.py, segprod round 1): a chunk hands
    the SUM of its members' shifts to the next level, and that sum must hold what a single chain applies — 0 for a negative shift,
    nothing for a skipped row.  Members: ct0, ct1 << 1 | (row 9, shift 5: skipped), ct2 with shift -3 | ct1 << 2, ct0 with shift -1."""
    key, pk, _ = keypair(1024)
    h = pk.pubkey.handle
    h.check_status(force=True)
    _, cts = random_container(pk, key, 3, np.zeros(3, np.int32), 22)
    ct = engine.to_device_words(engine.ints_to_words(cts, h.ct_words), h.device)
    rows, shift = [0, 1, 9, 2, 1, 0], [0, 1, 5, -3, 2, -1]
    nsq, acc = key.nsq, None
    for r, s in zip(rows, shift):
        if r < 3:
            acc = cts[r] if acc is None else pow(acc, 1 << max(s, 0), nsq) * cts[r] % nsq
    tune(monkeypatch, "segprod_chunk", chunk)
    out = h.ct_segment_prod(ct, torch.tensor(rows, dtype=torch.int32, device=h.device), torch.tensor(shift, dtype=torch.int32, device=h.device),
                            torch.tensor([0, 6], dtype=torch.int64, device=h.device))
    assert engine.words_to_ints(engine.to_host_words(out)) == [acc]
    with pytest.raises(engine._native.NativeError, match="ct_segment_prod"):
        h.check_status(force=True)
    h.check_status(force=True)


@pytest.mark.parametrize("chunk", [None, 2])
def test_first_shift_is_never_applied_and_its_sign_is_counted(monkeypatch, chunk):
    """The shift of a chain's first member is not applied, whatever it holds; a NEGATIVE value there still sets bit 2 of the status
    word (include/paillier_hip.h), a positive one does not — in one chain and in a chain cut into chunks."""
    key, pk, _ = keypair(1024)
    h = pk.pubkey.handle
    h.check_status(force=True)
    _, cts = random_container(pk, key, 5, np.zeros(5, np.int32), 23)
    ct = engine.to_device_words(engine.ints_to_words(cts, h.ct_words), h.device)
    nsq = key.nsq
    want = [pow(pow(pow(cts[0], 2, nsq) * cts[1] % nsq * cts[2] % nsq, 8, nsq) * cts[3] % nsq, 2, nsq) * cts[4] % nsq, cts[2]]
    tune(monkeypatch, "segprod_chunk", chunk)
    for garbage, flagged in ((-5, True), (1 << 20, False)):
        shift = torch.tensor([garbage, 1, 0, 3, 1, garbage], dtype=torch.int32, device=h.device)
        out = h.ct_segment_prod(ct, torch.tensor([0, 1, 2, 3, 4, 2], dtype=torch.int32, device=h.device), shift,
                                torch.tensor([0, 5, 6], dtype=torch.int64, device=h.device))
        assert engine.words_to_ints(engine.to_host_words(out)) == want, garbage
        if flagged:
            with pytest.raises(engine._native.NativeError, match="ct_segment_prod"):
                h.check_status(force=True)
        h.check_status(force=True)


def test_empty_input_and_empty_bins():
    key, pk, _ = keypair(1024)
    x, _ = random_container(pk, key, 0, np.zeros(0, np.int32), 1)
    got = x.segment_sum(np.zeros((0, 2), dtype=np.int64), 3)
    assert [int(c) for c in got.ciphertextBN()] == [1] * 6 and got.exponent() == [0] * 6


def test_full_size_decrypts_to_bincount():
    key, pk, sk = keypair(2048)
    n, F, K = 1 << 18, 2, 64
    rng = np.random.default_rng(17)
    g = rng.standard_normal(n)
    ids = rng.integers(0, K, (n, F))
    x = pk.raw_encrypt(g)
    got = x.segment_sum(torch.from_numpy(ids).cuda(), K)
    expo = np.asarray(x.exponent(), dtype=np.int64)
    mant = [int(v) for v in np.ldexp(g, expo)]                      # the encoded mantissas (exact: |mantissa| < 2^53)
    ge = got.exponent()
    raw = sk.raw_decrypt(got)
    for s in range(F * K):
        f, b = divmod(s, K)
        mem = np.nonzero(ids[:, f] == b)[0]
        assert ge[s] == int(expo[mem].max())
        assert int(raw[s]) == sum(mant[i] << (ge[s] - int(expo[i])) for i in mem) % key.n
    vals = sk.decrypt_to_numpy(got)
    for f in range(F):
        ref = np.bincount(ids[:, f], weights=g, minlength=K)
        assert np.allclose(vals[f * K:(f + 1) * K], ref, rtol=1e-9, atol=1e-9)
