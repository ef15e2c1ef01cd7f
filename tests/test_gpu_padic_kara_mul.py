"""GPU: CRT decryption on the 36-limb digit-pair kernel (k_dec_a_padic) with squarings AND products by signed Karatsuba
columns on digits held in registers (csrc/mont_padic.hpp: sqr_kara_reg / mul_kara_reg, kernel mode PADIC_LDS_KM), with
the products row-wise (PAI_DISABLE=padic_kara_mul) and with everything row-wise (PAI_DISABLE=padic_kara), against the
Python-int oracle at a 2048-bit key: ciphertexts whose residues modulo p^2 and q^2 sit at the extremes (1, s^2 - 1, s + 1,
...) next to random ones, in batches that are not a multiple of the 256-element tile.  One more key has primes whose
s - 1 is mostly zero bits: long runs of squarings between few products, and windows that are a single bit.  The cell
bounds of the product are held by tests/test_padic_kara_mul_cpu.py.  Structured primes (limbs all ones / all zero, halves at
opposite extremes, n0inv = 1 / 2^29 - 1) on all three modes: tests/test_gpu_extreme_keys.py."""
import random

import pytest
import torch

from oracle import paillier_oracle as orc
from pailliercryptolib_python_amd import engine
from tests._util import disable, tune

pytestmark = pytest.mark.gpu

MODES = {"kara_mul": (), "kara_sqr": ("padic_kara_mul",), "rowwise": ("padic_kara",)}


def handles(p, q):
    key = orc.make_key(p, q, djn_x=0x1234567, bits=2048)
    dev = torch.device("cuda", 0)
    pub = engine.PublicKeyHandle(key.n, 2048, key.hs, key.randbits, device=dev)
    priv = engine.PrivateKeyHandle(pub, key.p, key.q)
    return key, pub, priv, dev


@pytest.fixture(scope="module")
def keys():
    return handles(orc.BENCH_P, orc.BENCH_Q)


def sparse_prime(seed):
    """1024-bit prime, top two bits set, p % 4 == 3, whose p - 1 has one set bit every 150 positions above a 40-bit tail."""
    rng = random.Random(seed)
    c = (1 << 1023) | (1 << 1022) | sum(1 << (150 * i) for i in range(1, 7)) | rng.getrandbits(40) | 3
    while not orc.is_probable_prime(c):
        c += 4
    return c


@pytest.fixture(scope="module")
def sparse_keys():
    p, q = sparse_prime(1), sparse_prime(2)
    assert p != q and (p * q).bit_length() == 2048
    return handles(p, q)


def crt(a, b, p2, q2):
    return (a + p2 * ((b - a) * pow(p2, -1, q2) % q2)) % (p2 * q2)


def corner_cts(key, n, seed):
    p, q = key.p, key.q
    p2, q2 = p * p, q * q
    sp = [1, p2 - 1, 2, p2 - 2, p + 1, p2 - p - 1, (p2 - 1) // 2]
    sq = [1, q2 - 1, q2 - 2, 2, q + 1, q2 - q - 1, (q2 - 1) // 2]
    cts = [crt(a, b, p2, q2) for a in sp for b in sq]
    rng = random.Random(seed)
    while len(cts) < n:
        cts.append(rng.randrange(1, key.nsq))
    return cts[:n]


def decrypt_on_kernel(pub, priv, dev, cts, monkeypatch, mode):
    monkeypatch.setenv("PAI_LATENCY_MAX", "0")            # no small-batch kernels
    tune(monkeypatch, "dec_mid_max", 0)                   # no lane-group stage A: every batch on k_dec_a_padic
    for name in ("padic_kara_mul", "padic_kara"):
        disable(monkeypatch, name, name in MODES[mode])
    ct = engine.to_device_words(engine.ints_to_words(cts, pub.ct_words), dev)
    out = priv.decrypt(ct)
    torch.cuda.synchronize()
    return engine.words_to_ints(engine.to_host_words(out))


@pytest.mark.parametrize("n", [49, 257, 600])
def test_padic_kara_mul_decrypt_matches_oracle(keys, monkeypatch, n):
    key, pub, priv, dev = keys
    cts = corner_cts(key, n, seed=n)
    want = [orc.decrypt_crt(key, c) for c in cts]
    got = {mode: decrypt_on_kernel(pub, priv, dev, cts, monkeypatch, mode) for mode in MODES}
    assert got["kara_mul"] == want
    assert got["kara_sqr"] == want
    assert got["rowwise"] == want


def test_padic_kara_mul_sparse_exponent(sparse_keys, monkeypatch):
    key, pub, priv, dev = sparse_keys
    cts = corner_cts(key, 257, seed=11)
    want = [orc.decrypt_crt(key, c) for c in cts]
    got = {mode: decrypt_on_kernel(pub, priv, dev, cts, monkeypatch, mode) for mode in MODES}
    assert got["kara_mul"] == want
    assert got["kara_sqr"] == want
    assert got["rowwise"] == want


def test_padic_kara_mul_more_tiles_than_workgroups(keys, monkeypatch):
    """A batch of more 256-element tiles than the launch has workgroups per prime (at most one per two compute units, so at
    most 128 on a 256-CU device: 257 tiles here), so that every workgroup walks its tile loop more than once on the
    register-resident path, with a tail tile.  All three modes agree on the whole batch; the oracle holds the corner
    residues at the front and samples from every pass of the loop and the tail."""
    key, pub, priv, dev = keys
    n = 2 * 128 * 256 + 77
    cts = corner_cts(key, n, seed=5)
    got = {mode: decrypt_on_kernel(pub, priv, dev, cts, monkeypatch, mode) for mode in MODES}
    assert got["kara_mul"] == got["kara_sqr"]
    assert got["kara_mul"] == got["rowwise"]
    sample = list(range(49)) + [255, 256, 32767, 32768, 40000, 65535, 65536, n - 77, n - 2, n - 1]
    assert [got["kara_mul"][i] for i in sample] == [orc.decrypt_crt(key, cts[i]) for i in sample]
