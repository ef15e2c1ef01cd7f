"""GPU: CRT decryption on the 36-limb digit-pair kernel (k_dec_a_padic) with its squarings by signed Karatsuba product
columns (csrc/mont_padic.hpp: sqr_kara, the default) and by the row-wise form (PAI_DISABLE=padic_kara), against the
Python-int oracle at a 2048-bit key: ciphertexts whose residues modulo p^2 and q^2 sit at the extremes (1, s^2 - 1, s + 1,
...) next to random ones, in batches that are not a multiple of the 256-element tile.  The cell bounds of the squaring are
held by tests/test_padic_kara_cpu.py.  Structured primes (limbs all ones / all zero, halves at opposite extremes):
tests/test_gpu_extreme_keys.py."""
import random

import pytest
import torch

from oracle import paillier_oracle as orc
from pailliercryptolib_python_amd import engine
from tests._util import disable, tune

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def keys():
    key = orc.make_key(orc.BENCH_P, orc.BENCH_Q, djn_x=0x1234567, bits=2048)
    dev = torch.device("cuda", 0)
    pub = engine.PublicKeyHandle(key.n, 2048, key.hs, key.randbits, device=dev)
    priv = engine.PrivateKeyHandle(pub, orc.BENCH_P, orc.BENCH_Q)
    return key, pub, priv, dev


def crt(a, b, p2, q2):
    return (a + p2 * ((b - a) * pow(p2, -1, q2) % q2)) % (p2 * q2)


def corner_cts(key, n, seed):
    p, q = orc.BENCH_P, orc.BENCH_Q
    p2, q2 = p * p, q * q
    sp = [1, p2 - 1, 2, p2 - 2, p + 1, p2 - p - 1, (p2 - 1) // 2]
    sq = [1, q2 - 1, q2 - 2, 2, q + 1, q2 - q - 1, (q2 - 1) // 2]
    cts = [crt(a, b, p2, q2) for a in sp for b in sq]
    rng = random.Random(seed)
    while len(cts) < n:
        cts.append(rng.randrange(1, key.nsq))
    return cts[:n]


def decrypt_on_kernel(pub, priv, dev, cts, monkeypatch, kara):
    monkeypatch.setenv("PAI_LATENCY_MAX", "0")            # no small-batch kernels
    tune(monkeypatch, "dec_mid_max", 0)                   # no lane-group stage A: every batch on k_dec_a_padic
    disable(monkeypatch, "padic_kara", not kara)
    ct = engine.to_device_words(engine.ints_to_words(cts, pub.ct_words), dev)
    out = priv.decrypt(ct)
    torch.cuda.synchronize()
    return engine.words_to_ints(engine.to_host_words(out))


@pytest.mark.parametrize("n", [49, 257, 600])
def test_padic_kara_decrypt_matches_oracle(keys, monkeypatch, n):
    key, pub, priv, dev = keys
    cts = corner_cts(key, n, seed=n)
    got = decrypt_on_kernel(pub, priv, dev, cts, monkeypatch, kara=True)
    assert got == [orc.decrypt_crt(key, c) for c in cts]


def test_padic_kara_on_off_agree(keys, monkeypatch):
    key, pub, priv, dev = keys
    cts = corner_cts(key, 300, seed=3)
    on = decrypt_on_kernel(pub, priv, dev, cts, monkeypatch, kara=True)
    off = decrypt_on_kernel(pub, priv, dev, cts, monkeypatch, kara=False)
    assert on == off
    assert on[:49] == [orc.decrypt_crt(key, c) for c in cts[:49]]
