"""GPU: CRT decryption on the 36-limb digit-pair kernel with one stored sum per column (csrc/mont_padic.hpp: kara_pass_bal with
ONES, kernel mode PADIC_LDS_KMRBS, the default) against its predecessor with two (PAI_DISABLE=padic_one_sum: mode
PADIC_LDS_KMRB), against the kernel on unsigned limbs (PAI_DISABLE=padic_balanced: mode PADIC_LDS_KMR) and against the
Python-int oracle, through pai_decrypt.

Keys, ciphertext pool and expectations are those of tests/test_gpu_padic_kred.py (shared, computed once): the 2048-bit bench
key, the seeded 1536-bit key (768-bit primes on 36 limbs) and the structured keys with 1024-bit primes of
tests/golden/extreme_keys.json; real encryptions, 0, 1, n^2 - 1, and values = 0 and = -1 modulo p^2 resp. q^2.
Batches: 1, 255 / 256 / 257, and on the bench key one batch of 256 (workgroups + 1) elements, so that the tile loop wraps once.
All three modes must give the same words for every ciphertext, the oracle's words wherever the ciphertext is a unit, and the
profile record must name the kernel that ran (pai_profile_last_mode: "kmrb" / "kmrb2s" / "kmr" behind the path
"padic_kara_mul").  The cells of the new passes: tests/test_padic_onesum_cpu.py."""
import ctypes as C
import random

import pytest

from pailliercryptolib_python_amd import _native
from tests._util import DevArray, disable, ints_to_limbs, limbs_to_ints, tune
from tests.test_gpu_paillier_abi import NativeKey, _last_kernels, bench_key
from tests.test_gpu_padic_kred import _CASES, KEYS, Case, ciphertext_pool, oracle_decrypt

pytestmark = pytest.mark.gpu

MODES = {"kmrb": (), "kmrb2s": ("padic_one_sum",), "kmr": ("padic_balanced",)}
KNOBS = ("padic_one_sum", "padic_balanced", "padic_kara_red", "padic_kara_mul", "padic_kara")


@pytest.fixture(params=list(KEYS))
def case(request):
    if request.param not in _CASES:
        _CASES[request.param] = Case(request.param)
    return _CASES[request.param]


def decrypt_modes(nk, dct, n, monkeypatch):
    """{mode: plaintext integers} of the first n ciphertexts at dct, every batch on k_dec_a_padic"""
    monkeypatch.setenv("PAI_LATENCY_MAX", "0")            # no small-batch kernels
    tune(monkeypatch, "dec_mid_max", 0)                   # no lane-group stage A
    _native.check(nk.lib.pai_profile_enable(1))
    got = {}
    try:
        for mode, off in MODES.items():
            for name in KNOBS:
                disable(monkeypatch, name, name in off)
            out = DevArray(shape=(n, nk.nw))
            _native.check(nk.lib.pai_decrypt(nk.sk, dct.ptr, n, out.ptr, None))
            buf = C.create_string_buffer(64)
            assert _last_kernels(nk.lib)[0] == "k_dec_a"
            _native.check(nk.lib.pai_profile_last_path(0, buf, 64))
            assert buf.value.decode() == "padic_kara_mul"
            _native.check(nk.lib.pai_profile_last_mode(0, buf, 64))
            assert buf.value.decode() == mode
            got[mode] = limbs_to_ints(out.get())
    finally:
        _native.check(nk.lib.pai_profile_enable(0))
    return got


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_padic_onesum_decrypt(case, monkeypatch, n):
    got = decrypt_modes(case.nk, case.dct, n, monkeypatch)
    assert got["kmrb"] == got["kmrb2s"]
    assert got["kmrb"] == got["kmr"]
    for i in range(n):
        if case.want[i] is not None:
            assert got["kmrb"][i] == case.want[i], i


def test_padic_onesum_tile_loop_wraps_once(monkeypatch):
    """256 (workgroups + 1) elements on the bench key: one tile more than the launch has workgroups per prime (half the
    compute units), so the first workgroup walks its tile loop twice.  The three modes agree on the whole batch; the oracle
    holds the special residues at the front and samples from both passes of the loop."""
    import torch

    key = bench_key()
    nk = NativeKey(key)
    workgroups = torch.cuda.get_device_properties(0).multi_processor_count // 2
    n = 256 * (workgroups + 1)
    rng = random.Random(17)
    cts = ciphertext_pool(key, 64, seed=17) + [rng.randrange(1, key.nsq) for _ in range(n - 64)]
    dct = DevArray(ints_to_limbs(cts, nk.cw))
    got = decrypt_modes(nk, dct, n, monkeypatch)
    assert got["kmrb"] == got["kmrb2s"]
    assert got["kmrb"] == got["kmr"]
    sample = list(range(64)) + [255, 256, 257, n // 2, n - 257, n - 256, n - 255, n - 2, n - 1]
    want = oracle_decrypt(key, [cts[i] for i in sample])
    for i, w in zip(sample, want):
        if w is not None:
            assert got["kmrb"][i] == w, i
