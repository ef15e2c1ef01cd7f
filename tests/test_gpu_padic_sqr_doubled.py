"""GPU: CRT decryption on the 36-limb digit-pair kernel whose squarings sum the off-diagonal products of their first pass on the
doubled operand (csrc/mont_padic.hpp: kara_pass_bal, DSYM; csrc/kernels_padic.hpp: kernel mode PADIC_LDS_KMRBT, PAI_KMRBT_PARTS
bit 2; a build with further bits of PAI_KMRBT_PARTS is held to the same rows) against the kernel that keeps the shifted chain
and loads a product's operand at its head (PAI_DISABLE=padic_stage: mode PADIC_LDS_KMRBS, untouched), and against the
Python-int oracle, through pai_decrypt.

Coverage is that of tests/test_gpu_padic_stage.py, whose cases, pools and helpers this file takes as they are (one pool and
one oracle run per key, shared between the two files): the 2048-bit bench key, the seeded 1536-bit key (768-bit primes on 36
limbs) and the structured keys with 1024-bit primes; batches 1, 255 / 256 / 257; per key 257 rows with the steered
ciphertexts of tests/_steer.py at rows 0, 63, 64, 255 and 256 — their targets put limbs at +-2^28 into the registers, so the
squaring that follows meets its largest columns and the doubled operand its largest terms (2^29 and, for the half
differences, 2^30 in magnitude: a sum kept in fewer than 64 bits would show there); and one batch of 256 (workgroups + 1)
rows on the bench key, so that a wave runs more than one tile.  Every row equals PAI_DISABLE=padic_stage, equals the oracle
wherever the ciphertext is a unit, and pai_profile_last_mode names the kernel that ran ("kmrb" / "kmrbh").
The cells of the pass: tests/test_padic_sqr_doubled_cpu.py."""
import gc
import random

import pytest

from tests import test_gpu_padic_stage as stage
from tests._util import DevArray, ints_to_limbs
from tests.test_gpu_paillier_abi import NativeKey, bench_key
from tests.test_gpu_padic_kred import KEYS, ciphertext_pool, oracle_decrypt
from tests.test_gpu_padic_stage import STEERED_ROWS, decrypt_modes, rows_that_differ

pytestmark = pytest.mark.gpu


@pytest.fixture(params=list(KEYS))
def case(request):
    ident = request.param
    if ident not in stage._MINE:
        stage._MINE[ident] = stage.Case(ident)
    stage.release_handles(keep=ident)
    stage._MINE[ident].open()
    return stage._MINE[ident]


@pytest.fixture(scope="module", autouse=True)
def no_handles_left_behind():
    yield
    stage.release_handles()
    gc.collect()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_padic_sqr_doubled_decrypt(case, monkeypatch, n):
    got = decrypt_modes(case.nk, case.dct, n, monkeypatch)      # asserts the mode each launch reports
    assert set(got) == {"kmrb", "kmrbh"}
    assert not rows_that_differ(got["kmrb"], got["kmrbh"])
    assert not [i for i in range(n) if case.want[i] is not None and got["kmrb"][i] != case.want[i]]


def test_padic_sqr_doubled_steered_rows(case, monkeypatch):
    assert len(case.mixed) == 257
    got = decrypt_modes(case.nk, case.dmixed, len(case.mixed), monkeypatch)
    assert not rows_that_differ(got["kmrb"], got["kmrbh"])
    assert not [i for i, w in enumerate(case.mixed_want) if w is not None and got["kmrb"][i] != w]
    assert all(case.mixed_want[r] is not None for r in STEERED_ROWS)


def test_padic_sqr_doubled_second_tile(monkeypatch):
    """256 (workgroups + 1) rows on the bench key: the first workgroup of either prime runs two tiles, the second with the
    registers and LDS buffers the first left behind."""
    import torch

    stage.release_handles()
    key = bench_key()
    nk = NativeKey(key)
    workgroups = torch.cuda.get_device_properties(0).multi_processor_count // 2
    n = 256 * (workgroups + 1)
    rng = random.Random(25)
    cts = ciphertext_pool(key, 64, seed=25) + [rng.randrange(1, key.nsq) for _ in range(n - 64)]
    dct = DevArray(ints_to_limbs(cts, nk.cw))
    got = decrypt_modes(nk, dct, n, monkeypatch)
    assert not rows_that_differ(got["kmrb"], got["kmrbh"])
    sample = list(range(64)) + [255, 256, 257, n // 2, n - 257, n - 256, n - 255, n - 2, n - 1]
    want = oracle_decrypt(key, [cts[i] for i in sample])
    assert not [i for i, w in zip(sample, want) if w is not None and got["kmrb"][i] != w]
    del dct, nk
    gc.collect()
