"""GPU: CRT decryption on the 36-limb digit-pair kernel with the right operand of a product staged in LDS ahead of the step's
squarings (csrc/kernels_padic.hpp: kernel mode PADIC_LDS_KMRBT, the default; a build with -DPAI_KMRBT_PARTS=3 runs the second
pass of a product in the one-sum form as well and is held to the same rows) against its predecessor, which loads the operand
into registers at the head of the product (PAI_DISABLE=padic_stage: mode PADIC_LDS_KMRBS), and against the Python-int oracle,
through pai_decrypt.

Keys, ciphertext pool and expectations are those of tests/test_gpu_padic_kred.py: the 2048-bit bench key, the seeded 1536-bit
key (768-bit primes on 36 limbs) and the structured keys with 1024-bit primes of tests/golden/extreme_keys.json; real
encryptions, 0, 1, n^2 - 1, and values = 0 and = -1 modulo p^2 resp. q^2.
Batches: 1, 255 / 256 / 257; on the bench key one batch of 256 (workgroups + 1) elements, so that a workgroup walks its tile
loop twice and would multiply by the previous tile's staged operand if the staged index were not reset; and per key 257 rows
with the steered ciphertexts of tests/_steer.py at rows 0, 63, 64, 255 and 256 (limbs at +-2^28 in the registers, the largest
columns the second pass of the following products and the squarings meet).
The new default must equal its predecessor on every row and the oracle wherever the ciphertext is a unit, and the profile
record must name the kernel that ran (pai_profile_last_mode: "kmrb" / "kmrbh" behind the path "padic_kara_mul").
The cells of the new second pass: tests/test_padic_mul2_onesum_cpu.py."""
import ctypes as C
import gc
import random

import pytest

from pailliercryptolib_python_amd import _native
from tests import _steer as st
from tests import test_gpu_padic_kred as kred
from tests._util import DevArray, disable, ints_to_limbs, limbs_to_ints, tune
from tests.test_gpu_paillier_abi import NativeKey, _last_kernels, bench_key
from tests.test_gpu_padic_kred import KEYS, ciphertext_pool, oracle_decrypt

pytestmark = pytest.mark.gpu

MODES = {"kmrb": (), "kmrbh": ("padic_stage",)}
KNOBS = ("padic_stage", "padic_one_sum", "padic_balanced", "padic_kara_red", "padic_kara_mul", "padic_kara")
STEERED_ROWS = (0, 63, 64, 255, 256)


class Case:
    """The key's pool and expectations (taken from tests/test_gpu_padic_kred.py's cache where that file has run) on key
    handles and device arrays of this file's own."""

    def __init__(self, ident):
        shared = kred._CASES.get(ident)
        if shared is not None:
            self.key, self.cts, self.want = shared.key, shared.cts, shared.want
        else:
            self.key = KEYS[ident]()
            self.cts = ciphertext_pool(self.key, kred.POOL, seed=len(ident))
            self.want = oracle_decrypt(self.key, self.cts)
        assert sum(w is None for w in self.want) >= 7 and self.want[0] is not None
        # the pool with steered ciphertexts at the lane edges of a wave, in both tiles
        rng = random.Random(len(ident) + 200)
        steered = []
        for which in (0, 1):
            s = st.prime_of(self.key, which)
            if st.usable_steps(s):
                steered += [st.steered_ciphertext(self.key, which, w, v, rng) for _, w, v in st.target_pairs(s)]
        assert len(steered) >= len(STEERED_ROWS), ident
        step = len(steered) // len(STEERED_ROWS)
        picks = [steered[i * step] for i in range(len(STEERED_ROWS))]
        assert len(set(picks)) == len(STEERED_ROWS)
        self.mixed, self.mixed_want = list(self.cts), list(self.want)
        for row, c, w in zip(STEERED_ROWS, picks, oracle_decrypt(self.key, picks)):
            assert w is not None
            self.mixed[row], self.mixed_want[row] = c, w
        self.open()

    def open(self):
        if getattr(self, "nk", None) is None:
            self.nk = NativeKey(self.key)
            self.dct = DevArray(ints_to_limbs(self.cts, self.nk.cw))
            self.dmixed = DevArray(ints_to_limbs(self.mixed, self.nk.cw))

    def release(self):
        self.nk = self.dct = self.dmixed = None


_MINE = {}


def release_handles(keep=None):
    """destroys this file's key handles and device arrays of every case but `keep`"""
    for ident, c in _MINE.items():
        if ident != keep:
            c.release()
    gc.collect()


@pytest.fixture(params=list(KEYS))
def case(request):
    ident = request.param
    if ident not in _MINE:
        _MINE[ident] = Case(ident)
    release_handles(keep=ident)
    _MINE[ident].open()
    return _MINE[ident]


@pytest.fixture(scope="module", autouse=True)
def no_handles_left_behind():
    yield
    release_handles()
    _MINE.clear()
    gc.collect()


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


def rows_that_differ(a, b):
    return [i for i, (x, y) in enumerate(zip(a, b)) if x != y]


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_padic_stage_decrypt(case, monkeypatch, n):
    got = decrypt_modes(case.nk, case.dct, n, monkeypatch)
    assert not rows_that_differ(got["kmrb"], got["kmrbh"])
    assert not [i for i in range(n) if case.want[i] is not None and got["kmrb"][i] != case.want[i]]


def test_padic_stage_steered_rows(case, monkeypatch):
    got = decrypt_modes(case.nk, case.dmixed, len(case.mixed), monkeypatch)
    assert not rows_that_differ(got["kmrb"], got["kmrbh"])
    assert not [i for i, w in enumerate(case.mixed_want) if w is not None and got["kmrb"][i] != w]
    assert all(case.mixed_want[r] is not None for r in STEERED_ROWS)


def test_padic_stage_tile_loop_wraps_once(monkeypatch):
    """256 (workgroups + 1) elements on the bench key: one tile more than the launch has workgroups per prime (half the
    compute units), so the first workgroup walks its tile loop twice: its second tile starts with the LDS digit buffers
    holding the exit product of the first, not the operand last staged.  The two modes agree on the whole batch; the oracle
    holds the special residues at the front and samples from both passes of the loop."""
    import torch

    release_handles()
    key = bench_key()
    nk = NativeKey(key)
    workgroups = torch.cuda.get_device_properties(0).multi_processor_count // 2
    n = 256 * (workgroups + 1)
    rng = random.Random(23)
    cts = ciphertext_pool(key, 64, seed=23) + [rng.randrange(1, key.nsq) for _ in range(n - 64)]
    dct = DevArray(ints_to_limbs(cts, nk.cw))
    got = decrypt_modes(nk, dct, n, monkeypatch)
    assert not rows_that_differ(got["kmrb"], got["kmrbh"])
    sample = list(range(64)) + [255, 256, 257, n // 2, n - 257, n - 256, n - 255, n - 2, n - 1]
    want = oracle_decrypt(key, [cts[i] for i in sample])
    assert not [i for i, w in zip(sample, want) if w is not None and got["kmrb"][i] != w]
    del dct, nk
    gc.collect()
