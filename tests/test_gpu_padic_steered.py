"""GPU: CRT decryption of STEERED ciphertexts (tests/_steer.py) on the 36-limb digit-pair kernel, through pai_decrypt.

Every other test of k_dec_a_padic feeds real encryptions, random residues and 0, 1, -1 modulo s^2: after the first product their
limbs are uniform and the columns of the balanced passes (csrc/mont_padic.hpp: kara_pass_bal) stay near 2^60, a factor six
below the bound |d_k| < 2^62.76 that lets a whole column live in one signed 64-bit cell.  A steered ciphertext is the e_k-th
root modulo s^2 of a chosen digit pair: after schedule entry k the kernel's registers hold limbs at +-2^28 (all low, all high,
alternating, halves at opposite extremes), and the squaring that follows runs its columns to 2^62.1 and its carries past 2^33
(2^61.7 / 2^32.7 on the 768-bit primes; the model's figures: tests/test_padic_steered_cpu.py).  Modulo the other prime's
square the ciphertext is a random unit, so the CPython oracle defines its decryption.

Keys: those of tests/test_gpu_padic_kred.py.  Every target pair goes on every steerable prime of the key.  Batches: the steered
ciphertexts alone (12 per key with one steerable prime, 24 with two), and 257 rows with steered ciphertexts at rows 0, 63, 64,
255 and 256 among random units (lane edges of a wave, both tiles).  Each batch is decrypted by the default kernel (one stored
sum per column), with PAI_DISABLE=padic_one_sum, padic_balanced, padic_kara_red, padic_kara_mul, padic_kara (row-wise) and on a
handle created with PAI_DISABLE=padic (the modexp modulo s^2, an engine that shares no code with the digit pairs); all seven
must give the oracle's words on every row, and the profile record must name the kernel that ran."""
import ctypes as C
import math
import random

import pytest

from pailliercryptolib_python_amd import _native
from tests import _steer as st
from tests._steer import km
from tests._util import DevArray, disable, ints_to_limbs, limbs_to_ints, tune
from tests.test_gpu_paillier_abi import NativeKey, _last_kernels
from tests.test_gpu_padic_kred import KEYS, oracle_decrypt

pytestmark = pytest.mark.gpu

KNOBS = ("padic_one_sum", "padic_balanced", "padic_kara_red", "padic_kara_mul", "padic_kara")
# run: (PAI_DISABLE entry, path, mode)
RUNS = {"one_sum": (None, "padic_kara_mul", "kmrb"), "two_sums": ("padic_one_sum", "padic_kara_mul", "kmrb2s"),
        "unsigned": ("padic_balanced", "padic_kara_mul", "kmr"), "schoolbook_quotients": ("padic_kara_red", "padic_kara_mul", "km"),
        "rowwise_products": ("padic_kara_mul", "padic_kara", ""), "rowwise": ("padic_kara", "padic_rowwise", "")}
MIXED_ROWS = (0, 63, 64, 255, 256)


class Case:
    def __init__(self, ident, monkeypatch):
        self.key = key = KEYS[ident]()
        rng = random.Random(len(ident) + 100)
        self.steered = []
        for which in (0, 1):
            s = st.prime_of(key, which)
            if not st.usable_steps(s):
                continue
            two = len(st.usable_steps(st.prime_of(key, 1 - which))) > 0
            for name, w, v in st.target_pairs(s):
                for _ in range(1 if two else 2):                         # the same residue modulo s^2 beside two units of the other prime
                    c = st.steered_ciphertext(key, which, w, v, rng)
                    c_s, k, e = st.steer(s, w, v)
                    assert (pow(c, e, s * s) * st.R - (km.value(w) + km.value(v) * s)) % (s * s) == 0
                    self.steered.append(c)
        assert len(self.steered) in (12, 24), ident
        self.mixed = []
        while len(self.mixed) < 257:
            c = rng.randrange(1, key.nsq)
            if math.gcd(c, key.n) == 1:
                self.mixed.append(c)
        step = len(self.steered) // len(MIXED_ROWS)
        for i, row in enumerate(MIXED_ROWS):                             # five different targets; rows 63 and 64 differ
            self.mixed[row] = self.steered[1 + i * step]
        assert len({self.mixed[r] for r in MIXED_ROWS}) == len(MIXED_ROWS)
        self.want = {"steered": oracle_decrypt(key, self.steered), "mixed": oracle_decrypt(key, self.mixed)}
        assert all(w is not None for batch in self.want.values() for w in batch)
        self.nk = NativeKey(key)
        disable(monkeypatch, "padic")
        self.nk_modexp = NativeKey(key)                                  # no digit-pair engine on this handle
        disable(monkeypatch, "padic", False)
        self.dct = {"steered": DevArray(ints_to_limbs(self.steered, self.nk.cw)), "mixed": DevArray(ints_to_limbs(self.mixed, self.nk.cw))}


_CASES = {}


@pytest.fixture(params=list(KEYS))
def case(request, monkeypatch):
    if request.param not in _CASES:
        _CASES[request.param] = Case(request.param, monkeypatch)
    return _CASES[request.param]


def _record(lib):
    path, mode = C.create_string_buffer(64), C.create_string_buffer(64)
    assert _last_kernels(lib)[0] == "k_dec_a"
    _native.check(lib.pai_profile_last_path(0, path, 64))
    _native.check(lib.pai_profile_last_mode(0, mode, 64))
    return path.value.decode(), mode.value.decode()


def decrypt_runs(case, batch, monkeypatch):
    """{run: plaintext integers} of the batch, every run on the throughput kernels (k_dec_a_padic resp. the modexp stage A)"""
    nk, dct, n = case.nk, case.dct[batch], len(case.want[batch])
    monkeypatch.setenv("PAI_LATENCY_MAX", "0")            # no small-batch kernels
    tune(monkeypatch, "dec_mid_max", 0)                   # no lane-group stage A
    _native.check(nk.lib.pai_profile_enable(1))
    got = {}
    try:
        for run, (off, path, mode) in RUNS.items():
            for name in KNOBS:
                disable(monkeypatch, name, name == off)
            out = DevArray(shape=(n, nk.nw))
            _native.check(nk.lib.pai_decrypt(nk.sk, dct.ptr, n, out.ptr, None))
            assert _record(nk.lib) == (path, mode), run
            got[run] = limbs_to_ints(out.get())
        for name in KNOBS:
            disable(monkeypatch, name, False)
        disable(monkeypatch, "padic")
        out = DevArray(shape=(n, nk.nw))
        _native.check(nk.lib.pai_decrypt(case.nk_modexp.sk, dct.ptr, n, out.ptr, None))
        assert _record(nk.lib) in (("lane_group", ""), ("wide", "")), "modexp"
        got["modexp"] = limbs_to_ints(out.get())
    finally:
        _native.check(nk.lib.pai_profile_enable(0))
    return got


@pytest.mark.parametrize("batch", ["steered", "mixed"])
def test_padic_steered_decrypt(case, monkeypatch, batch):
    got = decrypt_runs(case, batch, monkeypatch)
    want = case.want[batch]
    assert set(got) == set(RUNS) | {"modexp"}
    bad = {run: [i for i, (g, w) in enumerate(zip(words, want)) if g != w] for run, words in got.items()}
    assert not {run: rows for run, rows in bad.items() if rows}      # {run: rows that differ from the oracle}
