"""GPU: DJN encryption at 72 limbs on the Karatsuba-column kernel (csrc/kernels_padic_enc.hpp: k_encrypt_padic with KARA — a
balanced digit pair held in registers, every table product by csrc/mont_padic.hpp: mul_kara2_c0_bal in two half-width steps)
against the row-wise kernel it replaces (PAI_DISABLE=enc_kara) and against oracle.paillier_oracle.encrypt, through pai_encrypt.

Keys: the 2048-bit bench key, every structured key of tests/golden/extreme_keys.json with a 2048-bit n, and one seeded key of
1408 bits (two seeded 704-bit primes: the low end of the 72-limb engine).  Batches: 1, 255, 256, 257, and on the bench key
256 (workgroups + 1) elements, so that the tile loop wraps.  r: 0, 1, 2^randbits - 1, one window all ones with the rest zero
(the first, a middle one, the last) and seeded random values; m: 0, 1, n - 1, max_int and random values.  Windows: PAI_TUNE
fb_digit_wbits=8 (128 short windows) for all keys and the default width once on the bench key.  For every row the words of the
new kernel equal those of the previous kernel and the oracle's, and the profile record names the kernel that ran
(pai_profile_last_mode "enc_kara" / "rows" behind the path "padic").  The cells of the pass: tests/test_enc_kara_cpu.py."""
import ctypes as C
import gc
import random

import pytest

from oracle import paillier_oracle as orc
from pailliercryptolib_python_amd import _native
from tests._util import DevArray, disable, ints_to_limbs, limbs_to_ints, tune
from tests.test_extreme_keys_cpu import load_extreme_keys
from tests.test_gpu_paillier_abi import NativeKey, _last_kernels, bench_key

pytestmark = pytest.mark.gpu

WB = 8
ROWS = 257


def key_1408():
    seed = 0
    while True:
        p, q = orc.seeded_prime(704, 14080 + seed), orc.seeded_prime(704, 24080 + seed)
        if p != q and (p * q).bit_length() == 1408:
            return orc.make_key(p, q, djn_x=0xABCDEF1234567, bits=1408)
        seed += 1


KEYS = {"bench-2048": bench_key, "seeded-1408": key_1408}
for _ident, _family, _b, _p, _q in load_extreme_keys():
    if _b == 1024:
        KEYS[_ident] = (lambda p=_p, q=_q: orc.make_key(p, q, djn_x=(1 << 70) + 12345, bits=2048))


def rows_for(key, n, seed):
    """(m, r) of n rows: the corners of either operand first, then seeded random values; the one-window values of r for the
    8-bit windows of the tests and for the 18-bit windows of the default table"""
    rng = random.Random(seed)
    rb = key.randbits
    rs = [0, 1, (1 << rb) - 1]
    for wb in (WB, 18):
        windows = (rb + wb - 1) // wb
        ones = (1 << wb) - 1
        rs += [ones, ones << (wb * (windows // 2)), ones << (wb * (windows - 1)) & ((1 << rb) - 1)]
    ms = [0, 1, key.n - 1, key.max_int]
    m = [rng.randrange(key.n) for _ in range(n)]
    r = [rng.getrandbits(rb) for _ in range(n)]
    # rows 1 ..: every corner of r with a rotating corner of m, then every corner of m with a random r (row 0 stays random:
    # the batch of one is an ordinary encryption)
    for i, rv in enumerate(rs):
        if 1 + i < n:
            r[1 + i], m[1 + i] = rv, ms[i % len(ms)]
    for i, mv in enumerate(ms):
        if 1 + len(rs) + i < n:
            m[1 + len(rs) + i] = mv
    return m, r


class Case:
    """Inputs and the oracle's ciphertexts of one key, computed once; one key handle per window width."""

    def __init__(self, ident):
        self.key = KEYS[ident]()
        self.m, self.r = rows_for(self.key, ROWS, 19)
        self.want = [orc.encrypt(self.key, x, rr) for x, rr in zip(self.m, self.r)]
        self.handles = {}

    def handle(self, wb):
        """(key handle, m and r on the device); created by the first test that asks, under that test's PAI_TUNE (the table
        is built by the handle's first call)"""
        if wb not in self.handles:
            nk = NativeKey(self.key)
            self.handles[wb] = (nk, DevArray(ints_to_limbs(self.m, nk.nw)), DevArray(ints_to_limbs(self.r, nk.rw)))
        return self.handles[wb]


_CASES = {}


def release_handles(keep=None):
    """destroys the key handles of every case but `keep`: a handle that has encrypted holds its fixed-base table, and the
    library sizes the table of a new key by the tables resident on the device (csrc/capi_pubkey_tables.hpp: PAI_FB_BIG_KEYS)"""
    for ident, case in _CASES.items():
        if ident != keep:
            case.handles.clear()
    gc.collect()


def get_case(ident):
    if ident not in _CASES:
        _CASES[ident] = Case(ident)
    release_handles(keep=ident)
    return _CASES[ident]


@pytest.fixture(scope="module", autouse=True)
def no_tables_left_behind():
    """the tests after this file find the device as this file found it: no key handle of it, hence no table, stays"""
    yield
    release_handles()
    _CASES.clear()
    gc.collect()


def encrypt_modes(nk, dm, dr, n, monkeypatch, wb):
    """{mode: ciphertext integers} of the first n rows, every batch on k_encrypt_padic"""
    monkeypatch.setenv("PAI_LATENCY_MAX", "0")            # no small-batch kernels
    tune(monkeypatch, "enc_mid_max", 0)                   # no lane-group digit-pair kernel
    tune(monkeypatch, "fb_digit_wbits", wb if wb else None)
    _native.check(nk.lib.pai_profile_enable(1))
    got = {}
    try:
        for mode, off in (("enc_kara", False), ("rows", True)):
            disable(monkeypatch, "enc_kara", off)
            ct = DevArray(shape=(n, nk.cw))
            _native.check(nk.lib.pai_encrypt(nk.pk, dm.ptr, dr.ptr, n, ct.ptr, None))
            buf = C.create_string_buffer(64)
            assert _last_kernels(nk.lib) == ["k_encrypt(djn)"]
            _native.check(nk.lib.pai_profile_last_path(0, buf, 64))
            assert buf.value.decode() == "padic"
            _native.check(nk.lib.pai_profile_last_mode(0, buf, 64))
            assert buf.value.decode() == mode
            got[mode] = limbs_to_ints(ct.get())
    finally:
        _native.check(nk.lib.pai_profile_enable(0))
    return got


@pytest.mark.parametrize("n", [1, 255, 256, 257])
@pytest.mark.parametrize("ident", list(KEYS))
def test_enc_kara_encrypt(ident, n, monkeypatch):
    case = get_case(ident)
    tune(monkeypatch, "fb_digit_wbits", WB)
    nk, dm, dr = case.handle(WB)
    got = encrypt_modes(nk, dm, dr, n, monkeypatch, WB)
    assert got["enc_kara"] == got["rows"]
    assert got["enc_kara"] == case.want[:n]


def test_enc_kara_default_window_width(monkeypatch):
    """the table geometry a key gets without tuning, once on the bench key"""
    case = get_case("bench-2048")
    tune(monkeypatch, "fb_digit_wbits", None)
    nk, dm, dr = case.handle(0)
    got = encrypt_modes(nk, dm, dr, ROWS, monkeypatch, 0)
    assert got["enc_kara"] == got["rows"]
    assert got["enc_kara"] == case.want


def test_enc_kara_tile_loop_wraps(monkeypatch):
    """256 (workgroups + 1) elements on the bench key: one tile more than the launch has workgroups (one per compute unit), so
    the first workgroup walks its tile loop twice.  Both kernels agree on the whole batch; the oracle holds the rows of the
    shared case at the front and samples from both passes of the loop."""
    import torch

    case = get_case("bench-2048")
    tune(monkeypatch, "fb_digit_wbits", WB)
    nk, _, _ = case.handle(WB)
    key = case.key
    workgroups = torch.cuda.get_device_properties(0).multi_processor_count
    n = 256 * (workgroups + 1)
    m, r = rows_for(key, n, 23)
    m[:ROWS], r[:ROWS] = case.m, case.r
    dm, dr = DevArray(ints_to_limbs(m, nk.nw)), DevArray(ints_to_limbs(r, nk.rw))
    got = encrypt_modes(nk, dm, dr, n, monkeypatch, WB)
    assert got["enc_kara"] == got["rows"]
    assert got["enc_kara"][:ROWS] == case.want
    for i in (n // 2, n - 257, n - 256, n - 255, n - 2, n - 1):
        assert got["enc_kara"][i] == orc.encrypt(key, m[i], r[i]), i
