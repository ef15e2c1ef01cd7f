"""CPU: the row operations of packed ciphertexts (PaillierPackedNumber.segment_sum / cumsum / sum / take / repack) — the headroom
rule, the repack layout and every argument check, on host containers that never touch a device; and the pai_ct_pack_step entry
point.  The expectations come from Python ints and from the format's definition, never from the code
under test."""
import itertools
import json
from pathlib import Path
import re

import numpy as np
import pytest
import torch

from pailliercryptolib_python_amd import PaillierPackedNumber, PaillierPublicKey, _native, packed
from pailliercryptolib_python_amd.bindings import ipclCipherText

ROOT = Path(__file__).resolve().parents[1]
KEYS = json.loads((ROOT / "tests" / "golden" / "fixture_keys.json").read_text())


def modulus(bits):
    return int(KEYS[str(bits)]["p"], 16) * int(KEYS[str(bits)]["q"], 16)


def host_key(bits=1024):
    """a public key object that never touches a device (standard scheme: nothing to precompute)"""
    return PaillierPublicKey(modulus(bits), bits, False)


def host_packed(pk, n_elems, b, k, E=10, v=20, fill=1):
    G = (n_elems + k - 1) // k
    return PaillierPackedNumber(pk, ipclCipherText(pk.pubkey, [fill] * G), slot_bits=b, slots=k, exponent=E, value_bits=v, length=n_elems)


def no_device(pk):
    """the key's device handle was never created (it would need a GPU: the checks under test come before it)"""
    return "_home_handle" not in vars(pk.pubkey) and not pk.pubkey._handles


# ---- the headroom rule ----------------------------------------------------------------------------------------------------------
def test_sum_value_bits_follows_the_bit_length_of_count_minus_one():
    assert packed.sum_value_bits(20, 1, 32) == 20         # one member: nothing added
    for e in range(1, 12):
        c = 1 << e
        assert packed.sum_value_bits(5, c - 1, 64) == 5 + (c - 2).bit_length()
        assert packed.sum_value_bits(5, c, 64) == 5 + e
        assert packed.sum_value_bits(5, c + 1, 64) == 5 + e + 1
    for c in range(1, 70):
        assert packed.sum_value_bits(7, c, 128) == 7 + (c - 1).bit_length()


def test_sum_value_bits_bounds_every_sum_by_brute_force():
    """|m| < 2^v for c members: the extreme sums are +-c (2^v - 1), and the bound must hold strictly — and must not be loose by more
    than one bit (c 2^v > 2^(bound - 1))"""
    for v, c in itertools.product(range(1, 7), range(1, 40)):
        bound = packed.sum_value_bits(v, c, 64)
        top = c * ((1 << v) - 1)
        assert top < 1 << bound and -top > -(1 << bound), (v, c)
        assert c * (1 << v) > 1 << (bound - 1), (v, c)
    # every sum of three members at v = 2, exhaustively
    lim = 3
    bound = packed.sum_value_bits(2, 3, 64)
    assert all(abs(a + b + c) < 1 << bound for a, b, c in itertools.product(range(-lim, lim + 1), repeat=3))


def test_sum_value_bits_overflow_edge():
    assert packed.sum_value_bits(20, 2048, 32) == 31       # exactly the b - 1 bits a 32-bit slot holds
    with pytest.raises(OverflowError):
        packed.sum_value_bits(20, 2049, 32)
    with pytest.raises(OverflowError):
        packed.sum_value_bits(31, 2, 32)
    assert packed.sum_value_bits(31, 1, 32) == 31


# ---- repack: the layout -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [1024, 2048, 3072])
def test_repack_default_factor_is_the_largest_that_fits(bits):
    nb = modulus(bits).bit_length()
    for b, k in ((8, 1), (32, 2), (100, 2), (64, 3), (128, 7), (53, 19), (64, (nb - 2) // 64)):
        f = packed.repack_factor(nb, b, k)
        assert f >= 1 and f * k * b <= nb - 2 < (f + 1) * k * b, (bits, b, k)
        assert packed.repack_factor(nb, b, k, f) == f
        assert packed.repack_factor(nb, b, k, 1) == 1
        with pytest.raises(ValueError):
            packed.repack_factor(nb, b, k, f + 1)
        for bad in (0, -1):
            with pytest.raises(ValueError):
                packed.repack_factor(nb, b, k, bad)
        with pytest.raises(TypeError):
            packed.repack_factor(nb, b, k, 1.5)


def test_repack_row_count_is_the_nested_ceiling_for_ragged_lengths():
    nb = 1024
    for b, k, f in ((16, 3, 5), (100, 2, 5), (8, 7, 18), (64, 1, 15)):
        assert f * k * b <= nb - 2
        for N in list(range(0, 4 * k * f + 3)) + [1000, 1001, 12345]:
            G = -(-N // k)
            lay = packed.layout(nb, b, k * f)
            assert lay.groups(N) == -(-G // f), (b, k, f, N)


def test_repack_keeps_element_i_in_slot_i_mod_kf_on_a_model_of_the_plaintexts():
    """the plaintext of output row r is sum_(j<f) P_(r f + j) 2^(k b j) (the exponents of a product of powers add): read as a row
    of k f slots of b bits it holds element i in slot i % (k f) — signed slots included, no bias anywhere"""
    rng = np.random.default_rng(11)
    b, k, f = 16, 3, 4
    for N in (1, 2, 3, 4, 11, 12, 13, 35, 36, 37, 50):
        ms = [int(x) for x in rng.integers(-(1 << 14), 1 << 14, N)]
        G = -(-N // k)
        P = [sum(m << (b * j) for j, m in enumerate(ms[g * k:(g + 1) * k])) for g in range(G)]
        Q = [sum(P[r * f + j] << (k * b * j) for j in range(f) if r * f + j < G) for r in range(-(-G // f))]
        kf = k * f
        want = [sum(m << (b * j) for j, m in enumerate(ms[r * kf:(r + 1) * kf])) for r in range(-(-N // kf))]
        assert Q == want, N
        # ... and the signed slots read back element by element
        for i, m in enumerate(ms):
            row, slot = divmod(i, kf)
            q = Q[row] + sum(1 << (b * j + b - 1) for j in range(kf))            # the bias of unpacking
            assert ((q >> (b * slot)) & ((1 << b) - 1)) - (1 << (b - 1)) == m


def test_repack_factor_that_does_not_fit_raises_before_any_device_use():
    pk = host_key()
    p = host_packed(pk, 20, 100, 2)                        # 200-bit rows: 5 of them fit 1022 bits
    with pytest.raises(ValueError):
        p.repack(factor=6)
    with pytest.raises(ValueError):
        p.repack(factor=0)
    with pytest.raises(TypeError):
        p.repack(factor=2.0)
    assert no_device(pk)


# ---- argument checks come before the device ----------------------------------------------------------------------------------------
def test_segment_sum_argument_checks():
    pk = host_key()
    p = host_packed(pk, 20, 100, 2)
    assert p.rows == 10
    ok = np.zeros(10, dtype=np.int64)
    for ids in (np.zeros(9, dtype=np.int64), np.zeros(20, dtype=np.int64), np.zeros((10, 2, 1), dtype=np.int64),
                np.zeros((2, 10), dtype=np.int64), torch.zeros(11, dtype=torch.int64)):
        with pytest.raises(ValueError):
            p.segment_sum(ids, 4)
    for ids in (np.zeros(10), np.zeros(10, dtype=bool), torch.zeros(10), torch.zeros(10, dtype=torch.bool), [0] * 10):
        with pytest.raises(TypeError):
            p.segment_sum(ids, 4)
    bad = ok.copy()
    bad[3] = 4
    with pytest.raises(ValueError):
        p.segment_sum(bad, 4)                              # an id >= num_segments
    with pytest.raises(ValueError):
        p.segment_sum(torch.from_numpy(bad.reshape(10, 1)), 4)
    with pytest.raises(ValueError):
        p.segment_sum(ok, 0)
    with pytest.raises(TypeError):
        p.segment_sum(ok, 2.0)
    with pytest.raises(TypeError):
        p.segment_sum(ok, True)
    assert no_device(pk)


def test_cumsum_argument_checks_and_overflow():
    pk = host_key()
    p = host_packed(pk, 24, 32, 2, v=20)                   # 12 rows
    for L in (5, 7, 24, 13):
        with pytest.raises(ValueError):
            p.cumsum(L)                                    # does not divide the 12 ROWS (24 elements do not count)
    for L in (0, -3):
        with pytest.raises(ValueError):
            p.cumsum(L)
    for L in (2.0, True, "4"):
        with pytest.raises(TypeError):
            p.cumsum(L)
    big = host_packed(pk, 2 * 4098, 32, 2, v=20)            # 4098 rows
    with pytest.raises(OverflowError):
        big.cumsum()                                       # 20 + bit_length(4097) = 33 bits
    with pytest.raises(OverflowError):
        big.cumsum(2049)                                   # 20 + 12 = 32 > 31
    with pytest.raises(OverflowError):
        big.cumsum(2049, reverse=True)
    with pytest.raises(OverflowError):
        big.sum()
    with pytest.raises(OverflowError):
        host_packed(pk, 6, 32, 2, v=31).sum()              # full slots: no second member fits
    assert no_device(pk)


def test_take_argument_checks():
    pk = host_key()
    p = host_packed(pk, 20, 100, 2)                        # 10 rows
    for rows in ([10], [0, 3, -11], np.array([1, 2, 10]), torch.tensor([0, 10]), np.array([-11], dtype=np.int64)):
        with pytest.raises(IndexError):
            p.take(rows)
    for rows in (np.zeros(3), torch.zeros(3), np.zeros(3, dtype=bool), [0.5, 1.0]):
        with pytest.raises(TypeError):
            p.take(rows)
    with pytest.raises(ValueError):
        p.take(np.zeros((2, 2), dtype=np.int64))
    assert no_device(pk)


def test_zero_row_containers_stay_zero_row_without_a_device():
    pk = host_key()
    p = host_packed(pk, 0, 100, 2, v=30)
    assert p.rows == 0
    outs = [p.segment_sum(np.zeros(0, dtype=np.int64), 4), p.segment_sum(np.zeros((0, 3), dtype=np.int64), 4), p.cumsum(),
            p.cumsum(16, reverse=True), p.sum(), p.take([]), p.take(slice(None)), p.take(np.zeros(0, dtype=np.int64)), p.repack(),
            p.repack(factor=2)]
    for q in outs:
        assert isinstance(q, PaillierPackedNumber) and q.rows == 0 and len(q) == 0
        assert (q.slot_bits, q.exponent, q.value_bits) == (100, p.exponent, 30)
    assert [q.slots for q in outs[:8]] == [2] * 8 and outs[8].slots == 10 and outs[9].slots == 4
    with pytest.raises(ValueError):
        p.segment_sum(np.zeros(1, dtype=np.int64), 4)      # the checks still run
    with pytest.raises(IndexError):
        p.take([0])
    assert no_device(pk)


# ---- the entry point and the surface ----------------------------------------------------------------------------------------------
def test_pai_ct_pack_step_is_declared_bound_and_exported():
    name = "pai_ct_pack_step"
    assert name in _native.PROTOTYPES
    assert _native.PROTOTYPES[name] == _native.PROTOTYPES["pai_ct_pack"]      # the same argument list, two ints re-read
    header = (ROOT / "include" / "paillier_hip.h").read_text()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
    assert m and re.search(r"int\s+step_bits\s*,\s*int\s+count", m.group(1))
    assert hasattr(_native.load(), name)


def test_python_surface():
    from pailliercryptolib_python_amd import engine

    assert callable(getattr(engine.PublicKeyHandle, "ct_pack_step", None))
    for meth in ("segment_sum", "cumsum", "sum", "take", "repack"):
        assert callable(getattr(PaillierPackedNumber, meth, None)), meth
    assert isinstance(PaillierPackedNumber.rows, property)
    assert callable(packed.sum_value_bits) and callable(packed.add_value_bits)
    p = host_packed(host_key(), 7, 32, 7)
    assert p.rows == 1 and host_packed(host_key(), 8, 32, 7).rows == 2
    for meth in ("segment_sum", "cumsum", "sum", "take", "repack"):
        assert meth in packed.__doc__
