"""CPU: packed ciphertexts (pailliercryptolib_python_amd/packed.py) — the layout rule, the headroom algebra and the argument
checks of every public method, against a Python-int model of the format written here (include/paillier_hip.h, "packed
ciphertexts"); and the presence of the three C-ABI entry points in the header, the ctypes table and the built library."""
import json
from pathlib import Path
import pickle
import re

import numpy as np
import pytest

from pailliercryptolib_python_amd import PaillierPackedNumber, PaillierPrivateKey, PaillierPublicKey, _native, packed
from pailliercryptolib_python_amd.bindings import ipclCipherText
from pailliercryptolib_python_amd.paillier import PaillierEncryptedNumber

ROOT = Path(__file__).resolve().parents[1]
KEYS = json.loads((ROOT / "tests" / "golden" / "fixture_keys.json").read_text())
KEY_BITS = (1024, 2048, 3072, 4096)
SLOT_BITS = (8, 29, 32, 53, 64, 65, 100, 128)


# ---- the model of the format (Python ints only) -----------------------------------------------------------------------------
def model_max_slots(n_bits, b):
    k = 0
    while (k + 1) * b <= n_bits - 2:
        k += 1
    return k


def model_bias(b, k):
    return sum(1 << (b * j + b - 1) for j in range(k))


def model_pack(mantissas, b, k, n):
    """residues of P_g = sum_j m_(g k + j) 2^(b j) mod n; the tail slots of the last row hold 0"""
    assert all(-(1 << (b - 1)) <= m < (1 << (b - 1)) for m in mantissas)
    return [sum(m << (b * j) for j, m in enumerate(mantissas[g:g + k])) % n for g in range(0, len(mantissas), k)]


def model_unpack(residue, b, k, n):
    """(0, mantissas) | (1, None) overflow zone | (2, None) residue >= n"""
    if residue >= n:
        return 2, None
    q = (residue + model_bias(b, k)) % n
    if q >= 1 << (k * b):
        return 1, None
    return 0, [((q >> (b * j)) & ((1 << b) - 1)) - (1 << (b - 1)) for j in range(k)]


def model_add_bits(va, vb, b):
    v = max(va, vb) + 1
    if v + 1 > b:
        raise OverflowError
    return v


def model_mul_bits(v, c, b):
    v = v + abs(c).bit_length()
    if v + 1 > b:
        raise OverflowError
    return v


def modulus(bits):
    return int(KEYS[str(bits)]["p"], 16) * int(KEYS[str(bits)]["q"], 16)


def host_key(bits=1024):
    """a public key object that never touches a device (standard scheme: nothing to precompute)"""
    return PaillierPublicKey(modulus(bits), bits, False)


def host_packed(pk, n_elems, b, k, E=10, v=20, fill=1):
    G = (n_elems + k - 1) // k
    return PaillierPackedNumber(pk, ipclCipherText(pk.pubkey, [fill] * G), slot_bits=b, slots=k, exponent=E, value_bits=v, length=n_elems)


# ---- layout -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", KEY_BITS)
def test_layout_default_slots_guard_bias_groups_tail(bits):
    n = modulus(bits)
    nb = n.bit_length()
    assert nb == bits
    for b in SLOT_BITS:
        lay = packed.layout(nb, b)
        k = model_max_slots(nb, b)
        assert (lay.n_bits, lay.slot_bits, lay.slots) == (nb, b, k) and packed.max_slots(nb, b) == k
        assert k * b <= nb - 2 < (k + 1) * b
        assert lay.bias == model_bias(b, k) and lay.bias < 1 << (k * b) <= n // 2
        assert packed.layout(nb, b, k).slots == k and packed.layout(nb, b, 1).bias == 1 << (b - 1)
        with pytest.raises(ValueError):
            packed.layout(nb, b, k + 1)                  # the k b <= bits(n) - 2 guard, exactly at the edge
        with pytest.raises(ValueError):
            packed.layout(nb, b, 0)
        for N in (0, 1, k - 1, k, k + 1, 5 * k + 3):
            if N < 0:
                continue
            G = -(-N // k)
            assert lay.groups(N) == G and lay.tail(N) == G * k - N and 0 <= lay.tail(N) < k
        # the largest packed magnitude stays below n / 4: unpacking needs one conditional subtraction only
        extreme = model_pack([-(1 << (b - 1))] * k, b, k, n)[0]
        assert n - extreme < n // 4
    assert packed.layout(2048, 64).slots == 31 and packed.layout(2048, 100).slots == 20
    for bad in (7, 129, 0, -8):
        with pytest.raises(ValueError):
            packed.layout(nb, bad)
    with pytest.raises(TypeError):
        packed.layout(nb, 32.0)


def test_model_round_trip_is_the_unique_inverse():
    rng = np.random.default_rng(3)
    n = modulus(1024)
    for b in SLOT_BITS:
        k = model_max_slots(1024, b)
        lo, hi = -(1 << (b - 1)), (1 << (b - 1)) - 1
        for ms in ([lo] * k, [hi] * k, [0] * k, [int(rng.integers(-100, 100)) for _ in range(k)], [lo, hi] * (k // 2) + [0] * (k % 2)):
            (r,) = model_pack(ms, b, k, n)
            assert model_unpack(r, b, k, n) == (0, ms)
        assert model_unpack(n, b, k, n)[0] == 2
        assert model_unpack((1 << (k * b)) - model_bias(b, k), b, k, n)[0] == 1
        assert model_unpack((n - model_bias(b, k) - 1) % n, b, k, n)[0] == 1


# ---- headroom -----------------------------------------------------------------------------------------------------------------
def test_headroom_algebra_and_overflow_exactly_at_the_slot_width():
    for b in (8, 32, 64, 100, 128):
        for va in range(1, b):
            for vb in (1, va, b - 1):
                try:
                    want = model_add_bits(va, vb, b)
                except OverflowError:
                    with pytest.raises(OverflowError):
                        packed.add_value_bits(va, vb, b)
                else:
                    assert packed.add_value_bits(va, vb, b) == want
            for c in (0, 1, -1, 2, -3, 255, -256, (1 << 70) + 1):
                try:
                    want = model_mul_bits(va, c, b)
                except OverflowError:
                    with pytest.raises(OverflowError):
                        packed.mul_value_bits(va, c, b)
                else:
                    assert packed.mul_value_bits(va, c, b) == want
        # exactly at v + 1 > b
        assert packed.add_value_bits(b - 2, 1, b) == b - 1
        with pytest.raises(OverflowError):
            packed.add_value_bits(b - 1, 1, b)
        assert packed.mul_value_bits(b - 3, -3, b) == b - 1
        with pytest.raises(OverflowError):
            packed.mul_value_bits(b - 2, -3, b)
        assert packed.check_value_bits(b - 1, b) == b - 1
        for bad in (0, b, -1):
            with pytest.raises(ValueError):
                packed.check_value_bits(bad, b)


def test_headroom_bounds_really_bound_the_slots():
    """a chain (p + q) * c + r on extreme mantissas stays inside its proven bound, and the bound inside the slot"""
    b = 32
    va, vb, c, vr = 10, 12, -3, 5
    v = model_add_bits(model_mul_bits(model_add_bits(va, vb, b), c, b), vr, b)
    worst = (((1 << va) - 1) + ((1 << vb) - 1)) * abs(c) + ((1 << vr) - 1)
    assert worst < 1 << v <= 1 << (b - 1)
    assert packed.add_value_bits(packed.mul_value_bits(packed.add_value_bits(va, vb, b), c, b), vr, b) == v


def test_container_chain_carries_the_bound_without_a_device():
    pk = host_key()
    p = host_packed(pk, 40, 32, 7, v=27)
    with pytest.raises(OverflowError):
        p * 16                                           # 27 + 5 = 32 > 31
    with pytest.raises(OverflowError):
        p * -16
    q = host_packed(pk, 40, 32, 7, v=31)
    with pytest.raises(OverflowError):
        p + q                                            # max(27, 31) + 1
    with pytest.raises(OverflowError):
        PaillierPackedNumber.add_many([p, q])
    with pytest.raises(OverflowError):
        p + np.full(40, 2.0 ** 21)                       # mantissa 2^31 at exponent 10: does not fit a 32-bit slot at all
    with pytest.raises(OverflowError):
        q + np.ones(40)
    with pytest.raises(OverflowError):
        q - q


# ---- argument checks ----------------------------------------------------------------------------------------------------------
def test_constructor_checks():
    pk = host_key()
    p = host_packed(pk, 40, 32, 7)
    assert len(p) == 40 and p.slot_bits == 32 and p.slots == 7 and p.exponent == 10 and p.value_bits == 20
    assert p.ciphertext().getSize() == 6 and p.public_key == pk
    ct = ipclCipherText(pk.pubkey, [1] * 6)
    for kw in (dict(slot_bits=32, slots=7, exponent=0, value_bits=32, length=40),      # v + 1 > b
               dict(slot_bits=32, slots=7, exponent=0, value_bits=0, length=40),
               dict(slot_bits=32, slots=32, exponent=0, value_bits=5, length=40),      # k b > bits(n) - 2
               dict(slot_bits=4, slots=7, exponent=0, value_bits=2, length=40),
               dict(slot_bits=32, slots=7, exponent=0, value_bits=5, length=43),       # 43 elements need 7 rows
               dict(slot_bits=32, slots=7, exponent=0, value_bits=5, length=35)):
        with pytest.raises(ValueError):
            PaillierPackedNumber(pk, ct, **kw)
    other = host_key(2048)
    with pytest.raises(ValueError):
        PaillierPackedNumber(other, ct, slot_bits=32, slots=7, exponent=0, value_bits=5, length=40)


def test_add_rejects_mismatched_operands():
    pk = host_key()
    p = host_packed(pk, 40, 32, 7)
    for q in (host_packed(pk, 40, 16, 7, v=10), host_packed(pk, 40, 32, 8), host_packed(pk, 40, 32, 7, E=11),
              host_packed(pk, 41, 32, 7), host_packed(host_key(2048), 40, 32, 7)):
        with pytest.raises(ValueError):
            p + q
        with pytest.raises(ValueError):
            p - q
    with pytest.raises(ValueError):
        p + np.ones(39)
    with pytest.raises(ValueError):
        [1.0] * 41 + p
    with pytest.raises(ValueError):
        p + np.ones((40, 1))
    with pytest.raises(ValueError):
        p + np.array([np.nan] * 40)
    with pytest.raises(ValueError):
        host_packed(pk, 40, 32, 7, E=-1) + np.ones(40, dtype=np.int64)                # integers need E >= 0
    with pytest.raises(TypeError):
        p + "x"
    with pytest.raises(TypeError):
        p + PaillierEncryptedNumber(pk, ipclCipherText(pk.pubkey, [1] * 40), [0] * 40, 40)


def test_multiplier_must_be_one_integer():
    p = host_packed(host_key(), 40, 32, 7)
    for c in (2.0, np.float64(3), "2", [2] * 40, np.ones(40, dtype=np.int64), True, None):
        with pytest.raises(TypeError):
            p * c
    with pytest.raises(TypeError):
        1.5 * p


def test_encrypt_packed_argument_checks():
    pk = host_key()
    ok = dict(exponent=10, value_bits=20, slot_bits=32)
    for kw in (dict(ok, slot_bits=7), dict(ok, slot_bits=129), dict(ok, slots=32), dict(ok, slots=0), dict(ok, value_bits=32),
               dict(ok, value_bits=0)):
        with pytest.raises(ValueError):
            pk.encrypt_packed(np.ones(5), **kw)
    for bad in (np.ones((5, 2)), np.array([1.0, np.nan]), np.array([np.inf]), ["a"], np.array([True, False]), [1 << 80],
                np.ones(3, dtype=np.complex128)):
        with pytest.raises(ValueError):
            pk.encrypt_packed(bad, **ok)
    with pytest.raises(ValueError):
        pk.encrypt_packed(np.arange(5), exponent=-1, value_bits=20, slot_bits=32)     # integers: E >= 0
    with pytest.raises(TypeError):
        pk.encrypt_packed(np.ones(5), 10, 20, 32)                                     # keyword-only parameters


def test_pack_argument_checks():
    pk = host_key()
    x = PaillierEncryptedNumber(pk, ipclCipherText(pk.pubkey, [1] * 10), [3, 5, 4, 5, 0, 1, 2, 3, 4, 5], 10)
    for kw in (dict(slot_bits=32, value_bits=20, exponent=4),                         # below the container's maximum 5
               dict(slot_bits=7, value_bits=5), dict(slot_bits=32, value_bits=32), dict(slot_bits=32, value_bits=20, slots=32),
               dict(slot_bits=32, value_bits=0)):
        with pytest.raises(ValueError):
            x.pack(**kw)
    with pytest.raises(TypeError):
        x.pack(32, 20)


def test_decrypt_packed_checks_type_and_key():
    fx = KEYS["1024"]
    pk = host_key()
    sk = PaillierPrivateKey(pk, int(fx["p"], 16), int(fx["q"], 16))
    with pytest.raises(ValueError):
        sk.decrypt_packed(host_packed(host_key(2048), 40, 32, 7))
    with pytest.raises(ValueError):
        sk.decrypt_packed_mantissas(host_packed(host_key(2048), 40, 32, 7))
    x = PaillierEncryptedNumber(pk, ipclCipherText(pk.pubkey, [1] * 4), [0] * 4, 4)
    with pytest.raises(TypeError):
        sk.decrypt_packed(x)


def test_pickle_round_trip_of_a_host_container():
    pk = host_key()
    p = host_packed(pk, 40, 32, 7, fill=12345)
    q = pickle.loads(pickle.dumps(p))
    assert isinstance(q, PaillierPackedNumber) and q.public_key == pk and len(q) == 40
    assert (q.slot_bits, q.slots, q.exponent, q.value_bits) == (32, 7, 10, 20)
    assert [int(c) for c in q.ciphertext().getTexts()] == [12345] * 6


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pai_fp_pack", "pai_fp_unpack", "pai_ct_pack"])
def test_entry_points_are_declared_bound_and_exported(name):
    assert name in _native.PROTOTYPES
    header = (ROOT / "include" / "paillier_hip.h").read_text()
    assert re.search(r"\bint\s+%s\s*\(" % name, header)
    assert hasattr(_native.load(), name)


def test_python_surface():
    from pailliercryptolib_python_amd import engine

    for meth in ("fp_pack", "fp_unpack", "ct_pack"):
        assert callable(getattr(engine.PublicKeyHandle, meth, None))
    assert callable(getattr(PaillierPublicKey, "encrypt_packed", None))
    assert callable(getattr(PaillierEncryptedNumber, "pack", None))
    assert callable(getattr(PaillierPrivateKey, "decrypt_packed", None))
    assert callable(getattr(PaillierPrivateKey, "decrypt_packed_mantissas", None))
    for attr in ("public_key", "slot_bits", "slots", "exponent", "value_bits"):
        assert hasattr(host_packed(host_key(), 7, 32, 7), attr)
