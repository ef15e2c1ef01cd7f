"""Packed ciphertexts (extension; no reference counterpart): k fixed-point slots of b bits in one Paillier plaintext.

FATE's "cipher compress" / BatchCrypt: ``prod_j ct_j^(2^(b j))`` is an encryption of ``sum_j m_j 2^(b j)``, so one ciphertext —
one decryption, one row on the wire and, when the key owner packs before encrypting, one encryption — carries k values.

The format (``include/paillier_hip.h``, "packed ciphertexts"; ``DESIGN.md`` section 2.13):

* parameters: the key, ``slot_bits`` b (8..128), ``slots`` k >= 1 with k b <= bits(n) - 2, one base-2 ``exponent`` E for the whole
  container (value = mantissa 2^-E), the logical ``length`` N and ``value_bits`` v; G = ceil(N / k) ciphertexts;
* element i lives in ciphertext i // k, slot i % k, bits [j b, (j + 1) b); unused tail slots hold 0;
* the plaintext of ciphertext g is the signed integer P_g = sum_j m_(g k + j) 2^(b j) mod n with -2^(b-1) <= m < 2^(b-1);
* unpacking: with the bias B = sum_(j<k) 2^(b-1) 2^(b j), Q = (residue + B) mod n < 2^(k b) and
  m_j = ((Q >> b j) & (2^b - 1)) - 2^(b-1);
* headroom is tracked, not guessed: ``value_bits`` is a proven bound |m| < 2^v for every slot, v + 1 <= b always; a + b gives
  max(v_a, v_b) + 1, multiplication by an integer c gives v + bit_length(|c|), and an operation whose bound would exceed b - 1
  raises ``OverflowError`` before any kernel runs.

Row operations (``DESIGN.md`` section 2.13a).  A packed container of length N is a G x k matrix, G = ceil(N / k) rows (one
ciphertext each), the tail slots of the last row 0; a product of rows modulo n^2 adds their plaintexts slot by slot, so the
middle of a histogram pipeline runs on packed rows as it does on plain ciphertexts — with one exponent for the whole container
(no alignment: every chain is pure products) and no bias (it appears only in ``pai_fp_unpack``):

* ``rows``: G;
* ``segment_sum(row_ids, num_segments)``: sums of rows by key, F * num_segments rows, feature-major (pai_ct_segment_prod);
* ``cumsum(rows_per_run=None, reverse=False)``: prefix sums along runs of rows (pai_ct_scan);
* ``sum()``: the one row that sums all of them (pai_ct_prod);
* ``take(rows)``: the selected rows in the given order (a device gather, no arithmetic);
* ``repack(factor=None)``: f consecutive rows become one row of k f slots, ``prod_(j<f) ct_(r f + j)^(2^(k b j))``
  (pai_ct_pack_step) — element i stays element i, so the result is an ordinary packed container with fewer rows to decrypt.

A sum of c members with |m| < 2^v satisfies |sum| < 2^(v + bit_length(c - 1)) (``sum_value_bits``): c is the largest member
count of a segment, the run length, or G; like the arithmetic, an operation whose bound would exceed b - 1 raises
``OverflowError`` before any Paillier kernel runs.  The results are canonical products, not re-randomised; they carry the
inversion taint of their input, and a container without rows gives one without rows.

Linear maps of rows (``DESIGN.md`` section 2.13b).  A product of POWERS of rows forms ``sum_i w_i P_i`` slot by slot, so a plaintext
matrix acts on the rows of a container — the encrypted gradient ``X.T @ [[D]]`` of a linear model with the k residual columns of a
sample in the k slots of its row, one multi-exponentiation per feature instead of k:

* ``scale_rows(c)``: row i becomes ``ct_i^(c_i)`` for integers c_i (pai_ct_mul; negative ones through the inverse);
* ``rmatmul(W, weight_exponent=0)`` / ``W @ packed``: W dense (F, G) or (G,), output row f = ``prod_i ct_i^(w_fi)``
  (pai_fp_quantize, then pai_ct_multiexp);
* ``csr_rmatmul(indptr, indices, data, shape, weight_exponent=0)`` / ``A @ packed`` for a scipy sparse A: the same over the stored
  entries of a CSR matrix (pai_fp_quantize per segment, then pai_ct_sparse_multiexp).

A container has ONE exponent, so every weight is brought to one grid: integer dtypes exactly, w = x << weight_exponent, float
dtypes as w = rint(x 2^weight_exponent) (ties to even), and the result's exponent is E + weight_exponent.  With |m| < 2^v a weighted
sum satisfies |sum_i w_i m_i| <= (2^v - 1) S < 2^(v + bit_length(S)), S = sum_i |w_i| (``weighted_sum_value_bits``); S is the largest
such sum of an output row, read from the device before any Paillier kernel runs (two read-backs per product: the extremes of
the weights, which give the exact exponent width of the multi-exponentiation, then the sums).  ``packed @ W`` is a TypeError: a
matrix on the right would have to split rows, which no operation on ciphertexts can do.

Everything runs on the key's home device (no multi-GPU fan-out, as for ``segment_sum``).
"""
from __future__ import annotations

import operator
from typing import List, NamedTuple, Optional

import numpy as np
import torch

from . import _native, engine
from .bindings import ipclCipherText, merge_taint
from .paillier import (ADDN_RPOW_SPAN, PaillierEncryptedNumber, _csr_args, _cumsum_args, _host_array, _scipy_sparse, _segment_ids,
                       _segment_plan)

SLOT_BITS_MIN, SLOT_BITS_MAX = 8, 128
WEIGHT_BITS_MAX = 126           # the widest |w| pai_fp_quantize forms
# routes taken by rmatmul / csr_rmatmul since import: "fast" = pai_ct_multiexp / pai_ct_sparse_multiexp, "composite" = gather,
# pai_ct_mul and pai_ct_segment_prod (the defining route)
PACKED_ROUTES = {"fast": 0, "composite": 0}


class Layout(NamedTuple):
    """The bit layout of a packed plaintext under a modulus of n_bits bits."""
    n_bits: int
    slot_bits: int
    slots: int

    @property
    def bias(self) -> int:
        """B = sum_(j<k) 2^(b-1) 2^(b j): added to a packed plaintext it makes every slot an unsigned b-bit field."""
        b = self.slot_bits
        return sum(1 << (b * j + b - 1) for j in range(self.slots))

    def groups(self, length: int) -> int:
        """Ciphertexts that hold `length` elements."""
        return (int(length) + self.slots - 1) // self.slots

    def tail(self, length: int) -> int:
        """Unused (zero) slots of the last ciphertext."""
        return self.groups(length) * self.slots - int(length)


def max_slots(n_bits: int, slot_bits: int) -> int:
    """The largest k with k b <= n_bits - 2."""
    return (int(n_bits) - 2) // int(slot_bits)


def layout(n_bits: int, slot_bits: int, slots: Optional[int] = None) -> Layout:
    """The checked layout: 8 <= b <= 128, k >= 1 (default: the largest the modulus allows), k b <= n_bits - 2."""
    n_bits, b = int(n_bits), operator.index(slot_bits)
    if not SLOT_BITS_MIN <= b <= SLOT_BITS_MAX:
        raise ValueError(f"packed layout: slot_bits must lie in {SLOT_BITS_MIN} .. {SLOT_BITS_MAX}, got {b}")
    k = max_slots(n_bits, b) if slots is None else operator.index(slots)
    if k < 1 or k * b > n_bits - 2:
        raise ValueError(f"packed layout: {k} slots of {b} bits do not fit a {n_bits}-bit modulus (slots * slot_bits <= bits(n) - 2)")
    return Layout(n_bits, b, k)


def check_value_bits(value_bits: int, slot_bits: int) -> int:
    """value_bits as given by a caller: 1 <= v and v + 1 <= b (ValueError otherwise)."""
    v = operator.index(value_bits)
    if v < 1 or v + 1 > slot_bits:
        raise ValueError(f"packed: value_bits must lie in 1 .. slot_bits - 1 = {slot_bits - 1}, got {v}")
    return v


def _headroom(v: int, slot_bits: int, what: str) -> int:
    if v + 1 > slot_bits:
        raise OverflowError(f"packed {what}: the result needs {v} value bits, slots of {slot_bits} bits hold {slot_bits - 1}")
    return v


def add_value_bits(va: int, vb: int, slot_bits: int) -> int:
    """|a + b| < 2^(max(va, vb) + 1); OverflowError when that exceeds slot_bits - 1."""
    return _headroom(max(int(va), int(vb)) + 1, slot_bits, "addition")


def mul_value_bits(v: int, c: int, slot_bits: int) -> int:
    """|c m| < 2^(v + bit_length(|c|)); OverflowError when that exceeds slot_bits - 1."""
    return _headroom(int(v) + abs(int(c)).bit_length(), slot_bits, "multiplication")


def sum_value_bits(v: int, count: int, slot_bits: int) -> int:
    """|sum of `count` members| < 2^(v + bit_length(count - 1)) when every |m| < 2^v (count 2^v <= 2^(v + ceil(log2 count)));
    OverflowError when that exceeds slot_bits - 1.  A sum of one member (or none) keeps v."""
    return _headroom(int(v) + max(0, int(count) - 1).bit_length(), slot_bits, "sum")


def weighted_sum_value_bits(v: int, abs_sum: int, slot_bits: int) -> int:
    """|sum_i w_i m_i| <= (2^v - 1) S < 2^(v + bit_length(S)) when every |m_i| < 2^v and S = sum_i |w_i| = abs_sum (S = 0 keeps v);
    OverflowError when that exceeds slot_bits - 1."""
    S = int(abs_sum)
    if S < 0:
        raise ValueError("weighted_sum_value_bits: abs_sum is a sum of magnitudes")
    return _headroom(int(v) + S.bit_length(), slot_bits, "weighted sum")


def _weight_exponent(weight_exponent) -> int:
    if isinstance(weight_exponent, (bool, np.bool_)) or not isinstance(weight_exponent, (int, np.integer)):
        raise TypeError(f"weight_exponent must be an integer, got {type(weight_exponent).__name__}")
    return int(weight_exponent)


def _weights(x, what: str, weight_exponent: int) -> torch.Tensor:
    """A weight array of a caller (numpy, list or torch on any device) as a float64 / int64 torch tensor of the same shape and,
    for tensors, on its own device.  TypeError for bool, complex and object dtypes; ValueError for integers that do not fit 64
    signed bits or come with a negative weight_exponent."""
    if isinstance(x, torch.Tensor):
        if x.dtype == torch.bool or x.dtype.is_complex:
            raise TypeError(f"{what}: weights must be integers or floats, got {x.dtype}")
        if x.dtype == getattr(torch, "uint64", None):
            x = torch.from_numpy(_host_array(x, what))
        t = x.detach()
    else:
        a = np.asarray(x)
        if a.dtype.kind not in "fiu":
            raise TypeError(f"{what}: weights must be integers or floats, got dtype {a.dtype}")
        if a.dtype == np.uint64:
            if a.size and int(a.max()) >= 1 << 63:
                raise ValueError(f"{what}: integer weights must fit 64 signed bits")
            a = a.astype(np.int64)
        if a.dtype == np.float16 or (a.dtype.kind == "f" and a.dtype.itemsize > 8):
            a = a.astype(np.float64)
        t = torch.from_numpy(np.ascontiguousarray(a)) if a.size else torch.zeros(a.shape, dtype=torch.float64 if a.dtype.kind == "f"
                                                                                   else torch.int64)
    if t.dtype.is_floating_point:
        return t.to(torch.float64)
    if weight_exponent < 0:
        raise ValueError(f"{what}: integer weights need a weight_exponent >= 0")
    return t.to(torch.int64)


def _weight_bits(t: torch.Tensor, weight_exponent: int, what: str) -> int:
    """The bit length of the largest |w| of a checked weight tensor (>= 1), from its extremes (one read-back): ValueError for a NaN
    or an infinity, OverflowError past WEIGHT_BITS_MAX."""
    if t.numel() == 0:
        return 1
    lo, hi = torch.stack([t.min(), t.max()]).tolist()
    if t.dtype.is_floating_point:
        from fractions import Fraction

        if not (np.isfinite(lo) and np.isfinite(hi)):
            raise ValueError(f"{what}: NaN or infinity among the weights")
        top = round(Fraction(max(abs(lo), abs(hi))) * Fraction(2) ** weight_exponent)      # ties to even, as the device rounds
    else:
        top = max(abs(int(lo)), abs(int(hi))) << weight_exponent
    bits = max(1, int(top).bit_length())
    if bits > WEIGHT_BITS_MAX:
        raise OverflowError(f"{what}: a weight of {bits} bits at weight_exponent {weight_exponent} (|w| < 2^{WEIGHT_BITS_MAX} is served)")
    return bits


def _mexp_min_terms() -> int:
    import os

    try:
        return int(os.environ.get("PAI_MEXP_MIN_TERMS", PaillierEncryptedNumber.MEXP_MIN_TERMS))
    except ValueError:
        return PaillierEncryptedNumber.MEXP_MIN_TERMS


def _row_multipliers(c, rows: int) -> np.ndarray:
    """scale_rows' argument checks: a 1-D integer array / tensor of length `rows` -> int64 (TypeError / ValueError before any launch)."""
    if isinstance(c, torch.Tensor):
        if c.dtype.is_floating_point or c.dtype.is_complex or c.dtype == torch.bool:
            raise TypeError(f"scale_rows: multipliers must have an integer dtype, got {c.dtype}")
        a = _host_array(c, "scale_rows")
    else:
        a = np.asarray(c)
        if a.size == 0 and a.dtype.kind == "f":          # an empty list
            a = a.astype(np.int64)
    if a.dtype.kind not in "iu":
        raise TypeError(f"scale_rows: multipliers must have an integer dtype, got {a.dtype}")
    if a.ndim != 1 or a.shape[0] != rows:
        raise ValueError(f"scale_rows: expected {rows} multipliers (one per row), got shape {tuple(a.shape)}")
    if a.dtype == np.uint64 and a.size and int(a.max()) >= 1 << 63:
        raise ValueError("scale_rows: multipliers must fit 64 signed bits")
    return np.ascontiguousarray(a.astype(np.int64))


def repack_factor(n_bits: int, slot_bits: int, slots: int, factor: Optional[int] = None) -> int:
    """The checked factor of repack(): f >= 1 rows of `slots` slots become one row, f slots slot_bits <= n_bits - 2 (default: the
    largest such f; ValueError through layout() for one that does not fit)."""
    f = max_slots(n_bits, slot_bits * slots) if factor is None else operator.index(factor)
    if f < 1:
        raise ValueError(f"repack: factor must be a positive integer, got {f}")
    layout(n_bits, slot_bits, slots * f)
    return f


def _take_index(rows, G: int) -> np.ndarray:
    """take()'s argument checks: a slice or a 1-D integer array / tensor -> int64 row indices in [0, G) (negative indices count from
    the end, as in numpy).  TypeError / IndexError before anything is launched."""
    if isinstance(rows, slice):
        return np.arange(*rows.indices(G), dtype=np.int64)
    if isinstance(rows, torch.Tensor):
        if rows.dtype.is_floating_point or rows.dtype.is_complex or rows.dtype == torch.bool:
            raise TypeError(f"take: rows must have an integer dtype, got {rows.dtype}")
        idx = rows.detach().cpu().numpy()
    else:
        idx = np.asarray(rows)
        if idx.size == 0 and idx.dtype.kind == "f":      # an empty list
            idx = idx.astype(np.int64)
    if idx.dtype.kind not in "iu":
        raise TypeError(f"take: rows must be a slice or an integer array, got dtype {idx.dtype}")
    if idx.ndim != 1:
        raise ValueError(f"take: rows must be 1-D, got shape {tuple(idx.shape)}")
    if idx.size and (int(idx.max()) >= G or int(idx.min()) < -G):
        raise IndexError(f"take: row index out of range for {G} rows")
    idx = idx.astype(np.int64)
    return np.where(idx < 0, idx + G, idx)


def _as_batch(values, exponent: int, what: str) -> np.ndarray:
    """A 1-D float64 or int64 array of the caller's values (ValueError for anything else, NaN / infinity, or integers at E < 0)."""
    if isinstance(values, np.ndarray):
        x = values
    else:
        try:
            x = np.asarray(list(values))
        except (TypeError, OverflowError) as e:
            raise ValueError(f"{what}: values should be a 1-D array or list of integers or floats") from e
    if x.ndim != 1 or x.dtype == bool or not (np.issubdtype(x.dtype, np.integer) or np.issubdtype(x.dtype, np.floating)):
        raise ValueError(f"{what}: values should be a 1-D array or list of integers or floats")
    if np.issubdtype(x.dtype, np.floating):
        x = np.ascontiguousarray(x, dtype=np.float64)
        if not np.all(np.isfinite(x)):
            raise ValueError(f"{what}: NaN or infinity cannot be packed")
        return x
    if x.dtype == np.uint64 and x.size and int(x.max()) >= 1 << 63:
        raise ValueError(f"{what}: integer values must fit 64 signed bits")
    if exponent < 0:
        raise ValueError(f"{what}: integer values need an exponent >= 0")
    return np.ascontiguousarray(x, dtype=np.int64)


def _measured_value_bits(x: np.ndarray, exponent: int) -> int:
    """The smallest v >= 1 with |mantissa| < 2^v for every element of a checked batch."""
    if x.size == 0:
        return 1
    if x.dtype == np.float64:
        with np.errstate(over="ignore"):
            top = float(np.ldexp(np.max(np.abs(x)), exponent))
        m = int(np.rint(top)) if np.isfinite(top) else 1 << 1100
    else:
        m = max(abs(int(x.max())), abs(int(x.min()))) << exponent
    return max(1, m.bit_length())


def _pack_plain(h: engine.PublicKeyHandle, x: np.ndarray, exponent: int, value_bits: int, lay: Layout, what: str) -> torch.Tensor:
    """Residues [G, n_words] of a checked batch (pai_fp_pack); ValueError when a mantissa reaches 2^value_bits."""
    xs = torch.from_numpy(x).to(h.device)
    m, flag = h.fp_pack(xs, exponent, value_bits, lay.slot_bits, lay.slots)
    f = int(flag.item())
    if f & 2:
        raise ValueError(f"{what}: NaN or infinity cannot be packed")
    if f & 1:
        raise ValueError(f"{what}: a mantissa at exponent {exponent} does not satisfy |m| < 2^{value_bits}")
    return m


def _key_layout(public_key, slot_bits, slots) -> Layout:
    return layout(public_key.n.bit_length(), slot_bits, slots)


def encrypt_packed(public_key, values, *, exponent: int, value_bits: int, slot_bits: int, slots: Optional[int] = None,
                   apply_obfuscator: bool = True, r: Optional[torch.Tensor] = None, _encrypt_words=None) -> "PaillierPackedNumber":
    """PaillierPublicKey.encrypt_packed: encode and pack on the device, then encrypt G = ceil(N / k) rows."""
    lay = _key_layout(public_key, slot_bits, slots)
    v = check_value_bits(value_bits, lay.slot_bits)
    E = operator.index(exponent)
    x = _as_batch(values, E, "encrypt_packed")
    pub = public_key.pubkey
    h = pub.handle
    if x.size == 0:
        ct = h.empty_ct(0)
    else:
        ct = (pub.encrypt_words if _encrypt_words is None else _encrypt_words)(_pack_plain(h, x, E, v, lay, "encrypt_packed"),
                                                                               apply_obfuscator, r)
    return PaillierPackedNumber(public_key, ipclCipherText(pub, ct), slot_bits=lay.slot_bits, slots=lay.slots, exponent=E,
                                value_bits=v, length=x.shape[0])


def pack_encrypted(enc, *, slot_bits: int, value_bits: int, exponent: Optional[int] = None, slots: Optional[int] = None
                   ) -> "PaillierPackedNumber":
    """PaillierEncryptedNumber.pack: bring every element to one exponent, then one Horner chain per output row (pai_ct_pack)."""
    public_key = enc.public_key
    lay = _key_layout(public_key, slot_bits, slots)
    v = check_value_bits(value_bits, lay.slot_bits)
    expo = np.asarray(enc._expo, dtype=np.int64)
    N = len(enc)
    top = int(expo.max()) if N else 0
    E = top if exponent is None else operator.index(exponent)
    if E < top:
        raise ValueError(f"pack: exponent {E} is below the container's largest exponent {top} (exponents can only be raised)")
    pub = public_key.pubkey
    h = pub.handle
    if N == 0:
        out = h.empty_ct(0)
    else:
        words = enc.words                                 # wire form; pending inversion outcomes are checked here
        delta = (E - expo).astype(np.int32)
        if (delta > 0).any():
            words = h.ct_pow2_(words.clone(), delta)
        out = h.ct_pack(words, lay.slot_bits, lay.slots)
    return PaillierPackedNumber(public_key, ipclCipherText(pub, out), slot_bits=lay.slot_bits, slots=lay.slots, exponent=E,
                                value_bits=v, length=N)


def _decrypt_fields(private_handle_decrypt, pub_handle, p: "PaillierPackedNumber"):
    """(mantissa tensor on the host, wide) of a packed container: pai_decrypt on G rows, pai_fp_unpack on the device."""
    N = len(p)
    wide = p.slot_bits > 64
    if N == 0:
        return np.zeros((0, 2) if wide else (0,), dtype=np.int64), wide
    t = private_handle_decrypt(p.ciphertext().words)
    out, flag = pub_handle.fp_unpack(t, p.slot_bits, p.slots)
    f = flag.cpu().numpy()
    if (f == 2).any():
        raise ValueError("Attempted to decode corrupted number")
    if (f == 1).any():
        raise OverflowError(f"Overflow detected in packed ciphertext {int(np.nonzero(f == 1)[0][0])}: a slot left its {p.slot_bits} bits")
    return out.cpu().numpy()[:N], wide


def mantissas_to_ints(m: np.ndarray, wide: bool) -> List[int]:
    if not wide:
        return [int(v) for v in m]
    lo = m[:, 0].view(np.uint64)
    return [(int(h) << 64) + int(l) for l, h in zip(lo, m[:, 1])]


def mantissas_to_float64(m: np.ndarray, wide: bool, exponent: int) -> np.ndarray:
    """mantissa 2^-exponent as float64: exact whenever the mantissa has at most 53 significant bits (|m| < 2^53 in particular)."""
    if not wide:
        return np.ldexp(m.astype(np.float64), -exponent)
    # (low, high) two's-complement pairs: the magnitude's halves are converted separately (each keeps its share of the
    # significant bits), high 2^(64 - E) + low 2^-E, then the sign
    lo = np.ascontiguousarray(m[:, 0]).view(np.uint64)
    hi = np.ascontiguousarray(m[:, 1]).view(np.uint64)
    neg = m[:, 1] < 0
    mlo = np.where(neg, ~lo + np.uint64(1), lo)
    mhi = np.where(neg, ~hi + (lo == 0).astype(np.uint64), hi)
    mag = np.ldexp(mhi.astype(np.float64), 64 - exponent) + np.ldexp(mlo.astype(np.float64), -exponent)
    return np.where(neg, -mag, mag)


class PaillierPackedNumber:
    """G = ceil(N / slots) ciphertexts that hold N fixed-point values, `slots` per plaintext (module docstring: the format)."""

    def __init__(self, public_key, ciphertext: ipclCipherText, *, slot_bits: int, slots: int, exponent: int, value_bits: int,
                 length: int):
        if ciphertext.public_key != public_key.pubkey:
            raise ValueError("PaillierPackedNumber: public key mismatch")
        lay = _key_layout(public_key, slot_bits, slots)
        self.public_key = public_key
        self.slot_bits, self.slots = lay.slot_bits, lay.slots
        self.exponent = operator.index(exponent)
        self.value_bits = check_value_bits(value_bits, lay.slot_bits)
        self.__length = operator.index(length)
        if self.__length < 0 or ciphertext.getSize() != lay.groups(self.__length):
            raise ValueError(f"PaillierPackedNumber: {self.__length} elements in {lay.slots} slots need {lay.groups(self.__length)} "
                             f"ciphertexts, got {ciphertext.getSize()}")
        self.__ct = ciphertext

    __array_ufunc__ = None                               # array + packed and numpy_int * packed come to __radd__ / __rmul__

    # -- container ----------------------------------------------------------------------------------
    @property
    def layout(self) -> Layout:
        return Layout(self.public_key.n.bit_length(), self.slot_bits, self.slots)

    def __len__(self) -> int:
        return self.__length

    def ciphertext(self) -> ipclCipherText:
        """The G-row ciphertext container."""
        return self.__ct

    def __repr__(self):
        return (f"<PaillierPackedNumber {self.__length} x {self.slot_bits} bits in {self.__ct.getSize()} ciphertexts, "
                f"exponent {self.exponent}, value_bits {self.value_bits}>")

    def __getstate__(self) -> tuple:
        return (self.public_key, self.__length, self.slot_bits, self.slots, self.exponent, self.value_bits,
                [int(b) for b in self.__ct.getTexts()])

    def __setstate__(self, state: tuple):
        (self.public_key, self.__length, self.slot_bits, self.slots, self.exponent, self.value_bits, ints) = state
        self.__ct = ipclCipherText(self.public_key.pubkey, [int(i) for i in ints])

    def _like(self, ct: torch.Tensor, value_bits: int, taint: tuple = ()) -> "PaillierPackedNumber":
        return PaillierPackedNumber(self.public_key, ipclCipherText(self.public_key.pubkey, ct, taint=taint), slot_bits=self.slot_bits,
                                    slots=self.slots, exponent=self.exponent, value_bits=value_bits, length=self.__length)

    def _rows_like(self, ct, value_bits: int, *, slots: Optional[int] = None, length: Optional[int] = None, dom: int = 0
                   ) -> "PaillierPackedNumber":
        """The result of a row operation: rows `ct` (a device tensor at domain tag `dom`, or host words), whole rows of `slots`
        slots unless `length` says otherwise; this container's inversion taint travels with it."""
        k = self.slots if slots is None else slots
        c = ipclCipherText(self.public_key.pubkey, ct, dom=dom, taint=self.__ct._taint)
        return PaillierPackedNumber(self.public_key, c, slot_bits=self.slot_bits, slots=k, exponent=self.exponent,
                                    value_bits=value_bits, length=c.getSize() * k if length is None else length)

    def _no_rows(self):
        return np.zeros((0, 2 * ((self.public_key.n.bit_length() + 31) // 32)), dtype=np.uint32)

    def _tagged(self, h):
        """(rows on the device, domain tag) for the chain runners that take tagged rows (a cumsum() result rests at tag 1)"""
        t, dom = self.__ct._raw()
        if abs(dom) > ADDN_RPOW_SPAN - 2:
            t, dom = h.ct_retag(t, dom, 0), 0
        return t, dom

    @property
    def rows(self) -> int:
        """G: the ciphertexts of this container."""
        return self.__ct.getSize()

    def apply_obfuscator(self, *, r: Optional[torch.Tensor] = None, _obfuscate=None) -> None:
        """Re-randomise the G ciphertexts in place (pack() and the arithmetic below return canonical residues).
        (_obfuscate, private: PaillierPrivateKey.apply_obfuscator's route.)"""
        pub = self.public_key.pubkey
        ct = self.__ct._t.clone()
        if ct.shape[0]:
            (pub.handle.obfuscate_ if _obfuscate is None else _obfuscate)(ct, pub._draw_r(ct.shape[0]) if r is None else r)
        self.__ct = ipclCipherText(pub, ct, taint=self.__ct._taint)

    # -- arithmetic (slot-wise) ---------------------------------------------------------------------
    def _same_shape(self, other: "PaillierPackedNumber") -> None:
        if self.public_key != other.public_key:
            raise ValueError("PaillierPackedNumber: PublicKey mismatch")
        mine = (self.slot_bits, self.slots, self.exponent, self.__length)
        theirs = (other.slot_bits, other.slots, other.exponent, len(other))
        if mine != theirs:
            raise ValueError(f"PaillierPackedNumber: (slot_bits, slots, exponent, length) differ: {mine} and {theirs}")

    def __add__(self, other):
        pub = self.public_key.pubkey                     # (the device handle only after every check: errors launch nothing)
        if isinstance(other, PaillierPackedNumber):
            self._same_shape(other)
            v = add_value_bits(self.value_bits, other.value_bits, self.slot_bits)
            oc = other.ciphertext()
            taint = merge_taint(self.__ct._taint, oc._taint)
            if self.__length == 0:
                return self._like(pub.handle.empty_ct(0), v, taint)
            return self._like(pub.handle.ct_add(self.__ct._t, oc._t), v, taint)
        if np.isscalar(other) and isinstance(other, (int, float, np.integer, np.floating)) and not isinstance(other, (bool, np.bool_)):
            other = np.full(self.__length, other)
        if not isinstance(other, (np.ndarray, list)):
            return NotImplemented
        if len(other) != self.__length:
            raise ValueError("PaillierPackedNumber.__add__: array(list) size mismatch with PaillierPackedNumber")
        x = _as_batch(other, self.exponent, "PaillierPackedNumber.__add__")
        vx = _headroom(_measured_value_bits(x, self.exponent), self.slot_bits, "addend")
        v = add_value_bits(self.value_bits, vx, self.slot_bits)
        h = pub.handle
        if self.__length == 0:
            return self._like(h.empty_ct(0), v, self.__ct._taint)
        m = _pack_plain(h, x, self.exponent, vx, self.layout, "PaillierPackedNumber.__add__")
        return self._like(h.ct_add_plain(self.__ct._t, m), v, self.__ct._taint)

    def __radd__(self, other):
        return self + other

    def __mul__(self, c):
        if isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, np.integer)):
            raise TypeError(f"PaillierPackedNumber.__mul__: one integer multiplies every slot, got {type(c).__name__}")
        c = int(c)
        v = mul_value_bits(self.value_bits, c, self.slot_bits)
        pub = self.public_key.pubkey
        h = pub.handle
        ct, taint = self.__ct._t, self.__ct._taint
        if self.__length == 0 or c == 1:
            return self._like(ct.clone(), v, taint)
        if c == 0:                                       # ct^0 = 1, the raw encryption of an all-zero row
            return self._like(h.raw_encrypt(torch.zeros((ct.shape[0], h.n_words), dtype=torch.int32, device=h.device)), v)
        if c < 0:
            flag = h.new_flag()                          # the inversion's outcome travels with the result
            ct = h.ct_invert(ct, flag=flag)
            taint = merge_taint(taint, (flag,))
            if c == -1:
                return self._like(ct, v, taint)
        bits = abs(c).bit_length()
        ew = (bits + 31) // 32
        return self._like(pub.ct_mul_words(ct, engine.ints_to_words([abs(c)], ew), bits), v, taint)

    def __rmul__(self, c):
        return self * c

    def __neg__(self):
        return self * -1

    def __sub__(self, other):
        if isinstance(other, list):
            other = np.asarray(other)
        if not isinstance(other, (PaillierPackedNumber, np.ndarray)) and not np.isscalar(other):
            return NotImplemented
        if isinstance(other, PaillierPackedNumber):      # both checks before the inversion behind other * -1 is launched
            self._same_shape(other)
            add_value_bits(self.value_bits, mul_value_bits(other.value_bits, -1, self.slot_bits), self.slot_bits)
        return self + (other * -1)

    def __rsub__(self, other):
        return (self * -1) + other

    @staticmethod
    def add_many(items) -> "PaillierPackedNumber":
        """The sum of several packed containers (a chain of additions; every step checks the headroom)."""
        items = list(items)
        if not items:
            raise ValueError("PaillierPackedNumber.add_many: nothing to add")
        acc = items[0]
        for it in items[1:]:
            acc = acc + it
        return acc

    # -- row operations (module docstring; slot-wise on the plaintexts) ------------------------------------------------------------
    def segment_sum(self, row_ids, num_segments: int) -> "PaillierPackedNumber":
        """Sums of rows by key: the encrypted histograms of GH-packed samples.  row_ids: an integer numpy array or torch tensor of
        shape (G,) or (G, F), G = self.rows (the rules and errors of PaillierEncryptedNumber.segment_sum); a negative id drops
        that (row, feature) pair.  The result has F * num_segments rows, feature-major: row f * num_segments + b is the product
        modulo n^2 of the rows i with row_ids[i, f] == b, so each of its slots is the sum of that slot over those rows; an empty
        segment gives the ciphertext 1 (all slots 0).  Same slot_bits, slots and exponent; value_bits grows by
        bit_length(c - 1), c the largest member count of a segment (one scalar read from the plan), OverflowError before any
        Paillier kernel when that leaves the slot.  The outputs are NOT re-randomised (as PaillierEncryptedNumber.segment_sum):
        an empty bin is recognisable as 1 — call .apply_obfuscator() on the result before the histogram leaves the party."""
        G = self.rows
        ids = _segment_ids(row_ids, G, num_segments)
        K = int(num_segments)
        if G == 0:                                       # no rows in, no rows out (as every row operation)
            return self._rows_like(self._no_rows(), self.value_bits)
        h = self.public_key.pubkey.handle
        # one exponent for the whole container: nothing to sort by, every shift 0 (NULL) — the chains are pure products
        rows, _, offsets, _ = _segment_plan(ids.to(h.device), np.zeros(G, dtype=np.int64), K)
        v = sum_value_bits(self.value_bits, int((offsets[1:] - offsets[:-1]).max()), self.slot_bits)
        t, dom = self._tagged(h)
        return self._rows_like(h.ct_segment_prod(t, rows, None, offsets, tag=dom), v)

    def cumsum(self, rows_per_run: Optional[int] = None, *, reverse: bool = False) -> "PaillierPackedNumber":
        """Prefix sums along rows: the G rows are G / rows_per_run contiguous runs (None: one run; the rules and errors of
        PaillierEncryptedNumber.cumsum) — the feature-major layout segment_sum produces, so h.cumsum(num_segments) is the
        cumulative histogram of every feature and slot.  Row i of the result is the product of its run's rows from the run's
        start through i; with reverse=True, from i to the run's end.  The result has rows * slots elements (the tail slots of
        the last row are sums now); value_bits grows by bit_length(rows_per_run - 1).  Not re-randomised: the first row of a
        run is the input row itself.  (The rows rest at the Montgomery tag where pai_ct_scan's products are closed; whoever
        reads them — ciphertext().getTexts(), pickling, decryption, the arithmetic — gets the wire form.)"""
        G = self.rows
        L = _cumsum_args(rows_per_run, G)
        if G == 0:
            return self._rows_like(self._no_rows(), self.value_bits)
        v = sum_value_bits(self.value_bits, L, self.slot_bits)
        h = self.public_key.pubkey.handle
        t, dom = self._tagged(h)
        return self._rows_like(h.ct_scan(t, L, tag=dom, dom_out=1, reverse=bool(reverse)), v, dom=1)

    def sum(self) -> "PaillierPackedNumber":
        """One row, the product of all G rows: slot j holds the sum of slot j over the rows (length `slots`); value_bits grows by
        bit_length(G - 1).  Not re-randomised."""
        G = self.rows
        if G == 0:
            return self._rows_like(self._no_rows(), self.value_bits)
        v = sum_value_bits(self.value_bits, G, self.slot_bits)
        h = self.public_key.pubkey.handle
        return self._rows_like(h.ct_prod(self.__ct._t.contiguous(), 1), v)

    def take(self, rows) -> "PaillierPackedNumber":
        """The selected rows in the given order (the shuffle / split-candidate step of the protocol): `rows` is a slice or a 1-D
        integer array or tensor of row indices (negative ones count from the end; IndexError outside [-G, G)).  A device gather
        with no arithmetic: value_bits is unchanged, the result has len(rows) * slots elements."""
        idx = _take_index(rows, self.rows)
        if idx.size == 0:
            return self._rows_like(self._no_rows(), self.value_bits)
        t, dom = self.__ct._raw()
        return self._rows_like(t.index_select(0, torch.from_numpy(idx).to(t.device)), self.value_bits, dom=dom)

    def repack(self, *, factor: Optional[int] = None) -> "PaillierPackedNumber":
        """`factor` consecutive rows become one row of slots * factor slots of the same width: output row r is
        prod_(j<f) ct_(r f + j)^(2^(slots slot_bits j)) mod n^2 (pai_ct_pack_step), so element i stays element i — row
        i // (slots f), slot i % (slots f) — and the result is an ordinary packed container of the same length with
        ceil(G / f) rows to send and decrypt.  factor defaults to the largest that fits (f slots slot_bits <= bits(n) - 2); one
        that does not fit is a ValueError.  value_bits is unchanged (no slot is added to); factor 1 returns a copy."""
        f = repack_factor(self.public_key.n.bit_length(), self.slot_bits, self.slots, factor)
        G = self.rows
        if G == 0:
            return self._rows_like(self._no_rows(), self.value_bits, slots=self.slots * f, length=0)
        h = self.public_key.pubkey.handle
        if f == 1:
            t, dom = self.__ct._raw()
            return self._rows_like(t.clone(), self.value_bits, length=self.__length, dom=dom)
        t, dom = self._tagged(h)
        out = h.ct_pack_step(t, self.slots * self.slot_bits, f, tag=dom)
        return self._rows_like(out, self.value_bits, slots=self.slots * f, length=self.__length)

    # -- linear maps of rows (module docstring) -----------------------------------------------------------
    def __array__(self, dtype=None, copy=None):
        """A 0-d object array holding self (as PaillierEncryptedNumber.__array__): scipy's `A @ packed` then returns NotImplemented
        and Python calls __rmatmul__."""
        a = np.empty((), dtype=object)
        a[()] = self
        return a

    def _pow_rows(self, h, ct: torch.Tensor, e: torch.Tensor, sign: Optional[torch.Tensor], bits: int, taint: tuple):
        """(ct_i^(+-e_i), taint): e int32 [N, ew] magnitudes on the device, sign bool [N] or None (all non-negative): the rows with
        a negative multiplier are inverted first (pai_ct_invert_flag, its word joins the taint), then one pai_ct_mul."""
        if sign is not None:
            idx = torch.nonzero(sign).reshape(-1)
            if idx.numel():
                flag = h.new_flag()
                taint = merge_taint(taint, (flag,))
                if idx.numel() == ct.shape[0]:
                    ct = h.ct_invert(ct, flag=flag)
                else:
                    ct = ct.clone()
                    ct[idx] = h.ct_invert(ct[idx].contiguous(), flag=flag)
        return h.ct_mul(ct, e, bits), taint              # on the home device, as everything here (no fan-out)

    def scale_rows(self, c) -> "PaillierPackedNumber":
        """Row i becomes ct_i^(c_i) mod n^2: every slot of row i is multiplied by the integer c_i.  c: a 1-D integer array or tensor
        of length `rows` (TypeError for floats or bools, ValueError for another length).  A negative c_i goes through the inverse of
        the row (the inversion's outcome travels with the result, as for `* -1`), c_i = 0 gives the ciphertext 1.  value_bits
        becomes v + bit_length(max |c_i|), OverflowError before any launch when that leaves the slot.  Not re-randomised (a row
        with c_i = 0 or 1 is recognisable): call .apply_obfuscator() on the result before it leaves the party."""
        G = self.rows
        c64 = _row_multipliers(c, G)
        if G == 0:
            return self._rows_like(self._no_rows(), self.value_bits)
        mag = np.abs(c64).view(np.uint64)                # (|-2^63| wraps back to the bit pattern of 2^63)
        bits = int(mag.max()).bit_length()
        v = _headroom(self.value_bits + bits, self.slot_bits, "scale_rows")
        h = self.public_key.pubkey.handle
        ew = (max(bits, 1) + 31) // 32
        e = mag.view(np.uint32).reshape(-1, 2)
        e = engine.to_device_words(e if ew == 2 else e[:, :1], h.device)
        neg = c64 < 0
        sign = torch.from_numpy(neg).to(h.device) if neg.any() else None
        out, taint = self._pow_rows(h, self.__ct._t, e, sign, max(bits, 1), self.__ct._taint)
        return PaillierPackedNumber(self.public_key, ipclCipherText(self.public_key.pubkey, out, taint=taint), slot_bits=self.slot_bits,
                                    slots=self.slots, exponent=self.exponent, value_bits=v, length=G * self.slots)

    def _linear_result(self, out, v: int, we: int, taint: tuple) -> "PaillierPackedNumber":
        c = ipclCipherText(self.public_key.pubkey, out, taint=taint)
        return PaillierPackedNumber(self.public_key, c, slot_bits=self.slot_bits, slots=self.slots, exponent=self.exponent + we,
                                    value_bits=v, length=c.getSize() * self.slots)

    def _composite(self, h, base: torch.Tensor, e: torch.Tensor, sign: torch.Tensor, neg: bool, bits: int, offsets: torch.Tensor):
        """The defining route of the linear maps: gather the term rows (terms in segment order), raise each to its weight
        (pai_ct_mul, as scale_rows), multiply the terms of every segment (pai_ct_segment_prod, as segment_sum; an empty segment
        gives 1).  The headroom was settled by the caller from the exact sums, so the per-step bounds of scale_rows and
        segment_sum (each looser than the weighted bound) are not applied in between."""
        PACKED_ROUTES["composite"] += 1
        terms, taint = self._pow_rows(h, self.__ct._t.index_select(0, base), e, sign.to(torch.bool) if neg else None, bits,
                                      self.__ct._taint)
        return h.ct_segment_prod(terms, None, None, offsets), taint

    @staticmethod
    def _quantized(h, x: torch.Tensor, we: int, bits: int, offsets: Optional[torch.Tensor], what: str):
        """pai_fp_quantize and its read-back (flag, any w < 0 and the sums in one copy): (e, sign, S = the largest sum of |w|,
        any w < 0).  `bits` comes from _weight_bits, which has already rejected NaN, infinity and |w| >= 2^126 and is the exact
        width of the largest |w| — the multi-exponentiation's cost follows it, so it is not replaced by the cap — hence the
        kernel's flag can only confirm it here; the two branches are the cross-check of the host rounding against the device's."""
        e, sign, sums, flag = h.fp_quantize(x, we, bits, (bits + 31) // 32, offsets)
        back = torch.cat([flag.to(torch.int64), sign.any().to(torch.int64).reshape(1), sums.reshape(-1)]).cpu().numpy()
        if back[0] & 2:
            raise ValueError(f"{what}: NaN or infinity among the weights")
        if back[0] & 1:
            raise OverflowError(f"{what}: a weight does not satisfy |w| < 2^{bits}")
        pairs = back[2:].view(np.uint64).reshape(-1, 2)
        S = max(((int(hi) << 64) + int(lo) for lo, hi in pairs), default=0)
        return e, sign, S, bool(back[1])

    def rmatmul(self, W, *, weight_exponent: int = 0) -> "PaillierPackedNumber":
        """W @ self for a plaintext dense W of shape (F, G), or (G,) for one output row, G = self.rows (numpy, list, or torch on
        any device): output row f is prod_i ct_i^(w_fi) mod n^2, so slot j of it holds sum_i w_fi m_(i,j) — with the k residuals of
        sample i in row i and W = X.T this is the encrypted gradient of all k outputs, one multi-exponentiation per feature.
        Integer dtypes are taken exactly as w = x << weight_exponent, float dtypes are rounded to w = rint(x 2^weight_exponent)
        (ties to even); the result has F rows and F * slots elements, the same slot_bits and slots, exponent E + weight_exponent,
        and value_bits v + bit_length(S), S = max_f sum_i |w_fi| (weighted_sum_value_bits), read from the device before any
        Paillier kernel runs.  Raises, launching no Paillier kernel: ValueError for a NaN or an infinity, OverflowError for
        |w| >= 2^126 and when the bound leaves the slot; TypeError / ValueError for dtypes and shapes before anything is launched.
        Routes with identical bits: pai_fp_quantize, pai_ct_invert when a weight is negative, pai_ct_multiexp; or, below
        PAI_MEXP_MIN_TERMS weights (the knob of PaillierEncryptedNumber.__matmul__) and for sizes the multi-exponentiation does not
        serve, term by term (PACKED_ROUTES counts both).  The outputs are canonical products, NOT re-randomised, and carry the
        input's inversion taint plus the word of an inversion made here: call .apply_obfuscator() on the result before it leaves
        the party."""
        we = _weight_exponent(weight_exponent)
        w = _weights(W, "rmatmul", we)
        G = self.rows
        if w.dim() == 1:
            w = w.reshape(1, -1)
        if w.dim() != 2 or w.shape[1] != G:
            raise ValueError(f"rmatmul: weights must have shape (F, {G}) or ({G},), got {tuple(w.shape)}")
        F = w.shape[0]
        if G == 0 or F == 0:
            return self._linear_result(self._no_rows(), self.value_bits, we, self.__ct._taint)
        h = self.public_key.pubkey.handle
        w = w.to(h.device)
        bits = _weight_bits(w, we, "rmatmul")
        e, sign, S, neg = self._quantized(h, w.t(), we, bits, None, "rmatmul")      # [G, F]: member-major, as pai_ct_multiexp reads
        v = weighted_sum_value_bits(self.value_bits, S, self.slot_bits)
        ct, taint = self.__ct._t, self.__ct._taint
        if F * G >= _mexp_min_terms() and F * G < 1 << 31 and G < 1 << 28:
            flag = h.new_flag() if neg else None
            inv = h.ct_invert(ct, flag=flag) if neg else None
            try:
                out = h.ct_multiexp(ct, inv, 1, G, F, e.reshape(1, G, F, -1), bits, sign if neg else None)
            except _native.NativeError as exc:
                if exc.code != _native.PAI_E_UNSUPPORTED:
                    raise
            else:
                PACKED_ROUTES["fast"] += 1
                return self._linear_result(out, v, we, merge_taint(taint, (flag,)) if neg else taint)
        # terms in output order: term f G + i is row i raised to w_fi
        dev = h.device
        base = torch.arange(G, device=dev).repeat(F)
        offsets = torch.arange(F + 1, device=dev, dtype=torch.int64) * G
        out, taint = self._composite(h, base, e.permute(1, 0, 2).reshape(F * G, -1).contiguous(), sign.t().reshape(-1), neg, bits, offsets)
        return self._linear_result(out, v, we, taint)

    def csr_rmatmul(self, indptr, indices, data, shape, *, weight_exponent: int = 0) -> "PaillierPackedNumber":
        """A @ self for a plaintext sparse A of shape (m, G), G = self.rows, given as CSR arrays (numpy, or torch on any device; no
        scipy needed) under the argument rules and errors of PaillierEncryptedNumber.csr_rmatmul: output row i is the product of
        ct_l^(w) over the STORED entries (i, l) — explicit zeros and duplicates count as terms, a row of A without stored entries
        gives the ciphertext 1 (all slots 0).  Weights, exponent, headroom (S = the largest per-row sum of |w|, from the device),
        errors and taint as for rmatmul; the fast route is pai_ct_sparse_multiexp on the CSR arrays as they are (d_base = indices,
        d_offsets = indptr), the term-by-term route is taken below PAI_MEXP_MIN_TERMS stored entries.  NOT re-randomised (a row
        without entries is recognisable as 1): call .apply_obfuscator() on the result before it leaves the party."""
        we = _weight_exponent(weight_exponent)
        G = self.rows
        ptr, idx, d, (m, n, k) = _csr_args(indptr, indices, data, shape, G, True)
        if k != 1:
            raise ValueError(f"csr_rmatmul: the matrix must have {G} columns (one per row of the container), got {n}")
        w = _weights(d, "csr_rmatmul", we)
        h = self.public_key.pubkey.handle
        dev = h.device
        w, offsets, base = w.to(dev), ptr.to(dev), idx.to(dev)
        T = w.shape[0]
        if T == 0:                                       # no stored entry: every row is the ciphertext 1
            one = h.raw_encrypt(torch.zeros((m, h.n_words), dtype=torch.int32, device=dev))
            return self._linear_result(one, self.value_bits, we, self.__ct._taint)
        bits = _weight_bits(w, we, "csr_rmatmul")
        e, sign, S, neg = self._quantized(h, w, we, bits, offsets, "csr_rmatmul")
        v = weighted_sum_value_bits(self.value_bits, S, self.slot_bits)
        ct, taint = self.__ct._t, self.__ct._taint
        if T >= _mexp_min_terms() and T < 1 << 31 and G < 1 << 28:
            flag = h.new_flag() if neg else None
            inv = h.ct_invert(ct, flag=flag) if neg else None
            try:
                out = h.ct_sparse_multiexp(ct, inv, base.to(torch.int32), e, bits, sign if neg else None, offsets)
            except _native.NativeError as exc:
                if exc.code != _native.PAI_E_UNSUPPORTED:
                    raise
            else:
                PACKED_ROUTES["fast"] += 1
                return self._linear_result(out, v, we, merge_taint(taint, (flag,)) if neg else taint)
        out, taint = self._composite(h, base, e, sign, neg, bits, offsets)
        return self._linear_result(out, v, we, taint)

    def __rmatmul__(self, other):
        """W @ packed: rmatmul for a dense W (weight_exponent 0), csr_rmatmul for a scipy sparse one."""
        sp = _scipy_sparse(other)
        if sp is not None:
            return self.csr_rmatmul(sp.indptr, sp.indices, sp.data, sp.shape)
        return self.rmatmul(other)

    def __matmul__(self, other):
        raise TypeError("PaillierPackedNumber @ W is not defined: a matrix on the right would have to split rows (the slots of a "
                        "ciphertext), which no operation on ciphertexts does; W @ packed combines whole rows")
