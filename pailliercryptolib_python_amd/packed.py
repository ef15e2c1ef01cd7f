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

Everything runs on the key's home device (no multi-GPU fan-out, as for ``segment_sum``).
"""
from __future__ import annotations

import operator
from typing import List, NamedTuple, Optional

import numpy as np
import torch

from . import engine
from .bindings import ipclCipherText, merge_taint
from .paillier import ADDN_RPOW_SPAN, _cumsum_args, _segment_ids, _segment_plan

SLOT_BITS_MIN, SLOT_BITS_MAX = 8, 128


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
                   apply_obfuscator: bool = True) -> "PaillierPackedNumber":
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
        ct = pub.encrypt_words(_pack_plain(h, x, E, v, lay, "encrypt_packed"), apply_obfuscator, None)
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

    def apply_obfuscator(self, *, r: Optional[torch.Tensor] = None) -> None:
        """Re-randomise the G ciphertexts in place (pack() and the arithmetic below return canonical residues)."""
        pub = self.public_key.pubkey
        ct = self.__ct._t.clone()
        if ct.shape[0]:
            pub.handle.obfuscate_(ct, pub._draw_r(ct.shape[0]) if r is None else r)
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
