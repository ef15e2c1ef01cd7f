"""Threshold decryption (extension; no reference counterpart): t of l parties decrypt together, nobody holds p and q afterwards.

The scheme is Damgard-Jurik / Fouque-Poupard-Stern at s = 1 with a trusted dealer, for honest-but-curious parties: there are NO
verification keys and NO zero-knowledge proofs, so a shareholder who sends a wrong partial decryption is detected only in so far
as the combined value fails the test c' = 1 (mod n) — it is not identified, and a wrong value that passes the test is accepted.

  dealer     lambda = lcm(p - 1, q - 1), gcd(n, lambda) = 1 required; d = 0 (mod lambda), d = 1 (mod n), 0 <= d < n lambda;
             f(X) = d + a_1 X + ... + a_(t-1) X^(t-1), a_k uniform in [0, n lambda); s_i = f(i) mod n lambda for i = 1 .. l
  partial    c_i = c^(2 Delta s_i) mod n^2, Delta = l!  (the exponent is not reduced: the shareholder does not know n lambda)
  combine    mu_i = Delta prod_(j in S, j != i) j / (j - i) (an integer);  c' = prod c_i^(2 mu_i) = c^(4 Delta^2 d)
             = 1 + (4 Delta^2 m mod n) n;  m = ((c' - 1) / n) theta mod n with theta = (4 Delta^2)^-1 mod n.
             Negative mu_i go on a second product: c' = P+ (P-)^-1 — one batch inversion per combine.

1 <= t <= l <= 16 (a condition of the combine's n-ary product, and Delta stays below 2^45).  The integer helpers deal / lagrange /
theta need no GPU; the classes run on the key's home device (pai_partial_decrypt, pai_threshold_combine)."""
from __future__ import annotations

import math
import secrets
import struct
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

MAX_PARTIES = 16
MU_WORDS = 4                         # words per coefficient 2 |mu_i| at the C ABI (|2 mu_i| < 2^66 for l <= 16)
MU_BITS_MAX = 66


# ---- integers only ------------------------------------------------------------------------------------------------------------------
def _check_shape(parties: int, threshold: int) -> None:
    if not (isinstance(parties, int) and isinstance(threshold, int)):
        raise TypeError("threshold sharing: parties and threshold must be integers")
    if not 1 <= parties <= MAX_PARTIES:
        raise ValueError(f"threshold sharing: parties must lie in 1 .. {MAX_PARTIES}, got {parties}")
    if not 1 <= threshold <= parties:
        raise ValueError(f"threshold sharing: threshold must lie in 1 .. parties = {parties}, got {threshold}")


def delta(parties: int) -> int:
    return math.factorial(parties)


def deal(p: int, q: int, parties: int, threshold: int, rng: Callable[[int], int]) -> Tuple[int, List[int]]:
    """(d, [s_1 .. s_l]): the dealer's secret and the shares f(i) mod n lambda.  rng(bound) returns a uniform integer in
    [0, bound) (secrets.randbelow, or SeededRng for reproducible tests).  ValueError when gcd(n, lambda) != 1."""
    _check_shape(parties, threshold)
    n = p * q
    lam = math.lcm(p - 1, q - 1)
    if p == q or math.gcd(n, lam) != 1:
        raise ValueError("threshold sharing: n is not coprime to lcm(p - 1, q - 1): this key cannot be shared")
    d = lam * pow(lam, -1, n)                                # 0 (mod lambda), 1 (mod n), below n lambda
    mod = n * lam
    coeff = [d] + [rng(mod) for _ in range(threshold - 1)]
    if any(not 0 <= a < mod for a in coeff):
        raise ValueError("threshold sharing: rng left [0, bound)")
    shares = []
    for i in range(1, parties + 1):
        acc = 0
        for a in reversed(coeff):                            # Horner
            acc = (acc * i + a) % mod
        shares.append(acc)
    return d, shares


def lagrange(indices: Sequence[int], parties: int) -> Tuple[List[int], List[bool]]:
    """(|mu_i|, mu_i < 0) for i in `indices` (distinct, in 1 .. parties): mu_i = parties! prod_(j != i) j / (j - i), an integer
    with sum mu_i f(i) = parties! f(0) for every polynomial of degree < len(indices)."""
    idx = [int(i) for i in indices]
    if not idx or len(set(idx)) != len(idx) or any(not 1 <= i <= parties for i in idx):
        raise ValueError(f"lagrange: indices must be distinct and lie in 1 .. {parties}")
    D = delta(parties)
    mags, negs = [], []
    for i in idx:
        num, den = D, 1
        for j in idx:
            if j != i:
                num *= j
                den *= j - i
        mu, rem = divmod(num, den)
        assert rem == 0, "Delta clears every Lagrange denominator"
        mags.append(abs(mu))
        negs.append(mu < 0)
    return mags, negs


def theta(n: int, parties: int) -> int:
    """(4 Delta^2)^-1 mod n."""
    D = delta(parties)
    if math.gcd(4 * D * D, n) != 1:
        raise ValueError("threshold sharing: n shares a factor with 4 (parties!)^2")
    return pow(4 * D * D, -1, n)


def _chacha_block(key8, counter: int, nonce3):
    """RFC 8439 section 2.3."""
    M = 0xFFFFFFFF
    s = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574] + list(key8) + [counter & M] + list(nonce3)
    x = list(s)

    def qr(a, b, c, d):
        x[a] = (x[a] + x[b]) & M; x[d] ^= x[a]; x[d] = ((x[d] << 16) & M) | (x[d] >> 16)
        x[c] = (x[c] + x[d]) & M; x[b] ^= x[c]; x[b] = ((x[b] << 12) & M) | (x[b] >> 20)
        x[a] = (x[a] + x[b]) & M; x[d] ^= x[a]; x[d] = ((x[d] << 8) & M) | (x[d] >> 24)
        x[c] = (x[c] + x[d]) & M; x[b] ^= x[c]; x[b] = ((x[b] << 7) & M) | (x[b] >> 25)

    for _ in range(10):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
    return [(a + b) & M for a, b in zip(x, s)]


class SeededRng:
    """rng(bound) for deal() from a caller's seed: the ChaCha20 key stream (RFC 8439 block function, zero nonce) under the seed as
    a 256-bit key, rejection-sampled.  For reproducible tests: shares dealt from a known seed are not secret."""

    def __init__(self, seed: int):
        if not isinstance(seed, int) or seed < 0:
            raise ValueError("threshold sharing: the seed is a non-negative integer")
        self._key = struct.unpack("<8I", (seed % (1 << 256)).to_bytes(32, "little"))
        self._counter = 0
        self._buf = b""

    def _bytes(self, k: int) -> bytes:
        while len(self._buf) < k:
            self._buf += struct.pack("<16I", *_chacha_block(self._key, self._counter, (0, 0, 0)))
            self._counter += 1
        out, self._buf = self._buf[:k], self._buf[k:]
        return out

    def __call__(self, bound: int) -> int:
        bits = max(1, (bound - 1).bit_length())
        while True:
            v = int.from_bytes(self._bytes((bits + 7) // 8), "little") & ((1 << bits) - 1)
            if v < bound:
                return v


# ---- the classes ----------------------------------------------------------------------------------------------------------------------
def share_key(private_key, parties: int, threshold: int, *, seed: Optional[int] = None) -> List["PaillierKeyShare"]:
    """PaillierPrivateKey.share."""
    p, q = int(private_key.prikey._p), int(private_key.prikey._q)
    rng = secrets.randbelow if seed is None else SeededRng(seed)
    _, shares = deal(p, q, parties, threshold, rng)
    pub = private_key._public()
    return [PaillierKeyShare(pub, i + 1, parties, threshold, s) for i, s in enumerate(shares)]


class PaillierKeyShare:
    """Share s_i of a dealt key: partial_decrypt raises every ciphertext of a container to 2 Delta s_i.  The share is as secret as
    p and q are together with t - 1 others; repr and error messages show the index and the shape, never the share."""

    def __init__(self, public_key, index: int, parties: int, threshold: int, share: int):
        _check_shape(parties, threshold)
        if not 1 <= index <= parties:
            raise ValueError(f"PaillierKeyShare: index must lie in 1 .. {parties}")
        if share < 0:
            raise ValueError(f"PaillierKeyShare {index} of ({parties}, {threshold}): negative share")
        self.public_key = public_key
        self.index, self.parties, self.threshold = int(index), int(parties), int(threshold)
        self.__share = int(share)
        self._handle = None

    def __repr__(self):
        return f"<PaillierKeyShare {self.index} of ({self.parties}, {self.threshold}), {self.public_key.n.bit_length()}-bit key>"

    def __getstate__(self):
        return (self.public_key, self.index, self.parties, self.threshold, self.__share)

    def __setstate__(self, state):
        (self.public_key, self.index, self.parties, self.threshold, self.__share) = state
        self._handle = None

    def __eq__(self, other):
        return isinstance(other, PaillierKeyShare) and self.__getstate__()[1:] == other.__getstate__()[1:] and \
            self.public_key.n == other.public_key.n

    def __hash__(self):
        return hash(("PaillierKeyShare", self.public_key.n, self.index, self.parties, self.threshold))

    def exponent(self) -> int:
        """2 Delta s_i: the exponent of this shareholder's partial decryptions (secret)."""
        return 2 * delta(self.parties) * self.__share

    def _native(self):
        from . import engine

        pub = self.public_key.pubkey.handle
        if self._handle is None or self._handle.pub is not pub:
            self._handle = engine.KeyShareHandle(pub, self.exponent())
        return self._handle

    def partial_decrypt(self, x) -> "PaillierPartialDecryption":
        """c_i = c^(2 Delta s_i) mod n^2 for every ciphertext of a PaillierEncryptedNumber or a PaillierPackedNumber, on the key's
        home device (pai_partial_decrypt)."""
        from . import packed as _packed
        from .paillier import PaillierEncryptedNumber

        if isinstance(x, _packed.PaillierPackedNumber):
            expo, packing = None, (x.slot_bits, x.slots, x.exponent, x.value_bits)
        elif isinstance(x, PaillierEncryptedNumber):
            expo, packing = x._expo, None
        else:
            raise TypeError("PaillierKeyShare.partial_decrypt: expected a PaillierEncryptedNumber or a PaillierPackedNumber")
        if x.public_key.n != self.public_key.n:
            raise ValueError(f"PaillierKeyShare {self.index} of ({self.parties}, {self.threshold}): public key mismatch")
        h = self._native()
        words = x.ciphertext().words                         # a failed asynchronous inversion behind x is raised here
        words = words if words.device == h.pub.device else words.to(h.pub.device)
        return PaillierPartialDecryption(self.public_key, h.partial_decrypt(words.contiguous()), self.index, self.parties,
                                         self.threshold, expo, len(x), packing)


class PaillierPartialDecryption:
    """The partial decryptions c_i of one container by shareholder `index`: a limb matrix [rows, ct_words] on the key's home device
    (host words after unpickling), with the container's exponents, length and packing fields."""

    def __init__(self, public_key, words, index: int, parties: int, threshold: int, exponents, length: int, packing=None):
        self.public_key = public_key
        self._t = words
        self.index, self.parties, self.threshold = int(index), int(parties), int(threshold)
        self._expo = None if exponents is None else np.asarray(exponents, dtype=np.int32).reshape(-1).copy()
        self._length = int(length)
        self.packing = None if packing is None else tuple(int(v) for v in packing)     # (slot_bits, slots, exponent, value_bits)

    def __len__(self) -> int:
        return self._length

    @property
    def rows(self) -> int:
        return int(self._t.shape[0])

    def __repr__(self):
        return (f"<PaillierPartialDecryption by share {self.index} of ({self.parties}, {self.threshold}): {self._length} "
                f"{'packed ' if self.packing else ''}elements in {self.rows} rows>")

    def words(self, device):
        from . import engine

        if isinstance(self._t, np.ndarray):
            self._t = engine.to_device_words(self._t, device)
        return self._t if self._t.device == device else self._t.to(device)

    def host_words(self) -> np.ndarray:
        from . import engine

        return self._t if isinstance(self._t, np.ndarray) else engine.to_host_words(self._t)

    def __getstate__(self):
        return (self.public_key, self.index, self.parties, self.threshold, None if self._expo is None else [int(e) for e in self._expo],
                self._length, self.packing, np.ascontiguousarray(self.host_words()))

    def __setstate__(self, state):
        (self.public_key, self.index, self.parties, self.threshold, expo, self._length, self.packing, self._t) = state
        self._expo = None if expo is None else np.asarray(expo, dtype=np.int32).reshape(-1).copy()


def select_parts(public_key, parts, packed: bool) -> list:
    """Validates a set of partial decryptions for `public_key` and returns the `threshold` parts with the smallest indices.
    ValueError — before anything is launched — for fewer than threshold parts, duplicate or out-of-range indices, and mixed
    parties, thresholds, lengths, containers or keys."""
    parts = list(parts)
    if not parts or not all(isinstance(p, PaillierPartialDecryption) for p in parts):
        raise ValueError("combine: expected a non-empty sequence of PaillierPartialDecryption")
    a = parts[0]
    _check_shape(a.parties, a.threshold)
    for p in parts:
        if p.public_key.n != public_key.n:
            raise ValueError("combine: a partial decryption belongs to another key")
        if (p.parties, p.threshold) != (a.parties, a.threshold):
            raise ValueError("combine: partial decryptions of different (parties, threshold)")
        if len(p) != len(a) or p.rows != a.rows or p.packing != a.packing or \
                (p._expo is None) != (a._expo is None) or (p._expo is not None and not np.array_equal(p._expo, a._expo)):
            raise ValueError("combine: partial decryptions of different containers")
        if not 1 <= p.index <= p.parties:
            raise ValueError(f"combine: index {p.index} outside 1 .. {p.parties}")
    if (a.packing is not None) != packed:
        raise ValueError("combine: these are partial decryptions of a packed container: combine_packed" if a.packing is not None
                         else "combine_packed: these are not partial decryptions of a packed container")
    idx = [p.index for p in parts]
    if len(set(idx)) != len(idx):
        raise ValueError(f"combine: duplicate indices in {sorted(idx)}")
    if len(parts) < a.threshold:
        raise ValueError(f"combine: {len(parts)} partial decryptions, the threshold is {a.threshold}")
    return sorted(parts, key=lambda p: p.index)[:a.threshold]


def combine_words(public_key, parts, packed: bool = False):
    """The residues m_i [rows, n_words] on the key's home device (pai_threshold_combine).  ValueError when rows fail the
    consistency test c' = 1 (mod n) or a negative-side product is no unit."""
    use = select_parts(public_key, parts, packed)
    a = use[0]
    h = public_key.pubkey.handle
    mags, negs = lagrange([p.index for p in use], a.parties)
    coeff = [2 * m for m in mags]
    if any(c.bit_length() > MU_BITS_MAX or c == 0 for c in coeff):
        raise AssertionError("Lagrange coefficient outside the bound 2^66")
    m, flag, rowflag = h.threshold_combine([p.words(h.device) for p in use], coeff, negs, theta(public_key.n, a.parties))
    f = int(flag.item())                                     # one synchronisation: the outcome of the whole call
    if f:
        bad = np.flatnonzero(rowflag.cpu().numpy())
        what = []
        if f & 2:
            what.append("a product of the negative side is not invertible modulo n^2")
        if f & 1:
            what.append(f"{bad.size} of {a.rows} rows fail the consistency test (the first: row {int(bad[0]) if bad.size else -1})")
        raise ValueError("combine: inconsistent partial decryptions by shares " + str([p.index for p in use]) + ": " + "; ".join(what))
    return m
