"""Threshold decryption (extension; no reference counterpart): t of l parties decrypt together, nobody holds p and q afterwards.

The scheme is Damgard-Jurik / Fouque-Poupard-Stern at s = 1 with a trusted dealer.  Without proofs it serves honest-but-curious
parties: a shareholder who sends a wrong partial decryption is detected only in so far as the combined value fails the test
c' = 1 (mod n) — it is not identified, and a wrong value that passes the test is accepted.  Shares dealt with verifiable=True carry
a verification key, and partial_decrypt(x, prove=True) attaches ONE proof of correct exponentiation per container (below).

  dealer     lambda = lcm(p - 1, q - 1), gcd(n, lambda) = 1 required; d = 0 (mod lambda), d = 1 (mod n), 0 <= d < n lambda;
             f(X) = d + a_1 X + ... + a_(t-1) X^(t-1), a_k uniform in [0, n lambda); s_i = f(i) mod n lambda for i = 1 .. l
  partial    c_i = c^(2 Delta s_i) mod n^2, Delta = l!  (the exponent is not reduced: the shareholder does not know n lambda)
  combine    mu_i = Delta prod_(j in S, j != i) j / (j - i) (an integer);  c' = prod c_i^(2 mu_i) = c^(4 Delta^2 d)
             = 1 + (4 Delta^2 m mod n) n;  m = ((c' - 1) / n) theta mod n with theta = (4 Delta^2)^-1 mod n.
             Negative mu_i go on a second product: c' = P+ (P-)^-1 — one batch inversion per combine.

1 <= t <= l <= 16 (a condition of the combine's n-ary product, and Delta stays below 2^45).  The integer helpers deal / lagrange /
theta need no GPU; the classes run on the key's home device (pai_partial_decrypt, pai_threshold_combine).

Proofs of correct partial decryption.  lambda = 128 throughout; x_i = Delta s_i; W = ct_words; a residue's bytes
are its W (modulo n^2) or n_words (n) little-endian wire words.

  dealer     v = u^2 mod n^2 for a uniform unit u (drawn after the polynomial), v_i = v^(x_i) mod n^2
  leaves     leaf_j = SHA-256(c_j || c_(i,j))                                                       (device: pai_sha256_rows)
  root       SHA-256("pai-tdec-v1" || LE32(key_bits) || n || LE32(l) || LE32(t) || LE32(i) || v || v_i || LE64(N) || leaf_0 || ..)
  rho_j      the first 16 bytes of SHA-256(root || "pai-rho" || LE64(j)), little-endian             (device: pai_sha256_expand)
  fold       C = prod c_j^(rho_j), P = prod c_(i,j)^(rho_j) mod n^2                                 (pai_ct_sparse_multiexp, twice)
  prove      r < 2^B, B = 2 bitlen(n) + bitlen(Delta) + 256;  a = C^(4 r), b = v^r;  e = the first 16 bytes of
             SHA-256(root || "pai-chal" || C || P || a || b);  z = r + e x_i over the integers;  the proof is (a, b, z)
  verify     a, b in [1, n^2), z < 2^(B+1), C^(4 z) = a P^(2 e) and v^z = b v_i^e (mod n^2); every row of the part below n^2

An accepted proof certifies c_(i,j)^2 = c_j^(4 x_i) for every row — the squares are all that combine uses: a part with a row
replaced by n^2 - c_(i,j) is accepted and combines to the same plaintext.  The soundness error is about 2^-127 when (p - 1) / 2 and
(q - 1) / 2 are prime (`safe_primes`, the setting of the published proofs); for other keys a cheating prover succeeds with
probability at most 1 / ell for the smallest odd prime ell dividing lcm(p - 1, q - 1) (`small_order_factor` shows it when
ell < 2^20).  This package's key generator does NOT make safe primes.  The dealer is trusted for v and the v_i.  The integer
functions below (verification_values .. verify_int) are the one definition of the byte layout and the oracle of the device path."""
from __future__ import annotations

import hashlib
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


# ---- proofs of correct partial decryption: integers and hashlib only ----------------------------------------------------------------
PROOF_BITS = 128                     # lambda: bits of the fold's coefficients rho_j and of the challenge e
ROOT_TAG, RHO_TAG, CHAL_TAG = b"pai-tdec-v1", b"pai-rho", b"pai-chal"
SMALL_ORDER_LIMIT = 1 << 20


def _le(v: int, nbytes: int) -> bytes:
    return int(v).to_bytes(nbytes, "little")


def key_words(key_bits: int) -> Tuple[int, int]:
    """(n_words, ct_words) of a key of key_bits bits."""
    nw = (int(key_bits) + 31) // 32
    return nw, 2 * nw


def nonce_bits(n: int, parties: int) -> int:
    """B: the prover's nonce r is uniform below 2^B — 256 bits above e x_i, so that z = r + e x_i hides x_i statistically."""
    return 2 * n.bit_length() + delta(parties).bit_length() + 256


def is_probable_prime(m: int, rounds: int = 40) -> bool:
    """Miller-Rabin with the first `rounds` primes as bases (deterministic below 3.3 10^24, error below 4^-rounds above)."""
    if m < 2:
        return False
    small = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97, 101, 103, 107, 109, 113,
             127, 131, 137, 139, 149, 151, 157, 163, 167, 173)
    for q in small:
        if m % q == 0:
            return m == q
    d, s = m - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    for a in small[:rounds]:
        x = pow(a, d, m)
        if x in (1, m - 1):
            continue
        for _ in range(s - 1):
            x = x * x % m
            if x == m - 1:
                break
        else:
            return False
    return True


def safe_primes(p: int, q: int) -> bool:
    """(p - 1) / 2 and (q - 1) / 2 are both prime."""
    return p % 2 == 1 and q % 2 == 1 and is_probable_prime((p - 1) // 2) and is_probable_prime((q - 1) // 2)


_ODD_PRIMES: List[int] = []


def small_order_factor(p: int, q: int) -> int:
    """The smallest odd prime below 2^20 that divides (p - 1)(q - 1), or 0: a cheating prover's chance is bounded by its inverse."""
    if not _ODD_PRIMES:
        sieve = bytearray([1]) * SMALL_ORDER_LIMIT
        sieve[0:2] = b"\x00\x00"
        for i in range(2, int(SMALL_ORDER_LIMIT ** 0.5) + 1):
            if sieve[i]:
                sieve[i * i::i] = bytearray(len(range(i * i, SMALL_ORDER_LIMIT, i)))
        _ODD_PRIMES.extend(i for i in range(3, SMALL_ORDER_LIMIT) if sieve[i])
    m = (p - 1) * (q - 1)
    for ell in _ODD_PRIMES:
        if m % ell == 0:
            return ell
    return 0


def draw_base(n: int, rng: Callable[[int], int]) -> int:
    """v = u^2 mod n^2 for a uniform unit u."""
    nsq = n * n
    while True:
        u = rng(nsq)
        if u and math.gcd(u, n) == 1:
            return u * u % nsq


def verification_values(n: int, parties: int, shares: Sequence[int], v: int, modexp=pow) -> List[int]:
    """[v_1 .. v_l], v_i = v^(Delta s_i) mod n^2.  modexp(base, exponent, modulus): pow, or _native.host_modexp at real key sizes."""
    D, nsq = delta(parties), n * n
    return [modexp(v, D * int(s), nsq) for s in shares]


def deal_verifiable(p: int, q: int, parties: int, threshold: int, rng: Callable[[int], int], modexp=pow):
    """(d, shares, v, [v_1 .. v_l]): deal(), then the base — drawn AFTER the polynomial, so a seed gives the shares it gives deal()."""
    d, shares = deal(p, q, parties, threshold, rng)
    v = draw_base(p * q, rng)
    return d, shares, v, verification_values(p * q, parties, shares, v, modexp)


def transcript_leaves(cts: Sequence[int], parts: Sequence[int], key_bits: int) -> bytes:
    """leaf_0 || leaf_1 || ..: leaf_j = SHA-256(bytes of c_j || bytes of c_(i,j))."""
    W = key_words(key_bits)[1]
    if len(cts) != len(parts):
        raise ValueError("transcript: one partial decryption per ciphertext")
    return b"".join(hashlib.sha256(_le(c, 4 * W) + _le(ci, 4 * W)).digest() for c, ci in zip(cts, parts))


def transcript_root(n: int, key_bits: int, parties: int, threshold: int, index: int, v: int, v_i: int, leaves: bytes) -> bytes:
    nw, W = key_words(key_bits)
    if len(leaves) % 32:
        raise ValueError("transcript: the leaves are 32 bytes each")
    h = hashlib.sha256(ROOT_TAG + _le(key_bits, 4) + _le(n, 4 * nw) + _le(parties, 4) + _le(threshold, 4) + _le(index, 4) + _le(v, 4 * W)
                       + _le(v_i, 4 * W) + _le(len(leaves) // 32, 8))
    h.update(leaves)
    return h.digest()


def rho(root: bytes, count: int, first: int = 0) -> List[int]:
    """[rho_first .. rho_(first + count - 1)]."""
    return [int.from_bytes(hashlib.sha256(root + RHO_TAG + _le(j, 8)).digest()[:PROOF_BITS // 8], "little") for j in range(first, first + count)]


def challenge(root: bytes, key_bits: int, C: int, P: int, a: int, b: int) -> int:
    W = key_words(key_bits)[1]
    return int.from_bytes(hashlib.sha256(root + CHAL_TAG + b"".join(_le(x, 4 * W) for x in (C, P, a, b))).digest()[:PROOF_BITS // 8], "little")


def _multiexp(bases: Sequence[int], exps: Sequence[int], mod: int) -> int:
    """prod bases[j]^(exps[j]) mod `mod` on one chain of squarings (most significant bit first)."""
    acc = 1
    for bit in range(max((e.bit_length() for e in exps), default=0) - 1, -1, -1):
        acc = acc * acc % mod
        for b, e in zip(bases, exps):
            if (e >> bit) & 1:
                acc = acc * b % mod
    return acc


def _fold_int(n: int, key_bits: int, parties: int, threshold: int, index: int, v: int, v_i: int, cts, parts):
    nsq = n * n
    root = transcript_root(n, key_bits, parties, threshold, index, v, v_i, transcript_leaves(cts, parts, key_bits))
    coeff = rho(root, len(cts))
    return root, _multiexp([int(c) % nsq for c in cts], coeff, nsq), _multiexp([int(c) % nsq for c in parts], coeff, nsq)


def _check_cts(cts, nsq: int) -> None:
    if any(not 0 <= int(c) < nsq for c in cts):
        raise ValueError("partial decryption proof: a ciphertext is not a residue modulo n^2")


def prove_int(n: int, key_bits: int, parties: int, threshold: int, index: int, share: int, v: int, v_i: int, cts: Sequence[int],
              parts: Sequence[int], nonce: int) -> Tuple[int, int, int]:
    """(a, b, z) for the partial decryptions `parts` of `cts` under x_i = Delta share and the nonce r = `nonce` < 2^B (uniform and
    used ONCE: two proofs under one nonce reveal the share)."""
    nsq = n * n
    _check_cts(cts, nsq)
    if not 0 <= nonce < (1 << nonce_bits(n, parties)):
        raise ValueError("partial decryption proof: the nonce must lie in [0, 2^B)")
    root, C, P = _fold_int(n, key_bits, parties, threshold, index, v, v_i, cts, parts)
    a, b = pow(C, 4 * nonce, nsq), pow(v, nonce, nsq)
    e = challenge(root, key_bits, C, P, a, b)
    return a, b, nonce + e * delta(parties) * share


def verify_int(n: int, key_bits: int, parties: int, threshold: int, index: int, v: int, v_i: int, cts: Sequence[int], parts: Sequence[int],
               proof) -> bool:
    """The verifier.  ValueError for a ciphertext outside [0, n^2); False for everything wrong with the part or the proof."""
    nsq = n * n
    _check_cts(cts, nsq)
    if proof is None or len(parts) != len(cts) or any(not 0 <= int(c) < nsq for c in parts):
        return False
    a, b, z = (int(x) for x in proof)
    if not (1 <= a < nsq and 1 <= b < nsq and 0 <= z < (1 << (nonce_bits(n, parties) + 1))):
        return False
    root, C, P = _fold_int(n, key_bits, parties, threshold, index, v, v_i, cts, parts)
    e = challenge(root, key_bits, C, P, a, b)
    return pow(C, 4 * z, nsq) == a * pow(P, 2 * e, nsq) % nsq and pow(v, z, nsq) == b * pow(v_i, e, nsq) % nsq


# ---- the classes ----------------------------------------------------------------------------------------------------------------------
def _host_modexp(base: int, exponent: int, modulus: int) -> int:
    """pai_host_modexp where it serves the modulus (a CPython pow with a 4096-bit exponent costs 0.2 s at 2048-bit keys), else pow."""
    from . import _native

    if modulus % 2 and (modulus.bit_length() + 31) // 32 <= _native.HOST_MODEXP_MAX_WORDS:
        return _native.host_modexp(base, exponent, modulus)
    return pow(base, exponent, modulus)


def share_key(private_key, parties: int, threshold: int, *, seed: Optional[int] = None, verifiable: bool = False) -> List["PaillierKeyShare"]:
    """PaillierPrivateKey.share."""
    p, q = int(private_key.prikey._p), int(private_key.prikey._q)
    rng = secrets.randbelow if seed is None else SeededRng(seed)
    pub = private_key._public()
    if not verifiable:
        _, shares = deal(p, q, parties, threshold, rng)
        return [PaillierKeyShare(pub, i + 1, parties, threshold, s) for i, s in enumerate(shares)]
    _, shares, v, values = deal_verifiable(p, q, parties, threshold, rng, _host_modexp)
    vk = PaillierVerificationKey(p * q, parties, threshold, v, values, safe_primes(p, q), small_order_factor(p, q))
    return [PaillierKeyShare(pub, i + 1, parties, threshold, s, vk) for i, s in enumerate(shares)]


class PaillierVerificationKey:
    """The public verification values of a dealing: v = u^2 and v_i = v^(Delta s_i) mod n^2, with what the dealer saw of the
    primes — `safe_primes` ((p - 1) / 2 and (q - 1) / 2 both prime: the proofs' error is about 2^-127) and `small_order_factor`
    (the smallest odd prime ell < 2^20 dividing (p - 1)(q - 1), or 0: a cheating prover's chance is at most 1 / ell).  The dealer is
    trusted for all of it.  Public; pickles."""

    def __init__(self, n: int, parties: int, threshold: int, v: int, values: Sequence[int], safe_primes: bool = False,
                 small_order_factor: int = 0):
        _check_shape(parties, threshold)
        nsq = int(n) * int(n)
        values = tuple(int(x) for x in values)
        if len(values) != parties or not all(0 < x < nsq for x in (int(v),) + values):
            raise ValueError("PaillierVerificationKey: one residue modulo n^2 per party, and the base")
        self.n, self.parties, self.threshold, self.v, self.values = int(n), int(parties), int(threshold), int(v), values
        self.safe_primes, self.small_order_factor = bool(safe_primes), int(small_order_factor)

    def _state(self):
        return (self.n, self.parties, self.threshold, self.v, self.values, self.safe_primes, self.small_order_factor)

    def __eq__(self, other):
        return isinstance(other, PaillierVerificationKey) and self._state() == other._state()

    def __hash__(self):
        return hash(("PaillierVerificationKey", self.n, self.parties, self.threshold, self.v))

    def __repr__(self):
        return (f"<PaillierVerificationKey of ({self.parties}, {self.threshold}), {self.n.bit_length()}-bit key, "
                f"safe_primes={self.safe_primes}, small_order_factor={self.small_order_factor}>")


class PaillierDecryptionProof:
    """(a, b, z): one proof that every row of a partial decryption is the ciphertext's row to the share's exponent, up to sign."""

    def __init__(self, a: int, b: int, z: int):
        self.a, self.b, self.z = int(a), int(b), int(z)

    def __iter__(self):
        return iter((self.a, self.b, self.z))

    def __eq__(self, other):
        return isinstance(other, PaillierDecryptionProof) and tuple(self) == tuple(other)

    def __hash__(self):
        return hash(("PaillierDecryptionProof",) + tuple(self))

    def __repr__(self):
        return f"<PaillierDecryptionProof, z of {self.z.bit_length()} bits>"


class PaillierKeyShare:
    """Share s_i of a dealt key: partial_decrypt raises every ciphertext of a container to 2 Delta s_i.  The share is as secret as
    p and q are together with t - 1 others; repr and error messages show the index and the shape, never the share."""

    def __init__(self, public_key, index: int, parties: int, threshold: int, share: int, verification_key=None):
        _check_shape(parties, threshold)
        if not 1 <= index <= parties:
            raise ValueError(f"PaillierKeyShare: index must lie in 1 .. {parties}")
        if share < 0:
            raise ValueError(f"PaillierKeyShare {index} of ({parties}, {threshold}): negative share")
        self.public_key = public_key
        self.index, self.parties, self.threshold = int(index), int(parties), int(threshold)
        self.__share = int(share)
        if verification_key is not None and (verification_key.n, verification_key.parties, verification_key.threshold) != \
                (public_key.n, self.parties, self.threshold):
            raise ValueError(f"PaillierKeyShare {index} of ({parties}, {threshold}): the verification key belongs to another dealing")
        self.verification_key = verification_key                # None for shares dealt without verifiable=True
        self._handle = None

    def __repr__(self):
        return f"<PaillierKeyShare {self.index} of ({self.parties}, {self.threshold}), {self.public_key.n.bit_length()}-bit key>"

    def __getstate__(self):                                      # the verification key is appended only when there is one
        st = (self.public_key, self.index, self.parties, self.threshold, self.__share)
        return st if self.verification_key is None else st + (self.verification_key,)

    def __setstate__(self, state):
        (self.public_key, self.index, self.parties, self.threshold, self.__share) = state[:5]
        self.verification_key = state[5] if len(state) > 5 else None
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

    def partial_decrypt(self, x, prove: bool = False, *, _nonce: Optional[int] = None) -> "PaillierPartialDecryption":
        """c_i = c^(2 Delta s_i) mod n^2 for every ciphertext of a PaillierEncryptedNumber or a PaillierPackedNumber, on the key's
        home device (pai_partial_decrypt).  prove=True (the share needs a verification key: share(.., verifiable=True)) sets
        part.proof, ONE PaillierDecryptionProof for the container, checked by PaillierPublicKey.verify_partial: it certifies
        c_(i,j)^2 = c_j^(4 Delta s_i) for every row — what combine uses; ValueError when a ciphertext row is not below n^2.
        _nonce: the prover's nonce r < 2^B, for tests only — a nonce used for two proofs reveals the share."""
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
        if prove and self.verification_key is None:
            raise ValueError(f"PaillierKeyShare {self.index} of ({self.parties}, {self.threshold}): dealt without verifiable=True, "
                             "there is nothing to prove against")
        words = words.contiguous()
        if prove:
            _require_residues(self.public_key, h.pub, words)
        part = PaillierPartialDecryption(self.public_key, h.partial_decrypt(words), self.index, self.parties, self.threshold, expo,
                                         len(x), packing)
        if prove:
            part.proof = _prove_device(h.pub, self.verification_key, self.index, self.__share, words, part.words(h.pub.device), _nonce)
        return part


class PaillierPartialDecryption:
    """The partial decryptions c_i of one container by shareholder `index`: a limb matrix [rows, ct_words] on the key's home device
    (host words after unpickling), with the container's exponents, length and packing fields."""

    def __init__(self, public_key, words, index: int, parties: int, threshold: int, exponents, length: int, packing=None, proof=None):
        self.public_key = public_key
        self.proof = proof                                       # a PaillierDecryptionProof, or None
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

    def __getstate__(self):                                      # the proof is appended only when there is one
        st = (self.public_key, self.index, self.parties, self.threshold, None if self._expo is None else [int(e) for e in self._expo],
              self._length, self.packing, np.ascontiguousarray(self.host_words()))
        return st if self.proof is None else st + (self.proof,)

    def __setstate__(self, state):
        (self.public_key, self.index, self.parties, self.threshold, expo, self._length, self.packing, self._t) = state[:8]
        self.proof = state[8] if len(state) > 8 else None
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


# ---- proofs of correct partial decryption on the device -----------------------------------------------------------------------------------
def _rows_above(pub, words, bound: int):
    """Device bool [rows]: the row is >= bound (a modulus of ct_words words)."""
    import torch

    from . import bindings as _bindings
    from . import engine

    b = torch.from_numpy(engine.int_to_words(bound, words.shape[1]).astype(np.int64)).to(words.device)
    return _bindings._rows_not_in_1_n(words, b) & (words != 0).any(dim=1)


def _require_residues(public_key, pub, words) -> None:
    if words.shape[0] and bool(_rows_above(pub, words, public_key.n * public_key.n).any()):
        raise ValueError("partial decryption proof: a ciphertext row is not a residue modulo n^2")


def _fold_device(pub, vk, index: int, ct, part):
    """(root, C, P, their device rows [2, W]) of the transcript of (ct, part): leaves and coefficients by pai_sha256_rows /
    pai_sha256_expand, the two folds by pai_ct_sparse_multiexp with the identity term list and one segment."""
    import torch

    from . import engine

    rows = int(ct.shape[0])
    leaves = engine.to_host_words(pub.sha256_rows([ct, part])).tobytes() if rows else b""
    root = transcript_root(vk.n, pub.key_bits, vk.parties, vk.threshold, index, vk.v, vk.values[index - 1], leaves)
    if rows == 0:
        one = engine.to_device_words(engine.ints_to_words([1, 1], pub.ct_words), pub.device)
        return root, 1, 1, one
    coeff = pub.sha256_expand(root, RHO_TAG, 0, rows, PROOF_BITS)
    base = torch.arange(rows, dtype=torch.int32, device=pub.device)
    off = torch.tensor([0, rows], dtype=torch.int64, device=pub.device)
    CP = torch.cat([pub.ct_sparse_multiexp(t, None, base, coeff, PROOF_BITS, None, off) for t in (ct, part)]).contiguous()
    C, P = engine.words_to_ints(engine.to_host_words(CP))
    return root, C, P, CP


def _pow_rows(pub, rows_t, exponents):
    """rows_t[k]^(exponents[k]) mod n^2 for a handful of rows with long exponents of their own: one pai_ct_mul.  Returns the device
    rows; the device copy of the exponents is zeroed behind the call."""
    from . import engine

    bits = max(1, max(int(e).bit_length() for e in exponents))
    ew = (bits + 31) // 32
    e_t = engine.to_device_words(engine.ints_to_words([int(e) for e in exponents], ew), pub.device)
    out = pub.ct_mul(rows_t.contiguous(), e_t, bits)
    e_t.zero_()
    return out


def _prove_device(pub, vk, index: int, share: int, ct, part, nonce: Optional[int]):
    from . import engine

    B = nonce_bits(vk.n, vk.parties)
    r = secrets.randbits(B) if nonce is None else int(nonce)
    if not 0 <= r < (1 << B):
        raise ValueError("partial decryption proof: the nonce must lie in [0, 2^B)")
    root, C, P, CP = _fold_device(pub, vk, index, ct, part)
    bases = engine.to_device_words(engine.ints_to_words([C, vk.v], pub.ct_words), pub.device)
    a, b = engine.words_to_ints(engine.to_host_words(_pow_rows(pub, bases, [4 * r, r])))
    e = challenge(root, pub.key_bits, C, P, a, b)
    return PaillierDecryptionProof(a, b, r + e * delta(vk.parties) * share)


def verify_part(public_key, x, part, vk) -> bool:
    """PaillierPublicKey.verify_partial."""
    import torch

    from . import engine
    from . import packed as _packed
    from .paillier import PaillierEncryptedNumber

    if isinstance(x, _packed.PaillierPackedNumber):
        expo, packing = None, (x.slot_bits, x.slots, x.exponent, x.value_bits)
    elif isinstance(x, PaillierEncryptedNumber):
        expo, packing = np.asarray(x._expo, dtype=np.int32).reshape(-1), None
    else:
        raise TypeError("verify_partial: expected a PaillierEncryptedNumber or a PaillierPackedNumber")
    if x.public_key.n != public_key.n:
        raise ValueError("verify_partial: the container belongs to another key")
    pub = public_key.pubkey.handle
    ct = x.ciphertext().words
    ct = (ct if ct.device == pub.device else ct.to(pub.device)).contiguous()
    _require_residues(public_key, pub, ct)
    if not (isinstance(part, PaillierPartialDecryption) and isinstance(vk, PaillierVerificationKey)):
        return False
    proof = part.proof
    if not isinstance(proof, PaillierDecryptionProof):
        return False
    if part.public_key.n != public_key.n or vk.n != public_key.n or (part.parties, part.threshold) != (vk.parties, vk.threshold) or \
            not 1 <= part.index <= vk.parties:
        return False
    if part.rows != ct.shape[0] or len(part) != len(x) or part.packing != packing or (part._expo is None) != (expo is None) or \
            (expo is not None and not np.array_equal(part._expo, expo)):
        return False
    nsq = public_key.n * public_key.n
    a, b, z = proof.a, proof.b, proof.z
    if not (1 <= a < nsq and 1 <= b < nsq and 0 <= z < (1 << (nonce_bits(vk.n, vk.parties) + 1))):
        return False
    pw = part.words(pub.device).contiguous()
    if pw.shape[0] and bool(_rows_above(pub, pw, nsq).any()):     # before any fold: the kernels take residues
        return False
    root, C, P, CP = _fold_device(pub, vk, part.index, ct, pw)
    e = challenge(root, pub.key_bits, C, P, a, b)
    v_i = vk.values[part.index - 1]
    lhs = _pow_rows(pub, engine.to_device_words(engine.ints_to_words([C, vk.v], pub.ct_words), pub.device), [4 * z, z])
    if e:
        pe = _pow_rows(pub, engine.to_device_words(engine.ints_to_words([P, v_i], pub.ct_words), pub.device), [2 * e, e])
    else:
        pe = engine.to_device_words(engine.ints_to_words([1, 1], pub.ct_words), pub.device)
    rhs = pub.ct_add(engine.to_device_words(engine.ints_to_words([a, b], pub.ct_words), pub.device), pe)
    return bool(torch.equal(lhs, rhs))


def verified_parts(public_key, x, parts, vk):
    """PaillierPublicKey.verified_parts."""
    good, rejected = [], []
    for p in parts:
        if verify_part(public_key, x, p, vk):
            good.append(p)
        else:
            rejected.append(getattr(p, "index", None))
    return good, rejected
