/* paillier_hip.h — C ABI of libpaillier_hip.so, the MI355X (gfx950) Paillier engine.
 *
 * This library is the drop-in replacement for the native layer under the reference's Python API:
 * the pybind11 module `ipcl_bindings` (src/ipcl_python/bindings/ipcl_bindings.cpp:21-63) plus the
 * un-vendored ipcl / IPP-Crypto libraries it forwards to.  Each entry point cites the reference
 * interface it replaces.  Conventions:
 *
 *  - every function returns 0 on success, a negative PAI_E_* code on failure; pai_last_error()
 *    returns a thread-local message for the last failure (C++ exceptions never cross the ABI);
 *  - big integers are little-endian arrays of native-endian uint32_t words (the wire order of
 *    pyByte2BN / BN2bytes, ipcl_bindings.cpp:100-138), batches are row-major [N][words];
 *  - pointers named d_* are DEVICE pointers on the key's device; h_* are HOST pointers;
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream); calls are asynchronous
 *    with respect to the host unless stated otherwise;
 *  - a key handle owns device scratch (window tables, quotient-digit columns) that its operations reuse.  The
 *    library orders the users of that scratch itself: operations of one handle issued on the SAME stream are
 *    ordered by the stream, operations issued on DIFFERENT streams are chained with an event (the later call makes
 *    its stream wait for the earlier one), so any mix of threads and streams on one handle is safe, and handles
 *    of the same key material on different devices are independent.  Only pai_ct_invert (it reports
 *    non-invertible inputs; pai_ct_invert_async + pai_pubkey_status is the asynchronous form), pai_pubkey_status,
 *    pai_pubkey_trim and pai_ct_pow2 without a hint return after their stream work has completed; everything else,
 *    pai_decrypt and pai_modexp_fixed (its host exponent is copied to pinned staging) included, is asynchronous.  The library keeps HIP
 *    events beyond a call — one per handle that orders its scratch, one per slot of the calling thread's host staging ring — and waits
 *    for them in later calls, possibly after the caller has destroyed the stream they were last recorded on.  What is established about
 *    that: with the staging ring's events last recorded on destroyed streams, hipEventSynchronize has failed in the ring with
 *    hipErrorCapturedEvent although nothing captures.  Until that is settled, keep a stream alive while handles (and, for host staging,
 *    the thread) that were used with it live on; tests/test_gpu_stream_contract.py, which holds this contract on non-blocking streams,
 *    keeps its streams for the life of the process for that reason;
 *  - memory contract (held by tests/test_gpu_memory_contract.py).  Alignment: a device pointer needs the alignment of its C
 *    type and no more — 4 bytes for uint32_t / int32_t rows, 8 for double / int64_t / uint64_t, 1 for uint8_t; row r of a batch
 *    is a valid operand whatever the row length (rows of 34 or 102 words are not 16-byte multiples).  Kernels that move rows as
 *    16-byte vectors test the address at run time and fall back to word accesses.  Extent: a call reads its operands, writes the
 *    outputs it documents — N rows, ceil(N / k) rows, S rows, one flag word — and nothing else: no word before or behind an
 *    output, no word of an input, whatever lies next to them.  Aliasing: an output may be EXACTLY an operand (same address, same
 *    extent) where the call says so.  The calls that state an aliasing rule below (pai_ct_add, pai_ct_mont_mul, pai_ct_add_aligned*,
 *    pai_ct_addn, pai_ct_add_plain, pai_ct_mul*, pai_ct_invert*, pai_ct_scan, pai_ct_pack*, pai_buf_slice, pai_buf_rotate,
 *    pai_modmul, pai_partial_decrypt, pai_threshold_combine, pai_sha256_rows) answer any other overlap of the output's byte range with the named operand's byte range with PAI_E_INVALID and
 *    launch nothing; in every other call, and for the small operands of these (shifts, entry constants), an output that overlaps
 *    an operand is undefined.  In particular a broadcast row (b_bcast != 0) may be the output only when N == 1: with N > 1 other
 *    waves still load it while output row 0 is stored;
 *  - a call never changes the calling thread's current HIP device (it is restored on return);
 *  - there is NO CPU fallback: without a usable gfx950 device key creation fails with
 *    PAI_E_NODEVICE.
 *
 * Word counts for a key of `key_bits` bits: n_words = ceil(key_bits/32) (plaintext residues mod n),
 * ct_words = 2*n_words (ciphertexts mod n^2), r_words = ceil(randbits/32) (DJN randomness).
 */
#ifndef PAILLIER_HIP_H_
#define PAILLIER_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PAI_OK 0
#define PAI_E_INVALID (-1)    /* bad argument */
#define PAI_E_NODEVICE (-2)   /* no gfx950 device / HIP runtime failure at set-up */
#define PAI_E_HIP (-3)        /* HIP runtime error during a call */
#define PAI_E_UNSUPPORTED (-4)/* key size outside the compiled geometries (moduli up to 8192 bits) */
#define PAI_E_INTERNAL (-5)

typedef struct pai_pubkey pai_pubkey;      /* replaces ipclPublicKey  (ipcl_bindings_classes.cpp:12-91)  */
typedef struct pai_privkey pai_privkey;    /* replaces ipclPrivateKey (ipcl_bindings_classes.cpp:93-163) */
typedef struct pai_modulus pai_modulus;    /* a bare odd modulus for pai_modmul / pai_modexp_*           */

/* ---- library ---------------------------------------------------------------------------------- */
int pai_version(void);                                   /* 100*major + minor */
int pai_device_count(int* count);                        /* number of visible HIP devices */
const char* pai_last_error(void);

/* Per-kernel timing (HIP events on the caller's stream).  While enabled, pai_encrypt / pai_decrypt
 * become synchronous and record the duration of each kernel they launch; pai_profile_last(i, ...)
 * returns entry i of the calling thread's last call (PAI_E_INVALID past the end). */
int pai_profile_enable(int on);
int pai_profile_last(int index, char* name_out, size_t name_cap, float* ms_out);
/* The kernel family behind entry i where one name covers several ("pp", "rl", "window", "pair4", "padic", "padic_kara_mul", "pair",
 * "wide", "lane_group", "lat", ...; "" where the name says it all): what a test asserts after forcing a path with PAI_TUNE / PAI_DISABLE. */
int pai_profile_last_path(int index, char* path_out, size_t path_cap);
/* The kernel within that family where several share one path name: "kmrb", "kmrb2s", "kmr" or "km" for the register-resident 36-limb
 * decrypt kernels behind "padic_kara_mul" (balanced digits with one stored sum per column, the default / with two / Karatsuba
 * quotient products on unsigned limbs / schoolbook ones), "" elsewhere. */
int pai_profile_last_mode(int index, char* mode_out, size_t mode_cap);

/* ---- device memory helpers (for callers that do not bring their own allocator) ---------------- */
int pai_malloc(int device, size_t bytes, void** d_ptr);
int pai_free(int device, void* d_ptr);
int pai_memcpy_h2d(int device, void* d_dst, const void* h_src, size_t bytes, void* stream);
int pai_memcpy_d2h(int device, void* h_dst, const void* d_src, size_t bytes, void* stream);
int pai_stream_sync(int device, void* stream);

/* Small host operands of asynchronous calls without a copy on the stream (round 6).  The reference's pybind layer takes host
 * vectors by value (bindings/ipcl_bindings_classes.cpp:318-325: the exponents of CipherText * PlainText, the shifts the
 * Python layer computes for ipcl_python.py:570-741); at its own benchmark sizes (16 / 64 elements, bench/bench_ipcl_python.py:
 * 22-78) an H2D copy per operand costs as much as the kernel.  pai_host_stage copies `parts` host arrays (together at most
 * PAI_HOST_STAGE_MAX bytes, each part 16-byte aligned) into one slot of a pinned, device-mapped ring of the calling thread
 * and returns, per part, a pointer a kernel may READ through directly.  Contract: the pointers may be passed as read-only
 * device operands (exponents, shifts, codec inputs) of calls enqueued on `stream` BEFORE the calling thread's next
 * pai_host_stage for that device; the library keeps the slot intact until those calls have executed.  It marks the point behind
 * them on `stream` at the calling thread's NEXT pai_host_stage for that device: `stream` must still exist then (a caller that destroys
 * it first stages once more on a stream that lives on, NULL for instance).  The calls that stage and launch in one (the two _host calls
 * below, pai_threshold_combine) mark that point themselves before they return and never touch their stream again. */
#define PAI_HOST_STAGE_MAX 4096
int pai_host_stage(int device, int parts, const void* const* h_src, const size_t* bytes, void* stream, void** d_ptrs);
/* pai_ct_add_aligned / pai_ct_mul (below) with their small operand — the shifts, the exponents — still on the HOST (at most
 * PAI_HOST_STAGE_MAX bytes): staged as by pai_host_stage and read by the kernel in place, in one call. */
int pai_ct_add_aligned_host(const pai_pubkey* pk, const uint32_t* d_a, const uint32_t* d_b, int b_bcast, const int32_t* h_delta,
                            size_t N, uint32_t* d_out, void* stream);
int pai_ct_mul_host(const pai_pubkey* pk, const uint32_t* d_ct, const uint32_t* h_e, int e_words, int ebits_max, int e_bcast, size_t N,
                    uint32_t* d_out, void* stream);

/* ---- container operations on device rows (no arithmetic) -----------------------------------------
 * ipclPlainText / ipclCipherText __getitem__ with a slice and rotate (bindings/ipcl_bindings_classes.cpp:224-262,328-366;
 * rotate is what the reference's reductions are built from, ipcl_python.py:810-827).  Rows of `row_words` words.
 * slice:  d_out[i] = d_src[start + i * step] for i < count (step >= 1);  rotate:  d_out[i] = d_src[(i + shift) mod N]
 * (any sign of shift).  d_out must not overlap the rows the call reads (PAI_E_INVALID; slice: rows start .. start + (count - 1) step).
 * Asynchronous on `stream`. */
int pai_buf_slice(int device, const uint32_t* d_src, int row_words, size_t start, size_t count, size_t step, uint32_t* d_out,
                  void* stream);
int pai_buf_rotate(int device, const uint32_t* d_src, int row_words, size_t N, long long shift, uint32_t* d_out, void* stream);

/* ---- keys ------------------------------------------------------------------------------------- */
/* ipclPublicKey(n, bits, enableDJN) — classes.cpp:24-27 — and the pickle form
 * (scheme, n, bits, hs, randbits) — ipcl_bindings.cpp:66-98.  h_hs == NULL selects the standard
 * scheme (obfuscator r^n); otherwise the DJN scheme (obfuscator hs^r, r of `randbits` bits) and the
 * fixed-base table for hs is built on the device by the first call that obfuscates (pai_encrypt with randomness /
 * pai_obfuscate): a handle that only adds, multiplies or decrypts never allocates it. */
int pai_pubkey_create(const uint32_t* h_n, int n_words, int key_bits, const uint32_t* h_hs, int hs_words,
                      int randbits, int device, pai_pubkey** out);
void pai_pubkey_destroy(pai_pubkey* pk);
/* Extension for many-key (federated) deployments: frees what the handle holds beyond its constants — the DJN fixed-base
 * tables (8.6 GB at 2048-bit keys; the next obfuscating call rebuilds them, sized from the memory that is free THEN) and
 * the grow-only scratch of the batch operations.  Synchronises the device.  *freed_bytes (optional): device memory returned. */
int pai_pubkey_trim(pai_pubkey* pk, size_t* freed_bytes);
/* fills any non-NULL out-parameter */
int pai_pubkey_info(const pai_pubkey* pk, int* key_bits, int* n_words, int* ct_words, int* r_words,
                    int* randbits, int* is_djn, int* device);
/* The DJN fixed-base table this handle holds right now (zeros before its first obfuscating call and after a trim or an
 * eviction): device bytes, window width in bits, number of windows.  The first keys of a device get the big table (1/32 of
 * the device memory), later ones the small operating point (PAI_FB_BIG_KEYS / PAI_FB_SMALL_TABLE_MB). */
int pai_pubkey_table_info(const pai_pubkey* pk, size_t* table_bytes, int* window_bits, int* windows);
/* The batch sizes at which this key's calls change kernel family on its device (csrc/path_ranges.hpp: every range is a number
 * of elements per compute unit times the device's CU count; PAI_LATENCY_MAX / PAI_LAT_ADD_MAX / PAI_TUNE overrides included):
 * op 0 = pai_decrypt, 1 = pai_encrypt (DJN), 2 = pai_ct_mul, 3 = pai_ct_add*, 4 = pai_ct_pack (its edge counts OUTPUT rows).  An edge E
 * separates N = E from N = E + 1.
 * Writes at most `cap` edges (ascending) and the full count.  For tests and probes that want to stand on both sides of a switch
 * (tests/test_gpu_path_edges.py); no reference counterpart. */
int pai_path_edges(const pai_pubkey* pk, int op, size_t* edges, int cap, int* count);

/* ipclKeypair.generate_keypair(n_length, enable_DJN) — bindings/ipcl_bindings.cpp:12-15 -> ipcl::generateKeypair
 * (timed by the reference's BM_KeyGen, bench/bench_ipcl_python.py:13-19).  Host-only (no device work): two random primes
 * of key_bits/2 bits with the two top bits set (so p*q has exactly key_bits bits), p != q; djn != 0 adds upstream's DJN
 * constraints p = q = 3 (mod 4), gcd(p-1, q-1) = 2.  Incremental search over a sieve of the primes below 2^16, Miller-
 * Rabin with base 2 and 24 random bases, the two primes searched on two host threads.  key_bits: a multiple of 64,
 * 128..8192.  h_seed == NULL: the kernel CSPRNG (getrandom); a seed makes the key reproducible (tests only — such a
 * key is NOT secret).  h_p, h_q receive key_bits/64 words each, p < q not guaranteed. */
int pai_keygen(int key_bits, int djn, const uint64_t* h_seed, uint32_t* h_p, uint32_t* h_q);
/* Host big-integer modular exponentiation for key set-up (the DJN base hs = (-x^2)^n mod n^2 of ipcl::PublicKey's
 * constructor, classes.cpp:24-27): h_out = h_base ^ h_exp mod h_mod for an odd modulus of mod_words words (<= 260);
 * h_base: mod_words words, < modulus; h_out: mod_words words.  Host-only, synchronous. */
int pai_host_modexp(const uint32_t* h_base, const uint32_t* h_exp, int exp_words, const uint32_t* h_mod, int mod_words,
                    uint32_t* h_out);
/* h_out = h_a^-1 mod h_m (m_words words, canonical).  PAI_E_INVALID when gcd(a, m) != 1 or m < 2.  a may exceed m.  Any modulus,
 * even ones included (extended Euclid): the exponents n^-1 mod (s - 1) of pai_recover_r.  Host-only, synchronous. */
int pai_host_modinv(const uint32_t* h_a, int a_words, const uint32_t* h_m, int m_words, uint32_t* h_out);

/* ipclPrivateKey(pubkey, p, q) — classes.cpp:96-101.  p and q may come in either order; n == p*q is
 * checked.  Derives p^2, q^2, hp, hq, p^-1 mod q. */
int pai_privkey_create(const pai_pubkey* pk, const uint32_t* h_p, int p_words, const uint32_t* h_q, int q_words,
                       pai_privkey** out);
/* Every call on sk needs its public handle alive; pai_privkey_destroy alone may come after pai_pubkey_destroy (it frees the private
 * handle's own device memory on the device recorded at creation and does not look at pk). */
void pai_privkey_destroy(pai_privkey* sk);

/* ---- hot path --------------------------------------------------------------------------------- */
/* ipclPublicKey.encrypt(pt, make_secure=false) — classes.cpp:53-60; L3 raw_encrypt, ipcl_python.py:103-106.
 * d_ct[i] = (1 + d_m[i] * n) mod n^2.   d_m: [N][n_words], each < n.   d_ct: [N][ct_words]. */
int pai_raw_encrypt(const pai_pubkey* pk, const uint32_t* d_m, size_t N, uint32_t* d_ct, void* stream);
/* PaillierEncryptedNumber + plaintext — ipcl_python.py:495-504 raw-encrypts the plaintext (classes.cpp:53-60 with make_secure=false)
 * and :365-381 / classes.cpp:318-321 multiply the two ciphertexts; in ONE pass here:
 * d_out[i] = d_ct[i] * (1 + d_m[i] * n) mod n^2, wire form in and out (round 6: the reference's BM_Add_CTPT is two launches and an
 * intermediate array otherwise).  d_m: [N][n_words] residues < n (already encoded AT the ciphertext's exponents: pai_fp_encode_at).
 * d_out may alias d_ct (exactly; it must not overlap d_m).  Small batches run on the latency geometry (three sequential products),
 * others on lane groups. */
int pai_ct_add_plain(const pai_pubkey* pk, const uint32_t* d_ct, const uint32_t* d_m, size_t N, uint32_t* d_out, void* stream);

/* ipclPublicKey.encrypt(pt, make_secure=true) — classes.cpp:53-60 with the randomness made explicit.
 * DJN keys:      d_r: [N][r_words], r_i < 2^randbits;   ct_i = (1 + m_i n) * hs^{r_i} mod n^2.
 * standard keys: d_r: [N][n_words], 0 < r_i < n;         ct_i = (1 + m_i n) * r_i^n   mod n^2. */
int pai_encrypt(const pai_pubkey* pk, const uint32_t* d_m, const uint32_t* d_r, size_t N, uint32_t* d_ct,
                void* stream);

/* ipclPublicKey.apply_obfuscator(CipherText) — classes.cpp:77-83: d_ct[i] <- d_ct[i] * obf(r_i) mod n^2. */
int pai_obfuscate(const pai_pubkey* pk, uint32_t* d_ct, const uint32_t* d_r, size_t N, void* stream);

/* ipclPrivateKey.decrypt(CipherText) — classes.cpp:127-133 (CRT).  d_m: [N][n_words]. */
int pai_decrypt(pai_privkey* sk, const uint32_t* d_ct, size_t N, uint32_t* d_m, void* stream);

/* Ciphertext openings (extension; no reference counterpart).  (m, r) -> (1 + m n) r^n mod n^2 maps Z_n x Z_n^* one-to-one onto the
 * units modulo n^2, so every ciphertext — fresh, summed, scaled, packed, inverted — has exactly one opening, and the holder of p and
 * q computes its r by two half-width exponentiations modulo the primes themselves and one Garner lift (k_rrec_a, k_rrec_b).  With m
 * from pai_decrypt, anyone who holds the public key checks the opening by one standard-scheme encryption with that r, bit for bit.
 *
 * d_r[i] = the unique r in [0, n) with r = (d_ct[i] mod s)^(n^-1 mod (s-1)) mod s for s = p, q, Garner-lifted modulo n.
 * For a unit d_ct[i] this is the r of its opening d_ct[i] = (1 + m n) r^n mod n^2.  d_ct: [N][ct_words] wire form;
 * d_r: [N][n_words].  A row that shares a factor with n gives the same arithmetic (r_s = 0 for that prime), no error.
 * The exponents and the constants that reduce a row modulo s are built by the first call; PAI_E_INVALID, and nothing launched, when
 * n is not coprime to (p - 1)(q - 1) (pai_privkey_create accepts such keys: they decrypt).  One route for every key and batch size;
 * `PAI_TUNE rrec_grid` caps the workgroups per prime.  Asynchronous on `stream`. */
int pai_recover_r(pai_privkey* sk, const uint32_t* d_ct, size_t N, uint32_t* d_r, void* stream);

/* Batch verification of openings (extension): the two sides of the small-exponent test, one exponentiation by n per SEGMENT instead
 * of one per row.  The N rows are cut into S = ceil(N / seg_len) segments of consecutive rows (the last may be short); with the
 * caller's coefficients e_i,
 *     d_lhs[s] = prod ct_i^(e_i) mod n^2,      d_rhs[s] = (1 + n M_s) B_s^n mod n^2,
 *     M_s = sum e_i m_i mod n,                 B_s = prod r_i^(e_i) mod n          (over the rows i of segment s),
 * both [S][ct_words] canonical residues in the wire form.  If every ct_i = (1 + m_i n) r_i^n mod n^2 the two agree for any
 * coefficients; comparing them, and what an agreement proves for secret random coefficients, is the caller's business
 * (PaillierPublicKey.verify_openings).  *d_flag is one device word the caller zeroes: bit 0 is set when some B_s is not a unit modulo n —
 * the rows of d_rhs then prove nothing (a multiple of a prime factor squares to 0 in that component on both sides).
 * d_ct: [N][ct_words] residues modulo n^2; d_m, d_r: [N][n_words] residues modulo n (range checks are the caller's: a row the caller
 * excludes enters as ct = 1, m = 0, r = 1); d_e: [N][e_words] little-endian words of at most ebits_max
 * bits, 1 <= e_words <= 8, 0 < ebits_max <= 32 e_words; seg_len >= 1 — anything else is PAI_E_INVALID and launches nothing.
 * Keys the digit engine serves fold r and m modulo n in k_open_fold over the chunk plan of the ciphertexts' sparse
 * multi-exponentiation; wider keys, and every key under PAI_DISABLE=open_fold, run three sparse multi-exponentiations modulo n^2
 * instead — the same bits.  PAI_TUNE open_chunk: elements per lane (default: smexp_chunk's rule); open_wbits: window of the chain
 * modulo n.  A call whose power tables do not fit the device is cut into row blocks on segment boundaries.  Synchronises `stream`
 * (the combine steps' sizes). */
int pai_opening_fold(const pai_pubkey* pk, const uint32_t* d_ct, const uint32_t* d_m, const uint32_t* d_r, size_t N, const uint32_t* d_e,
                     int e_words, int ebits_max, size_t seg_len, uint32_t* d_lhs, uint32_t* d_rhs, int32_t* d_flag, void* stream);

/* Threshold decryption (extension; no reference counterpart): Damgard-Jurik / Fouque-Poupard-Stern at s = 1
 * with a trusted dealer.  The dealing is host arithmetic of the Python layer (threshold.py); the library raises ciphertexts to a
 * shareholder's exponent and combines t partial decryptions with the public key alone.  Honest-but-curious parties only: there are
 * no verification keys and no proofs.
 *
 * A key-share handle owns ONE exponent E (for shareholder i of l: 2 l! s_i, not reduced — the shareholder does not know the
 * group order), its e_words little-endian words on the device and its sliding-window schedule.  The schedule makes the kernel's control
 * flow — the run lengths of squarings, the table indices — a function of the share, exactly as the decrypt kernels' schedules are
 * functions of p - 1 and q - 1: a party that can time or trace the device learns about E what it learns about p and q there.
 * pai_keyshare_destroy overwrites the exponent and the schedule, on the device and on the host, before freeing them.  The public handle
 * must outlive every call on the share (not its destruction). */
typedef struct pai_keyshare pai_keyshare;
int pai_keyshare_create(const pai_pubkey* pk, const uint32_t* h_e, int e_words, pai_keyshare** out);   /* E > 0, 1 <= e_words <= 1024 */
void pai_keyshare_destroy(pai_keyshare* share);
/* d_out[i] = d_ct[i]^E mod n^2, the canonical residue in the wire form; d_ct, d_out: [N][ct_words].  Routes with identical bits:
 * keys the digit engine serves, from the hand-over edge `PAI_TUNE tpart_min` on (default: where pai_ct_mul reaches its
 * one-element-per-lane kernel), run k_pow_padic on the share's own schedule (`PAI_TUNE tpart_grid` caps its workgroups: a small batch
 * then walks the tile loop); every other call — small and mid-size batches, wider keys — takes the routes of pai_ct_mul with E as the
 * broadcast exponent.  d_out must not overlap d_ct in any way (k_pow_padic reads its input through __restrict__): PAI_E_INVALID, nothing
 * launched.  Asynchronous on `stream`. */
int pai_partial_decrypt(pai_keyshare* share, const uint32_t* d_ct, size_t N, uint32_t* d_out, void* stream);
/* Combines t partial decryptions of the same N ciphertexts:
 *     d_m[i] = L( prod_j parts_j[i]^(+-mu_j) mod n^2 ) theta mod n,      L(x) = (x - 1) / n,
 * d_m: [N][n_words].  h_parts: HOST array of t device pointers to [N][ct_words] wire-form rows; h_mu: HOST [t][mu_words] little-endian
 * magnitudes of the exponents (for a share set S: |2 mu_j|, mu_j = l! prod_(k in S, k != j) k / (k - j)); h_neg: HOST t flags, non-zero =
 * the exponent is negative; h_theta: HOST [n_words], a residue modulo n ((4 (l!)^2)^-1 mod n).  The members with a negative exponent
 * form a second product P-, inverted once: x = P+ (P-)^-1.  *d_flag (one device word the caller zeroes): bit 0 — some row's x is not
 * 1 modulo n: an inconsistent set of partial decryptions (a wrong index, a corrupted row, too few shares); that row of d_m is defined
 * but meaningless; bit 1 — some row of P- is not a unit modulo n^2 (its row of d_m is then undefined).  d_rowflag: NULL, or int32 [N]
 * the caller zeroes: 1 on the rows behind bit 0.
 * PAI_E_INVALID, nothing launched: t outside 1 .. 16, mu_words outside 1 .. 4, a zero coefficient, theta >= n, d_m overlapping a part.
 * Routes with identical bits: keys the digit engine serves form P+ and P- in one kernel, k_tcomb_padic (the t partials in Montgomery
 * digit form in a per-lane table, one binary chain per side; `PAI_TUNE tcomb_min`: from this many rows on; default: t >= 3 and pai_partial_decrypt's edge, where it was measured ahead;
 * `PAI_TUNE tcomb_grid` caps its workgroups); wider keys, and every key under PAI_DISABLE=tcombine, form them by pai_ct_mul per
 * part and pai_ct_addn per side.  Then pai_ct_invert_flag on P-, pai_ct_add, and k_tfinish (exact division by n, the test, times theta).
 * Asynchronous on `stream`. */
int pai_threshold_combine(const pai_pubkey* pk, const uint32_t* const* h_parts, int t, const uint32_t* h_mu, const int32_t* h_neg,
                          int mu_words, const uint32_t* h_theta, size_t N, uint32_t* d_m, int32_t* d_flag, int32_t* d_rowflag,
                          void* stream);

/* The Fiat-Shamir transcript of verifiable threshold decryption (extension; threshold.py holds the byte layout):
 * SHA-256 (FIPS 180-4) on the device, so that ciphertexts and partial decryptions are hashed where they lie.
 *
 * pai_sha256_rows: one digest per row.  h_parts: HOST array of K device pointers, part k [N][h_words[k]] 32-bit words; h_words: HOST K
 * word counts.  The message of row j is the concatenation over k < K of row j of part k, the words exactly as they lie in memory (for
 * wire-form residues: their little-endian bytes); d_digest: [N][8] words whose 32 bytes, in memory order, are the standard digest —
 * hashlib.sha256(message).digest().  1 <= K <= 4, 1 <= h_words[k] <= 4096 (any value, not only multiples of 16), N < 2^31; d_digest
 * must not overlap a part — anything else is PAI_E_INVALID and launches nothing.  N == 0 is a no-op.  One row per lane, a grid-stride
 * loop over tiles of 256 rows (`PAI_TUNE sha_grid` caps the workgroups: a small batch then walks the loop).  A 64-byte block that lies
 * inside one part whose rows keep 16-byte alignment is loaded as four 16-byte vectors, every other block word by word.  Kernel name
 * k_sha256_rows.  Asynchronous on `stream`.
 *
 * pai_sha256_expand: row j of d_e [N][e_words] holds the first 4 e_words bytes of SHA-256(seed || tag || LE64(first_index + j)) as
 * little-endian words, the top word masked so that the row is below 2^bits.  h_seed32: HOST 32 bytes; h_tag: HOST tag_len bytes,
 * tag_len <= 15 (the message is one block); 32 <= bits <= 256, e_words = ceil(bits / 32), N < 2^31 — anything else is PAI_E_INVALID and
 * launches nothing.  first_index + j wraps modulo 2^64.  Kernel name k_sha256_expand.  Asynchronous on `stream`. */
int pai_sha256_rows(const pai_pubkey* pk, const uint32_t* const* h_parts, const int32_t* h_words, int K, size_t N, uint32_t* d_digest,
                    void* stream);
int pai_sha256_expand(const pai_pubkey* pk, const uint8_t* h_seed32, const uint8_t* h_tag, int tag_len, uint64_t first_index, size_t N,
                      int bits, uint32_t* d_e, int e_words, void* stream);

/* Owner-side encryption: pai_encrypt / pai_obfuscate by the party that holds p and q — the same bits for the same r.  Served
 * calls (DJN keys whose primes the encryption digit engine accepts, batches from the hand-over edge `PAI_TUNE crtenc_min` on,
 * PAI_DISABLE=crtenc not set) compute hs^r as two half-width fixed-base exponentiations modulo p^2 and q^2 and one Garner lift
 * (k_crt_lift), then multiply 1 + m n [the ciphertext] in modulo n^2; every other call is the public call.  The base-p / base-q
 * tables are built by the first served call and belong to the public handle's table set: same byte budget (PAI_FB_CACHE_MB), evicted
 * with the public tables, freed by pai_pubkey_trim, rebuilt bit-identical. */
int pai_encrypt_crt(pai_privkey* sk, const uint32_t* d_m, const uint32_t* d_r, size_t N, uint32_t* d_ct, void* stream);
int pai_obfuscate_crt(pai_privkey* sk, uint32_t* d_ct, const uint32_t* d_r, size_t N, void* stream);
/* The base-p / base-q tables held right now: bytes of both, window width and windows of each (zeros before the first served call). */
int pai_privkey_crt_table_info(const pai_privkey* sk, size_t* table_bytes, int* window_bits, int* windows);

/* ipclCipherText.__add__(ct, ct) — classes.cpp:318-321: d_out[i] = d_a[i] * d_b[i] mod n^2.
 * b_bcast != 0: d_b holds one ciphertext used for every i (size-1 broadcast).  d_out may alias d_a, or d_b when b_bcast == 0 or
 * N == 1 (exactly: the memory contract above; a broadcast row inside a longer output is PAI_E_INVALID).
 * Operands are residues modulo n^2 (as everywhere in this ABI); the result is the canonical residue.  (Batches beyond the
 * small-batch range run one most-significant-limb-first product per element, csrc/mont_msb.hpp, which would also accept rows that
 * are not reduced; the small-batch route does not promise that.) */
int pai_ct_add(const pai_pubkey* pk, const uint32_t* d_a, const uint32_t* d_b, int b_bcast, size_t N,
               uint32_t* d_out, void* stream);

/* ipclCipherText.__mul__(ct, pt) — classes.cpp:324-325: d_out[i] = d_ct[i] ^ e_i mod n^2, e_i >= 0.
 * d_e: [N][e_words] (or one row if e_bcast); ebits_max bounds the bit length of every e_i.  d_out may alias d_ct (exactly: every
 * path reads row i before it stores row i, with per-element and with broadcast exponents); it must not overlap d_e. */
int pai_ct_mul(const pai_pubkey* pk, const uint32_t* d_ct, const uint32_t* d_e, int e_words, int ebits_max,
               int e_bcast, size_t N, uint32_t* d_out, void* stream);

/* Replaces the per-element gmpy2.invert of PaillierEncryptedNumber.__invert_ct (ipcl_python.py:272-276):
 * d_out[i] = d_ct[i]^-1 mod n^2 (batched: simultaneous inversion as a product tree + one extended GCD per top-level
 * product).  Synchronous; fails with PAI_E_INVALID if some ciphertext shares a factor with n.  d_out may alias d_ct
 * (exactly; a partial overlap is PAI_E_INVALID, here and in the two forms below). */
int pai_ct_invert(const pai_pubkey* pk, const uint32_t* d_ct, size_t N, uint32_t* d_out, void* stream);
/* The same work without the synchronisation: returns as soon as the kernels are queued on `stream`; a non-invertible input
 * sets bit 0 of the handle's sticky status word (pai_pubkey_status below) instead of failing the call. */
int pai_ct_invert_async(const pai_pubkey* pk, const uint32_t* d_ct, size_t N, uint32_t* d_out, void* stream);
/* The asynchronous form whose outcome travels with the RESULT instead of the handle: *d_flag (one device word the caller owns,
 * zeroed by the caller) receives bit 0 when an input of THIS call is not invertible (the output rows are then undefined).  The
 * Python layer keeps the word with the container built from d_out (and with everything computed from it) and reads it — one
 * synchronisation — when that container is exported or decrypted, so the error is raised on the faulty object. */
int pai_ct_invert_flag(const pai_pubkey* pk, const uint32_t* d_ct, size_t N, uint32_t* d_out, int32_t* d_flag, void* stream);

/* __raw_add with its exponent alignment fused (ipcl_python.py:490-526 + :570-741): delta_i = exponent(a_i) - exponent(b_i)
 * (base-2 fixed-point exponents, int32 on the device); the operand with the LOWER exponent is raised first:
 * d_out[i] = delta_i > 0 ? d_a[i] * d_b[i]^(2^delta_i) : d_a[i]^(2^-delta_i) * d_b[i]   (mod n^2).
 * The result's exponent is max(exponent(a_i), exponent(b_i)) (the caller's bookkeeping).  One pass over the data instead
 * of two pai_ct_pow2 passes and a pai_ct_add.  b_bcast != 0: one ciphertext b for every i.  d_out may alias d_a, or d_b
 * when b_bcast == 0 or N == 1 (exactly; a broadcast row inside a longer output is PAI_E_INVALID, as for pai_ct_add; the same holds
 * for pai_ct_add_aligned_host and pai_ct_add_aligned_dom). */
int pai_ct_add_aligned(const pai_pubkey* pk, const uint32_t* d_a, const uint32_t* d_b, int b_bcast, const int32_t* d_delta,
                       size_t N, uint32_t* d_out, void* stream);

/* n-ary ciphertext sum in one pass — the aggregation sum_j E(x_j) over k parties' arrays, which the reference spells as a chain
 * of PaillierEncryptedNumber.__add__ calls with their exponent alignments (ipcl_python.py:365-381, 490-526, 570-741;
 * tests/ipcl_python_test.py:21-38):  d_out[i] = prod_{j<k} op_j[i]^(2^raise_j[i]) mod n^2, 2 <= k <= 16.
 * h_ops: HOST array of k device pointers to [N][ct_words] rows; h_raise: NULL, or a HOST array of k device pointers (entries may
 * be NULL) to int32 [N] squaring counts >= 0 — the caller raises every operand to the per-element maximum exponent of the sum.
 * Lazy-domain bookkeeping as for pai_ct_mont_mul: operand 0 holds x R^tag0, the others x R^tag, the result x R^dom_out (any tags
 * with |.| small: wire form is 0; tag0 + (k-1)(tag-1) is the tag that costs no extra product; a raised operand 0 needs tag0 ==
 * tag).  k - 1 Montgomery products per element (+1 per raised operand and per squaring), one store.  d_out may alias an operand (exactly: any
 * one of the k; a partial overlap with any of them is PAI_E_INVALID).
 * Asynchronous on `stream`. */
int pai_ct_addn(const pai_pubkey* pk, const uint32_t* const* h_ops, const int32_t* const* h_raise, int k, int tag0, int tag,
                int dom_out, size_t N, uint32_t* d_out, void* stream);

/* Lazy Montgomery domain for chains of additions (extension).  A ciphertext buffer may hold x R^k mod n^2
 * instead of x (R = 2^bits of pai_pubkey_mont_bits; the caller tracks the integer k per buffer — k = 0 is the wire form).
 * pai_ct_mont_mul: d_out[i] = d_a[i] * d_b[i] * R^-1 mod n^2 (canonical residue), ONE Montgomery product per element where
 * pai_ct_add needs two (or the 1.4 x dearer most-significant-limb-first product): operands with tags ka, kb give ciphertext-addition with tag ka + kb - 1.  Multiplying by the
 * broadcast constant R^(1 + k' - k) mod n^2 (b_bcast != 0) moves a buffer from tag k to tag k', e.g. back to the wire
 * form before decryption, export or pickling — the bits at every boundary are those of CipherText::operator+
 * (classes.cpp:318-321).  d_out may alias d_a, or d_b when b_bcast == 0 or N == 1 (exactly, as for pai_ct_add). */
int pai_ct_mont_mul(const pai_pubkey* pk, const uint32_t* d_a, const uint32_t* d_b, int b_bcast, size_t N, uint32_t* d_out,
                    void* stream);
int pai_pubkey_mont_bits(const pai_pubkey* pk, int* bits);
/* pai_ct_add_aligned on buffers that share a tag k: d_entry = one packed row holding R^(2 - k) mod n^2 (for k = 0 this
 * is what pai_ct_add_aligned uses); the result carries tag k. */
int pai_ct_add_aligned_dom(const pai_pubkey* pk, const uint32_t* d_a, const uint32_t* d_b, int b_bcast, const int32_t* d_delta,
                           size_t N, uint32_t* d_out, const uint32_t* d_entry, void* stream);

/* The reductions of PaillierEncryptedNumber.sum / __matmul__ (ipcl_python.py:746-762, 810-880): upstream pads to a
 * power of two with E_raw(0) = 1 and runs log2 steps of CipherText::rotate + operator+ (__padded_ct, :810-827),
 * i.e. computes the product of a group of ciphertexts modulo n^2.  Here: d_ct holds `count` rows read as
 * [count/groups][groups] (member-major), and d_out[g] = prod_l d_ct[l*groups + g] mod n^2 for g < groups — a
 * product tree over halves, one Montgomery product per node.  The product is order-independent, so the bits equal
 * upstream's rotate-and-add result.  count must be a positive multiple of groups; groups == 1 is sum(). */
int pai_ct_prod(const pai_pubkey* pk, const uint32_t* d_ct, size_t count, size_t groups, uint32_t* d_out, void* stream);

/* The matrix products PaillierEncryptedNumber.__matmul__ / __rmatmul__ / dot (ipcl_python.py:829-930): every output
 * element is a sum of ciphertext * plaintext terms aligned to a common exponent, i.e. the product of powers
 *     d_out[r * M + j] = prod_{l < K}  base(r, l, j)^(e[r][l][j])  mod n^2,
 * base(r, l, j) = d_ct[r * K + l], or d_ct_inv[r * K + l] (the caller's pai_ct_invert of d_ct) where d_sign[l * M + j] != 0
 * (negative multipliers, ipcl_python.py:426-437); e = |mantissa| << alignment shift, e_words words each, little endian,
 * laid out [R][K][M][e_words]; ebits_max bounds every exponent.  d_sign and d_ct_inv are both NULL or both given.
 * One chain of squarings per output element and chunk of members instead of one per term (Straus; windows of 2..7 bits
 * over per-base power tables built on the fly, the width chosen from the shape; on base-n digit pairs for keys up to 2048 bits,
 * on lane groups above).  PAI_E_UNSUPPORTED when the power tables (2^w entries per base and sign) do not fit — the caller then takes
 * the term-by-term route (pai_ct_mul + pai_ct_add_aligned / pai_ct_prod).  The bits equal that route's: the result is the
 * canonical residue of the same product. */
int pai_ct_multiexp(const pai_pubkey* pk, const uint32_t* d_ct, const uint32_t* d_ct_inv, size_t R, size_t K, size_t M,
                    const uint32_t* d_e, int e_words, int ebits_max, const uint8_t* d_sign, uint32_t* d_out, void* stream);

/* Segment products behind PaillierEncryptedNumber.segment_sum (extension; no reference counterpart): S Horner chains over
 * gathered rows,  d_out[s] = the chain  acc <- acc^(2^d_shift[j]) * d_ct[d_rows[j]]  over members j = d_offsets[s] ..
 * d_offsets[s+1] - 1, in the wire form (canonical residues), the shift of a chain's first member ignored; an empty chain gives 1.
 * With the members of a segment sorted by exponent and shift = the step to the previous member's exponent, this is
 * prod_j ct_j^(2^(E_s - e_j)) mod n^2 — the exponent-aligned sum of the segment — at one Montgomery product per member plus
 * one per unit of the segment's exponent spread.  d_ct: [N][ct_words] at domain tag `tag` (pai_ct_mont_mul; 0 = wire form,
 * |tag| <= 46); d_rows: uint32 row indices (NULL: member j is row j); d_shift: int32 steps >= 0 (NULL: all 0); d_offsets: int64
 * [S + 1], nondecreasing, d_offsets[S] = the number of members.  A row >= N is skipped together with its shift and a negative
 * shift counts as 0, at every chunk length alike; either sets bit 2 of the handle's status word (pai_pubkey_status) and never
 * reads outside d_ct.  The first member's shift is never applied, but its sign is counted like any other: a negative value there
 * sets bit 2 as well.  Long segments are cut into chunks whose partial products are combined by further levels on the handle's
 * scratch (PAI_TUNE segprod_chunk: the chunk length).
 * Reads d_offsets[S] and the longest segment back first (one synchronisation of `stream`); the rest is asynchronous. */
int pai_ct_segment_prod(const pai_pubkey* pk, const uint32_t* d_ct, size_t N, int tag, const uint32_t* d_rows, const int32_t* d_shift,
                        const int64_t* d_offsets, size_t S, uint32_t* d_out, void* stream);

/* Segment scans behind PaillierEncryptedNumber.cumsum (extension; no reference counterpart): the N rows of d_ct are N / seg_len
 * contiguous runs of seg_len rows, and within each run, in scan order (ascending rows, or descending when reverse != 0),
 *     acc_first = ct_first^(2^raise_first),   acc_i = acc_prev^(2^step_i) * ct_i^(2^raise_i)  mod n^2,
 *     d_out[i] = acc_i * R^dom_out, the canonical residue (dom_out = 0: the wire form).
 * With raise_i = E_i - e_i and step_i = E_i - E_(i-1), E the running maximum of the exponents e, row i is the exponent-aligned sum
 * of its run's rows up to i.  d_ct: [N][ct_words] at domain tag `tag` (pai_ct_mont_mul; |tag|, |dom_out| <= 46); d_raise, d_step:
 * int32 [N] indexed by row, NULL = all 0; the step of a run's first row is ignored; both may be non-zero on one row.  seg_len must
 * divide N (PAI_E_INVALID otherwise); d_out: [N][ct_words], must not overlap d_ct (PAI_E_INVALID).  A negative raise or step counts as 0 and sets
 * bit 4 of the handle's status word (pai_pubkey_status) — also the step of a run's first row, which is never applied.  Cost: 1 + [tag != 1] + [dom_out != 1] Montgomery products per row plus
 * one per squaring, when there are enough runs to give every lane group of the device one.  Fewer runs are cut into chunks
 * (PAI_TUNE scan_chunk: the chunk length): chunk totals, the scan of the totals (the same call on the handle's scratch, level by
 * level), then the chunks again, seeded with their carries — three launches and about twice the products per level, and no
 * workgroup waits for another.  Runs are uniform, so no size is read back: the call is fully asynchronous on `stream`. */
int pai_ct_scan(const pai_pubkey* pk, const uint32_t* d_ct, size_t N, int tag, int dom_out, size_t seg_len, int reverse,
                const int32_t* d_raise, const int32_t* d_step, uint32_t* d_out, void* stream);

/* Sparse multi-exponentiation behind PaillierEncryptedNumber.csr_matmul / csr_rmatmul and the scipy forms of @ (extension; no
 * reference counterpart): T terms in segment order, d_out[s] = prod over the terms t = d_offsets[s] .. d_offsets[s+1] - 1 of
 * B_t^(e_t) mod n^2, in the wire form (canonical residues); an empty segment gives 1.  B_t = d_ct[d_base[t]], or
 * d_ct_inv[d_base[t]] when d_sign[t] != 0.  d_ct, d_ct_inv: [N][ct_words] wire form (d_ct_inv and d_sign both NULL or both
 * given); d_base: int32 [T]; d_e: [T][e_words] little-endian exponent words of at most ebits_max bits; d_sign: uint8 [T];
 * d_offsets: int64 [S + 1], nondecreasing, d_offsets[S] = T.  One power table per base (and sign), shared by all its terms;
 * chunks of consecutive terms of a segment run one Straus chain each (PAI_TUNE smexp_chunk: the chunk length) and their partials
 * are combined per segment as in pai_ct_segment_prod.  A base outside [0, N) is skipped, offsets that step back or leave [0, T]
 * are clamped (those terms are dropped); either sets bit 3 of the handle's status word and never reads out of bounds.
 * PAI_E_UNSUPPORTED: T >= 2^31, N >= 2^28, or the tables do not fit the device.  Synchronises `stream` once (the combine's
 * sizes). */
int pai_ct_sparse_multiexp(const pai_pubkey* pk, const uint32_t* d_ct, const uint32_t* d_ct_inv, size_t N, const int32_t* d_base,
                           const uint32_t* d_e, int e_words, int ebits_max, const uint8_t* d_sign, size_t T, const int64_t* d_offsets,
                           size_t S, uint32_t* d_out, void* stream);

/* Exponent alignment, ipcl_python.py:570-741 (ct * 2^delta as ciphertext^(2^delta)):
 * for delta_i > 0: d_ct[i] <- d_ct[i]^(2^delta_i) mod n^2; other elements are left untouched.
 * Batches of >= 16384 elements (PAI_POW2_DIGIT_MIN) on keys up to 2048 bits read the largest shift back first (this
 * synchronises `stream`) and run shifts of 8..62 as ct^e with the one-bit exponent 2^delta on the base-n digit engine. */
int pai_ct_pow2(const pai_pubkey* pk, uint32_t* d_ct, const int32_t* d_delta, int delta_bcast, size_t N,
                void* stream);
/* The same with the caller's knowledge of max_i delta_i (the Python layer builds delta on the host and knows it): no
 * read-back, the call is asynchronous for every batch size.  max_delta must be >= every delta_i (0: nothing to do). */
int pai_ct_pow2_hint(const pai_pubkey* pk, uint32_t* d_ct, const int32_t* d_delta, int delta_bcast, size_t N, int max_delta,
                     void* stream);
/* Sticky status word of a handle's ASYNCHRONOUS calls, read with a synchronisation of `stream` (and cleared when
 * clear != 0): bit 0 — pai_ct_invert_async met a ciphertext that is not invertible modulo n^2 (its output rows are then
 * undefined); bit 1 — a pai_ct_pow2_hint call was given a max_delta below a shift of its batch on the digit-engine path
 * (batches >= PAI_POW2_DIGIT_MIN on keys up to 2048 bits, hints the digit path serves; the raised ciphertexts of that call are
 * then wrong — a hint outside that range runs the lane-group kernel, which is correct for any shift, and flags nothing); bit 2 —
 * a pai_ct_segment_prod call met a member row >= N (skipped) or a negative shift (taken as 0); bit 3 — a pai_ct_sparse_multiexp
 * call met a base outside [0, N) (the term skipped) or segment offsets that step back or leave [0, T] (clamped; the terms they
 * drop are skipped); bit 4 — a pai_ct_scan call met a negative raise or step (taken as 0).  The Python layer computes its hints from host arrays, uses pai_ct_invert_flag and builds and checks its
 * segment and term plans itself, so it never depends on this word. */
int pai_pubkey_status(const pai_pubkey* pk, int* status_out, int clear, void* stream);


/* ---- data formats either side of the path --------------------------------------------------------------
 * Fixed-point codec of bindings/fixedpoint.py:54-115 for float64 arrays (the hot Python loops of
 * ipcl_python.py:136-140 and :229-243), on the device so that 8 B instead of 256 B per element cross PCIe.
 * Both need n > 2^66 (any real key).  encode: d_x[N] finite doubles (the caller rejects NaN/Inf like the
 * reference's int()) -> residues d_m[N][n_words] and base-2 exponents d_expo[N].  decode: residues ->
 * signed mantissas d_mant[N] with d_flag[i] = 0, or d_flag[i] = 1 when element i needs the exact big-integer
 * path (|mantissa| >= 2^63, overflow zone or corrupt residue: the host path raises the reference's errors). */
int pai_fp_encode_f64(const pai_pubkey* pk, const double* d_x, size_t N, uint32_t* d_m, int32_t* d_expo, void* stream);
/* the same for int64 arrays: exponent 0, residue = x mod n (fixedpoint.py:72-74,89-96) */
int pai_fp_encode_i64(const pai_pubkey* pk, const int64_t* d_x, size_t N, uint32_t* d_m, int32_t* d_expo, void* stream);
/* Encoders with a target exponent per element (d_target[N], or one value when target_bcast), for the plaintext operand
 * of ct + plaintext (ipcl_python.py:495-504 raw-encrypts it, :570-741 then raise the lower-exponent side by
 * ct^(2^delta)): for a RAW encryption (1 + m n)^(2^d) = 1 + (m 2^d mod n) n, so an element whose own exponent e is below
 * its target t is encoded at t directly (mantissa shifted left by t - e; same ciphertext bits, same exponent, no
 * squarings) whenever |mantissa| 2^(t-e) < 2^(bits(n) - 2); other elements keep e (d_expo tells).  is_f64: d_x is
 * double[N], else int64[N]. */
int pai_fp_encode_at(const pai_pubkey* pk, const void* d_x, int is_f64, size_t N, const int32_t* d_target, int target_bcast,
                     uint32_t* d_m, int32_t* d_expo, void* stream);
int pai_fp_decode_i64(const pai_pubkey* pk, const uint32_t* d_m, size_t N, int64_t* d_mant, int32_t* d_flag, void* stream);

/* ---- packed ciphertexts: k fixed-point slots of b bits per plaintext (extension; no reference counterpart) ---------------
 * Layout of a packed batch of N elements at `slot_bits` b (8..128) and `slots` k >= 1 with k b <= bits(n) - 2: G = ceil(N / k)
 * rows; element i lives in row i / k, slot i % k, bits [j b, (j + 1) b); the plaintext of row g is the signed integer
 * P_g = sum_j m_(g k + j) 2^(b j) reduced modulo n, with signed mantissas -2^(b-1) <= m < 2^(b-1); unused tail slots hold 0.
 * With the bias B = sum_(j<k) 2^(b-1) 2^(b j), Q = (residue + B) mod n < 2^(k b) and m_j = ((Q >> b j) & (2^b - 1)) - 2^(b-1).
 * A layout outside these bounds is PAI_E_INVALID and launches nothing.
 *
 * pai_fp_pack: d_x = double[N] (is_f64) or int64[N]; mantissa = rint(x 2^exponent), ties to even (exact), or x << exponent;
 * d_m: [G][n_words] residues of P_g.  *d_flag (one device word the caller zeroes) receives bit 0 for a mantissa with
 * |m| >= 2^value_bits (1 <= value_bits <= b - 1), bit 1 for a NaN or an infinity; the rows are then undefined. */
int pai_fp_pack(const pai_pubkey* pk, const void* d_x, int is_f64, size_t N, int exponent, int value_bits, int slot_bits, int slots,
                uint32_t* d_m, int32_t* d_flag, void* stream);
/* pai_fp_unpack: d_m: [G][n_words] residues; d_out: int64 [G k] mantissas for b <= 64, int64 [G k][2] = (low 64 bits as uint64,
 * high 64 bits, signed) above; d_flag: int32 [G]: 0 ok, 1 overflow zone (Q >= 2^(k b)), 2 residue >= n (the row's mantissas are
 * then undefined). */
int pai_fp_unpack(const pai_pubkey* pk, const uint32_t* d_m, size_t G, int slot_bits, int slots, int64_t* d_out, int32_t* d_flag,
                  void* stream);
/* pai_ct_pack: packs N ciphertexts (equal exponents: the caller's bookkeeping) into G: d_out[g] = prod_j d_ct[g k + j]^(2^(b j))
 * mod n^2, an encryption of P_g, in the wire form (canonical residues, not re-randomised).  d_ct: [N][ct_words] at domain tag `tag`
 * (as pai_ct_segment_prod); d_out: [G][ct_words], must not overlap d_ct (PAI_E_INVALID; pai_ct_pack_step too).  One Horner chain acc <- acc^(2^b) * ct_j, j = k-1 ... 0,
 * per output row — b squarings and one product per packed element.  Two routes with identical results: the level driver of
 * pai_ct_segment_prod (the member list is written on the device; synchronises `stream` once, like that call), and, for keys up to
 * 2048 bits, wire-form input and batches of more output rows than the pai_path_edges(op 4) edge, one chain per lane on base-n
 * digit pairs (asynchronous; PAI_DISABLE=pack_padic leaves it out). */
int pai_ct_pack(const pai_pubkey* pk, const uint32_t* d_ct, size_t N, int tag, int slot_bits, int slots, uint32_t* d_out, void* stream);
/* pai_ct_pack_step: the same chains with a free step — d_out[g] = prod_(j<count) d_ct[g count + j]^(2^(step_bits j)) mod n^2 in
 * the wire form, G = ceil(N / count) rows, a ragged last chain multiplying only the rows it has.  With step_bits = k b it repacks
 * packed rows of k slots of b bits: `count` consecutive rows become one row of count k slots (element i stays element i, in row
 * i / (count k), slot i % (count k)); pai_ct_pack(b, k) is the case step_bits = b, count = k, with identical bits.  Constraints:
 * step_bits >= 8, count >= 1 and count step_bits <= bits(n) - 2; anything else is PAI_E_INVALID and launches nothing.  Arguments,
 * routes and knobs otherwise as pai_ct_pack (the hand-over counts output rows; PAI_DISABLE=pack_padic, PAI_TUNE pack_padic_min): the
 * level driver synchronises `stream` once, one chain per lane is asynchronous. */
int pai_ct_pack_step(const pai_pubkey* pk, const uint32_t* d_ct, size_t N, int tag, int step_bits, int count, uint32_t* d_out,
                     void* stream);

/* pai_fp_quantize: a plaintext weight matrix at ONE common exponent as the operands of pai_ct_multiexp (R = 1) and
 * pai_ct_sparse_multiexp — the linear maps of packed rows (PaillierPackedNumber.rmatmul / csr_rmatmul): a packed container has one
 * exponent, so per-weight mantissa exponents are not allowed and every weight is rounded to the same grid.  A product of powers of
 * packed rows, prod_l ct_l^(w_l) mod n^2, holds sum_l w_l m_(l,j) in slot j: with |m| < 2^v it satisfies |sum| <= (2^v - 1) S
 * < 2^(v + bit_length(S)), S = sum_l |w_l| — the sums below are what the caller's headroom test needs before any Paillier kernel.
 * Weight (l, j), l < K, j < M, is d_x[l stride_k + j stride_m] (strides in elements, either may be the unit one: X and X.T views go
 * in without a copy); is_f64: doubles, w = rint(x 2^exponent), ties to even, formed on the 53-bit significand as in pai_fp_pack;
 * else int64, w = x << exponent (exact).  d_e[(l M + j) e_words ..]: |w| in little-endian words; d_sign[l M + j] = (w < 0): the
 * [K][M] operands of pai_ct_multiexp, at M = 1 the [T] operands of pai_ct_sparse_multiexp.  d_sum: exact sums of |w| as (low 64 bits,
 * high 64 bits) pairs — d_offsets == NULL: one pair per column j, summed over l (M pairs); d_offsets: int64 [S + 1], nondecreasing
 * (requires M = 1): one pair per segment [d_offsets[s], d_offsets[s + 1]) (S pairs; rows outside every segment count nowhere; S = 0 is allowed: words and signs only).  The
 * call overwrites d_sum; a sum of 2^128 or more is stored as 2^128 - 1.  *d_flag (one device word the caller zeroes): bit 0 for some
 * |w| >= 2^weight_bits (the operands are then undefined), bit 1 for a NaN or an infinity.  1 <= weight_bits <= min(126, 32 e_words),
 * 1 <= e_words <= 4; anything else is PAI_E_INVALID and launches nothing.  Asynchronous on `stream`. */
int pai_fp_quantize(const pai_pubkey* pk, const void* d_x, int is_f64, size_t K, size_t M, long long stride_k, long long stride_m,
                    int exponent, int weight_bits, const int64_t* d_offsets, size_t S, uint32_t* d_e, int e_words, uint8_t* d_sign,
                    uint64_t* d_sum, int32_t* d_flag, void* stream);

/* Obfuscator randomness, replacing upstream ipcl's per-element getRandomBN inside
 * PublicKey::encrypt (called at classes.cpp:57): d_r[N][r_words] <- ChaCha20 key stream (RFC 8439 block
 * function; h_key8 = 256-bit key from the OS CSPRNG, h_nonce3 = 96-bit nonce, 32-bit block counter starting
 * at counter0, carried into nonce word 0), top word of every row masked to randbits.  Standard-scheme keys get rows of
 * bits(n) random bits: candidates for r, of which the caller keeps those in [1, n) (rejection sampling). */
int pai_draw_r(const pai_pubkey* pk, const uint32_t* h_key8, const uint32_t* h_nonce3, uint32_t counter0, size_t N,
               uint32_t* d_r, void* stream);

/* ---- multi-GPU (one node) --------------------------------------------------------------------------------
 * The hot operations are element-wise (encrypt / decrypt / add / mul forward whole std::vector<BigNumber> batches:
 * classes.cpp:53-60, 127-133, 318-325), so a batch shards by contiguous blocks with no exchange inside an operation:
 * shard g of G owns rows [g*ceil(N/G), min(N, (g+1)*ceil(N/G))) (trailing shards may be empty). */
int pai_shard_plan(size_t N, int nshards, int shard, size_t* begin, size_t* count);
/* Single-process fan-out over the visible devices (one key handle per device): gathers row shards living on
 * devices[i] (rows[i] rows of row_words words each, back to back in shard order) into d_out on dst_device, or
 * scatters d_in on src_device into the shards — peer copies over xGMI, all shards in flight at once; returns when
 * the copies have completed.  (One-process-per-GPU jobs gather with RCCL instead: sharding.py.)
 * The two calls take no stream: they copy on the NULL streams of the devices involved and wait for those.  Shards (or d_in) that
 * were produced on a non-blocking stream are not ordered before the copies by anything the library does: the caller synchronises
 * that stream first, as engine._peer_copy does (torch.cuda.synchronize on every device involved). */
int pai_gather(int nshards, const int* devices, const void* const* d_shards, const size_t* rows, int row_words,
               int dst_device, void* d_out);
int pai_scatter(int nshards, const int* devices, void* const* d_shards, const size_t* rows, int row_words,
                int src_device, const void* d_in);

/* ---- generic modular building blocks (arbitrary odd modulus up to 8192 bits) ------------------- */
int pai_modulus_create(const uint32_t* h_m, int m_words, int device, pai_modulus** out);
void pai_modulus_destroy(pai_modulus* m);
/* out[i] = a[i] * b[i] mod M; rows of w32 words (w32 = ceil(bits(M)/32)).  d_out may alias d_a, or d_b when b_bcast == 0 or N == 1
 * (exactly, as for pai_ct_add). */
int pai_modmul(pai_modulus* m, const uint32_t* d_a, const uint32_t* d_b, int b_bcast, size_t N, uint32_t* d_out,
               void* stream);
/* out[i] = base[i] ^ E mod M, E given on the HOST (wave-uniform exponent, fixed 5-bit window) */
int pai_modexp_fixed(pai_modulus* m, const uint32_t* d_base, const uint32_t* h_e, int e_words, size_t N,
                     uint32_t* d_out, void* stream);
/* out[i] = base[i] ^ e[i] mod M, per-element exponents on the DEVICE */
int pai_modexp_var(pai_modulus* m, const uint32_t* d_base, int base_bcast, const uint32_t* d_e, int e_words,
                   int ebits_max, int e_bcast, size_t N, uint32_t* d_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PAILLIER_HIP_H_ */
