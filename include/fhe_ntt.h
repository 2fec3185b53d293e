/*
 * fhe_ntt.h — C ABI of libfhe_ntt.so: the MI355X (gfx950) negacyclic-NTT engine
 * for R_q = Z_q[X]/(X^N+1).
 *
 * This is the drop-in boundary for the hot path of arnaucube/fhe-study's
 * `arith` crate.  The reference has no FFI of its own (it is 100 % safe Rust);
 * the seam is the Rust API `arith::NTT::{ntt,intt}` and `ring_nq::{mul,mul_mut}`.
 * Each entry point below names the reference item it replaces (paths relative
 * to the reference root).  INTEGRATION.md shows the Rust-side binding.
 *
 * Conventions
 *   - Polynomials are `batch × n` row-major arrays of uint64_t coefficient
 *     VALUES (the `v` of `Zq{q,v}`, arith/src/zq.rs:6-10), canonical: v < q.
 *   - The caller owns every buffer; `out` may alias `in` (in-place).
 *   - The arithmetic behind an entry point is the library's choice and never
 *     shows in the words: moduli up to 2^62 run on 64-bit Shoup butterflies (a
 *     pseudo-Mersenne one on five-multiply butterflies: fhe_ntt_plan_arithmetic;
 *     2^62 <= q < 2^63 on strict ones, every value canonical, in the same kernels); a
 *     modulus below 2^30 (e.g. the reference's test moduli 65537, 12289)
 *     and the keyed products whose integers are small run in 32-bit words on
 *     the same tables (env FHE_EXT32=0 disables that; results are identical).
 *   - No function unwinds or aborts: every failure is a negative FHE_E_* code
 *     and a message retrievable with fhe_last_error() (thread-local).  The
 *     reference panics in the same situations; the Rust shim turns a non-zero
 *     return into `panic!`.
 *   - All functions are thread-safe and may be called concurrently, on the same
 *     or different plans, streams and threads.  Entry points that need
 *     intermediates use a library-owned workspace keyed by (device, stream,
 *     calling thread): a thread's calls on a stream are ordered by the stream,
 *     and no two threads or streams ever share a buffer — two host threads
 *     enqueueing on the SAME stream (the NULL default stream included) are
 *     fine.  Plans are immutable and owned by the library until
 *     fhe_ntt_shutdown().
 *   - `*_dev` variants take DEVICE pointers of the current HIP device and a
 *     `hipStream_t` passed as `void*` (NULL = the default stream); they only
 *     enqueue work and never synchronise — except the first use of a plan on a
 *     device, which uploads its tables (call fhe_ntt_plan_prepare() beforehand
 *     to keep that out of, e.g., a stream capture; the products of rows N1 - N3
 *     — BFV, TGGSW x TGLWE, key switching — upload the tables of their internal
 *     primes on the first call per (n, device): run one call before capturing),
 *     growth of a library workspace, and the opt-in FHE_NTT_CHECK_CANONICAL mode.  Device buffers must be 16-byte
 *     aligned (FHE_E_INVALID otherwise; anything hipMalloc returns is).  Host-pointer variants copy
 *     host→device→host around the same kernels and return when `out` is valid.
 *   - There is no CPU fallback: without a HIP device every compute entry point
 *     returns FHE_E_NO_DEVICE.
 */
#ifndef FHE_NTT_H
#define FHE_NTT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes -------------------------------------------------------- */
#define FHE_OK 0
/* n is not a power of two (assert, arith/src/ntt.rs:116), n < 2 (degenerate
 * in the reference, ntt.rs:139) or n > 2^20 (engine limit). */
#define FHE_E_BAD_N (-1)
/* (q-1) % 2n != 0 (assert, ntt.rs:117), q < 3, or q >= 2^63 (where the
 * reference's own Zq::add overflows, zq.rs:225). */
#define FHE_E_BAD_Q (-2)
/* the k = 1,2,... search found no primitive 2n-th root (panic, ntt.rs:130). */
#define FHE_E_NO_ROOT (-3)
/* a NULL pointer where a buffer / plan is required. */
#define FHE_E_NULL (-4)
/* a HIP runtime call or kernel launch failed (message has the HIP error). */
#define FHE_E_HIP (-5)
/* no usable HIP device in this process. */
#define FHE_E_NO_DEVICE (-6)
/* operands of a ring multiply have different (q,n)
 * (assert_eq!(lhs.param, rhs.param), arith/src/ring_nq.rs:565,587). */
#define FHE_E_PARAM_MISMATCH (-7)
/* a coefficient >= q was found by fhe_rq_check_canonical(). */
#define FHE_E_NOT_CANONICAL (-8)
/* invalid argument other than the above (e.g. bad flag, count overflow). */
#define FHE_E_INVALID (-9)

typedef struct fhe_ntt_plan fhe_ntt_plan; /* opaque */

/* ---- plan cache: replaces `roots(q,n)` + CACHE, arith/src/ntt.rs:18-38 ---
 * Memoised per (q,n).  Derives psi by the reference's k=1,2,.. search
 * (ntt.rs:115-131), roots[i] = psi^bitrev(i) (ntt.rs:133-147), roots_inv[i] =
 * roots[i]^(q-2) (ntt.rs:149-161, the same Fermat power, so the tables agree
 * with the reference even for a composite q) and n_inv (ntt.rs:27-30).
 * Host-only: needs no GPU. */
int fhe_ntt_plan_get(uint64_t q, uint64_t n, const fhe_ntt_plan **out);
int fhe_ntt_plan_info(const fhe_ntt_plan *plan, uint64_t *q, uint64_t *n, uint64_t *psi,
                      uint64_t *n_inv);
/* copies the n-entry tables (either pointer may be NULL). */
int fhe_ntt_plan_tables(const fhe_ntt_plan *plan, uint64_t *roots, uint64_t *roots_inv);
/* Uploads the plan's twiddle tables to the CURRENT device now (blocking) instead
 * of at the first transform there — the device-side half of CACHE's one-off
 * table build (ntt.rs:20-38). */
int fhe_ntt_plan_prepare(const fhe_ntt_plan *plan);
/* Which arithmetic the transform kernels run for this plan's modulus — Zq::mul (arith/src/zq.rs:315-328) is generic
 * over q; the engine picks the cheapest exact form at plan time.  Host-only, never fails for a valid plan:
 *   FHE_ARITH_SHOUP62   q < 2^62: Shoup product (10 32-bit multiplies), values in [0,4q) between stages
 *   FHE_ARITH_SHOUP61   q < 2^61: the same with compile-time value bounds (a correction every other stage)
 *   FHE_ARITH_PMERSENNE q = 2^k - delta, 56 <= k <= 61, delta <= 2^(k-39) (2^61 - 2^21 + 1 is one): split
 *                       multiplicand, no quotient, 5 multiplies (FHE_PM=0 in the environment selects SHOUP61 instead)
 *   FHE_ARITH_WORD32    q < 2^30 and 2^8 <= n <= 2^18: one 32-bit word per coefficient (FHE_EXT32=0: SHOUP61); without
 *                       any conditional subtraction in the forward transform below 2^32/25, Harvey's form above.
 *                       Moduli between 2^30 and 2^32, and n outside that range, are NOT covered by this form.
 *   FHE_ARITH_STRICT63  2^62 <= q < 2^63 (the top of the reference's range, zq.rs:225): 4q no longer fits a word, so
 *                       every value is canonical between stages (three conditional subtractions per butterfly, ~33
 *                       instructions against 13 - 21) in the same two-pass / fused kernels: about 0.6 x the Shoup rate
 *   FHE_ARITH_MONTGOMERY q = 1 (mod 2^32), q < 2^61, n >= 16: transforms and Rq x Rq run word-Montgomery butterflies on
 *                       {w 2^32, w 2^64 mod q} — q^-1 = 1 (mod 2^32), so a word step needs no multiplication by it: 5
 *                       multiplies; only the inverse transform that multiplies two evaluation operands in its load keeps
 *                       SHOUP61's kernel (FHE_MG=0: everything does)
 * Results are the same words in every case.  Returns a negative FHE_E_* for a NULL plan. */
#define FHE_ARITH_SHOUP62 0
#define FHE_ARITH_SHOUP61 1
#define FHE_ARITH_PMERSENNE 2
#define FHE_ARITH_WORD32 3
#define FHE_ARITH_STRICT63 4
#define FHE_ARITH_MONTGOMERY 5
int fhe_ntt_plan_arithmetic(const fhe_ntt_plan *plan);

/* ---- transforms: host buffers ------------------------------------------- */
/* NTT::ntt(&Rq)->Rq, arith/src/ntt.rs:44-73: natural order in, bit-reversed
 * order out, canonical. */
int fhe_ntt_forward(const fhe_ntt_plan *plan, const uint64_t *in, uint64_t *out, size_t batch);
/* NTT::intt(&Rq)->Rq, arith/src/ntt.rs:78-110 (includes the n_inv scaling). */
int fhe_ntt_inverse(const fhe_ntt_plan *plan, const uint64_t *in, uint64_t *out, size_t batch);

/* Rq x Rq, arith/src/ring_nq.rs:564-607 (`mul`, `mul_mut`, the `Mul` impls
 * :490-503 and Rq::mul :294-296).
 *   a, b           operands, batch × n each.
 *   a_is_evals /   non-zero: that operand pointer already holds NTT-domain
 *   b_is_evals     values (the reference's cached `evals`, ring_nq.rs:590-599).
 *   c              product coefficients (required).
 *   c_evals        nullable: pointwise product in the NTT domain — the `evals`
 *                  the reference attaches to the product (ring_nq.rs:606).
 *   a_evals_out /  nullable: NTT(a), NTT(b) — what `mul_mut` stores back into
 *   b_evals_out    its operands (ring_nq.rs:568-573). */
int fhe_rq_mul(const fhe_ntt_plan *plan, const uint64_t *a, int a_is_evals, const uint64_t *b,
               int b_is_evals, uint64_t *c, uint64_t *c_evals, uint64_t *a_evals_out,
               uint64_t *b_evals_out, size_t batch);
/* same with two plans, as the reference compares `param` of both operands;
 * returns FHE_E_PARAM_MISMATCH unless they are the same (q,n). */
int fhe_rq_mul_checked(const fhe_ntt_plan *plan_a, const fhe_ntt_plan *plan_b, const uint64_t *a,
                       const uint64_t *b, uint64_t *c, uint64_t *c_evals, size_t batch);
/* zip_eq(l,r).map(l*r), arith/src/ring_nq.rs:601-604: c[i] = a[i]*b[i] mod q */
int fhe_rq_pointwise_mul(const fhe_ntt_plan *plan, const uint64_t *a, const uint64_t *b,
                         uint64_t *c, size_t batch);
/* FHE_OK, or FHE_E_NOT_CANONICAL if any of the batch*n values is >= q. */
int fhe_rq_check_canonical(const fhe_ntt_plan *plan, const uint64_t *x, size_t batch);
/* Opt-in validation: with FHE_NTT_CHECK_CANONICAL=1 in the environment, or after
 * fhe_ntt_set_check_canonical(1), fhe_ntt_forward/inverse, fhe_rq_mul and
 * fhe_rq_pointwise_mul (host and _dev forms) scan their coefficient inputs on the
 * device first and return FHE_E_NOT_CANONICAL for a value >= q instead of
 * undefined words (the reference cannot build such a Zq, zq.rs:21-30; a C caller
 * can).  The scan synchronises the stream: a debugging aid, off by default. */
int fhe_ntt_set_check_canonical(int on);

/* ---- transforms: device-resident buffers -------------------------------- */
int fhe_ntt_forward_dev(const fhe_ntt_plan *plan, const void *d_in, void *d_out, size_t batch,
                        void *hip_stream);
int fhe_ntt_inverse_dev(const fhe_ntt_plan *plan, const void *d_in, void *d_out, size_t batch,
                        void *hip_stream);
/* d_work: device scratch of fhe_rq_mul_workspace_bytes(plan,batch) bytes, or
 * NULL to use a library-owned grow-only workspace (not graph-capturable while
 * it grows). */
int fhe_rq_mul_dev(const fhe_ntt_plan *plan, const void *d_a, int a_is_evals, const void *d_b,
                   int b_is_evals, void *d_c, void *d_c_evals, void *d_a_evals_out,
                   void *d_b_evals_out, size_t batch, void *d_work, void *hip_stream);
size_t fhe_rq_mul_workspace_bytes(const fhe_ntt_plan *plan, size_t batch);
int fhe_rq_pointwise_mul_dev(const fhe_ntt_plan *plan, const void *d_a, const void *d_b, void *d_c,
                             size_t batch, void *hip_stream);
/* Synthetic coefficients: x[i] = mulhi64(splitmix64(seed ^
 * (first_index+i)), q), generated on the device. */
int fhe_fill_synthetic_dev(uint64_t q, uint64_t seed, uint64_t first_index, size_t count,
                           void *d_out, void *hip_stream);

/* ---- tuning / measurement ----------------------------------------------- */
/* Polynomials per launch for two-pass sizes (n >= 2^14): the batch can be
 * walked in tiles so that the intermediate of the first pass is still in the
 * 256 MiB Infinity Cache when the second pass reads it.  0 restores the default
 * (one launch per pass over the whole batch — measured fastest). */
int fhe_ntt_set_batch_tile(size_t polys);
/* (The one-launch forward transform of round 4 — persistent workgroups, slower than the two-pass kernels on every
 * setting measured — is NOT part of this boundary: its switches live in include/fhe_ntt_experimental.h.) */
/* When enabled, every kernel launch is bracketed by HIP events on its stream;
 * fhe_ntt_kernel_timing_read() synchronises, and returns per-kernel totals
 * since the last reset.  `names` receives up to `cap` NUL-terminated names of
 * at most 63 chars (64-byte slots), `total_ms`/`launches` the matching sums.
 * Returns the number of distinct kernels recorded (may exceed cap). */
int fhe_ntt_kernel_timing_enable(int on);
int fhe_ntt_kernel_timing_read(char *names, double *total_ms, uint64_t *launches, int cap);
int fhe_ntt_kernel_timing_reset(void);

/* ======================================================================== *
 * Next rows: the reference's SCHOOLBOOK callers either side
 * of the NTT path, rebuilt on the engine.  Products over Z are exact (K <= 3
 * CRT primes of 61 bits, chosen from the operand sizes) and only then reduced
 * mod 2^64, which is what the reference's `as i64` / `as u64` truncation keeps.
 * ======================================================================== */

/* arith::ring_n::naive_mul, arith/src/ring_n.rs:307-320: linear convolution of
 * two length-n coefficient vectors over Z, truncated `as i64`.  Operands are read
 * as NON-NEGATIVE 64-bit integers (Rq::to_r yields [0,q), ring_n.rs:72-79).
 * out: batch x 2n words (the 2n-1 results, then one 0).  a_bits/b_bits: bound on
 * the operands' bit length (0 = 64), used to pick the number of primes. */
int fhe_r_naive_mul(uint64_t n, const int64_t *a, const int64_t *b, int64_t *out, size_t batch);
int fhe_r_naive_mul_dev(uint64_t n, const void *d_a, const void *d_b, void *d_out, size_t batch,
                        unsigned a_bits, unsigned b_bits, void *hip_stream);

/* arith::ring_n::mul_div_round(q, n, v, num, den) -> Rq, arith/src/ring_n.rs:130-138:
 * z[i] = Zq::from_f64(((num as f64 * v[i] as f64) / den as f64).round())  (zq.rs:32-39),
 * then the X^n+1 fold of ring_nq.rs:132-141.  d_v: batch x 2n words read as i64
 * (layout of fhe_r_naive_mul_dev); d_out: batch x n words mod q.  IEEE f64, one
 * rounding per operation, round half away from zero — as the Rust. */
int fhe_mul_div_round_dev(uint64_t q, uint64_t n, const void *d_v, uint64_t num, uint64_t den,
                          void *d_out, size_t batch, void *hip_stream);

/* RLWE::tensor(t, a, b) -> (c0, c1, c2), bfv/src/lib.rs:59-85.
 * ab = [a0 | a1 | b0 | b1], each batch x n words mod q; c = [c0 | c1 | c2]. */
int fhe_bfv_tensor(uint64_t q, uint64_t n, uint64_t t, const uint64_t *ab, uint64_t *c, size_t batch);
int fhe_bfv_tensor_dev(uint64_t q, uint64_t n, uint64_t t, const void *d_ab, void *d_c, size_t batch,
                       void *hip_stream);
/* BFV::relinearize_204(rlk, c0, c1, c2) -> (c0 + r0, c1 + r1), bfv/src/lib.rs:251-271.
 * rlk = [rlk0 | rlk1], n words each mod pq (one key for the whole batch), p = pq / q;
 * c as produced by fhe_bfv_tensor_dev; out = [o0 | o1], each batch x n. */
int fhe_bfv_relinearize_dev(uint64_t q, uint64_t n, uint64_t pq, const void *d_rlk, const void *d_c,
                            void *d_out, size_t batch, void *hip_stream);
/* RLWE::mul(t, rlk, a, b) = relinearize_204(tensor(..)), bfv/src/lib.rs:87-90. */
int fhe_bfv_mul(uint64_t q, uint64_t n, uint64_t t, uint64_t pq, const uint64_t *rlk, const uint64_t *ab,
                uint64_t *out, size_t batch);
int fhe_bfv_mul_dev(uint64_t q, uint64_t n, uint64_t t, uint64_t pq, const void *d_rlk, const void *d_ab,
                    void *d_out, size_t batch, void *hip_stream);
/* Resident relinearisation key (RLWE::mul is called with the same `rlk` for every product of a computation,
 * bfv/src/lib.rs:87-90; relinearize_204 :251-271): rlk in the form the products consume — its transforms modulo three
 * 27-bit primes where the products stay below 2^82 (q = 65537, p = q^2, n <= 8192), else split in two halves and
 * transformed modulo one 61-bit prime where the half-products fit, reduced and transformed per CRT prime otherwise — built
 * once per key (fhe_bfv_rlk_prepared_words words; 0 = invalid parameters; the layout is opaque) and reused by every
 * later call; same words as the plain entry points produce. */
size_t fhe_bfv_rlk_prepared_words(uint64_t q, uint64_t n, uint64_t pq);
int fhe_bfv_rlk_prepare_dev(uint64_t q, uint64_t n, uint64_t pq, const void *d_rlk, void *d_prepared, void *hip_stream);
int fhe_bfv_relinearize_prepared_dev(uint64_t q, uint64_t n, uint64_t pq, const void *d_prepared, const void *d_c,
                                     void *d_out, size_t batch, void *hip_stream);
int fhe_bfv_mul_prepared_dev(uint64_t q, uint64_t n, uint64_t t, uint64_t pq, const void *d_prepared, const void *d_ab,
                             void *d_out, size_t batch, void *hip_stream);

/* Tn x Tn, arith/src/ring_torus.rs:251-298 (naive_poly_mul): negacyclic product of
 * coefficient vectors mod 2^64. */
int fhe_tn_mul(uint64_t n, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t batch);
int fhe_tn_mul_dev(uint64_t n, const void *d_a, const void *d_b, void *d_out, size_t batch,
                   void *hip_stream);

/* TGGSW x TGLWE external product, tfhe/src/tggsw.rs:45-62 with TGLev x Vec<Tn> (:139-149),
 * TGLWE x Tn (tglwe.rs:182-194) and Tn::decompose(beta = 2, l) (ring_torus.rs:67-77,
 * torus.rs:43-52; the reference hard-codes l = 64).
 *   tggsw [(k+1)][l][(k+1)][n]   TGLev i (i < k: the `a` rows; i = k: the `b` row), level d,
 *                                component c (c < k: mask a_c; c = k: body)   — one key
 *   tglwe [batch][(k+1)][n]      (a_0 .. a_{k-1}, b) per ciphertext;  out likewise. */
int fhe_tggsw_external_product(uint64_t n, unsigned k, unsigned l, const uint64_t *tggsw,
                               const uint64_t *tglwe, uint64_t *out, size_t batch);
int fhe_tggsw_external_product_dev(uint64_t n, unsigned k, unsigned l, const void *d_tggsw,
                                   const void *d_tglwe, void *d_out, size_t batch, void *hip_stream);
/* Resident key ("pre-transformed, reusable across the 630 products"): the TGGSW rows in
 * the layout the product consumes (32-bit halves, forward-transformed), built once and used by every
 * later call — the bootstrapping key of a blind rotation serves all its external products.
 *   fhe_tggsw_prepared_words   u64 words d_prepared must hold (0: this shape has no prepared form,
 *                              i.e. (k+1)*l*n > 2^26 or n outside [16, 2^13]: use the plain entry point)
 *   fhe_tggsw_prepare_dev      d_tggsw [(k+1)][l][(k+1)][n]  ->  d_prepared
 *   ..._prepared_dev           the external product against a prepared key; same words as
 *                              fhe_tggsw_external_product_dev on the original key. */
size_t fhe_tggsw_prepared_words(uint64_t n, unsigned k, unsigned l);
int fhe_tggsw_prepare_dev(uint64_t n, unsigned k, unsigned l, const void *d_tggsw, void *d_prepared, void *hip_stream);
int fhe_tggsw_external_product_prepared_dev(uint64_t n, unsigned k, unsigned l, const void *d_prepared,
                                            const void *d_tglwe, void *d_out, size_t batch, void *hip_stream);

/* TGLWE x Tn (plaintext product), tfhe/src/tglwe.rs:182-194: out[b][i] = tglwe[b][i] * p[b] mod
 * (2^64, X^n+1), i <= k.  tglwe, out: [batch][(k+1)][n]; p: [batch][n]. */
int fhe_tglwe_mul_tn(uint64_t n, unsigned k, const uint64_t *tglwe, const uint64_t *p, uint64_t *out, size_t batch);
int fhe_tglwe_mul_tn_dev(uint64_t n, unsigned k, const void *d_tglwe, const void *d_p, void *d_out,
                         size_t batch, void *hip_stream);
/* TGLev x Vec<Tn> -> TGLWE, tfhe/src/tggsw.rs:139-149: out[b] = sum_{d<l} tglev[d] * v[b][d].
 * tglev: [l][(k+1)][n] (one for the batch); v: [batch][l][n] (any 64-bit words, e.g. a decomposition);
 * out: [batch][(k+1)][n]. */
int fhe_tglev_mul(uint64_t n, unsigned k, unsigned l, const uint64_t *tglev, const uint64_t *v, uint64_t *out,
                  size_t batch);
int fhe_tglev_mul_dev(uint64_t n, unsigned k, unsigned l, const void *d_tglev, const void *d_v, void *d_out,
                      size_t batch, void *hip_stream);

/* ---- TFHE bootstrapping (tfhe/src/tlwe.rs:101-161, tglwe.rs:89-118; definitions in DESIGN.md §10) ----
 * N = n = 2^L, k = GLWE rank, every word u64 wrapping mod 2^64.  A TLWE of dimension m is [a_0 .. a_{m-1}, b]
 * (m + 1 words); a TGLWE is [(k+1)][n] as above.  Output buffers must not overlap the inputs.
 *   fhe_tfhe_bsk_prepared_words  u64 words a prepared bootstrapping key holds: n_lwe x fhe_tggsw_prepared_words
 *                                (0: no prepared form for this shape)
 *   fhe_tfhe_bsk_prepare_dev     d_bsk [n_lwe][(k+1)][l][(k+1)][n] (TGGSW j encrypts LWE key bit j) -> d_prepared;
 *                                key j's prepared form is what fhe_tggsw_prepare_dev makes of TGGSW j, at word
 *                                offset j * fhe_tggsw_prepared_words
 *   fhe_tfhe_blind_rotation_dev  d_lwe [batch][n_lwe + 1], d_table [(k+1)][n] (the test vector v, one for the batch)
 *                                -> d_out [batch][(k+1)][n]: with a~ = round(a 2N / 2^64) mod 2N (rounding, not the
 *                                reference's floor to kN), ACC = X^{-b~} v, then for every j
 *                                ACC += BSK_j [x] (X^{a~_j} ACC - ACC)  (cmux, tggsw.rs:39-41; [x] as
 *                                fhe_tggsw_external_product_prepared_dev).  Decrypts to X^{-phi~} v.
 *   fhe_tglwe_sample_extraction_dev  d_tglwe [batch][(k+1)][n] -> d_tlwe [batch][k n + 1], coefficient h < n
 *                                (tglwe.rs:89-115)
 *   fhe_tlwe_key_switch_dev      d_in [batch][n_in + 1], d_ksk [n_in][l][n_out + 1] (TLev of input key bit i under the
 *                                output key) -> d_out [batch][n_out + 1] = (0 .. 0, b) - sum_i sum_{d<l} bit_{l-1-d}(a_i)
 *                                ksk[i][d] (tlwe.rs:101-111); beta = 2 only, 1 <= l <= 64
 *   fhe_tfhe_bootstrap_dev       blind rotation -> sample extraction (h = 0) -> key switch (n_in = k n, n_out = n_lwe,
 *                                ks_l levels): d_in, d_out [batch][n_lwe + 1] (tlwe.rs:150-161) */
size_t fhe_tfhe_bsk_prepared_words(uint64_t n, unsigned k, unsigned l, unsigned n_lwe);
int fhe_tfhe_bsk_prepare_dev(uint64_t n, unsigned k, unsigned l, unsigned n_lwe, const void *d_bsk, void *d_prepared,
                             void *hip_stream);
int fhe_tfhe_blind_rotation_dev(uint64_t n, unsigned k, unsigned l, unsigned n_lwe, const void *d_bsk_prepared,
                                const void *d_table, const void *d_lwe, void *d_out, size_t batch, void *hip_stream);
int fhe_tglwe_sample_extraction_dev(uint64_t n, unsigned k, unsigned h, const void *d_tglwe, void *d_tlwe, size_t batch,
                                    void *hip_stream);
int fhe_tlwe_key_switch_dev(unsigned n_in, unsigned n_out, unsigned beta, unsigned l, const void *d_ksk,
                            const void *d_in, void *d_out, size_t batch, void *hip_stream);
int fhe_tfhe_bootstrap_dev(uint64_t n, unsigned k, unsigned l, unsigned n_lwe, const void *d_bsk_prepared,
                           const void *d_table, unsigned ks_l, const void *d_ksk, const void *d_in, void *d_out,
                           size_t batch, void *hip_stream);

/* ---- TFHE with the signed base-2^b gadget (definitions in DESIGN.md §11) ----
 * b = log_beta, l levels, 1 <= b, b l <= 64, s = 64 - b l.  Level d (0 = most significant) has gadget value
 * g_d = 2^(64 - b(d+1)); digit_d(w) in [-2^(b-1), 2^(b-1)) and sum_d digit_d(w) g_d = w rounded half up to its top
 * b l bits (mod 2^64).  Keys use the layouts of the beta = 2 twins, with level d encrypting m g_d.  The products take
 * k = 1, 256 <= n <= 4096 and (k+1) l n (2^32 - 1) 2^(b-1) < pA pB / 2 (fhe_tggsw_gadget_prepared_words is 0
 * otherwise): at n = 1024, b <= 10 for l = 2 and 3.  The key switch takes 1 <= b <= 32.  Outputs must not overlap inputs.
 *   fhe_tn_gadget_decompose_dev      d_a [rows][n] -> d_out [rows][l][n]: the signed digits as int64 words
 *   fhe_tggsw_gadget_prepared_words  u64 words of a prepared gadget TGGSW (always the two-prime layout; 0: not admitted)
 *   fhe_tggsw_gadget_prepare_dev     d_tggsw [(k+1)][l][(k+1)][n] -> d_prepared
 *   fhe_tggsw_gadget_external_product_dev  d_tglwe [batch][(k+1)][n] -> d_out [batch][(k+1)][n] =
 *                                    sum_i sum_d digit_d(tglwe_i) TGGSW[i][d]  in T64[X]/(X^n+1)
 *   fhe_tfhe_gadget_bsk_prepared_words / fhe_tfhe_gadget_bsk_prepare_dev  n_lwe gadget TGGSWs side by side
 *   fhe_tfhe_gadget_blind_rotation_dev  as fhe_tfhe_blind_rotation_dev with the gadget product
 *   fhe_tlwe_gadget_key_switch_dev   d_ksk [n_in][l][n_out + 1] (level d: TLev of s_in[i] g_d) -> d_out [batch][n_out + 1]
 *                                    = (0 .. 0, b) - sum_i sum_d digit_d(a_i) ksk[i][d]
 *   fhe_tfhe_gadget_bootstrap_dev    gadget blind rotation -> sample extraction (h = 0) -> gadget key switch
 *                                    (ks_log_beta, ks_l) from dimension k n back to n_lwe */
int fhe_tn_gadget_decompose_dev(uint64_t n, unsigned log_beta, unsigned l, const void *d_a, void *d_out, size_t rows,
                                void *hip_stream);
size_t fhe_tggsw_gadget_prepared_words(uint64_t n, unsigned k, unsigned log_beta, unsigned l);
int fhe_tggsw_gadget_prepare_dev(uint64_t n, unsigned k, unsigned log_beta, unsigned l, const void *d_tggsw,
                                 void *d_prepared, void *hip_stream);
int fhe_tggsw_gadget_external_product_dev(uint64_t n, unsigned k, unsigned log_beta, unsigned l, const void *d_prepared,
                                          const void *d_tglwe, void *d_out, size_t batch, void *hip_stream);
size_t fhe_tfhe_gadget_bsk_prepared_words(uint64_t n, unsigned k, unsigned log_beta, unsigned l, unsigned n_lwe);
int fhe_tfhe_gadget_bsk_prepare_dev(uint64_t n, unsigned k, unsigned log_beta, unsigned l, unsigned n_lwe,
                                    const void *d_bsk, void *d_prepared, void *hip_stream);
int fhe_tfhe_gadget_blind_rotation_dev(uint64_t n, unsigned k, unsigned log_beta, unsigned l, unsigned n_lwe,
                                       const void *d_bsk_prepared, const void *d_table, const void *d_lwe, void *d_out,
                                       size_t batch, void *hip_stream);
int fhe_tlwe_gadget_key_switch_dev(unsigned n_in, unsigned n_out, unsigned log_beta, unsigned l, const void *d_ksk,
                                   const void *d_in, void *d_out, size_t batch, void *hip_stream);
int fhe_tfhe_gadget_bootstrap_dev(uint64_t n, unsigned k, unsigned log_beta, unsigned l, unsigned n_lwe,
                                  const void *d_bsk_prepared, const void *d_table, unsigned ks_log_beta, unsigned ks_l,
                                  const void *d_ksk, const void *d_in, void *d_out, size_t batch, void *hip_stream);

/* ---- TFHE circuit bootstrapping and a CMux with a selector per ciphertext (definitions in DESIGN.md §12) ----
 * k = 1, 256 <= n <= 4096; K = the extracted LWE key of the GLWE key s (dimension k n), g_d(b) = 2^(64 - b(d+1)) and
 * digit_d are §11's.  Outputs must not overlap inputs.
 *   fhe_tfhe_pfksk_words            u64 words of a private functional key switching key [(k+1)][k n + 1][l][(k+1)][n]
 *                                   (1 <= b <= 32, b l <= 64; 0 otherwise).  Function r < k is x -> -s_r x, function k
 *                                   x -> x; entry [r][j][d] is a TGLWE under s of f_r(K~_j) g_d, K~ = (-K_0 .. -K_{kn-1}, 1)
 *   fhe_tlwe_gadget_private_key_switch_dev  d_in [batch][k n + 1] -> d_out [batch][(k+1)][(k+1)][n]:
 *                                   out_r = sum_{j <= kn} sum_d digit_d(c_j) pfksk[r][j][d], c_kn the body (wrapping u64)
 *   fhe_tggsw_gadget_prepare_many_dev  `count` gadget TGGSWs [count][(k+1)][l][(k+1)][n] -> count prepared ones side by
 *                                   side (count * fhe_tggsw_gadget_prepared_words)
 *   fhe_tggsw_gadget_cmux_dev       out_j = c0_j + C[idx_j] [x] (c1_j - c0_j): d_prepared holds `count` prepared TGGSWs,
 *                                   d_idx [batch] u32; an idx_j >= count selects nothing (out_j = c0_j).  c0, c1, out:
 *                                   [batch][(k+1)][n]
 *   fhe_tfhe_circuit_bootstrap_dev  d_lwe [batch][n_lwe + 1], phase mu 2^63 + e (mu in {0, 1}) -> d_out
 *                                   [batch][(k+1)][cb_l][(k+1)][n]: raw gadget TGGSWs of mu with (cb_log_beta, cb_l), for
 *                                   fhe_tggsw_gadget_prepare(_many)_dev.  BSK (log_beta, l) and (cb_log_beta, cb_l) must be
 *                                   admitted by fhe_tggsw_gadget_prepared_words, cb_log_beta cb_l <= 63; PFKSK
 *                                   (pf_log_beta, pf_l) as fhe_tfhe_pfksk_words */
size_t fhe_tfhe_pfksk_words(uint64_t n, unsigned k, unsigned log_beta, unsigned l);
int fhe_tlwe_gadget_private_key_switch_dev(uint64_t n, unsigned k, unsigned log_beta, unsigned l, const void *d_pfksk,
                                           const void *d_in, void *d_out, size_t batch, void *hip_stream);
int fhe_tggsw_gadget_prepare_many_dev(uint64_t n, unsigned k, unsigned log_beta, unsigned l, size_t count,
                                      const void *d_tggsw, void *d_prepared, void *hip_stream);
int fhe_tggsw_gadget_cmux_dev(uint64_t n, unsigned k, unsigned log_beta, unsigned l, size_t count, const void *d_prepared,
                              const void *d_idx, const void *d_c0, const void *d_c1, void *d_out, size_t batch,
                              void *hip_stream);
int fhe_tfhe_circuit_bootstrap_dev(uint64_t n, unsigned k, unsigned log_beta, unsigned l, unsigned n_lwe,
                                   const void *d_bsk_prepared, unsigned cb_log_beta, unsigned cb_l, unsigned pf_log_beta,
                                   unsigned pf_l, const void *d_pfksk, const void *d_lwe, void *d_out, size_t batch,
                                   void *hip_stream);

/* ---- TFHE boolean gates with gate bootstrapping (definitions in DESIGN.md §13) ----
 * The gadget shapes of fhe_tfhe_gadget_bootstrap_dev: BSK (log_beta, l) admitted by fhe_tggsw_gadget_prepared_words,
 * KSK (ks_log_beta, ks_l) as fhe_tlwe_gadget_key_switch_dev.  A bit is a TLWE of dimension n_lwe with phase +mu (1) or
 * -mu (0), mu = 2^61; outputs are again bits under the same LWE key.  d_pool [wires][n_lwe + 1] holds the inputs.
 *   fhe_tfhe_gate_bootstrap_dev  d_gates [batch][3] u32 (op, a, b), ops FHE_GATE_* mixed freely -> d_out [batch][n_lwe + 1]:
 *                                bootstrap (0 .. 0, o) + alpha c_a + beta c_b (wrapping u64) with the test vector
 *                                (mask 0, body mu), extract at 0, key switch
 *   fhe_tfhe_gate_mux_dev        d_sel [batch][3] u32 (s, a, b) -> d_out [batch][n_lwe + 1] = s ? a : b: blind rotations of
 *                                AND(s, a) and ANDNY(s, b), both extracted at 0, added, + mu on the body, one key switch
 * A row whose op is >= FHE_GATE_COUNT, or whose indices are not all < wires, combines as all-zero inputs with o = 0 (and
 * reads no pool word); for a MUX the rule holds per blind rotation: AND(s, a) and ANDNY(s, b).  d_out may lie inside the
 * pool but must not overlap a row that the descriptors read. */
#define FHE_GATE_AND 0   /* (alpha, beta, o) = ( 1,  1, -mu) */
#define FHE_GATE_NAND 1  /*                   (-1, -1, +mu) */
#define FHE_GATE_OR 2    /*                   ( 1,  1, +mu) */
#define FHE_GATE_NOR 3   /*                   (-1, -1, -mu) */
#define FHE_GATE_XOR 4   /*                   ( 2,  2, +2mu) */
#define FHE_GATE_XNOR 5  /*                   (-2, -2, -2mu) */
#define FHE_GATE_ANDNY 6 /* !a & b            (-1,  1, -mu) */
#define FHE_GATE_ANDYN 7 /* a & !b            ( 1, -1, -mu) */
#define FHE_GATE_ORNY 8  /* !a | b            (-1,  1, +mu) */
#define FHE_GATE_ORYN 9  /* a | !b            ( 1, -1, +mu) */
#define FHE_GATE_COUNT 10
int fhe_tfhe_gate_bootstrap_dev(uint64_t n, unsigned k, unsigned log_beta, unsigned l, unsigned n_lwe,
                                const void *d_bsk_prepared, unsigned ks_log_beta, unsigned ks_l, const void *d_ksk,
                                const void *d_pool, size_t wires, const void *d_gates, void *d_out, size_t batch,
                                void *hip_stream);
int fhe_tfhe_gate_mux_dev(uint64_t n, unsigned k, unsigned log_beta, unsigned l, unsigned n_lwe,
                          const void *d_bsk_prepared, unsigned ks_log_beta, unsigned ks_l, const void *d_ksk,
                          const void *d_pool, size_t wires, const void *d_sel, void *d_out, size_t batch, void *hip_stream);

/* ---- TFHE small integers: a lookup table per row in one bootstrap (definitions in DESIGN.md §14) ----
 * The gadget shapes of the gates above (k = 1, 2^8 <= n = 2^L <= 2^12; anything else is FHE_E_INVALID).  t = t_bits,
 * 1 <= t <= L, P = 2^t, Delta = 2^(63 - t): a value x in [0, P) is a TLWE of phase x Delta + e; the top bit is padding, 0.
 *   d_luts [lut_count][P] u64 torus words (not values: an output may use any encoding).  Table T stands for the test vector
 *          (mask 0, body v), v[i] = T[m] for m = (i + half) >> (L - t) < P and 0 - T[0] otherwise, half = N / 2P (0 at
 *          P = N); it is never written out.  A phase within half a box of x Delta gives T[x]; a row whose padding bit is set
 *          gives 0 - T[x - P] (negacyclic).
 *   d_desc [batch][6] u32 (lut, x, y, sx, sy, o_hi), sx and sy read as int32: the combined input of a row is
 *          c = sx pool[x] + sy pool[y] + (0 .. 0, o_hi 2^32) (wrapping u64; Delta >= 2^51, so any multiple of Delta is an
 *          o_hi).  An operand whose scale is 0 is never read and its index may be anything (FHE_LUT_NONE by convention).
 *          A row is invalid if an operand with a non-zero scale has an index >= wires, or, in the bootstrap only, if
 *          lut >= lut_count: it reads no pool or table word and its output row is all-zero words.
 *   fhe_tlwe_lincomb_dev        d_out [batch][n_lwe + 1] = c of each row; the lut word is ignored; no bootstrap
 *   fhe_tfhe_lut_bootstrap_dev  d_out [batch][n_lwe + 1]: combine, mod switch, ACC_0 = rot(v_lut, b~), the n_lwe CMux steps,
 *                               extraction at 0, key switch: 2 n_lwe + 3 launches whatever the mix of tables
 * batch, wires and lut_count must be at least 1.  d_out may lie inside the pool but must not overlap a row that the
 * descriptors read. */
#define FHE_LUT_NONE 0xFFFFFFFFu
int fhe_tlwe_lincomb_dev(unsigned n_lwe, const void *d_pool, size_t wires, const void *d_desc, void *d_out, size_t batch,
                         void *hip_stream);
int fhe_tfhe_lut_bootstrap_dev(uint64_t n, unsigned k, unsigned log_beta, unsigned l, unsigned n_lwe,
                               const void *d_bsk_prepared, unsigned ks_log_beta, unsigned ks_l, const void *d_ksk,
                               unsigned t_bits, const void *d_luts, size_t lut_count, const void *d_pool, size_t wires,
                               const void *d_desc, void *d_out, size_t batch, void *hip_stream);

/* ---- TFHE small integers: several lookup tables from one blind rotation (definitions in DESIGN.md §15) ----
 * The many-output bootstrap of Chillotti, Ligier, Orfila and Tap (ePrint 2021/729, "PBSmanyLUT") on the shapes, keys,
 * encoding and descriptors of fhe_tfhe_lut_bootstrap_dev above.  nu: 0 <= nu <= min(L - t_bits, 4), F = 2^nu.
 *   mod switch  ms_nu(w) = ((((w >> (62 - L + nu)) + 1) >> 1) << nu) & (2N - 1): rounding to a multiple of F in Z_2N, applied
 *          to the body and to every mask word of the combined input (ms_0 is the mod switch of every other call), so each
 *          unit of nu costs one bit of mod-switch precision.
 *   d_luts [lut_count][P]: a row's lut word names the first of F consecutive tables T_0 .. T_{F-1}.  The test vector
 *          interleaves them: for i < N, h = i mod F, q = (i - h + half) >> (L - t), v[i] = T_h[q] if q < P, else 0 - T_h[0]
 *          (q = P never occurs at nu = L - t); it is never written out.  After the one blind rotation coefficient h holds
 *          T_h[x] for phases within half a box of x Delta, and 0 - T_h[x - P] with the padding bit set.
 *   d_desc as above.  A row is invalid under the operand rule above or if lut + F > lut_count (in 64 bits): it reads no
 *          pool or table word and all F of its output rows are all-zero words.
 *   d_out  [F][batch][n_lwe + 1], function-major: function h of row m is row h batch + m.
 * Combine, ms_nu, ACC_0 = rot(v, b~), the n_lwe CMux steps, extraction of coefficients 0 .. F - 1 in one launch, one key
 * switch over the F batch rows: 2 n_lwe + 3 launches whatever nu is.  With nu = 0 every output word is
 * fhe_tfhe_lut_bootstrap_dev's.  d_out (all F batch rows) must not overlap a key, the tables or the descriptors
 * (FHE_E_INVALID); it may lie inside the pool but must not overlap a row that the descriptors read. */
int fhe_tfhe_lut_many_bootstrap_dev(uint64_t n, unsigned k, unsigned log_beta, unsigned l, unsigned n_lwe,
                                    const void *d_bsk_prepared, unsigned ks_log_beta, unsigned ks_l, const void *d_ksk,
                                    unsigned t_bits, unsigned nu, const void *d_luts, size_t lut_count, const void *d_pool,
                                    size_t wires, const void *d_desc, void *d_out, size_t batch, void *hip_stream);

/* ---- TFHE packing key switch and a bootstrap with a test vector per row (definitions in DESIGN.md §16) ----
 * The pieces of the tree-based functional bootstrap of Guimaraes, Borin and Aranha (TCHES 2021/2): LWE results of one
 * lookup are packed into a TGLWE (the public functional key switch of Chillotti et al., J. Cryptology 2020), which a
 * second blind rotation reads as its test vector.  k = 1, 2^8 <= n = 2^L <= 2^12, u64 wrapping words, digit_d, g_d and
 * gadget_cadd are §11's; anything else is FHE_E_INVALID.  Outputs must not overlap inputs.
 *   fhe_tfhe_pksk_words   u64 words of a packing key switching key [n_in][l][(k+1)][n] (n_in >= 1, 1 <= b <= 32,
 *          b l <= 64; 0 otherwise).  Entry [j][d] is a TGLWE under s of the constant polynomial K_in[j] g_d(b), K_in the
 *          key of the input TLWEs.
 *   fhe_tlwe_gadget_packing_key_switch_dev   KS(c) = (0, b X^0) - sum_j sum_d digit_d(a_j) pksk[j][d] for c = (a, b); a
 *          group packs `count` ciphertexts at stride = 2^log_stride (count >= 1, count stride <= n):
 *          out_g = sum_{i < count} X^(i stride) KS(c_{g,i}) in T64[X]/(X^n + 1), d_out [groups][(k+1)][n].  Ciphertext i
 *          of group g starts at word g in_group_stride + i in_item_stride of d_in; both strides are at least n_in + 1
 *          and the addressed rows must not alias.  A contiguous [groups][count][n_in + 1] block has strides
 *          (count (n_in + 1), n_in + 1); fhe_tfhe_lut_many_bootstrap_dev's [F][batch][n_lwe + 1] has (n_lwe + 1,
 *          batch (n_lwe + 1)).  Only d_in itself need be 16-byte aligned.  groups = 0 is FHE_E_INVALID.
 *   fhe_tglwe_box_expand_dev   1 <= t_bits <= L, box = n >> t_bits, half = box / 2: every component row becomes
 *          X^(-half) (1 + X + .. + X^(box-1)) times itself, out[i] = sum_{u < box} in~[i + half - u] with in~ the negacyclic
 *          extension.  A packed TGLWE holding m_q at coefficient q box becomes §14's test vector of the table q -> m_q;
 *          t_bits = L copies.  d_in, d_out [batch][(k+1)][n].
 *   fhe_tfhe_gadget_bootstrap_rows_dev   fhe_tfhe_gadget_bootstrap_dev with a test vector per row: d_tables
 *          [batch][(k+1)][n] holds full TGLWEs (mask rows included) and row b of d_in rotates row b of d_tables over all
 *          k + 1 components; then the n_lwe CMux steps, extraction at 0 and the gadget key switch: 2 n_lwe + 3 launches. */
size_t fhe_tfhe_pksk_words(uint64_t n, unsigned k, unsigned n_in, unsigned log_beta, unsigned l);
int fhe_tlwe_gadget_packing_key_switch_dev(uint64_t n, unsigned k, unsigned n_in, unsigned log_beta, unsigned l,
                                           const void *d_pksk, const void *d_in, size_t in_group_stride,
                                           size_t in_item_stride, size_t count, unsigned log_stride, void *d_out,
                                           size_t groups, void *hip_stream);
int fhe_tglwe_box_expand_dev(uint64_t n, unsigned k, unsigned t_bits, const void *d_in, void *d_out, size_t batch,
                             void *hip_stream);
int fhe_tfhe_gadget_bootstrap_rows_dev(uint64_t n, unsigned k, unsigned log_beta, unsigned l, unsigned n_lwe,
                                       const void *d_bsk_prepared, const void *d_tables, unsigned ks_log_beta,
                                       unsigned ks_l, const void *d_ksk, const void *d_in, void *d_out, size_t batch,
                                       void *hip_stream);

/* ---- TFHE key generation, encryption and decryption: the client side (definitions in DESIGN.md §17) ----
 * Exact and independent of launch geometry; u64 wrapping words.  `seed` is a HOST pointer to 32 bytes, the ChaCha20 key
 * (RFC 8439: 32-bit block counter, 96-bit nonce, 20 rounds); it is the whole secret.  A row (one LWE sample, one TGLWE
 * sample, one secret key) has the nonce (purpose, row index lo, row index hi); block c of a row (counter c, from 0) gives
 * 8 stream words, word j = output u32 word 2j | output u32 word 2j + 1 << 32; stream word i is word i mod 8 of block
 * i div 8.  Mask word i of a row is FHE_STREAM_MASK word i, secret-key bit i is FHE_STREAM_KEY word i AND 1, error sample i
 * is drawn from FHE_STREAM_ERR word i.  Two samples of one seed must never share a row index.
 *   errors   d_cdt [m] strictly increasing thresholds below 2^63, m <= 1024 (m = 0: no error, d_cdt may be NULL).  For a
 *            stream word u, r = u >> 1: the magnitude is the number of i with cdt[i] <= r, negative when u AND 1; the
 *            error word is the signed value << log_scale (0 <= log_scale <= 63), wrapping.  The table is checked on a host
 *            copy in every call that takes one, which synchronises hip_stream.
 *   keys     d_key holds 0/1 words; only bit 0 of a word is read.
 *   fhe_tfhe_stream_words_dev  d_out [rows][row_words] = stream words 0 .. row_words - 1 of rows first_row .. of `purpose`
 *            (1 <= row_words <= 2^35, i.e. at most 2^32 blocks); FHE_STREAM_BITS: every word AND 1 (a secret key)
 *   fhe_tlwe_encrypt_dev       d_out [batch][n + 1], row r = [a_0 .. a_{n-1}, b] with a = the mask words of row first_row + r
 *            and b = sum a_i s_i + d_mu[r] + e (d_mu NULL: 0), e from error sample 0 of the row; any n >= 1; one fused
 *            kernel.
 *   fhe_tlwe_phase_dev         d_out [batch] = b - sum a_i s_i of d_in [batch][n + 1]
 *   fhe_tglwe_encrypt_dev      k = 1, 2^8 <= n = 2^L <= 2^12.  d_out [rows][(k+1)][n], row r = (A, A S + M_r + E) in
 *            T64[X]/(X^n + 1) with A the n mask words and E the n error samples of row first_row + r; M_r = d_msg +
 *            r msg_stride (msg_stride = 0: one message for every row, otherwise >= n; d_msg NULL: M = 0)
 *   fhe_tglwe_phase_dev        d_out [rows][n] = B - A S of d_in [rows][(k+1)][n]
 * Every device buffer of these five entry points needs 8-byte alignment and nothing more (LWE rows hold n + 1 words, and a
 * msg_stride may be odd).  Anything outside these ranges, first_row + rows past 2^64, and an output that overlaps the key,
 * the messages or the table is FHE_E_INVALID and writes nothing; batch (rows) = 0 is a no-op. */
#define FHE_STREAM_MASK 1u
#define FHE_STREAM_ERR 2u
#define FHE_STREAM_KEY 3u
#define FHE_STREAM_BITS 1u /* flag of fhe_tfhe_stream_words_dev */
int fhe_tfhe_stream_words_dev(const uint8_t *seed, unsigned purpose, uint64_t first_row, uint64_t row_words, unsigned flags,
                              void *d_out, size_t rows, void *hip_stream);
int fhe_tlwe_encrypt_dev(unsigned n, const uint8_t *seed, uint64_t first_row, const void *d_key, const void *d_mu,
                         const void *d_cdt, unsigned m, unsigned log_scale, void *d_out, size_t batch, void *hip_stream);
int fhe_tlwe_phase_dev(unsigned n, const void *d_key, const void *d_in, void *d_out, size_t batch, void *hip_stream);
int fhe_tglwe_encrypt_dev(uint64_t n, unsigned k, const uint8_t *seed, uint64_t first_row, const void *d_key,
                          const void *d_msg, size_t msg_stride, const void *d_cdt, unsigned m, unsigned log_scale,
                          void *d_out, size_t rows, void *hip_stream);
int fhe_tglwe_phase_dev(uint64_t n, unsigned k, const void *d_key, const void *d_in, void *d_out, size_t rows,
                        void *hip_stream);

/* ---- BFV key generation, encryption and decryption: the client side (bfv/src/lib.rs:118-225) ----
 * Exact and independent of launch geometry.  The stream is the one above, unchanged (`seed`: a HOST pointer to 32 bytes, the
 * whole secret), under four purposes of its own, so no BFV row shares a nonce with a TFHE row (fhe_tfhe_stream_words_dev
 * does not serve them): FHE_STREAM_BFV_MASK, _ERR, _KEY, _EPH.  A row is one polynomial.
 *   uniform  coefficient i modulo Q (Q = q or pq < 2^63) from MASK words w0 = 2i, w1 = 2i + 1 of the row:
 *            floor((w1 2^64 + w0) Q / 2^128); no rejection, bias below 2^-65
 *   secret   s_i = KEY word i AND 1; where a key is read, only bit 0 of a word counts
 *   u        EPH word w of coefficient i: (w AND 1) - ((w >> 1) AND 1), as the residue 0, 1 or q - 1
 *   errors   the table-inversion sampler above at log_scale 0 (d_cdt [m], m <= 1024), as the residue e or Q - |e|: a discrete
 *            Gaussian, not the reference's rounded Normal(0, 3.2).  Encryption row r takes e1 from ERR row 2r and e2 from ERR
 *            row 2r + 1, key row r takes e from ERR row 2r, so row indices stay below 2^63.  The table is checked on a host
 *            copy (synchronises hip_stream), and its largest magnitude m must be below the modulus.
 *   fhe_bfv_secret_key_dev   d_s [n] = the 0/1 words of KEY row key_row
 *   fhe_bfv_public_key_dev   d_pk = [pk0 | pk1] = (-a s + e, a) mod q, n words each; a = the uniform MASK row `row`
 *   fhe_bfv_relin_key_dev    d_rlk = [rlk0 | rlk1] = (-(a s + e) + p s^2, a) mod pq, p = pq / q, in the layout of
 *            fhe_bfv_relinearize_dev / fhe_bfv_rlk_prepare_dev.  EXACT: the reference routes a s and s^2 through f64
 *            (tmp_naive_mul -> from_vec_i64), exact while a coefficient of the integer product stays below 2^53; these are the
 *            reference's words wherever that route is exact.  Needs pq a multiple of q and n pq < 2^63.
 *   fhe_bfv_encrypt_dev      d_out = [c0 | c1], each batch x n: row r is encryption row first_row + r, c0 = pk0 u + e1 +
 *            floor(q / t) (m_r mod q), c1 = pk1 u + e2.  d_pk_evals [2][n] = fhe_ntt_forward_dev of d_pk, made once per key.
 *            m_r = d_msg + r msg_stride (msg_stride = 0: one message for every row, otherwise >= n; d_msg NULL: m = 0).
 *   fhe_bfv_decrypt_dev      d_out [batch][n] = (round(t (c0 + c1 s mod q) / q) mod q) mod t with the f64 steps of
 *            fhe_rq_mul_div_round_dev; d_s_evals [n] = fhe_ntt_forward_dev of the secret; d_ct = [c0 | c1]
 * Device buffers need 8-byte alignment.  t < 2 or t >= q, m > 1024 or a table §17 rejects or whose magnitudes reach the
 * modulus, first_row + rows past 2^63, n pq >= 2^63 or pq not a multiple of q, an output that overlaps an input and extents
 * past 2^60 words are FHE_E_INVALID and write nothing; batch = 0 is a no-op.  A plan fixes (q, n). */
#define FHE_STREAM_BFV_MASK 0x11u
#define FHE_STREAM_BFV_ERR 0x12u
#define FHE_STREAM_BFV_KEY 0x13u
#define FHE_STREAM_BFV_EPH 0x14u
int fhe_bfv_secret_key_dev(uint64_t n, const uint8_t *seed, uint64_t key_row, void *d_s, void *hip_stream);
int fhe_bfv_public_key_dev(const fhe_ntt_plan *plan, const uint8_t *seed, uint64_t row, const void *d_s, const void *d_cdt,
                           unsigned m, void *d_pk, void *hip_stream);
int fhe_bfv_relin_key_dev(uint64_t q, uint64_t n, uint64_t pq, const uint8_t *seed, uint64_t row, const void *d_s,
                          const void *d_cdt, unsigned m, void *d_rlk, void *hip_stream);
int fhe_bfv_encrypt_dev(const fhe_ntt_plan *plan, uint64_t t, const uint8_t *seed, uint64_t first_row,
                        const void *d_pk_evals, const void *d_msg, size_t msg_stride, const void *d_cdt, unsigned m,
                        void *d_out, size_t batch, void *hip_stream);
int fhe_bfv_decrypt_dev(const fhe_ntt_plan *plan, uint64_t t, const void *d_s_evals, const void *d_ct, void *d_out,
                        size_t batch, void *hip_stream);

/* ---- CKKS: the encoder, key generation, encryption and decryption (ckks/src/encoder.rs, ckks/src/lib.rs:46-118;
 * DESIGN.md §21) ----
 * The embedding: w = exp(i pi / n); slot i of n/2 is the value of the polynomial at w^(2i+1), i < n/2 (the reference's
 * order, not the 5^j order); the conjugate slots n-1-i are never stored.  Complex values are interleaved double pairs.
 *   fhe_ckks_twiddles    HOST only, needs no device: out [n] pairs (cos, sin)(pi k / n), k < n, each within 1 ulp (long
 *            double, arguments reduced to [0, pi/4]).  The caller uploads the table and passes it as d_tw.
 *   fhe_ckks_encode_dev  d_out [batch][n] signed 64-bit words: coefficient j = f64_as_i64(round(a_j)), round half away from
 *            zero, a_j = (1/n) Re(w^-j sum_i h_i w^(-2ij)) over the Hermitian extension h of delta z as the device's f64
 *            transform computes it (error bound in §21; not bit-compatible with the reference's MKL solve).  Row r of d_z
 *            starts at complex value r z_stride (z_stride = 0: one vector for every row, otherwise >= n/2).
 *   fhe_ckks_decode_dev  d_out [batch][n/2] complex: z_i = (1/delta) sum_j p_j w^((2i+1) j), d_p [batch][n] signed words
 *            converted to f64 first.
 * The encoder takes 2 <= n <= 2^13 (one workgroup's LDS holds a polynomial) and a finite, positive delta.
 * The scheme runs on the stream above under FHE_STREAM_CKKS_MASK, _ERR, _KEY, _EPH (fhe_tfhe_stream_words_dev does not
 * serve them); a row is one polynomial; samples, row numbering and the error table are those of the BFV block, except:
 *   secret   ternary: s_i = (w AND 1) - ((w >> 1) AND 1) of KEY word i, as the residue 0, 1 or q - 1; the ephemeral v the
 *            same on EPH words
 *   mask     uniform modulo q (the reference draws it from the secret's distribution, which hides nothing: not followed)
 *   fhe_ckks_secret_key_dev  d_s [n] residues 0, 1, q - 1 of KEY row key_row
 *   fhe_ckks_public_key_dev  d_pk = [pk0 | pk1] = (-a s + e, a) mod q; d_s as written by fhe_ckks_secret_key_dev
 *   fhe_ckks_encrypt_dev     d_out = [c0 | c1], each batch x n: c0 = v pk0 + e0 + (m_r mod q), c1 = v pk1 + e1; the message
 *            rows are SIGNED words (d_msg NULL: m = 0; msg_stride 0: one message); d_pk_evals as for BFV
 *   fhe_ckks_decrypt_dev     d_out [batch][n] signed words: d = c0 + c1 s mod q, then d - q where d > floor(q / 2)
 * Device buffers need 8-byte alignment.  Rejections are those of the BFV block (table, row range, overlap, extents):
 * FHE_E_INVALID, nothing written; batch = 0 is a no-op. */
#define FHE_STREAM_CKKS_MASK 0x21u
#define FHE_STREAM_CKKS_ERR 0x22u
#define FHE_STREAM_CKKS_KEY 0x23u
#define FHE_STREAM_CKKS_EPH 0x24u
int fhe_ckks_twiddles(uint64_t n, double *out);
int fhe_ckks_encode_dev(uint64_t n, double delta, const void *d_tw, const void *d_z, size_t z_stride, void *d_out,
                        size_t batch, void *hip_stream);
int fhe_ckks_decode_dev(uint64_t n, double delta, const void *d_tw, const void *d_p, void *d_out, size_t batch,
                        void *hip_stream);
int fhe_ckks_secret_key_dev(const fhe_ntt_plan *plan, const uint8_t *seed, uint64_t key_row, void *d_s, void *hip_stream);
int fhe_ckks_public_key_dev(const fhe_ntt_plan *plan, const uint8_t *seed, uint64_t row, const void *d_s, const void *d_cdt,
                            unsigned m, void *d_pk, void *hip_stream);
int fhe_ckks_encrypt_dev(const fhe_ntt_plan *plan, const uint8_t *seed, uint64_t first_row, const void *d_pk_evals,
                         const void *d_msg, size_t msg_stride, const void *d_cdt, unsigned m, void *d_out, size_t batch,
                         void *hip_stream);
int fhe_ckks_decrypt_dev(const fhe_ntt_plan *plan, const void *d_s_evals, const void *d_ct, void *d_out, size_t batch,
                         void *hip_stream);

/* ---- CKKS: the encoder up to n = 2^16 (ckks_client.hip) ----
 * The three encoder entry points above with the ring-size bound 2 <= n <= 2^16; arguments, layouts, alignment, overlap
 * rules, error codes and the order of the checks are theirs, and nothing is written on a rejection.
 *   fhe_ckks_embed_twiddles     HOST only: the table of fhe_ckks_twiddles (the same entries where both accept n)
 *   fhe_ckks_embed_encode_dev   n <= 2^13: the kernel of fhe_ckks_encode_dev, the same words.  2^14 <= n <= 2^16: the
 *            transform of M = n/2 points as two passes, M = M1 M2 (2^6 2^7, 2^7 2^7, 2^7 2^8), through [batch][M] complex
 *            values of library workspace, `chunk` polynomials at a time; the roundings differ from a one-pass transform's
 *            in the last bits, the error bound of §21 holds.
 *   fhe_ckks_embed_decode_dev   the same for fhe_ckks_decode_dev
 *   fhe_ckks_embed_workspace_bytes  the library workspace one such call takes: 8 n min(batch, max(1, 2^21 / n)) bytes for
 *            2^14 <= n <= 2^16 and batch > 0; 0 for n <= 2^13, for batch = 0 and for a shape the calls refuse
 * fhe_ckks_twiddles, fhe_ckks_encode_dev and fhe_ckks_decode_dev keep their bound n <= 2^13. */
int fhe_ckks_embed_twiddles(uint64_t n, double *out);
int fhe_ckks_embed_encode_dev(uint64_t n, double delta, const void *d_tw, const void *d_z, size_t z_stride, void *d_out,
                              size_t batch, void *hip_stream);
int fhe_ckks_embed_decode_dev(uint64_t n, double delta, const void *d_tw, const void *d_p, void *d_out, size_t batch,
                              void *hip_stream);
size_t fhe_ckks_embed_workspace_bytes(uint64_t n, size_t batch);

/* ---- CKKS on an RNS modulus chain: ct x ct, relinearisation, rescaling (ckks_eval.hip) ----
 * A chain is `limbs` plans (1 <= limbs <= 8) of distinct primes q_0 .. and the same n, passed as a HOST array `plans`; the
 * entry points that switch keys also take the plan of one special prime P >= max q_i, distinct from all of them.  A
 * ciphertext at `limbs` limbs is d [limbs][2][batch][n]: evaluation domain (the order of fhe_ntt_forward_dev), canonical
 * residues; dropping the top limb is truncation.  lift(x mod q_j -> q_i): x centred (x - q_j where x > floor(q_j / 2)),
 * reduced modulo q_i.
 *   fhe_ckks_rns_from_i64_dev     d_out [limbs][batch][n] = evals of the signed 64-bit rows d_in [batch][n] modulo each prime
 *   fhe_ckks_rns_relin_key_dev    d_rlk [limbs][limbs + 1][2][n] evals, column i < limbs modulo q_i, column `limbs` modulo P:
 *            rlk[j][i] = (-a_ji s + e_j + [i = j] (P mod q_j) s^2, a_ji) = fhe_ckks_public_key_dev on plan i with row
 *            first_row + j, plus the diagonal term.  d_s [limbs + 1][n]: fhe_ckks_secret_key_dev of one (seed, key_row) under
 *            every plan, the special prime's last.
 *   fhe_ckks_rns_tensor_dev       d_out [limbs][3][batch][n]: d0 = a0 b0, d1 = a0 b1 + a1 b0, d2 = a1 b1 per limb
 *   fhe_ckks_rns_relinearize_dev  d_out [limbs][2][batch][n] from a tensor d_d: digit j = d2 modulo q_j in coefficients,
 *            lifted to every limb of {0 .. limbs - 1, P}; t_i = sum_j D_ji rlk[j][i]; r_i = (t_i - lift(t_P)) P^-1 mod q_i;
 *            out = (d0 + r0, d1 + r1).  d_rlk was made for key_limbs >= limbs limbs: its digits j < limbs and columns
 *            {0 .. limbs - 1, key_limbs} are read, so one key serves every level.
 *   fhe_ckks_rns_mul_dev          the two above in one call, the tensor kept in the library workspace
 *   fhe_ckks_rns_rescale_dev      d_out [limbs - 1][2][batch][n]: c'_i = (c_i - lift(c_top)) q_top^-1 mod q_i, top = limbs - 1
 *   fhe_ckks_rns_workspace_bytes  the most library workspace one of these calls takes at (n, limbs, batch); 0 for a shape they refuse
 * Device buffers need 8-byte alignment.  FHE_E_NULL for a NULL pointer (a plan included); FHE_E_PARAM_MISMATCH for plans
 * whose n differ; FHE_E_INVALID for limbs outside [1, 8], a repeated modulus, P < max q_i, key_limbs < limbs or > 8, an
 * output that overlaps an input, a rescale at one limb, and the table and row-range conditions of the BFV block.  Nothing
 * is written on rejection; batch = 0 is a no-op. */
int fhe_ckks_rns_from_i64_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const void *d_in, void *d_out, size_t batch,
                              void *hip_stream);
int fhe_ckks_rns_relin_key_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *special,
                               const uint8_t *seed, uint64_t first_row, const void *d_s, const void *d_cdt, unsigned m,
                               void *d_rlk, void *hip_stream);
int fhe_ckks_rns_tensor_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const void *d_a, const void *d_b, void *d_out,
                            size_t batch, void *hip_stream);
int fhe_ckks_rns_relinearize_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *special,
                                 const void *d_rlk, unsigned key_limbs, const void *d_d, void *d_out, size_t batch,
                                 void *hip_stream);
int fhe_ckks_rns_mul_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *special, const void *d_rlk,
                         unsigned key_limbs, const void *d_a, const void *d_b, void *d_out, size_t batch, void *hip_stream);
int fhe_ckks_rns_rescale_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const void *d_in, void *d_out, size_t batch,
                             void *hip_stream);
size_t fhe_ckks_rns_workspace_bytes(uint64_t n, unsigned limbs, size_t batch);

/* ---- CKKS on the RNS chain: slot rotations and conjugation with Galois keys (ckks_eval.hip) ----
 * sigma_g: a(X) -> a(X^g) in Z[X]/(X^n + 1) for g odd, 1 <= g < 2n; a rotation of the slots by `step` is g = 5^step mod 2n,
 * the conjugation g = 2n - 1.  On evals in the engine's order sigma_g is an index permutation that does not depend on q:
 * sigma_g(a)[x] = a[pi_g(x)], pi_g(x) = brv((((2 brv(x) + 1) g mod 2n) - 1) / 2), brv the reversal of log2 n bits.
 *   fhe_ckks_galois_evals_dev     d_out [polys][n] = the rows d_in [polys][n] of evals under sigma_g (plaintexts, keys, tests)
 *   fhe_ckks_rns_galois_key_dev   d_gk, the shape and columns of d_rlk above: gk[j][i] = (-a_ji s + e_j + [i = j] (P mod q_j)
 *            sigma_g(s), a_ji) from rows first_row + j
 *   fhe_ckks_rns_galois_dev       d_out [count][limbs][2][batch][n]: d_in [limbs][2][batch][n] under sigma_gs[r] for every
 *            r < count, each (pi_g(c0) + r0, r1) with (r0, r1) the key switch of pi_g(c1) against d_gks[r] (relinearisation's
 *            steps with d2 = pi_g(c1)); level and scale are unchanged.  d_gks and gs are HOST arrays of `count` device key
 *            pointers and Galois elements; the digit decomposition of c1 runs once per chunk whatever `count` is.
 *   fhe_ckks_rns_galois_workspace_bytes  the library workspace that call takes; 0 for a shape it refuses
 * As the block above, and: FHE_E_INVALID for g even or >= 2n, count > FHE_CKKS_GALOIS_MAX_COUNT, an output that overlaps the
 * input or a key; FHE_E_NULL for a NULL entry of d_gks; batch = 0 or count = 0 is a no-op. */
#define FHE_CKKS_GALOIS_MAX_COUNT 256
int fhe_ckks_galois_evals_dev(const fhe_ntt_plan *plan, uint64_t g, const void *d_in, void *d_out, size_t polys,
                              void *hip_stream);
int fhe_ckks_rns_galois_key_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *special,
                                const uint8_t *seed, uint64_t first_row, uint64_t g, const void *d_s, const void *d_cdt,
                                unsigned m, void *d_gk, void *hip_stream);
int fhe_ckks_rns_galois_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *special,
                            const void *const *d_gks, const uint64_t *gs, unsigned count, unsigned key_limbs,
                            const void *d_in, void *d_out, size_t batch, void *hip_stream);
size_t fhe_ckks_rns_galois_workspace_bytes(uint64_t n, unsigned limbs, size_t batch, unsigned count);

/* ---- CKKS on the RNS chain: plaintext linear transforms, the double-hoisted diagonal sum (ckks_eval.hip) ----
 *   fhe_ckks_rns_diag_sum_dev     d_out [outputs][limbs][2][batch][n]: out_o = sum_{r < count} m_{o,r} (.) sigma_{gs[r]}(d_in) for
 *            d_in [limbs][2][batch][n] and the plaintexts d_pts [outputs][count][limbs + 1][n], canonical evals under the chain
 *            primes and, as limb `limbs`, under P, shared by the batch.  The digit decomposition of c1 runs once per chunk;
 *            the key sums of all elements are weighted and added in the basis Q P, and each output takes ONE division by P.
 *            An element gs[r] = 1 is the identity: it takes no key, d_gks[r] is not read and may be NULL (d_gks itself may be
 *            NULL where every element is 1; then nothing is transformed and no key switch runs).  Elements may repeat.
 *            Level is unchanged; the scale is the ciphertext's times the plaintexts'.  The words are those of the formula
 *            in §24 whatever the order of accumulation: every sum is exact modulo q_i.
 *   fhe_ckks_rns_diag_workspace_bytes  the library workspace that call takes at most; 0 for a shape it refuses
 * d_gks and gs are HOST arrays, as for fhe_ckks_rns_galois_dev, and the conditions are that block's, and: FHE_E_INVALID for
 * outputs = 0 or > FHE_CKKS_DIAG_MAX_OUTPUTS and for an output that overlaps the plaintexts; FHE_E_NULL for a NULL key of an
 * element other than 1.  A plaintext word must be below its modulus: like the ciphertext's canonicity this is the caller's
 * contract and is not checked on the device.  batch = 0 or count = 0 is a no-op (count = 0 writes nothing, not zeros). */
#define FHE_CKKS_DIAG_MAX_OUTPUTS 64
int fhe_ckks_rns_diag_sum_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *special,
                              const void *const *d_gks, const uint64_t *gs, unsigned count, unsigned key_limbs,
                              const void *d_pts, unsigned outputs, const void *d_in, void *d_out, size_t batch,
                              void *hip_stream);
size_t fhe_ckks_rns_diag_workspace_bytes(uint64_t n, unsigned limbs, size_t batch, unsigned count, unsigned outputs);

/* ---- CKKS on the RNS chain: baby-step giant-step linear transforms with hoisted giant steps (ckks_eval.hip) ----
 *   fhe_ckks_rns_bsgs_dev         d_out [limbs][2][batch][n] = sum_{a < giants} sigma_{giant_gs[a]}(sum_{b < babies} m_{a,b} (.)
 *            sigma_{baby_gs[b]}(d_in)) for d_in [limbs][2][batch][n] and the plaintexts d_pts [giants][babies][limbs + 1][n], the
 *            layout and contract of fhe_ckks_rns_diag_sum_dev's with `giants` for its outputs.  With i over {0 .. limbs - 1, P}:
 *            (1) U_{a,i,c}: the key sums of the baby steps weighted by the plaintexts, plus (P mod q_i) times the addends
 *                pi_{g_b}(c0) in component 0 and c1 (for g_b = 1) in component 1; the digits of c1 are made once per chunk.
 *            (2) V = 0 in the basis Q P.  For h_a = 1: V += U_a.  Otherwise w_a = (U_{a,i,1} - lift(U_{a,P,1})) P^-1 mod q_i, the
 *                modulus-down of component 1 of U_a alone; D^(a) the digits of w_a; S_{a,i,c}[x] = sum_j D^(a)_{j,i}[pi_{h_a}(x)]
 *                gk_{h_a}[j][i][c][x]; V_{i,0} += S_{a,i,0} + U_{a,i,0}[pi_{h_a}(x)], V_{i,1} += S_{a,i,1}, on every i, P included.
 *            (3) d_out = the modulus-down by P of both components of V.
 *            Every word is canonical modulo its limb's prime, so the result does not depend on the order or grouping of the
 *            giant steps.  One division by P of one component per giant step with a key and one of both components per call,
 *            where the composition of fhe_ckks_rns_diag_sum_dev and fhe_ckks_rns_galois_dev takes two of both per giant step.
 *            An element 1 is the identity in either role: it takes no key and its entry is not read.  Where every element is
 *            1 no digit, transform or modulus-down runs.  Level unchanged; the scale is the ciphertext's times the plaintexts'.
 *   fhe_ckks_rns_bsgs_workspace_bytes  the library workspace that call takes at most; 0 for a shape it refuses
 * d_baby_gks, baby_gs, d_giant_gks and giant_gs are HOST arrays.  The conditions are those of fhe_ckks_rns_diag_sum_dev for
 * both lists, and: FHE_E_INVALID for babies outside [1, FHE_CKKS_GALOIS_MAX_COUNT] or giants outside [1,
 * FHE_CKKS_DIAG_MAX_OUTPUTS]; FHE_E_NULL for a NULL key of an element other than 1, baby or giant; FHE_E_INVALID for an output
 * that overlaps the input, a key or the plaintexts.  Nothing is written on rejection; batch = 0 is a no-op. */
int fhe_ckks_rns_bsgs_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *special,
                          const void *const *d_baby_gks, const uint64_t *baby_gs, unsigned babies,
                          const void *const *d_giant_gks, const uint64_t *giant_gs, unsigned giants, unsigned key_limbs,
                          const void *d_pts, const void *d_in, void *d_out, size_t batch, void *hip_stream);
size_t fhe_ckks_rns_bsgs_workspace_bytes(uint64_t n, unsigned limbs, size_t batch, unsigned babies, unsigned giants);

/* ---- CKKS on the RNS chain: fused sums of ciphertexts by public scalars (ckks_eval.hip) ----
 *   fhe_ckks_rns_lincomb_dev      d_out [outputs][limbs][2][batch][n]: per limb i, component c and word e
 *            out_o[c][e] = (sum_{r < count} w[o][r][i] ct_r[c][e] + [c = 0] k[o][i]) mod q_i.
 *            d_cts is a HOST array of `count` device pointers to ciphertexts [>= limbs][2][batch][n] (a ciphertext at a
 *            higher level is read as it is: the limb stride does not depend on the level); a pointer may repeat.  w
 *            [outputs][count][limbs] and k [outputs][limbs] (NULL: no constant) are HOST arrays of canonical residues,
 *            consumed before the call returns.  A constant polynomial has every eval equal to the constant, so k is added
 *            to every word of component 0.  Every input word is read once per launch of up to four outputs; no workspace.
 *            The level is `limbs - 1`; what the weights do to the scale is the caller's bookkeeping.
 * FHE_E_NULL for a NULL plan, array or buffer; FHE_E_PARAM_MISMATCH for plans whose n differ; FHE_E_INVALID for limbs not in
 * [1, 8], repeated moduli, count not in [1, FHE_CKKS_LINCOMB_MAX_COUNT], outputs not in [1, FHE_CKKS_LINCOMB_MAX_OUTPUTS], a
 * weight or constant that is not below its q_i, and an output that overlaps an input.  Everything is checked before any
 * device call and nothing is written on rejection; batch = 0 is a no-op. */
#define FHE_CKKS_LINCOMB_MAX_COUNT 64
#define FHE_CKKS_LINCOMB_MAX_OUTPUTS 16
int fhe_ckks_rns_lincomb_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const void *const *d_cts, unsigned count,
                             const uint64_t *w, const uint64_t *k, unsigned outputs, void *d_out, size_t batch,
                             void *hip_stream);

/* ---- CKKS on the RNS chain: inner products, a sum of ct x ct pairs with one relinearisation (ckks_eval.hip) ----
 *   fhe_ckks_rns_dot_dev          d_out [limbs][2][batch][n] = relinearize(sum_{r < count} w_r tensor(a_r, b_r)): per limb i
 *            d0 = sum_r w[r][i] a_r0 b_r0, d1 = sum_r w[r][i] (a_r0 b_r1 + a_r1 b_r0), d2 = sum_r w[r][i] a_r1 b_r1 mod q_i, then
 *            the steps of fhe_ckks_rns_relinearize_dev on (d0, d1, d2).  A key switch is linear in d2, so the call takes ONE
 *            key switch whatever `count` is, and one relinearisation noise term.  The words are those of
 *            fhe_ckks_rns_relinearize_dev applied to the exact sum modulo q_i of the weighted tensors: every sum is exact, so
 *            the order of accumulation does not matter.  d_as and d_bs are HOST arrays of `count` device pointers to
 *            ciphertexts [>= limbs][2][batch][n] (a ciphertext at a higher level is read as it is, as for
 *            fhe_ckks_rns_lincomb_dev); a_r and b_r may be the same pointer (a square) and a pointer may repeat across pairs.
 *            w [count][limbs] is a HOST array of canonical residues, consumed before the call returns; NULL: every weight is
 *            1.  d_rlk and key_limbs as for fhe_ckks_rns_mul_dev: one key serves every level.  The level is `limbs - 1`; the
 *            result is not rescaled, and what the weights do to the scale is the caller's bookkeeping.
 * The library workspace is that of fhe_ckks_rns_mul_dev at the same (n, limbs, batch): the summed tensor lies where that call
 * stages its tensor, so fhe_ckks_rns_workspace_bytes answers for this call too and there is no size query of its own.
 * FHE_E_NULL for a NULL plan (the special prime's included), key, host array, entry of either array or output;
 * FHE_E_PARAM_MISMATCH for plans whose n differ; FHE_E_INVALID for the chain conditions of the §22 block, key_limbs < limbs or
 * > 8, count not in [1, FHE_CKKS_DOT_MAX_COUNT], a weight that is not below its q_i, a misaligned buffer, an output that overlaps
 * an operand or the key, and the batch-size limit of fhe_ckks_rns_mul_dev.  Everything is checked before any device call and
 * nothing is written on rejection; batch = 0 is a no-op. */
#define FHE_CKKS_DOT_MAX_COUNT 64
int fhe_ckks_rns_dot_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *special, const void *d_rlk,
                         unsigned key_limbs, const void *const *d_as, const void *const *d_bs, unsigned count,
                         const uint64_t *w, void *d_out, size_t batch, void *hip_stream);

/* ---- BFV on an RNS modulus chain: exact ct x ct, message scaling, decryption (bfv_rns.hip) ----
 * The chain is q_0 .. q_{k-1}, 1 <= k <= 4, Q their product; the auxiliary base b_0 .. b_k, B its product; the special prime P
 * of the key switch; the plaintext modulus t >= 2.  Every prime is distinct, below 2^62 and has a plan of the same n.  A
 * ciphertext is [k][2][batch][n] evals over all k limbs (the layout of the CKKS block of §22; BFV has no levels), and public
 * keys, relinearisation keys and Galois keys are those of fhe_ckks_public_key_dev, fhe_ckks_rns_relin_key_dev and
 * fhe_ckks_rns_galois_key_dev with limbs = k; slot rotations are fhe_ckks_rns_galois_dev unchanged.
 *   fhe_rns_extend_dev            d_in [src][count], the canonical residues of an integer x modulo src_mods[0 .. src) (M their
 *            product) -> d_out [dst][count], its residues modulo dst_mods[0 .. dst), exactly: x is taken in [0, M), or with
 *            `centred` != 0 in (-M / 2, M / 2].  The moduli are HOST arrays; each is odd, at least 3 and below 2^62, no modulus
 *            repeats within a side, the source moduli are pairwise coprime, and a side has 1 to 9 of them.
 *   fhe_bfv_rns_tensor_dev        d_out [k][3][batch][n] evals: for every coefficient of every component
 *            floor((t d + floor(Q / 2)) / Q) mod q_i, d the negacyclic tensor over the integers (d0 = a0 b0, d1 = a0 b1 + a1 b0,
 *            d2 = a1 b1) of the operands' coefficients centred in Q: round-to-nearest of t d / Q, Q being odd.  Admission:
 *            B > t n Q + 1.  d_out is 16-byte aligned.
 *   fhe_bfv_rns_mul_dev           that, kept in the library workspace, then the steps of fhe_ckks_rns_relinearize_dev against
 *            d_rlk [k][k + 1][2][n] -> d_out [k][2][batch][n]
 *   fhe_bfv_rns_workspace_bytes   the library workspace of fhe_bfv_rns_mul_dev in bytes, or 0 for a shape the calls refuse
 *   fhe_bfv_rns_scale_msg_dev     d_msg [batch][n], words in [0, t) -> d_out [k][batch][n]: floor(Q / t) m mod q_i as centred
 *            signed words, the message fhe_ckks_encrypt_dev takes under limb i (on the same fresh rows for every limb)
 *   fhe_bfv_rns_decrypt_dev       d_ct [k][2][batch][n] evals, d_s_evals [k][n] -> d_out [batch][n]:
 *            floor((t v + floor(Q / 2)) / Q) mod t for the phase v = c0 + c1 s centred in Q; aux0 is one auxiliary prime,
 *            odd, above 2 t + 2, below 2^62 and coprime to Q (t < 2^60)
 * FHE_E_NULL for a NULL plan, modulus array or buffer; FHE_E_PARAM_MISMATCH for plans whose n differ; FHE_E_INVALID for k not
 * in [1, 4] (more than 9 moduli on a side of fhe_rns_extend_dev), a repeated, even or too large modulus, a base that misses
 * the admission, t < 2, a misaligned buffer, an output that overlaps an input, and a batch whose words pass 2^60.  Everything is
 * checked before any device call and nothing is written on rejection; batch = 0 (count = 0) is a no-op. */
int fhe_rns_extend_dev(const uint64_t *src_mods, unsigned src, const uint64_t *dst_mods, unsigned dst, int centred,
                       const void *d_in, void *d_out, size_t count, void *hip_stream);
int fhe_bfv_rns_tensor_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *const *aux, uint64_t t,
                           const void *d_a, const void *d_b, void *d_out, size_t batch, void *hip_stream);
int fhe_bfv_rns_mul_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *const *aux,
                        const fhe_ntt_plan *special, uint64_t t, const void *d_rlk, const void *d_a, const void *d_b,
                        void *d_out, size_t batch, void *hip_stream);
size_t fhe_bfv_rns_workspace_bytes(uint64_t n, unsigned limbs, size_t batch);
int fhe_bfv_rns_scale_msg_dev(const fhe_ntt_plan *const *plans, unsigned limbs, uint64_t t, const void *d_msg, void *d_out,
                              size_t batch, void *hip_stream);
int fhe_bfv_rns_decrypt_dev(const fhe_ntt_plan *const *plans, unsigned limbs, uint64_t aux0, uint64_t t,
                            const void *d_s_evals, const void *d_ct, void *d_out, size_t batch, void *hip_stream);

/* ---- BFV inner products on the chain: sum of ct x ct pairs, one rounding, one relinearisation (bfv_rns.hip) ----
 *   fhe_bfv_rns_dot_dev   d_as, d_bs HOST arrays of `count` device pointers to ciphertexts [k][2][batch][n]; a_r = b_r is a
 *            square and a pointer may repeat across pairs.  w a HOST array of `count` signed weights, each non-zero and below
 *            2^61 in absolute value; NULL: every weight is 1.  For every coefficient of every component
 *                D = sum_r w_r d^(r),   out = floor((t D + floor(Q / 2)) / Q) mod q_i,
 *            d^(r) the negacyclic integer tensor (d0, d1, d2) of pair r's operands centred in Q as fhe_bfv_rns_tensor_dev takes
 *            it; then the steps of fhe_ckks_rns_relinearize_dev against d_rlk [k][k + 1][2][n] -> d_out [k][2][batch][n].  ONE
 *            rounding and ONE key switch whatever `count` is; one pair with w = NULL is fhe_bfv_rns_mul_dev word for word.
 *            Admission: B > t n Q W + 1, W = sum_r |w_r| (|D| <= W n Q^2 / 2).  The library workspace is that of
 *            fhe_bfv_rns_mul_dev: fhe_bfv_rns_workspace_bytes answers for this call too.
 * The rejections are those of fhe_bfv_rns_mul_dev, and FHE_E_INVALID for count not in [1, FHE_BFV_DOT_MAX_COUNT], a zero weight, a
 * weight of 2^61 or more in absolute value, a base that admits fhe_bfv_rns_mul_dev but not this W, and an output that overlaps
 * an operand or the key; FHE_E_NULL for a NULL array or entry.  Everything is checked before any device call and nothing is
 * written on rejection; batch = 0 is a no-op. */
#define FHE_BFV_DOT_MAX_COUNT 64
int fhe_bfv_rns_dot_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *const *aux,
                        const fhe_ntt_plan *special, uint64_t t, const void *d_rlk, const void *const *d_as,
                        const void *const *d_bs, unsigned count, const int64_t *w, void *d_out, size_t batch, void *hip_stream);

/* ---- CKKS on a deep RNS chain: grouped-digit key switching, up to 32 limbs (ckks_deep.hip) ----
 * The block of §22 / §23 with the digits of the key switch grouped: `limbs` plans (1 <= limbs <= 32) of chain primes q_0 ..
 * and `alpha` plans (1 <= alpha <= 8) of special primes p_0 .., P their product, as HOST arrays `plans` and `specials`; all
 * primes distinct, below 2^62, of the same n.  Digit group j holds limbs [j alpha, min((j + 1) alpha, limbs)), Q_j is the
 * product of its primes, dnum = ceil(limbs / alpha).  Admission: P >= Q_j for every j, compared exactly.  Ciphertexts, the
 * tensor, alignment (8 bytes) and the overlap rules are §22's.  A group's integer x_j is the one with d's residues modulo the
 * group's primes, centred in (-Q_j / 2, Q_j / 2].
 *   fhe_ckks_deep_relin_key_dev   d_key [dnum][limbs + alpha][2][n] evals, column i < limbs modulo q_i, column limbs + m modulo
 *            p_m: key[j][i] = (-a_ji s + e_j + [i in group j] (P mod q_i) s^2, a_ji) = fhe_ckks_public_key_dev on plan i with
 *            row first_row + j, plus the diagonal term.  d_s [limbs + alpha][n], the special primes' rows last.  At alpha = 1
 *            the words of fhe_ckks_rns_relin_key_dev.
 *   fhe_ckks_deep_galois_key_dev  the same with sigma_g(s) for s^2
 *   fhe_ckks_deep_relinearize_dev d_out [limbs][2][batch][n] from a tensor d_d [limbs][3][batch][n]: D_ji = x_j mod m_i for every
 *            m_i of {q_0 .. q_{limbs-1}, p_0 .. p_{alpha-1}}, x_j of d2 (i in group j: d2's own limb); t_i = sum_j D_ji key[j][col(i)],
 *            col(i) = i for a chain limb and key_limbs + m for p_m; y the centred integer of t modulo P;
 *            r_i = (t_i - y) P^-1 mod q_i; out = (d0 + r0, d1 + r1).  d_key was made for key_limbs >= limbs limbs with the
 *            same alpha: one key serves every level.
 *   fhe_ckks_deep_mul_dev         the tensor of d_a and d_b and that, the tensor kept in the library workspace
 *   fhe_ckks_deep_galois_dev      d_out [count][limbs][2][batch][n], fhe_ckks_rns_galois_dev's contract: (pi_g(c0) + r0, r1) per
 *            element of the HOST arrays d_gks, gs; one digit decomposition per chunk whatever `count` is
 *   fhe_ckks_deep_rescale_dev     d_out [limbs - 1][2][batch][n], fhe_ckks_rns_rescale_dev's formula for limbs up to 32
 *   fhe_ckks_deep_workspace_bytes the most library workspace one of these calls takes; 0 for a shape they refuse.  With
 *            ng = ceil(limbs / alpha) a key switch stages S = (limbs + alpha) ng + 7 limbs + 2 alpha slabs of n words a
 *            ciphertext (the tensor 3 limbs, the limbs in coefficients, the lifted digits (limbs + alpha) ng - limbs, the key
 *            sums 2 (limbs + alpha), the lifted t_P 2 limbs) over chunks of c = min(batch, max(1, floor(floor(2^21 / n) / S)))
 *            ciphertexts, a rescale 2 limbs slabs over chunks of c' = min(batch, max(1, floor(floor(2^21 / n) / (2 limbs)))):
 *            8 max(S n c, 2 limbs n c') bytes.  The extension tables of a chain (a few KB) are kept on the device apart from it.
 * At alpha = 1 and limbs <= 8 every output equals the §22 / §23 entry point's word for word.  FHE_E_NULL for a NULL pointer (a
 * plan or a key included); FHE_E_PARAM_MISMATCH for plans whose n differ; FHE_E_INVALID for limbs outside [1, 32], alpha
 * outside [1, 8], a repeated prime, a prime of 2^62 or more, a missed admission, key_limbs < limbs or > 32, g even or >= 2n,
 * count > FHE_CKKS_GALOIS_MAX_COUNT, a rescale at one limb, an output that overlaps an input or a key, and the table and
 * row-range conditions of the BFV block.  Nothing is written on rejection; batch = 0 (or count = 0) is a no-op. */
#define FHE_CKKS_DEEP_MAX_LIMBS 32
#define FHE_CKKS_DEEP_MAX_SPECIALS 8
int fhe_ckks_deep_relin_key_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *const *specials,
                                unsigned alpha, const uint8_t *seed, uint64_t first_row, const void *d_s, const void *d_cdt,
                                unsigned m, void *d_key, void *hip_stream);
int fhe_ckks_deep_galois_key_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *const *specials,
                                 unsigned alpha, const uint8_t *seed, uint64_t first_row, uint64_t g, const void *d_s,
                                 const void *d_cdt, unsigned m, void *d_key, void *hip_stream);
int fhe_ckks_deep_relinearize_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *const *specials,
                                  unsigned alpha, const void *d_key, unsigned key_limbs, const void *d_d, void *d_out,
                                  size_t batch, void *hip_stream);
int fhe_ckks_deep_mul_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *const *specials,
                          unsigned alpha, const void *d_key, unsigned key_limbs, const void *d_a, const void *d_b,
                          void *d_out, size_t batch, void *hip_stream);
int fhe_ckks_deep_galois_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *const *specials,
                             unsigned alpha, const void *const *d_gks, const uint64_t *gs, unsigned count,
                             unsigned key_limbs, const void *d_in, void *d_out, size_t batch, void *hip_stream);
int fhe_ckks_deep_rescale_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const void *d_in, void *d_out, size_t batch,
                              void *hip_stream);
size_t fhe_ckks_deep_workspace_bytes(uint64_t n, unsigned limbs, unsigned alpha, size_t batch);

/* ---- CKKS on a deep RNS chain: plaintext linear transforms, the double-hoisted diagonal sum (ckks_deep.hip) ----
 * fhe_ckks_rns_diag_sum_dev (§24) on the chain of the block above, with its plans, specials, alpha, key layout and key_limbs.
 *   fhe_ckks_deep_diag_sum_dev    d_out [outputs][limbs][2][batch][n]: out_o = sum_{r < count} m_{o,r} (.) sigma_{gs[r]}(d_in) for
 *            d_in [limbs][2][batch][n] and the plaintexts d_pts [outputs][count][limbs + alpha][n], canonical evals under the
 *            chain primes and then under the special primes p_0 .. p_{alpha-1} in order, shared by the batch (at alpha = 1
 *            §24's layout).  The grouped digits of c1 are made once per chunk; the key sums of all elements are weighted and
 *            added in the basis Q P, the addends riding along as (P mod q_i) ct, and each output takes ONE division by P.
 *            An element gs[r] = 1 is the identity: it takes no key, d_gks[r] is not read and may be NULL (d_gks itself may be
 *            NULL where every element is 1; then no digit is made, nothing is transformed and no modulus-down runs).  Elements
 *            may repeat.  Level is unchanged; the scale is the ciphertext's times the plaintexts'.  At alpha = 1 and limbs <= 8
 *            the output equals fhe_ckks_rns_diag_sum_dev's word for word.
 *   fhe_ckks_deep_diag_workspace_bytes  the library workspace that call takes at most; 0 for a shape it refuses.  With
 *            ng = ceil(limbs / alpha) and s = min(outputs, 2), the outputs one launch accumulates, the call stages
 *            S = limbs + ((limbs + alpha) ng - limbs) + 2 (limbs + alpha) s + 2 limbs slabs of n words a ciphertext (the limbs in
 *            coefficients, the lifted digits, s sets U of the sums in the basis Q P, the lifted t_P) over chunks of
 *            c = min(batch, max(1, floor(floor(2^21 / n) / S))) ciphertexts: 8 S n c bytes.  `count` does not enter: the
 *            elements are added in registers.
 * d_gks and gs are HOST arrays.  The conditions are the block's above, and: FHE_E_INVALID for count > FHE_CKKS_GALOIS_MAX_COUNT,
 * outputs = 0 or > FHE_CKKS_DIAG_MAX_OUTPUTS, g even or >= 2n, a misaligned buffer or key, a batch too large, and an output that
 * overlaps the input, a key or the plaintexts; FHE_E_NULL for a NULL key of an element other than 1.  A plaintext word must be
 * below its modulus: the caller's contract, not checked on the device.  Nothing is written on rejection; batch = 0 or
 * count = 0 is a no-op (count = 0 writes nothing, not zeros). */
int fhe_ckks_deep_diag_sum_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *const *specials,
                               unsigned alpha, const void *const *d_gks, const uint64_t *gs, unsigned count,
                               unsigned key_limbs, const void *d_pts, unsigned outputs, const void *d_in, void *d_out,
                               size_t batch, void *hip_stream);
size_t fhe_ckks_deep_diag_workspace_bytes(uint64_t n, unsigned limbs, unsigned alpha, size_t batch, unsigned count,
                                          unsigned outputs);

/* ---- CKKS on a deep RNS chain: scalar sums and inner products (ckks_deep.hip) ----
 * fhe_ckks_rns_lincomb_dev (§27) and fhe_ckks_rns_dot_dev (§29) on the chain of the §36 block, for limbs up to 32: what a
 * Chebyshev plan is made of.  The definitions, the HOST arrays, FHE_CKKS_LINCOMB_MAX_COUNT, FHE_CKKS_LINCOMB_MAX_OUTPUTS and
 * FHE_CKKS_DOT_MAX_COUNT are those two blocks'; one launch covers a slice of up to 8 limbs.
 *   fhe_ckks_deep_lincomb_dev     d_out [outputs][limbs][2][batch][n]: out_o[c][e] = (sum_{r < count} w[o][r][i] ct_r[c][e] +
 *            [c = 0] k[o][i]) mod q_i per limb i.  d_cts `count` device pointers to ciphertexts [>= limbs][2][batch][n], a
 *            pointer may repeat; w [outputs][count][limbs] and k [outputs][limbs] (NULL: no constant) canonical residues,
 *            consumed before the call returns: they travel in the kernel arguments, never through a copy from host memory.
 *            Takes no special primes, no workspace and no chunk: ceil(limbs / 8) ceil(outputs / 4) ceil(count / 8) launches
 *            over the whole batch.  The operation is limb-independent, so the words are those of fhe_ckks_rns_lincomb_dev on
 *            slices of at most 8 plans of the same buffers.
 *   fhe_ckks_deep_dot_dev         d_out [limbs][2][batch][n] = relinearize(sum_{r < count} w_r tensor(a_r, b_r)), the relinearisation
 *            fhe_ckks_deep_relinearize_dev's: ONE key switch and one switch error whatever `count` is.  d_as, d_bs `count`
 *            device pointers each, a_r = b_r (a square) and repeated pointers allowed; w [count][limbs] canonical residues or
 *            NULL (every weight 1); d_key, key_limbs, specials and alpha as for fhe_ckks_deep_mul_dev.  The workspace and the
 *            chunk are those of fhe_ckks_deep_mul_dev (the summed tensor lies where that call stages its tensor), so
 *            fhe_ckks_deep_workspace_bytes answers for this call too; a chunk takes ceil(limbs / 8) ceil(count / 16) launches
 *            for the summed tensor and then those of the relinearisation.  With count = 1 and w = NULL the words of
 *            fhe_ckks_deep_mul_dev; at alpha = 1 and limbs <= 8 those of fhe_ckks_rns_dot_dev.
 * FHE_E_NULL for a NULL plan, key, host array, entry of an array or output; FHE_E_PARAM_MISMATCH for plans whose n differ;
 * FHE_E_INVALID for the chain conditions of the §36 block (the dot: with the admission and key_limbs < limbs or > 32), count or
 * outputs outside their ranges, a weight or constant that is not below its q_i, a misaligned buffer, an output that overlaps an
 * input, an operand or the key, and a batch too large.  Everything is checked before any device call and nothing is written on
 * rejection; batch = 0 is a no-op after the host checks. */
int fhe_ckks_deep_lincomb_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const void *const *d_cts, unsigned count,
                              const uint64_t *w, const uint64_t *k, unsigned outputs, void *d_out, size_t batch,
                              void *hip_stream);
int fhe_ckks_deep_dot_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *const *specials,
                          unsigned alpha, const void *d_key, unsigned key_limbs, const void *const *d_as,
                          const void *const *d_bs, unsigned count, const uint64_t *w, void *d_out, size_t batch,
                          void *hip_stream);

/* ---- rows N3 / N4: batch surfaces and element-wise glue, device-resident ----
 * Sums of products are accumulated in the NTT domain and transformed back once; arithmetic
 * mod q is exact, so the words equal the reference's sum of canonical products.
 *
 * `flags` generalise the cached `Rq.evals` (arith/src/ring_nq.rs:24-26,590-599) to the batch
 * surfaces: an operand that is already in the NTT domain (fhe_ntt_forward_dev of it, e.g. a
 * key transformed once) is not transformed again, and a result can be left there for the next
 * product.  Output buffers must not overlap the inputs. */
#define FHE_A_IS_EVALS 1u /* first operand (a / glev / ksk) holds NTT-domain values          */
#define FHE_B_IS_EVALS 2u /* second operand (b / p / v) holds NTT-domain values              */
#define FHE_OUT_EVALS  4u /* leave the result in the NTT domain (no inverse transform)       */

/* TR<Rq> . TR<Rq>, arith/src/tuple_ring.rs:117-134: c[b] = sum_{i<k} a[b][i] * b[b][i].
 * a, b: [batch][k][n]; c: [batch][n]. */
int fhe_tr_dot_dev(const fhe_ntt_plan *plan, const void *d_a, const void *d_b, void *d_c, unsigned k,
                   size_t batch, unsigned flags, void *hip_stream);
/* TR<Rq> x Rq (tuple_ring.rs:137-155) and GLWE<Rq> x Rq (gfhe/src/glwe.rs:263-280):
 * out[b][i] = a[b][i] * p[b], i < rows.  a, out: [batch][rows][n]; p: [batch][n]. */
int fhe_tr_mul_r_dev(const fhe_ntt_plan *plan, const void *d_a, const void *d_p, void *d_out,
                     unsigned rows, size_t batch, unsigned flags, void *hip_stream);
/* GLev<Rq> x Vec<Rq> -> GLWE, gfhe/src/glev.rs:68-80: out[b][c] = sum_{d<l} glev[d][c] * v[b][d].
 * glev: [l][k+1][n] (a key: shared by the batch); v: [batch][l][n]; out: [batch][k+1][n]. */
int fhe_glev_mul_dev(const fhe_ntt_plan *plan, unsigned k, unsigned l, const void *d_glev,
                     const void *d_v, void *d_out, size_t batch, unsigned flags, void *hip_stream);
/* GLWE<Rq>::key_switch, gfhe/src/glwe.rs:126-137: (0, b) - sum_{i<k} ksk[i] * decompose(a_i, beta, l).
 * glwe, out: [batch][k+1][n] as (a_0..a_{k-1}, b); ksk: [k][l][k+1][n] (shared).
 * flags: FHE_A_IS_EVALS only (the key; the ciphertext is decomposed in coefficients). */
int fhe_glwe_key_switch_dev(const fhe_ntt_plan *plan, unsigned k, unsigned beta, unsigned l,
                            const void *d_glwe, const void *d_ksk, void *d_out, size_t batch,
                            unsigned flags, void *hip_stream);
/* Resident key-switching key: the key in the form the product consumes, built once and used by every later call
 * (a key-switching key serves every ciphertext under its secret).  The form is OPAQUE and depends on the shape: with
 * beta = 2, k = 1, 2^8 <= n <= 2^12 and q < 2^61 it holds transforms of the key's 32-bit halves modulo two 27-bit
 * primes (twice the words of the key); otherwise fhe_ntt_forward_dev of the key (what FHE_A_IS_EVALS takes).
 *   fhe_glwe_ksk_prepared_words   u64 words d_prepared must hold (0: invalid arguments)
 *   fhe_glwe_ksk_prepare_dev      d_ksk [k][l][k+1][n] -> d_prepared (distinct buffers)
 *   ..._prepared_dev              the key switch against a prepared key; same words as fhe_glwe_key_switch_dev on
 *                                 the original key.  plan, k, beta, l must be those of the preparation. */
size_t fhe_glwe_ksk_prepared_words(const fhe_ntt_plan *plan, unsigned k, unsigned beta, unsigned l);
int fhe_glwe_ksk_prepare_dev(const fhe_ntt_plan *plan, unsigned k, unsigned beta, unsigned l, const void *d_ksk,
                             void *d_prepared, void *hip_stream);
int fhe_glwe_key_switch_prepared_dev(const fhe_ntt_plan *plan, unsigned k, unsigned beta, unsigned l,
                                     const void *d_glwe, const void *d_prepared, void *d_out, size_t batch,
                                     void *hip_stream);

/* Host-buffer forms of the four surfaces above (same layouts, no flags): what a shim of `gfhe`,
 * whose ciphertexts are host `Vec`s, binds.  They stage through device memory on the calling
 * thread's stream and return when `out` is complete. */
int fhe_tr_dot(const fhe_ntt_plan *plan, const uint64_t *a, const uint64_t *b, uint64_t *c, unsigned k, size_t batch);
int fhe_tr_mul_r(const fhe_ntt_plan *plan, const uint64_t *a, const uint64_t *p, uint64_t *out, unsigned rows, size_t batch);
int fhe_glev_mul(const fhe_ntt_plan *plan, unsigned k, unsigned l, const uint64_t *glev, const uint64_t *v,
                 uint64_t *out, size_t batch);
int fhe_glwe_key_switch(const fhe_ntt_plan *plan, unsigned k, unsigned beta, unsigned l, const uint64_t *glwe,
                        const uint64_t *ksk, uint64_t *out, size_t batch);

/* Rq + Rq, Rq - Rq, -Rq (ring_nq.rs:406-488,551-561), Rq::mul_by_u64 (ring_nq.rs:274-281). */
int fhe_rq_add_dev(const fhe_ntt_plan *plan, const void *d_a, const void *d_b, void *d_c, size_t batch, void *hip_stream);
int fhe_rq_sub_dev(const fhe_ntt_plan *plan, const void *d_a, const void *d_b, void *d_c, size_t batch, void *hip_stream);
int fhe_rq_neg_dev(const fhe_ntt_plan *plan, const void *d_a, void *d_c, size_t batch, void *hip_stream);
int fhe_rq_mul_by_u64_dev(const fhe_ntt_plan *plan, const void *d_a, uint64_t s, void *d_c, size_t batch, void *hip_stream);
/* Rq::mod_switch(p), ring_nq.rs:88-98 / zq.rs:134-139: round(v * p / q) in f64, mod p. */
int fhe_rq_mod_switch_dev(uint64_t q, uint64_t p, const void *d_a, void *d_c, size_t count, void *hip_stream);
/* Ring::mul_div_round for Rq, ring_nq.rs:100-113: Zq::from_f64(round(num * v / den)). */
int fhe_rq_mul_div_round_dev(uint64_t q, uint64_t num, uint64_t den, const void *d_a, void *d_c, size_t count, void *hip_stream);
/* Rq::remodule(p), ring_nq.rs:82-88: every coefficient through Zq::from_u64(p, v) (v mod p).
 * Rq::mul_by_f64(s), ring_nq.rs:282-292: Zq::from_f64(q, v as f64 * s).
 * Rq::div_round(s), ring_nq.rs:299-306: Zq::from_f64(q, round(v as f64 / s as f64)).
 * f64 steps are single IEEE operations, `round` is half away from zero, `as i64` saturates. */
int fhe_rq_remodule_dev(uint64_t p, const void *d_a, void *d_c, size_t count, void *hip_stream);
int fhe_rq_mul_by_f64_dev(uint64_t q, double s, const void *d_a, void *d_c, size_t count, void *hip_stream);
int fhe_rq_div_round_dev(uint64_t q, uint64_t s, const void *d_a, void *d_c, size_t count, void *hip_stream);
/* Rq::decompose(beta, l), ring_nq.rs:67-78 with Zq::decompose zq.rs:141-207 (base 2 and
 * base beta, including their saturation branch).  a: [rows][n] -> out: [rows][l][n].
 * Argument ranges: beta = 2 takes 1 <= l <= 64; at l = 64 the reference's `1 << l` (zq.rs:176-180) overflows — a
 * panic in a debug build, a shift taken modulo 64 in a --release build — and the kernels follow the RELEASE build
 * (the saturation threshold is then 1).  beta > 2 needs beta^l < 2^32 and q / beta^l > 0; anything else is
 * FHE_E_INVALID (the reference panics there in every build).  The same ranges hold for key switching. */
int fhe_rq_decompose_dev(uint64_t q, uint64_t n, unsigned beta, unsigned l, const void *d_a, void *d_out, size_t rows, void *hip_stream);

/* ---- misc ---------------------------------------------------------------- */
/* ---- multi-device --------------------------------------------------------
 * The path shards over independent polynomials / products: one
 * host thread (or process) per device, each calling hipSetDevice() and then the
 * entry points above on its own block of rows; plans are shared, tables and
 * workspaces are per device.  fhe_shard_range gives the contiguous block
 * [*begin, *end) of `total` units owned by `rank` of `world`: ceil(total/world)
 * units per rank, the last ranks short or empty (630 units over 8 ranks:
 * 79 x 7 + 77).  No collective is involved; gathering shards, where a consumer
 * needs them on one device, is the caller's (RCCL all-gather / hipMemcpyPeer). */
int fhe_shard_range(size_t total, unsigned world, unsigned rank, size_t *begin, size_t *end);
/* The one gather a block-partitioned batch may need ("only when a downstream op needs the full batch on one rank"), for a
 * caller WITHOUT torch / RCCL — one host process driving several devices, as a Rust shim behind arith::Rq would: entry r
 * of d_src_shards points at rank r's rows [begin_r, end_r) of fhe_shard_range(total_rows, world, r) on device
 * src_devices[r]; they are copied, in rank order, into d_dst (total_rows x row_words 64-bit words on dst_device) with
 * hipMemcpyPeerAsync (xGMI between devices, a plain copy on the same one) on `hip_stream`, a stream of dst_device.
 * Ordering against the kernels that produced the shards on OTHER devices' streams is the caller's (events or a
 * synchronise), as for any cross-device copy.  Empty shards (ranks past the end) may be NULL. */
int fhe_shard_gather_dev(size_t total_rows, size_t row_words, unsigned world, const int *src_devices,
                         const void *const *d_src_shards, int dst_device, void *d_dst, void *hip_stream);

/* Library workspaces are kept per (device, stream, calling thread) until fhe_ntt_shutdown(): two host threads that
 * enqueue on one stream never share an intermediate.  A thread that exits leaves its buffers to the next thread that
 * needs one on the same (device, stream) — stream order makes that safe — so short-lived threads do not accumulate
 * buffers.  A caller about to DESTROY a stream returns that stream's workspaces — every thread's, whatever entry point
 * took them — with this call, which synchronises the stream first; the caller must make sure that no other thread is
 * inside a library call on that stream at that moment (the same condition under which the stream may be destroyed at
 * all): a buffer another thread has just been handed would be freed under it.  hipStreamPerThread names a different
 * stream in every thread: the call then returns only the calling thread's buffers (a thread that used the host-buffer
 * entry points, which run on hipStreamPerThread, may call it before it exits; otherwise those buffers are released at
 * shutdown). */
int fhe_ntt_release_stream_workspace(void *hip_stream);
/* bytes of library workspace currently held, over all devices, streams and threads (diagnostic) */
size_t fhe_ntt_workspace_bytes(void);

int fhe_ntt_device_count(void);            /* HIP devices visible (0 if none) */
const char *fhe_last_error(void);          /* thread-local, never NULL */
const char *fhe_ntt_version(void);
int fhe_ntt_shutdown(void);                /* frees plans, tables, workspaces */

#ifdef __cplusplus
}
#endif
#endif /* FHE_NTT_H */
