// bfv_client.hip — the client side of BFV on the device (bfv/src/lib.rs:118-225): the secret key, the
// public key, the relinearisation key, encryption and decryption.  Everything is exact and independent of launch geometry.
//
//   stream    the ChaCha20 stream of §17 unchanged (chacha_stream.hpp): key = the 32-byte seed, nonce = (purpose, row lo, row
//             hi), stream word j of a block = u32 word 2j | u32 word 2j + 1 << 32.  Four purposes of their own: BFV_MASK =
//             0x11, BFV_ERR = 0x12, BFV_KEY = 0x13, BFV_EPH = 0x14, so no BFV row shares a nonce with a TFHE row.
//   uniform   coefficient i modulo Q (Q = q or pq, below 2^63) from MASK words w0 = 2i, w1 = 2i + 1 of the row:
//             a_i = floor((w1 2^64 + w0) Q / 2^128) = ((u128) w1 Q + mulhi64(w0, Q)) >> 64.  No rejection: a_i depends on i only.
//   secret    s_i = KEY word i AND 1                                   (the reference's Uniform(0, 2))
//   u         from EPH word i: (w AND 1) - ((w >> 1) AND 1), i.e. -1, 0, 1 with probability 1/4, 1/2, 1/4 (the law of the
//             reference's rounded Uniform(-1.0, 1.0)), stored as 0, 1 or Q - 1
//   errors    cdt_error of §17 at log_scale 0, taken into [0, Q) as e or Q - |e|: the discrete Gaussian of §17, NOT the
//             reference's rounded Normal(0, 3.2).  Encryption row r draws e1 from ERR row 2r and e2 from ERR row 2r + 1, a key
//             row r draws e from ERR row 2r: hence first_row + rows <= 2^63.
//   pk        (-a s + e, a) mod q
//   encrypt   c0 = pk0 u + e1 + Delta (m mod q), c1 = pk1 u + e2, Delta = floor(q / t)
//   decrypt   cs = c0 + c1 s mod q, then Zq::from_f64(q, round(t as f64 * cs as f64 / q as f64)) reduced mod t: the f64 steps
//             of fhe_rq_mul_div_round_dev (glue.hip) on the same f64_as_i64 helper (zq_device.hpp), then fhe_rq_remodule_dev's
//   rlk       (-(a s + e) + p s^2, a) mod pq, EXACTLY.  The reference forms a s and s^2 through `as f64` (tmp_naive_mul ->
//             from_vec_i64), which is exact only while a coefficient of the integer product stays below 2^53; the device
//             computes the exact value everywhere, which is the reference's wherever its route is exact.  Admitted for
//             n pq < 2^63 only: the signed negacyclic product mod 2^64 of fhe_tn_mul_dev is then the integer product, and one
//             reduction mod pq finishes it (p s^2 mod pq = p (s^2 mod q)).
//
// Encryption, the pointwise route: bfv_ephemeral_kernel writes u, the forward transform runs in place,
// bfv_pk_pointwise_kernel multiplies u^ by both key rows (a thread keeps its two key words in registers and walks down the
// batch: the key is read once per workgroup, never staged per row), the two inverse transforms run in place and
// rlwe_encrypt_epilogue_kernel adds e1 + Delta m and e2 on the way to the caller's buffer: one forward and two inverse
// transforms per ciphertext, two staging rows.  The staged route, taken where fhe_rq_mul_dev is one fused kernel because it
// measured faster there: bfv_broadcast_kernel copies both key rows over a chunk once per call and fhe_rq_mul_dev forms
// each product as one fused 32-bit kernel (u is transformed twice); five staging rows.  The staging is bounded by processing
// 2^21 coefficients at a time in workspace slot 10 (32 MiB, 80 MiB staged); every word is a function of its (row, index)
// alone, so the result depends neither on the chunking nor on the route.  Decryption stages c1 the same way (pointwise).
// The kernels make u64 accesses only and the transforms run on library workspace, so callers' buffers need 8-byte alignment.
// The sampling kernels, the pointwise product, the key broadcast, the public-key and encryption epilogues and the host paths of
// public key, encryption and decryption live in bfv_client_kernels.hpp, which ckks_client.hip shares: here are BFV's description
// (`Bfv`), its own kernels and its checks.
#include "bfv_client_kernels.hpp"

using fhe::Mod;
using fhe::u32;
using fhe::u64;

namespace fhe {

// BFV as bfv_client_kernels.hpp's paths take a scheme: its rows of the stream, the unsigned message times Delta, workspace
// slot 10 (slots 0-9 are taken)
struct Bfv {
    static constexpr u32 MASK = 0x11, ERR = 0x12, KEY = 0x13, EPH = 0x14;
    static constexpr bool SIGNED_MSG = false;
    static constexpr int slot = 10;
    static constexpr const char *route_env = "FHE_BFV_ENCRYPT_STAGED", *pk_label = "bfv_pk_epilogue", *encrypt_label = "bfv_encrypt_epilogue",
                                *decrypt_label = "bfv_decrypt_epilogue";
};

// x mod Q for a signed word and any Q below 2^63
__device__ __forceinline__ u64 bfv_smod(u64 x, u64 Q) {
    const long long r = (long long)x % (long long)Q;
    return r < 0 ? (u64)(r + (long long)Q) : (u64)r;
}

// out = Zq::from_f64(q, round(t (c0 + P mod q) / q)) mod t: zq_device.hpp's zq_from_f64, the helper of the library's other
// f64 epilogues (round of an integral value is itself, so its words are rq_mul_div_round_kernel's, glue.hip, which spells
// the same steps out; tests/test_bfv_client_gpu.py compares the two at every residue of q = 65537), then Rq::remodule
__global__ __launch_bounds__(256) void bfv_decrypt_epilogue_kernel(const u64 *__restrict__ c0, const u64 *__restrict__ P, u64 *__restrict__ out, u64 count,
                                                                   u64 t, Mod m) {
    const u64 stride = (u64)gridDim.x * 256;
    const double nf = (double)t, df = (double)m.q;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) {
        const u64 cs = add63(c0[i], P[i], m);
        const u64 v = zq_from_f64(m.q, round((nf * (double)cs) / df));
        out[i] = v >= t ? v % t : v;
    }
}

// dst [n] = src[i] AND 1: a secret key as canonical 0/1 words
__global__ __launch_bounds__(256) void bfv_key_bits_kernel(const u64 *__restrict__ src, u64 *__restrict__ dst, u64 n) {
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) dst[i] = src[i] & 1ull;
}

// rlk [2][n] = (-(a s + e) + p s^2, a) mod pq from the integer products as = a s and ss = s s (signed words, |.| < n pq <
// 2^63): one reduction mod pq each; p (ss mod q) < pq is p ss mod pq
__global__ __launch_bounds__(256) void bfv_rlk_epilogue_kernel(ChaChaKey key, u64 row, const u64 *__restrict__ a, const u64 *__restrict__ as,
                                                               const u64 *__restrict__ ss, const u64 *__restrict__ cdt, u32 cm, u64 *__restrict__ rlk, u64 n,
                                                               u64 q, u64 pq) {
    __shared__ u64 scdt[CDT_MAX];
    for (u32 i = threadIdx.x; i < cm; i += 256) scdt[i] = cdt[i];
    __syncthreads();
    const u64 blocks = (n + 7) / 8, p = pq / q;
    for (u64 c = (u64)blockIdx.x * 256 + threadIdx.x; c < blocks; c += (u64)gridDim.x * 256) {
        u64 w[8];
        if (cm) chacha_block(key, (u32)c, Bfv::ERR, 2 * row, w);
#pragma unroll
        for (u32 j = 0; j < 8; j++) {
            const u64 i = 8 * c + j;
            if (i < n) {
                const u64 e = cm ? bfv_err_residue(cdt_error(scdt, cm, w[j], 0), pq) : 0ull;
                u64 x = bfv_smod(as[i], pq) + e;                       // below 2 pq < 2^64
                x = x >= pq ? x - pq : x;
                u64 y = (x ? pq - x : 0ull) + p * bfv_smod(ss[i], q);
                rlk[i] = y >= pq ? y - pq : y;
                rlk[n + i] = a[i];
            }
        }
    }
}

}  // namespace fhe

// ---- host side -----------------------------------------------------------------------------------------------------
extern "C" int fhe_bfv_secret_key_dev(uint64_t n, const uint8_t *seed, uint64_t key_row, void *d_s, void *hip_stream) {
    const char *who = "fhe_bfv_secret_key_dev";
    int rc = check_ring(n, who);
    if (rc != FHE_OK) return rc;
    if (!seed) return fhe_fail(FHE_E_NULL, "%s: NULL seed", who);
    if (!d_s) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_s)) return fhe_fail(FHE_E_INVALID, "%s: d_s must be 8-byte aligned", who);
    int dev;
    if ((rc = fhe_current_device(&dev)) != FHE_OK) return rc;
    return small_fill(seed_key(seed), fhe::Bfv::KEY, 1, key_row, 0, n, (u64 *)d_s, 1, (hipStream_t)hip_stream);
}

extern "C" int fhe_bfv_public_key_dev(const fhe_ntt_plan *plan, const uint8_t *seed, uint64_t row, const void *d_s, const void *d_cdt, unsigned m,
                                      void *d_pk, void *hip_stream) {
    const char *who = "fhe_bfv_public_key_dev";
    if (!plan) return fhe_fail(FHE_E_NULL, "%s: plan is NULL", who);
    if (!seed) return fhe_fail(FHE_E_NULL, "%s: NULL seed", who);
    const u64 n = plan->n;
    return rlwe_public_key<fhe::Bfv>(who, plan, seed, row, d_s, d_cdt, m, d_pk, (hipStream_t)hip_stream, [&](u64 *S, hipStream_t st) {
        return launch("bfv_key_bits", 0, st, fhe::bfv_key_bits_kernel, fhe_ew_grid(n), 256, d_s, S, n);
    });
}

extern "C" int fhe_bfv_relin_key_dev(uint64_t q, uint64_t n, uint64_t pq, const uint8_t *seed, uint64_t row, const void *d_s, const void *d_cdt,
                                     unsigned m, void *d_rlk, void *hip_stream) {
    const char *who = "fhe_bfv_relin_key_dev";
    int rc = check_ring(n, who);
    if (rc != FHE_OK) return rc;
    if (q < 2 || pq < q || pq % q != 0)
        return fhe_fail(FHE_E_INVALID, "%s: need q >= 2 and pq a multiple of q (q=%llu, pq=%llu)", who, (unsigned long long)q, (unsigned long long)pq);
    if (!mul_fits(n, pq, kRowLimit - 1))
        return fhe_fail(FHE_E_INVALID, "%s: need n pq < 2^63 (n=%llu, pq=%llu)", who, (unsigned long long)n, (unsigned long long)pq);
    if (!seed) return fhe_fail(FHE_E_NULL, "%s: NULL seed", who);
    if ((rc = check_cdt_shape(d_cdt, m, pq, who)) != FHE_OK) return rc;
    if (row >= kRowLimit) return fhe_fail(FHE_E_INVALID, "%s: row must be below 2^63", who);
    if (!d_s || !d_rlk) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_s) || misaligned8(d_rlk)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    if (overlaps_any(d_rlk, 2 * n * 8, {{d_s, n * 8}, {d_cdt, (u64)m * 8}})) return fhe_fail(FHE_E_INVALID, "%s: d_rlk overlaps the key or the error table", who);
    hipStream_t st = (hipStream_t)hip_stream;
    if ((rc = check_cdt_words(d_cdt, m, st, who)) != FHE_OK) return rc;
    void *w = nullptr;
    if ((rc = fhe_workspace_get(fhe::Bfv::slot, 4 * n * 8, st, &w)) != FHE_OK) return rc;
    u64 *A = (u64 *)w, *S = A + n, *AS = S + n, *SS = AS + n;
    const fhe::ChaChaKey key = seed_key(seed);
    if ((rc = uniform_fill(key, fhe::Bfv::MASK, row, pq, n, A, 1, st)) != FHE_OK) return rc;
    if ((rc = launch("bfv_key_bits", 0, st, fhe::bfv_key_bits_kernel, fhe_ew_grid(n), 256, d_s, S, n)) != FHE_OK) return rc;
    if ((rc = fhe_tn_mul_dev(n, A, S, AS, 1, st)) != FHE_OK) return rc;
    if ((rc = fhe_tn_mul_dev(n, S, S, SS, 1, st)) != FHE_OK) return rc;
    return launch("bfv_rlk_epilogue", (int)log2_of(n), st, fhe::bfv_rlk_epilogue_kernel, fhe_ew_grid((n + 7) / 8), 256, key, row, A, AS, SS, d_cdt, m, d_rlk, n,
                  q, pq);
}

extern "C" int fhe_bfv_encrypt_dev(const fhe_ntt_plan *plan, uint64_t t, const uint8_t *seed, uint64_t first_row, const void *d_pk_evals,
                                   const void *d_msg, size_t msg_stride, const void *d_cdt, unsigned m, void *d_out, size_t batch, void *hip_stream) {
    const char *who = "fhe_bfv_encrypt_dev";
    if (!plan) return fhe_fail(FHE_E_NULL, "%s: plan is NULL", who);
    if (!seed) return fhe_fail(FHE_E_NULL, "%s: NULL seed", who);
    const u64 q = plan->q;
    if (t < 2 || t >= q) return fhe_fail(FHE_E_INVALID, "%s: need 2 <= t < q (t=%llu, q=%llu)", who, (unsigned long long)t, (unsigned long long)q);
    return rlwe_encrypt<fhe::Bfv>(who, plan, q / t, seed, first_row, d_pk_evals, d_msg, msg_stride, d_cdt, m, d_out, batch, (hipStream_t)hip_stream);
}

extern "C" int fhe_bfv_decrypt_dev(const fhe_ntt_plan *plan, uint64_t t, const void *d_s_evals, const void *d_ct, void *d_out, size_t batch,
                                   void *hip_stream) {
    const char *who = "fhe_bfv_decrypt_dev";
    if (!plan) return fhe_fail(FHE_E_NULL, "%s: plan is NULL", who);
    const u64 q = plan->q;
    if (t < 2 || t >= q) return fhe_fail(FHE_E_INVALID, "%s: need 2 <= t < q (t=%llu, q=%llu)", who, (unsigned long long)t, (unsigned long long)q);
    hipStream_t st = (hipStream_t)hip_stream;
    return rlwe_decrypt<fhe::Bfv>(who, plan, d_s_evals, d_ct, d_out, batch, st, [&](const char *label, const u64 *c0, const u64 *P, u64 *out, u64 count) {
        return launch(label, (int)plan->log_n, st, fhe::bfv_decrypt_epilogue_kernel, fhe_ew_grid(count), 256, c0, P, out, count, t, plan->mod);
    });
}
