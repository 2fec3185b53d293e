// bfv_client_kernels.hpp — what the RLWE client units share (bfv_client.hip; ckks_client.hip, §21): the
// sampling kernels over the ChaCha20 stream of chacha_stream.hpp (uniform rows modulo Q, the ternary / bit rows), the
// broadcast pointwise product against a key, the key broadcast of the staged route, the public-key and encryption
// epilogues, and the host side: the helpers that launch and check the kernels and the one path each of public key,
// encryption and decryption, which a unit instantiates with the description of its scheme (`Scheme`, below).
// A kernel can only be launched from the translation unit that defines it, so the kernels are `static` or templates here
// and each unit gets its own copy; the words are defined in §20 and do not depend on the including unit.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "capi_internal.hpp"
#include "chacha_stream.hpp"
#include "smallq.hpp"

namespace fhe {

__device__ __forceinline__ u64 bfv_uniform(u64 w0, u64 w1, u64 Q) {
    return (u64)(((unsigned __int128)w1 * Q + __umul64hi(w0, Q)) >> 64);
}
// a b mod q for canonical or arbitrary words and any q below 2^63 (uniform branch)
__device__ __forceinline__ u64 bfv_mulmod(u64 a, u64 b, const Mod &m) { return (m.q >> 62) ? mul_mod_var63(a, b, m) : mul_mod_var(a, b, m); }
// the signed error word e (|e| < Q) as a residue
__device__ __forceinline__ u64 bfv_err_residue(u64 e, u64 Q) { return (long long)e < 0 ? Q + e : e; }

// A thread holds `1 << lper` (at most PER) consecutive words of the flat output, thread i the words from i << lper on; the
// block's words leave through LDS so that every store instruction writes 256 consecutive words.  All 256 threads call it.
template <u32 PER>
__device__ __forceinline__ void bfv_store_block(u64 *stage, const u64 (&v)[PER], u32 lper, u64 block_first_word, u64 total_words, u64 *__restrict__ out) {
    const u32 tid = threadIdx.x, per = 1u << lper;
#pragma unroll
    for (u32 j = 0; j < PER; j++)
        if (j < per) stage[tid * (PER + 1) + j] = v[j];
    __syncthreads();
#pragma unroll
    for (u32 k = 0; k < PER; k++) {
        const u32 t = k * 256 + tid;
        if (t < (256u << lper) && block_first_word + t < total_words) out[block_first_word + t] = stage[(t >> lper) * (PER + 1) + (t & (per - 1))];
    }
    __syncthreads();
}

// out [rows][n]: uniform coefficients modulo Q of `purpose` rows first_row ..; a thread takes a ChaCha block = 4 coefficients
// (n = 2: the two of its row).  lper = log2 min(n, 4), row_blocks = max(n / 4, 1).
static __global__ __launch_bounds__(256) void bfv_uniform_kernel(ChaChaKey key, u32 purpose, u64 first_row, u64 Q, u32 lper, u64 row_blocks, u64 rows,
                                                                 u64 *__restrict__ out) {
    __shared__ u64 stage[256 * 5];
    const u64 total = rows * row_blocks;
    for (u64 base = (u64)blockIdx.x * 256; base < total; base += (u64)gridDim.x * 256) {
        const u64 i = base + threadIdx.x;
        u64 v[4] = {0, 0, 0, 0};
        if (i < total) {
            const u64 r = i / row_blocks, c = i - r * row_blocks;
            u64 w[8];
            chacha_block(key, (u32)c, purpose, first_row + r, w);
#pragma unroll
            for (u32 j = 0; j < 4; j++) v[j] = bfv_uniform(w[2 * j], w[2 * j + 1], Q);
        }
        bfv_store_block<4>(stage, v, lper, base << lper, total << lper, out);
    }
}

// out [rows][n] from `purpose` rows first_row ..: key != 0: the secret-key bits w AND 1 (BFV_KEY); key = 0: the ternary
// (w AND 1) - ((w >> 1) AND 1) as the residue 0, 1 or Q - 1 (BFV's ephemeral u, CKKS's secret and ephemeral), ready for the
// forward transform.  A thread takes a block = 8 coefficients.
static __global__ __launch_bounds__(256) void bfv_ephemeral_kernel(ChaChaKey key, u32 purpose, u32 is_key, u64 first_row, u64 Q, u32 lper, u64 row_blocks,
                                                                   u64 rows, u64 *__restrict__ out) {
    __shared__ u64 stage[256 * 9];
    const u64 total = rows * row_blocks;
    for (u64 base = (u64)blockIdx.x * 256; base < total; base += (u64)gridDim.x * 256) {
        const u64 i = base + threadIdx.x;
        u64 v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (i < total) {
            const u64 r = i / row_blocks, c = i - r * row_blocks;
            u64 w[8];
            chacha_block(key, (u32)c, purpose, first_row + r, w);
#pragma unroll
            for (u32 j = 0; j < 8; j++) {
                const u32 b0 = (u32)w[j] & 1u, b1 = ((u32)w[j] >> 1) & 1u;
                v[j] = is_key ? (u64)b0 : (b0 == b1 ? 0ull : (b0 ? 1ull : Q - 1));
            }
        }
        bfv_store_block<8>(stage, v, lper, base << lper, total << lper, out);
    }
}

// KEYS = 2: out0[r] = u^[r] (.) key[0], out1[r] = u^[r] (.) key[1] (encryption; out0 may be u^ itself); KEYS = 1: out0[r] =
// u^[r] (.) key[0] (decryption).  key [KEYS][n] is shared by the batch: a thread loads its column's key words once and walks
// down the rows, rpb = 256 / min(n, 256) rows per pass.  Any q below 2^63: the 128-bit product with zq_device.hpp's reduction.
template <int KEYS>
__global__ __launch_bounds__(256) void bfv_pk_pointwise_kernel(const u64 *u, const u64 *__restrict__ key, u64 *out0, u64 *__restrict__ out1, u32 L, u64 rows,
                                                               Mod m) {
    const u64 n = 1ull << L;
    const u32 lc = L < 8u ? L : 8u, rpb = 256u >> lc;                        // columns of a block = 1 << lc
    const u64 col = ((u64)blockIdx.x << lc) + (threadIdx.x & ((1u << lc) - 1u));
    const u64 k0 = key[col], k1 = KEYS == 2 ? key[n + col] : 0ull;
    for (u64 r = (u64)blockIdx.y * rpb + (threadIdx.x >> lc); r < rows; r += (u64)gridDim.y * rpb) {
        const u64 x = u[(r << L) + col];
        out0[(r << L) + col] = bfv_mulmod(x, k0, m);
        if (KEYS == 2) out1[(r << L) + col] = bfv_mulmod(x, k1, m);
    }
}

// dst [rows][n] = src [n]: the key rows of the staged route, once per call
static __global__ __launch_bounds__(256) void bfv_broadcast_kernel(const u64 *__restrict__ src, u64 *__restrict__ dst, u32 L, u64 rows) {
    const u64 total = rows << L, N = 1ull << L;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < total; i += (u64)gridDim.x * 256) dst[i] = src[i & (N - 1)];
}

// x mod q for a signed word and any q below 2^63, by the multiplication of reduce_any
__device__ __forceinline__ u64 ckks_smod(u64 x, const Mod &m) {
    const bool neg = (long long)x < 0;
    const u64 r = reduce_any(neg ? 0ull - x : x, m);
    return (neg && r) ? m.q - r : r;
}

// pk [2][n] = (-(a s) + e, a) mod q: as = a s mod q, e from row 2 row of the scheme's error purpose ERR; a thread takes 8
// coefficients
template <u32 ERR>
__global__ __launch_bounds__(256) void rlwe_pk_epilogue_kernel(ChaChaKey key, u64 row, const u64 *__restrict__ a, const u64 *__restrict__ as,
                                                               const u64 *__restrict__ cdt, u32 cm, u64 *__restrict__ pk, u64 n, Mod m) {
    __shared__ u64 scdt[CDT_MAX];
    for (u32 i = threadIdx.x; i < cm; i += 256) scdt[i] = cdt[i];
    __syncthreads();
    const u64 blocks = (n + 7) / 8;
    for (u64 c = (u64)blockIdx.x * 256 + threadIdx.x; c < blocks; c += (u64)gridDim.x * 256) {
        u64 w[8];
        if (cm) chacha_block(key, (u32)c, ERR, 2 * row, w);
#pragma unroll
        for (u32 j = 0; j < 8; j++) {
            const u64 i = 8 * c + j;
            if (i < n) {
                const u64 e = cm ? bfv_err_residue(cdt_error(scdt, cm, w[j], 0), m.q) : 0ull;
                pk[i] = add63(sub63(0ull, as[i], m), e, m);
                pk[n + i] = a[i];
            }
        }
    }
}

// out0[r] = P0[r] + e1 + M(msg_r), out1[r] = P1[r] + e2 (mod q, canonical) for encryption row first_row + r: e1 from ERR row
// 2 (first_row + r), e2 from the row after it; a thread takes 8 coefficients (one ChaCha block of each error row), the
// table sits in LDS.  The message term M of a word x: delta (x mod q), x unsigned (BFV), or with SIGNED_MSG x mod q, x signed,
// delta unread (CKKS).  msg null: M = 0; msg_stride 0: one message for every row.
template <u32 ERR, bool SIGNED_MSG>
__global__ __launch_bounds__(256) void rlwe_encrypt_epilogue_kernel(ChaChaKey key, u64 first_row, const u64 *__restrict__ P0, const u64 *__restrict__ P1,
                                                                    const u64 *__restrict__ msg, u64 msg_stride, const u64 *__restrict__ cdt, u32 cm,
                                                                    u64 delta, u64 *__restrict__ out0, u64 *__restrict__ out1, u32 L, u64 rows, Mod m) {
    __shared__ u64 scdt[CDT_MAX];
    for (u32 i = threadIdx.x; i < cm; i += 256) scdt[i] = cdt[i];
    __syncthreads();
    const u32 LB = L > 3u ? L - 3u : 0u;                          // blocks per row = max(n / 8, 1)
    const u64 n = 1ull << L, total = rows << LB, stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const u64 r = i >> LB, c = i & ((1ull << LB) - 1u), erow = 2 * (first_row + r);
        u64 w1[8], w2[8];
        if (cm) {
            chacha_block(key, (u32)c, ERR, erow, w1);
            chacha_block(key, (u32)c, ERR, erow + 1, w2);
        }
        const u64 at = (r << L) + 8 * c;
        const u64 *__restrict__ mp = msg ? msg + r * msg_stride + 8 * c : nullptr;
#pragma unroll
        for (u32 j = 0; j < 8; j++) {
            if (8 * c + j < n) {
                const u64 e1 = cm ? bfv_err_residue(cdt_error(scdt, cm, w1[j], 0), m.q) : 0ull;
                const u64 e2 = cm ? bfv_err_residue(cdt_error(scdt, cm, w2[j], 0), m.q) : 0ull;
                const u64 dm = !mp ? 0ull : SIGNED_MSG ? ckks_smod(mp[j], m) : bfv_mulmod(reduce_any(mp[j], m), delta, m);
                out0[at + j] = add63(add63(P0[at + j], e1, m), dm, m);
                out1[at + j] = add63(P1[at + j], e2, m);
            }
        }
    }
}

}  // namespace fhe

// ---- host side -----------------------------------------------------------------------------------------------------
namespace {

constexpr fhe::u64 kChunkWords = 1ull << 21;         // ciphertexts are processed 2^21 coefficients at a time: 32 MiB of staging
constexpr fhe::u64 kRowLimit = 1ull << 63;           // error rows are 2 r and 2 r + 1

// the table's shape without a device: m <= 1024 entries, every magnitude (at most m) below the modulus
inline int check_cdt_shape(const void *d_cdt, unsigned m, fhe::u64 Q, const char *who) {
    if (m > fhe::CDT_MAX) return fhe_fail(FHE_E_INVALID, "%s: m=%u thresholds, at most %u", who, m, fhe::CDT_MAX);
    if (m >= Q) return fhe_fail(FHE_E_INVALID, "%s: the largest error magnitude m=%u must be below the modulus %llu", who, m, (unsigned long long)Q);
    if (m && !d_cdt) return fhe_fail(FHE_E_NULL, "%s: NULL error table with m=%u", who, m);
    if (m && misaligned8(d_cdt)) return fhe_fail(FHE_E_INVALID, "%s: d_cdt must be 8-byte aligned", who);
    return FHE_OK;
}
// its words, as §17 checks them: strictly increasing thresholds below 2^63, on a host copy (synchronises `st`)
inline int check_cdt_words(const void *d_cdt, unsigned m, hipStream_t st, const char *who) {
    if (m == 0) return FHE_OK;
    std::vector<fhe::u64> t(m);
    HIP_TRY(hipMemcpyAsync(t.data(), d_cdt, (size_t)m * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (unsigned i = 0; i < m; i++)
        if (t[i] >> 63 || (i && t[i] <= t[i - 1]))
            return fhe_fail(FHE_E_INVALID, "%s: the error table must be strictly increasing and below 2^63 (entry %u)", who, i);
    return FHE_OK;
}

inline fhe::u32 log2_of(fhe::u64 n) { return (fhe::u32)__builtin_ctzll(n); }

// out [rows][n]: the uniform rows modulo Q of `purpose`
inline int uniform_fill(const fhe::ChaChaKey &key, fhe::u32 purpose, fhe::u64 first_row, fhe::u64 Q, fhe::u64 n, fhe::u64 *out, fhe::u64 rows, hipStream_t st) {
    const fhe::u32 lper = std::min<fhe::u32>(log2_of(n), 2u);
    const fhe::u64 row_blocks = n >> lper;
    return launch("bfv_uniform", (int)log2_of(n), st, fhe::bfv_uniform_kernel, fhe_ew_grid(rows * row_blocks), 256, key, purpose, first_row, Q, lper, row_blocks,
                  rows, out);
}
// out [rows][n]: secret-key bits (is_key) or the ternary residues modulo Q
inline int small_fill(const fhe::ChaChaKey &key, fhe::u32 purpose, fhe::u32 is_key, fhe::u64 first_row, fhe::u64 Q, fhe::u64 n, fhe::u64 *out, fhe::u64 rows,
                      hipStream_t st) {
    const fhe::u32 lper = std::min<fhe::u32>(log2_of(n), 3u);
    const fhe::u64 row_blocks = n >> lper;
    return launch("bfv_ephemeral", (int)log2_of(n), st, fhe::bfv_ephemeral_kernel, fhe_ew_grid(rows * row_blocks), 256, key, purpose, is_key, first_row, Q, lper,
                  row_blocks, rows, out);
}

template <int KEYS>
int pointwise(const fhe_ntt_plan *plan, const fhe::u64 *u, const fhe::u64 *key, fhe::u64 *out0, fhe::u64 *out1, fhe::u64 rows, hipStream_t st) {
    const fhe::u32 L = plan->log_n, lc = std::min<fhe::u32>(L, 8u), rpb = 256u >> lc;
    const unsigned gx = (unsigned)(plan->n >> lc);
    const fhe::u64 passes = (rows + rpb - 1) / rpb;
    const unsigned gy = (unsigned)std::min<fhe::u64>(passes, std::max<fhe::u64>(1, 4096 / gx));
    {
        fhe::KernelTimer kt_("bfv_pk_pointwise", (int)L, st);
        hipLaunchKernelGGL(fhe::bfv_pk_pointwise_kernel<KEYS>, dim3(gx, gy), dim3(256), 0, st, u, key, out0, out1, L, rows, plan->mod);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FHE_OK : fhe_hip_fail(e, "bfv_pk_pointwise_kernel");
}

// BFV's route rule between the staged and the pointwise product: staged where fhe_rq_mul_dev is one fused
// kernel; `env` = "0" / "1" (read per call) forces the pointwise / the staged route
inline int encrypt_route_staged(const fhe_ntt_plan *plan, const char *env, bool *staged) {
    fhe::DevicePlan dp;
    const int rc = fhe_device_plan(plan, &dp);
    if (rc != FHE_OK) return rc;
    fhe::SmallQArgs sq{};
    const char *route = getenv(env);
    const bool fused_product = fhe_smallq_args(plan, dp, &sq) || (plan->log_n >= 8 && plan->log_n <= 13);
    *staged = route && route[0] == '1' ? true : fused_product && !(route && route[0] == '0');
    return FHE_OK;
}

// The transforms take 16-byte aligned rows and the ABI promises 8: the rows a transform can read, `src` itself or, where
// it is misaligned, its `words` copied into the workspace rows `ws`
inline int aligned_rows(const fhe::u64 *src, fhe::u64 *ws, fhe::u64 words, hipStream_t st, const fhe::u64 **rows) {
    *rows = src;
    if (!fhe_misaligned(src)) return FHE_OK;
    HIP_TRY(hipMemcpyAsync(ws, src, words * 8, hipMemcpyDeviceToDevice, st));
    *rows = ws;
    return FHE_OK;
}

// ---- the client paths, once for every scheme -------------------------------------------------------------------------
// A unit describes its scheme by a struct `Scheme` of constants: MASK, ERR, KEY, EPH, the purposes of its rows of the
// stream; SIGNED_MSG, the message term of rlwe_encrypt_epilogue_kernel; slot, the fhe_workspace_get slot of its staging
// rows; route_env, the switch that forces a route of encryption; pk_label, encrypt_label, decrypt_label, the KernelTimer
// labels of its epilogues.  The entry point checks plan, seed and what only its scheme has (BFV's t) and passes its own
// steps in; the rest of the call is here, the remaining checks included, in the order the ABI documents.

// pk = (-a s + e, a) of key row `row`.  stage_key(S, st) writes the secret as n canonical words to the 16-byte aligned row S.
template <class Scheme, class StageKey>
int rlwe_public_key(const char *who, const fhe_ntt_plan *plan, const uint8_t *seed, fhe::u64 row, const void *d_s, const void *d_cdt, unsigned m, void *d_pk,
                    hipStream_t st, StageKey stage_key) {
    using fhe::u64;
    const u64 n = plan->n, q = plan->q;
    int rc = check_cdt_shape(d_cdt, m, q, who);
    if (rc != FHE_OK) return rc;
    if (row >= kRowLimit) return fhe_fail(FHE_E_INVALID, "%s: row must be below 2^63", who);
    if (!d_s || !d_pk) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_s) || misaligned8(d_pk)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    if (overlaps_any(d_pk, 2 * n * 8, {{d_s, n * 8}, {d_cdt, (u64)m * 8}})) return fhe_fail(FHE_E_INVALID, "%s: d_pk overlaps the key or the error table", who);
    if ((rc = check_cdt_words(d_cdt, m, st, who)) != FHE_OK) return rc;
    void *w = nullptr;
    if ((rc = fhe_workspace_get(Scheme::slot, 3 * n * 8, st, &w)) != FHE_OK) return rc;
    u64 *A = (u64 *)w, *S = A + n, *P = S + n;
    const fhe::ChaChaKey key = seed_key(seed);
    if ((rc = uniform_fill(key, Scheme::MASK, row, q, n, A, 1, st)) != FHE_OK) return rc;
    if ((rc = stage_key(S, st)) != FHE_OK) return rc;
    if ((rc = fhe_rq_mul_dev(plan, A, 0, S, 0, P, nullptr, nullptr, nullptr, 1, nullptr, st)) != FHE_OK) return rc;
    return launch(Scheme::pk_label, (int)plan->log_n, st, fhe::rlwe_pk_epilogue_kernel<Scheme::ERR>, fhe_ew_grid((n + 7) / 8), 256, key, row, A, P, d_cdt, m, d_pk,
                  n, plan->mod);
}

// [c0 | c1] of `batch` fresh rows from first_row; delta is the factor of BFV's message term (unread under SIGNED_MSG)
template <class Scheme>
int rlwe_encrypt(const char *who, const fhe_ntt_plan *plan, fhe::u64 delta, const uint8_t *seed, fhe::u64 first_row, const void *d_pk_evals, const void *d_msg,
                 size_t msg_stride, const void *d_cdt, unsigned m, void *d_out, size_t batch, hipStream_t st) {
    using fhe::u32;
    using fhe::u64;
    const u64 n = plan->n, q = plan->q;
    int rc = check_cdt_shape(d_cdt, m, q, who);
    if (rc != FHE_OK) return rc;
    if (d_msg && msg_stride != 0 && msg_stride < n) return fhe_fail(FHE_E_INVALID, "%s: msg_stride must be 0 (one message) or at least n", who);
    if (batch == 0) return FHE_OK;
    if (first_row > kRowLimit || (u64)batch > kRowLimit - first_row) return fhe_fail(FHE_E_INVALID, "%s: first_row + batch passes 2^63", who);
    if (!mul_fits((u64)batch, 2 * n, kWordLimit) || !mul_fits((u64)batch - 1, (u64)msg_stride, kWordLimit - n))
        return fhe_fail(FHE_E_INVALID, "%s: batch or msg_stride too large", who);
    if (!d_pk_evals || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_pk_evals) || misaligned8(d_msg) || misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    const u64 out_bytes = (u64)batch * 2 * n * 8, msg_bytes = d_msg ? (((u64)batch - 1) * msg_stride + n) * 8 : 0;
    if (overlaps_any(d_out, out_bytes, {{d_pk_evals, 2 * n * 8}, {d_msg, msg_bytes}, {d_cdt, (u64)m * 8}}))
        return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps the key, the messages or the error table", who);
    if ((rc = check_cdt_words(d_cdt, m, st, who)) != FHE_OK) return rc;
    const u32 L = plan->log_n;
    const u64 chunk = std::min<u64>(batch, std::max<u64>(1, kChunkWords >> L));
    // Two routes to the two products, same words (DESIGN.md §20 has the rule and the measurements).  Where fhe_rq_mul_dev is
    // one fused kernel (moduli with a 32-bit form, smallq.hip: q < 2^30, 2^8 <= n <= 2^18; any modulus at the single-pass
    // sizes 2^8 <= n <= 2^13), two of them against the key rows staged over a chunk (once per call) measured faster than
    // forward + pointwise + two inverses.  Everything else: the pointwise route.  FHE_BFV_ENCRYPT_STAGED / FHE_CKKS_ENCRYPT_STAGED
    // = 0 / = 1 (read per call: tools/bfv_client_rate.py times both routes in one process) forces the pointwise / the staged route.
    bool staged = false;
    if ((rc = encrypt_route_staged(plan, Scheme::route_env, &staged)) != FHE_OK) return rc;
    void *w = nullptr;
    if ((rc = fhe_workspace_get(Scheme::slot, (staged ? 5 : 2) * chunk * n * 8, st, &w)) != FHE_OK) return rc;
    u64 *U = (u64 *)w, *H = U + chunk * n, *P = nullptr, *K0 = nullptr, *K1 = nullptr;
    if (staged) {
        P = H + chunk * n; K0 = P + chunk * n; K1 = K0 + chunk * n;
        if ((rc = launch("bfv_broadcast", (int)L, st, fhe::bfv_broadcast_kernel, fhe_ew_grid(chunk << L), 256, d_pk_evals, K0, L, chunk)) != FHE_OK) return rc;
        if ((rc = launch("bfv_broadcast", (int)L, st, fhe::bfv_broadcast_kernel, fhe_ew_grid(chunk << L), 256, (const u64 *)d_pk_evals + n, K1, L, chunk)) != FHE_OK)
            return rc;
    }
    const fhe::ChaChaKey key = seed_key(seed);
    const u32 LB = L > 3 ? L - 3 : 0;
    for (u64 r0 = 0; r0 < batch; r0 += chunk) {
        const u64 cr = std::min<u64>(chunk, batch - r0);
        const u64 *R0 = U, *R1 = H;                               // the two products of the chunk
        if ((rc = small_fill(key, Scheme::EPH, 0, first_row + r0, q, n, U, cr, st)) != FHE_OK) return rc;
        if (staged) {
            if ((rc = fhe_rq_mul_dev(plan, U, 0, K0, 1, P, nullptr, nullptr, nullptr, cr, nullptr, st)) != FHE_OK) return rc;
            if ((rc = fhe_rq_mul_dev(plan, U, 0, K1, 1, H, nullptr, nullptr, nullptr, cr, nullptr, st)) != FHE_OK) return rc;
            R0 = P;
        } else {
            if ((rc = fhe_ntt_forward_dev(plan, U, U, cr, st)) != FHE_OK) return rc;
            if ((rc = pointwise<2>(plan, U, (const u64 *)d_pk_evals, U, H, cr, st)) != FHE_OK) return rc;
            if ((rc = fhe_ntt_inverse_dev(plan, U, U, cr, st)) != FHE_OK) return rc;
            if ((rc = fhe_ntt_inverse_dev(plan, H, H, cr, st)) != FHE_OK) return rc;
        }
        const u64 *msg = d_msg ? (const u64 *)d_msg + r0 * msg_stride : nullptr;
        u64 *o0 = (u64 *)d_out + r0 * n, *o1 = (u64 *)d_out + ((u64)batch + r0) * n;
        if ((rc = launch(Scheme::encrypt_label, (int)L, st, fhe::rlwe_encrypt_epilogue_kernel<Scheme::ERR, Scheme::SIGNED_MSG>, fhe_ew_grid(cr << LB), 256, key,
                         first_row + r0, R0, R1, msg, msg_stride, d_cdt, m, delta, o0, o1, L, cr, plan->mod)) != FHE_OK)
            return rc;
    }
    return FHE_OK;
}

// out = the scheme's epilogue of (c0, c1 s): c1 is staged (pointwise), then epilogue(label, c0, P, out, count) launches the
// unit's own kernel over the `count` words of a chunk
template <class Scheme, class Epilogue>
int rlwe_decrypt(const char *who, const fhe_ntt_plan *plan, const void *d_s_evals, const void *d_ct, void *d_out, size_t batch, hipStream_t st, Epilogue epilogue) {
    using fhe::u64;
    const u64 n = plan->n;
    if (batch == 0) return FHE_OK;
    if (!mul_fits((u64)batch, 2 * n, kWordLimit)) return fhe_fail(FHE_E_INVALID, "%s: batch too large", who);
    if (!d_s_evals || !d_ct || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_s_evals) || misaligned8(d_ct) || misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    const u64 out_bytes = (u64)batch * n * 8;
    if (overlaps_any(d_out, out_bytes, {{d_s_evals, n * 8}, {d_ct, 2 * out_bytes}})) return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps the key or the ciphertexts", who);
    const u64 chunk = std::min<u64>(batch, std::max<u64>(1, kChunkWords >> plan->log_n));
    void *w = nullptr;
    int rc = fhe_workspace_get(Scheme::slot, chunk * n * 8, st, &w);
    if (rc != FHE_OK) return rc;
    u64 *W = (u64 *)w;
    for (u64 r0 = 0; r0 < batch; r0 += chunk) {
        const u64 cr = std::min<u64>(chunk, batch - r0);
        const u64 *c0 = (const u64 *)d_ct + r0 * n, *c1 = nullptr;
        if ((rc = aligned_rows((const u64 *)d_ct + ((u64)batch + r0) * n, W, cr * n, st, &c1)) != FHE_OK) return rc;
        if ((rc = fhe_ntt_forward_dev(plan, c1, W, cr, st)) != FHE_OK) return rc;
        if ((rc = pointwise<1>(plan, W, (const u64 *)d_s_evals, W, nullptr, cr, st)) != FHE_OK) return rc;
        if ((rc = fhe_ntt_inverse_dev(plan, W, W, cr, st)) != FHE_OK) return rc;
        if ((rc = epilogue(Scheme::decrypt_label, c0, W, (u64 *)d_out + r0 * n, cr * n)) != FHE_OK) return rc;
    }
    return FHE_OK;
}

}  // namespace
