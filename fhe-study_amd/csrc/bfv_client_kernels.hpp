// bfv_client_kernels.hpp — what the RLWE client units share (bfv_client.hip; ckks_client.hip, §21): the
// sampling kernels over the ChaCha20 stream of chacha_stream.hpp (uniform rows modulo Q, the ternary / bit rows), the
// broadcast pointwise product against a key, the key broadcast of the staged route, and the host helpers that launch and
// check them.  A kernel can only be launched from the translation unit that defines it, so the kernels are `static` here
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

}  // namespace fhe

// ---- host side -----------------------------------------------------------------------------------------------------
namespace {

constexpr fhe::u64 kChunkWords = 1ull << 21;         // ciphertexts are processed 2^21 coefficients at a time: 32 MiB of staging
constexpr fhe::u64 kRowLimit = 1ull << 63;           // error rows are 2 r and 2 r + 1

inline bool misaligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) != 0; }

inline fhe::ChaChaKey seed_key(const uint8_t *seed) {
    fhe::ChaChaKey k;
    for (int i = 0; i < 8; i++)
        k.w[i] = (fhe::u32)seed[4 * i] | ((fhe::u32)seed[4 * i + 1] << 8) | ((fhe::u32)seed[4 * i + 2] << 16) | ((fhe::u32)seed[4 * i + 3] << 24);
    return k;
}

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

}  // namespace
