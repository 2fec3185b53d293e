// tfhe_client.hip — the client side of TFHE on the device: the random stream, LWE and TGLWE encryption, and their phases
// (DESIGN.md §17).  Everything is exact and independent of launch geometry; words are u64 and wrap mod 2^64.
//
//   stream   ChaCha20 (RFC 8439: 256-bit key, 32-bit block counter, 96-bit nonce, 20 rounds).  key = the caller's 32-byte
//            seed; a row (one LWE sample, one TGLWE sample, one secret key) has the nonce (purpose, row lo, row hi), purpose
//            MASK = 1, ERR = 2, KEY = 3; block c of a row (counter c, from 0) gives 8 words, word j = u32 word 2j | u32 word
//            2j + 1 << 32; stream word i is word i mod 8 of block i div 8.
//   errors   table inversion: cdt[m] strictly increasing thresholds below 2^63; for a stream word u, r = u >> 1, the
//            magnitude is #{i : cdt[i] <= r}, negative when u & 1; the error word is the signed value << log_scale.  m = 0:
//            no error.  No floating point runs here.
//   LWE      [a_0 .. a_{n-1}, b], a_i = MASK word i of the row, b = sum a_i s_i + mu + e, e from ERR word 0 of the row
//   TGLWE    k = 1, [(A), (B)], A = MASK words 0 .. N-1 of the row, B = A S + M + E, E_i from ERR word i of the row
//   phases   b - sum a_i s_i and B - A S
// A secret key is read as 0/1 words: only bit 0 of a key word counts.
//
// tlwe_encrypt_kernel is fused: a wave owns a row, a lane a ChaCha block (8 mask words), 512 words a pass.  The key words of
// a pass are loaded coalesced and turned into eight 64-bit ballots (SGPR pairs); a lane takes the byte that covers its 8
// words, accumulates the dot product from registers, and the pass goes out through LDS so that every store instruction
// writes 512 contiguous bytes.  The mask never makes a round trip through memory.  Rows have n + 1 words, odd or even: 8-byte
// alignment and nothing more is assumed.
// TGLWE encryption is a stream fill of the masks, fhe_tn_mul_dev for A S against a broadcast copy of the key, and one
// epilogue kernel that writes A and A S + M + E (a lane generates the ChaCha block of its 8 error samples).  The kernels
// here make u64 accesses only, so callers' buffers need 8-byte alignment (a msg_stride may be odd); what goes to
// fhe_tn_mul_dev is library workspace.  Known cost: fhe_tn_mul_dev takes two [rows][N] operands, so the one key row is
// staged and forward-transformed once per row of a chunk: a third of the product's transforms and of the staging.
#include <algorithm>
#include <vector>

#include "capi_internal.hpp"
#include "chacha_stream.hpp"   // ChaChaKey, seed_key, misaligned8, chacha_block, cdt_error, CDT_MAX: shared with bfv_client.hip

using fhe::u32;
using fhe::u64;

namespace fhe {

constexpr u32 STREAM_MASK = 1, STREAM_ERR = 2, STREAM_KEY = 3;

// out [rows][row_words]: stream word i of row first_row + r under `purpose`; bits: every word AND 1.  A thread takes a block.
__global__ __launch_bounds__(256) void tfhe_stream_words_kernel(ChaChaKey key, u32 purpose, u64 first_row, u64 row_words, u64 row_blocks, u64 rows,
                                                                u32 bits, u64 *__restrict__ out) {
    const u64 total = rows * row_blocks, stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const u64 r = i / row_blocks, c = i - r * row_blocks;
        u64 w[8];
        chacha_block(key, (u32)c, purpose, first_row + r, w);
        u64 *__restrict__ dst = out + r * row_words + 8 * c;
        const u64 left = row_words - 8 * c;
#pragma unroll
        for (u32 j = 0; j < 8; j++)
            if (j < left) dst[j] = bits ? (w[j] & 1ull) : w[j];
    }
}

// a wave per row (grid-stride over rows), 512 mask words a pass; see the head of the file
constexpr int LE_TH = 64, LE_PAD = 9;   // a lane's 8 words sit 9 apart in LDS: the transposed read is conflict-free
__global__ __launch_bounds__(LE_TH) void tlwe_encrypt_kernel(ChaChaKey key, u64 first_row, const u64 *__restrict__ skey, const u64 *__restrict__ mu,
                                                             const u64 *__restrict__ cdt, u32 m, u32 log_scale, u64 *__restrict__ out, u32 n,
                                                             u64 batch) {
    __shared__ u64 stage[LE_TH * LE_PAD];
    const u32 lane = threadIdx.x;
    for (u64 row = blockIdx.x; row < batch; row += gridDim.x) {
        const u64 ridx = first_row + row;
        u64 *__restrict__ dst = out + row * ((u64)n + 1u);
        u64 acc = 0;
        for (u64 base = 0; base < n; base += 8 * LE_TH) {
            u64 mine = 0;                                     // the ballot that covers this lane's 8 words
#pragma unroll
            for (u32 q = 0; q < 8; q++) {
                const u64 idx = base + 64u * q + lane;
                const u64 bal = __ballot(idx < n && (skey[idx] & 1ull));
                mine = (lane >> 3) == q ? bal : mine;
            }
            const u32 sel = (u32)(mine >> (8u * (lane & 7u))) & 0xFFu;   // bit j: key bit of word base + 8 lane + j (0 past the row)
            if (base + 8u * lane < n) {
                u64 w[8];
                chacha_block(key, (u32)(base / 8u) + lane, STREAM_MASK, ridx, w);
#pragma unroll
                for (u32 j = 0; j < 8; j++) {
                    acc += ((sel >> j) & 1u) ? w[j] : 0ull;
                    stage[lane * LE_PAD + j] = w[j];
                }
            }
            __syncthreads();
#pragma unroll
            for (u32 q = 0; q < 8; q++) {
                const u32 t = 64u * q + lane;
                if (base + t < n) dst[base + t] = stage[t + (t >> 3)];
            }
            __syncthreads();
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
        if (lane == 0) {
            u64 e = 0;
            if (m) {
                u64 w[8];
                chacha_block(key, 0u, STREAM_ERR, ridx, w);
                e = cdt_error(cdt, m, w[0], log_scale);
            }
            dst[n] = acc + (mu ? mu[row] : 0ull) + e;
        }
    }
}

// out[row] = b - sum a_i s_i: a wave per row, coalesced reads
__global__ __launch_bounds__(LE_TH) void tlwe_phase_kernel(const u64 *__restrict__ skey, const u64 *__restrict__ in, u64 *__restrict__ out, u32 n,
                                                           u64 batch) {
    const u32 lane = threadIdx.x;
    for (u64 row = blockIdx.x; row < batch; row += gridDim.x) {
        const u64 *__restrict__ src = in + row * ((u64)n + 1u);
        u64 acc = 0;
        for (u64 i = lane; i < n; i += LE_TH) acc += (skey[i] & 1ull) ? src[i] : 0ull;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
        if (lane == 0) out[row] = src[n] - acc;
    }
}

// dst [rows][N] = src[row src_stride + i] & mask: src_stride 0 and mask 1 broadcast a key as 0/1 words, src_stride 2N
// gathers the mask rows of TGLWEs
__global__ __launch_bounds__(256) void tn_rows_copy_kernel(const u64 *__restrict__ src, u64 src_stride, u64 mask, u64 *__restrict__ dst, u32 L,
                                                           u64 rows) {
    const u64 total = rows << L, stride = (u64)gridDim.x * 256, N = 1ull << L;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) dst[i] = src[(i >> L) * src_stride + (i & (N - 1))] & mask;
}

// out[row] = (A[row], P[row] + M[row] + E[row]), E_i from ERR word i of row first_row + row; a thread takes 8 coefficients
// (one ChaCha block).  msg null: M = 0; msg_stride 0: one M for every row.
__global__ __launch_bounds__(256) void tglwe_encrypt_epilogue_kernel(ChaChaKey key, u64 first_row, const u64 *__restrict__ A, const u64 *__restrict__ P,
                                                                     const u64 *__restrict__ msg, u64 msg_stride, const u64 *__restrict__ cdt, u32 m,
                                                                     u32 log_scale, u64 *__restrict__ out, u32 L, u64 rows) {
    __shared__ u64 scdt[CDT_MAX];
    for (u32 i = threadIdx.x; i < m; i += 256) scdt[i] = cdt[i];
    __syncthreads();
    const u32 LB = L - 3u;                                       // blocks per row = N / 8
    const u64 total = rows << LB, stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const u64 r = i >> LB, c = i & ((1ull << LB) - 1u);
        u64 w[8];
        if (m) chacha_block(key, (u32)c, STREAM_ERR, first_row + r, w);
        const u64 *__restrict__ a = A + (r << L) + 8 * c, *__restrict__ p = P + (r << L) + 8 * c;
        const u64 *__restrict__ mp = msg ? msg + r * msg_stride + 8 * c : nullptr;
        u64 *__restrict__ oa = out + (r << (L + 1u)) + 8 * c, *__restrict__ ob = oa + (1ull << L);
#pragma unroll
        for (u32 j = 0; j < 8; j++) {
            oa[j] = a[j];
            ob[j] = p[j] + (mp ? mp[j] : 0ull) + (m ? cdt_error(scdt, m, w[j], log_scale) : 0ull);
        }
    }
}

// out [rows][N] = B - P, B the body rows of in [rows][2][N]
__global__ __launch_bounds__(256) void tglwe_phase_epilogue_kernel(const u64 *__restrict__ in, const u64 *__restrict__ P, u64 *__restrict__ out, u32 L,
                                                                   u64 rows) {
    const u64 total = rows << L, stride = (u64)gridDim.x * 256, N = 1ull << L;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) out[i] = in[((i >> L) << (L + 1u)) + N + (i & (N - 1))] - P[i];
}

}  // namespace fhe

// ---- host side -----------------------------------------------------------------------------------------------------
namespace {

constexpr int kClientSlot = 9;                  // fhe_workspace_get slot of the TGLWE staging rows (fhe_tn_mul_dev takes slot 1)
constexpr u64 kChunkWords = 1ull << 21;         // TGLWE rows are processed 2^21 coefficients at a time: 48 MiB of staging

// rows first_row .. first_row + rows - 1 must not wrap past 2^64
bool rows_wrap(u64 first_row, u64 rows) { return rows && first_row + (rows - 1) < first_row; }

// k = 1, 2^8 <= n = 2^L <= 2^12 (the scope of DESIGN.md §11-§16): FHE_E_INVALID otherwise
int check_client_ring(uint64_t n, unsigned k, const char *who) {
    if (k != 1 || n < 256 || n > 4096 || (n & (n - 1)) != 0)
        return fhe_fail(FHE_E_INVALID, "%s: needs k = 1 and n a power of two in [256, 4096] (n=%llu, k=%u)", who, (unsigned long long)n, k);
    return FHE_OK;
}

// the error table of a call: m <= 1024 strictly increasing thresholds below 2^63, checked on a host copy (synchronises `st`)
int check_cdt(const void *d_cdt, unsigned m, unsigned log_scale, hipStream_t st, const char *who) {
    if (log_scale > 63) return fhe_fail(FHE_E_INVALID, "%s: log_scale=%u must be at most 63", who, log_scale);
    if (m > fhe::CDT_MAX) return fhe_fail(FHE_E_INVALID, "%s: m=%u thresholds, at most %u", who, m, fhe::CDT_MAX);
    if (m == 0) return FHE_OK;
    if (!d_cdt) return fhe_fail(FHE_E_NULL, "%s: NULL error table with m=%u", who, m);
    if (misaligned8(d_cdt)) return fhe_fail(FHE_E_INVALID, "%s: d_cdt must be 8-byte aligned", who);
    std::vector<u64> t(m);
    HIP_TRY(hipMemcpyAsync(t.data(), d_cdt, (size_t)m * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (unsigned i = 0; i < m; i++)
        if (t[i] >> 63 || (i && t[i] <= t[i - 1]))
            return fhe_fail(FHE_E_INVALID, "%s: the error table must be strictly increasing and below 2^63 (entry %u)", who, i);
    return FHE_OK;
}

int stream_fill(const fhe::ChaChaKey &key, u32 purpose, u64 first_row, u64 row_words, u32 bits, u64 *d_out, u64 rows, hipStream_t st) {
    const u64 row_blocks = (row_words + 7) / 8;
    return launch("tfhe_stream_words", (int)purpose, st, fhe::tfhe_stream_words_kernel, fhe_ew_grid(rows * row_blocks), 256, key, purpose, first_row,
                  row_words, row_blocks, rows, bits, d_out);
}

int rows_copy(const u64 *src, u64 src_stride, u64 mask, u64 *dst, u32 L, u64 rows, hipStream_t st) {
    return launch("tn_rows_copy", (int)L, st, fhe::tn_rows_copy_kernel, fhe_ew_grid(rows << L), 256, src, src_stride, mask, dst, L, rows);
}

// staging of a TGLWE call: A, S (the key broadcast over a chunk as 0/1 words) and P = A S, `chunk` rows each
int tglwe_stage(uint64_t n, u32 L, const void *d_key, u64 rows, hipStream_t st, u64 *chunk, u64 **A, u64 **S, u64 **P) {
    *chunk = std::min<u64>(rows, std::max<u64>(1, kChunkWords >> L));
    void *w = nullptr;
    int rc = fhe_workspace_get(kClientSlot, 3 * *chunk * n * 8, st, &w);
    if (rc != FHE_OK) return rc;
    *A = (u64 *)w;
    *S = *A + *chunk * n;
    *P = *S + *chunk * n;
    return rows_copy((const u64 *)d_key, 0, 1ull, *S, L, *chunk, st);
}

}  // namespace

extern "C" int fhe_tfhe_stream_words_dev(const uint8_t *seed, unsigned purpose, uint64_t first_row, uint64_t row_words, unsigned flags,
                                         void *d_out, size_t rows, void *hip_stream) {
    const char *who = "fhe_tfhe_stream_words_dev";
    if (!seed) return fhe_fail(FHE_E_NULL, "%s: NULL seed", who);
    if (purpose < FHE_STREAM_MASK || purpose > FHE_STREAM_KEY)
        return fhe_fail(FHE_E_INVALID, "%s: purpose=%u is not FHE_STREAM_MASK, FHE_STREAM_ERR or FHE_STREAM_KEY", who, purpose);
    if (flags & ~FHE_STREAM_BITS) return fhe_fail(FHE_E_INVALID, "%s: unknown flags %#x", who, flags);
    if (row_words < 1 || row_words > (8ull << 32))
        return fhe_fail(FHE_E_INVALID, "%s: a row holds 1 .. 2^35 words (2^32 blocks); row_words=%llu", who, (unsigned long long)row_words);
    if (rows == 0) return FHE_OK;
    if (rows_wrap(first_row, rows)) return fhe_fail(FHE_E_INVALID, "%s: first_row + rows passes 2^64", who);
    if (!mul_fits((u64)rows, row_words + 7, kWordLimit)) return fhe_fail(FHE_E_INVALID, "%s: rows row_words is too large", who);
    if (!d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: d_out must be 8-byte aligned", who);
    return stream_fill(seed_key(seed), purpose, first_row, row_words, flags & FHE_STREAM_BITS, (u64 *)d_out, rows, (hipStream_t)hip_stream);
}

extern "C" int fhe_tlwe_encrypt_dev(unsigned n, const uint8_t *seed, uint64_t first_row, const void *d_key, const void *d_mu, const void *d_cdt,
                                    unsigned m, unsigned log_scale, void *d_out, size_t batch, void *hip_stream) {
    const char *who = "fhe_tlwe_encrypt_dev";
    if (n < 1) return fhe_fail(FHE_E_INVALID, "%s: n must be at least 1", who);
    if (!seed) return fhe_fail(FHE_E_NULL, "%s: NULL seed", who);
    if (log_scale > 63 || m > fhe::CDT_MAX)
        return fhe_fail(FHE_E_INVALID, "%s: need log_scale <= 63 and m <= %u (log_scale=%u, m=%u)", who, fhe::CDT_MAX, log_scale, m);
    if (batch == 0) return FHE_OK;
    if (rows_wrap(first_row, batch)) return fhe_fail(FHE_E_INVALID, "%s: first_row + batch passes 2^64", who);
    if (!mul_fits((u64)batch, (u64)n + 1, kWordLimit)) return fhe_fail(FHE_E_INVALID, "%s: batch too large", who);
    if (!d_key || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_key) || misaligned8(d_mu) || misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    const u64 out_bytes = (u64)batch * ((u64)n + 1) * 8;
    if (overlaps(d_out, out_bytes, d_key, (u64)n * 8) || overlaps(d_out, out_bytes, d_mu, (u64)batch * 8) ||
        overlaps(d_out, out_bytes, d_cdt, (u64)m * 8))
        return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps the key, the messages or the error table", who);
    hipStream_t st = (hipStream_t)hip_stream;
    int rc = check_cdt(d_cdt, m, log_scale, st, who);
    if (rc != FHE_OK) return rc;
    return launch("tlwe_encrypt", (int)std::min<u64>(n, 1u << 20), st, fhe::tlwe_encrypt_kernel, (unsigned)std::min<u64>(batch, 1u << 16), fhe::LE_TH,
                  seed_key(seed), first_row, d_key, d_mu, d_cdt, m, log_scale, d_out, n, batch);
}

extern "C" int fhe_tlwe_phase_dev(unsigned n, const void *d_key, const void *d_in, void *d_out, size_t batch, void *hip_stream) {
    const char *who = "fhe_tlwe_phase_dev";
    if (n < 1) return fhe_fail(FHE_E_INVALID, "%s: n must be at least 1", who);
    if (batch == 0) return FHE_OK;
    if (!mul_fits((u64)batch, (u64)n + 1, kWordLimit)) return fhe_fail(FHE_E_INVALID, "%s: batch too large", who);
    if (!d_key || !d_in || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_key) || misaligned8(d_in) || misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    const u64 out_bytes = (u64)batch * 8;
    if (overlaps(d_out, out_bytes, d_key, (u64)n * 8) || overlaps(d_out, out_bytes, d_in, (u64)batch * ((u64)n + 1) * 8))
        return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps the key or the input", who);
    hipStream_t st = (hipStream_t)hip_stream;
    return launch("tlwe_phase", (int)std::min<u64>(n, 1u << 20), st, fhe::tlwe_phase_kernel, (unsigned)std::min<u64>(batch, 1u << 16), fhe::LE_TH, d_key,
                  d_in, d_out, n, batch);
}

extern "C" int fhe_tglwe_encrypt_dev(uint64_t n, unsigned k, const uint8_t *seed, uint64_t first_row, const void *d_key, const void *d_msg,
                                     size_t msg_stride, const void *d_cdt, unsigned m, unsigned log_scale, void *d_out, size_t rows,
                                     void *hip_stream) {
    const char *who = "fhe_tglwe_encrypt_dev";
    int rc = check_client_ring(n, k, who);
    if (rc != FHE_OK) return rc;
    if (!seed) return fhe_fail(FHE_E_NULL, "%s: NULL seed", who);
    if (log_scale > 63 || m > fhe::CDT_MAX)
        return fhe_fail(FHE_E_INVALID, "%s: need log_scale <= 63 and m <= %u (log_scale=%u, m=%u)", who, fhe::CDT_MAX, log_scale, m);
    if (d_msg && msg_stride != 0 && msg_stride < n) return fhe_fail(FHE_E_INVALID, "%s: msg_stride must be 0 (one message) or at least n", who);
    if (rows == 0) return FHE_OK;
    if (rows_wrap(first_row, rows)) return fhe_fail(FHE_E_INVALID, "%s: first_row + rows passes 2^64", who);
    if (!mul_fits((u64)rows, 2 * n, kWordLimit) || !mul_fits((u64)rows - 1, (u64)msg_stride, kWordLimit - n))
        return fhe_fail(FHE_E_INVALID, "%s: rows or msg_stride too large", who);
    if (!d_key || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_key) || misaligned8(d_msg) || misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    const u64 out_bytes = (u64)rows * 2 * n * 8, msg_bytes = (((u64)rows - 1) * msg_stride + n) * 8;
    if (overlaps(d_out, out_bytes, d_key, n * 8) || overlaps(d_out, out_bytes, d_msg, msg_bytes) || overlaps(d_out, out_bytes, d_cdt, (u64)m * 8))
        return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps the key, the messages or the error table", who);
    hipStream_t st = (hipStream_t)hip_stream;
    if ((rc = check_cdt(d_cdt, m, log_scale, st, who)) != FHE_OK) return rc;
    const u32 L = (u32)__builtin_ctzll(n);
    const fhe::ChaChaKey key = seed_key(seed);
    u64 chunk = 0, *A = nullptr, *S = nullptr, *P = nullptr;
    if ((rc = tglwe_stage(n, L, d_key, rows, st, &chunk, &A, &S, &P)) != FHE_OK) return rc;
    for (u64 r0 = 0; r0 < rows; r0 += chunk) {
        const u64 cr = std::min<u64>(chunk, rows - r0);
        if ((rc = stream_fill(key, fhe::STREAM_MASK, first_row + r0, n, 0, A, cr, st)) != FHE_OK) return rc;
        if ((rc = fhe_tn_mul_dev(n, A, S, P, cr, st)) != FHE_OK) return rc;
        const u64 *msg = d_msg ? (const u64 *)d_msg + r0 * msg_stride : nullptr;
        if ((rc = launch("tglwe_encrypt_epilogue", (int)L, st, fhe::tglwe_encrypt_epilogue_kernel, fhe_ew_grid(cr << (L - 3)), 256, key, first_row + r0, A,
                         P, msg, msg_stride, d_cdt, m, log_scale, (u64 *)d_out + r0 * 2 * n, L, cr)) != FHE_OK)
            return rc;
    }
    return FHE_OK;
}

extern "C" int fhe_tglwe_phase_dev(uint64_t n, unsigned k, const void *d_key, const void *d_in, void *d_out, size_t rows, void *hip_stream) {
    const char *who = "fhe_tglwe_phase_dev";
    int rc = check_client_ring(n, k, who);
    if (rc != FHE_OK) return rc;
    if (rows == 0) return FHE_OK;
    if (!mul_fits((u64)rows, 2 * n, kWordLimit)) return fhe_fail(FHE_E_INVALID, "%s: rows too large", who);
    if (!d_key || !d_in || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_key) || misaligned8(d_in) || misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    const u64 out_bytes = (u64)rows * n * 8;
    if (overlaps(d_out, out_bytes, d_key, n * 8) || overlaps(d_out, out_bytes, d_in, 2 * out_bytes))
        return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps the key or the input", who);
    hipStream_t st = (hipStream_t)hip_stream;
    const u32 L = (u32)__builtin_ctzll(n);
    u64 chunk = 0, *A = nullptr, *S = nullptr, *P = nullptr;
    if ((rc = tglwe_stage(n, L, d_key, rows, st, &chunk, &A, &S, &P)) != FHE_OK) return rc;
    for (u64 r0 = 0; r0 < rows; r0 += chunk) {
        const u64 cr = std::min<u64>(chunk, rows - r0);
        const u64 *src = (const u64 *)d_in + r0 * 2 * n;
        if ((rc = rows_copy(src, 2 * n, ~0ull, A, L, cr, st)) != FHE_OK) return rc;
        if ((rc = fhe_tn_mul_dev(n, A, S, P, cr, st)) != FHE_OK) return rc;
        if ((rc = launch("tglwe_phase_epilogue", (int)L, st, fhe::tglwe_phase_epilogue_kernel, fhe_ew_grid(cr << L), 256, src, P, (u64 *)d_out + r0 * n, L,
                         cr)) != FHE_OK)
            return rc;
    }
    return FHE_OK;
}
