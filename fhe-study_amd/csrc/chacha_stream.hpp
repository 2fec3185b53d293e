// chacha_stream.hpp — the random stream and the error sampler that the client-side units share (tfhe_client.hip, DESIGN.md
// §17; bfv_client.hip, §20): the ChaCha20 block function (RFC 8439) keyed by the caller's 32-byte seed with the nonce
// (purpose, row lo, row hi), and the table-inversion error sampler; the words are defined in §17.  And the two host helpers
// every client entry point starts with: the seed as a key, and the 8-byte alignment the client ABI promises.
#pragma once
#include <cstdint>

#include "zq_device.hpp"

namespace fhe {

constexpr u32 CDT_MAX = 1024;

struct ChaChaKey { u32 w[8]; };   // by value: the seed sits in SGPRs

__device__ __forceinline__ u32 rotl32(u32 x, u32 r) { return (x << r) | (x >> (32u - r)); }
__device__ __forceinline__ void chacha_qr(u32 &a, u32 &b, u32 &c, u32 &d) {
    a += b; d ^= a; d = rotl32(d, 16);
    c += d; b ^= c; b = rotl32(b, 12);
    a += b; d ^= a; d = rotl32(d, 8);
    c += d; b ^= c; b = rotl32(b, 7);
}
// block `counter` of row `row` under `purpose` -> the 8 stream words of the block
__device__ __forceinline__ void chacha_block(const ChaChaKey &key, u32 counter, u32 purpose, u64 row, u64 (&out)[8]) {
    const u32 in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key.w[0], key.w[1], key.w[2], key.w[3],
                        key.w[4], key.w[5], key.w[6], key.w[7], counter, purpose, (u32)row, (u32)(row >> 32)};
    u32 x0 = in[0], x1 = in[1], x2 = in[2], x3 = in[3], x4 = in[4], x5 = in[5], x6 = in[6], x7 = in[7], x8 = in[8], x9 = in[9], x10 = in[10],
        x11 = in[11], x12 = in[12], x13 = in[13], x14 = in[14], x15 = in[15];
    for (int r = 0; r < 10; r++) {
        chacha_qr(x0, x4, x8, x12); chacha_qr(x1, x5, x9, x13); chacha_qr(x2, x6, x10, x14); chacha_qr(x3, x7, x11, x15);
        chacha_qr(x0, x5, x10, x15); chacha_qr(x1, x6, x11, x12); chacha_qr(x2, x7, x8, x13); chacha_qr(x3, x4, x9, x14);
    }
    out[0] = (u64)(x0 + in[0]) | ((u64)(x1 + in[1]) << 32);
    out[1] = (u64)(x2 + in[2]) | ((u64)(x3 + in[3]) << 32);
    out[2] = (u64)(x4 + in[4]) | ((u64)(x5 + in[5]) << 32);
    out[3] = (u64)(x6 + in[6]) | ((u64)(x7 + in[7]) << 32);
    out[4] = (u64)(x8 + in[8]) | ((u64)(x9 + in[9]) << 32);
    out[5] = (u64)(x10 + in[10]) | ((u64)(x11 + in[11]) << 32);
    out[6] = (u64)(x12 + in[12]) | ((u64)(x13 + in[13]) << 32);
    out[7] = (u64)(x14 + in[14]) | ((u64)(x15 + in[15]) << 32);
}

// the error word of stream word u: magnitude #{i < m : cdt[i] <= u >> 1} (the table is strictly increasing: a binary search),
// negative when u & 1, shifted left by log_scale
__device__ __forceinline__ u64 cdt_error(const u64 *cdt, u32 m, u64 u, u32 log_scale) {
    const u64 r = u >> 1;
    u32 lo = 0, hi = m;
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (cdt[mid] <= r) lo = mid + 1; else hi = mid;
    }
    const u64 mag = lo;
    return ((u & 1u) ? 0ull - mag : mag) << log_scale;
}

}  // namespace fhe

// ---- host side -----------------------------------------------------------------------------------------------------
namespace {

// the caller's 32 bytes as the key's little-endian words
inline fhe::ChaChaKey seed_key(const uint8_t *seed) {
    fhe::ChaChaKey k;
    for (int i = 0; i < 8; i++)
        k.w[i] = (fhe::u32)seed[4 * i] | ((fhe::u32)seed[4 * i + 1] << 8) | ((fhe::u32)seed[4 * i + 2] << 16) | ((fhe::u32)seed[4 * i + 3] << 24);
    return k;
}
// the client kernels make u64 accesses only
inline bool misaligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) != 0; }

}  // namespace
