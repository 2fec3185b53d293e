// digit32.hpp — internal interface of the 27-bit-prime external product (digit32.hip).  Not part of the public boundary.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ntt_kernels.hpp"

namespace fhe {


// the two primes: the largest below 2^32 / 25 with p = 1 mod 2^15 (27.36 and 27.35 bits; product 2^54.7).  Below
// 2^32 / 25 so that up to twelve lazy butterfly stages need no conditional subtraction (digit32.hip: ct32_loose).
constexpr uint32_t kExt32PrimeA = 0x0a3c8001u, kExt32PrimeB = 0x0a320001u;
// the next one down, for the products that need three (bfv32.hip: relinearisation, integers below 2^82)
constexpr uint32_t kExt32PrimeC = 0x0a318001u;
static_assert((uint64_t)kExt32PrimeA * 25 < (1ull << 32) && kExt32PrimeA > kExt32PrimeB && kExt32PrimeA - kExt32PrimeB < kExt32PrimeB, "prime bounds");

struct Ext32Args {
    // key preparation
    const u64 *key64;          // [T][key_k1][n] 64-bit words (the key as the reference holds it)
    uint32_t *key32;           // [prime][T][half][key_k1][n], NTT domain
    u64 rows;                  // T * 2 * key_k1
    uint32_t key_k1;
    uint32_t sel_count;        // SRC32_GSEL: prepared keys at key32 (a selector >= sel_count contributes 0); in key_k1's padding word
    // product
    const u64 *src;            // ciphertexts, source row r of ciphertext b at src + b*ct_stride + r*n
    u64 ct_stride;
    uint32_t *part32;          // [batch][parts][prime][NC][n] canonical partial sums
    u64 *out;                  // [batch][k+1][n]
    u64 batch;
    uint32_t l, T, parts, tpp;
    // per prime
    const Tw32 *tw_fwd[3], *tw_inv[3];
    const uint32_t *lut[3];
    uint32_t p[3];             // kExt32PrimeA, B, C (digit32.hip uses the first two)
    u64 mu[3];                 // floor(2^64 / p)
    uint32_t bq[3];            // floor(2^32 / p)
    Tw32 ninv[3];              // n^-1 mod p
    Tw32 crt;                  // pA^-1 mod pB
    Tw32 crt_ac, crt_bc;       // pA^-1 mod pC, pB^-1 mod pC (Garner's third digit)
    u64 P, halfP;              // pA * pB, ceil(P / 2)
    // key switching tail (digit_tail32_ks_kernel)
    Mod mod;                   // the ring's q
    u64 two32;                 // 2^32 mod q
    union {
        const u64 *glwe;       // the ciphertexts again, for the body row
        const u64 *src1;       // SRC32_GSEL: the second CMux input c1, laid out as src (the source row is c1 - c0)
    };
    uint32_t k;
    uint32_t log_beta;         // SRC32_GADGET / SRC32_GCMUX: b of the base 2^b; in k's padding word
    // several keys in one preparation launch (gridDim.z keys): key z at key64 + z*key_stride64, key32 + z*key_stride32
    u64 key_stride64, key_stride32;
    // SRC32_CMUX (blind rotation step): ciphertext b's source row r is rot(src_r, e_b) - src_r, e_b = shift[b*shift_stride]
    // SRC32_GSEL (CMux with a selector per ciphertext): ciphertext b's key is key32 + sel[b*shift_stride]
    // * key_stride32; src holds c0, src1 c1, and the tail writes c0 + lift.  The three pointers share their words with
    // fields the mode does not use, so the layout of every other mode is unchanged.
    union {
        const uint32_t *shift;
        const uint32_t *sel;
    };
    u64 shift_stride;
};

// source modes of digit_mac32_kernel next to SRC_DIGITS / SRC_ZQBITS (ntt_kernels.hpp): the digits of X^-e ACC - ACC;
// the signed base-2^b digits of DESIGN.md §11 of the rows (SRC32_GADGET) or of X^-e ACC - ACC (SRC32_GCMUX); the same
// digits of c1 - c0 against a key chosen per ciphertext (SRC32_GSEL)
enum : int { SRC32_CMUX = 4, SRC32_GADGET = 5, SRC32_GCMUX = 6, SRC32_GSEL = 7 };

bool ext32_shape_supported(u64 n, unsigned k, unsigned l);        // TGGSW x TGLWE
bool ks32_shape_supported(u64 n, unsigned k, unsigned l);         // GLWE::key_switch, base 2
// the base-2^b gadget product: k = 1, 2^8 <= n <= 2^12, 1 <= b, b l <= 64, and the half-sum bound
// (k+1) l n (2^32 - 1) 2^(b-1) below P / 2
// digit_d(w) + 2^(b-1) = ((w + cadd) >> (64 - b (d+1))) & (2^b - 1) with cadd = the rounding bit 2^(s-1) (s = 64 - b l > 0)
// plus the balancing constant B 2^s = sum_{d<l} 2^(63 - b d): every level's digit without a carry chain
__host__ __device__ inline u64 gadget_cadd(uint32_t b, uint32_t l) {
    const uint32_t s = 64u - b * l;
    u64 c = s ? 1ull << (s - 1u) : 0ull;
    for (uint32_t d = 0; d < l; d++) c += 1ull << (63u - b * d);
    return c;
}
bool ext32_gadget_supported(u64 n, unsigned k, unsigned log_beta, unsigned l);
uint32_t ext32_units(int log_n);                                   // digits per step of the fused kernel
// parts (workgroups per ciphertext) and digits per part of the fused kernel for `batch` ciphertexts of T digit rows;
// shared by the external product and the blind rotation's CMux steps
void ext32_split(u64 n, u64 batch, uint32_t T, uint32_t *parts, uint32_t *tpp);
// the same for the gadget modes, whose T = (k+1) l is a few steps of ext32_units digits
void ext32_gadget_split(u64 n, u64 batch, uint32_t T, uint32_t *parts, uint32_t *tpp);
hipError_t launch_ext32_key(const Ext32Args &a, int log_n, hipStream_t st);
hipError_t launch_ext32_mac(const Ext32Args &a, int log_n, int src_kind, hipStream_t st);
hipError_t launch_ext32_tail(const Ext32Args &a, int log_n, hipStream_t st);
hipError_t launch_ext32_tail_ks(const Ext32Args &a, int log_n, hipStream_t st);
hipError_t launch_ext32_tail_cmux(const Ext32Args &a, int log_n, hipStream_t st);   // out[b] += lift (in place)
hipError_t launch_ext32_tail_sel(const Ext32Args &a, int log_n, hipStream_t st);    // out[b] = src[b] + lift (SRC32_GSEL)
hipError_t launch_ext32_key_many(const Ext32Args &a, int log_n, u64 keys, hipStream_t st);   // `keys` TGGSWs, strides above

}  // namespace fhe
