// rns_ext_device.hpp — the device half of the exact basis extension that bfv_rns.hip and ckks_deep.hip (§36)
// share: the word arithmetic against a modulus known at run time, and Garner's mixed-radix digits with the centring compare;
// and the index permutation of a Galois automorphism on evals (§23), which ckks_eval.hip and ckks_deep.hip share.
#pragma once
#include "zq_device.hpp"

namespace fhe {

__device__ __forceinline__ u64 ext_csub(u64 x, u64 q) { return x >= q ? x - q : x; }
// x w mod q for ANY 64-bit x and w < q < 2^63: x w - floor(x wp / 2^64) q lies in [0, 2q)
__device__ __forceinline__ u64 ext_mul(u64 x, u64 w, u64 wp, u64 q) { return ext_csub(x * w - __umul64hi(x, wp) * q, q); }
// x mod q for any 64-bit x, onep = floor(2^64 / q)
__device__ __forceinline__ u64 ext_red(u64 x, u64 q, u64 onep) { return ext_csub(x - __umul64hi(x, onep) * q, q); }

// Garner: the mixed-radix digits a of the integer in [0, M) whose canonical residues are x (x[i] for i >= s is not read into
// a digit that is used).  s (s - 1) / 2 multiplications.  -> whether the integer is above floor(M / 2).  E is a table with the
// source fields of ExtArgs (rns_tables.hpp): mq, monep, inv, invp, half, s.
template <u32 S, class E>
__device__ __forceinline__ bool ext_digits(const u64 (&x)[S], u64 (&a)[S], const E &e) {
#pragma unroll
    for (u32 i = 0; i < S; i++) {
        u64 v = x[i];
        if (i < e.s) {
            const u64 q = e.mq[i];
#pragma unroll
            for (u32 j = 0; j < i; j++) v = ext_mul(v + q - ext_red(a[j], q, e.monep[i]), e.inv[j][i], e.invp[j][i], q);   // v + q - r in (0, 2q)
        }
        a[i] = v;
    }
    bool gt = false, eq = true;
#pragma unroll
    for (u32 ii = 0; ii < S; ii++) {
        const u32 i = S - 1 - ii;
        if (i < e.s && eq && a[i] != e.half[i]) {
            gt = a[i] > e.half[i];
            eq = false;
        }
    }
    return gt;
}

// pi_g(x) of DESIGN.md §23: index x of the engine's order holds the value at psi^(2 brv_L(x) + 1), so sigma_g(a)^[x] = a^[pi_g(x)]
// with pi_g(x) = brv_L((((2 brv_L(x) + 1) g mod 2n) - 1) / 2).  2n divides 2^32, so the 32-bit product may wrap; L >= 1, so
// the shifts by 32 - L are defined.  pi_g maps an aligned block of 2^t indices onto an aligned block of 2^t indices.
__device__ __forceinline__ u32 galois_index(u32 x, u32 g, u32 L) {
    const u32 e = (2u * (__brev(x) >> (32u - L)) + 1u) * g;
    return __brev((e & ((2u << L) - 1u)) >> 1) >> (32u - L);
}

}  // namespace fhe
