// host_tables.hpp — the host arithmetic behind every table the library uploads, once: modular powers and inverses, the
// forms a twiddle w is stored in (Shoup pairs in 64 and 32 bits, the pseudo-Mersenne and word-Montgomery pairs), the word
// inverse of the 32-bit Montgomery kernels, bit reversal, and the 136-word table of round0_bits.  Plain C++17, no HIP:
// host/test_host_tables.cpp checks each of these against its definition without the library.  A pair is returned as the
// caller's type P = {w, wp} (fhe::Tw, fhe::Tw32), which this header does not need to know.
#pragma once
#include <array>
#include <cstdint>

namespace fhe {
namespace host {

typedef unsigned long long u64;   // as fhe::u64 (zq_device.hpp)
typedef unsigned __int128 u128;

inline u64 mulmod(u64 a, u64 b, u64 q) { return (u64)(((u128)a * b) % q); }

// ntt.rs:164-179 const_exp_mod
inline u64 exp_mod(u64 q, u64 x, u64 k) {
    u64 r = 1;
    x %= q;
    while (k > 0) {
        if (k & 1) r = mulmod(r, x, q);
        x = mulmod(x, x, q);
        k >>= 1;
    }
    return r;
}
// ntt.rs:182-185 const_inv_mod (Fermat; q assumed prime as in the reference)
inline u64 inv_mod(u64 q, u64 x) { return exp_mod(q, x, q - 2); }

inline u64 bitrev(u64 i, unsigned log_n) {
    u64 r = 0;
    for (unsigned b = 0; b < log_n; b++) r |= ((i >> b) & 1ull) << (log_n - 1 - b);
    return r;
}

// {w, floor(w 2^64 / q)}: what the Shoup product multiplies by
inline u64 shoup(u64 w, u64 q) { return (u64)((((u128)w) << 64) / q); }
template <class P>
P shoup_pair(u64 w, u64 q) { return P{w, shoup(w, q)}; }
// the same in 32-bit words, {w, floor(w 2^32 / q)}, for w < q < 2^32
template <class P>
P shoup32_pair(u64 w, u64 q) { return P{(uint32_t)w, (uint32_t)((w << 32) / q)}; }
// pseudo-Mersenne moduli: {w, w 2^32 mod q} (zq_device.hpp)
template <class P>
P pm_pair(u64 w, u64 q) { return P{w, mulmod(w, 1ull << 32, q)}; }
// q = 1 (mod 2^32), word Montgomery: {w 2^32, w 2^64 mod q}
template <class P>
P mg_pair(u64 w, u64 q) {
    const u64 w32 = mulmod(w, 1ull << 32, q);
    return P{w32, mulmod(w32, 1ull << 32, q)};
}

// -(q^-1) mod 2^32 for an odd word q, by Newton's iteration: q itself has 3 correct bits, doubled per step
inline uint32_t neg_inv32(uint32_t q) {
    uint32_t inv = q;
    for (int it = 0; it < 5; it++) inv *= 2u - q * inv;
    return 0u - inv;
}

// Tables for transforms of 0/1 polynomials (gadget digits): the outcomes of the first stages per input bit pattern
// (ntt_rounds.hpp: round0_bits), from r = roots[0..7] modulo q (so n >= 8).  W is the word the kernels read: u64 for the
// plans, uint32_t for the 27-bit primes.  [0,64): 16 patterns x 4 outputs of stages 0-1; [64,128): those times roots[4+j]
// (stage 2's products); [128,136): 4 patterns x 2 outputs of one stage with roots[1].
template <class W>
std::array<W, 136> bit_lut(const u64 *r, u64 q) {
    std::array<W, 136> lut{};
    auto add = [&](u64 x, u64 y) { u64 s = x + y; return s >= q ? s - q : s; };
    auto sub = [&](u64 x, u64 y) { return x >= y ? x - y : x + q - y; };
    for (unsigned p = 0; p < 16; p++) {
        const u64 x0 = p & 1, x1 = (p >> 1) & 1, x2 = (p >> 2) & 1, x3 = (p >> 3) & 1;   // registers c, c+4, c+8, c+12
        const u64 a0 = add(x0, mulmod(r[1], x2, q)), a2 = sub(x0, mulmod(r[1], x2, q));   // stage 0: pairs (c, c+8), (c+4, c+12)
        const u64 a1 = add(x1, mulmod(r[1], x3, q)), a3 = sub(x1, mulmod(r[1], x3, q));
        u64 y[4];
        y[0] = add(a0, mulmod(r[2], a1, q)); y[1] = sub(a0, mulmod(r[2], a1, q));         // stage 1: (c, c+4) with roots[2]
        y[2] = add(a2, mulmod(r[3], a3, q)); y[3] = sub(a2, mulmod(r[3], a3, q));         //          (c+8, c+12) with roots[3]
        for (int j = 0; j < 4; j++) {
            lut[4 * p + j] = (W)y[j];
            lut[64 + 4 * p + j] = (W)mulmod(r[4 + j], y[j], q);                           // stage 2's products
        }
    }
    for (unsigned p = 0; p < 4; p++) {
        const u64 x = p & 1, y = (p >> 1) & 1;
        lut[128 + 2 * p] = (W)add(x, mulmod(r[1], y, q));
        lut[128 + 2 * p + 1] = (W)sub(x, mulmod(r[1], y, q));
    }
    return lut;
}

}  // namespace host
}  // namespace fhe
