// rns_tables.hpp — the host tables of the exact basis extension (bfv_rns.hip): Garner's inverses, the
// mixed-radix digits of floor(M / 2), the weights of the Horner sums, and the small multi-word integers they are made with.
// Plain C++17, no HIP: host/test_rns_tables.cpp checks each of these against its definition without the library.
#pragma once
#include <cstdint>
#include <vector>

#include "host_tables.hpp"

namespace fhe {

constexpr unsigned kExtMax = 9;            // the most source or target moduli of one extension
constexpr unsigned long long kExtModLimit = 1ull << 62;

// What the extension kernel needs of the source moduli m_0 .. m_{s-1} (M their product) and the targets p_0 .. p_{t-1}, by
// value: indexed by unrolled constants only.  A pair {w, wp} is w and floor(w 2^64 / modulus), the Shoup companion.
//   digits   x = a_0 + a_1 m_0 + a_2 m_0 m_1 + ..., 0 <= a_i < m_i; a_i = (..((x_i - a_0) inv[0][i] - a_1) inv[1][i] ..) mod m_i
//   half     the digits of floor(M / 2): x > floor(M / 2) exactly when its digits are greater, compared from the top
//   W[j][t]  m_0 .. m_{j-1} mod p_t, so x = sum_j a_j W[j][t] mod p_t; pM[t] = M mod p_t, subtracted for a centred x above half
template <unsigned S, unsigned T>
struct ExtArgs {
    unsigned long long mq[S], monep[S];              // m_i, floor(2^64 / m_i)
    unsigned long long inv[S][S], invp[S][S];        // [j][i], j < i: m_j^-1 mod m_i and its companion
    unsigned long long half[S];
    unsigned long long pq[T], ponep[T], pr64[T], pr64p[T], pM[T];   // p_t, floor(2^64 / p_t), 2^64 mod p_t and its companion, M mod p_t
    unsigned long long W[S][T];
    uint32_t s, t;
};

namespace host {

// a non-negative integer in 64-bit words, least significant first, no leading zero word
struct Big {
    std::vector<u64> w;
    Big() = default;
    explicit Big(u64 x) { if (x) w.push_back(x); }
    void trim() { while (!w.empty() && w.back() == 0) w.pop_back(); }
    void mul(u64 x) {
        u64 carry = 0;
        for (u64 &d : w) {
            const u128 p = (u128)d * x + carry;
            d = (u64)p;
            carry = (u64)(p >> 64);
        }
        if (carry) w.push_back(carry);
        trim();
    }
    void add(u64 x) {
        for (size_t i = 0; x && i < w.size(); i++) {
            const u64 s = w[i] + x;
            x = s < x ? 1 : 0;
            w[i] = s;
        }
        if (x) w.push_back(x);
    }
    // this = floor(this / x), returns the remainder; x != 0
    u64 divmod(u64 x) {
        u64 rem = 0;
        for (size_t i = w.size(); i-- > 0;) {
            const u128 cur = ((u128)rem << 64) | w[i];
            w[i] = (u64)(cur / x);
            rem = (u64)(cur % x);
        }
        trim();
        return rem;
    }
    u64 mod(u64 x) const {
        u64 rem = 0;
        for (size_t i = w.size(); i-- > 0;) rem = (u64)((((u128)rem << 64) | w[i]) % x);
        return rem;
    }
    // -1, 0, 1
    int cmp(const Big &o) const {
        if (w.size() != o.w.size()) return w.size() < o.w.size() ? -1 : 1;
        for (size_t i = w.size(); i-- > 0;)
            if (w[i] != o.w[i]) return w[i] < o.w[i] ? -1 : 1;
        return 0;
    }
};

inline Big big_product(const u64 *m, unsigned count) {
    Big p(1);
    for (unsigned i = 0; i < count; i++) p.mul(m[i]);
    return p;
}

// a x for a 128-bit x: a lo + 2^64 (a hi), the second product added one word up
inline Big big_mul128(const Big &a, u128 x) {
    Big lo = a, hi = a;
    lo.mul((u64)x);
    hi.mul((u64)(x >> 64));
    u64 carry = 0;
    for (size_t i = 0; i < hi.w.size() || carry; i++) {
        if (lo.w.size() <= i + 1) lo.w.resize(i + 2, 0);
        const u128 s = (u128)lo.w[i + 1] + (i < hi.w.size() ? hi.w[i] : 0) + carry;
        lo.w[i + 1] = (u64)s;
        carry = (u64)(s >> 64);
    }
    lo.trim();
    return lo;
}

// The admission of the BFV products: B > t n Q W + 1, B the product of aux[0 .. na), Q of mods[0 .. nq),
// W the sum of the absolute weights of an inner product (1 for a single product; at most 64 (2^61 - 1), so 128 bits).  Exact.
inline bool bfv_admits(const u64 *aux, unsigned na, const u64 *mods, unsigned nq, u64 t, u64 n, u128 W) {
    Big rhs = big_product(mods, nq);
    rhs.mul(t);
    rhs.mul(n);
    rhs = big_mul128(rhs, W);
    rhs.add(1);
    return big_product(aux, na).cmp(rhs) > 0;
}

// x^-1 mod m by the extended Euclidean algorithm, for any m >= 2; false where gcd(x, m) != 1
inline bool inv_mod_any(u64 x, u64 m, u64 *out) {
    typedef __int128 i128;
    i128 r0 = (i128)m, r1 = (i128)(x % m), t0 = 0, t1 = 1;
    while (r1 != 0) {
        const i128 qt = r0 / r1, r2 = r0 - qt * r1, t2 = t0 - qt * t1;
        r0 = r1; r1 = r2; t0 = t1; t1 = t2;
    }
    if (r0 != 1) return false;
    *out = (u64)(t0 < 0 ? t0 + (i128)m : t0);
    return true;
}

// the moduli of one side of an extension: 1 .. max of them, each odd, at least 3 and below 2^62, pairwise coprime
inline bool ext_moduli_ok(const u64 *m, unsigned count, unsigned max) {
    if (count < 1 || count > max) return false;
    for (unsigned i = 0; i < count; i++) {
        if (m[i] < 3 || (m[i] & 1) == 0 || m[i] >= kExtModLimit) return false;
        for (unsigned j = 0; j < i; j++) {
            u64 inv;
            if (m[j] == m[i] || !inv_mod_any(m[j] % m[i], m[i], &inv)) return false;
        }
    }
    return true;
}

// the tables of the extension from src[0 .. s) to dst[0 .. t); false where a side is not ext_moduli_ok (nothing usable is
// left in *e).  The targets need not be coprime to the sources.
template <unsigned S, unsigned T>
bool ext_tables(const u64 *src, unsigned s, const u64 *dst, unsigned t, ExtArgs<S, T> *e) {
    *e = ExtArgs<S, T>{};
    if (!ext_moduli_ok(src, s, S) || t < 1 || t > T) return false;
    for (unsigned i = 0; i < t; i++)
        if (dst[i] < 3 || (dst[i] & 1) == 0 || dst[i] >= kExtModLimit) return false;
    e->s = s;
    e->t = t;
    for (unsigned i = 0; i < s; i++) {
        e->mq[i] = src[i];
        e->monep[i] = (u64)((((u128)1) << 64) / src[i]);
        for (unsigned j = 0; j < i; j++) {
            if (!inv_mod_any(src[j] % src[i], src[i], &e->inv[j][i])) return false;
            e->invp[j][i] = shoup(e->inv[j][i], src[i]);
        }
    }
    Big h = big_product(src, s);
    h.divmod(2);                                                     // floor(M / 2)
    for (unsigned i = 0; i < s; i++) e->half[i] = h.divmod(src[i]);   // its mixed-radix digits, least significant first
    for (unsigned k = 0; k < t; k++) {
        const u64 p = dst[k];
        e->pq[k] = p;
        e->ponep[k] = (u64)((((u128)1) << 64) / p);
        e->pr64[k] = (u64)((((u128)1) << 64) % p);
        e->pr64p[k] = shoup(e->pr64[k], p);
        u64 w = 1 % p;
        for (unsigned j = 0; j < s; j++) {
            e->W[j][k] = w;
            w = mulmod(w, src[j] % p, p);
        }
        e->pM[k] = w;
    }
    return true;
}

}  // namespace host

// ---- the grouped-digit key switch of the deep CKKS chain (ckks_deep.hip) -------------------------------------
constexpr unsigned kDeepMaxLimbs = 32, kDeepMaxSpecials = 8, kDeepMaxTargets = kDeepMaxLimbs + kDeepMaxSpecials;

// The source side of one extension from a digit group (or from the special primes) of 1 .. 8 moduli: what Garner's digits and
// the centring need, ExtArgs' fields of the same names.  By value, indexed by unrolled constants only.
struct DeepSrc {
    unsigned long long mq[kDeepMaxSpecials], monep[kDeepMaxSpecials];
    unsigned long long inv[kDeepMaxSpecials][kDeepMaxSpecials], invp[kDeepMaxSpecials][kDeepMaxSpecials];
    unsigned long long half[kDeepMaxSpecials];
    uint32_t s;
};
// One target of that extension, an entry of a device table: p, floor(2^64 / p), 2^64 mod p and its companion, M mod p, the
// place of the target's residues in the destination (in units the launch names) and the radix weights m_0 .. m_{j-1} mod p.
struct DeepTarget {
    unsigned long long q, onep, r64, r64p, pM, off;
    unsigned long long W[kDeepMaxSpecials];
};

namespace host {

// digit groups of `limbs` limbs in groups of alpha: group j holds limbs [j alpha, min((j + 1) alpha, limbs))
inline unsigned deep_groups(unsigned limbs, unsigned alpha) { return (limbs + alpha - 1) / alpha; }

// The admission of the grouped key switch: P >= Q_j for every digit group j of q[0 .. limbs), P the product of p[0 .. alpha),
// Q_j that of the group's primes.  Exact: both sides are products of at most eight words.
inline bool deep_admits(const u64 *q, unsigned limbs, const u64 *p, unsigned alpha) {
    if (alpha < 1 || alpha > kDeepMaxSpecials) return false;
    const Big P = big_product(p, alpha);
    for (unsigned j0 = 0; j0 < limbs; j0 += alpha)
        if (P.cmp(big_product(q + j0, limbs - j0 < alpha ? limbs - j0 : alpha)) < 0) return false;
    return true;
}

// the tables of the centred extension from src[0 .. s), s <= 8, to dst[0 .. t), target k's residues at off[k]; false where a
// side is not ext_moduli_ok's kind (nothing usable is left).  tab holds t entries.
inline bool deep_ext_tables(const u64 *src, unsigned s, const u64 *dst, const u64 *off, unsigned t, DeepSrc *e, DeepTarget *tab) {
    *e = DeepSrc{};
    if (!ext_moduli_ok(src, s, kDeepMaxSpecials)) return false;
    for (unsigned k = 0; k < t; k++)
        if (dst[k] < 3 || (dst[k] & 1) == 0 || dst[k] >= kExtModLimit) return false;
    e->s = s;
    for (unsigned i = 0; i < s; i++) {
        e->mq[i] = src[i];
        e->monep[i] = (u64)((((u128)1) << 64) / src[i]);
        for (unsigned j = 0; j < i; j++) {
            if (!inv_mod_any(src[j] % src[i], src[i], &e->inv[j][i])) return false;
            e->invp[j][i] = shoup(e->inv[j][i], src[i]);
        }
    }
    Big h = big_product(src, s);
    h.divmod(2);
    for (unsigned i = 0; i < s; i++) e->half[i] = h.divmod(src[i]);
    for (unsigned k = 0; k < t; k++) {
        const u64 p = dst[k];
        DeepTarget &d = tab[k];
        d = DeepTarget{};
        d.q = p;
        d.onep = (u64)((((u128)1) << 64) / p);
        d.r64 = (u64)((((u128)1) << 64) % p);
        d.r64p = shoup(d.r64, p);
        d.off = off[k];
        u64 w = 1 % p;
        for (unsigned j = 0; j < s; j++) {
            d.W[j] = w;
            w = mulmod(w, src[j] % p, p);
        }
        d.pM = w;
    }
    return true;
}

}  // namespace host

// ---- scalar sums and inner products on the deep chain (ckks_deep.hip) ----------------------------------------
// One launch covers a slice of up to kDeepPolyLimbs limbs (blockIdx.y); a scalar sum up to kDeepLinInputs inputs into up to
// kDeepLinOutputs outputs, a summed tensor up to kDeepDotPairs pairs.  The slice's weights and constants pass by value.
constexpr unsigned kDeepPolyLimbs = 8, kDeepLinInputs = 8, kDeepLinOutputs = 4, kDeepDotPairs = 16;

// the scalars of one scalar-sum launch: w[l][o][r] of slice limb l, launch output o and launch input r; k[l][o]
struct DeepLinWords {
    unsigned long long w[kDeepPolyLimbs][kDeepLinOutputs][kDeepLinInputs];
    unsigned long long k[kDeepPolyLimbs][kDeepLinOutputs];
};
// the weights of one summed-tensor launch: w[l][r] of slice limb l and launch pair r
struct DeepDotWords {
    unsigned long long w[kDeepPolyLimbs][kDeepDotPairs];
};

namespace host {

// launches of a scalar sum: ceil(limbs / 8) ceil(outputs / 4) ceil(count / 8)
inline u64 deep_lincomb_launches(unsigned limbs, unsigned outputs, unsigned count) {
    return (u64)((limbs + kDeepPolyLimbs - 1) / kDeepPolyLimbs) * ((outputs + kDeepLinOutputs - 1) / kDeepLinOutputs) * ((count + kDeepLinInputs - 1) / kDeepLinInputs);
}
// launches of the summed tensor of one chunk of a dot: ceil(limbs / 8) ceil(count / 16)
inline u64 deep_tensorsum_launches(unsigned limbs, unsigned count) {
    return (u64)((limbs + kDeepPolyLimbs - 1) / kDeepPolyLimbs) * ((count + kDeepDotPairs - 1) / kDeepDotPairs);
}

// The launches of a scalar sum in the order they are issued: f(o0, no, i0, nl, r0, nr) covers outputs [o0, o0 + no), limbs
// [i0, i0 + nl) and inputs [r0, r0 + nr); the groups of inputs of one (outputs, limbs) block follow each other, so every one
// after the first (r0 > 0) carries the words the former left.  Stops at and returns the first non-zero result.
template <class F>
inline int deep_lincomb_each(unsigned limbs, unsigned outputs, unsigned count, F f) {
    for (unsigned o0 = 0; o0 < outputs; o0 += kDeepLinOutputs)
        for (unsigned i0 = 0; i0 < limbs; i0 += kDeepPolyLimbs)
            for (unsigned r0 = 0; r0 < count; r0 += kDeepLinInputs) {
                const unsigned no = outputs - o0 < kDeepLinOutputs ? outputs - o0 : kDeepLinOutputs, nl = limbs - i0 < kDeepPolyLimbs ? limbs - i0 : kDeepPolyLimbs,
                               nr = count - r0 < kDeepLinInputs ? count - r0 : kDeepLinInputs;
                if (const int rc = f(o0, no, i0, nl, r0, nr)) return rc;
            }
    return 0;
}
// The same for the summed tensor: f(i0, nl, p0, np), pairs [p0, p0 + np); p0 > 0 carries.
template <class F>
inline int deep_tensorsum_each(unsigned limbs, unsigned count, F f) {
    for (unsigned i0 = 0; i0 < limbs; i0 += kDeepPolyLimbs)
        for (unsigned p0 = 0; p0 < count; p0 += kDeepDotPairs) {
            const unsigned nl = limbs - i0 < kDeepPolyLimbs ? limbs - i0 : kDeepPolyLimbs, np = count - p0 < kDeepDotPairs ? count - p0 : kDeepDotPairs;
            if (const int rc = f(i0, nl, p0, np)) return rc;
        }
    return 0;
}

// the scalars of that launch from the call's arrays: w [outputs][count][limbs], k [outputs][limbs] or NULL (zeros).  What the
// launch does not cover stays zero.
inline void deep_lincomb_words(const u64 *w, const u64 *k, unsigned limbs, unsigned count, unsigned o0, unsigned no, unsigned i0, unsigned nl, unsigned r0, unsigned nr,
                               DeepLinWords *out) {
    *out = DeepLinWords{};
    for (unsigned l = 0; l < nl; l++)
        for (unsigned o = 0; o < no; o++) {
            for (unsigned r = 0; r < nr; r++) out->w[l][o][r] = w[((u64)(o0 + o) * count + r0 + r) * limbs + i0 + l];
            out->k[l][o] = k ? k[(u64)(o0 + o) * limbs + i0 + l] : 0;
        }
}
// w [count][limbs] or NULL (ones)
inline void deep_tensorsum_words(const u64 *w, unsigned limbs, unsigned i0, unsigned nl, unsigned p0, unsigned np, DeepDotWords *out) {
    *out = DeepDotWords{};
    for (unsigned l = 0; l < nl; l++)
        for (unsigned r = 0; r < np; r++) out->w[l][r] = w ? w[(u64)(p0 + r) * limbs + i0 + l] : 1;
}

}  // namespace host
}  // namespace fhe
