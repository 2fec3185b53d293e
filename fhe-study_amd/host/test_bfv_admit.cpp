// test_bfv_admit.cpp — the admission of the BFV products on the chain (csrc/rns_tables.hpp: bfv_admits, big_mul128; DESIGN.md
// §34), without the library or a GPU.  B > t n Q W + 1 holds exactly for W <= floor((B - 2) / (t n Q)); that boundary is computed
// here by successive divisions of B - 2 (floor(floor(x / a) / b) = floor(x / (a b))), which shares nothing with the products
// bfv_admits compares, and the two are held against each other at W = 1, the boundary, the boundary + 1 and 64 (2^61 - 1), the
// largest W the entry point can be asked for.  Also the program the sanitizers run on this arithmetic (`make san_admit`).
#include <cstdio>
#include <cstdlib>

#include "../csrc/rns_tables.hpp"

using fhe::host::Big;
using fhe::host::u128;
using fhe::host::u64;

static int failures = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            failures++;                                              \
        }                                                            \
    } while (0)

static u64 rng_state = 0x9E3779B97F4A7C15ull;
static u64 rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static Big big_of(u128 x) {
    Big b;
    b.w = {(u64)x, (u64)(x >> 64)};
    b.trim();
    return b;
}

// x - y for x >= y
static Big big_sub_small(Big x, u64 y) {
    for (size_t i = 0; y && i < x.w.size(); i++) {
        const u64 before = x.w[i];
        x.w[i] = before - y;
        y = before < y ? 1 : 0;
    }
    x.trim();
    return x;
}

// floor((B - 2) / (t n Q)), by one division per factor
static Big boundary(const u64 *aux, unsigned na, const u64 *mods, unsigned nq, u64 t, u64 n) {
    Big x = big_sub_small(fhe::host::big_product(aux, na), 2);
    x.divmod(t);
    x.divmod(n);
    for (unsigned i = 0; i < nq; i++) x.divmod(mods[i]);
    return x;
}

static const u128 kLargestW = (u128)64 * ((1ull << 61) - 1);

static void test_mul128() {
    for (int it = 0; it < 2000; it++) {
        Big a = big_of(((u128)rnd() << 64 | rnd()) >> (rnd() % 120));
        a.mul(rnd() >> (rnd() % 64));                                // up to three words, zero included
        const u128 x = ((u128)rnd() << 64 | rnd()) >> (rnd() % 128);
        const Big p = fhe::host::big_mul128(a, x);
        CHECK(p.w.empty() || p.w.back() != 0);
        for (int j = 0; j < 4; j++) {
            const u64 m = (rnd() >> (rnd() % 60)) | 1;
            CHECK(p.mod(m) == fhe::host::mulmod(a.mod(m), (u64)(x % m), m));
        }
        CHECK(p.w.empty() == (a.w.empty() || x == 0));
    }
    CHECK(fhe::host::big_mul128(big_of(~(u128)0), ~(u128)0).w.size() == 4);   // (2^128 - 1)^2: every carry taken
}

struct Base {
    unsigned nq;
    u64 mods[4], aux[5];
    u64 t, n;
};

static void check_base(const Base &b, int line) {
    const Big wb = boundary(b.aux, b.nq + 1, b.mods, b.nq, b.t, b.n);
    auto admits = [&](u128 W) { return fhe::host::bfv_admits(b.aux, b.nq + 1, b.mods, b.nq, b.t, b.n, W); };
    auto within = [&](u128 W) { return big_of(W).cmp(wb) <= 0; };
    const u128 cases[] = {1, 2, 63, 64, kLargestW - 1, kLargestW};
    for (u128 W : cases)
        if (admits(W) != within(W)) {
            printf("FAILED line %d: W = %llu * 2^64 + %llu\n", line, (unsigned long long)(W >> 64), (unsigned long long)W);
            failures++;
        }
    if (wb.w.size() <= 2 && !wb.w.empty()) {                         // the boundary itself fits 128 bits: one either side of it
        const u128 w = (u128)wb.w[0] | (wb.w.size() > 1 ? (u128)wb.w[1] << 64 : 0);
        CHECK(admits(w));
        if (w != ~(u128)0) CHECK(!admits(w + 1));
    }
    if (wb.w.empty()) CHECK(!admits(1));
}

int main() {
    test_mul128();
    // primes 1 modulo 128 just below 2^40 and 2^41 (what tests/_bfv_rns_numpy.chain(64, 2, bq=40, bb=41) gives is of this size);
    // the arithmetic does not need primes, only the sizes
    Base edge{2, {(1ull << 40) - 87, (1ull << 40) - 167}, {(1ull << 41) - 21, (1ull << 41) - 31, (1ull << 41) - 49}, 0, 64};
    {   // t chosen so that the boundary W is exactly 7: inside [2, 64]
        Big x = boundary(edge.aux, 3, edge.mods, 2, 1, edge.n);      // floor((B - 2) / (n Q))
        x.divmod(7);
        CHECK(x.w.size() == 1);
        edge.t = x.w[0];
        const Big wb = boundary(edge.aux, 3, edge.mods, 2, edge.t, edge.n);
        CHECK(wb.w.size() == 1 && wb.w[0] == 7);
        CHECK(fhe::host::bfv_admits(edge.aux, 3, edge.mods, 2, edge.t, edge.n, 7));
        CHECK(!fhe::host::bfv_admits(edge.aux, 3, edge.mods, 2, edge.t, edge.n, 8));
        check_base(edge, __LINE__);
    }
    // the measured shape's sizes: three 59-bit primes, four 61-bit ones, t = 65537, n = 8192
    check_base(Base{3, {(1ull << 59) - 55, (1ull << 59) - 99, (1ull << 59) - 225}, {(1ull << 61) - 1, (1ull << 61) - 31, (1ull << 61) - 85, (1ull << 61) - 259}, 65537, 8192},
               __LINE__);
    // a base that does not admit a single product: the boundary is 0
    check_base(Base{1, {(1ull << 59) - 55}, {(1ull << 30) - 35, (1ull << 30) - 41}, 65537, 64}, __LINE__);
    // a base far past the largest W: 64 (2^61 - 1) is admitted
    {
        const Base wide{1, {(1ull << 20) - 3}, {(1ull << 61) - 1, (1ull << 61) - 31}, 2, 2};
        CHECK(fhe::host::bfv_admits(wide.aux, 2, wide.mods, 1, wide.t, wide.n, kLargestW));
        check_base(wide, __LINE__);
    }
    // the boundary between 2^64 and 64 (2^61 - 1): a weight sum that needs the high word
    check_base(Base{1, {(1ull << 20) - 3}, {(1ull << 61) - 1, (1ull << 27) - 39}, 2, 2}, __LINE__);
    // four limbs, random odd sizes
    for (int it = 0; it < 200; it++) {
        Base b{};
        b.nq = 1 + (unsigned)(rnd() % 4);
        for (unsigned i = 0; i < b.nq; i++) b.mods[i] = (rnd() >> (2 + rnd() % 40)) | 3;
        for (unsigned i = 0; i <= b.nq; i++) b.aux[i] = (rnd() >> (2 + rnd() % 30)) | 3;
        b.t = 2 + (rnd() >> (4 + rnd() % 58));
        b.n = 2ull << (rnd() % 19);
        check_base(b, __LINE__);
    }
    if (failures) {
        printf("%d FAILURES\n", failures);
        return 1;
    }
    printf("all bfv admission tests passed\n");
    return 0;
}
