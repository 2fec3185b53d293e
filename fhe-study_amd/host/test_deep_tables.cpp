// test_deep_tables.cpp — the host side of the grouped-digit key switch (csrc/rns_tables.hpp: deep_groups, deep_admits,
// deep_ext_tables), without the library or a GPU.  The admission is held against a comparison by successive
// divisions, which shares nothing with the products deep_admits compares; the tables against their definitions, and the
// kernel's route (Garner's digits, the centring compare, one 128-bit sum per target) against the CRT definition on multiword
// integers, at the edges 0, 1, floor(M / 2), floor(M / 2) + 1, M - 1 and at random.  Also the program the sanitizers run on this
// arithmetic (`make san_deep`).
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

static bool is_prime(u64 x) {
    if (x < 2) return false;
    for (u64 p : {2ull, 3ull, 5ull, 7ull, 11ull, 13ull, 17ull, 19ull, 23ull, 29ull, 31ull, 37ull})
        if (x % p == 0) return x == p;
    u64 d = x - 1;
    unsigned r = 0;
    while ((d & 1) == 0) d >>= 1, r++;
    for (u64 a : {2ull, 3ull, 5ull, 7ull, 11ull, 13ull, 17ull, 19ull, 23ull, 29ull, 31ull, 37ull}) {
        u64 y = fhe::host::exp_mod(x, a, d);
        if (y == 1 || y == x - 1) continue;
        bool comp = true;
        for (unsigned i = 1; i < r && comp; i++) {
            y = fhe::host::mulmod(y, y, x);
            if (y == x - 1) comp = false;
        }
        if (comp) return false;
    }
    return true;
}

// the first `count` primes 1 modulo `step` below 2^bits, downward
static std::vector<u64> primes_below(unsigned bits, u64 step, unsigned count) {
    std::vector<u64> out;
    for (u64 c = (1ull << bits) + 1 - step; out.size() < count; c -= step)
        if (is_prime(c)) out.push_back(c);
    return out;
}

// P >= Q exactly when floor(P / Q) >= 1: divide P by every factor of Q in turn (floor(floor(x / a) / b) = floor(x / (a b)))
static bool ge_by_division(const u64 *p, unsigned np, const u64 *q, unsigned nq) {
    Big x = fhe::host::big_product(p, np);
    for (unsigned i = 0; i < nq; i++) x.divmod(q[i]);
    return !x.w.empty();
}

static void test_groups() {
    CHECK(fhe::host::deep_groups(1, 1) == 1 && fhe::host::deep_groups(32, 1) == 32 && fhe::host::deep_groups(32, 8) == 4);
    CHECK(fhe::host::deep_groups(5, 2) == 3 && fhe::host::deep_groups(17, 8) == 3 && fhe::host::deep_groups(3, 8) == 1 && fhe::host::deep_groups(9, 3) == 3);
}

static void test_admission() {
    const std::vector<u64> q40 = primes_below(40, 128, 12), q41 = primes_below(41, 128, 4), q39 = primes_below(39, 128, 4);
    // every group's product below P: three 41-bit special primes over groups of three 40-bit primes
    CHECK(fhe::host::deep_admits(q40.data(), 12, q41.data(), 3));
    CHECK(fhe::host::deep_admits(q40.data(), 11, q41.data(), 3));                       // a partial last group
    CHECK(fhe::host::deep_admits(q40.data(), 2, q41.data(), 3));                        // alpha > L
    CHECK(!fhe::host::deep_admits(q40.data(), 12, q39.data(), 3));                      // P below the groups
    CHECK(!fhe::host::deep_admits(q40.data(), 3, q39.data(), 0) && !fhe::host::deep_admits(q40.data(), 3, q39.data(), 9));
    // one either side of P = Q_j: the same primes on both sides are equal (admitted); the group's smallest prime replaced by the
    // next larger one passes P by the least amount these primes allow (refused), by the next smaller one stays below (admitted)
    {
        const u64 p[3] = {q40[1], q40[2], q40[3]};
        const u64 eq[3] = {q40[3], q40[1], q40[2]}, above[3] = {q40[0], q40[1], q40[2]}, below[3] = {q40[4], q40[1], q40[2]};
        CHECK(fhe::host::deep_admits(eq, 3, p, 3));
        CHECK(!fhe::host::deep_admits(above, 3, p, 3));
        CHECK(fhe::host::deep_admits(below, 3, p, 3));
        // only the LAST group misses
        const u64 chain[6] = {q40[4], q40[1], q40[2], q41[0], q40[5], q40[6]};
        CHECK(fhe::host::deep_admits(chain, 3, p, 3) && !fhe::host::deep_admits(chain, 6, p, 3));
    }
    // alpha = 1 is "P >= max q_i"
    for (int it = 0; it < 200; it++) {
        u64 q[8], P = (rnd() >> (2 + rnd() % 40)) | 3, mx = 0;
        const unsigned L = 1 + (unsigned)(rnd() % 8);
        for (unsigned i = 0; i < L; i++) q[i] = (rnd() >> (2 + rnd() % 40)) | 3, mx = q[i] > mx ? q[i] : mx;
        CHECK(fhe::host::deep_admits(q, L, &P, 1) == (P >= mx));
    }
    // random sizes against the division
    for (int it = 0; it < 2000; it++) {
        u64 q[32], p[8];
        const unsigned L = 1 + (unsigned)(rnd() % 32), alpha = 1 + (unsigned)(rnd() % 8);
        for (unsigned i = 0; i < L; i++) q[i] = (rnd() >> (2 + rnd() % 8)) | 3;
        for (unsigned i = 0; i < alpha; i++) p[i] = (rnd() >> (2 + rnd() % 8)) | 3;
        bool want = true;
        for (unsigned j = 0; j < L; j += alpha) want = want && ge_by_division(p, alpha, q + j, L - j < alpha ? L - j : alpha);
        CHECK(fhe::host::deep_admits(q, L, p, alpha) == want);
    }
}

// the integer with the given mixed-radix digits
static Big from_digits(const u64 *src, unsigned s, const u64 *a) {
    Big x;
    for (unsigned i = s; i-- > 0;) {
        x.mul(src[i]);
        x.add(a[i]);
    }
    return x;
}

// the kernel's route on the host for one word, and the definition beside it
static void check_word(const std::vector<u64> &src, const std::vector<u64> &dst, const u64 *digits_of_x) {
    const unsigned s = (unsigned)src.size(), t = (unsigned)dst.size();
    fhe::DeepSrc e;
    std::vector<fhe::DeepTarget> tab(t);
    std::vector<u64> off(t);
    for (unsigned k = 0; k < t; k++) off[k] = 3 * k + 1;
    CHECK(fhe::host::deep_ext_tables(src.data(), s, dst.data(), off.data(), t, &e, tab.data()));
    const Big X = from_digits(src.data(), s, digits_of_x);
    u64 x[8], a[8];
    for (unsigned i = 0; i < s; i++) x[i] = X.mod(src[i]);
    for (unsigned i = 0; i < s; i++) {                               // Garner, as ext_digits
        u64 v = x[i];
        const u64 q = src[i];
        for (unsigned j = 0; j < i; j++) v = fhe::host::mulmod((v + q - a[j] % q) % q, e.inv[j][i], q);
        a[i] = v;
        CHECK(a[i] == digits_of_x[i]);
    }
    bool gt = false, eq = true;
    for (unsigned i = s; i-- > 0;)
        if (eq && a[i] != e.half[i]) gt = a[i] > e.half[i], eq = false;
    // the definition: X > floor(M / 2)
    Big half = fhe::host::big_product(src.data(), s);
    half.divmod(2);
    CHECK(gt == (X.cmp(half) > 0));
    const Big M = fhe::host::big_product(src.data(), s);
    for (unsigned k = 0; k < t; k++) {
        const fhe::DeepTarget &d = tab[k];
        const u64 p = dst[k];
        CHECK(d.q == p && d.off == off[k] && d.pM == M.mod(p) && d.onep == (u64)((((u128)1) << 64) / p) && d.r64 == (u64)((((u128)1) << 64) % p));
        u128 acc = 0;
        for (unsigned j = 0; j < s; j++) {
            CHECK(d.W[j] == fhe::host::big_product(src.data(), j).mod(p));
            acc += (u128)a[j] * d.W[j];                              // at most eight terms below 2^124
        }
        u64 v = (u64)(acc % p);
        if (gt) v = (v + p - d.pM) % p;
        const u64 want = gt ? (X.mod(p) + p - M.mod(p)) % p : X.mod(p);   // X - M modulo p for a centred X above half
        CHECK(v == want);
    }
}

static void test_extension() {
    const std::vector<u64> small = primes_below(30, 128, 4), big = primes_below(62, 128, 4), mid = primes_below(40, 128, 8);
    std::vector<u64> targets = primes_below(55, 128, 5);
    targets.push_back(small[3]);
    targets.push_back(big[3]);
    for (unsigned s = 1; s <= 8; s++) {
        std::vector<u64> src;
        for (unsigned i = 0; i < s; i++) src.push_back(i % 3 == 0 ? big[i / 3] : i % 3 == 1 ? small[i / 3] : mid[i]);   // 30-bit beside 2^62
        fhe::DeepSrc e;
        std::vector<fhe::DeepTarget> tab(targets.size());
        std::vector<u64> off(targets.size(), 0);
        CHECK(fhe::host::deep_ext_tables(src.data(), s, targets.data(), off.data(), (unsigned)targets.size(), &e, tab.data()));
        CHECK(e.s == s);
        u64 zero[8] = {0}, one[8] = {1}, top[8], halfp[8];
        for (unsigned i = 0; i < s; i++) top[i] = src[i] - 1, halfp[i] = e.half[i];
        check_word(src, targets, zero);
        check_word(src, targets, one);
        check_word(src, targets, e.half);                            // floor(M / 2): not above
        for (unsigned i = 0; i < s; i++) {                           // floor(M / 2) + 1: add with carry through the radices
            if (++halfp[i] < src[i]) break;
            halfp[i] = 0;
        }
        check_word(src, targets, halfp);
        check_word(src, targets, top);                               // M - 1
        for (int it = 0; it < 200; it++) {
            u64 a[8];
            for (unsigned i = 0; i < s; i++) a[i] = rnd() % src[i];
            check_word(src, targets, a);
        }
    }
    // refused: nine sources, a repeated source, an even target, a target of 2^62 or more
    fhe::DeepSrc e;
    fhe::DeepTarget tab[2];
    const u64 off[2] = {0, 1}, rep[2] = {mid[0], mid[0]}, even[1] = {1ull << 40}, wide[1] = {(1ull << 62) + 1};
    std::vector<u64> nine = primes_below(40, 128, 9);
    CHECK(!fhe::host::deep_ext_tables(nine.data(), 9, mid.data(), off, 1, &e, tab));
    CHECK(!fhe::host::deep_ext_tables(rep, 2, mid.data() + 1, off, 1, &e, tab));
    CHECK(!fhe::host::deep_ext_tables(mid.data(), 2, even, off, 1, &e, tab));
    CHECK(!fhe::host::deep_ext_tables(mid.data(), 2, wide, off, 1, &e, tab));
    CHECK(fhe::host::deep_ext_tables(mid.data(), 2, mid.data() + 2, off, 0, &e, tab));   // no target: a group that is the whole chain
}

int main() {
    test_groups();
    test_admission();
    test_extension();
    if (failures) {
        printf("%d FAILURES\n", failures);
        return 1;
    }
    printf("all deep table tests passed\n");
    return 0;
}
