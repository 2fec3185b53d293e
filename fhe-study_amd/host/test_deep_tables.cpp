// test_deep_tables.cpp — the host side of the grouped-digit key switch (csrc/rns_tables.hpp: deep_groups, deep_admits,
// deep_ext_tables), without the library or a GPU.  The admission is held against a comparison by successive
// divisions, which shares nothing with the products deep_admits compares; the tables against their definitions, and the
// kernel's route (Garner's digits, the centring compare, one 128-bit sum per target) against the CRT definition on multiword
// integers, at the edges 0, 1, floor(M / 2), floor(M / 2) + 1, M - 1 and at random; on the bases of §38's sweep (every prime just
// below 2^62; 30-bit beside 37, 61 and 62-bit primes in both orders) the source tables against their definitions, the device's word
// formulas against the digits, and the compare decided at every digit position.  Also the program the sanitizers run on this
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

// ---- the bases of the sweep ----------------------------------------------------------------------------------------
// the device's word arithmetic (csrc/rns_ext_device.hpp), restated with 128-bit products
static u64 hi64(u64 a, u64 b) { return (u64)(((u128)a * b) >> 64); }
static u64 csub(u64 x, u64 q) { return x >= q ? x - q : x; }
static u64 dev_mul(u64 x, u64 w, u64 wp, u64 q) { return csub(x * w - hi64(x, wp) * q, q); }
static u64 dev_red(u64 x, u64 q, u64 onep) { return csub(x - hi64(x, onep) * q, q); }

// the source tables against their definitions, and Garner's digits by the device's formulas (ext_red of an earlier digit modulo a
// later source, ext_mul by the Shoup pair) against the digits the integer was made from
static void check_sources(const std::vector<u64> &src, const std::vector<u64> &dst, const u64 *digits_of_x) {
    const unsigned s = (unsigned)src.size(), t = (unsigned)dst.size();
    fhe::DeepSrc e;
    std::vector<fhe::DeepTarget> tab(t);
    std::vector<u64> off(t, 0);
    CHECK(fhe::host::deep_ext_tables(src.data(), s, dst.data(), off.data(), t, &e, tab.data()));
    Big half = fhe::host::big_product(src.data(), s);
    half.divmod(2);
    CHECK(from_digits(src.data(), s, e.half).cmp(half) == 0);
    for (unsigned i = 0; i < s; i++) {
        CHECK(e.mq[i] == src[i] && e.monep[i] == (u64)((((u128)1) << 64) / src[i]) && e.half[i] < src[i]);
        for (unsigned j = 0; j < i; j++) {
            CHECK(e.inv[j][i] < src[i] && (u64)((u128)e.inv[j][i] * (src[j] % src[i]) % src[i]) == 1);
            CHECK(e.invp[j][i] == (u64)((((u128)e.inv[j][i]) << 64) / src[i]));
        }
    }
    for (unsigned k = 0; k < t; k++) CHECK(tab[k].r64p == (u64)((((u128)tab[k].r64) << 64) / dst[k]));
    const Big X = from_digits(src.data(), s, digits_of_x);
    u64 a[8];
    for (unsigned i = 0; i < s; i++) {
        const u64 q = src[i];
        u64 v = X.mod(q);
        for (unsigned j = 0; j < i; j++) v = dev_mul(v + q - dev_red(a[j], q, e.monep[i]), e.inv[j][i], e.invp[j][i], q);
        a[i] = v;
        CHECK(a[i] == digits_of_x[i]);
    }
    // one target's sum by the device's reduction: the low word by ext_red, the high word times 2^64 mod p by ext_mul
    for (unsigned k = 0; k < t; k++) {
        const fhe::DeepTarget &d = tab[k];
        u128 acc = 0;
        for (unsigned j = 0; j < s; j++) acc += (u128)a[j] * d.W[j];
        const u64 v = csub(dev_red((u64)acc, d.q, d.onep) + dev_mul((u64)(acc >> 64), d.r64, d.r64p, d.q), d.q);
        CHECK(v == X.mod(d.q));
    }
}

// for every digit position i: the digits of floor(M / 2) above i, one more or one less at i, and below i those of floor(M / 2), all
// zero, or all m_j - 1: the compare is decided at every depth, with the low digits pointing the other way
static void check_depths(const std::vector<u64> &src, const std::vector<u64> &dst) {
    const unsigned s = (unsigned)src.size();
    fhe::DeepSrc e;
    std::vector<fhe::DeepTarget> tab(dst.size());
    std::vector<u64> off(dst.size(), 0);
    CHECK(fhe::host::deep_ext_tables(src.data(), s, dst.data(), off.data(), (unsigned)dst.size(), &e, tab.data()));
    u64 top[8];
    for (unsigned i = 0; i < s; i++) top[i] = src[i] - 1;
    check_sources(src, dst, top);
    check_sources(src, dst, e.half);
    for (unsigned i = 0; i < s; i++)
        for (int step = -1; step <= 1; step += 2) {
            if ((step < 0 && e.half[i] == 0) || (step > 0 && e.half[i] + 1 >= src[i])) continue;
            for (int low = 0; low < 3; low++) {
                u64 a[8];
                for (unsigned j = 0; j < s; j++) a[j] = j > i ? e.half[j] : j == i ? e.half[i] + (u64)step : low == 0 ? e.half[j] : low == 1 ? 0 : src[j] - 1;
                check_word(src, dst, a);
                check_sources(src, dst, a);
            }
        }
}

static void test_sweep_bases() {
    for (u64 step : {16ull, 128ull}) {                               // the primes of n = 8 and n = 64
        // A1: every prime just below 2^62; the first alpha are the special primes, the next L the chain
        const unsigned shapes[4][3] = {{32, 1, 32}, {17, 8, 17}, {9, 3, 7}, {5, 2, 4}};
        for (const auto &sh : shapes) {
            const unsigned L = sh[0], alpha = sh[1], l = sh[2];
            const std::vector<u64> ps = primes_below(62, step, alpha + L);
            const u64 *sp = ps.data(), *q = ps.data() + alpha;
            CHECK(fhe::host::deep_admits(q, L, sp, alpha) && fhe::host::deep_admits(q, l, sp, alpha));
            for (unsigned j0 = 0; j0 < l; j0 += alpha) {
                const unsigned s = l - j0 < alpha ? l - j0 : alpha;
                std::vector<u64> src(q + j0, q + j0 + s), dst(sp, sp + alpha);
                for (unsigned i = 0; i < l && dst.size() < 12; i++)
                    if (i < j0 || i >= j0 + s) dst.push_back(q[i]);
                check_depths(src, dst);
            }
            check_depths(std::vector<u64>(sp, sp + alpha), std::vector<u64>(q, q + (l < 8 ? l : 8)));   // the modulus-down
        }
        // A3: a 30-bit prime beside 37, 61 and 62-bit ones, small before large and large before small
        const std::vector<u64> p30 = primes_below(30, step, 4), p37 = primes_below(37, step, 4), p61 = primes_below(61, step, 4), p62 = primes_below(62, step, 12);
        for (unsigned alpha : {2u, 4u, 8u})
            for (int down = 0; down < 2; down++) {
                std::vector<u64> grp;
                for (unsigned i = 0; i < alpha; i++) grp.push_back(i % 4 == 0 ? p30[i / 4] : i % 4 == 1 ? p62[8 + i / 4] : i % 4 == 2 ? p37[i / 4] : p61[i / 4]);
                if (down) grp = std::vector<u64>(grp.rbegin(), grp.rend());
                std::vector<u64> dst(p62.begin(), p62.begin() + alpha);
                dst.push_back(p30[2]);
                dst.push_back(p37[2]);
                dst.push_back(p61[2]);
                CHECK(fhe::host::deep_admits(grp.data(), alpha, p62.data(), alpha));
                check_depths(grp, dst);
                if (alpha == 2) {                                    // the other neighbours of the 30-bit prime at alpha = 2
                    check_depths(down ? std::vector<u64>{p61[0], p30[1]} : std::vector<u64>{p30[1], p61[0]}, dst);
                    check_depths(down ? std::vector<u64>{p37[0], p30[3]} : std::vector<u64>{p30[3], p37[0]}, dst);
                }
            }
    }
}

int main() {
    test_groups();
    test_admission();
    test_extension();
    test_sweep_bases();
    if (failures) {
        printf("%d FAILURES\n", failures);
        return 1;
    }
    printf("all deep table tests passed\n");
    return 0;
}
