// test_rns_tables.cpp — csrc/rns_tables.hpp against its definitions, without the library or a GPU: the multi-word integers
// against 128-bit arithmetic, Garner's inverses, the mixed-radix digits of floor(M / 2), the weights and M mod p of every
// target, and the whole route (digits, comparison from the top, weighted sum) against x mod p for integers that fit 128 bits.
// Also the program the sanitizers run on these builders (`make san`, or alone `make san_tables`).
#include <cstdio>
#include <cstdlib>
#include <vector>

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
    for (u64 p : {2ull, 3ull, 5ull, 7ull, 11ull, 13ull, 17ull, 19ull, 23ull, 29ull, 31ull, 37ull}) {
        if (x % p == 0) return x == p;
    }
    u64 d = x - 1;
    int r = 0;
    while ((d & 1) == 0) d >>= 1, r++;
    for (u64 a : {2ull, 3ull, 5ull, 7ull, 11ull, 13ull, 17ull, 19ull, 23ull, 29ull, 31ull, 37ull}) {
        u64 y = fhe::host::exp_mod(x, a, d);
        if (y == 1 || y == x - 1) continue;
        bool comp = true;
        for (int i = 1; i < r && comp; i++) {
            y = fhe::host::mulmod(y, y, x);
            if (y == x - 1) comp = false;
        }
        if (comp) return false;
    }
    return true;
}
static void primes_below(unsigned bits, unsigned count, u64 *out) {
    u64 c = (1ull << bits) - 1;
    for (unsigned k = 0; k < count; c -= 2)
        if (is_prime(c)) out[k++] = c;
}

static Big big_of(u128 x) {
    Big b;
    b.w = {(u64)x, (u64)(x >> 64)};
    b.trim();
    return b;
}

static void test_big() {
    for (int it = 0; it < 2000; it++) {
        const u128 x = ((u128)rnd() << 64 | rnd()) >> (rnd() % 100);
        const u64 m = (rnd() >> (rnd() % 60)) | 1;
        Big b = big_of(x);
        CHECK(b.mod(m) == (u64)(x % m));
        Big q = b;
        CHECK(q.divmod(m) == (u64)(x % m) && q.cmp(big_of(x / m)) == 0);
        const u64 s = rnd() >> 40;
        Big p = big_of(x >> 30);
        p.mul(s);
        CHECK(p.cmp(big_of((x >> 30) * s)) == 0);
        Big a = big_of(x >> 1);
        a.add(m);
        CHECK(a.cmp(big_of((x >> 1) + m)) == 0);
        CHECK(big_of(x).cmp(big_of(x + 1)) == -1 && big_of(x + 1).cmp(big_of(x)) == 1);
    }
    Big carry = big_of(~(u128)0);
    carry.add(1);
    CHECK(carry.w.size() == 3 && carry.w[0] == 0 && carry.w[1] == 0 && carry.w[2] == 1);
    Big zero(0);
    zero.mul(5);
    CHECK(zero.w.empty() && zero.mod(7) == 0 && zero.cmp(Big(0)) == 0);
}

static void test_inverses() {
    u64 inv;
    for (int it = 0; it < 2000; it++) {
        const u64 m = (rnd() >> (2 + rnd() % 50)) | 3, x = rnd();
        if (fhe::host::inv_mod_any(x, m, &inv)) CHECK(inv < m && fhe::host::mulmod(inv, x % m, m) == 1 % m);
    }
    CHECK(!fhe::host::inv_mod_any(15, 21, &inv) && !fhe::host::inv_mod_any(0, 7, &inv));
    CHECK(fhe::host::inv_mod_any(1, 3, &inv) && inv == 1);
}

// the tables of any shape against their definitions
template <unsigned S, unsigned T>
static void check_tables(const u64 *src, unsigned s, const u64 *dst, unsigned t) {
    fhe::ExtArgs<S, T> e;
    CHECK((fhe::host::ext_tables<S, T>(src, s, dst, t, &e)));
    CHECK(e.s == s && e.t == t);
    const Big M = fhe::host::big_product(src, s);
    Big half = M;
    half.divmod(2);
    Big back(0);                                                     // the digits of floor(M / 2), recombined from the top
    for (unsigned i = s; i-- > 0;) {
        CHECK(e.half[i] < src[i]);
        back.mul(src[i]);
        back.add(e.half[i]);
    }
    CHECK(back.cmp(half) == 0);
    for (unsigned i = 0; i < s; i++) {
        CHECK(e.mq[i] == src[i] && e.monep[i] == (u64)((((u128)1) << 64) / src[i]));
        for (unsigned j = 0; j < i; j++) {
            CHECK(fhe::host::mulmod(e.inv[j][i], src[j] % src[i], src[i]) == 1);
            CHECK(e.invp[j][i] == (u64)(((u128)e.inv[j][i] << 64) / src[i]));
        }
    }
    for (unsigned k = 0; k < t; k++) {
        const u64 p = dst[k];
        CHECK(e.pq[k] == p && e.pM[k] == M.mod(p) && e.pr64[k] == (u64)((((u128)1) << 64) % p));
        CHECK(e.ponep[k] == (u64)((((u128)1) << 64) / p) && e.pr64p[k] == (u64)(((u128)e.pr64[k] << 64) / p));
        for (unsigned j = 0; j < s; j++) CHECK(e.W[j][k] == fhe::host::big_product(src, j).mod(p));
    }
}

// the kernel's route in host arithmetic on the tables -> x (less M where centred and above half) modulo target k
template <unsigned S, unsigned T>
static u64 route(const fhe::ExtArgs<S, T> &e, const u64 *res, bool centred, unsigned k) {
    u64 a[S];
    for (unsigned i = 0; i < e.s; i++) {
        u64 v = res[i];
        const u64 q = e.mq[i];
        for (unsigned j = 0; j < i; j++) v = fhe::host::mulmod((v + q - a[j] % q) % q, e.inv[j][i], q);
        a[i] = v;
    }
    bool gt = false;
    for (unsigned i = e.s; i-- > 0;)
        if (a[i] != e.half[i]) {
            gt = a[i] > e.half[i];
            break;
        }
    const u64 p = e.pq[k];
    u64 v = 0;
    for (unsigned j = 0; j < e.s; j++) v = (u64)(((u128)v + (u128)fhe::host::mulmod(a[j] % p, e.W[j][k], p)) % p);
    if (centred && gt) v = (v + p - e.pM[k]) % p;
    return v;
}

static void test_route() {
    u64 p61[4], p40[3], p20[6];
    primes_below(61, 4, p61);
    primes_below(40, 3, p40);
    primes_below(20, 6, p20);
    struct Case { const u64 *src; unsigned s; const u64 *dst; unsigned t; };
    const Case cases[] = {{p61, 2, p61 + 2, 2}, {p40, 3, p61, 4}, {p20, 6, p40, 3}, {p61, 1, p20, 6}};
    for (const Case &c : cases) {
        fhe::ExtArgs<9, 9> e;
        CHECK((fhe::host::ext_tables<9, 9>(c.src, c.s, c.dst, c.t, &e)));
        u128 M = 1;
        for (unsigned i = 0; i < c.s; i++) M *= c.src[i];
        for (int it = 0; it < 3000; it++) {
            const u128 edge[] = {0, 1, M - 1, M / 2, M / 2 + 1, M / 2 - 1};
            const u128 x = it < 6 ? edge[it] : (((u128)rnd() << 64) | rnd()) % M;
            u64 res[9];
            for (unsigned i = 0; i < c.s; i++) res[i] = (u64)(x % c.src[i]);
            for (unsigned k = 0; k < c.t; k++) {
                const u64 p = c.dst[k];
                CHECK(route(e, res, false, k) == (u64)(x % p));
                const u64 want = x > M / 2 ? (u64)((p - (u64)((M - x) % p)) % p) : (u64)(x % p);
                CHECK(route(e, res, true, k) == want);
            }
        }
    }
}

static void test_shapes_and_rejections() {
    u64 big[18], small[9];
    primes_below(62, 18, big);                                       // below 2^62
    primes_below(37, 9, small);
    check_tables<9, 9>(big, 9, big + 9, 9);
    check_tables<9, 9>(small, 9, big, 9);
    check_tables<9, 9>(big, 1, big + 1, 2);
    check_tables<4, 5>(big, 4, big + 4, 5);
    check_tables<5, 4>(big + 4, 5, big, 4);
    check_tables<4, 1>(big, 3, small, 1);
    fhe::ExtArgs<9, 9> e;
    u64 bad[3] = {big[0], big[0], big[1]};
    CHECK(!(fhe::host::ext_tables<9, 9>(bad, 3, small, 2, &e)));    // repeated
    bad[1] = big[1] + 1;
    CHECK(!(fhe::host::ext_tables<9, 9>(bad, 3, small, 2, &e)));    // even
    bad[1] = (1ull << 62) + 1;
    CHECK(!(fhe::host::ext_tables<9, 9>(bad, 3, small, 2, &e)));    // 2^62 and above
    bad[0] = 15, bad[1] = 21;
    CHECK(!(fhe::host::ext_tables<9, 9>(bad, 3, small, 2, &e)));    // not coprime
    CHECK(!(fhe::host::ext_tables<9, 9>(big, 0, small, 2, &e)) && !(fhe::host::ext_tables<9, 9>(big, 10, small, 2, &e)));
    CHECK(!(fhe::host::ext_tables<9, 9>(big, 2, small, 0, &e)) && !(fhe::host::ext_tables<9, 9>(small, 2, big, 10, &e)));
    u64 even_dst[2] = {small[0], 4};
    CHECK(!(fhe::host::ext_tables<9, 9>(big, 2, even_dst, 2, &e)));
    fhe::ExtArgs<4, 5> narrow;
    CHECK(!(fhe::host::ext_tables<4, 5>(big, 5, small, 2, &narrow)));   // more sources than the shape holds
}

// sources and targets of mixed size in one base: 3, 5 and 7 beside primes of 20, 37 and 62 bits, small before
// large and large before small.  The tables against their definitions at every size; the route against 128-bit arithmetic where
// M fits, on the integers that differ from floor(M / 2) in one mixed-radix digit, with the digits below it all zero and all
// m_j - 1, so that digit 0 alone points the wrong way.
static void test_mixed_sizes() {
    u64 p20[4], p37[4], p62[4];
    primes_below(20, 4, p20);
    primes_below(37, 4, p37);
    primes_below(62, 4, p62);
    const u64 up9[9] = {3, 5, 7, p20[0], p20[1], p37[0], p37[1], p62[0], p62[1]};
    const u64 dst9[9] = {3, 5, 11, p20[2], p20[3], p37[2], p37[3], p62[2], p62[3]};
    u64 down9[9], ddst9[9];
    for (unsigned i = 0; i < 9; i++) down9[i] = up9[8 - i], ddst9[i] = dst9[8 - i];
    check_tables<9, 9>(up9, 9, dst9, 9);
    check_tables<9, 9>(down9, 9, ddst9, 9);
    check_tables<9, 9>(up9, 9, dst9, 1);                             // the one target 3, a source as well
    const u64 up5[5] = {3, 7, p20[0], p37[0], p62[0]}, down5[5] = {p62[0], p37[0], p20[0], 7, 3};
    const u64 up3[3] = {5, p37[0], p62[0]}, down3[3] = {p62[0], p37[0], 5};
    const u64 up2[2] = {7, p62[0]}, down2[2] = {p62[0], 7};
    check_tables<4, 5>(up3, 3, dst9, 5);
    check_tables<5, 4>(down5, 5, ddst9, 4);
    check_tables<4, 1>(down2, 2, dst9, 1);
    struct Case { const u64 *src; unsigned s; };
    const Case cases[] = {{up5, 5}, {down5, 5}, {up3, 3}, {down3, 3}, {up2, 2}, {down2, 2}};   // M < 2^124
    for (const Case &c : cases) {
        for (const u64 *dst : {(const u64 *)dst9, (const u64 *)ddst9}) {
            fhe::ExtArgs<9, 9> e;
            CHECK((fhe::host::ext_tables<9, 9>(c.src, c.s, dst, 9, &e)));
            u128 M = 1, w[9];
            for (unsigned i = 0; i < c.s; i++) w[i] = M, M *= c.src[i];
            std::vector<u128> xs = {0, 1, M - 1, M / 2, M / 2 + 1, M / 2 - 1};
            for (unsigned i = 0; i < c.s; i++) {
                for (int step = -1; step <= 1; step += 2) {
                    if ((step < 0 && e.half[i] == 0) || (step > 0 && e.half[i] + 1 == c.src[i])) continue;
                    for (int low = 0; low < 3; low++) {              // the digits below i: those of floor(M / 2), zero, m_j - 1
                        u128 x = 0;
                        for (unsigned j = 0; j < c.s; j++) {
                            const u64 d = j > i ? e.half[j] : j == i ? e.half[i] + step : low == 0 ? e.half[j] : low == 1 ? 0 : c.src[j] - 1;
                            x += w[j] * d;
                        }
                        xs.push_back(x);
                    }
                }
                xs.push_back(w[i] * (c.src[i] - 1));                 // a single non-zero digit
                xs.push_back(w[i]);
            }
            for (int it = 0; it < 500; it++) xs.push_back((((u128)rnd() << 64) | rnd()) % M);
            for (const u128 x : xs) {
                CHECK(x < M);
                u64 res[9];
                for (unsigned i = 0; i < c.s; i++) res[i] = (u64)(x % c.src[i]);
                for (unsigned k = 0; k < 9; k++) {
                    const u64 p = dst[k];
                    CHECK(route(e, res, false, k) == (u64)(x % p));
                    const u64 want = x > M / 2 ? (u64)((p - (u64)((M - x) % p)) % p) : (u64)(x % p);
                    CHECK(route(e, res, true, k) == want);
                }
            }
        }
    }
}

int main() {
    test_mixed_sizes();
    test_big();
    test_inverses();
    test_shapes_and_rejections();
    test_route();
    if (failures) {
        printf("%d rns table checks FAILED\n", failures);
        return 1;
    }
    printf("all rns table tests passed\n");
    return 0;
}
