// test_host_tables.cpp — csrc/host_tables.hpp against the definitions of what it builds: needs neither the library nor
// a GPU.  Every comparison is exact.  The moduli are one of each table family: 65537 (32-bit words), a 27-bit prime of
// digit32.hpp, 2^61 - 2^21 + 1 (pseudo-Mersenne), the q = 1 (mod 2^32) and the 2^62 <= q < 2^63 primes of
// tests/test_rq_rows_cpu.py (QMG, Q63); n = 8 and 16.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../csrc/host_tables.hpp"

namespace h = fhe::host;
using h::u128;
using h::u64;

struct Tw { u64 w, wp; };
struct Tw32 { uint32_t w, wp; };

static int g_failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (g_failures++ < 20) {                      \
                printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                printf(__VA_ARGS__);                      \
                printf("\n");                             \
            }                                             \
        }                                                 \
    } while (0)

// arithmetic of the checks themselves: nothing from the header
static u64 mm(u64 a, u64 b, u64 q) { return (u64)((u128)a * b % q); }
static u64 addm(u64 a, u64 b, u64 q) { return (u64)(((u128)a + b) % q); }
static u64 negm(u64 a, u64 q) { return (q - a % q) % q; }

// the plan's roots: psi = the first k^((q-1)/2n) of order 2n (ntt.rs:120-129), roots[bitrev(j)] = psi^j
static std::vector<u64> roots_of(u64 q, u64 n, unsigned log_n) {
    u64 psi = 0;
    for (u64 k = 1; k < q && !psi; k++) {
        const u64 w = h::exp_mod(q, k, (q - 1) / (2 * n));
        if (h::exp_mod(q, w, n) != 1) psi = w;
    }
    std::vector<u64> r(n);
    u64 pw = 1;
    for (u64 j = 0; j < n; j++) {
        r[h::bitrev(j, log_n)] = pw;
        pw = mm(pw, psi, q);
    }
    return r;
}

template <class W>
static void check_bit_lut(const std::vector<u64> &r, u64 q, const char *word) {
    const auto lut = h::bit_lut<W>(r.data(), q);
    const u64 r1 = r[1], r2 = r[2], r3 = r[3];
    for (unsigned p = 0; p < 16; p++) {
        const u64 x0 = p & 1, x1 = (p >> 1) & 1, x2 = (p >> 2) & 1, x3 = (p >> 3) & 1;
        const u64 t2 = mm(r2, x1, q), t3 = mm(r3, x1, q), t1 = mm(r1, x2, q), t12 = mm(mm(r1, r2, q), x3, q), t13 = mm(mm(r1, r3, q), x3, q);
        u64 y[4];
        y[0] = addm(addm(x0, t2, q), addm(t1, t12, q), q);                               // x0 + r2 x1 + r1 x2 + r1 r2 x3
        y[1] = addm(addm(x0, negm(t2, q), q), addm(t1, negm(t12, q), q), q);              // x0 - r2 x1 + r1 x2 - r1 r2 x3
        y[2] = addm(addm(x0, t3, q), addm(negm(t1, q), negm(t13, q), q), q);              // x0 + r3 x1 - r1 x2 - r1 r3 x3
        y[3] = addm(addm(x0, negm(t3, q), q), addm(negm(t1, q), t13, q), q);              // x0 - r3 x1 - r1 x2 + r1 r3 x3
        for (int j = 0; j < 4; j++) {
            CHECK((u64)lut[4 * p + j] == y[j], "bit_lut<%s> q=%llu word %u: %llu != %llu", word, q, 4 * p + j, (u64)lut[4 * p + j], y[j]);
            CHECK((u64)lut[64 + 4 * p + j] == mm(r[4 + j], y[j], q), "bit_lut<%s> q=%llu word %u", word, q, 64 + 4 * p + j);
        }
    }
    for (unsigned p = 0; p < 4; p++) {
        const u64 x = p & 1, y = (p >> 1) & 1;
        CHECK((u64)lut[128 + 2 * p] == addm(x, mm(r1, y, q), q), "bit_lut<%s> q=%llu word %u", word, q, 128 + 2 * p);
        CHECK((u64)lut[128 + 2 * p + 1] == addm(x, negm(mm(r1, y, q), q), q), "bit_lut<%s> q=%llu word %u", word, q, 128 + 2 * p + 1);
    }
}

static void check_modulus(u64 q, u64 n, unsigned log_n) {
    const std::vector<u64> r = roots_of(q, n, log_n);
    CHECK(r[0] == 1 && h::exp_mod(q, r[1], 2) == q - 1, "q=%llu n=%llu: roots[1] is not a square root of -1", q, n);
    check_bit_lut<u64>(r, q, "u64");
    if (q >> 32 == 0) {
        check_bit_lut<uint32_t>(r, q, "u32");
        const auto a = h::bit_lut<u64>(r.data(), q);
        const auto b = h::bit_lut<uint32_t>(r.data(), q);
        for (int i = 0; i < 136; i++) CHECK(a[i] == b[i], "q=%llu: bit_lut<u64> and <u32> differ at word %d", q, i);
    }
    const u64 two32 = (u64)(((u128)1 << 32) % q), two64 = (u64)(((u128)1 << 64) % q);
    for (u64 k = 0; k < n; k++) {
        const u64 w = r[k], wi = h::inv_mod(q, w);
        CHECK(mm(w, wi, q) == 1, "q=%llu: inv_mod(%llu) = %llu", q, w, wi);
        for (u64 x : {w, wi}) {
            const Tw s = h::shoup_pair<Tw>(x, q);
            const u128 num = (u128)x << 64, rem = num - (u128)s.wp * q;                 // x < 2^63: x 2^64 fits 127 bits
            CHECK(s.w == x && s.wp == (u64)(num / q) && rem < q, "q=%llu: shoup_pair(%llu) = {%llu, %llu}", q, x, s.w, s.wp);
            if (q >> 32 == 0) {
                const Tw32 s32 = h::shoup32_pair<Tw32>(x, q);
                const u128 num32 = (u128)x << 32;
                CHECK(s32.w == x && s32.wp == (u64)(num32 / q) && num32 - (u128)s32.wp * q < q, "q=%llu: shoup32_pair(%llu) = {%u, %u}", q, x, s32.w, s32.wp);
            }
            const Tw pm = h::pm_pair<Tw>(x, q), mg = h::mg_pair<Tw>(x, q);
            CHECK(pm.w == x && pm.wp == mm(x, two32, q), "q=%llu: pm_pair(%llu) = {%llu, %llu}", q, x, pm.w, pm.wp);
            CHECK(mg.w == mm(x, two32, q) && mg.wp == mm(x, two64, q), "q=%llu: mg_pair(%llu) = {%llu, %llu}", q, x, mg.w, mg.wp);
        }
    }
    for (u64 x : {(u64)2, (u64)3, n, q - 1, q / 2}) CHECK(mm(h::inv_mod(q, x), x % q, q) == 1, "q=%llu: inv_mod(%llu)", q, x);
    const uint32_t lo = (uint32_t)q;                                                    // every modulus is odd
    CHECK((uint32_t)(lo * (0u - h::neg_inv32(lo))) == 1u, "neg_inv32(%u) = %u", lo, h::neg_inv32(lo));
}

int main() {
    const u64 moduli[] = {65537ull, 0x0a3c8001ull, 2305843009211596801ull, 2305842979148922881ull, 9223372036844421121ull};
    for (u64 q : moduli)
        for (unsigned log_n : {3u, 4u}) check_modulus(q, 1ull << log_n, log_n);
    for (uint32_t p : {0x0a3c8001u, 0x0a320001u, 0x0a318001u, 1u, 3u, 0xffffffffu})
        CHECK((uint32_t)(p * (0u - h::neg_inv32(p))) == 1u, "neg_inv32(%u)", p);
    for (unsigned log_n : {0u, 1u, 3u, 4u, 13u, 20u})
        for (u64 i = 0; i < (1ull << log_n); i += (log_n > 10 ? 997 : 1)) {
            const u64 b = h::bitrev(i, log_n);
            CHECK(b < (1ull << log_n) && h::bitrev(b, log_n) == i, "bitrev(%llu, %u) = %llu", i, log_n, b);
        }
    CHECK(h::bitrev(1, 4) == 8 && h::bitrev(6, 3) == 3, "bitrev values");
    CHECK(h::exp_mod(65537, 3, 65536) == 1 && h::exp_mod(65537, 3, 32768) == 65536 && h::mulmod(~0ull, ~0ull, 9223372036844421121ull) == mm(~0ull, ~0ull, 9223372036844421121ull), "exp_mod / mulmod values");
    if (g_failures) {
        printf("%d host table checks FAILED\n", g_failures);
        return 1;
    }
    printf("all host table tests passed\n");
    return 0;
}
