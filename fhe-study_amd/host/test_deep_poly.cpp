// test_deep_poly.cpp — the host side of the scalar sums and inner products on the deep chain (csrc/rns_tables.hpp:
// deep_lincomb_each, deep_lincomb_words, deep_tensorsum_each, deep_tensorsum_words and the launch formulas),
// without the library or a GPU.  Every (output, limb, input) of a call lies in exactly one launch, within the launch's
// bounds, with the weight and constant the call's arrays hold for it; what a launch does not cover is zero; the groups of
// inputs of one block follow each other, so that a carried launch finds the words of the one before; the launch counts are
// the formulas.  Also the program the sanitizers run on this arithmetic (`make san_deep_poly`).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/rns_tables.hpp"

using fhe::host::u64;

static int failures = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            failures++;                                              \
        }                                                            \
    } while (0)

static u64 ceil_div(u64 a, u64 b) { return (a + b - 1) / b; }

// arrays sized exactly, on the heap: an index past the call's arrays is the sanitizer's to report
static void lincomb_case(unsigned limbs, unsigned outputs, unsigned count, bool consts) {
    std::vector<u64> w((size_t)outputs * count * limbs), k((size_t)outputs * limbs);
    for (size_t i = 0; i < w.size(); i++) w[i] = 1000 + i;
    for (size_t i = 0; i < k.size(); i++) k[i] = 7000000 + i;
    std::vector<unsigned> seen(w.size(), 0);
    u64 launches = 0;
    unsigned last_o0 = 0, last_i0 = 0, last_r0 = 0, last_nr = 0;
    const int rc = fhe::host::deep_lincomb_each(limbs, outputs, count, [&](unsigned o0, unsigned no, unsigned i0, unsigned nl, unsigned r0, unsigned nr) {
        CHECK(no >= 1 && no <= fhe::kDeepLinOutputs && nl >= 1 && nl <= fhe::kDeepPolyLimbs && nr >= 1 && nr <= fhe::kDeepLinInputs);
        CHECK(o0 + no <= outputs && i0 + nl <= limbs && r0 + nr <= count);
        if (r0 > 0) CHECK(launches > 0 && last_o0 == o0 && last_i0 == i0 && last_r0 + last_nr == r0);   // a carried launch follows its block's former group
        last_o0 = o0, last_i0 = i0, last_r0 = r0, last_nr = nr;
        launches++;
        fhe::DeepLinWords s;
        fhe::host::deep_lincomb_words(w.data(), consts ? k.data() : nullptr, limbs, count, o0, no, i0, nl, r0, nr, &s);
        for (unsigned l = 0; l < fhe::kDeepPolyLimbs; l++)
            for (unsigned o = 0; o < fhe::kDeepLinOutputs; o++) {
                const bool in = l < nl && o < no;
                CHECK(s.k[l][o] == (in && consts ? k[(size_t)(o0 + o) * limbs + i0 + l] : 0));
                for (unsigned r = 0; r < fhe::kDeepLinInputs; r++) {
                    if (in && r < nr) {
                        const size_t at = ((size_t)(o0 + o) * count + r0 + r) * limbs + i0 + l;
                        CHECK(s.w[l][o][r] == w[at]);
                        seen[at]++;
                    } else {
                        CHECK(s.w[l][o][r] == 0);
                    }
                }
            }
        return 0;
    });
    CHECK(rc == 0);
    for (unsigned x : seen) CHECK(x == 1);
    CHECK(launches == fhe::host::deep_lincomb_launches(limbs, outputs, count));
    CHECK(launches == ceil_div(limbs, 8) * ceil_div(outputs, 4) * ceil_div(count, 8));
}

static void tensorsum_case(unsigned limbs, unsigned count, bool weighted) {
    std::vector<u64> w((size_t)count * limbs);
    for (size_t i = 0; i < w.size(); i++) w[i] = 500 + i;
    std::vector<unsigned> seen(w.size(), 0);
    u64 launches = 0;
    unsigned last_i0 = 0, last_p0 = 0, last_np = 0;
    const int rc = fhe::host::deep_tensorsum_each(limbs, count, [&](unsigned i0, unsigned nl, unsigned p0, unsigned np) {
        CHECK(nl >= 1 && nl <= fhe::kDeepPolyLimbs && np >= 1 && np <= fhe::kDeepDotPairs && i0 + nl <= limbs && p0 + np <= count);
        if (p0 > 0) CHECK(launches > 0 && last_i0 == i0 && last_p0 + last_np == p0);
        last_i0 = i0, last_p0 = p0, last_np = np;
        launches++;
        fhe::DeepDotWords s;
        fhe::host::deep_tensorsum_words(weighted ? w.data() : nullptr, limbs, i0, nl, p0, np, &s);
        for (unsigned l = 0; l < fhe::kDeepPolyLimbs; l++)
            for (unsigned r = 0; r < fhe::kDeepDotPairs; r++) {
                if (l < nl && r < np) {
                    const size_t at = (size_t)(p0 + r) * limbs + i0 + l;
                    CHECK(s.w[l][r] == (weighted ? w[at] : 1));
                    seen[at]++;
                } else {
                    CHECK(s.w[l][r] == 0);
                }
            }
        return 0;
    });
    CHECK(rc == 0);
    for (unsigned x : seen) CHECK(x == 1);
    CHECK(launches == fhe::host::deep_tensorsum_launches(limbs, count));
    CHECK(launches == ceil_div(limbs, 8) * ceil_div(count, 16));
}

int main() {
    static_assert(sizeof(fhe::DeepLinWords) == 2048 + 256 && sizeof(fhe::DeepDotWords) == 1024, "the sizes DESIGN.md §39 states");
    for (unsigned limbs : {1u, 7u, 8u, 9u, 16u, 17u, 24u, 31u, 32u})
        for (unsigned outputs : {1u, 3u, 4u, 5u, 16u})
            for (unsigned count : {1u, 7u, 8u, 9u, 15u, 16u, 17u, 64u}) {
                lincomb_case(limbs, outputs, count, true);
                lincomb_case(limbs, outputs, count, false);
            }
    for (unsigned limbs : {1u, 7u, 8u, 9u, 16u, 17u, 24u, 31u, 32u})
        for (unsigned count : {1u, 4u, 5u, 15u, 16u, 17u, 33u, 64u}) {
            tensorsum_case(limbs, count, true);
            tensorsum_case(limbs, count, false);
        }
    // a failing launch stops the walk and is what the walk returns
    unsigned calls = 0;
    CHECK(fhe::host::deep_lincomb_each(32, 16, 64, [&](unsigned, unsigned, unsigned, unsigned, unsigned, unsigned) { return ++calls == 3 ? -7 : 0; }) == -7 && calls == 3);
    calls = 0;
    CHECK(fhe::host::deep_tensorsum_each(32, 64, [&](unsigned, unsigned, unsigned, unsigned) { return ++calls == 2 ? -5 : 0; }) == -5 && calls == 2);
    CHECK(fhe::host::deep_lincomb_launches(24, 4, 15) == 6 && fhe::host::deep_tensorsum_launches(24, 16) == 3);
    if (failures) {
        printf("%d deep poly partition checks FAILED\n", failures);
        return 1;
    }
    printf("all deep poly partition tests passed\n");
    return 0;
}
