// test_dispatch.cpp — csrc/host_dispatch.hpp: dispatch_int reaches f exactly once with the matching compile-time value for
// every value of the range, and returns on_miss without calling f outside it.  Needs neither the library nor a GPU.
#include <cstdio>
#include <initializer_list>
#include <type_traits>

#include "../csrc/host_dispatch.hpp"

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            failures++;                                                   \
        }                                                                 \
    } while (0)

template <int Lo, int Hi>
static void check_range() {
    for (int v = Lo; v <= Hi; v++) {
        int calls = 0, seen = -1;
        const int r = fhe::dispatch_int<Lo, Hi>(v, -1, [&](auto c) {
            static_assert(decltype(c)::value >= Lo && decltype(c)::value <= Hi, "a value outside the range was instantiated");
            constexpr int V = c;      // usable as a template argument
            calls++;
            seen = std::integral_constant<int, V>::value;
            return 100 + V;
        });
        CHECK(calls == 1);
        CHECK(seen == v);
        CHECK(r == 100 + v);
    }
    for (int v : {Lo - 1, Hi + 1, 0, -7}) {
        int calls = 0;
        const int r = fhe::dispatch_int<Lo, Hi>(v, -1, [&](auto c) {
            calls++;
            return (int)c;
        });
        CHECK(calls == 0);
        CHECK(r == -1);
    }
}

int main() {
    check_range<4, 13>();
    check_range<8, 12>();
    check_range<13, 14>();
    if (failures) {
        printf("%d dispatch tests FAILED\n", failures);
        return 1;
    }
    printf("all dispatch tests passed\n");
    return 0;
}
