// host_dispatch.hpp — a runtime integer to a template argument: the one size switch of the launchers (plain C++17, no HIP).
#pragma once
#include <type_traits>

namespace fhe {

// f(std::integral_constant<int, V>{}) for the V in [Lo, Hi] that equals value; on_miss, without calling f, when there is none.
// Call sites pass a generic lambda: dispatch_int<8, 12>(log_n, hipErrorNotSupported, [&](auto lp) { return run<lp()>(a, st); });
template <int Lo, int Hi, class R, class F>
R dispatch_int(int value, R on_miss, F &&f) {
    if constexpr (Lo > Hi) {
        return on_miss;
    } else {
        if (value == Lo) return f(std::integral_constant<int, Lo>{});
        return dispatch_int<Lo + 1, Hi>(value, on_miss, f);
    }
}

}  // namespace fhe
