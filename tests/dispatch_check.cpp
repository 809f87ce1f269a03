// Stand-alone host program for tests/test_dispatch.py: prints which tag every helper of csrc/dispatch.h hands to its body, one line per call of the helper.
#include <cstdio>
#include <type_traits>

#include "dispatch.h"

using namespace seg;

template <class T> const char* name_of() {
    if (std::is_same<T, float>::value) return "float";
    if (std::is_same<T, f16>::value) return "f16";
    if (std::is_same<T, bf16>::value) return "bf16";
    return "?";
}

int main() {
    for (int dt = 0; dt <= 2; ++dt) {
        printf("by_dtype %d:", dt);
        by_dtype(dt, [&](auto t) { printf(" %s(%d)", name_of<tag_type<decltype(t)>>(), dtype_of<tag_type<decltype(t)>>::v); });
        printf("\n");
    }
    for (int b = 0; b <= 1; ++b) {
        printf("by_bool %d:", b);
        by_bool(b != 0, [&](auto f) {
            constexpr bool v = f();               // usable as a template argument
            printf(" %s", std::integral_constant<bool, v>::value ? "true" : "false");
        });
        printf("\n");
    }
    for (int v : {1, 2, 3, 4, 5, 0, 6, -1, 7}) {
        printf("by_int %d:", v);
        const bool hit = by_int<1, 2, 3, 4, 5, 0>(v, [&](auto k) {
            constexpr int c = k();
            printf(" %d", std::integral_constant<int, c>::value);
        });
        printf(" -> %s\n", hit ? "true" : "false");
    }
    return 0;
}
