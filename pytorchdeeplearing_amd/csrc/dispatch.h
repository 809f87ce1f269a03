// Host side only: turn the runtime values of a launch (run dtype, flags, small integers) into the template arguments of its kernel.  Every helper calls the
// body with a tag TYPE that carries the value, so the body names its kernel once and the lists at the call sites are the set of instantiations the library
// carries.  None of them falls through silently: an unknown dtype aborts, and by_int() reports a value that is not in its list.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "common.h"

namespace seg {

template <class T> struct type_tag { using type = T; };
template <class Tag> using tag_type = typename Tag::type;        // using T = tag_type<decltype(t)>;

[[noreturn]] inline void no_kernel(const char* what, int v) {
    fprintf(stderr, "segengine: %s: no kernel for %d (internal error)\n", what, v);
    abort();
}

// f(type_tag<float | f16 | bf16>{})
template <class F> void by_dtype(int dtype, F&& f) {
    if (dtype == DT_F32) f(type_tag<float>{});
    else if (dtype == DT_F16) f(type_tag<f16>{});
    else if (dtype == DT_BF16) f(type_tag<bf16>{});
    else no_kernel("run dtype", dtype);
}

// f(std::true_type{} | std::false_type{})
template <class F> void by_bool(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// f(std::integral_constant<int, V>{}) for the first V of the list that equals v; false (and no call) when none does.  A caller whose ladder had a catch-all
// maps v to the listed value first.
template <int... Vs, class F> bool by_int(int v, F&& f) {
    return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

}  // namespace seg
