// Host-side dispatch from a runtime value to a template instantiation of a kernel launcher (hipcc and g++ -DMG_EMU alike).
// Every site spells out its own list: a value that is not listed instantiates nothing.
//     dispatch_int<1, 2, 3, 4, 6, 8>(G, [&](auto GG) { MG_LAUNCH((kernel<decltype(GG)::value>), ...); });
#pragma once
#include "mg_device.h"

#include <type_traits>

namespace mg {

// f(std::integral_constant<int, Vi>{}) for the Vi that equals value; returns whether one did (no match: nothing runs).
template <int... Vs, typename F>
inline bool dispatch_int(int value, F&& f) {
    return ((value == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

// The same for an epilogue id, with the LAST entry of the list as the fallback of every id that is not listed (the `default:` of a
// switch); returns whether epi itself was listed.
template <int... Es, typename F>
inline bool dispatch_epi(int epi, F&& f) {
    if (dispatch_int<Es...>(epi, f)) return true;
    constexpr int list[] = {Es...};
    f(std::integral_constant<int, list[sizeof...(Es) - 1]>{});
    return false;
}

}  // namespace mg

// Permission for a kernel's large dynamic-LDS request, asked once per expansion - inside a function template or a generic lambda: once
// per instantiation.  The initialisation of a function-local static is race-free.
#define MG_SET_MAX_SMEM_ONCE(kern, bytes)                                      \
    do {                                                                       \
        static const bool mg_smem_set_ = (MG_SET_MAX_SMEM(kern, bytes), true); \
        (void)mg_smem_set_;                                                    \
    } while (0)
