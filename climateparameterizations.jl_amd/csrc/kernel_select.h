// kernel_select.h — host-only helpers that turn a launch's runtime flags into ONE template instantiation.
// Every kernel family of an engine has one selector (or one table) built on these; the launcher and the engine's
// set-attributes function both go through it, so a kernel that can be launched has had its dynamic-LDS limit raised.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "../../include/colnde.h"

// f(std::integral_constant<int, COLNDE_ACT_*>) for every activation a kernel is instantiated for
template <class F>
inline void for_each_act(F&& f) {
    f(std::integral_constant<int, COLNDE_ACT_IDENTITY>{});
    f(std::integral_constant<int, COLNDE_ACT_RELU>{});
    f(std::integral_constant<int, COLNDE_ACT_MISH>{});
    f(std::integral_constant<int, COLNDE_ACT_SWISH>{});
    f(std::integral_constant<int, COLNDE_ACT_TANH>{});
    f(std::integral_constant<int, COLNDE_ACT_LEAKYRELU>{});
}

// ... for the one that equals act; false: act is none of them (f not called)
template <class F>
inline bool with_act(int act, F&& f) {
    bool found = false;
    for_each_act([&](auto A) {
        if (A() == act) {
            f(A);
            found = true;
        }
    });
    return found;
}

// f(std::bool_constant...) for the runtime flags b...: with_bools([&](auto RICH, auto RKC) { k = kernel<RICH(), RKC()>; }, rich, rkc)
template <class F>
inline void with_bools(F&& f) { f(); }
template <class F, class... B>
inline void with_bools(F&& f, bool b, B... rest) {
    if (b) with_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else with_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

template <class K>
inline hipError_t set_max_lds(K* kernel, size_t bytes) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
