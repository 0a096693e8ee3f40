// dispatch.h -- host-only vocabulary of the entry points: which element types an entry accepts, the ladders that turn a runtime
// mtlora_dtype into a template argument, and the null / alignment tests over pointer lists.  Every host-side type selection of the
// library goes through one of the mtl_dispatch_* below; a new entry uses these helpers instead of a ladder of its own.
#pragma once
#include <initializer_list>
#include <type_traits>

#include "common.h"

template <typename T>
struct MtlTag {
    using type = T;
};
template <int V>
using MtlInt = std::integral_constant<int, V>;

// accepted-type sets: one bit per mtlora_dtype code
constexpr unsigned MTL_DT_ALL = 1u << MTLORA_F32 | 1u << MTLORA_BF16 | 1u << MTLORA_F16;
constexpr unsigned MTL_DT_F32_BF16 = 1u << MTLORA_F32 | 1u << MTLORA_BF16;  // losses, metrics, column sums
constexpr unsigned MTL_DT_16 = 1u << MTLORA_BF16 | 1u << MTLORA_F16;        // the implicit-hidden Mlp
static inline bool mtl_dtype_in(int dtype, unsigned set) { return dtype >= 0 && dtype < 32 && (set >> dtype & 1u); }
static inline int mtl_vec_elems(int dtype) { return dtype == MTLORA_F32 ? 4 : 8; }  // elements per 16 bytes (mtl_elem_size: internal.h)

// f(MtlTag<T>{}) for the element type of `dtype`; f's result is returned.  The caller has checked dtype against the matching set
template <typename F>
decltype(auto) mtl_dispatch_dtype(int dtype, F&& f) {
    if (dtype == MTLORA_F32) return f(MtlTag<float>{});
    if (dtype == MTLORA_F16) return f(MtlTag<f16>{});
    return f(MtlTag<bf16>{});
}
template <typename F>
decltype(auto) mtl_dispatch_dtype16(int dtype, F&& f) {
    if (dtype == MTLORA_F16) return f(MtlTag<f16>{});
    return f(MtlTag<bf16>{});
}
template <typename F>
decltype(auto) mtl_dispatch_f32_bf16(int dtype, F&& f) {
    if (dtype == MTLORA_F32) return f(MtlTag<float>{});
    return f(MtlTag<bf16>{});
}

// a pair is valid when neither side is outside MTL_DT_ALL and there is no bf16 <-> fp16 mix
static inline bool mtl_dtype_pair_ok(int a, int b) {
    return mtl_dtype_in(a, MTL_DT_ALL) && mtl_dtype_in(b, MTL_DT_ALL) && (a == MTLORA_F32 || b == MTLORA_F32 || a == b);
}
// f(MtlTag<TA>{}, MtlTag<TB>{}) for the seven pairs: fp32 / fp32, and fp32 on either side or neither for fp16 and bf16
template <typename F>
decltype(auto) mtl_dispatch_dtype_pair(int a, int b, F&& f) {
    auto with16 = [&](auto t16) {
        using T = typename decltype(t16)::type;
        if (a == MTLORA_F32) return f(MtlTag<float>{}, MtlTag<T>{});
        if (b == MTLORA_F32) return f(MtlTag<T>{}, MtlTag<float>{});
        return f(MtlTag<T>{}, MtlTag<T>{});
    };
    if (a == MTLORA_F32 && b == MTLORA_F32) return f(MtlTag<float>{}, MtlTag<float>{});
    if (a == MTLORA_F16 || b == MTLORA_F16) return with16(MtlTag<f16>{});  // fp16 autocast (the reference's default, main.py:341)
    return with16(MtlTag<bf16>{});
}

// ------------------------------------------------------------------------------------------------
// validation: single pointers and per-stream arrays (arrays[j][k], k < n) go through the same helper
// ------------------------------------------------------------------------------------------------
using MtlPtrs = std::initializer_list<const void*>;
using MtlArrs = std::initializer_list<const void* const*>;
template <typename T>
const void* const* mtl_arr(T* const* a) {
    return reinterpret_cast<const void* const*>(a);
}

// every pointer, every array and every array element is required
static inline bool mtl_any_null(MtlPtrs one, int n = 0, MtlArrs per = {}) {
    for (const void* q : one)
        if (!q) return true;
    for (const void* const* a : per) {
        if (!a) return true;
        for (int k = 0; k < n; ++k)
            if (!a[k]) return true;
    }
    return false;
}

// optional pointers / arrays / elements may be null (0 is aligned); align: a power of two
static inline bool mtl_any_misaligned(MtlPtrs one, int n = 0, MtlArrs per = {}, uintptr_t align = 16) {
    uintptr_t bits = 0;
    for (const void* q : one) bits |= (uintptr_t)q;
    for (const void* const* a : per)
        for (int k = 0; a && k < n; ++k) bits |= (uintptr_t)a[k];
    return (bits & (align - 1)) != 0;
}
