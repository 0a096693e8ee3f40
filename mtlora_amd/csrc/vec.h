// vec.h -- 16-byte vector load / store / convert helpers and the lane-group sum shared by the streaming kernels (ln.h: LayerNorm
// family; glue.hip: BatchNorm + ReLU, residual + DropPath).  fp32 vectors hold 4 elements, 16-bit vectors 8.
#pragma once

#include "common.h"

namespace {

template <typename T>
__device__ __forceinline__ void ld_vec(const T* p, float (&f)[8]);
template <>
__device__ __forceinline__ void ld_vec<float>(const float* p, float (&f)[8]) {
    f32x4 v = *reinterpret_cast<const f32x4*>(p);
    f[0] = v[0];
    f[1] = v[1];
    f[2] = v[2];
    f[3] = v[3];
}
template <>
__device__ __forceinline__ void ld_vec<bf16>(const bf16* p, float (&f)[8]) {
    Vec16<bf16> v = mtl_ld16<bf16>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = (float)v.e[e];
}
template <>
__device__ __forceinline__ void ld_vec<f16>(const f16* p, float (&f)[8]) {
    Vec16<f16> v = mtl_ld16<f16>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = (float)v.e[e];
}
// store NE consecutive elements
template <typename T, int NE>
__device__ __forceinline__ void st_vec(T* p, const float* f) {
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int e = 0; e < NE; e += 4) *reinterpret_cast<f32x4*>(p + e) = f32x4{f[e], f[e + 1], f[e + 2], f[e + 3]};
    } else if constexpr (NE == 8) {
        Vec16<T> v;
#pragma unroll
        for (int e = 0; e < 8; ++e) v.e[e] = (T)f[e];
        *reinterpret_cast<u32x4*>(p) = v.raw;
    } else {
        *reinterpret_cast<u32x2*>(p) = u32x2{mtl_pack2<T>(f[0], f[1]), mtl_pack2<T>(f[2], f[3])};
    }
}

template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// raw 16-byte vector -> floats
template <typename T>
__device__ __forceinline__ void cvt_vec(const u32x4& r, float (&f)[8]);
template <>
__device__ __forceinline__ void cvt_vec<float>(const u32x4& r, float (&f)[8]) {
    const f32x4 v = __builtin_bit_cast(f32x4, r);
    f[0] = v[0];
    f[1] = v[1];
    f[2] = v[2];
    f[3] = v[3];
}
template <>
__device__ __forceinline__ void cvt_vec<bf16>(const u32x4& r, float (&f)[8]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f[2 * q] = __builtin_bit_cast(float, r[q] << 16);
        f[2 * q + 1] = __builtin_bit_cast(float, r[q] & 0xFFFF0000u);
    }
}
template <>
__device__ __forceinline__ void cvt_vec<f16>(const u32x4& r, float (&f)[8]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f[2 * q] = mtl_lo2<f16>(r[q]);
        f[2 * q + 1] = mtl_hi2<f16>(r[q]);
    }
}

// NE elements of type T -> floats (NE = 4 or 8)
template <typename T, int NE>
__device__ __forceinline__ void ld_n(const T* p, float (&f)[8]) {
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int e = 0; e < NE; e += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(p + e);
            f[e] = v[0];
            f[e + 1] = v[1];
            f[e + 2] = v[2];
            f[e + 3] = v[3];
        }
    } else if constexpr (NE == 8) {
        cvt_vec<T>(*reinterpret_cast<const u32x4*>(p), f);
    } else {
        const u32x2 r = *reinterpret_cast<const u32x2*>(p);
        f[0] = mtl_lo2<T>(r[0]);
        f[1] = mtl_hi2<T>(r[0]);
        f[2] = mtl_lo2<T>(r[1]);
        f[3] = mtl_hi2<T>(r[1]);
    }
}
// floats -> one raw 16-byte vector of T (4 fp32 or 8 bf16)
template <typename T>
__device__ __forceinline__ u32x4 pack_vec(const float (&f)[8]) {
    if constexpr (sizeof(T) == 4) {
        return __builtin_bit_cast(u32x4, f32x4{f[0], f[1], f[2], f[3]});
    } else {
        Vec16<T> v;
#pragma unroll
        for (int e = 0; e < 8; ++e) v.e[e] = (T)f[e];
        return v.raw;
    }
}

}  // namespace
