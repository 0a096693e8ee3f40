// delta.hip -- host side of the rank-aware dense update (kernels and the work split: delta.h):
//
//   mtlora_delta_fwd   out_i = s_i B_i A_i for the n updates of a layer                        k_delta_fwd, one launch
//   mtlora_delta_bwd   dA_i = s_i B_i^T Z_i and dB_i = s_i Z_i A_i^T, null outputs skipped     k_delta_bwd, one launch
//
// Each entry is  validate -> fill DeltaParams (the by-value unit table) -> launch.  Validation, first failure wins:
//   null arrays -> shape (n, N, K, K % 4, r_i, unit count) -> null elements -> alignment -> an output inside an input
// No workspace, nothing allocated or retained, no host read of a scale: a captured launch replays as it is.
#include "delta.h"
#include "dispatch.h"

namespace {

constexpr int64_t DL_DIM_MAX = ((int64_t)1 << 31) - 1;

int delta_shape(int n, int64_t N, int64_t K, const int32_t* r) {
    if (n < 1 || n > DL_MAXN || N < 1 || K < 1 || N > DL_DIM_MAX || K > DL_DIM_MAX || K % 4) return MTLORA_ERR_SHAPE;
    for (int i = 0; i < n; ++i)
        if (r[i] < 1) return MTLORA_ERR_SHAPE;
    return MTLORA_OK;
}

bool delta_overlap(const float* o, int64_t no, const float* in, int64_t ni) {
    const uintptr_t a = (uintptr_t)o, b = (uintptr_t)in;
    return o && in && a < b + (uintptr_t)ni * 4 && b < a + (uintptr_t)no * 4;
}

// does output o (no elements) reach into A_j, B_j or (backward) Z_j of any update?
bool delta_aliased(const float* o, int64_t no, int n, int64_t N, int64_t K, const int32_t* r, const float* const* A, const float* const* B,
                   const float* const* Z) {
    for (int j = 0; j < n; ++j)
        if (delta_overlap(o, no, A[j], r[j] * K) || delta_overlap(o, no, B[j], N * r[j]) || (Z && delta_overlap(o, no, Z[j], N * K)))
            return true;
    return false;
}

int delta_launch(bool bwd, const DeltaParams& P, hipStream_t s) {
    if (P.units == 0) return MTLORA_OK;  // (backward with every output null)
    const dim3 grid((unsigned)mtl_ceil_div(P.units, DL_WAVES)), block(DL_WAVES * 64);
    if (bwd)
        hipLaunchKernelGGL(k_delta_bwd, grid, block, 0, s, P);
    else
        hipLaunchKernelGGL(k_delta_fwd, grid, block, 0, s, P);
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

}  // namespace

extern "C" {

int mtlora_delta_fwd(int n, int64_t N, int64_t K, const int32_t* r, const float* const* A, const float* const* B, const float* scale,
                     const float* const* scale_dev, float* const* out, void* stream) {
    if (mtl_any_null({r, A, B, scale, out})) return MTLORA_ERR_NULL;
    int st = delta_shape(n, N, K, r);
    if (st != MTLORA_OK) return st;
    const int64_t tiles_n = mtl_ceil_div(N, DL_T), tiles_k = mtl_ceil_div(K, DL_T);
    if (tiles_n * tiles_k * n > DL_DIM_MAX) return MTLORA_ERR_SHAPE;
    if (mtl_any_null({}, n, {mtl_arr(A), mtl_arr(B), mtl_arr(out)})) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({}, n, {mtl_arr(A), mtl_arr(out)}) || mtl_any_misaligned({}, n, {mtl_arr(B), mtl_arr(scale_dev)}, 4))
        return MTLORA_ERR_ALIGN;
    for (int i = 0; i < n; ++i)
        if (delta_aliased(out[i], N * K, n, N, K, r, A, B, nullptr)) return MTLORA_ERR_UNSUPPORTED;
    DeltaParams P = {};
    P.n = n;
    P.N = N;
    P.K = K;
    P.tiles_n = (int)tiles_n;
    P.tiles_k = (int)tiles_k;
    for (int i = 0; i < n; ++i) {
        DeltaUpd& u = P.u[i];
        u.A = A[i];
        u.B = B[i];
        u.out = out[i];
        u.scale_dev = scale_dev ? scale_dev[i] : nullptr;
        u.scale = scale[i];
        u.r = r[i];
        u.first = P.units;
        P.units += (int)(tiles_n * tiles_k);
    }
    return delta_launch(false, P, (hipStream_t)stream);
}

int mtlora_delta_bwd(int n, int64_t N, int64_t K, const int32_t* r, const float* const* A, const float* const* B, const float* scale,
                     const float* const* scale_dev, const float* const* Z, float* const* dA, float* const* dB, void* stream) {
    if (mtl_any_null({r, A, B, scale, Z, dA, dB})) return MTLORA_ERR_NULL;
    int st = delta_shape(n, N, K, r);
    if (st != MTLORA_OK) return st;
    const int64_t tiles_n = mtl_ceil_div(N, DL_T), tiles_k = mtl_ceil_div(K, DL_T);
    int64_t units = 0;
    for (int i = 0; i < n; ++i) units += mtl_ceil_div(r[i], DL_T) * ((dA[i] ? tiles_k : 0) + (dB[i] ? tiles_n : 0));
    if (units > DL_DIM_MAX) return MTLORA_ERR_SHAPE;
    if (mtl_any_null({}, n, {mtl_arr(A), mtl_arr(B), mtl_arr(Z)})) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({}, n, {mtl_arr(A), mtl_arr(Z), mtl_arr(dA)}) ||
        mtl_any_misaligned({}, n, {mtl_arr(B), mtl_arr(dB), mtl_arr(scale_dev)}, 4))
        return MTLORA_ERR_ALIGN;
    for (int i = 0; i < n; ++i)
        if (delta_aliased(dA[i], r[i] * K, n, N, K, r, A, B, Z) || delta_aliased(dB[i], N * r[i], n, N, K, r, A, B, Z))
            return MTLORA_ERR_UNSUPPORTED;
    DeltaParams P = {};
    P.n = n;
    P.N = N;
    P.K = K;
    P.tiles_n = (int)tiles_n;
    P.tiles_k = (int)tiles_k;
    for (int i = 0; i < n; ++i) {
        DeltaUpd& u = P.u[i];
        const int64_t tiles_r = mtl_ceil_div(r[i], DL_T);
        u.A = A[i];
        u.B = B[i];
        u.Z = Z[i];
        u.out = dA[i];
        u.dB = dB[i];
        u.scale_dev = scale_dev ? scale_dev[i] : nullptr;
        u.scale = scale[i];
        u.r = r[i];
        u.first = P.units;
        u.n_dA = dA[i] ? (int)(tiles_r * tiles_k) : 0;
        P.units += u.n_dA + (dB[i] ? (int)(tiles_n * tiles_r) : 0);
    }
    return delta_launch(true, P, (hipStream_t)stream);
}

}  // extern "C"
