// delta.h -- device code of the rank-aware dense update (host side: delta.hip; lora.py "rank-aware association"):
//
//   k_delta_fwd   out_i (N x K) = s_i B_i A_i                                   i < n, one launch
//   k_delta_bwd   dA_i (r_i x K) = s_i B_i^T Z_i,  dB_i (N x r_i) = s_i Z_i A_i^T   i < n, one launch for both
//
// with A_i (r_i x K), B_i (N x r_i), Z_i (N x K) row-major fp32 and s_i = scale_i * (scale_dev_i ? *scale_dev_i : 1), the device
// word read by the kernel.  These are the 1 + T updates of one MTLoRALinear, each a GEMM far too small for a launch of its own
// (288 x 96 x 256 at stage 0 of c5:256), so a launch treats them as ONE problem:
//
//   work unit   one 32 x 32 output tile of one update, owned by one wave from the first product to the store: the reduction is
//               never split, every output element is produced once in a fixed order (no atomics, no partials, no memset; results
//               are bit-reproducible).  Units are numbered update-major (backward: an update's dA tiles, then its dB tiles; a
//               null output has no tiles) and dealt DL_WAVES to a workgroup; the wave finds its update in a by-value table read
//               through the kernarg segment (the unit index is wave-uniform).  n = 9, N x K = 288 x 96 gives 243 forward units,
//               about one per CU.
//   matrix op   v_mfma_f32_32x32x2_f32 through mtl_mma(Frag<float>): a lane holds 8 reduction elements per operand and step
//               (slot e of half h <-> element  8 (lane >> 5) + 4 h + e  of the step, the same map on both operands), the two lane
//               halves of the wave together 16, so the reduction advances 16 per Frag pair.  The next step's operands are in
//               flight while the eight MFMAs of the current one issue.
//   operands    straight from global memory into the fragment registers, no LDS: a tile's two operand panels are read by exactly
//               one wave exactly once, so staging them would add a write, a barrier and a read for no reuse.  Three load shapes:
//                 DL_COL    the reduction index selects the row, the lane's tile index the column: one 128-byte row segment per
//                           half wave and slot, fully coalesced.  A as the B operand of the forward; B^T and Z of dA.
//                 DL_ROW4   the lane's tile index selects a 16-byte-aligned row, the reduction runs along it: two 16-byte loads
//                           per lane and step.  Z and A of dB (their rows have K elements, K % 4 == 0).
//                 DL_ROW    as DL_ROW4 for rows of ANY element stride: eight dword loads per lane and step, the 32 bytes of a lane
//                           and the 64 of its row shared by the two halves.  B of the forward: its row stride r_i need not be a
//                           multiple of 4, which rules 16-byte loads out, and the L2-resident 32 x r_i panel is read once.
//   edges       a reduction tail (r_i, N or K not a multiple of 16) and partial tiles are ZERO-FILLED operands (0 * 0 on both
//               sides, so nothing non-finite is invented) -- no address outside a row or a matrix is ever formed into a load -- and
//               the store skips what lies outside the output.  Non-finite inputs propagate as in any fp32 matmul.
#pragma once

#include "common.h"

namespace {

constexpr int DL_T = 32;                        // tile edge
constexpr int DL_KS = 16;                       // reduction elements per step (8 per lane half)
constexpr int DL_WAVES = 4;                     // units per workgroup, one per SIMD
constexpr int DL_MAXN = MTLORA_MAX_TASKS + 1;   // the shared update and the tasks'

struct DeltaUpd {
    const float* A;          // (r x K)
    const float* B;          // (N x r)
    const float* Z;          // backward: (N x K)
    float* out;              // forward: Delta W (N x K); backward: dA (r x K) or null
    float* dB;               // backward: (N x r) or null
    const float* scale_dev;  // 1-element device scale or null
    float scale;
    int r;
    int first;               // index of the update's first unit
    int n_dA;                // backward: how many of its units are dA tiles (they come first)
};
struct DeltaParams {
    DeltaUpd u[DL_MAXN];
    int64_t N, K;
    int n, tiles_n, tiles_k, units;
};
typedef const __attribute__((address_space(4))) DeltaParams* DeltaKargs;

enum { DL_ROW = 0, DL_ROW4 = 1, DL_COL = 2 };

// the lane's 8 operand elements of one step: tile index `idx` (valid below n_idx), reduction elements k .. k + 7 (valid below n_k)
template <int KIND>
__device__ __forceinline__ Frag<float> delta_load(const float* __restrict__ p, int64_t ld, int64_t idx, int64_t n_idx, int64_t k, int64_t n_k) {
    Frag<float> f;
    const bool in = idx < n_idx;
    if constexpr (KIND == DL_ROW4) {  // (n_k % 4 == 0: a vector is inside or outside as a whole)
#pragma unroll
        for (int h = 0; h < 2; ++h)
            f.v[h] = (in && k + 4 * h < n_k) ? *reinterpret_cast<const u32x4*>(p + idx * ld + k + 4 * h) : u32x4{0u, 0u, 0u, 0u};
    } else {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t kk = k + 4 * h + e;
                float v = 0.f;
                if (in && kk < n_k) v = KIND == DL_ROW ? p[idx * ld + kk] : p[kk * ld + idx];
                f.v[h][e] = __builtin_bit_cast(uint32_t, v);
            }
    }
    return f;
}

// out[a0 + i][b0 + j] = s * sum_k opA(i, k) opB(k, j) for one 32 x 32 tile, the whole reduction in this wave
template <int KA, int KB>
__device__ __forceinline__ void delta_tile(const float* __restrict__ a, int64_t lda, int64_t a0, int64_t na, const float* __restrict__ b,
                                           int64_t ldb, int64_t b0, int64_t nb, int64_t nk, float s, float* __restrict__ out, int64_t ldo,
                                           int lane) {
    const int64_t ia = a0 + (lane & 31), ib = b0 + (lane & 31), kg = (lane >> 5) * 8;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    Frag<float> fa = delta_load<KA>(a, lda, ia, na, kg, nk), fb = delta_load<KB>(b, ldb, ib, nb, kg, nk);
    for (int64_t k = 0; k < nk; k += DL_KS) {
        // (behind the end both loads are all-zero without touching memory)
        const Frag<float> ga = delta_load<KA>(a, lda, ia, na, k + DL_KS + kg, nk), gb = delta_load<KB>(b, ldb, ib, nb, k + DL_KS + kg, nk);
        mtl_mma(fa, fb, acc);
        fa = ga;
        fb = gb;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t i = a0 + mtl_d_row(lane, r), j = b0 + mtl_d_col(lane);
        if (i < na && j < nb) out[i * ldo + j] = s * acc[r];
    }
}

// the update that owns unit `unit` (first[] ascends; empty updates repeat a value and are passed over)
__device__ __forceinline__ int delta_owner(DeltaKargs P, int n, int unit) {
    int i = 0;
    while (i + 1 < n && P->u[i + 1].first <= unit) ++i;
    return i;
}

__global__ __launch_bounds__(DL_WAVES * 64) void k_delta_fwd(const DeltaParams params) {
    DeltaKargs P = (DeltaKargs)__builtin_amdgcn_kernarg_segment_ptr();
    const int lane = threadIdx.x & 63;
    const int unit = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * DL_WAVES + (threadIdx.x >> 6)));
    if (unit >= P->units) return;
    const int i = delta_owner(P, P->n, unit);
    const int t = unit - P->u[i].first;
    const int64_t N = P->N, K = P->K, r = P->u[i].r;
    float s = P->u[i].scale;
    if (P->u[i].scale_dev) s *= *P->u[i].scale_dev;
    delta_tile<DL_ROW, DL_COL>(P->u[i].B, r, (int64_t)(t / P->tiles_k) * DL_T, N, P->u[i].A, K, (int64_t)(t % P->tiles_k) * DL_T, K, r, s,
                               P->u[i].out, K, lane);
}

__global__ __launch_bounds__(DL_WAVES * 64) void k_delta_bwd(const DeltaParams params) {
    DeltaKargs P = (DeltaKargs)__builtin_amdgcn_kernarg_segment_ptr();
    const int lane = threadIdx.x & 63;
    const int unit = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * DL_WAVES + (threadIdx.x >> 6)));
    if (unit >= P->units) return;
    const int i = delta_owner(P, P->n, unit);
    int t = unit - P->u[i].first;
    const int64_t N = P->N, K = P->K, r = P->u[i].r;
    float s = P->u[i].scale;
    if (P->u[i].scale_dev) s *= *P->u[i].scale_dev;
    if (t < P->u[i].n_dA) {  // dA[rho][k] = s sum_n B[n][rho] Z[n][k]
        delta_tile<DL_COL, DL_COL>(P->u[i].B, r, (int64_t)(t / P->tiles_k) * DL_T, r, P->u[i].Z, K, (int64_t)(t % P->tiles_k) * DL_T, K, N, s,
                                   P->u[i].out, K, lane);
    } else {  // dB[n][rho] = s sum_k Z[n][k] A[rho][k]
        t -= P->u[i].n_dA;
        const int tiles_r = (int)((r + DL_T - 1) / DL_T);
        delta_tile<DL_ROW4, DL_ROW4>(P->u[i].Z, K, (int64_t)(t / tiles_r) * DL_T, N, P->u[i].A, K, (int64_t)(t % tiles_r) * DL_T, r, K, s,
                                     P->u[i].dB, r, lane);
    }
}

}  // namespace
