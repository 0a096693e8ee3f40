// sum_ln_add.h -- device code of SHARED_MODE "addition" (host dispatch: layernorm.hip; reference lora.py:275-284):
//
//   forward   tot = sum_k y_t[k] (fp32, index order);  out = y + gamma (tot - mean) rstd + beta, rounded once;  mean / rstd saved
//   backward  d_tot = LayerNorm-backward(dout) with tot formed again from y_t;  dy_t[k] = addend[k] + d_tot;  dgamma / dbeta partials
//
// The row layout is k_ln_fwd's (ln.h): LPR lanes hold a row entirely in registers as MAXV 16-byte vectors per lane, 64 / LPR rows
// per wave-instruction, two-pass statistics in fp32.  tot never reaches memory in either direction.  A non-finite value in a row of
// any y_t makes that row's statistics, and with them its out and dy_t, non-finite; rows share nothing but the column sums, so every
// other row is computed exactly as without it, and dgamma carries the NaN.
#pragma once

#include "common.h"
#include "vec.h"

namespace {

constexpr int SNA_MAXV = 16;  // fp32 rows up to 64 lanes * 16 vectors * 4 = 4096; 16-bit rows reach 4096 with 8

struct SnaParams {
    const void* yt[MTLORA_MAX_TASKS];   // the task outputs summed
    const void* add[MTLORA_MAX_TASKS];  // backward: gradient that reached y_t[k] from downstream, or null
    void* dyt[MTLORA_MAX_TASKS];        // backward: add[k] + d_tot
    const void* y;                      // forward: the pretrained output; backward: dout
    void* out;
    const float* gamma;
    const float* beta;
    float* mean;
    float* rstd;
    float* part;  // [gridDim.x][2][C]
    int64_t M;
    int C;
    int n;
    float eps;
};
// (the pointer arrays are indexed through the kernarg segment, as LnKargs of ln.h)
typedef const __attribute__((address_space(4))) SnaParams* SnaKargs;

// tot[i][e] = sum_k y_t[k][row][...] for this lane's vectors; out-of-range rows / vectors give zeros
template <typename T, int LPR, int MAXV>
__device__ __forceinline__ void sna_total(SnaKargs K, int n, bool rv, int64_t rbase, int lr, int nvec, float (&tot)[MAXV][ET<T>::VEC]) {
    constexpr int VE = ET<T>::VEC;
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
#pragma unroll
        for (int e = 0; e < VE; ++e) tot[i][e] = 0.f;
    for (int k = 0; k < n; ++k) {
        const T* src = reinterpret_cast<const T*>(K->yt[k]);
        u32x4 raw[MAXV];
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {  // issued back to back, converted after
            const int v = lr + i * LPR;
            raw[i] = (rv && v < nvec) ? *reinterpret_cast<const u32x4*>(src + rbase + v * VE) : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            float f[8];
            cvt_vec<T>(raw[i], f);
#pragma unroll
            for (int e = 0; e < VE; ++e) tot[i][e] += f[e];
        }
    }
}

template <typename T, int LPR, int MAXV>
__global__ __launch_bounds__(256) void k_sum_ln_add_fwd(const SnaParams p) {
    constexpr int VE = ET<T>::VEC;
    constexpr int RPW = 64 / LPR;
    SnaKargs K = (SnaKargs)__builtin_amdgcn_kernarg_segment_ptr();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane / LPR, lr = lane % LPR;
    const int nvec = p.C / VE;
    const T* y = reinterpret_cast<const T*>(p.y);
    T* out = reinterpret_cast<T*>(p.out);
    const float inv_c = 1.f / (float)p.C;
    const int64_t rows_per_blk = 4 * RPW;
    for (int64_t r0 = (int64_t)blockIdx.x * rows_per_blk; r0 < p.M; r0 += (int64_t)gridDim.x * rows_per_blk) {
        const int64_t row = r0 + wave * RPW + sub;
        const bool rv = row < p.M;
        const int64_t rbase = (rv ? row : 0) * p.C;
        u32x4 ry[MAXV];  // fetched before anything is stored: out may be y
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int v = lr + i * LPR;
            ry[i] = (rv && v < nvec) ? *reinterpret_cast<const u32x4*>(y + rbase + v * VE) : u32x4{0u, 0u, 0u, 0u};
        }
        float tot[MAXV][VE];
        sna_total<T, LPR, MAXV>(K, p.n, rv, rbase, lr, nvec, tot);
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i)
#pragma unroll
            for (int e = 0; e < VE; ++e) s += tot[i][e];  // out-of-range vectors are zero
        const float mean = group_sum<LPR>(s) * inv_c;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            if (lr + i * LPR < nvec) {
#pragma unroll
                for (int e = 0; e < VE; ++e) {
                    const float d = tot[i][e] - mean;
                    q += d * d;
                }
            }
        }
        const float rstd = rsqrtf(group_sum<LPR>(q) * inv_c + p.eps);
        if (rv) {
            if (lr == 0) {
                p.mean[row] = mean;
                p.rstd[row] = rstd;
            }
#pragma unroll
            for (int i = 0; i < MAXV; ++i) {
                const int v = lr + i * LPR;
                if (v < nvec) {
                    float fy[8], g[8], b[8], o[8];
                    cvt_vec<T>(ry[i], fy);
                    ld_n<float, VE>(p.gamma + v * VE, g);
                    ld_n<float, VE>(p.beta + v * VE, b);
#pragma unroll
                    for (int e = 0; e < VE; ++e) o[e] = fy[e] + ((tot[i][e] - mean) * rstd * g[e] + b[e]);
                    st_vec<T, VE>(out + rbase + v * VE, o);
                }
            }
        }
    }
}

template <typename T, int LPR, int MAXV>
__global__ __launch_bounds__(256) void k_sum_ln_add_bwd(const SnaParams p) {
    constexpr int VE = ET<T>::VEC;
    constexpr int RPW = 64 / LPR;
    constexpr bool GREG = MAXV <= 3;  // gamma in registers for the narrow rows; the wide ones read it per row group (cache hits)
    __shared__ float sm[4 * RPW][2][LPR * VE];  // one vector column of every row group's dgamma / dbeta accumulators at a time
    SnaKargs K = (SnaKargs)__builtin_amdgcn_kernarg_segment_ptr();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane / LPR, lr = lane % LPR;
    const int nvec = p.C / VE;
    const T* dout = reinterpret_cast<const T*>(p.y);
    float greg[GREG ? MAXV : 1][VE], ag[MAXV][VE], ab[MAXV][VE];
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int v = lr + i * LPR;
#pragma unroll
        for (int e = 0; e < VE; ++e) {
            if constexpr (GREG) greg[i][e] = v < nvec ? p.gamma[v * VE + e] : 0.f;
            ag[i][e] = 0.f;
            ab[i][e] = 0.f;
        }
    }
    const float inv_c = 1.f / (float)p.C;
    const int64_t rows_per_blk = 4 * RPW;
    for (int64_t r0 = (int64_t)blockIdx.x * rows_per_blk; r0 < p.M; r0 += (int64_t)gridDim.x * rows_per_blk) {
        const int64_t row = r0 + wave * RPW + sub;
        const bool rv = row < p.M;
        const int64_t rbase = (rv ? row : 0) * p.C;
        const float mean = rv ? p.mean[row] : 0.f;
        const float rstd = rv ? p.rstd[row] : 0.f;
        u32x4 rg[MAXV];
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int v = lr + i * LPR;
            rg[i] = (rv && v < nvec) ? *reinterpret_cast<const u32x4*>(dout + rbase + v * VE) : u32x4{0u, 0u, 0u, 0u};
        }
        float xh[MAXV][VE];  // tot, then the normalised tot
        sna_total<T, LPR, MAXV>(K, p.n, rv, rbase, lr, nvec, xh);
        float gy[MAXV][VE];
        float c1 = 0.f, c2 = 0.f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int v = lr + i * LPR;
            float fg[8], g[8];
            cvt_vec<T>(rg[i], fg);
            if constexpr (GREG) {
#pragma unroll
                for (int e = 0; e < VE; ++e) g[e] = greg[i][e];
            } else {
                ld_n<float, VE>(p.gamma + (v < nvec ? v : 0) * VE, g);
            }
            // out-of-range rows / vectors were loaded as zeros (rows: with mean = rstd = 0): every term below is then 0
#pragma unroll
            for (int e = 0; e < VE; ++e) {
                const float h = (xh[i][e] - mean) * rstd;
                xh[i][e] = h;
                ag[i][e] += fg[e] * h;
                ab[i][e] += fg[e];
                const float t = fg[e] * g[e];
                gy[i][e] = t;
                c1 += t;
                c2 += t * h;
            }
        }
        c1 = group_sum<LPR>(c1) * inv_c;
        c2 = group_sum<LPR>(c2) * inv_c;
#pragma unroll
        for (int i = 0; i < MAXV; ++i)
#pragma unroll
            for (int e = 0; e < VE; ++e) gy[i][e] = rstd * (gy[i][e] - c1 - xh[i][e] * c2);  // d_tot
        for (int k = 0; k < p.n; ++k) {
            const T* addp = reinterpret_cast<const T*>(K->add[k]);
            T* dst = reinterpret_cast<T*>(K->dyt[k]);
            u32x4 ra[MAXV];  // fetched before the stores of this k: dy_t[k] may be its addend
#pragma unroll
            for (int i = 0; i < MAXV; ++i) {
                const int v = lr + i * LPR;
                ra[i] = (addp && rv && v < nvec) ? *reinterpret_cast<const u32x4*>(addp + rbase + v * VE) : u32x4{0u, 0u, 0u, 0u};
            }
            if (rv) {
#pragma unroll
                for (int i = 0; i < MAXV; ++i) {
                    const int v = lr + i * LPR;
                    if (v < nvec) {
                        float fa[8], o[8];
                        cvt_vec<T>(ra[i], fa);
#pragma unroll
                        for (int e = 0; e < VE; ++e) o[e] = fa[e] + gy[i][e];
                        st_vec<T, VE>(dst + rbase + v * VE, o);
                    }
                }
            }
        }
    }
    // workgroup reduction of the column accumulators, one vector column (LPR * VE columns) at a time: each of the 4 * RPW row groups
    // writes its slab and the slabs are summed in a fixed order (deterministic, no float atomics); k_ln_reduce sums the workgroups
    float* dst = p.part + (int64_t)blockIdx.x * 2 * p.C;
    const int grp = wave * RPW + sub;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
#pragma unroll
        for (int e = 0; e < VE; ++e) {
            sm[grp][0][lr * VE + e] = ag[i][e];
            sm[grp][1][lr * VE + e] = ab[i][e];
        }
        __syncthreads();
        for (int t = threadIdx.x; t < 2 * LPR * VE; t += 256) {
            const int which = t / (LPR * VE), c = t - which * (LPR * VE);
            const int col = i * LPR * VE + c;
            float a = 0.f;
#pragma unroll
            for (int gi = 0; gi < 4 * RPW; ++gi) a += sm[gi][which][c];
            if (col < p.C) dst[(int64_t)which * p.C + col] = a;
        }
        __syncthreads();
    }
}

}  // namespace
