// ln.h -- the LayerNorm family's device code (host dispatch: layernorm.hip), HBM-bound streaming kernels.
//
//   k_ln_fwd / k_ln_bwd   LayerNorm over the last dim, fp32 or bf16 input, fp32 or bf16 OUTPUT written directly
//                         in the dtype the following MTLoRALinear consumes (the reference's autocast path
//                         writes an fp32 normalised tensor and then casts it: 2.5x the bytes), fp32 statistics.
//                         A row is handled by LPR lanes (8..64) holding it entirely in registers (two-pass mean /
//                         variance, no E[x^2] cancellation); 64/LPR rows per wave-instruction, 16 B per lane.
//                         Backward also produces dgamma / dbeta: per-thread column accumulators over the rows a
//                         workgroup visits, LDS reduction over its row groups, per-workgroup partials, and a
//                         deterministic second-stage reduce.
#pragma once

#include "common.h"
#include "internal.h"
#include "vec.h"

namespace {

constexpr int LN_MAXV = 8;  // most 16-byte vectors per lane per row (C <= 64 lanes * 8 vec * VEC); kernels are specialised on 3 / 8

struct LnParams {
    const void* x;
    const float* gamma;
    const float* beta;
    void* y;
    float* mean;
    float* rstd;
    // backward
    const void* dy;
    void* dx;
    const void* add;  // optional (dtype of x): dx = add + LayerNorm-backward(dy) -- the gradient of the skip path that forks off x
    float* part;  // [gridDim.x][2][C]
    int64_t M;
    int C;
    float eps;
    // patch-merging gather (PatchMerging: 2x2 neighbourhood concat before its LayerNorm): x / dx / add are (B, mg_H*mg_W, C/4)
    // token tensors and row r = (b, y2, x2) of the normalised (M, C) matrix is [x(2y2,2x2) | x(2y2+1,2x2) | x(2y2,2x2+1) |
    // x(2y2+1,2x2+1)]; mg_W == 0: plain rows
    int mg_H, mg_W;
    // fused residual (Swin block: x_new = shortcut + DropPath(branch) immediately followed by LayerNorm(x_new)):
    //   forward : x = shortcut, rb = branch (dtype of y), xsum = x_new (dtype of x) written by the kernel, then normalised
    //   backward: dbr = rscale[sample] * dx (dtype of dy): the branch gradient, written next to dx (= the shortcut gradient)
    const void* rb;
    void* xsum;
    void* dbr;
    const float* rscale;  // [B] per-sample DropPath scale or null (1)
    int64_t rows_per_sample;
    // multi-stream form (task-enabled block: ONE shortcut, 1+T branches, 1+T normalised outputs): stream k = blockIdx.y of the
    // forward launch / an inner loop of k_resln_bwd_multi; rscale is then [nk][B]
    int nk;
    const void* rb_k[MTLORA_MAX_TASKS + 1];
    void* xsum_k[MTLORA_MAX_TASKS + 1];
    void* y_k[MTLORA_MAX_TASKS + 1];
    float* mean_k[MTLORA_MAX_TASKS + 1];
    float* rstd_k[MTLORA_MAX_TASKS + 1];
    const void* dy_k[MTLORA_MAX_TASKS + 1];
    const void* add_k[MTLORA_MAX_TASKS + 1];
    void* dbr_k[MTLORA_MAX_TASKS + 1];
    // independent streams through the SAME LayerNorm in one launch (multi_x: blockIdx.y selects x / y / statistics, backward
    // dy / dx / addend and a partial-sum slab; PatchMerging's norm over the shared + task tensors)
    int multi_x;
    const void* x_k[MTLORA_MAX_TASKS + 1];
    void* dx_k[MTLORA_MAX_TASKS + 1];
};
// arrays of the parameter block are indexed through the kernarg segment (constant address space): dynamic indexing of the
// by-value copy would move the whole struct to scratch
typedef const __attribute__((address_space(4))) LnParams* LnKargs;

// row / d for 0 <= row < rows, 0 < d <= rows.  The int64 quotient costs ~100 VALU instructions per lane (software division),
// once per row group -- more than the arithmetic of a 96-wide row; every shape in use has rows < 2^31, where one 32-bit unsigned
// division (~20 instructions) gives the same result.  `rows` is wave-uniform.
__device__ __forceinline__ int64_t row_div(int64_t row, int64_t d, int64_t rows) {
    if (rows <= (int64_t)0x7FFFFFFF) return (int64_t)((uint32_t)row / (uint32_t)d);
    return row / d;
}

// element offset of column `col` (a multiple of the vector width) of row `row` in x / dx
struct LnRow {
    int64_t base;  // plain: row * C; merged: offset of token (2y2, 2x2)
};
__device__ __forceinline__ LnRow ln_row(const LnParams& p, int64_t row) {
    LnRow r;
    if (p.mg_W == 0) {
        r.base = row * p.C;
    } else {
        const int W2 = p.mg_W >> 1, H2 = p.mg_H >> 1, Cs = p.C >> 2;
        const int64_t b = row_div(row, (int64_t)H2 * W2, p.M);
        const int rem = (int)(row - b * H2 * W2);
        const int y2 = rem / W2, x2 = rem - y2 * W2;
        r.base = ((b * p.mg_H + 2 * y2) * p.mg_W + 2 * x2) * (int64_t)Cs;
    }
    return r;
}
// per-lane constant part: offset of column `col` relative to the row base
__device__ __forceinline__ int64_t ln_col(const LnParams& p, int col) {
    if (p.mg_W == 0) return col;
    const int Cs = p.C >> 2, q = col / Cs, within = col - q * Cs;
    return ((int64_t)(q & 1) * p.mg_W + (q >> 1)) * Cs + within;  // (dy = q & 1, dx = q >> 1)
}

// UNR row groups per wave iteration: their loads are issued back to back and kept as raw 16-byte vectors (a wave with a
// single 1.5 KB row group in flight per iteration ran at 1.5-2.8 TB/s for the stage-1..3 shapes)
template <typename TI, typename TO, int LPR, int MAXV, bool RES>
__global__ __launch_bounds__(256) void k_ln_fwd(const LnParams p) {
    constexpr int VE = ET<TI>::VEC;
    constexpr int RPW = 64 / LPR;  // rows per wave per group
    constexpr int UNR = MAXV <= 3 ? 4 : 1;  // (the wide-row specialisation already holds 8 vectors per lane)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane / LPR, lr = lane % LPR;
    const int nvec = p.C / VE;
    const TI* x = reinterpret_cast<const TI*>(p.x);
    TO* y = reinterpret_cast<TO*>(p.y);
    float* mean_out = p.mean;
    float* rstd_out = p.rstd;
    const void* rb_ptr = p.rb;
    void* xs_ptr = p.xsum;
    const float* rscale = p.rscale;
    if (p.multi_x) {
        LnKargs K = (LnKargs)__builtin_amdgcn_kernarg_segment_ptr();
        const int k = blockIdx.y;
        x = reinterpret_cast<const TI*>(K->x_k[k]);
        y = reinterpret_cast<TO*>(K->y_k[k]);
        mean_out = K->mean_k[k];
        rstd_out = K->rstd_k[k];
        if constexpr (RES) {  // independent streams, each with its own residual: x_k + s_k * branch_k
            rb_ptr = K->rb_k[k];
            xs_ptr = K->xsum_k[k];
            if (rscale) rscale += (int64_t)k * (p.M / p.rows_per_sample);
        }
    }
    if constexpr (RES) {
        if (p.nk > 0) {  // multi-stream launch: blockIdx.y selects the branch / outputs; the shortcut x is shared (an in-kernel
                         // loop over the streams that reads it once was slower: 473 vs 424 us at stage 0 -- fewer workgroups)
            LnKargs K = (LnKargs)__builtin_amdgcn_kernarg_segment_ptr();
            const int k = blockIdx.y;
            y = reinterpret_cast<TO*>(K->y_k[k]);
            mean_out = K->mean_k[k];
            rstd_out = K->rstd_k[k];
            rb_ptr = K->rb_k[k];
            xs_ptr = K->xsum_k[k];
            if (rscale) rscale += (int64_t)k * (p.M / p.rows_per_sample);
        }
    }
    float g[MAXV][VE], b[MAXV][VE];
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int v = lr + i * LPR;
#pragma unroll
        for (int e = 0; e < VE; ++e) {
            g[i][e] = v < nvec ? p.gamma[v * VE + e] : 0.f;
            b[i][e] = v < nvec ? p.beta[v * VE + e] : 0.f;
        }
    }
    int64_t coff[MAXV];  // x offset of this lane's vectors relative to the row base (plain or patch-merging gather)
#pragma unroll
    for (int i = 0; i < MAXV; ++i) coff[i] = ln_col(p, (lr + i * LPR < nvec ? lr + i * LPR : 0) * VE);
    const float inv_c = 1.f / (float)p.C;
    const int64_t rows_per_blk = 4 * RPW * UNR;
    for (int64_t r0 = (int64_t)blockIdx.x * rows_per_blk; r0 < p.M; r0 += (int64_t)gridDim.x * rows_per_blk) {
        u32x4 raw[UNR][MAXV];
        int64_t row[UNR], xbs[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            row[u] = r0 + (int64_t)(wave * UNR + u) * RPW + sub;
            const int64_t xb = ln_row(p, row[u] < p.M ? row[u] : 0).base;
            xbs[u] = xb;
#pragma unroll
            for (int i = 0; i < MAXV; ++i) {
                const int v = lr + i * LPR;
                raw[u][i] = (row[u] < p.M && v < nvec) ? *reinterpret_cast<const u32x4*>(x + xb + coff[i])
                                                      : u32x4{0u, 0u, 0u, 0u};
            }
        }
        if constexpr (RES) {  // x_new = shortcut + s * branch, stored (rounded to the stream dtype) and normalised
            const TO* rb = reinterpret_cast<const TO*>(rb_ptr);
            TI* xs = reinterpret_cast<TI*>(xs_ptr);
            // the branch vectors and the per-sample scales are fetched for ALL row groups before the first x_new store: the
            // compiler cannot move a load above a store that may alias it, so loading inside the store loop left one branch
            // vector in flight at a time (the shortcut loads above are already issued back to back)
            constexpr bool PRE = sizeof(TO) * VE <= 16;  // a branch vector fits one 16-byte register (all but fp32 branch / bf16 x)
            u32x4 braw[PRE ? UNR : 1][PRE ? MAXV : 1];
            float scv[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const bool rok = row[u] < p.M;
                scv[u] = (rok && rscale) ? rscale[row_div(row[u], p.rows_per_sample, p.M)] : 1.f;
                if constexpr (PRE) {
#pragma unroll
                    for (int i = 0; i < MAXV; ++i) {
                        const int v = lr + i * LPR;
                        u32x4 b = {0u, 0u, 0u, 0u};
                        if (rok && v < nvec) {
                            if constexpr (sizeof(TO) * VE == 16) {
                                b = *reinterpret_cast<const u32x4*>(rb + xbs[u] + coff[i]);
                            } else {
                                const u32x2 h2 = *reinterpret_cast<const u32x2*>(rb + xbs[u] + coff[i]);
                                b[0] = h2[0];
                                b[1] = h2[1];
                            }
                        }
                        braw[u][i] = b;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                if (row[u] >= p.M) continue;
                const float sc = scv[u];
#pragma unroll
                for (int i = 0; i < MAXV; ++i) {
                    const int v = lr + i * LPR;
                    if (v < nvec) {
                        float fb[8], fx[8];
                        // (branch and x_new share the layout of x: plain rows, or the token tensor of the merge gather)
                        if constexpr (!PRE) {
                            ld_n<TO, VE>(rb + xbs[u] + coff[i], fb);
                        } else if constexpr (sizeof(TO) == 4) {
                            const f32x4 q4 = __builtin_bit_cast(f32x4, braw[u][i]);
                            fb[0] = q4[0];
                            fb[1] = q4[1];
                            fb[2] = q4[2];
                            fb[3] = q4[3];
                        } else if constexpr (VE == 8) {
                            cvt_vec<TO>(braw[u][i], fb);
                        } else {
                            fb[0] = mtl_lo2<TO>(braw[u][i][0]);
                            fb[1] = mtl_hi2<TO>(braw[u][i][0]);
                            fb[2] = mtl_lo2<TO>(braw[u][i][1]);
                            fb[3] = mtl_hi2<TO>(braw[u][i][1]);
                        }
                        cvt_vec<TI>(raw[u][i], fx);
#pragma unroll
                        for (int e = 0; e < VE; ++e) fx[e] += sc * fb[e];
                        raw[u][i] = pack_vec<TI>(fx);
                        *reinterpret_cast<u32x4*>(xs + xbs[u] + coff[i]) = raw[u][i];
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            float f[8];
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < MAXV; ++i) {
                cvt_vec<TI>(raw[u][i], f);
#pragma unroll
                for (int e = 0; e < VE; ++e) s += f[e];  // out-of-range vectors are zero
            }
            const float mean = group_sum<LPR>(s) * inv_c;
            float q = 0.f;
#pragma unroll
            for (int i = 0; i < MAXV; ++i) {
                if (lr + i * LPR < nvec) {
                    cvt_vec<TI>(raw[u][i], f);
#pragma unroll
                    for (int e = 0; e < VE; ++e) {
                        const float d = f[e] - mean;
                        q += d * d;
                    }
                }
            }
            const float rstd = rsqrtf(group_sum<LPR>(q) * inv_c + p.eps);
            if (row[u] < p.M) {
                if (lr == 0) {
                    mean_out[row[u]] = mean;
                    rstd_out[row[u]] = rstd;
                }
#pragma unroll
                for (int i = 0; i < MAXV; ++i) {
                    const int v = lr + i * LPR;
                    if (v < nvec) {
                        cvt_vec<TI>(raw[u][i], f);
                        float o[8];
#pragma unroll
                        for (int e = 0; e < VE; ++e) o[e] = (f[e] - mean) * rstd * g[i][e] + b[i][e];
                        st_vec<TO, VE>(y + row[u] * p.C + v * VE, o);
                    }
                }
            }
        }
    }
}

// TX: dtype of x and dx; TG: dtype of dy
template <typename TX, typename TG, int LPR, int MAXV>
__global__ __launch_bounds__(256) void k_ln_bwd(const LnParams p) {
    constexpr int VE = ET<TX>::VEC;  // elements per lane-vector (x drives the vector width; dy read with the same count)
    constexpr int RPW = 64 / LPR;
    extern __shared__ __attribute__((aligned(16))) float sm[];  // [4 * RPW row groups][2][C] column partials
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane / LPR, lr = lane % LPR;
    const int nvec = p.C / VE;
    const TX* x = reinterpret_cast<const TX*>(p.x);
    const TG* dy = reinterpret_cast<const TG*>(p.dy);
    TX* dx = reinterpret_cast<TX*>(p.dx);
    const TX* addp = reinterpret_cast<const TX*>(p.add);
    const float* mean_in = p.mean;
    const float* rstd_in = p.rstd;
    void* dbr_ptr = p.dbr;
    const float* rscale_in = p.rscale;
    float* part_out = p.part + (int64_t)blockIdx.x * 2 * p.C;
    if (p.multi_x) {
        LnKargs K = (LnKargs)__builtin_amdgcn_kernarg_segment_ptr();
        const int k = blockIdx.y;
        x = reinterpret_cast<const TX*>(K->x_k[k]);
        dy = reinterpret_cast<const TG*>(K->dy_k[k]);
        dx = reinterpret_cast<TX*>(K->dx_k[k]);
        addp = reinterpret_cast<const TX*>(K->add_k[k]);
        mean_in = K->mean_k[k];
        rstd_in = K->rstd_k[k];
        part_out = p.part + ((int64_t)k * gridDim.x + blockIdx.x) * 2 * p.C;
        dbr_ptr = K->dbr_k[k];
        if (rscale_in) rscale_in += (int64_t)k * (p.M / p.rows_per_sample);
    }
    float g[MAXV][VE], ag[MAXV][VE], ab[MAXV][VE];
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int v = lr + i * LPR;
#pragma unroll
        for (int e = 0; e < VE; ++e) {
            g[i][e] = v < nvec ? p.gamma[v * VE + e] : 0.f;
            ag[i][e] = 0.f;
            ab[i][e] = 0.f;
        }
    }
    int64_t coff[MAXV];  // x / dx / addend offsets of this lane's vectors relative to the row base
#pragma unroll
    for (int i = 0; i < MAXV; ++i) coff[i] = ln_col(p, (lr + i * LPR < nvec ? lr + i * LPR : 0) * VE);
    // UNR row groups per wave iteration, loads issued back to back as raw vectors before any arithmetic (as in k_ln_fwd)
    // (bf16 rows hold 8 elements per vector: two row groups in flight need > 256 VGPRs -- one wave per SIMD -- and ran slower)
    constexpr int UNR = (MAXV <= 3 && sizeof(TX) == 4) ? 2 : 1;
    constexpr int GW = sizeof(TG) == sizeof(TX) ? 4 : (sizeof(TG) == 2 ? 2 : 8);  // dwords of dy per lane-vector
    const int64_t rows_per_blk = 4 * RPW * UNR;
    for (int64_t r0 = (int64_t)blockIdx.x * rows_per_blk; r0 < p.M; r0 += (int64_t)gridDim.x * rows_per_blk) {
        u32x4 rx[UNR][MAXV], ra[UNR][MAXV];
        uint32_t rg[UNR][MAXV][GW];
        int64_t row[UNR], xb[UNR];
        float mean[UNR], rstd[UNR], scv[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            row[u] = r0 + (int64_t)(wave * UNR + u) * RPW + sub;
            const bool rv = row[u] < p.M;
            xb[u] = ln_row(p, rv ? row[u] : 0).base;
            mean[u] = rv ? mean_in[row[u]] : 0.f;
            rstd[u] = rv ? rstd_in[row[u]] : 0.f;
            // (fetched with the other operands: a load placed after the dx stores cannot be hoisted above them)
            scv[u] = (rv && dbr_ptr && rscale_in) ? rscale_in[row_div(row[u], p.rows_per_sample, p.M)] : 1.f;
#pragma unroll
            for (int i = 0; i < MAXV; ++i) {
                const int v = lr + i * LPR;
                const bool ok = rv && v < nvec;
                rx[u][i] = ok ? *reinterpret_cast<const u32x4*>(x + xb[u] + coff[i]) : u32x4{0u, 0u, 0u, 0u};
                const TG* gp = dy + (rv ? row[u] : 0) * p.C + (v < nvec ? v : 0) * VE;
                if constexpr (GW == 4) {
                    const u32x4 t = ok ? *reinterpret_cast<const u32x4*>(gp) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
                    for (int q = 0; q < 4; ++q) rg[u][i][q] = t[q];
                } else if constexpr (GW == 2) {
                    const u32x2 t = ok ? *reinterpret_cast<const u32x2*>(gp) : u32x2{0u, 0u};
                    rg[u][i][0] = t[0];
                    rg[u][i][1] = t[1];
                } else {
                    const u32x4 t0 = ok ? *reinterpret_cast<const u32x4*>(gp) : u32x4{0u, 0u, 0u, 0u};
                    const u32x4 t1 = ok ? *reinterpret_cast<const u32x4*>(gp + 4) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        rg[u][i][q] = t0[q];
                        rg[u][i][4 + q] = t1[q];
                    }
                }
                ra[u][i] = (ok && addp) ? *reinterpret_cast<const u32x4*>(addp + xb[u] + coff[i]) : u32x4{0u, 0u, 0u, 0u};
            }
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const bool rv = row[u] < p.M;
            float xh[MAXV][VE], gy[MAXV][VE];
            float c1 = 0.f, c2 = 0.f;
#pragma unroll
            for (int i = 0; i < MAXV; ++i) {
                float fx[8], fg[8];
                cvt_vec<TX>(rx[u][i], fx);
                if constexpr (GW == 4) {
                    cvt_vec<TG>(u32x4{rg[u][i][0], rg[u][i][1], rg[u][i][2], rg[u][i][3]}, fg);
                } else if constexpr (GW == 2) {  // x fp32 (4 per vector), dy bf16
                    fg[0] = mtl_lo2<TG>(rg[u][i][0]);
                    fg[1] = mtl_hi2<TG>(rg[u][i][0]);
                    fg[2] = mtl_lo2<TG>(rg[u][i][1]);
                    fg[3] = mtl_hi2<TG>(rg[u][i][1]);
                } else {  // x bf16 (8 per vector), dy fp32
#pragma unroll
                    for (int q = 0; q < 8; ++q) fg[q] = __builtin_bit_cast(float, rg[u][i][q]);
                }
                // out-of-range rows / vectors were loaded as zeros with mean = rstd = 0: every term below is then 0
#pragma unroll
                for (int e = 0; e < VE; ++e) {
                    const float h = (fx[e] - mean[u]) * rstd[u];
                    xh[i][e] = h;
                    ag[i][e] += fg[e] * h;
                    ab[i][e] += fg[e];
                    const float t = fg[e] * g[i][e];
                    gy[i][e] = t;
                    c1 += t;
                    c2 += t * h;
                }
            }
            c1 = group_sum<LPR>(c1) / p.C;
            c2 = group_sum<LPR>(c2) / p.C;
            if (rv) {
#pragma unroll
                for (int i = 0; i < MAXV; ++i) {
                    const int v = lr + i * LPR;
                    if (v < nvec) {
                        float o[8], fa[8];
                        cvt_vec<TX>(ra[u][i], fa);
#pragma unroll
                        for (int e = 0; e < VE; ++e) o[e] = rstd[u] * (gy[i][e] - c1 - xh[i][e] * c2) + fa[e];
                        st_vec<TX, VE>(dx + xb[u] + coff[i], o);
                        if (dbr_ptr) {  // gradient of the residual branch (layout of x / dx): DropPath scale, dtype of dy
                            const float sc = scv[u];
#pragma unroll
                            for (int e = 0; e < VE; ++e) o[e] *= sc;
                            st_vec<TG, VE>(reinterpret_cast<TG*>(dbr_ptr) + xb[u] + coff[i], o);
                        }
                    }
                }
            }
        }
    }
    // workgroup reduction of the column accumulators: the 4 waves x RPW row groups hold the same columns; each
    // group writes its own LDS slab and the slabs are summed in a fixed order (deterministic, no float atomics)
    float* mine = sm + (size_t)(wave * RPW + sub) * 2 * p.C;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int v = lr + i * LPR;
        if (v < nvec) {
#pragma unroll
            for (int e = 0; e < VE; ++e) {
                mine[v * VE + e] = ag[i][e];
                mine[p.C + v * VE + e] = ab[i][e];
            }
        }
    }
    __syncthreads();
    float* dst = part_out;
    for (int i = threadIdx.x; i < 2 * p.C; i += 256) {
        float t = 0.f;
        for (int gi = 0; gi < 4 * RPW; ++gi) t += sm[(size_t)gi * 2 * p.C + i];
        dst[i] = t;
    }
}

// Backward of the multi-stream residual + LayerNorm (task-enabled block half): for its rows a wave walks the nk streams --
// two in flight -- and forms per stream  dx_k = add_k + LN'(dy_k)  (never stored),  d_branch_k = s_k dx_k  (stored, dtype of
// dy), while  d_shortcut = sum_k dx_k  and the dgamma / dbeta partials accumulate in registers across the streams: one pass
// instead of nk LayerNorm backward launches + their reduces + the shared-residual backward (which re-read all nk dx_k).
template <typename TX, typename TG, int LPR, int MAXV>
__global__ __launch_bounds__(256) void k_resln_bwd_multi(const LnParams p) {
    constexpr int VE = ET<TX>::VEC;
    constexpr int RPW = 64 / LPR;
    constexpr int GW = sizeof(TG) == sizeof(TX) ? 4 : (sizeof(TG) == 2 ? 2 : 8);
    extern __shared__ __attribute__((aligned(16))) float sm[];
    LnKargs K = (LnKargs)__builtin_amdgcn_kernarg_segment_ptr();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane / LPR, lr = lane % LPR;
    const int nvec = p.C / VE;
    TX* dsh = reinterpret_cast<TX*>(p.dx);
    const int64_t Bn = p.M / p.rows_per_sample;
    float g[MAXV][VE], ag[MAXV][VE], ab[MAXV][VE];
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int v = lr + i * LPR;
#pragma unroll
        for (int e = 0; e < VE; ++e) {
            g[i][e] = v < nvec ? p.gamma[v * VE + e] : 0.f;
            ag[i][e] = 0.f;
            ab[i][e] = 0.f;
        }
    }
    struct Regs {
        u32x4 rx[MAXV], ra[MAXV];
        uint32_t rg[MAXV][GW];
        float mean, rstd, sc;
    };
    const int64_t rows_per_blk = 4 * RPW;
    for (int64_t r0 = (int64_t)blockIdx.x * rows_per_blk; r0 < p.M; r0 += (int64_t)gridDim.x * rows_per_blk) {
        const int64_t row = r0 + wave * RPW + sub;
        const bool rv = row < p.M;
        const int64_t rbase = (rv ? row : 0) * p.C;
        float dsum[MAXV][VE];
#pragma unroll
        for (int i = 0; i < MAXV; ++i)
#pragma unroll
            for (int e = 0; e < VE; ++e) dsum[i][e] = 0.f;
        auto load = [&](Regs& R, int k) __attribute__((always_inline)) {
            const TX* x = reinterpret_cast<const TX*>(K->xsum_k[k]);
            const TG* dy = reinterpret_cast<const TG*>(K->dy_k[k]);
            const TX* addp = reinterpret_cast<const TX*>(K->add_k[k]);
            R.mean = rv ? K->mean_k[k][row] : 0.f;
            R.rstd = rv ? K->rstd_k[k][row] : 0.f;
            R.sc = (rv && p.rscale) ? p.rscale[(int64_t)k * Bn + row_div(row, p.rows_per_sample, p.M)] : 1.f;
#pragma unroll
            for (int i = 0; i < MAXV; ++i) {
                const int v = lr + i * LPR;
                const bool ok = rv && v < nvec;
                const int64_t off = rbase + (v < nvec ? v : 0) * VE;
                R.rx[i] = ok ? *reinterpret_cast<const u32x4*>(x + off) : u32x4{0u, 0u, 0u, 0u};
                R.ra[i] = (ok && addp) ? *reinterpret_cast<const u32x4*>(addp + off) : u32x4{0u, 0u, 0u, 0u};
                const TG* gp = dy + off;
                if constexpr (GW == 4) {
                    const u32x4 t = ok ? *reinterpret_cast<const u32x4*>(gp) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
                    for (int q = 0; q < 4; ++q) R.rg[i][q] = t[q];
                } else if constexpr (GW == 2) {
                    const u32x2 t = ok ? *reinterpret_cast<const u32x2*>(gp) : u32x2{0u, 0u};
                    R.rg[i][0] = t[0];
                    R.rg[i][1] = t[1];
                } else {
                    const u32x4 t0 = ok ? *reinterpret_cast<const u32x4*>(gp) : u32x4{0u, 0u, 0u, 0u};
                    const u32x4 t1 = ok ? *reinterpret_cast<const u32x4*>(gp + 4) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        R.rg[i][q] = t0[q];
                        R.rg[i][4 + q] = t1[q];
                    }
                }
            }
        };
        auto compute = [&](Regs& R, int k) __attribute__((always_inline)) {
            TG* dbr = reinterpret_cast<TG*>(K->dbr_k[k]);
            float xh[MAXV][VE], gy[MAXV][VE];
            float c1 = 0.f, c2 = 0.f;
#pragma unroll
            for (int i = 0; i < MAXV; ++i) {
                float fx[8], fg[8];
                cvt_vec<TX>(R.rx[i], fx);
                if constexpr (GW == 4) {
                    cvt_vec<TG>(u32x4{R.rg[i][0], R.rg[i][1], R.rg[i][2], R.rg[i][3]}, fg);
                } else if constexpr (GW == 2) {
                    fg[0] = mtl_lo2<TG>(R.rg[i][0]);
                    fg[1] = mtl_hi2<TG>(R.rg[i][0]);
                    fg[2] = mtl_lo2<TG>(R.rg[i][1]);
                    fg[3] = mtl_hi2<TG>(R.rg[i][1]);
                } else {
#pragma unroll
                    for (int q = 0; q < 8; ++q) fg[q] = __builtin_bit_cast(float, R.rg[i][q]);
                }
#pragma unroll
                for (int e = 0; e < VE; ++e) {
                    const float h = (fx[e] - R.mean) * R.rstd;
                    xh[i][e] = h;
                    ag[i][e] += fg[e] * h;
                    ab[i][e] += fg[e];
                    const float t = fg[e] * g[i][e];
                    gy[i][e] = t;
                    c1 += t;
                    c2 += t * h;
                }
            }
            c1 = group_sum<LPR>(c1) / p.C;
            c2 = group_sum<LPR>(c2) / p.C;
            if (rv) {
#pragma unroll
                for (int i = 0; i < MAXV; ++i) {
                    const int v = lr + i * LPR;
                    if (v < nvec) {
                        float o[8], fa[8];
                        cvt_vec<TX>(R.ra[i], fa);
#pragma unroll
                        for (int e = 0; e < VE; ++e) {
                            o[e] = R.rstd * (gy[i][e] - c1 - xh[i][e] * c2) + fa[e];
                            dsum[i][e] += o[e];
                            o[e] *= R.sc;
                        }
                        if (dbr) st_vec<TG, VE>(dbr + rbase + v * VE, o);
                    }
                }
            }
        };
        if constexpr (sizeof(TX) == 4) {  // two streams in flight (bf16 rows: 8 elements per vector, that needs > 256 VGPRs)
            Regs A, Bq;
            load(A, 0);
            for (int k = 0; k < p.nk; k += 2) {
                if (k + 1 < p.nk) load(Bq, k + 1);
                compute(A, k);
                if (k + 1 < p.nk) {
                    if (k + 2 < p.nk) load(A, k + 2);
                    compute(Bq, k + 1);
                }
            }
        } else {
            Regs A;
            for (int k = 0; k < p.nk; ++k) {
                load(A, k);
                compute(A, k);
            }
        }
        if (rv) {
#pragma unroll
            for (int i = 0; i < MAXV; ++i) {
                const int v = lr + i * LPR;
                if (v < nvec) st_vec<TX, VE>(dsh + rbase + v * VE, dsum[i]);
            }
        }
    }
    float* mine = sm + (size_t)(wave * RPW + sub) * 2 * p.C;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int v = lr + i * LPR;
        if (v < nvec) {
#pragma unroll
            for (int e = 0; e < VE; ++e) {
                mine[v * VE + e] = ag[i][e];
                mine[p.C + v * VE + e] = ab[i][e];
            }
        }
    }
    __syncthreads();
    float* dst = p.part + (int64_t)blockIdx.x * 2 * p.C;
    for (int i = threadIdx.x; i < 2 * p.C; i += 256) {
        float t = 0.f;
        for (int gi = 0; gi < 4 * RPW; ++gi) t += sm[(size_t)gi * 2 * p.C + i];
        dst[i] = t;
    }
}

// second stage: one workgroup per 64 columns; its 16 waves stride over the partial rows (coalesced 256-byte reads, 4
// independent chains each: 8 dependent iterations for 512 partials instead of 32), then a fixed-order LDS combine ->
// deterministic
constexpr int LN_RW = 16;
__global__ __launch_bounds__(64 * LN_RW) void k_ln_reduce(const float* part, float* dgamma, float* dbeta, int nblk, int C) {
    __shared__ float sm[LN_RW][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;  // column in [0, 2C)
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (c < 2 * C) {
        int b = wave;
        for (; b + 3 * LN_RW < nblk; b += 4 * LN_RW) {
            a0 += part[(int64_t)b * 2 * C + c];
            a1 += part[(int64_t)(b + LN_RW) * 2 * C + c];
            a2 += part[(int64_t)(b + 2 * LN_RW) * 2 * C + c];
            a3 += part[(int64_t)(b + 3 * LN_RW) * 2 * C + c];
        }
        for (; b < nblk; b += LN_RW) a0 += part[(int64_t)b * 2 * C + c];
    }
    sm[wave][lane] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (wave == 0 && c < 2 * C) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < LN_RW; ++w) t += sm[w][lane];
        if (c < C)
            dgamma[c] = t;
        else
            dbeta[c - C] = t;
    }
}

}  // namespace
