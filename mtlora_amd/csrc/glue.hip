// glue.hip -- streaming glue kernels beside the LayerNorm family (ln.h / layernorm.hip): the decoder heads' training-mode
// BatchNorm + ReLU and the residual + DropPath of a block half.  HBM-bound; the 16-byte vector helpers are in vec.h.
#include "act_dropout.h"
#include "dispatch.h"
#include "internal.h"
#include "vec.h"

// =================================================================================================
// BatchNorm (training) + optional ReLU over a channels-last (R rows x C channels) matrix -- the decoder heads'
// conv1x1 -> BN -> ReLU (seg_hrnet.py:498-526) evaluated on the (pixels, 1080) matrix.  Replaces ATen's
// batch_norm_*_channels_last kernels + the separate ReLU pass (13 ms/step at ~0.6 TB/s on MI355X).
//   forward : k_bn_stats (per-workgroup column sums / sums of squares -> (count, mean, M2) partials)
//             k_bn_finalize (Chan combine -> mean, rstd, scale = gamma*rstd, shift = beta - mean*scale, running stats)
//             k_bn_apply    (y = relu(x*scale + shift), 16 B per lane)
//   backward: k_bn_bwd_stats (sum dy', sum dy'*xhat with dy' = dy * [y > 0]) -> k_bn_bwd_finalize (dgamma, dbeta)
//             k_bn_bwd_apply (dx = scale * (dy' - mean(dy') - xhat * mean(dy' xhat)))
// A thread owns ONE 16-byte channel vector for all rows it visits (fixed column -> register accumulators).
// =================================================================================================
namespace {

struct BnParams {
    const void* x;
    const void* dy;
    void* y;
    void* dx;
    const float* gamma;
    const float* beta;
    float* running_mean;
    float* running_var;
    float* mean;    // (C)
    float* rstd;    // (C)
    float* scale;   // (C) gamma * rstd
    float* shift;   // (C) beta - mean * scale
    float* part;    // [nblk][2][C] (+ counts)
    float* dgamma;
    float* dbeta;
    float* c1;      // (C) mean(dy')
    float* c2;      // (C) mean(dy' xhat)
    int64_t R;
    int C, VW, rows_per_iter, nblk, relu;
    float momentum, eps;
};

// column sums over the rows of this workgroup: s0 = sum f0(row), s1 = sum f1(row)
template <typename T, bool BWD>
__global__ __launch_bounds__(512) void k_bn_colsum(const BnParams p) {
    constexpr int VE = ET<T>::VEC;
    extern __shared__ __attribute__((aligned(16))) float sm[];  // [rows_per_iter][2][C]
    const int tid = threadIdx.x;
    const int ro = tid / p.VW, v = tid % p.VW;
    const bool active = ro < p.rows_per_iter;
    const T* x = reinterpret_cast<const T*>(p.x);
    const T* dy = reinterpret_cast<const T*>(p.dy);
    float a0[VE], a1[VE], sc[VE], sh[VE], mu[VE], rs[VE];
#pragma unroll
    for (int e = 0; e < VE; ++e) {
        a0[e] = a1[e] = 0.f;
        if (BWD && active) {
            sc[e] = p.scale[v * VE + e];
            sh[e] = p.shift[v * VE + e];
            mu[e] = p.mean[v * VE + e];
            rs[e] = p.rstd[v * VE + e];
        }
    }
    const int64_t rows_blk = mtl_ceil_div(p.R, p.nblk);
    const int64_t r_lo = (int64_t)blockIdx.x * rows_blk;
    int64_t r_hi = r_lo + rows_blk;
    if (r_hi > p.R) r_hi = p.R;
    if (active) {
        constexpr int UN = 4;  // rows in flight per thread (one 16-byte load each; a single load per iteration ran at 2 TB/s)
        for (int64_t r = r_lo + ro; r < r_hi; r += (int64_t)UN * p.rows_per_iter) {
            u32x4 rx[UN], rg[UN];
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                const int64_t rr = r + (int64_t)u * p.rows_per_iter;
                const bool ok = rr < r_hi;
                rx[u] = ok ? *reinterpret_cast<const u32x4*>(x + rr * p.C + v * VE) : u32x4{0u, 0u, 0u, 0u};
                if (BWD) rg[u] = ok ? *reinterpret_cast<const u32x4*>(dy + rr * p.C + v * VE) : u32x4{0u, 0u, 0u, 0u};
            }
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                float fx[8];
                cvt_vec<T>(rx[u], fx);
                if (!BWD) {  // rows past the end were loaded as zeros: they add nothing
#pragma unroll
                    for (int e = 0; e < VE; ++e) {
                        a0[e] += fx[e];
                        a1[e] += fx[e] * fx[e];
                    }
                } else {
                    float fg[8];
                    cvt_vec<T>(rg[u], fg);  // (zero gradient for rows past the end)
#pragma unroll
                    for (int e = 0; e < VE; ++e) {
                        const float yv = fx[e] * sc[e] + sh[e];
                        const float g = (p.relu && yv <= 0.f) ? 0.f : fg[e];
                        a0[e] += g;
                        a1[e] += g * (fx[e] - mu[e]) * rs[e];
                    }
                }
            }
        }
        float* mine = sm + (size_t)ro * 2 * p.C;
#pragma unroll
        for (int e = 0; e < VE; ++e) {
            mine[v * VE + e] = a0[e];
            mine[p.C + v * VE + e] = a1[e];
        }
    }
    __syncthreads();
    float* dst = p.part + (int64_t)blockIdx.x * 2 * p.C;
    for (int i = tid; i < 2 * p.C; i += blockDim.x) {
        float t = 0.f;
        for (int g = 0; g < p.rows_per_iter; ++g) t += sm[(size_t)g * 2 * p.C + i];
        dst[i] = t;
    }
}

// forward finalize: per channel combine (count, sum, sumsq) partials with Chan's formula.
// One workgroup per 64 channels: its 4 waves each fold a strided quarter of the partials (coalesced 256-byte reads),
// then wave 0 folds the four results in a fixed order.
// Finalize kernels: the per-workgroup partials (fp32 sums of x and x^2, resp. of dy' and dy' xhat) are summed in fp64 by
// 16 waves with two independent chains each and combined in a fixed order (deterministic).  Plain fp64 sums carry the
// same information as a Chan fold of the fp32 partials (var = (Q - S^2/R)/R loses < 1e-12 relative in fp64) without the
// two fp64 divisions per partial that made the fold take 29-67 us.
constexpr int BN_FW = 16;
__global__ __launch_bounds__(64 * BN_FW) void k_bn_finalize(const BnParams p) {
    __shared__ double sm[BN_FW][2][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    double s0 = 0.0, q0 = 0.0, s1 = 0.0, q1 = 0.0;
    if (c < p.C) {
        int b = wave;
        for (; b + BN_FW < p.nblk; b += 2 * BN_FW) {
            s0 += p.part[(int64_t)b * 2 * p.C + c];
            q0 += p.part[(int64_t)b * 2 * p.C + p.C + c];
            s1 += p.part[(int64_t)(b + BN_FW) * 2 * p.C + c];
            q1 += p.part[(int64_t)(b + BN_FW) * 2 * p.C + p.C + c];
        }
        for (; b < p.nblk; b += BN_FW) {
            s0 += p.part[(int64_t)b * 2 * p.C + c];
            q0 += p.part[(int64_t)b * 2 * p.C + p.C + c];
        }
    }
    sm[wave][0][lane] = s0 + s1;
    sm[wave][1][lane] = q0 + q1;
    __syncthreads();
    if (wave != 0 || c >= p.C) return;
    double S = 0.0, Q = 0.0;
    for (int w = 0; w < BN_FW; ++w) {
        S += sm[w][0][lane];
        Q += sm[w][1][lane];
    }
    const double n = (double)p.R, mean = S / n;
    double m2 = Q - S * mean;
    m2 = m2 < 0.0 ? 0.0 : m2;
    const double var = m2 / n;
    const float rstd = (float)(1.0 / sqrt(var + (double)p.eps));
    const float sc = p.gamma[c] * rstd;
    p.mean[c] = (float)mean;
    p.rstd[c] = rstd;
    p.scale[c] = sc;
    p.shift[c] = p.beta[c] - (float)mean * sc;
    if (p.running_mean) {
        const double unb = n > 1.0 ? m2 / (n - 1.0) : var;
        p.running_mean[c] = (1.f - p.momentum) * p.running_mean[c] + p.momentum * (float)mean;
        p.running_var[c] = (1.f - p.momentum) * p.running_var[c] + p.momentum * (float)unb;
    }
}

__global__ __launch_bounds__(64 * BN_FW) void k_bn_bwd_finalize(const BnParams p) {
    __shared__ double sm[BN_FW][2][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    double s0 = 0.0, s1 = 0.0, t0 = 0.0, t1 = 0.0;
    if (c < p.C) {
        int b = wave;
        for (; b + BN_FW < p.nblk; b += 2 * BN_FW) {
            s0 += p.part[(int64_t)b * 2 * p.C + c];
            s1 += p.part[(int64_t)b * 2 * p.C + p.C + c];
            t0 += p.part[(int64_t)(b + BN_FW) * 2 * p.C + c];
            t1 += p.part[(int64_t)(b + BN_FW) * 2 * p.C + p.C + c];
        }
        for (; b < p.nblk; b += BN_FW) {
            s0 += p.part[(int64_t)b * 2 * p.C + c];
            s1 += p.part[(int64_t)b * 2 * p.C + p.C + c];
        }
    }
    sm[wave][0][lane] = s0 + t0;
    sm[wave][1][lane] = s1 + t1;
    __syncthreads();
    if (wave != 0 || c >= p.C) return;
    s0 = s1 = 0.0;
    for (int w = 0; w < BN_FW; ++w) {
        s0 += sm[w][0][lane];
        s1 += sm[w][1][lane];
    }
    p.dbeta[c] = (float)s0;
    p.dgamma[c] = (float)s1;
    p.c1[c] = (float)(s0 / (double)p.R);
    p.c2[c] = (float)(s1 / (double)p.R);
}

// a thread owns ONE channel vector (its per-channel constants stay in registers -- re-reading 2-6 per-channel arrays per
// element through the vector cache held the backward at 3.4 TB/s) and walks the rows of its workgroup's slab, 4 in flight
constexpr int BN_APPLY_BLOCKS = 2048;
template <typename T, bool BWD>
__global__ __launch_bounds__(512) void k_bn_apply(const BnParams p) {
    constexpr int VE = ET<T>::VEC;
    constexpr int UN = 4;
    const int tid = threadIdx.x;
    const int ro = tid / p.VW, v = tid % p.VW;
    if (ro >= p.rows_per_iter) return;
    const T* x = reinterpret_cast<const T*>(p.x);
    const T* dy = reinterpret_cast<const T*>(p.dy);
    T* out = reinterpret_cast<T*>(BWD ? p.dx : p.y);
    // forward: y = relu(x * sc + sh);  backward: dx = sc * g + kx * x + k0 with g = dy * [x * sc + sh > 0]
    float sc[VE], sh[VE], kx[VE], k0[VE];
#pragma unroll
    for (int e = 0; e < VE; ++e) {
        const int c = v * VE + e;
        sc[e] = p.scale[c];
        sh[e] = p.shift[c];
        if (BWD) {
            const float t = sc[e] * p.c2[c] * p.rstd[c];
            kx[e] = -t;
            k0[e] = t * p.mean[c] - sc[e] * p.c1[c];
        }
    }
    const int64_t rows_blk = mtl_ceil_div(p.R, (int64_t)gridDim.x);
    const int64_t r_lo = (int64_t)blockIdx.x * rows_blk;
    int64_t r_hi = r_lo + rows_blk;
    if (r_hi > p.R) r_hi = p.R;
    for (int64_t r = r_lo + ro; r < r_hi; r += (int64_t)UN * p.rows_per_iter) {
        u32x4 rx[UN], rg[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int64_t rr = r + (int64_t)u * p.rows_per_iter;
            const bool ok = rr < r_hi;
            rx[u] = ok ? *reinterpret_cast<const u32x4*>(x + rr * p.C + v * VE) : u32x4{0u, 0u, 0u, 0u};
            if (BWD) rg[u] = ok ? *reinterpret_cast<const u32x4*>(dy + rr * p.C + v * VE) : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int64_t rr = r + (int64_t)u * p.rows_per_iter;
            if (rr >= r_hi) continue;
            float fx[8], o[8];
            cvt_vec<T>(rx[u], fx);
            if (!BWD) {
#pragma unroll
                for (int e = 0; e < VE; ++e) {
                    const float yv = fx[e] * sc[e] + sh[e];
                    o[e] = (p.relu && yv < 0.f) ? 0.f : yv;
                }
            } else {
                float fg[8];
                cvt_vec<T>(rg[u], fg);
#pragma unroll
                for (int e = 0; e < VE; ++e) {
                    const float yv = fx[e] * sc[e] + sh[e];
                    const float g = (p.relu && yv <= 0.f) ? 0.f : fg[e];
                    o[e] = sc[e] * g + kx[e] * fx[e] + k0[e];
                }
            }
            st_vec<T, VE>(out + rr * p.C + v * VE, o);
        }
    }
}

int bn_setup(BnParams& p, int64_t R, int64_t C, int dtype) {
    if (!mtl_dtype_in(dtype, MTL_DT_ALL)) return MTLORA_ERR_DTYPE;
    const int ve = mtl_vec_elems(dtype);
    if (R <= 0 || C <= 0 || C % ve) return MTLORA_ERR_SHAPE;
    p.R = R;
    p.C = (int)C;
    p.VW = (int)(C / ve);
    if (p.VW > 512) return MTLORA_ERR_UNSUPPORTED;
    p.rows_per_iter = 512 / p.VW;
    if (p.rows_per_iter > 8) p.rows_per_iter = 8;
    int64_t nblk = mtl_ceil_div(R, 64);
    if (nblk > 512) nblk = 512;
    p.nblk = (int)nblk;
    return MTLORA_OK;
}

}  // namespace

extern "C" {

// scratch: [nblk][2][C] partials + 4 C floats (scale, shift, c1, c2)
int64_t mtlora_bn_scratch_bytes(int64_t R, int64_t C, int dtype) {
    BnParams p = {};
    if (bn_setup(p, R, C, dtype) != MTLORA_OK) return -1;
    return ((int64_t)p.nblk * 2 * C + 4 * C) * 4 + 256;
}

int mtlora_bn_relu_fwd(const void* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                       float momentum, float eps, int relu, void* y, float* save_mean, float* save_rstd,
                       float* save_scale, float* save_shift, int64_t R, int64_t C, int dtype, void* scratch,
                       int64_t scratch_bytes, void* stream) {
    BnParams p = {};
    int st = bn_setup(p, R, C, dtype);
    if (st != MTLORA_OK) return st;
    if (mtl_any_null({x, gamma, beta, y, save_mean, save_rstd, save_scale, save_shift, scratch})) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({x, y, scratch})) return MTLORA_ERR_ALIGN;
    if (scratch_bytes < mtlora_bn_scratch_bytes(R, C, dtype) - 256) return MTLORA_ERR_WORKSPACE;
    p.x = x;
    p.y = y;
    p.gamma = gamma;
    p.beta = beta;
    p.running_mean = running_mean;
    p.running_var = running_var;
    p.mean = save_mean;
    p.rstd = save_rstd;
    p.scale = save_scale;
    p.shift = save_shift;
    p.part = reinterpret_cast<float*>(scratch);
    p.momentum = momentum;
    p.eps = eps;
    p.relu = relu;
    hipStream_t s = (hipStream_t)stream;
    const int threads = (int)mtl_round_up((int64_t)p.rows_per_iter * p.VW, 64);
    const unsigned apply_blocks = (unsigned)(mtl_ceil_div(R, 16) < BN_APPLY_BLOCKS ? mtl_ceil_div(R, 16) : BN_APPLY_BLOCKS);
    const size_t lds = (size_t)p.rows_per_iter * 2 * C * 4;
    const int es = mtl_elem_size(dtype);
    {
        MtlProfScope prof(PK_BN, (double)R * C * es, s);
        mtl_dispatch_dtype(dtype, [&](auto t) {
            hipLaunchKernelGGL((k_bn_colsum<typename decltype(t)::type, false>), dim3(p.nblk), dim3(threads), lds, s, p);
        });
    }
    hipLaunchKernelGGL(k_bn_finalize, dim3((unsigned)mtl_ceil_div(C, 64)), dim3(64 * BN_FW), 0, s, p);
    {
        MtlProfScope prof(PK_BN, (double)R * C * es * 2, s);
        mtl_dispatch_dtype(dtype, [&](auto t) {
            hipLaunchKernelGGL((k_bn_apply<typename decltype(t)::type, false>), dim3(apply_blocks), dim3(threads), 0, s, p);
        });
    }
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

int mtlora_bn_relu_bwd(const void* dy, const void* x, const float* save_mean, const float* save_rstd,
                       const float* save_scale, const float* save_shift, int relu, void* dx, float* dgamma, float* dbeta,
                       int64_t R, int64_t C, int dtype, void* scratch, int64_t scratch_bytes, void* stream) {
    BnParams p = {};
    int st = bn_setup(p, R, C, dtype);
    if (st != MTLORA_OK) return st;
    if (mtl_any_null({dy, x, save_mean, save_rstd, save_scale, save_shift, dx, dgamma, dbeta, scratch})) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({x, dy, dx, scratch})) return MTLORA_ERR_ALIGN;
    if (scratch_bytes < mtlora_bn_scratch_bytes(R, C, dtype) - 256) return MTLORA_ERR_WORKSPACE;
    p.x = x;
    p.dy = dy;
    p.dx = dx;
    p.mean = const_cast<float*>(save_mean);
    p.rstd = const_cast<float*>(save_rstd);
    p.scale = const_cast<float*>(save_scale);
    p.shift = const_cast<float*>(save_shift);
    p.part = reinterpret_cast<float*>(scratch);
    p.c1 = p.part + (int64_t)p.nblk * 2 * C;
    p.c2 = p.c1 + C;
    p.dgamma = dgamma;
    p.dbeta = dbeta;
    p.relu = relu;
    hipStream_t s = (hipStream_t)stream;
    const int threads = (int)mtl_round_up((int64_t)p.rows_per_iter * p.VW, 64);
    const unsigned apply_blocks = (unsigned)(mtl_ceil_div(R, 16) < BN_APPLY_BLOCKS ? mtl_ceil_div(R, 16) : BN_APPLY_BLOCKS);
    const size_t lds = (size_t)p.rows_per_iter * 2 * C * 4;
    const int es = mtl_elem_size(dtype);
    {
        MtlProfScope prof(PK_BN, (double)R * C * es * 2, s);
        mtl_dispatch_dtype(dtype, [&](auto t) {
            hipLaunchKernelGGL((k_bn_colsum<typename decltype(t)::type, true>), dim3(p.nblk), dim3(threads), lds, s, p);
        });
    }
    hipLaunchKernelGGL(k_bn_bwd_finalize, dim3((unsigned)mtl_ceil_div(C, 64)), dim3(64 * BN_FW), 0, s, p);
    {
        MtlProfScope prof(PK_BN, (double)R * C * es * 3, s);
        mtl_dispatch_dtype(dtype, [&](auto t) {
            hipLaunchKernelGGL((k_bn_apply<typename decltype(t)::type, true>), dim3(apply_blocks), dim3(threads), 0, s, p);
        });
    }
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}
}

// =================================================================================================
// residual + DropPath over the 1+T tensors of a block half (swin_transformer_mtlora.py:389-392, 398-408):
//   out_k[m] = res_k[m] + s_k[sample(m)] * y_k[m]        s = DropPath mask / keep (1 when off)
// forward : ONE launch for all k (reads res_k, y_k once, writes out_k) instead of a mul + an add per tensor;
// backward: ONE launch: dy_k = s_k * g_k and, when the residual is SHARED by all k (attention half: every task
//           output adds the same shortcut), d_res = sum_k g_k -- instead of T adds by the autograd engine.
// res / out dtype may be fp32 while y is bf16 (the stage-0 residual stream is fp32 under autocast).
// =================================================================================================
namespace {

struct ResParams {
    const void* res[MTLORA_MAX_TASKS + 1];
    const void* y[MTLORA_MAX_TASKS + 1];   // forward: y_k ; backward: g_k (dtype of out)
    void* out[MTLORA_MAX_TASKS + 1];       // forward: out_k ; backward: dy_k
    void* dres;                            // backward, shared residual: sum_k g_k
    const float* scale;                    // [n][B] or null (all ones)
    int64_t M;
    int C, n, B;
    int64_t rows_per_sample;
};

// TR: dtype of res / out / g ; TY: dtype of y / dy.  DROP: dropout on the branch (proj_drop / the Mlp's output drop, act_dropout.h):
//   out_k = res_k + s_k * keep_k / (1 - p) * y_k ,   dy_k = s_k * keep_k / (1 - p) * g_k   -- the dropped branch never exists in memory
template <typename TR, typename TY, bool DROP>
__global__ __launch_bounds__(256) void k_residual_fwd(const ResParams p, const ActDrop dr) {
    const int64_t nvec = p.M * p.C / 8;
    const int k = blockIdx.y;
    DropoutCfg cfg;
    if constexpr (DROP) {
        cfg = dr.cfg;
        mtl_dropout_resolve(cfg);
    }
    const TR* res = reinterpret_cast<const TR*>(p.res[k]);
    const TY* y = reinterpret_cast<const TY*>(p.y[k]);
    TR* out = reinterpret_cast<TR*>(p.out[k]);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
        const int64_t row = (i * 8) / p.C;
        const float s = p.scale ? p.scale[(int64_t)k * p.B + row / p.rows_per_sample] : 1.f;
        float fr[8], fy[8], o[8];
        if constexpr (sizeof(TR) == 4) {
            ld_vec<TR>(res + i * 8, fr);
            float hi[8];
            ld_vec<TR>(res + i * 8 + 4, hi);
#pragma unroll
            for (int e = 0; e < 4; ++e) fr[4 + e] = hi[e];
        } else {
            ld_vec<TR>(res + i * 8, fr);
        }
        if constexpr (sizeof(TY) == 4) {
            ld_vec<TY>(y + i * 8, fy);
            float hi[8];
            ld_vec<TY>(y + i * 8 + 4, hi);
#pragma unroll
            for (int e = 0; e < 4; ++e) fy[4 + e] = hi[e];
        } else {
            ld_vec<TY>(y + i * 8, fy);
        }
        if constexpr (DROP) {
            const uint32_t keep = mtl_act_keep8(cfg, mtl_act_rowhash(cfg, dr.site, k, row), (uint32_t)(i * 8 - row * p.C));
            const float sk = s * dr.inv_keep;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (keep >> e & 1u) ? fr[e] + sk * fy[e] : fr[e];
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = fr[e] + s * fy[e];
        }
        st_vec<TR, 8>(out + i * 8, o);
    }
}

template <typename TR, typename TY, bool DROP>
__global__ __launch_bounds__(256) void k_residual_bwd(const ResParams p, const ActDrop dr) {
    const int64_t nvec = p.M * p.C / 8;
    DropoutCfg cfg;
    if constexpr (DROP) {
        cfg = dr.cfg;
        mtl_dropout_resolve(cfg);
    }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
        const int64_t row = (i * 8) / p.C;
        const int64_t b = row / p.rows_per_sample;
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        for (int k = 0; k < p.n; ++k) {
            const TR* g = reinterpret_cast<const TR*>(p.y[k]);
            if (!g) continue;
            float fg[8];
            if constexpr (sizeof(TR) == 4) {
                ld_vec<TR>(g + i * 8, fg);
                float hi[8];
                ld_vec<TR>(g + i * 8 + 4, hi);
#pragma unroll
                for (int e = 0; e < 4; ++e) fg[4 + e] = hi[e];
            } else {
                ld_vec<TR>(g + i * 8, fg);
            }
            const float s = p.scale ? p.scale[(int64_t)k * p.B + b] : 1.f;
            float o[8];
            if constexpr (DROP) {
                const uint32_t keep = mtl_act_keep8(cfg, mtl_act_rowhash(cfg, dr.site, k, row), (uint32_t)(i * 8 - row * p.C));
                const float sk = s * dr.inv_keep;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    acc[e] += fg[e];
                    o[e] = (keep >> e & 1u) ? sk * fg[e] : 0.f;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    acc[e] += fg[e];
                    o[e] = s * fg[e];
                }
            }
            if (p.out[k]) st_vec<TY, 8>(reinterpret_cast<TY*>(p.out[k]) + i * 8, o);
        }
        if (p.dres) st_vec<TR, 8>(reinterpret_cast<TR*>(p.dres) + i * 8, acc);
    }
}

int res_check(int n, int64_t M, int64_t C, int64_t B, int rdt, int ydt) {
    if (!mtl_dtype_pair_ok(rdt, ydt)) return MTLORA_ERR_DTYPE;
    if (n < 1 || n > MTLORA_MAX_TASKS + 1 || M < 0 || C <= 0 || C % 8 || B <= 0 || M % B) return MTLORA_ERR_SHAPE;
    return MTLORA_OK;
}

void res_shape(ResParams& p, const float* scale, int n, int64_t M, int64_t C, int64_t B) {
    p.scale = scale;
    p.M = M;
    p.C = (int)C;
    p.n = n;
    p.B = (int)B;
    p.rows_per_sample = M / B;
}

// dr: null = the plain kernels
int res_fwd_launch(const ResParams& p, int res_dtype, int y_dtype, const ActDrop* dr, hipStream_t s) {
    int64_t blocks = mtl_ceil_div(p.M * p.C / 8, 256);
    if (blocks > 2048) blocks = 2048;
    dim3 g((unsigned)blocks, (unsigned)p.n);
    const int er = mtl_elem_size(res_dtype), ey = mtl_elem_size(y_dtype);
    MtlProfScope prof(PK_RESIDUAL, (double)p.n * p.M * p.C * (2 * er + ey), s);
    mtl_dispatch_dtype_pair(res_dtype, y_dtype, [&](auto tr, auto ty) {
        using TR = typename decltype(tr)::type;
        using TY = typename decltype(ty)::type;
        if (dr)
            hipLaunchKernelGGL((k_residual_fwd<TR, TY, true>), g, dim3(256), 0, s, p, *dr);
        else
            hipLaunchKernelGGL((k_residual_fwd<TR, TY, false>), g, dim3(256), 0, s, p, ActDrop{});
    });
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

int res_bwd_launch(const ResParams& p, int res_dtype, int y_dtype, const ActDrop* dr, hipStream_t s) {
    int64_t blocks = mtl_ceil_div(p.M * p.C / 8, 256);
    if (blocks > 2048) blocks = 2048;
    const int er = mtl_elem_size(res_dtype), ey = mtl_elem_size(y_dtype);
    MtlProfScope prof(PK_RESIDUAL, (double)p.M * p.C * (p.n * (er + ey) + (p.dres ? er : 0)), s);
    mtl_dispatch_dtype_pair(res_dtype, y_dtype, [&](auto tr, auto ty) {
        using TR = typename decltype(tr)::type;
        using TY = typename decltype(ty)::type;
        if (dr)
            hipLaunchKernelGGL((k_residual_bwd<TR, TY, true>), dim3((unsigned)blocks), dim3(256), 0, s, p, *dr);
        else
            hipLaunchKernelGGL((k_residual_bwd<TR, TY, false>), dim3((unsigned)blocks), dim3(256), 0, s, p, ActDrop{});
    });
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

// the _drop entries: one condition per step, in the order dtype, n, pointers, alignment, C, M / B, p, row range
int res_drop_check_head(int n, int rdt, int ydt) {
    if (!mtl_dtype_pair_ok(rdt, ydt)) return MTLORA_ERR_DTYPE;
    if (n < 1 || n > MTLORA_MAX_TASKS + 1) return MTLORA_ERR_SHAPE;
    return MTLORA_OK;
}
int res_drop_check_tail(const mtlora_attn_dropout* drop, int site, int64_t M, int64_t C, int64_t B, ActDrop& dr) {
    if (C <= 0 || C % 8 || C > INT32_MAX) return MTLORA_ERR_SHAPE;
    if (M < 0 || B <= 0 || B > INT32_MAX || M % B) return MTLORA_ERR_SHAPE;
    return mtl_act_drop_make(drop, site, M, dr);
}

}  // namespace

extern "C" {

int mtlora_residual_droppath_fwd(int n, const void* const* res, const void* const* y, void* const* out,
                                 const float* scale, int64_t M, int64_t C, int64_t B, int res_dtype, int y_dtype,
                                 void* stream) {
    int st = res_check(n, M, C, B, res_dtype, y_dtype);
    if (st != MTLORA_OK) return st;
    if (mtl_any_null({res, y, out})) return MTLORA_ERR_NULL;
    ResParams p = {};
    for (int k = 0; k < n; ++k) {  // (stream by stream: the first bad stream decides between NULL and ALIGN)
        if (mtl_any_null({res[k], y[k], out[k]})) return MTLORA_ERR_NULL;
        if (mtl_any_misaligned({res[k], y[k], out[k]})) return MTLORA_ERR_ALIGN;
        p.res[k] = res[k];
        p.y[k] = y[k];
        p.out[k] = out[k];
    }
    if (M == 0) return MTLORA_OK;
    res_shape(p, scale, n, M, C, B);
    return res_fwd_launch(p, res_dtype, y_dtype, nullptr, (hipStream_t)stream);
}

/* g[k]: gradient of out_k (res dtype) or NULL; dy[k]: written (y dtype) where non-NULL; dres: sum_k g_k or NULL */
int mtlora_residual_droppath_bwd(int n, const void* const* g, void* const* dy, void* dres, const float* scale,
                                 int64_t M, int64_t C, int64_t B, int res_dtype, int y_dtype, void* stream) {
    int st = res_check(n, M, C, B, res_dtype, y_dtype);
    if (st != MTLORA_OK) return st;
    if (mtl_any_null({g, dy})) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({}, n, {g, mtl_arr(dy)})) return MTLORA_ERR_ALIGN;  // (null elements of g / dy are allowed)
    ResParams p = {};
    for (int k = 0; k < n; ++k) {
        p.y[k] = g[k];
        p.out[k] = g[k] ? dy[k] : nullptr;
    }
    if (M == 0) return MTLORA_OK;
    p.dres = dres;
    res_shape(p, scale, n, M, C, B);
    return res_bwd_launch(p, res_dtype, y_dtype, nullptr, (hipStream_t)stream);
}

/* the same with dropout on the branch; a p below 2^-16 runs the plain kernels */
int mtlora_residual_droppath_drop_fwd(int n, const void* const* res, const void* const* y, void* const* out, const float* scale,
                                      const mtlora_attn_dropout* drop, int site, int64_t M, int64_t C, int64_t B, int res_dtype,
                                      int y_dtype, void* stream) {
    int st = res_drop_check_head(n, res_dtype, y_dtype);
    if (st != MTLORA_OK) return st;
    if (mtl_any_null({res, y, out, drop})) return MTLORA_ERR_NULL;
    ResParams p = {};
    for (int k = 0; k < n; ++k) {
        if (mtl_any_null({res[k], y[k], out[k]})) return MTLORA_ERR_NULL;
        if (mtl_any_misaligned({res[k], y[k], out[k]})) return MTLORA_ERR_ALIGN;
        p.res[k] = res[k];
        p.y[k] = y[k];
        p.out[k] = out[k];
    }
    ActDrop dr = {};
    if ((st = res_drop_check_tail(drop, site, M, C, B, dr)) != MTLORA_OK) return st;
    if (M == 0) return MTLORA_OK;
    res_shape(p, scale, n, M, C, B);
    return res_fwd_launch(p, res_dtype, y_dtype, dr.cfg.enabled() ? &dr : nullptr, (hipStream_t)stream);
}

int mtlora_residual_droppath_drop_bwd(int n, const void* const* g, void* const* dy, void* dres, const float* scale,
                                      const mtlora_attn_dropout* drop, int site, int64_t M, int64_t C, int64_t B, int res_dtype,
                                      int y_dtype, void* stream) {
    int st = res_drop_check_head(n, res_dtype, y_dtype);
    if (st != MTLORA_OK) return st;
    if (mtl_any_null({g, dy, drop})) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({dres}, n, {g, mtl_arr(dy)})) return MTLORA_ERR_ALIGN;  // (null elements of g / dy are allowed)
    ResParams p = {};
    for (int k = 0; k < n; ++k) {
        p.y[k] = g[k];
        p.out[k] = g[k] ? dy[k] : nullptr;
    }
    ActDrop dr = {};
    if ((st = res_drop_check_tail(drop, site, M, C, B, dr)) != MTLORA_OK) return st;
    if (M == 0) return MTLORA_OK;
    p.dres = dres;
    res_shape(p, scale, n, M, C, B);
    return res_bwd_launch(p, res_dtype, y_dtype, dr.cfg.enabled() ? &dr : nullptr, (hipStream_t)stream);
}
}
