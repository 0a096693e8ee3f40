// act_dropout.hip -- drop(act(h)) over the n = 1+T tensors of a call, one launch per direction (swin_transformer_mtlora.py:172-174:
// the Mlp's hidden tensors, act = exact GELU; :739 pos_drop, act = identity):
//   forward : a_k  = keep_k . act(h_k) / (1 - p)
//   backward: dh_k = g_k . keep_k / (1 - p) . act'(h_k)          (reads g and h, regenerates keep_k: act_dropout.h)
// instead of a GELU pass, a dropout pass and a stored bool mask per tensor and direction.  Streaming kernels: a lane owns 8 consecutive
// channels of one row per step (16 bytes of a 16-bit tensor, two 16-byte vectors of an fp32 one), products in fp32, rounded once.
// GELU as the linear kernels' epilogues form it (16-bit: mtl_erf2n; fp32: gelu_fwd / gelu_grad of common.h), so gelu(h) here is what
// fc1's gelu_out epilogue writes.
#include "act_dropout.h"
#include "dispatch.h"
#include "vec.h"

namespace {

struct ActParams {
    const void* h[MTLORA_MAX_TASKS + 1];  // pre-activation (not read by the backward of act = identity)
    const void* g[MTLORA_MAX_TASKS + 1];  // backward: gradient of a_k
    void* out[MTLORA_MAX_TASKS + 1];      // forward: a_k ; backward: dh_k
    int64_t M;
    int C;
    ActDrop drop;
};

// gelu (GRAD = false) or gelu' (GRAD = true) of 8 values, unrounded
template <typename T, bool GRAD>
__device__ __forceinline__ void act_gelu8(const float (&h)[8], float (&o)[8]) {
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = GRAD ? gelu_grad(h[e]) : gelu_fwd(h[e]);
    } else {
#pragma unroll
        for (int q2 = 0; q2 < 4; q2 += 2) {  // (two pairs in flight, as mtl_gelu_pk4)
            f32x2 hh[2], er[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) hh[q] = f32x2{h[2 * (q2 + q)], h[2 * (q2 + q) + 1]};
            mtl_erf2n<2>(hh, er);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                f32x2 r;
                if constexpr (GRAD) {
                    const f32x2 cdf = 0.5f + 0.5f * er[q];
                    const f32x2 qq = hh[q] * hh[q];
                    const f32x2 ex = {__builtin_amdgcn_exp2f(qq.x * -0.72134752044448170f), __builtin_amdgcn_exp2f(qq.y * -0.72134752044448170f)};
                    r = cdf + hh[q] * ex * 0.39894228040143268f;
                } else {
                    r = hh[q] * (0.5f + 0.5f * er[q]);
                }
                o[2 * (q2 + q)] = r.x;
                o[2 * (q2 + q) + 1] = r.y;
            }
        }
    }
}

// grid (blocks, n): blockIdx.y = tensor.  The (row, vector-of-the-row) pair of a lane advances by the grid stride without a division
template <typename T, int ACT, bool BWD>
__global__ __launch_bounds__(256) void k_act_dropout(const ActParams p) {
    const int k = blockIdx.y;
    DropoutCfg cfg = p.drop.cfg;
    mtl_dropout_resolve(cfg);
    const float inv = p.drop.inv_keep;
    const T* h = reinterpret_cast<const T*>(p.h[k]);
    const T* g = reinterpret_cast<const T*>(p.g[k]);
    T* out = reinterpret_cast<T*>(p.out[k]);
    const int64_t V = p.C / 8, nvec = p.M * V;
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t drow = stride / V, dcol = stride % V;
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t row = i / V, col = i % V;
    for (; i < nvec; i += stride) {
        uint32_t keep = 0xFFu;
        if (cfg.enabled()) keep = mtl_act_keep8(cfg, mtl_act_rowhash(cfg, p.drop.site, k, row), (uint32_t)col * 8u);
        float o[8];
        if constexpr (ACT != 0 || !BWD) {
            float fh[8];
            ld_n<T, 8>(h + i * 8, fh);
            if constexpr (ACT != 0) {
                act_gelu8<T, BWD>(fh, o);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = fh[e];
            }
        }
        if constexpr (BWD) {
            float fg[8];
            ld_n<T, 8>(g + i * 8, fg);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = ACT != 0 ? fg[e] * inv * o[e] : fg[e] * inv;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] *= inv;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (keep >> e & 1u) ? o[e] : 0.f;
        st_vec<T, 8>(out + i * 8, o);
        row += drow;
        col += dcol;
        if (col >= V) {
            col -= V;
            ++row;
        }
    }
}

// checks in the order of the glue entries: dtype, n / act, pointers, alignment, shape, dropout argument.  MTLORA_OK with run = false:
// nothing to launch
int act_setup(int n, const void* const* h, const void* const* g, void* const* out, bool need_h, bool need_g,
              const mtlora_attn_dropout* drop, int site, int act, int64_t M, int64_t C, int dtype, ActParams& p, bool& run) {
    run = false;
    if (!mtl_dtype_in(dtype, MTL_DT_ALL)) return MTLORA_ERR_DTYPE;
    if (n < 1 || n > MTLORA_MAX_TASKS + 1 || (act != 0 && act != 1)) return MTLORA_ERR_SHAPE;
    if (!drop || !out || (need_h && !h) || (need_g && !g)) return MTLORA_ERR_NULL;
    for (int k = 0; k < n; ++k) {  // (tensor by tensor: the first bad tensor decides between NULL and ALIGN)
        const void* hk = need_h ? h[k] : nullptr;
        const void* gk = need_g ? g[k] : nullptr;
        if (!out[k] || (need_h && !hk) || (need_g && !gk)) return MTLORA_ERR_NULL;
        if (mtl_any_misaligned({hk, gk, out[k]})) return MTLORA_ERR_ALIGN;
        p.h[k] = hk;
        p.g[k] = gk;
        p.out[k] = out[k];
    }
    if (M < 0 || C <= 0 || C % 8 || C > INT32_MAX) return MTLORA_ERR_SHAPE;
    const int st = mtl_act_drop_make(drop, site, M, p.drop);
    if (st != MTLORA_OK) return st;
    p.M = M;
    p.C = (int)C;
    run = M > 0;
    return MTLORA_OK;
}

template <bool BWD>
int act_launch(int n, int act, int dtype, const ActParams& p, hipStream_t s) {
    int64_t blocks = mtl_ceil_div(p.M * (p.C / 8), 256);
    if (blocks > 2048) blocks = 2048;
    const dim3 grid((unsigned)blocks, (unsigned)n);
    const int tensors = BWD ? (act ? 3 : 2) : 2;
    MtlProfScope prof(PK_ACT_DROP, (double)n * p.M * p.C * tensors * mtl_elem_size(dtype), s);
    mtl_dispatch_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        if (act)
            hipLaunchKernelGGL((k_act_dropout<T, 1, BWD>), grid, dim3(256), 0, s, p);
        else
            hipLaunchKernelGGL((k_act_dropout<T, 0, BWD>), grid, dim3(256), 0, s, p);
    });
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

}  // namespace

extern "C" {

int mtlora_act_dropout_fwd(int n, const void* const* h, void* const* a, const mtlora_attn_dropout* drop, int site, int act,
                           int64_t M, int64_t C, int dtype, void* stream) {
    ActParams p = {};
    bool run;
    const int st = act_setup(n, h, nullptr, a, true, false, drop, site, act, M, C, dtype, p, run);
    if (st != MTLORA_OK || !run) return st;
    return act_launch<false>(n, act, dtype, p, (hipStream_t)stream);
}

/* h is not read (and may be NULL) when act == 0 */
int mtlora_act_dropout_bwd(int n, const void* const* g, const void* const* h, void* const* dh, const mtlora_attn_dropout* drop,
                           int site, int act, int64_t M, int64_t C, int dtype, void* stream) {
    ActParams p = {};
    bool run;
    const int st = act_setup(n, h, g, dh, act == 1, true, drop, site, act, M, C, dtype, p, run);
    if (st != MTLORA_OK || !run) return st;
    return act_launch<true>(n, act, dtype, p, (hipStream_t)stream);
}
}
