// weight_grad.hip -- full fine-tuning of MTLoRALinear (MODEL.MTLORA.FREEZE_PRETRAINED False, reference config.py:317, main.py:254-262:
// mark_only_lora_as_trainable is not called, so every `linear.weight` trains next to the LoRA factors).
//
//   mtlora_linear_weight_grad   dW[n][k] = sum_m (dy_s[m][n] + sum_t dy_t[t][m][n]) x[m][k]     k_wgrad (+ k_tn_reduce when split over M)
//   mtlora_linear_weight_cast   Wc = T(W), Wt = T(W)^T from the fp32 master, one launch          k_wcast
//
// k_wgrad is a split-M "TN" GEMM as k_tn of tn.h (same transposed LDS fragment readers, same MFMA wrappers, same fixed-order
// reduce), with a SQUARE 128 x 128 output tile instead of k_tn's 64 x 256 window: dW is (N x K) with both sides in the hundreds
// to thousands, where a 64-column window would re-read dy K / 64 times.  The 1 + T sources are walked as an extension of the
// reduction dimension (dW = sum_o dy_o^T x): step (chunk, o) stages rows [chunk] of dy_o and of x, so no (M, N) sum exists and
// every product is accumulated exactly as issued (fp32 MFMA accumulators, no rounding of a summed gradient).
#include "dispatch.h"
#include "tn.h"

namespace {

constexpr int WG_T = 128;               // tile edge: WG_T output features (columns of dy) x WG_T input features (columns of x)
constexpr int WG_TILE = WG_T * WG_T;
constexpr int WG_MAXSRC = 1 + MTLORA_MAX_TASKS;
constexpr int WG_TARGET_BLOCKS = 512;   // 2 workgroups per CU (launch bounds) x 256 CUs
constexpr int WG_MIN_ROWS = 512;        // a split walks at least this many rows: a 64 KB partial tile per >= 256 KB of bf16 operands read
constexpr int WG_ROW_UNIT = 64;         // splits start on multiples of the largest staged chunk

struct WgParams {
    const void* src[WG_MAXSRC];  // the non-null output gradients, (M x N)
    const void* x;               // (M x K)
    int nsrc, N, K, tiles_k;
    int64_t M, rows_per_split;
    int nsplit;
    float* part;  // [nsplit][tiles][WG_T * WG_T]  (nsplit > 1)
    float* out;   // (N x K) fp32                  (nsplit == 1: written by k_wgrad itself)
};

template <typename T>
__global__ __launch_bounds__(256, 2) void k_wgrad(const WgParams P) {
    constexpr int SUB = TnCfg<T>::SUB;  // rows (m) per MFMA k-tile
    constexpr int KE = 2 * SUB;         // rows per staged chunk
    constexpr int ES = (int)sizeof(T);
    constexpr int VEC = ET<T>::VEC;
    // padded LDS rows, as k_tn: 16-bit rows at 16 dwords (mod 64) for the transposing read, fp32 rows + 16 B
    constexpr int LR = ES == 2 ? 320 : WG_T * ES + 16;
    constexpr int VP = WG_T / VEC;  // 16-byte vectors per tile row
    constexpr int RS = 256 / VP;    // rows covered by one sweep of the workgroup
    constexpr int NL = KE / RS;     // loads per thread, operand and chunk (4)
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * KE * LR];
    unsigned char* sA = smem;
    unsigned char* sB = smem + KE * LR;
    const int tile = blockIdx.y, split = blockIdx.x;
    const int tn = tile / P.tiles_k, tk = tile % P.tiles_k;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wa = wave >> 1, wb = wave & 1;  // the wave's 64 x 64 quadrant of the tile

    const int64_t m_lo = (int64_t)split * P.rows_per_split;
    int64_t m_hi = m_lo + P.rows_per_split;
    if (m_hi > P.M) m_hi = P.M;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int row = tid / VP, vec = tid % VP;
    const int ca = tn * WG_T + vec * VEC, cb = tk * WG_T + vec * VEC;
    const bool a_in = ca < P.N, b_in = cb < P.K;  // (N and K are multiples of VEC: a vector is inside or outside as a whole)
    const bool wave_on = tn * WG_T + wa * 64 < P.N && tk * WG_T + wb * 64 < P.K;
    const T* Xp = reinterpret_cast<const T*>(P.x) + cb;

    // the walk: step s = (chunk, source), sources innermost, so the x rows of a chunk are re-read while they are hot
    const int64_t nchunk = m_hi > m_lo ? (m_hi - m_lo + KE - 1) / KE : 0;
    const int64_t nstep = nchunk * P.nsrc;
    int64_t ld_m = m_lo;  // (loader state: the step the NEXT load() fetches)
    int ld_o = 0;

    u32x4 ra0[NL], rb0[NL], ra1[NL], rb1[NL];  // two register sets = prefetch distance 2 steps, as k_tn
    auto load = [&](u32x4* ra, u32x4* rb) __attribute__((always_inline)) {
        const T* Ap = reinterpret_cast<const T*>(P.src[ld_o]) + ca;
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            const int64_t m = ld_m + row + j * RS;
            ra[j] = (a_in && m < m_hi) ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(Ap + m * P.N)) : u32x4{0u, 0u, 0u, 0u};
            rb[j] = (b_in && m < m_hi) ? *reinterpret_cast<const u32x4*>(Xp + m * P.K) : u32x4{0u, 0u, 0u, 0u};
        }
        if (++ld_o == P.nsrc) {
            ld_o = 0;
            ld_m += KE;
        }
    };
    auto stage = [&](u32x4* ra, u32x4* rb) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            *reinterpret_cast<u32x4*>(sA + (row + j * RS) * LR + vec * 16) = ra[j];
            *reinterpret_cast<u32x4*>(sB + (row + j * RS) * LR + vec * 16) = rb[j];
        }
    };
    auto compute = [&]() __attribute__((always_inline)) {
        if (!wave_on) return;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const unsigned char* a_s = sA + sub * SUB * LR;
            const unsigned char* b_s = sB + sub * SUB * LR;
            Frag<T> fa0 = tn_frag(a_s, wa * 64, lane, LR, (T*)nullptr);
            Frag<T> fa1 = tn_frag(a_s, wa * 64 + 32, lane, LR, (T*)nullptr);
            Frag<T> fb0 = tn_frag(b_s, wb * 64, lane, LR, (T*)nullptr);
            Frag<T> fb1 = tn_frag(b_s, wb * 64 + 32, lane, LR, (T*)nullptr);
            mtl_mma(fa0, fb0, acc[0][0]);
            mtl_mma(fa0, fb1, acc[0][1]);
            mtl_mma(fa1, fb0, acc[1][0]);
            mtl_mma(fa1, fb1, acc[1][1]);
        }
    };

    if (nstep > 0) load(ra0, rb0);
    if (nstep > 1) load(ra1, rb1);
    for (int64_t s = 0; s < nstep; s += 2) {
        stage(ra0, rb0);
        __syncthreads();
        if (s + 2 < nstep) load(ra0, rb0);
        compute();
        __syncthreads();
        if (s + 1 < nstep) {
            stage(ra1, rb1);
            __syncthreads();
            if (s + 3 < nstep) load(ra1, rb1);
            compute();
            __syncthreads();
        }
    }

    if (!wave_on) return;  // (neither the reduce nor the direct store touches a quadrant outside N x K)
    if (P.nsplit == 1) {   // no split: the tile is final
#pragma unroll
        for (int ia = 0; ia < 2; ++ia)
#pragma unroll
            for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int n = tn * WG_T + wa * 64 + ia * 32 + mtl_d_row(lane, r), k = tk * WG_T + wb * 64 + jb * 32 + mtl_d_col(lane);
                    if (n < P.N && k < P.K) P.out[(int64_t)n * P.K + k] = acc[ia][jb][r];
                }
        return;
    }
    float* dst = P.part + ((int64_t)split * gridDim.y + tile) * WG_TILE;
#pragma unroll
    for (int ia = 0; ia < 2; ++ia)
#pragma unroll
        for (int jb = 0; jb < 2; ++jb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = wa * 64 + ia * 32 + mtl_d_row(lane, r), j = wb * 64 + jb * 32 + mtl_d_col(lane);
                dst[i * WG_T + j] = acc[ia][jb][r];
            }
}

// ------------------------------------------------------------------------------------------------
// k_wcast : the compute-dtype copies of a trainable fp32 master, Wc[n][k] = T(W[n][k]) and Wt[k][n] = T(W[n][k]), from ONE read
// of W: a 64 x 64 tile is converted (round to nearest even, the conversion of W.to(dtype)), stored row-major and transposed through
// LDS (odd dword row stride: the column reads of the transposed store are conflict-free), as the packing kernels of nt.h do.
// ------------------------------------------------------------------------------------------------
constexpr int WC_T = 64;
template <typename T>
__global__ __launch_bounds__(256) void k_wcast(const float* __restrict__ W, int N, int K, T* __restrict__ Wc, T* __restrict__ Wt) {
    constexpr int LD = sizeof(T) == 2 ? WC_T + 2 : WC_T + 1;
    __shared__ T sm[WC_T][LD];
    const int n0 = blockIdx.y * WC_T, k0 = blockIdx.x * WC_T;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < WC_T; r += 4) {
        const int n = n0 + r, k = k0 + tx;
        if (n < N && k < K) {
            const T v = mtl_from_f32<T>(W[(int64_t)n * K + k]);
            Wc[(int64_t)n * K + k] = v;
            sm[r][tx] = v;
        }
    }
    __syncthreads();
    for (int r = ty; r < WC_T; r += 4) {
        const int k = k0 + r, n = n0 + tx;
        if (n < N && k < K) Wt[(int64_t)k * N + n] = sm[tx][r];
    }
}

// ---- host side ----------------------------------------------------------------------------------
struct WgPlan {
    int tiles_n, tiles_k, nsplit;
    int64_t rows_per_split;
};

bool wg_shape_ok(const mtlora_linear_desc* d) {
    if (!mtl_dtype_in(d->dtype, MTL_DT_ALL) || d->T < 0 || d->T > MTLORA_MAX_TASKS) return false;
    const int ve = mtl_vec_elems(d->dtype);
    if (d->M < 0 || d->M > ((int64_t)1 << 40) || d->N <= 0 || d->K <= 0 || d->N > (1 << 20) || d->K > (1 << 20)) return false;
    if (d->N % ve || d->K % ve) return false;
    return mtl_ceil_div(d->N, WG_T) * mtl_ceil_div(d->K, WG_T) <= 65535;  // (the tile index is a grid y coordinate)
}

// split rule: enough workgroups to fill the chip twice over (2 per CU), but never a split shorter than WG_MIN_ROWS rows; splits
// start on multiples of the staged chunk.  The stage-3 shapes (hundreds of tiles, M of a few thousand) get 1 to 3 splits, the
// stage-0 shapes (1 to 4 tiles, M of 4 x 10^5) some hundreds.
WgPlan wg_plan(const mtlora_linear_desc* d) {
    WgPlan p;
    p.tiles_n = (int)mtl_ceil_div(d->N, WG_T);
    p.tiles_k = (int)mtl_ceil_div(d->K, WG_T);
    const int64_t tiles = (int64_t)p.tiles_n * p.tiles_k;
    int64_t ns = WG_TARGET_BLOCKS / tiles, cap = d->M / WG_MIN_ROWS;
    if (ns > cap) ns = cap;
    if (ns < 1) ns = 1;
    p.rows_per_split = mtl_round_up(mtl_ceil_div(d->M > 0 ? d->M : 1, ns), WG_ROW_UNIT);
    p.nsplit = (int)mtl_ceil_div(d->M > 0 ? d->M : 1, p.rows_per_split);
    return p;
}

}  // namespace

extern "C" {

int64_t mtlora_linear_weight_grad_scratch_bytes(const mtlora_linear_desc* d) {
    if (!d || !wg_shape_ok(d)) return -1;
    const WgPlan p = wg_plan(d);
    return (p.nsplit > 1 ? (int64_t)p.nsplit * p.tiles_n * p.tiles_k * WG_TILE * 4 : 0) + 256;
}

int mtlora_linear_weight_grad(const mtlora_linear_desc* d, const void* x, const void* dy_s, const void* const* dy_t, float* dW,
                              void* scratch, int64_t scratch_bytes, void* stream) {
    if (!d) return MTLORA_ERR_NULL;
    if (!mtl_dtype_in(d->dtype, MTL_DT_ALL)) return MTLORA_ERR_DTYPE;
    if (!wg_shape_ok(d)) return MTLORA_ERR_SHAPE;
    if (mtl_any_null({x, dW, scratch}) || (d->T > 0 && !dy_t)) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({x, dy_s, dW, scratch}, d->T, {dy_t})) return MTLORA_ERR_ALIGN;
    if (scratch_bytes < mtlora_linear_weight_grad_scratch_bytes(d)) return MTLORA_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const WgPlan pl = wg_plan(d);
    WgParams P = {};
    if (dy_s) P.src[P.nsrc++] = dy_s;  // an output that got no gradient (NULL) is skipped
    for (int t = 0; t < d->T; ++t)
        if (dy_t[t]) P.src[P.nsrc++] = dy_t[t];
    if (P.nsrc == 0 || d->M == 0) {  // nothing to sum: zeros, written by a kernel (no memset node)
        mtl_zero_async(dW, (size_t)d->N * (size_t)d->K * 4, s);
        MTL_CHECK_LAUNCH();
        return MTLORA_OK;
    }
    P.x = x;
    P.N = (int)d->N;
    P.K = (int)d->K;
    P.tiles_k = pl.tiles_k;
    P.M = d->M;
    P.rows_per_split = pl.rows_per_split;
    P.nsplit = pl.nsplit;
    P.part = reinterpret_cast<float*>(scratch);
    P.out = dW;
    const int tiles = pl.tiles_n * pl.tiles_k;
    mtl_dispatch_dtype(d->dtype, [&](auto t) {
        hipLaunchKernelGGL(k_wgrad<typename decltype(t)::type>, dim3((unsigned)pl.nsplit, (unsigned)tiles), dim3(256), 0, s, P);
    });
    if (pl.nsplit > 1) {  // the fixed-order combine of the factor gradients, over 128 x 128 tiles
        TnParams tp = {};
        tp.n_prob = 1;
        tp.nsplit = pl.nsplit;
        TnProblem& pr = tp.p[0];
        pr.tiles_a = pl.tiles_n;
        pr.tiles_b = pl.tiles_k;
        pr.part = P.part;
        pr.out = dW;
        pr.out_a = P.N;
        pr.out_b = P.K;
        pr.ldo = P.K;
        pr.transpose = 0;
        hipLaunchKernelGGL((k_tn_reduce<WG_T, WG_T>), dim3(WG_TILE / 1024, (unsigned)tiles, 1), dim3(256 * TN_RG), 0, s, tp);
    }
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

int mtlora_linear_weight_cast(const float* W, int N, int K, int dtype, void* Wc, void* Wt, void* stream) {
    if (!mtl_dtype_in(dtype, MTL_DT_ALL)) return MTLORA_ERR_DTYPE;
    if (N <= 0 || K <= 0 || mtl_ceil_div(N, WC_T) > 65535) return MTLORA_ERR_SHAPE;
    if (mtl_any_null({W, Wc, Wt})) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({W}, 0, {}, 4) || mtl_any_misaligned({Wc, Wt}, 0, {}, (uintptr_t)mtl_elem_size(dtype))) return MTLORA_ERR_ALIGN;
    mtl_dispatch_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(k_wcast<T>, dim3((unsigned)mtl_ceil_div(K, WC_T), (unsigned)mtl_ceil_div(N, WC_T)), dim3(256), 0,
                           (hipStream_t)stream, W, N, K, reinterpret_cast<T*>(Wc), reinterpret_cast<T*>(Wt));
    });
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

}  // extern "C"
