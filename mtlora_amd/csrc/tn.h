// tn.h -- the factor-gradient side of MTLoRALinear: k_tn + k_tn_reduce (split-M "TN" reduction, also mtlora_gemm_tn), k_sum (G = sum of
// the output gradients) and k_rank_out (task outputs of a dX launch with small task ranks).  Included by linear.hip after nt.h.
#pragma once

#include "nt.h"

namespace {

// ------------------------------------------------------------------------------------------------
// k_tn : Out[a][b] = sum_m SrcA[m][a0 + a] * SrcB[m][b0 + b], split over m.
// SrcA is always the NARROW (rank-side) operand (Q or P, <= 64 columns per tile) and SrcB the WIDE one
// (X or dY, 256 columns per tile), so a workgroup streams 64 + 256 columns per row and the wide matrix is
// read ~once (x1.25 with the narrow slab) instead of twice with square tiles.  dB = dY^T P is computed as
// its transpose P^T dY and written back transposed by k_tn_reduce.
// ------------------------------------------------------------------------------------------------
constexpr int TN_A = 64;
constexpr int TN_B = 256;
constexpr int TN_TILE = TN_A * TN_B;
struct TnProblem {
    const void* A;
    const void* B;
    int64_t lda, ldb;
    int a0, Na, b0, Nb;  // column windows
    int b_mask;          // dropout keep-mask on SrcB (keyed by (m, b0 + b))
    int tiles_a, tiles_b;
    float* part;         // [nsplit][tiles_a*tiles_b][64*256]
    float* out;          // fp32; element (a, b) at out[a*ldo + b], or out[b*ldo + a] when transpose
    int out_a, out_b, ldo, transpose;
};
struct TnParams {
    TnProblem p[2 * MAXO];
    int n_prob;
    int64_t M;
    int nsplit;
    int64_t rows_per_split;
    DropoutCfg drop;
};

template <typename T>
struct TnCfg;
template <>
struct TnCfg<bf16> {
    static constexpr int SUB = 32;  // rows (m) per MFMA k-tile
};
template <>
struct TnCfg<f16> {
    static constexpr int SUB = 32;
};
template <>
struct TnCfg<float> {
    static constexpr int SUB = 16;
};

// transposed fragment: lane (i = l & 31, h = l >> 5) gets Src[m = slot(h, e)][col0 + i]; ``lr`` = LDS row bytes
template <typename H>  // any 16-bit element type (the transposing read moves bits)
__device__ __forceinline__ Frag<H> tn_frag16(const unsigned char* s, int col0, int lane, int lr) {
    // ds_read_b64_tr_b16: within each 16-lane group, lane i supplies the 8-byte address of row (i>>2),
    // columns 4*(i&3)..+3 of a [4][16] block and receives column i of that block (4 rows).
    const int g = lane >> 4, i = lane & 15, h = g >> 1;
    const int col = col0 + 16 * (g & 1) + 4 * (i & 3);
    Frag<H> f;
    uint32_t w[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // rows: {8h+0..3}, {8h+4..7}, {16+8h+0..3}, {16+8h+4..7}
        const int row = ((j >> 1) * 16) + 8 * h + 4 * (j & 1) + (i >> 2);
        const unsigned char* p = s + row * lr + col * 2;
        s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) s16x4*)(p));
        u32x2 u = __builtin_bit_cast(u32x2, v);
        w[2 * j] = u[0];
        w[2 * j + 1] = u[1];
    }
    f.v[0] = u32x4{w[0], w[1], w[2], w[3]};
    f.v[1] = u32x4{w[4], w[5], w[6], w[7]};
    return f;
}
__device__ __forceinline__ Frag<bf16> tn_frag(const unsigned char* s, int col0, int lane, int lr, bf16*) {
    return tn_frag16<bf16>(s, col0, lane, lr);
}
__device__ __forceinline__ Frag<f16> tn_frag(const unsigned char* s, int col0, int lane, int lr, f16*) {
    return tn_frag16<f16>(s, col0, lane, lr);
}
__device__ __forceinline__ Frag<float> tn_frag(const unsigned char* s, int col0, int lane, int lr, float*) {
    const int h = lane >> 5, i = lane & 31;
    Frag<float> f;
    uint32_t w[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {  // rows {4h..4h+3} U {8+4h..8+4h+3}
        const int row = (e >> 2) * 8 + 4 * h + (e & 3);
        w[e] = *reinterpret_cast<const uint32_t*>(s + row * lr + (col0 + i) * 4);
    }
    f.v[0] = u32x4{w[0], w[1], w[2], w[3]};
    f.v[1] = u32x4{w[4], w[5], w[6], w[7]};
    return f;
}

template <typename T>
__global__ __launch_bounds__(256, 2) void k_tn(const TnParams P) {
    constexpr int SUB = TnCfg<T>::SUB;
    constexpr int KE = 2 * SUB;  // rows per staged chunk
    constexpr int ES = (int)sizeof(T);
    constexpr int VEC = ET<T>::VEC;
    // padded LDS rows.  bf16: a ds_read_b64_tr_b16 cycle serves 32 lanes = 4 rows x 2 column halves of 32 B; the 8
    // segments fall in distinct bank groups iff the row stride is 16 dwords (mod 64): 320 B / 576 B (strides of
    // 144 B / 528 B cost 42 % of the LDS cycles in conflicts).  f32 (scalar 4-byte reads across 32 columns): +16 B.
    constexpr int LRA = ES == 2 ? 320 : TN_A * ES + 16, LRB = ES == 2 ? 576 : TN_B * ES + 16;
    constexpr int VPA = TN_A / VEC, VPB = TN_B / VEC;          // 16-byte vectors per tile row
    constexpr int RSA = 256 / VPA, RSB = 256 / VPB;            // rows covered by one sweep of the workgroup
    constexpr int NLA = KE / RSA, NLB = KE / RSB;              // loads per thread per chunk (2 and 8)
    __shared__ __attribute__((aligned(16))) unsigned char smem[KE * (LRA + LRB)];
    unsigned char* sA = smem;
    unsigned char* sB = smem + KE * LRA;
    const TnProblem& pr = P.p[blockIdx.z];
    const int tile = blockIdx.y;
    if (tile >= pr.tiles_a * pr.tiles_b) return;
    const int ta = tile / pr.tiles_b, tb = tile % pr.tiles_b;
    const int split = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

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

    const int rowA = tid / VPA, vecA = tid % VPA, rowB = tid / VPB, vecB = tid % VPB;
    const int ca = ta * TN_A + vecA * VEC;  // column inside the A window
    const int cb = tb * TN_B + vecB * VEC;
    const bool a_in = ca < pr.Na, b_in = cb < pr.Nb;
    const bool wave_on = tb * TN_B + wave * 64 < pr.Nb;  // this wave's 64 wide columns hold data
    const T* Ap = reinterpret_cast<const T*>(pr.A) + pr.a0 + ca;
    const T* Bp = reinterpret_cast<const T*>(pr.B) + pr.b0 + cb;
    DropoutCfg drop = P.drop;
    mtl_dropout_resolve(drop);
    const bool bmask = pr.b_mask && drop.enabled();

    // two register sets = prefetch distance 2 chunks (the grid is sized to 2 workgroups per CU, i.e. 256 VGPRs per
    // wave, and a workgroup's streaming rate is bounded by bytes in flight / load latency)
    u32x4 ra0[NLA], rb0[NLB], ra1[NLA], rb1[NLB];
    auto load = [&](u32x4* ra, u32x4* rb, int64_t mrow) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NLA; ++j) {
            const int64_t m = mrow + rowA + j * RSA;
            ra[j] = (a_in && m < m_hi) ? *reinterpret_cast<const u32x4*>(Ap + m * pr.lda) : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int j = 0; j < NLB; ++j) {
            const int64_t m = mrow + rowB + j * RSB;
            rb[j] = (b_in && m < m_hi) ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(Bp + m * pr.ldb)) : u32x4{0u, 0u, 0u, 0u};
        }
    };
    auto stage = [&](u32x4* ra, u32x4* rb, int64_t mrow) __attribute__((always_inline)) {
        if (bmask && b_in) {  // dropout keep-mask, applied just before the LDS store
#pragma unroll
            for (int j = 0; j < NLB; ++j) {
                const uint32_t rh = mtl_dropout_rowhash(drop, 0u, (uint32_t)(mrow + rowB + j * RSB));
                Vec16<T> x;
                x.raw = rb[j];
#pragma unroll
                for (int e = 0; e < VEC; e += 2) {
                    const uint32_t h = mtl_dropout_pairbits(drop, rh, (uint32_t)(pr.b0 + cb + e));
                    if ((h & 0xFFFFu) < drop.thr16) x.e[e] = mtl_from_f32<T>(0.f);
                    if ((h >> 16) < drop.thr16) x.e[e + 1] = mtl_from_f32<T>(0.f);
                }
                rb[j] = x.raw;
            }
        }
#pragma unroll
        for (int j = 0; j < NLA; ++j) *reinterpret_cast<u32x4*>(sA + (rowA + j * RSA) * LRA + vecA * 16) = ra[j];
#pragma unroll
        for (int j = 0; j < NLB; ++j) *reinterpret_cast<u32x4*>(sB + (rowB + j * RSB) * LRB + vecB * 16) = rb[j];
    };
    auto compute = [&]() __attribute__((always_inline)) {
        if (!wave_on) return;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const unsigned char* a_s = sA + sub * SUB * LRA;
            const unsigned char* b_s = sB + sub * SUB * LRB;
            Frag<T> fa0 = tn_frag(a_s, 0, lane, LRA, (T*)nullptr);
            Frag<T> fa1 = tn_frag(a_s, 32, lane, LRA, (T*)nullptr);
            Frag<T> fb0 = tn_frag(b_s, wave * 64, lane, LRB, (T*)nullptr);
            Frag<T> fb1 = tn_frag(b_s, wave * 64 + 32, lane, LRB, (T*)nullptr);
            mtl_mma(fa0, fb0, acc[0][0]);
            mtl_mma(fa0, fb1, acc[0][1]);
            mtl_mma(fa1, fb0, acc[1][0]);
            mtl_mma(fa1, fb1, acc[1][1]);
        }
    };

    if (m_lo < m_hi) load(ra0, rb0, m_lo);
    if (m_lo + KE < m_hi) load(ra1, rb1, m_lo + KE);
    for (int64_t mrow = m_lo; mrow < m_hi; mrow += 2 * KE) {
        stage(ra0, rb0, mrow);
        __syncthreads();
        if (mrow + 2 * KE < m_hi) load(ra0, rb0, mrow + 2 * KE);
        compute();
        __syncthreads();
        if (mrow + KE < m_hi) {
            stage(ra1, rb1, mrow + KE);
            __syncthreads();
            if (mrow + 3 * KE < m_hi) load(ra1, rb1, mrow + 3 * KE);
            compute();
            __syncthreads();
        }
    }

    if (!wave_on) return;  // k_tn_reduce never reads columns outside the B window
    float* dst = pr.part + ((int64_t)split * (pr.tiles_a * pr.tiles_b) + tile) * TN_TILE;
#pragma unroll
    for (int ia = 0; ia < 2; ++ia)
#pragma unroll
        for (int jb = 0; jb < 2; ++jb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = ia * 32 + mtl_d_row(lane, r), j = wave * 64 + jb * 32 + mtl_d_col(lane);
                dst[i * TN_B + j] = acc[ia][jb][r];
            }
}

constexpr int TN_RG = 4;  // thread groups that share the splits of a 1024-element block
template <int TA = TN_A, int TB = TN_B>  // the partial tiles' shape: k_tn's 64 x 256, or the 128 x 128 of k_wgrad (weight_grad.hip)
__global__ __launch_bounds__(256 * TN_RG) void k_tn_reduce(const TnParams P) {
    // one workgroup per (problem, tile, 1024-element block): 4 outputs per thread (one 16-byte load per split, coalesced
    // across the wave); the splits are dealt round-robin to TN_RG groups of 256 threads, each summing its share in a
    // fixed order with 4 independent chains, then a fixed-order LDS combine (deterministic)
    __shared__ f32x4 sm[TN_RG][256];
    const TnProblem& pr = P.p[blockIdx.z];
    const int ntile = pr.tiles_a * pr.tiles_b;
    const int tile = blockIdx.y;
    if (tile >= ntile) return;
    const int t = threadIdx.x & 255, grp = threadIdx.x >> 8;
    const int e0 = blockIdx.x * 1024 + t * 4;  // element inside the TA x TB tile
    const int ta = tile / pr.tiles_b, tb = tile % pr.tiles_b;
    const int a = ta * TA + e0 / TB, b0 = tb * TB + e0 % TB;
    const bool live = a < pr.out_a && b0 < pr.out_b;
    f32x4 acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (live) {
        const float* src = pr.part + (int64_t)tile * (TA * TB) + e0;
        const int64_t stride = (int64_t)ntile * (TA * TB);
        int sp = grp;
        for (; sp + 3 * TN_RG < P.nsplit; sp += 4 * TN_RG) {
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] += *reinterpret_cast<const f32x4*>(src + (int64_t)(sp + u * TN_RG) * stride);
        }
        for (; sp < P.nsplit; sp += TN_RG) acc[0] += *reinterpret_cast<const f32x4*>(src + (int64_t)sp * stride);
    }
    sm[grp][t] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    __syncthreads();
    if (grp != 0 || !live) return;
    f32x4 tsum = sm[0][t];
#pragma unroll
    for (int gI = 1; gI < TN_RG; ++gI) tsum += sm[gI][t];
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (b0 + e < pr.out_b) {
            const int64_t at = pr.transpose ? (int64_t)(b0 + e) * pr.ldo + a : (int64_t)a * pr.ldo + b0 + e;
            pr.out[at] = tsum[e];
        }
}

// elementwise sum of up to MAXO tensors (matrixv2 backward: G for the shared factors)
struct SumParams {
    const void* src[MAXO];
    int n;
    int64_t nvec;
};
template <typename T>
__global__ __launch_bounds__(256) void k_sum(SumParams P, T* out) {
    constexpr int VEC = ET<T>::VEC;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < P.nvec; i += (int64_t)gridDim.x * 256) {
        float f[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) f[e] = 0.f;
        for (int s = 0; s < P.n; ++s) {
            Vec16<T> y = mtl_ld16<T>(reinterpret_cast<const T*>(P.src[s]) + i * VEC);
#pragma unroll
            for (int e = 0; e < VEC; ++e) f[e] += mtl_to_f32(y.e[e]);
        }
        Vec16<T> o;
#pragma unroll
        for (int e = 0; e < VEC; ++e) o.e[e] = mtl_from_f32<T>(f[e]);
        *reinterpret_cast<u32x4*>(out + i * VEC) = o.raw;
    }
}

// ------------------------------------------------------------------------------------------------
// k_scale_grad : d(loss)/d(scale_o) = <dB_o, B_o> / scale_o for the 1 + T segments of a layer whose scales are trainable 1-element
// Parameters (TRAINABLE_SCALE_*): y_o carries scale_o B_o (..), so dB_o = scale_o Z_o and d scale_o = <Z_o, B_o>.  dB_o (the fp32
// factor gradient the backward has just written) and B_o (the fp32 master) are (N x r_o) contiguous; the scale is read from the
// device.  Two steps in stream order, no atomics: blockIdx.y = segment, each of the SG_BLOCKS workgroups of a segment leaves one
// fp32 partial (a thread walks its elements in ascending order, the workgroup sums in a fixed order), then k_scale_grad_fin adds a
// segment's partials in ascending order in double and divides.  Same bits on every run.  Largest layer of the model family:
// N x r_s = 3072 x 128 elements (Swin-B stage-3 fc1) = 48 elements per thread.
// ------------------------------------------------------------------------------------------------
constexpr int SG_BLOCKS = 32;
struct ScaleGradParams {
    const float* dB[MAXO];     // null: segment skipped (its d_scale word is not written)
    const float* B[MAXO];
    const float* scale[MAXO];  // null: segment skipped
    int64_t n[MAXO];           // N * r_o
    float* part;               // MAXO x SG_BLOCKS
    float* d_scale;            // 1 + T
    int nseg;
};
__global__ __launch_bounds__(256) void k_scale_grad_part(ScaleGradParams P) {
    __shared__ float red[4];
    const int o = blockIdx.y;
    if (!P.dB[o] || !P.scale[o]) return;  // (uniform over the workgroup)
    const float* __restrict__ g = P.dB[o];
    const float* __restrict__ b = P.B[o];
    const int64_t n = P.n[o], step = (int64_t)SG_BLOCKS * 256;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + 3 * step < n; i += 4 * step) {  // four independent pairs of loads in flight
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] += g[i + u * step] * b[i + u * step];
    }
    for (; i < n; i += step) acc[0] += g[i] * b[i];
    float s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) s += __shfl_xor(s, w);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) P.part[o * SG_BLOCKS + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(64) void k_scale_grad_fin(ScaleGradParams P) {
    const int o = threadIdx.x;
    if (o >= P.nseg || !P.dB[o] || !P.scale[o]) return;
    double t = 0.0;
    for (int k = 0; k < SG_BLOCKS; ++k) t += (double)P.part[o * SG_BLOCKS + k];
    const float s = *P.scale[o];
    P.d_scale[o] = s == 0.f ? 0.f : (float)(t / (double)s);
}

// ------------------------------------------------------------------------------------------------
// k_rank_out : the task outputs of a dX launch,  dX_t = Q_t A_t  [.* gelu'(h_t)],  for SMALL task ranks (rp <= 16).
// They share nothing with the base GEMM (no dY W term), and with r_t = 4 the "GEMM" is 8 multiply-adds per element: in the tiled
// multi-output kernel each of them costs a full tile pass (rank k-tile staging, MFMA on a mostly-zero k-tile, LDS transposition) --
// the T = 4 fc2 dX spent ~180 us per task output at stage 0.  Here it is a streaming elementwise kernel: a thread owns ONE 16-byte
// column chunk (its rp x 8 factor values live in registers) and walks the rows, 4 in flight; rounding as the tiled epilogue
// (fp32 sum -> T, then T * gelu'(h) -> T).
// ------------------------------------------------------------------------------------------------
struct RankOutParams {
    const void* Q;      // (M x ldq)
    const void* Acat;   // (R x K) row-major, unscaled (Q carries alpha)
    int64_t ldq, M;
    int K, n_t;
    int seg[MAXO], rp[MAXO];
    void* out[MAXO];
    const void* gate[MAXO];
};
template <typename T, bool GATE, int RP>
__global__ __launch_bounds__(256) void k_rank_out(const RankOutParams P) {
    constexpr int UNR = 4;
    const int t = blockIdx.y;
    const int nchunk = P.K >> 3;
    const int rpb = 256 / nchunk;  // rows per block sweep (nchunk <= 256)
    const int tid = threadIdx.x;
    if (tid >= rpb * nchunk) return;
    const int chunk = tid % nchunk, r0 = tid / nchunk;
    const int seg = P.seg[t];
    float a[RP][8];
#pragma unroll
    for (int j = 0; j < RP; ++j) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(P.Acat) + (int64_t)(seg + j) * P.K + chunk * 8);
        VOps<T>::unpack(v, a[j]);
    }
    const T* q = reinterpret_cast<const T*>(P.Q) + seg;
    T* out = reinterpret_cast<T*>(P.out[t]);
    const T* gate = reinterpret_cast<const T*>(P.gate[t]);
    const int64_t step = (int64_t)gridDim.x * rpb;
    for (int64_t row = (int64_t)blockIdx.x * rpb + r0; row < P.M; row += UNR * step) {
        u32x4 qv[UNR][RP / 8], hv[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int64_t m = row + u * step;
            const int64_t mc = m < P.M ? m : P.M - 1;
#pragma unroll
            for (int w = 0; w < RP / 8; ++w) qv[u][w] = *reinterpret_cast<const u32x4*>(q + mc * P.ldq + w * 8);
            if constexpr (GATE) hv[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(gate + mc * P.K + chunk * 8));
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int64_t m = row + u * step;
            float acc[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
            for (int w = 0; w < RP / 8; ++w) {
                float qf[8];
                VOps<T>::unpack(qv[u][w], qf);
#pragma unroll
                for (int j = 0; j < 8; ++j)
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[e] += qf[j] * a[w * 8 + j][e];
            }
            u32x4 o = VOps<T>::pack(acc);
            if constexpr (GATE) o = mtl_gelu_gate_pk4<T, false>(o, hv[u]);
            if (m < P.M) __builtin_nontemporal_store(o, reinterpret_cast<u32x4*>(out + m * P.K + chunk * 8));
        }
    }
}

}  // namespace
