// patch_merge.hip -- PatchMerging (reference swin_transformer_mtlora.py:429-481: 2x2 neighbourhood concat -> LayerNorm(4C) -> bias-free
// Linear(4C -> 2C)) of n independent token streams, without the normalised (rows, 4C) matrix or its gradient ever reaching memory:
//
//   mtlora_patch_merge_fwd   y[m, :] = round(LN(row(m)) gamma + beta) W^T          k_pm_fwd, one launch
//   mtlora_patch_merge_bwd   dx (scattered to the tokens), dW, dgamma, dbeta        k_pm_dx, k_pm_dw, k_pm_finish
//
// Merged row m = (stream, b, i, j); its K = 4C values are the C-vectors x(2i, 2j), x(2i+1, 2j), x(2i, 2j+1), x(2i+1, 2j+1) of the
// stream's (B, H W, C) tensor: column k lies in segment q = k / C at token (2i + (q & 1), 2j + (q >> 1)).  N = 2C.  Workgroups are four
// waves; every grid is persistent over row blocks (k_pm_fwd, k_pm_dx) or owns one output tile and one row split (k_pm_dw).
//
//   forward   a workgroup owns R = 32 RT merged rows (RT = 4 / 2 / 1 for K <= 384 / 768 / 2048).  A wave takes rows wave, wave + 4, ...:
//             16-byte loads straight from the four token positions, the row (up to 32 values a lane) in registers, mean and rstd in
//             fp32 in two passes over the registers, z = fma((x - mean) rstd, gamma, beta) rounded to the compute dtype into the LDS
//             operand panel (R rows, pitch 2K + 16 bytes).  Then Y^T = W Z^T: the output columns go by in chunks of 256 (64 a wave:
//             RT x 2 accumulator tiles), W (the fp32 master) streams through a two-slot LDS ring in k-slabs of 32 (16 at RT = 1), cast
//             on the way in; the loads of slab s + 1 are in flight while slab s feeds the MFMAs, one barrier a slab.  A lane holds
//             columns 8g + 4hh + 0..3 of ITS row: the lane halves swap 8-byte pieces and write whole 16-byte runs.
//   dx        g = dY W per row block of R rows (RT = 2 / 1 for K <= 768 / 2048 here), never stored: pass A forms g chunk by chunk (256 of the K columns at a time, dY
//             straight from memory as the MFMA operand, W^T through the ring: pairs of W rows packed into dwords, so that a lane's
//             eight reduction values are contiguous) in the orientation lane = column, and leaves the row sums of g gamma and
//             g gamma xhat (in-lane over the chunks, one butterfly, the waves added in wave order through LDS) and the column sums
//             dgamma += g xhat, dbeta += g (each column owned by ONE lane, accumulated in LDS over the row blocks).  Pass B forms g
//             again in the orientation lane = row and writes dx = rstd (g gamma - s1 - xhat s2) as 16-byte (fp32) or 8-byte runs.
//   dW        dW = dY^T Z, split over rows: a workgroup owns a 128 x 256 tile of dW and one row split; per 32 rows it rebuilds z
//             (same expression as the forward) and writes Z^T and dY^T into LDS with 16-bit stores (eight rows by eight vectors a
//             wave: two-way bank conflicts), 4 x 2 accumulator tiles a wave; the partial tile goes to scratch.
//   finish    sums the dW partials over the splits and the dgamma / dbeta partials over the workgroups of k_pm_dx in index order:
//             no atomics, no memset, every output element written by one lane, bit-reproducible, capturable.
#include <type_traits>

#include "common.h"
#include "dispatch.h"

namespace {

constexpr int PM_THREADS = 256;
constexpr int PM_MAX_K = 2048;
constexpr int PM_RING_PITCH = 80;                  // 32 reduction values of 2 bytes + 16: rows of the W^T / Z^T / dY^T images
constexpr int PM_RING_SLOT = 256 * PM_RING_PITCH;  // one slot: 256 rows

struct PmParams {
    const void* x[MTLORA_PM_MAX_STREAMS];
    void* dx[MTLORA_PM_MAX_STREAMS];
    const float *gamma, *beta, *W;
    void* y;
    const void* dy;
    float *mean, *rstd;
    float *part_gb, *part_w;  // backward partials: [workgroup of k_pm_dx][2][K], [row split][N][K]
    int64_t img_stride;       // H W C: elements of one image of a stream
    int M, Ms, H2W2, W2, Wd, C, K, N, n_blocks, rows_per_split;
    float eps, inv_K;
};

template <typename T>
__device__ __forceinline__ void pm_mma(const u32x4& a, const u32x4& b, f32x16& c) {
    if constexpr (__is_same(T, f16))
        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// element offset of x(2i, 2j) of merged row m inside its stream
__device__ __forceinline__ int64_t pm_row_off(const PmParams& p, int m, int& stream) {
    stream = m / p.Ms;
    int r = m - stream * p.Ms;
    const int b = r / p.H2W2;
    r -= b * p.H2W2;
    const int i = r / p.W2, j = r - i * p.W2;
    return (int64_t)b * p.img_stride + ((int64_t)(2 * i) * p.Wd + 2 * j) * p.C;
}
// ... of merged column k relative to it
__device__ __forceinline__ int pm_seg_off(const PmParams& p, int k) {
    const int q = k / p.C, c = k - q * p.C;
    return ((q & 1) * p.Wd + (q >> 1)) * p.C + c;
}
// the normalised value, the ONE expression the forward and the weight gradient share
__device__ __forceinline__ float pm_z(float x, float mean, float rstd, float g, float b) { return __fmaf_rn((x - mean) * rstd, g, b); }

template <typename XT>
__device__ __forceinline__ void pm_ld_vec(const XT* q, float (&f)[16 / sizeof(XT)]) {  // one 16-byte vector as floats
    if constexpr (sizeof(XT) == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(q);
        f[0] = v[0], f[1] = v[1], f[2] = v[2], f[3] = v[3];
    } else {
        const u32x4 v = *reinterpret_cast<const u32x4*>(q);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            f[2 * w] = mtl_lo2<XT>(v[w]);
            f[2 * w + 1] = mtl_hi2<XT>(v[w]);
        }
    }
}
template <int N>
__device__ __forceinline__ void pm_ld_f32(const float* q, float (&f)[N]) {
#pragma unroll
    for (int w = 0; w < N; w += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(q + w);
        f[w] = v[0], f[w + 1] = v[1], f[w + 2] = v[2], f[w + 3] = v[3];
    }
}
__device__ __forceinline__ float pm_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float pm_half_sum(float v) {  // over the 32 lanes of a lane half
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__host__ __device__ constexpr int pm_kcap(int rt) { return rt == 1 ? PM_MAX_K : rt == 2 ? 768 : 384; }
__host__ __device__ constexpr int pm_ks(int rt) { return rt == 1 ? 16 : 32; }  // k-slab of the forward's weight ring
__host__ __device__ constexpr int pm_fwd_lds(int rt, int K) { return 32 * rt * (2 * K + 16) + 2 * 256 * (2 * pm_ks(rt) + 16); }
__host__ __device__ constexpr int pm_dx_lds(int rt, int K) { return 2 * PM_RING_SLOT + 32 * rt * (16 + 4 * 4 + 4 * 2 * 4) + 2 * K * 4; }
constexpr int PM_DW_LDS = (128 + 256) * PM_RING_PITCH;

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
template <typename T, bool X32, int RT>
__global__ __launch_bounds__(PM_THREADS) void k_pm_fwd(const PmParams p) {
    using XT = std::conditional_t<X32, float, T>;
    constexpr int VEC = 16 / (int)sizeof(XT), R = 32 * RT, KS = pm_ks(RT), MAXV = (pm_kcap(RT) / VEC + 63) / 64;
    constexpr int WP = 2 * KS + 16, SLOT = 256 * WP, NLD = KS / 4;  // ring row pitch, slot bytes, 16-byte loads a thread and slab
    extern __shared__ __attribute__((aligned(16))) unsigned char pm_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, hh = lane >> 5;
    const int PA = 2 * p.K + 16;
    unsigned char* panel = pm_lds;
    unsigned char* ring = pm_lds + R * PA;
    const int nvec = p.K / VEC, nslab = p.K / KS;
    float gam[MAXV][VEC], bet[MAXV][VEC];  // of the lane's vectors v = lane + 64 i
    int seg[MAXV];
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int v = lane + 64 * i;
        seg[i] = 0;
        if (v < nvec) {
            pm_ld_f32<VEC>(p.gamma + v * VEC, gam[i]);
            pm_ld_f32<VEC>(p.beta + v * VEC, bet[i]);
            seg[i] = pm_seg_off(p, v * VEC);
        }
    }

    for (int blk = blockIdx.x; blk < p.n_blocks; blk += gridDim.x) {
        const int m0 = blk * R;
        // ---- the operand panel: rows wave, wave + 4, ... of the block ----
        for (int rr = wave; rr < R; rr += 4) {
            const int m = m0 + rr;
            unsigned char* prow = panel + rr * PA;
            if (m < p.M) {
                int st;
                const int64_t off = pm_row_off(p, m, st);
                const XT* xs = reinterpret_cast<const XT*>(p.x[st]) + off;
                float xv[MAXV][VEC];
                float s = 0.f;
#pragma unroll
                for (int i = 0; i < MAXV; ++i)
                    if (lane + 64 * i < nvec) {
                        pm_ld_vec<XT>(xs + seg[i], xv[i]);
#pragma unroll
                        for (int e = 0; e < VEC; ++e) s += xv[i][e];
                    }
                const float mean = pm_wave_sum(s) * p.inv_K;
                float s2 = 0.f;
#pragma unroll
                for (int i = 0; i < MAXV; ++i)
                    if (lane + 64 * i < nvec) {
#pragma unroll
                        for (int e = 0; e < VEC; ++e) {
                            const float d = xv[i][e] - mean;
                            s2 += d * d;
                        }
                    }
                const float rstd = rsqrtf(pm_wave_sum(s2) * p.inv_K + p.eps);
#pragma unroll
                for (int i = 0; i < MAXV; ++i) {
                    const int v = lane + 64 * i;
                    if (v < nvec) {
                        uint32_t w[VEC / 2];
#pragma unroll
                        for (int e = 0; e < VEC; e += 2)
                            w[e / 2] = mtl_pk2<T>(pm_z(xv[i][e], mean, rstd, gam[i][e], bet[i][e]),
                                                  pm_z(xv[i][e + 1], mean, rstd, gam[i][e + 1], bet[i][e + 1]));
                        if constexpr (VEC == 4)
                            *reinterpret_cast<u32x2*>(prow + v * 8) = u32x2{w[0], w[1]};
                        else
                            *reinterpret_cast<u32x4*>(prow + v * 16) = u32x4{w[0], w[1], w[2], w[3]};
                    }
                }
                if (lane == 0) {
                    p.mean[m] = mean;
                    p.rstd[m] = rstd;
                }
            } else {  // a row past M: a zero operand, never stored
#pragma unroll
                for (int i = 0; i < MAXV; ++i) {
                    const int v = lane + 64 * i;
                    if (v < nvec) {
                        if constexpr (VEC == 4)
                            *reinterpret_cast<u32x2*>(prow + v * 8) = u32x2{0u, 0u};
                        else
                            *reinterpret_cast<u32x4*>(prow + v * 16) = u32x4{0u, 0u, 0u, 0u};
                    }
                }
            }
        }
        __syncthreads();

        // ---- Y^T = W Z^T, 256 output columns at a time ----
        for (int nc0 = 0; nc0 < p.N; nc0 += 256) {
            const bool active = nc0 + 64 * wave < p.N;  // (N is a multiple of 64: a wave's columns are all inside or all outside)
            f32x16 acc[RT][2];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[rt][ct][r] = 0.f;
            f32x4 wr[NLD];
            auto wload = [&](int s) {
#pragma unroll
                for (int i = 0; i < NLD; ++i) {
                    const int v = tid + 256 * i, row = v / (KS / 4), qv = v % (KS / 4), n = nc0 + row;
                    wr[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (n < p.N) wr[i] = *reinterpret_cast<const f32x4*>(p.W + (int64_t)n * p.K + s * KS + 4 * qv);
                }
            };
            auto wstore = [&](int slot) {
#pragma unroll
                for (int i = 0; i < NLD; ++i) {
                    const int v = tid + 256 * i, row = v / (KS / 4), qv = v % (KS / 4);
                    *reinterpret_cast<u32x2*>(ring + slot * SLOT + row * WP + qv * 8) =
                        u32x2{mtl_pk2<T>(wr[i][0], wr[i][1]), mtl_pk2<T>(wr[i][2], wr[i][3])};
                }
            };
            wload(0);
            wstore(0);
            __syncthreads();
            for (int s = 0; s < nslab; ++s) {
                if (s + 1 < nslab) wload(s + 1);
                if (active) {
                    const unsigned char* slot = ring + (s & 1) * SLOT;
#pragma unroll
                    for (int ks = 0; ks < KS / 16; ++ks) {
                        u32x4 b[RT];
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt)
                            b[rt] = *reinterpret_cast<const u32x4*>(panel + (32 * rt + li) * PA + (s * KS + 16 * ks + 8 * hh) * 2);
#pragma unroll
                        for (int ct = 0; ct < 2; ++ct) {
                            const u32x4 a = *reinterpret_cast<const u32x4*>(slot + (64 * wave + 32 * ct + li) * WP + (16 * ks + 8 * hh) * 2);
#pragma unroll
                            for (int rt = 0; rt < RT; ++rt) pm_mma<T>(a, b[rt], acc[rt][ct]);
                        }
                    }
                }
                if (s + 1 < nslab) wstore((s + 1) & 1);
                __syncthreads();
            }
            // register 4 g + e of tile (rt, ct) is column nc0 + 64 wave + 32 ct + 8 g + 4 hh + e of row 32 rt + li: the lower lane half
            // stores the 8-column runs g = 0, 1, the upper g = 2, 3; each hands the other its pieces
            if (active) {
                T* y = reinterpret_cast<T*>(p.y);
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const int m = m0 + 32 * rt + li;
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) {
                        const f32x16& v = acc[rt][ct];
                        const u32x4 lo = {mtl_pk2<T>(v[0], v[1]), mtl_pk2<T>(v[2], v[3]), mtl_pk2<T>(v[4], v[5]), mtl_pk2<T>(v[6], v[7])};
                        const u32x4 hi = {mtl_pk2<T>(v[8], v[9]), mtl_pk2<T>(v[10], v[11]), mtl_pk2<T>(v[12], v[13]), mtl_pk2<T>(v[14], v[15])};
                        u32x4 got;
#pragma unroll
                        for (int w = 0; w < 4; ++w) got[w] = (uint32_t)__shfl_xor((int)(hh ? lo[w] : hi[w]), 32, 64);
#pragma unroll
                        for (int g = 0; g < 2; ++g) {
                            const u32x4 upper = {got[2 * g], got[2 * g + 1], hi[2 * g], hi[2 * g + 1]};
                            const u32x4 lower = {lo[2 * g], lo[2 * g + 1], got[2 * g], got[2 * g + 1]};
                            if (m < p.M)
                                *reinterpret_cast<u32x4*>(y + (int64_t)m * p.N + nc0 + 64 * wave + 32 * ct + 8 * (g + 2 * hh)) = hh ? upper : lower;
                        }
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// backward: dx, and the partial dgamma / dbeta
// ------------------------------------------------------------------------------------------------
// g of the rows m0 .. m0 + 32 RT and the columns kc0 + 64 wave .. + 64, SWAP false: acc[rt][ct][r] = g[32 rt + d_row(r)][32 ct + li]
// (lane = column), SWAP true: = g[32 rt + li][32 ct + 8 (r >> 2) + 4 hh + (r & 3)] (lane = row).  A wave stages the rows of the W^T
// image it reads itself; the barriers keep the two slots apart.
template <typename T, int RT, bool SWAP>
__device__ __forceinline__ void pm_g_chunk(const PmParams& p, unsigned char* ring, int m0, int kc0, int tid, f32x16 (&acc)[RT][2]) {
    const int lane = tid & 63, wave = tid >> 6, li = lane & 31, hh = lane >> 5, kvl = lane & 15, npl = lane >> 4;
    const bool active = kc0 + 64 * wave < p.K;  // (K is a multiple of 128)
    const int kcol = kc0 + 64 * wave + 4 * kvl, nslab = p.N / 32;
    const T* dy = reinterpret_cast<const T*>(p.dy);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[rt][ct][r] = 0.f;
    f32x4 wr[8];
    auto wload = [&](int s) {  // rows 32 s + 2 np, + 1 of W (np = npl + 4 i), the lane's four columns
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = 32 * s + 2 * (npl + 4 * i);
            wr[2 * i] = wr[2 * i + 1] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (active) {
                wr[2 * i] = *reinterpret_cast<const f32x4*>(p.W + (int64_t)n * p.K + kcol);
                wr[2 * i + 1] = *reinterpret_cast<const f32x4*>(p.W + (int64_t)(n + 1) * p.K + kcol);
            }
        }
    };
    auto wstore = [&](int slot) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                *reinterpret_cast<uint32_t*>(ring + slot * PM_RING_SLOT + (64 * wave + 4 * kvl + e) * PM_RING_PITCH + (npl + 4 * i) * 4) =
                    mtl_pk2<T>(wr[2 * i][e], wr[2 * i + 1][e]);
    };
    wload(0);
    wstore(0);
    __syncthreads();
    for (int s = 0; s < nslab; ++s) {
        if (s + 1 < nslab) wload(s + 1);
        if (active) {
            const unsigned char* slot = ring + (s & 1) * PM_RING_SLOT;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                u32x4 d[RT];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const int m = m0 + 32 * rt + li;
                    d[rt] = u32x4{0u, 0u, 0u, 0u};
                    if (m < p.M) d[rt] = *reinterpret_cast<const u32x4*>(dy + (int64_t)m * p.N + 32 * s + 16 * ks + 8 * hh);
                }
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    const u32x4 w = *reinterpret_cast<const u32x4*>(slot + (64 * wave + 32 * ct + li) * PM_RING_PITCH + (16 * ks + 8 * hh) * 2);
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        if constexpr (SWAP)
                            pm_mma<T>(w, d[rt], acc[rt][ct]);
                        else
                            pm_mma<T>(d[rt], w, acc[rt][ct]);
                    }
                }
            }
        }
        if (s + 1 < nslab) wstore((s + 1) & 1);
        __syncthreads();
    }
}

template <typename T, bool X32, int RT>
__global__ __launch_bounds__(PM_THREADS) void k_pm_dx(const PmParams p) {
    using XT = std::conditional_t<X32, float, T>;
    constexpr int R = 32 * RT;
    extern __shared__ __attribute__((aligned(16))) unsigned char pm_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, hh = lane >> 5;
    unsigned char* ring = pm_lds;
    uint64_t* xptr = reinterpret_cast<uint64_t*>(pm_lds + 2 * PM_RING_SLOT);  // per row of the block: x(2i, 2j), 0 past M
    uint64_t* dxptr = xptr + R;
    float* stat = reinterpret_cast<float*>(dxptr + R);  // per row: mean, rstd, s1 / K, s2 / K
    float* red = stat + 4 * R;                          // [wave][row][2]
    float* colsum = red + 4 * R * 2;                    // dgamma[K], dbeta[K] of this workgroup
    for (int k = tid; k < 2 * p.K; k += PM_THREADS) colsum[k] = 0.f;

    for (int blk = blockIdx.x; blk < p.n_blocks; blk += gridDim.x) {
        const int m0 = blk * R;
        if (tid < R) {
            const int m = m0 + tid;
            uint64_t xa = 0, da = 0;
            float mu = 0.f, rs = 0.f;
            if (m < p.M) {
                int st;
                const int64_t off = pm_row_off(p, m, st);
                xa = (uint64_t)(reinterpret_cast<const XT*>(p.x[st]) + off);
                da = (uint64_t)(reinterpret_cast<XT*>(p.dx[st]) + off);
                mu = p.mean[m];
                rs = p.rstd[m];
            }
            xptr[tid] = xa;
            dxptr[tid] = da;
            stat[4 * tid] = mu;
            stat[4 * tid + 1] = rs;
        }
        __syncthreads();

        // ---- pass A: row sums of g gamma and g gamma xhat, column sums of g xhat and g ----
        float p1[RT][16], p2[RT][16];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) p1[rt][r] = p2[rt][r] = 0.f;
        for (int kc0 = 0; kc0 < p.K; kc0 += 256) {
            f32x16 acc[RT][2];
            pm_g_chunk<T, RT, false>(p, ring, m0, kc0, tid, acc);
            if (kc0 + 64 * wave < p.K) {
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    const int k = kc0 + 64 * wave + 32 * ct + li, so = pm_seg_off(p, k);
                    const float gm = p.gamma[k];
                    float dg = 0.f, db = 0.f;
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int row = 32 * rt + mtl_d_row(lane, r);
                            const XT* xp = reinterpret_cast<const XT*>(xptr[row]);
                            const float xh = xp ? (mtl_to_f32(xp[so]) - stat[4 * row]) * stat[4 * row + 1] : 0.f;
                            const float a = acc[rt][ct][r], gg = a * gm;  // (a row past M: dY, hence a, is zero)
                            p1[rt][r] += gg;
                            p2[rt][r] += gg * xh;
                            dg += a * xh;
                            db += a;
                        }
                    dg += __shfl_xor(dg, 32, 64);
                    db += __shfl_xor(db, 32, 64);
                    if (hh == 0) {  // column k belongs to this lane alone
                        colsum[k] += dg;
                        colsum[p.K + k] += db;
                    }
                }
            }
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v1 = pm_half_sum(p1[rt][r]), v2 = pm_half_sum(p2[rt][r]);
                if (li == 0) {
                    float* q = red + (wave * R + 32 * rt + mtl_d_row(lane, r)) * 2;
                    q[0] = v1;
                    q[1] = v2;
                }
            }
        __syncthreads();
        if (tid < R) {
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                s1 += red[(w * R + tid) * 2];
                s2 += red[(w * R + tid) * 2 + 1];
            }
            stat[4 * tid + 2] = s1 * p.inv_K;
            stat[4 * tid + 3] = s2 * p.inv_K;
        }
        __syncthreads();

        // ---- pass B: g again, lane = row; dx to the four token positions ----
        for (int kc0 = 0; kc0 < p.K; kc0 += 256) {
            f32x16 acc[RT][2];
            pm_g_chunk<T, RT, true>(p, ring, m0, kc0, tid, acc);
            if (kc0 + 64 * wave < p.K) {
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int k4 = kc0 + 64 * wave + 32 * ct + 8 * g + 4 * hh, so = pm_seg_off(p, k4);  // (four columns of one segment)
                        const f32x4 gm = *reinterpret_cast<const f32x4*>(p.gamma + k4);
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt) {
                            const int row = 32 * rt + li;
                            const XT* xp = reinterpret_cast<const XT*>(xptr[row]);
                            if (!xp) continue;
                            XT* dp = reinterpret_cast<XT*>(dxptr[row]) + so;
                            const float mu = stat[4 * row], rs = stat[4 * row + 1], s1 = stat[4 * row + 2], s2 = stat[4 * row + 3];
                            float xv[4], d[4];
                            if constexpr (X32) {
                                const f32x4 v = *reinterpret_cast<const f32x4*>(xp + so);
                                xv[0] = v[0], xv[1] = v[1], xv[2] = v[2], xv[3] = v[3];
                            } else {
                                const u32x2 v = *reinterpret_cast<const u32x2*>(xp + so);
                                xv[0] = mtl_lo2<T>(v[0]), xv[1] = mtl_hi2<T>(v[0]), xv[2] = mtl_lo2<T>(v[1]), xv[3] = mtl_hi2<T>(v[1]);
                            }
#pragma unroll
                            for (int e = 0; e < 4; ++e) d[e] = rs * (acc[rt][ct][4 * g + e] * gm[e] - s1 - (xv[e] - mu) * rs * s2);
                            if constexpr (X32)
                                *reinterpret_cast<f32x4*>(dp) = f32x4{d[0], d[1], d[2], d[3]};
                            else
                                *reinterpret_cast<u32x2*>(dp) = u32x2{mtl_pk2<T>(d[0], d[1]), mtl_pk2<T>(d[2], d[3])};
                        }
                    }
            }
        }
        __syncthreads();  // (the next block rewrites the row table)
    }
    __syncthreads();
    float* out = p.part_gb + (int64_t)blockIdx.x * 2 * p.K;
    for (int k = tid; k < 2 * p.K; k += PM_THREADS) out[k] = colsum[k];
}

// ------------------------------------------------------------------------------------------------
// backward: partial dW = dY^T Z of one 128 x 256 tile and one row split
// ------------------------------------------------------------------------------------------------
template <typename T, bool X32>
__global__ __launch_bounds__(PM_THREADS) void k_pm_dw(const PmParams p) {
    using XT = std::conditional_t<X32, float, T>;
    constexpr int VEC = 16 / (int)sizeof(XT), KVJ = 256 / VEC / 32;  // vectors of a row's 256 columns a lane loads: 2 (fp32), 1
    extern __shared__ __attribute__((aligned(16))) unsigned char pm_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, hh = lane >> 5;
    unsigned char* dyT = pm_lds;                        // [n 128][m 32]
    unsigned char* zT = pm_lds + 128 * PM_RING_PITCH;   // [k 256][m 32]
    const int k0 = blockIdx.x * 256, n0 = blockIdx.y * 128, split = blockIdx.z;
    const int r0 = split * p.rows_per_split, r1 = min(p.M, r0 + p.rows_per_split);
    const bool active = k0 + 64 * wave < p.K;
    // z: the lane's rows msub + 8 mh and vectors kvl + 8 (wave + 4 j) of the tile
    const int kvl = lane & 7, msub = lane >> 3;
    int kl[KVJ], seg[KVJ];
    bool kok[KVJ];
    float gam[KVJ][VEC], bet[KVJ][VEC];
#pragma unroll
    for (int j = 0; j < KVJ; ++j) {
        kl[j] = (kvl + 8 * (wave + 4 * j)) * VEC;
        kok[j] = k0 + kl[j] < p.K;
        seg[j] = 0;
        if (kok[j]) {
            seg[j] = pm_seg_off(p, k0 + kl[j]);
            pm_ld_f32<VEC>(p.gamma + k0 + kl[j], gam[j]);
            pm_ld_f32<VEC>(p.beta + k0 + kl[j], bet[j]);
        }
    }
    // dY: rows ms2 + 16 (c >> 2), vectors nvl + 4 (c & 3) for c = wave + 4 i
    const int nvl = lane & 3, ms2 = lane >> 2;
    const T* dy = reinterpret_cast<const T*>(p.dy);
    f32x16 acc[4][2];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nt][ct][r] = 0.f;

    for (int ms = r0; ms < r1; ms += 32) {
        uint32_t zr[4][KVJ][VEC / 2];
#pragma unroll
        for (int mh = 0; mh < 4; ++mh) {
            const int m = ms + msub + 8 * mh;
#pragma unroll
            for (int j = 0; j < KVJ; ++j)
#pragma unroll
                for (int e = 0; e < VEC / 2; ++e) zr[mh][j][e] = 0u;
            if (m < r1) {
                int st;
                const int64_t off = pm_row_off(p, m, st);
                const XT* xs = reinterpret_cast<const XT*>(p.x[st]) + off;
                const float mu = p.mean[m], rs = p.rstd[m];
#pragma unroll
                for (int j = 0; j < KVJ; ++j)
                    if (kok[j]) {
                        float xv[VEC];
                        pm_ld_vec<XT>(xs + seg[j], xv);
#pragma unroll
                        for (int e = 0; e < VEC; e += 2)
                            zr[mh][j][e / 2] = mtl_pk2<T>(pm_z(xv[e], mu, rs, gam[j][e], bet[j][e]), pm_z(xv[e + 1], mu, rs, gam[j][e + 1], bet[j][e + 1]));
                    }
            }
        }
        u32x4 dr[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c = wave + 4 * i, m = ms + ms2 + 16 * (c >> 2), n = n0 + 8 * (nvl + 4 * (c & 3));
            dr[i] = u32x4{0u, 0u, 0u, 0u};
            if (m < r1 && n < p.N) dr[i] = *reinterpret_cast<const u32x4*>(dy + (int64_t)m * p.N + n);
        }
        __syncthreads();  // (the previous slab's operands are read)
#pragma unroll
        for (int mh = 0; mh < 4; ++mh)
#pragma unroll
            for (int j = 0; j < KVJ; ++j)
#pragma unroll
                for (int e = 0; e < VEC; ++e)
                    *reinterpret_cast<uint16_t*>(zT + (kl[j] + e) * PM_RING_PITCH + (msub + 8 * mh) * 2) = (uint16_t)(zr[mh][j][e >> 1] >> (16 * (e & 1)));
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c = wave + 4 * i;
#pragma unroll
            for (int e = 0; e < 8; ++e)
                *reinterpret_cast<uint16_t*>(dyT + (8 * (nvl + 4 * (c & 3)) + e) * PM_RING_PITCH + (ms2 + 16 * (c >> 2)) * 2) =
                    (uint16_t)(dr[i][e >> 1] >> (16 * (e & 1)));
        }
        __syncthreads();
        if (active) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                u32x4 b[2];
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
                    b[ct] = *reinterpret_cast<const u32x4*>(zT + (64 * wave + 32 * ct + li) * PM_RING_PITCH + (16 * ks + 8 * hh) * 2);
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    const u32x4 a = *reinterpret_cast<const u32x4*>(dyT + (32 * nt + li) * PM_RING_PITCH + (16 * ks + 8 * hh) * 2);
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) pm_mma<T>(a, b[ct], acc[nt][ct]);
                }
            }
        }
    }
    if (active) {
        float* out = p.part_w + (int64_t)split * p.N * p.K;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n0 + 32 * nt + mtl_d_row(lane, r);
                if (n < p.N) {
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) out[(int64_t)n * p.K + k0 + 64 * wave + 32 * ct + li] = acc[nt][ct][r];
                }
            }
    }
}

// sums the S dW partials and the G dgamma / dbeta partials in index order; one thread per output element
__global__ __launch_bounds__(256) void k_pm_finish(const float* __restrict__ part_w, int S, const float* __restrict__ part_gb, int G, int N, int K,
                                                   float* dW, float* dgamma, float* dbeta) {
    const int64_t NK = (int64_t)N * K, q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q < NK) {
        if (!dW) return;
        float a = 0.f;
#pragma unroll 4
        for (int s = 0; s < S; ++s) a += part_w[s * NK + q];
        dW[q] = a;
    } else if (q < NK + 2 * K) {
        const int v = (int)(q - NK);
        float* dst = v < K ? dgamma : dbeta;
        if (!dst) return;
        float a = 0.f;
#pragma unroll 4
        for (int g = 0; g < G; ++g) a += part_gb[(int64_t)g * 2 * K + v];
        dst[v < K ? v : v - K] = a;
    }
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
int pm_rt(int K) { return K <= 384 ? 4 : K <= 768 ? 2 : 1; }
int pm_rt_dx(int K) { return K <= 768 ? 2 : 1; }  // (four row tiles and the two sets of row sums do not fit the registers)
template <typename F>
void pm_dispatch_rt(int rt, F&& f) {
    switch (rt) {
        case 4: return f(MtlInt<4>{});
        case 2: return f(MtlInt<2>{});
        default: return f(MtlInt<1>{});
    }
}

int64_t pm_rows(const mtlora_patch_merge_desc* d) { return (int64_t)d->n * d->B * (d->H / 2) * (d->W / 2); }

// MTLORA_OK when the kernels take the descriptor, else the status every entry returns for it
int pm_check(const mtlora_patch_merge_desc* d) {
    if (!d) return MTLORA_ERR_NULL;
    if (!mtl_dtype_in(d->dtype, MTL_DT_ALL) || !mtl_dtype_in(d->x_dtype, MTL_DT_ALL)) return MTLORA_ERR_DTYPE;
    if (d->B < 0 || d->n < 1 || d->H <= 0 || d->W <= 0 || d->C <= 0 || d->max_groups < 0) return MTLORA_ERR_SHAPE;
    if (!mtl_dtype_in(d->dtype, MTL_DT_16) || (d->x_dtype != MTLORA_F32 && d->x_dtype != d->dtype)) return MTLORA_ERR_UNSUPPORTED;
    if (d->n > MTLORA_PM_MAX_STREAMS || d->C % 32 || 4 * d->C > PM_MAX_K || d->H % 2 || d->W % 2) return MTLORA_ERR_UNSUPPORTED;
    if (d->B > ((int64_t)1 << 31) || pm_rows(d) >= ((int64_t)1 << 31) - 4096) return MTLORA_ERR_UNSUPPORTED;  // (rows are int, offsets 64-bit)
    return MTLORA_OK;
}

PmParams pm_params(const mtlora_patch_merge_desc* d) {
    PmParams p = {};
    p.C = d->C;
    p.K = 4 * d->C;
    p.N = 2 * d->C;
    p.Wd = d->W;
    p.W2 = d->W / 2;
    p.H2W2 = (d->H / 2) * p.W2;
    p.Ms = (int)(d->B * p.H2W2);
    p.M = (int)pm_rows(d);
    p.img_stride = (int64_t)d->H * d->W * d->C;
    p.n_blocks = (int)mtl_ceil_div(p.M, 32 * pm_rt(p.K));
    p.eps = d->eps;
    p.inv_K = 1.f / (float)p.K;
    return p;
}

int pm_cus() {
    int dev = 0, cus = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    return cus;
}
// workgroups of a persistent launch: `per_cu` per compute unit, at most one per row block, at most max_groups when that is set
int pm_groups(const mtlora_patch_merge_desc* d, int n_blocks, int per_cu) {
    int64_t g = (int64_t)pm_cus() * per_cu;
    if (d->max_groups > 0 && d->max_groups < g) g = d->max_groups;
    if (n_blocks < g) g = n_blocks;
    return (int)(g < 1 ? 1 : g);
}
// row splits of the dW launch (a function of the shape alone) and the rows of one; max_groups set: one split walks every row
int pm_splits(const mtlora_patch_merge_desc* d, const PmParams& p, int* rows_per_split) {
    const int64_t tiles = mtl_ceil_div(p.K, 256) * mtl_ceil_div(p.N, 128);
    int64_t S = d->max_groups > 0 ? 1 : mtl_ceil_div(1024, tiles);
    if (S > 64) S = 64;
    if (S > mtl_ceil_div(p.M, 32)) S = mtl_ceil_div(p.M, 32);
    *rows_per_split = (int)mtl_round_up(mtl_ceil_div(p.M, S), 32);  // (a trailing split may be left without rows: it writes zeros)
    return (int)S;
}

template <typename K>
void pm_launch(K fn, dim3 grid, int lds, const PmParams& p, hipStream_t s) {
    if (lds > 48 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipLaunchKernelGGL(fn, grid, dim3(PM_THREADS), lds, s, p);
}

template <typename F>
void pm_dispatch(const mtlora_patch_merge_desc* d, F&& f) {  // f(T tag, bool_constant<x is fp32>)
    mtl_dispatch_dtype16(d->dtype, [&](auto tt) {
        if (d->x_dtype == MTLORA_F32)
            f(tt, std::true_type{});
        else
            f(tt, std::false_type{});
    });
}

}  // namespace

extern "C" {

int mtlora_patch_merge_fwd(const mtlora_patch_merge_desc* d, const void* const* x, const float* gamma, const float* beta, const float* W,
                           void* y, float* mean, float* rstd, void* stream) {
    const int st = pm_check(d);
    if (st != MTLORA_OK) return st;
    if (pm_rows(d) == 0) return MTLORA_OK;
    if (mtl_any_null({gamma, beta, W, y, mean, rstd}, d->n, {x})) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({gamma, beta, W, y}, d->n, {x})) return MTLORA_ERR_ALIGN;  // (mean, rstd: scalar accesses only)
    PmParams p = pm_params(d);
    for (int k = 0; k < d->n; ++k) p.x[k] = x[k];
    p.gamma = gamma;
    p.beta = beta;
    p.W = W;
    p.y = y;
    p.mean = mean;
    p.rstd = rstd;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const double es_x = d->x_dtype == MTLORA_F32 ? 4 : 2;
    MtlProfScope prof(PK_NT_PLAIN_FWD, (double)p.M * (p.K * es_x + p.N * 2.0), s);
    const int grid = pm_groups(d, p.n_blocks, 1);
    pm_dispatch(d, [&](auto tt, auto x32) {
        using T = typename decltype(tt)::type;
        pm_dispatch_rt(pm_rt(p.K), [&](auto rtt) {
            constexpr int RT = decltype(rtt)::value;
            pm_launch(k_pm_fwd<T, decltype(x32)::value, RT>, dim3((unsigned)grid), pm_fwd_lds(RT, p.K), p, s);
        });
    });
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

int64_t mtlora_patch_merge_bwd_scratch_bytes(const mtlora_patch_merge_desc* d) {
    if (pm_check(d) != MTLORA_OK) return -1;
    if (pm_rows(d) == 0) return 0;
    const PmParams p = pm_params(d);
    int rps = 0;
    const int S = pm_splits(d, p, &rps), G = pm_groups(d, (int)mtl_ceil_div(p.M, 32 * pm_rt_dx(p.K)), 2);
    return ((int64_t)G * 2 * p.K + (int64_t)S * p.N * p.K) * 4;
}

int mtlora_patch_merge_bwd(const mtlora_patch_merge_desc* d, const void* const* x, const float* gamma, const float* beta, const float* W,
                           const float* mean, const float* rstd, const void* dy, void* const* dx, float* dW, float* dgamma, float* dbeta,
                           void* scratch, int64_t scratch_bytes, void* stream) {
    const int st = pm_check(d);
    if (st != MTLORA_OK) return st;
    if (pm_rows(d) == 0) return MTLORA_OK;
    if (mtl_any_null({gamma, beta, W, mean, rstd, dy, scratch}, d->n, {x, mtl_arr(dx)})) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({gamma, beta, W, dy, dW, dgamma, dbeta, scratch}, d->n, {x, mtl_arr(dx)})) return MTLORA_ERR_ALIGN;
    if (scratch_bytes < mtlora_patch_merge_bwd_scratch_bytes(d)) return MTLORA_ERR_WORKSPACE;
    PmParams p = pm_params(d);
    for (int k = 0; k < d->n; ++k) {
        p.x[k] = x[k];
        p.dx[k] = dx[k];
    }
    p.gamma = gamma;
    p.beta = beta;
    p.W = W;
    p.mean = const_cast<float*>(mean);
    p.rstd = const_cast<float*>(rstd);
    p.dy = dy;
    p.n_blocks = (int)mtl_ceil_div(p.M, 32 * pm_rt_dx(p.K));
    const int S = pm_splits(d, p, &p.rows_per_split), G = pm_groups(d, p.n_blocks, 2);
    p.part_gb = reinterpret_cast<float*>(scratch);
    p.part_w = p.part_gb + (int64_t)G * 2 * p.K;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const double es_x = d->x_dtype == MTLORA_F32 ? 4 : 2;
    MtlProfScope prof(PK_NT_PLAIN_DX, (double)p.M * (2.0 * p.K * es_x + p.N * 2.0), s);
    pm_dispatch(d, [&](auto tt, auto x32) {
        using T = typename decltype(tt)::type;
        pm_dispatch_rt(pm_rt_dx(p.K), [&](auto rtt) {
            constexpr int RT = decltype(rtt)::value;
            if constexpr (RT <= 2) pm_launch(k_pm_dx<T, decltype(x32)::value, RT>, dim3((unsigned)G), pm_dx_lds(RT, p.K), p, s);
        });
        if (dW)
            pm_launch(k_pm_dw<T, decltype(x32)::value>, dim3((unsigned)mtl_ceil_div(p.K, 256), (unsigned)mtl_ceil_div(p.N, 128), (unsigned)S),
                      PM_DW_LDS, p, s);
    });
    MTL_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_pm_finish, dim3((unsigned)mtl_ceil_div((int64_t)p.N * p.K + 2 * p.K, 256)), dim3(256), 0, s, p.part_w, S, p.part_gb, G,
                       p.N, p.K, dW, dgamma, dbeta);
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

}  // extern "C"
