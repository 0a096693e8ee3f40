// patch_embed.hip -- the patch embedding (reference swin_transformer_mtlora.py PatchEmbed: Conv2d(k = s = 4) -> flatten -> transpose ->
// LayerNorm) as ONE kernel each way, straight from the NCHW image:
//
//   mtlora_patch_embed_fwd   y[m, :] = LN(W patch(m) + b)              k_patch_embed_fwd, one launch
//   mtlora_patch_embed_bwd   dW, db, dgamma, dbeta (no input gradient) k_patch_embed_bwd + k_patch_embed_reduce
//
// Token m = (b, py, px); k = c 16 + dy 4 + dx indexes the K = 16 in_chans values of its patch.  A wave owns 32 consecutive tokens, a
// workgroup PE_WAVES such blocks ("super block"); the grid is persistent: workgroup g takes super blocks g, g + grid, ...
//
//   input     no LDS.  An MFMA k-step is 16 deep and a lane (token, hh = lane >> 5) holds 8 of the 16: k-step s is channel c = s, the
//             lane's 8 values are the pixel rows (c, dy = 2 hh) and (c, 2 hh + 1) of its patch -- two 16-byte fp32 loads (8 bytes for a
//             16-bit image), contiguous across the lanes of a patch row -- rounded to the compute dtype in registers.  Tokens at or past
//             M are zero fragments, never loaded, never stored.  The fragments are sized for in_chans <= 4; a k-step at or past
//             in_chans is skipped.
//   weights   W (E x K, the fp32 master) is cast once per workgroup into an LDS image of 32 NT rows x 64 k (rows past E, k past K zero;
//             row pitch an odd number of 16-byte vectors), b / gamma / beta next to it; they stay for the whole persistent loop.
//   forward   Y^T = W X^T: accumulator tile t of lane (token j = lane & 31, hh) holds channels 32 t + 8 g + 4 hh + 0..3 (g = r >> 2) of
//             ITS token: bias, mean and variance (two passes, fp32, on the unrounded accumulators) are in-lane sums plus one exchange
//             between the lane halves.  Stores are whole 16-byte runs: four fp32 channels per (t, g), or, for a 16-bit output, the two
//             halves swap their 8-byte pieces first.  Saved: mean and rstd per token.
//   backward  the other orientation, Z = X W^T (the SAME fragments, operands swapped): lane (channel j of tile t, hh) holds 16 tokens
//             i(r) = (r & 3) + 8 (r >> 2) + 4 hh.  The column sums (dgamma += dy xhat, dbeta += dy, db += dz) are then one register per
//             tile, summed in-lane over tokens and blocks; the two row means of the LayerNorm backward are butterflies over the 32
//             lanes of a half.  dz stays in the accumulator registers and IS the B operand of dW^T += X^T dz (k = the tile's rows, as
//             accfrag of attention_wide.h); the A operand X^T (row = k index, reduction over tokens) goes through one small per-wave
//             LDS transpose whose token order inside a row is the accumulator's row order.  dW^T is 2 x NT accumulator tiles.
//   reduce    the waves of a workgroup add their accumulators in wave order in LDS, the workgroup writes ONE partial set, and
//             k_patch_embed_reduce sums the sets in index order: no atomics, no memset, every output element written by one lane,
//             bit-reproducible, capturable.
#include "common.h"
#include "dispatch.h"

namespace {

constexpr int PE_KS = 4;      // k-steps of 16 the fragments are sized for (in_chans <= 4)
constexpr int PE_MAX_E = 256;
constexpr int PE_WAVES = 4;
constexpr int PE_THREADS = PE_WAVES * 64;

struct PeParams {
    const void* img;
    const float* W;
    const float* b;
    const float* gamma;
    const float* beta;
    void* y;            // forward output
    float* mean;        // forward: out; backward: in
    float* rstd;
    const void* dy;
    float* part;        // backward: one partial set per workgroup
    int64_t M, chan_stride;  // tokens; H * W
    int C, Wd, Wp, HpWp, E, K;
    int img16, out16;   // image / output (gradient) in the 16-bit compute dtype, else fp32
    int want_w, want_n, n_super;
    float eps, inv_E;
};

// eight elements of T: one lane's share of a 16-deep k-step
template <typename T>
struct PeOp {
    u32x4 v[sizeof(T) / 2];
};
template <typename T>
__device__ __forceinline__ PeOp<T> pe_zero_op() {
    PeOp<T> o;
#pragma unroll
    for (int i = 0; i < (int)(sizeof(T) / 2); ++i) o.v[i] = u32x4{0u, 0u, 0u, 0u};
    return o;
}
template <typename T>
__device__ __forceinline__ void pe_mma(const PeOp<T>& a, const PeOp<T>& b, f32x16& c) {
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const f32x4 av = __builtin_bit_cast(f32x4, a.v[h]), bv = __builtin_bit_cast(f32x4, b.v[h]);
#pragma unroll
            for (int e = 0; e < 4; ++e) c = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], bv[e], c, 0, 0, 0);
        }
    } else if constexpr (__is_same(T, f16)) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a.v[0]), __builtin_bit_cast(f16x8, b.v[0]), c, 0, 0, 0);
    } else {
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a.v[0]), __builtin_bit_cast(bf16x8, b.v[0]), c, 0, 0, 0);
    }
}
// accumulator registers 8 s .. 8 s + 7 as the operand of k-step s (k = the tile's rows 16 s + (e & 3) + 8 (e >> 2) + 4 hh)
template <typename T>
__device__ __forceinline__ PeOp<T> pe_acc_op(const f32x16& a, int s) {
    PeOp<T> o;
    const int r = 8 * s;
    if constexpr (sizeof(T) == 4) {
        o.v[0] = __builtin_bit_cast(u32x4, f32x4{a[r], a[r + 1], a[r + 2], a[r + 3]});
        o.v[1] = __builtin_bit_cast(u32x4, f32x4{a[r + 4], a[r + 5], a[r + 6], a[r + 7]});
    } else {
        o.v[0] = u32x4{mtl_pk2<T>(a[r], a[r + 1]), mtl_pk2<T>(a[r + 2], a[r + 3]), mtl_pk2<T>(a[r + 4], a[r + 5]), mtl_pk2<T>(a[r + 6], a[r + 7])};
    }
    return o;
}

template <typename T>
__host__ __device__ constexpr int pe_w_pitch() { return 64 * (int)sizeof(T) + 16; }   // bytes per row of the W image
template <typename T>
__host__ __device__ constexpr int pe_xt_pitch() { return 32 * (int)sizeof(T) + 16; }  // bytes per row of a wave's X^T image
template <typename T, int NT>
__host__ __device__ constexpr int pe_w_bytes() { return NT * 32 * pe_w_pitch<T>(); }
template <typename T, int NT>
__host__ __device__ constexpr int pe_fwd_lds() { return pe_w_bytes<T, NT>() + 3 * NT * 32 * 4; }
__host__ __device__ constexpr int pe_set_floats(int nt) { return nt * (2 * 1024 + 3 * 32); }  // one partial set: 2 nt tiles, 3 vectors
template <typename T, int NT>
__host__ __device__ constexpr int pe_bwd_lds() {
    const int work = pe_w_bytes<T, NT>() + PE_WAVES * 64 * pe_xt_pitch<T>(), red = pe_set_floats(NT) * 4;
    return work > red ? work : red;
}

// W (fp32 master) -> the LDS image in T; rows at or past E and k at or past K are zeros
template <typename T, int NT>
__device__ __forceinline__ void pe_stage_w(const PeParams& p, unsigned char* lds, int tid) {
    for (int v = tid; v < NT * 32 * 16; v += PE_THREADS) {
        const int row = v >> 4, q = v & 15;  // q: the four k values 4 q .. 4 q + 3
        f32x4 w = {0.f, 0.f, 0.f, 0.f};
        if (row < p.E && 4 * q < p.K) w = *reinterpret_cast<const f32x4*>(p.W + row * p.K + 4 * q);
        unsigned char* dst = lds + row * pe_w_pitch<T>() + q * 4 * (int)sizeof(T);
        if constexpr (sizeof(T) == 4)
            *reinterpret_cast<f32x4*>(dst) = w;
        else
            *reinterpret_cast<u32x2*>(dst) = u32x2{mtl_pk2<T>(w[0], w[1]), mtl_pk2<T>(w[2], w[3])};
    }
}
template <typename T>
__device__ __forceinline__ PeOp<T> pe_w_op(const unsigned char* lds, int row, int s, int hh) {
    PeOp<T> o;
    const unsigned char* q = lds + row * pe_w_pitch<T>() + (16 * s + 8 * hh) * (int)sizeof(T);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(T) / 2); ++i) o.v[i] = *reinterpret_cast<const u32x4*>(q + 16 * i);
    return o;
}

// the lane's fragments of token m (li = lane & 31 of block m0): x[s] = pixel rows (c = s, dy = 2 hh) and (s, 2 hh + 1) in T
template <typename T>
__device__ __forceinline__ void pe_load_x(const PeParams& p, int64_t m, int hh, PeOp<T> (&x)[PE_KS]) {
    const bool in = m < p.M;
    const int mm = in ? (int)m : 0;
    const int b = mm / p.HpWp, rem = mm - b * p.HpWp;
    const int py = rem / p.Wp, px = rem - py * p.Wp;
    const int64_t off0 = (int64_t)b * p.C * p.chan_stride + (int64_t)(4 * py + 2 * hh) * p.Wd + 4 * px;
#pragma unroll
    for (int s = 0; s < PE_KS; ++s) {
        x[s] = pe_zero_op<T>();
        if (in && s < p.C) {
            const int64_t off = off0 + s * p.chan_stride;
            if constexpr (sizeof(T) == 4) {
                const float* q = reinterpret_cast<const float*>(p.img) + off;
                x[s].v[0] = *reinterpret_cast<const u32x4*>(q);
                x[s].v[1] = *reinterpret_cast<const u32x4*>(q + p.Wd);
            } else if (p.img16) {
                const T* q = reinterpret_cast<const T*>(p.img) + off;
                const u32x2 r0 = *reinterpret_cast<const u32x2*>(q), r1 = *reinterpret_cast<const u32x2*>(q + p.Wd);
                x[s].v[0] = u32x4{r0[0], r0[1], r1[0], r1[1]};
            } else {
                const float* q = reinterpret_cast<const float*>(p.img) + off;
                const f32x4 r0 = *reinterpret_cast<const f32x4*>(q), r1 = *reinterpret_cast<const f32x4*>(q + p.Wd);
                x[s].v[0] = u32x4{mtl_pk2<T>(r0[0], r0[1]), mtl_pk2<T>(r0[2], r0[3]), mtl_pk2<T>(r1[0], r1[1]), mtl_pk2<T>(r1[2], r1[3])};
            }
        }
    }
}

// NT: channel tiles of 32 the accumulators are sized for (E <= 32 NT; whole tiles at or past E are skipped)
template <typename T, bool NORM, int NT>
__global__ __launch_bounds__(PE_THREADS) void k_patch_embed_fwd(const PeParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pe_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, hh = lane >> 5;
    const int nt = p.E >> 5;
    float* vec = reinterpret_cast<float*>(pe_lds + pe_w_bytes<T, NT>());  // b, gamma, beta: NT * 32 floats each
    pe_stage_w<T, NT>(p, pe_lds, tid);
    for (int c = tid; c < NT * 32; c += PE_THREADS) {
        const bool in = c < p.E;
        vec[c] = in ? p.b[c] : 0.f;
        vec[NT * 32 + c] = NORM && in ? p.gamma[c] : 0.f;
        vec[2 * NT * 32 + c] = NORM && in ? p.beta[c] : 0.f;
    }
    __syncthreads();

    for (int sb = blockIdx.x; sb < p.n_super; sb += gridDim.x) {
        const int64_t m = ((int64_t)sb * PE_WAVES + wave) * 32 + li;
        const bool in = m < p.M;
        PeOp<T> x[PE_KS];
        pe_load_x<T>(p, m, hh, x);
        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
            if (t < nt) {
#pragma unroll
                for (int s = 0; s < PE_KS; ++s)
                    if (s < p.C) pe_mma<T>(pe_w_op<T>(pe_lds, 32 * t + li, s, hh), x[s], acc[t]);
            }
        }
        // + bias; register 4 g + e of tile t is channel 32 t + 8 g + 4 hh + e of the lane's token
        float s1 = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if (t < nt) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 bv = *reinterpret_cast<const f32x4*>(vec + 32 * t + 8 * g + 4 * hh);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        acc[t][4 * g + e] += bv[e];
                        s1 += acc[t][4 * g + e];
                    }
                }
            }
        float mean = 0.f, rstd = 1.f;
        if constexpr (NORM) {
            s1 += __shfl_xor(s1, 32, 64);
            mean = s1 * p.inv_E;
            float s2 = 0.f;
#pragma unroll
            for (int t = 0; t < NT; ++t)
                if (t < nt) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float d = acc[t][r] - mean;
                        s2 += d * d;
                    }
                }
            s2 += __shfl_xor(s2, 32, 64);
            rstd = rsqrtf(s2 * p.inv_E + p.eps);
            if (in && hh == 0) {
                p.mean[m] = mean;
                p.rstd[m] = rstd;
            }
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (t >= nt) continue;
            float v[16];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int ch = 32 * t + 8 * g + 4 * hh;
                f32x4 gv = {1.f, 1.f, 1.f, 1.f}, ev = {0.f, 0.f, 0.f, 0.f};
                if constexpr (NORM) {
                    gv = *reinterpret_cast<const f32x4*>(vec + NT * 32 + ch);
                    ev = *reinterpret_cast<const f32x4*>(vec + 2 * NT * 32 + ch);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) v[4 * g + e] = NORM ? (acc[t][4 * g + e] - mean) * rstd * gv[e] + ev[e] : acc[t][4 * g + e];
            }
            bool stored = false;
            if constexpr (sizeof(T) == 2) {
                if (p.out16) {
                    // the lower lane half stores the 8-channel segments g = 0, 1, the upper g = 2, 3: each hands the other its pieces
                    u32x4 lo = {mtl_pk2<T>(v[0], v[1]), mtl_pk2<T>(v[2], v[3]), mtl_pk2<T>(v[4], v[5]), mtl_pk2<T>(v[6], v[7])};
                    u32x4 hi = {mtl_pk2<T>(v[8], v[9]), mtl_pk2<T>(v[10], v[11]), mtl_pk2<T>(v[12], v[13]), mtl_pk2<T>(v[14], v[15])};
                    u32x4 got;
#pragma unroll
                    for (int w = 0; w < 4; ++w) got[w] = (uint32_t)__shfl_xor((int)(hh ? lo[w] : hi[w]), 32, 64);
                    T* y = reinterpret_cast<T*>(p.y);
#pragma unroll
                    for (int g = 0; g < 2; ++g) {
                        const u32x4 upper = {got[2 * g], got[2 * g + 1], hi[2 * g], hi[2 * g + 1]};
                        const u32x4 lower = {lo[2 * g], lo[2 * g + 1], got[2 * g], got[2 * g + 1]};
                        if (in) *reinterpret_cast<u32x4*>(y + m * p.E + 32 * t + 8 * (g + 2 * hh)) = hh ? upper : lower;
                    }
                    stored = true;
                }
            }
            if (!stored && in) {
                float* y = reinterpret_cast<float*>(p.y) + m * p.E + 32 * t + 4 * hh;
#pragma unroll
                for (int g = 0; g < 4; ++g) *reinterpret_cast<f32x4*>(y + 8 * g) = f32x4{v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]};
            }
        }
    }
}

__device__ __forceinline__ float pe_half_sum(float v) {  // over the 32 lanes of a lane half, the result in every lane
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <typename T, bool NORM, int NT>
__global__ __launch_bounds__(PE_THREADS) void k_patch_embed_bwd(const PeParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pe_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, hh = lane >> 5;
    const int nt = p.E >> 5;
    unsigned char* xt = pe_lds + pe_w_bytes<T, NT>() + wave * 64 * pe_xt_pitch<T>();  // this wave's X^T image: row k, 32 tokens
    if constexpr (NORM) pe_stage_w<T, NT>(p, pe_lds, tid);
    // position of token li inside a row of X^T: the accumulator's row order, so that the 8 tokens of (k-step s, half hh) are contiguous
    const int xt_pos = 16 * (li >> 4) + 8 * ((li >> 2) & 1) + (li & 3) + 4 * ((li >> 3) & 1);
    float bias[NT], gam[NT];  // of the lane's channel 32 t + li
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const bool in = 32 * t + li < p.E;
        bias[t] = NORM && in ? p.b[32 * t + li] : 0.f;
        gam[t] = NORM && in ? p.gamma[32 * t + li] : 0.f;
    }
    f32x16 dwt[NT][2];
    float dgam[NT], dbet[NT], dbia[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        dgam[t] = dbet[t] = dbia[t] = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) dwt[t][0][r] = dwt[t][1][r] = 0.f;
    }
    __syncthreads();

    for (int sb = blockIdx.x; sb < p.n_super; sb += gridDim.x) {
        const int64_t m0 = ((int64_t)sb * PE_WAVES + wave) * 32;
        PeOp<T> x[PE_KS];
        pe_load_x<T>(p, m0 + li, hh, x);
        // dz[t][r]: row (token) i(r) = (r & 3) + 8 (r >> 2) + 4 hh of the block, column (channel) 32 t + li
        f32x16 dz[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t m = m0 + mtl_d_row(lane, r);
                float v = 0.f;
                if (t < nt && m < p.M) {
                    if (sizeof(T) == 2 && p.out16)
                        v = mtl_to_f32(reinterpret_cast<const T*>(p.dy)[m * p.E + 32 * t + li]);
                    else
                        v = reinterpret_cast<const float*>(p.dy)[m * p.E + 32 * t + li];
                }
                dz[t][r] = v;
            }
        if constexpr (NORM) {
            float mu[16], rs[16], p1[16], p2[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t m = m0 + mtl_d_row(lane, r);
                const bool in = m < p.M;
                mu[r] = in ? p.mean[m] : 0.f;
                rs[r] = in ? p.rstd[m] : 0.f;
                p1[r] = p2[r] = 0.f;
            }
            f32x16 xh[NT];  // Z = X W^T + b, then xhat; a token past M has rstd 0: xhat, g and dz are zeros
#pragma unroll
            for (int t = 0; t < NT; ++t) {
#pragma unroll
                for (int r = 0; r < 16; ++r) xh[t][r] = 0.f;
                if (t < nt) {
#pragma unroll
                    for (int s = 0; s < PE_KS; ++s)
                        if (s < p.C) pe_mma<T>(x[s], pe_w_op<T>(pe_lds, 32 * t + li, s, hh), xh[t]);
                    float sg = 0.f, sb2 = 0.f;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float xv = (xh[t][r] + bias[t] - mu[r]) * rs[r], d = dz[t][r], g = d * gam[t];
                        xh[t][r] = xv;
                        sg += d * xv;
                        sb2 += d;
                        p1[r] += g;
                        p2[r] += g * xv;
                        dz[t][r] = g;
                    }
                    dgam[t] += sg;
                    dbet[t] += sb2;
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                p1[r] = pe_half_sum(p1[r]) * p.inv_E;
                p2[r] = pe_half_sum(p2[r]) * p.inv_E;
            }
#pragma unroll
            for (int t = 0; t < NT; ++t)
                if (t < nt) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) dz[t][r] = rs[r] * (dz[t][r] - p1[r] - xh[t][r] * p2[r]);
                }
        }
        if (p.want_w) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                float s = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) s += dz[t][r];
                dbia[t] += s;
            }
            // X^T through LDS: element e of x[s] is k = 16 s + 8 hh + e of token li
            __syncthreads();  // (the previous block's reads of the image are done)
#pragma unroll
            for (int s = 0; s < PE_KS; ++s)
                if (s < p.C) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        unsigned char* dst = xt + (16 * s + 8 * hh + e) * pe_xt_pitch<T>() + xt_pos * (int)sizeof(T);
                        if constexpr (sizeof(T) == 4)
                            *reinterpret_cast<uint32_t*>(dst) = x[s].v[e >> 2][e & 3];
                        else
                            *reinterpret_cast<uint16_t*>(dst) = (uint16_t)(x[s].v[0][e >> 1] >> (16 * (e & 1)));
                    }
                }
            __syncthreads();
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) {
                if (32 * rt >= p.K) continue;
                const int row = 32 * rt + li;  // k index: the A operand's row; rows at or past K were never written: zero operands
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    PeOp<T> a = pe_zero_op<T>();
                    if (row < p.K) {
                        const unsigned char* q = xt + row * pe_xt_pitch<T>() + (16 * s + 8 * hh) * (int)sizeof(T);
#pragma unroll
                        for (int i = 0; i < (int)(sizeof(T) / 2); ++i) a.v[i] = *reinterpret_cast<const u32x4*>(q + 16 * i);
                    }
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        if (t < nt) pe_mma<T>(a, pe_acc_op<T>(dz[t], s), dwt[t][rt]);
                }
            }
        }
    }

    // the workgroup's partial set: [tile 2 t + rt][register][lane], then dgamma, dbeta, db as [NT * 32] each; waves add in wave order
    float* red = reinterpret_cast<float*>(pe_lds);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        dgam[t] += __shfl_xor(dgam[t], 32, 64);
        dbet[t] += __shfl_xor(dbet[t], 32, 64);
        dbia[t] += __shfl_xor(dbia[t], 32, 64);
    }
    __syncthreads();
    for (int w = 0; w < PE_WAVES; ++w) {
        if (wave == w) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                if (p.want_w) {
#pragma unroll
                    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            float* q = red + ((2 * t + rt) * 16 + r) * 64 + lane;
                            *q = w ? *q + dwt[t][rt][r] : dwt[t][rt][r];
                        }
                }
                if (hh == 0) {
                    float* q = red + 2 * NT * 1024 + 32 * t + li;
                    q[0] = w ? q[0] + dgam[t] : dgam[t];
                    q[NT * 32] = w ? q[NT * 32] + dbet[t] : dbet[t];
                    q[2 * NT * 32] = w ? q[2 * NT * 32] + dbia[t] : dbia[t];
                }
            }
        }
        __syncthreads();
    }
    float* out = p.part + (int64_t)blockIdx.x * pe_set_floats(NT);
    for (int q = tid + (p.want_w ? 0 : 2 * NT * 1024); q < pe_set_floats(NT); q += PE_THREADS) out[q] = red[q];  // (no dW tiles unless wanted)
}

// sums the G partial sets in index order; thread q owns element q of a set and writes the ONE output element it stands for
__global__ __launch_bounds__(256) void k_patch_embed_reduce(const float* __restrict__ part, int G, int NT, int E, int K, float* dW, float* db,
                                                            float* dgamma, float* dbeta) {
    const int S = pe_set_floats(NT);
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= S || (q < 2 * NT * 1024 && !dW)) return;  // (dW not wanted: its tiles were not written)
    float a = 0.f;
#pragma unroll 8
    for (int g = 0; g < G; ++g) a += part[(int64_t)g * S + q];
    if (q < 2 * NT * 1024) {
        const int tile = q >> 10, r = (q >> 6) & 15, lane = q & 63;
        const int ch = 32 * (tile >> 1) + (lane & 31), k = 32 * (tile & 1) + mtl_d_row(lane, r);
        if (dW && ch < E && k < K) dW[ch * K + k] = a;
    } else {
        const int v = q - 2 * NT * 1024, which = v / (NT * 32), ch = v - which * (NT * 32);
        float* dst = which == 0 ? dgamma : which == 1 ? dbeta : db;
        if (dst && ch < E) dst[ch] = a;
    }
}

int pe_nt(int E) {  // the instantiated tile counts: 1, 3, 4, 6, 8
    const int n = E / 32;
    return n <= 1 ? 1 : n <= 3 ? 3 : n <= 4 ? 4 : n <= 6 ? 6 : 8;
}
template <typename F>
void pe_dispatch_nt(int E, F&& f) {
    switch (pe_nt(E)) {
        case 1: return f(MtlInt<1>{});
        case 3: return f(MtlInt<3>{});
        case 4: return f(MtlInt<4>{});
        case 6: return f(MtlInt<6>{});
        default: return f(MtlInt<8>{});
    }
}

// MTLORA_OK when the kernels take the descriptor, else the status every entry returns for it
int pe_check(const mtlora_patch_embed_desc* d) {
    if (!d) return MTLORA_ERR_NULL;
    if (!mtl_dtype_in(d->dtype, MTL_DT_ALL) || !mtl_dtype_in(d->img_dtype, MTL_DT_ALL) || !mtl_dtype_in(d->out_dtype, MTL_DT_ALL))
        return MTLORA_ERR_DTYPE;
    if (d->B < 0 || d->in_chans <= 0 || d->H <= 0 || d->W <= 0 || d->patch <= 0 || d->E <= 0 || d->max_groups < 0 || d->grad_flags < 0 ||
        d->grad_flags > 3)
        return MTLORA_ERR_SHAPE;
    if (d->patch != 4 || d->in_chans > PE_KS || d->E % 32 || d->E > PE_MAX_E || d->H % 4 || d->W % 4) return MTLORA_ERR_UNSUPPORTED;
    // the image and the output are fp32 or in the compute dtype
    if ((d->img_dtype != MTLORA_F32 && d->img_dtype != d->dtype) || (d->out_dtype != MTLORA_F32 && d->out_dtype != d->dtype))
        return MTLORA_ERR_UNSUPPORTED;
    if (d->B * (d->H / 4) * (d->W / 4) >= ((int64_t)1 << 31)) return MTLORA_ERR_UNSUPPORTED;  // (element offsets are 64-bit, tokens int)
    return MTLORA_OK;
}

PeParams pe_params(const mtlora_patch_embed_desc* d) {
    PeParams p = {};
    p.C = d->in_chans;
    p.Wd = d->W;
    p.Wp = d->W / 4;
    p.HpWp = (d->H / 4) * p.Wp;
    p.M = d->B * p.HpWp;
    p.chan_stride = (int64_t)d->H * d->W;
    p.E = d->E;
    p.K = 16 * d->in_chans;
    p.img16 = d->img_dtype != MTLORA_F32;
    p.out16 = d->out_dtype != MTLORA_F32;
    p.eps = d->eps;
    p.inv_E = 1.f / (float)d->E;
    p.n_super = (int)mtl_ceil_div(p.M, PE_WAVES * 32);
    return p;
}

double pe_img_bytes(const mtlora_patch_embed_desc* d) {
    return (double)d->B * d->in_chans * d->H * d->W * (d->img_dtype == MTLORA_F32 ? 4 : 2);
}

int pe_cus() {
    int dev = 0, cus = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    return cus;
}
// workgroups of a launch: `per_cu` per compute unit, at most one per super block, at most max_groups when that is set
int pe_groups(const mtlora_patch_embed_desc* d, int n_super, int per_cu) {
    int64_t g = (int64_t)pe_cus() * per_cu;
    if (d->max_groups > 0 && d->max_groups < g) g = d->max_groups;
    if (n_super < g) g = n_super;
    return (int)(g < 1 ? 1 : g);
}

template <typename K>
void pe_launch(K fn, int grid, int lds, const PeParams& p, hipStream_t s) {
    if (lds > 48 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(PE_THREADS), lds, s, p);
}

}  // namespace

extern "C" {

int mtlora_patch_embed_supported(const mtlora_patch_embed_desc* d) { return pe_check(d) == MTLORA_OK ? 1 : 0; }

int mtlora_patch_embed_fwd(const mtlora_patch_embed_desc* d, const void* img, const float* W, const float* bias, const float* gamma,
                           const float* beta, void* y, float* mean, float* rstd, void* stream) {
    const int st = pe_check(d);
    if (st != MTLORA_OK) return st;
    if (d->B == 0) return MTLORA_OK;
    if (mtl_any_null({img, W, bias, y}) || (d->has_norm && mtl_any_null({gamma, beta, mean, rstd}))) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({img, W, bias, gamma, beta, y})) return MTLORA_ERR_ALIGN;  // (mean, rstd: scalar accesses only)
    PeParams p = pe_params(d);
    p.img = img;
    p.W = W;
    p.b = bias;
    p.gamma = gamma;
    p.beta = beta;
    p.y = y;
    p.mean = mean;
    p.rstd = rstd;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    MtlProfScope prof(PK_PATCH_EMBED_FWD, pe_img_bytes(d) + (double)p.M * d->E * (p.out16 ? 2 : 4), s);
    mtl_dispatch_dtype(d->dtype, [&](auto tt) {
        using T = typename decltype(tt)::type;
        pe_dispatch_nt(d->E, [&](auto ntt) {
            constexpr int NT = decltype(ntt)::value;
            constexpr int lds = pe_fwd_lds<T, NT>();
            const int grid = pe_groups(d, p.n_super, lds > 40 * 1024 ? 2 : 4);
            if (d->has_norm)
                pe_launch(k_patch_embed_fwd<T, true, NT>, grid, lds, p, s);
            else
                pe_launch(k_patch_embed_fwd<T, false, NT>, grid, lds, p, s);
        });
    });
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

int64_t mtlora_patch_embed_bwd_scratch_bytes(const mtlora_patch_embed_desc* d) {
    if (pe_check(d) != MTLORA_OK) return -1;
    const PeParams p = pe_params(d);
    return (int64_t)pe_groups(d, p.n_super, 1) * pe_set_floats(pe_nt(d->E)) * 4;
}

int mtlora_patch_embed_bwd(const mtlora_patch_embed_desc* d, const void* img, const float* W, const float* bias, const float* gamma,
                           const float* mean, const float* rstd, const void* dy, float* dW, float* db, float* dgamma, float* dbeta,
                           void* scratch, int64_t scratch_bytes, void* stream) {
    const int st = pe_check(d);
    if (st != MTLORA_OK) return st;
    const bool want_w = d->grad_flags & MTLORA_PE_GRAD_PROJ, want_n = d->has_norm && (d->grad_flags & MTLORA_PE_GRAD_NORM);
    if (d->B == 0 || !(want_w || want_n)) return MTLORA_OK;
    if (mtl_any_null({img, dy, scratch}) || (want_w && mtl_any_null({dW, db})) || (want_n && mtl_any_null({dgamma, dbeta})) ||
        (d->has_norm && mtl_any_null({W, bias, gamma, mean, rstd})))
        return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({img, W, bias, gamma, dy, dW, db, dgamma, dbeta, scratch})) return MTLORA_ERR_ALIGN;
    if (scratch_bytes < mtlora_patch_embed_bwd_scratch_bytes(d)) return MTLORA_ERR_WORKSPACE;
    PeParams p = pe_params(d);
    p.img = img;
    p.W = W;
    p.b = bias;
    p.gamma = gamma;
    p.mean = const_cast<float*>(mean);
    p.rstd = const_cast<float*>(rstd);
    p.dy = dy;
    p.part = reinterpret_cast<float*>(scratch);
    p.want_w = want_w;
    p.want_n = want_n;
    const int grid = pe_groups(d, p.n_super, 1), nt = pe_nt(d->E);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    MtlProfScope prof(PK_PATCH_EMBED_BWD, pe_img_bytes(d) + (double)p.M * d->E * (p.out16 ? 2 : 4), s);
    mtl_dispatch_dtype(d->dtype, [&](auto tt) {
        using T = typename decltype(tt)::type;
        pe_dispatch_nt(d->E, [&](auto ntt) {
            constexpr int NT = decltype(ntt)::value;
            if (d->has_norm)
                pe_launch(k_patch_embed_bwd<T, true, NT>, grid, pe_bwd_lds<T, NT>(), p, s);
            else
                pe_launch(k_patch_embed_bwd<T, false, NT>, grid, pe_bwd_lds<T, NT>(), p, s);
        });
    });
    MTL_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_patch_embed_reduce, dim3((unsigned)mtl_ceil_div(pe_set_floats(nt), 256)), dim3(256), 0, s, p.part, grid, nt, d->E,
                       p.K, want_w ? dW : nullptr, want_w ? db : nullptr, want_n ? dgamma : nullptr, want_n ? dbeta : nullptr);
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

}  // extern "C"
