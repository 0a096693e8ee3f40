// decoder_front.hip -- the front end of every task's decoder (reference models/swin_mtl.py:88-135, models/seg_hrnet.py:498-510): a
// bias-free 1x1 convolution of each stage's tokens, bilinear upsampling (align_corners=False) of the coarse maps to the finest grid,
// concatenation along channels -- as ONE launch forward and three backward, whatever the number of stages:
//
//   mtlora_decoder_front_fwd   out[(b, y, x), off_i + j] = sum_q U_i[(y, x), q] (x_i W_i^T)[(b, q), j]       k_df_fwd
//   mtlora_decoder_front_bwd   gz_i = U_i^T dout_i,  dx_i = gz_i W_i,  dW_i = gz_i^T x_i                      k_df_bwd, k_df_dw, k_df_dw_finish
//
// Convolution and interpolation commute, so every stage is projected at ITS resolution and interpolated on chip: the coarse maps are
// never rounded to 16 bits and never reach memory.  Scales are powers of two up to 8: the source index (o + 0.5) / s - 0.5 of
// upsample.hip is then exact in fp32, on the host and on the device alike, which is what the LDS images are sized by.
//
//   forward   one workgroup (4 waves) per (image, band of R fine rows).  The coarse rows a band taps are iy0(y0) .. iy1(y1 - 1) per stage:
//             its own rows plus a halo of at most one row on either side, clamped at the image border, never crossing it.  The tokens
//             of those rows are ONE contiguous run of the stage's token matrix, so the A operand of the MFMA (32 pixels x 16 k) is a
//             16-byte global load per lane and k-step, and the B operand the fp32 master W_i (32 channels x 16 k, two 16-byte loads
//             rounded to the compute dtype in registers): no operand goes through LDS, stage 0 included.  A wave takes the work items
//             (stage, 32-channel tile, group of DF_RT pixel tiles) round-robin -- at the Swin-T geometry 11 items of 84 to 96 MFMAs
//             for R = 4 -- and leaves the fp32 accumulators in the stage's LDS image [pixel][c_i rounded up to 4].  After one barrier
//             the workgroup walks its fine pixels: a thread forms 8 consecutive output columns (two 4-channel groups, each inside
//             one slice because slices start at multiples of 4; four taps of 16-byte LDS reads each, the weights in the order of
//             k_up_fwd) and writes them as one 16-byte store: complete rows, the +0 pad columns included.
//   backward  k_df_bwd, one workgroup per (image, band of Rb fine rows, Rb a multiple of the largest scale): it OWNS the coarse rows
//             y0 / s_i .. y1 / s_i of every stage.  gz_i is the gather of k_up_bwd over the <= 2 s_i fine rows and columns that tap a
//             coarse pixel, read from dout with a halo inside the image, summed in fp32 in a fixed order, and stored in LDS as the
//             16-bit pair hi = round(gz), lo = round(gz - hi): dx_i = gz_i W_i is then two MFMAs per k-step on one-load operands and
//             carries gz to 2^-17 (a single rounding of gz would dominate the error of dx wherever its terms cancel).  The B
//             operand W_i^T is 8 coalesced 4-byte loads per lane and k-step (lanes along C_i).  hi is also written to `scratch`
//             (stages >= 1; stage 0's gz IS its slice of dout) for
//             k_df_dw, one split-M "TN" launch over all stages: item (stage, 128-column panel of x_i, row split); 32-row chunks
//             of gz and x go through LDS and come back transposed (tn_frag16 of tn.h), 4 waves x up to 5 accumulators; every item
//             writes its partial c_i x 128 panel, and k_df_dw_finish adds the splits of each element in index order.
// No atomics, no memset, no allocation; every output element is written by exactly one lane: bit-reproducible and capturable.
#include "dispatch.h"
#include "tn.h"

namespace {

constexpr int DF_MAXS = MTLORA_DF_MAX_STAGES;
constexpr int DF_THREADS = 256;
constexpr int DF_WAVES = DF_THREADS / 64;
constexpr int DF_MAX_C = 160;             // widest projection: DF_CT column tiles of 32
constexpr int DF_CT = DF_MAX_C / 32;
constexpr int DF_MAX_SCALE = 8;
constexpr int DF_RT = 4;                  // pixel tiles of 32 a wave accumulates per work item
constexpr int DF_LDS_MAX = 96 * 1024;
constexpr int DF_DW_ROWS = 768;           // rows per split of k_df_dw aimed at
constexpr int DF_DW_LR = 320;             // LDS row bytes of its chunks: 16 dwords (mod 64), as k_tn
constexpr int DF_DW_KE = 32;              // rows per chunk = one transposed fragment

struct DfStage {
    const void* x;
    const float* W;
    void* dx;
    float* dW;
    void* gz;      // backward: round(gz) of the stage in scratch (k_df_dw's A operand; stage 0: its slice of dout)
    float* part;   // backward: nsplit partial (c x C) matrices
    int64_t lda;   // elements per row of gz
    int h, w, C, c, s, off;
    int pitch;     // forward: floats per pixel of the LDS image (c rounded up to 4); backward: bytes per pixel of the hi / lo images
    int lds_off;   // bytes
    int img;       // backward: bytes of one of the two images
    int nsplit, rps, npanel, item0;  // k_df_dw
};
struct DfParams {
    DfStage st[DF_MAXS];
    const void* dout;
    void* out;
    int64_t B;
    int n, H, W, ld, band, nbands, want_x, want_w, n_items, dw_total;
};

__host__ __device__ __forceinline__ int df_pad(int v, int m) { return (v + m - 1) / m * m; }
// upsample.hip's source index; exact for the power-of-two scales this file takes
__host__ __device__ __forceinline__ void df_src_index(int o, float rs, int n_in, int& i0, int& i1, float& f) {
    float s = ((float)o + 0.5f) * rs - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = (int)s;
    i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    f = s - (float)i0;
}
// the coarse rows lo .. hi of a stage that the fine rows y0 .. y1 - 1 tap
__host__ __device__ __forceinline__ void df_rows(int y0, int y1, int s, int h, int& lo, int& hi) {
    int a, b;
    float f;
    df_src_index(y0, 1.f / (float)s, h, lo, a, f);
    df_src_index(y1 - 1, 1.f / (float)s, h, b, hi, f);
}

template <typename T>
__device__ __forceinline__ void df_mma(const u32x4& a, const u32x4& b, f32x16& c) {  // one 16-deep k-step: D[i][j] += A[i][k] B[j][k]
    if constexpr (__is_same(T, f16))
        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
template <typename T>
__device__ __forceinline__ f32x4 df_ld4(const T* q) {  // four 16-bit elements, 8-byte aligned
    const u32x2 v = *reinterpret_cast<const u32x2*>(q);
    return f32x4{mtl_lo2<T>(v[0]), mtl_hi2<T>(v[0]), mtl_lo2<T>(v[1]), mtl_hi2<T>(v[1])};
}
template <typename T>
__device__ __forceinline__ uint16_t df_bits(float v) {
    return __builtin_bit_cast(uint16_t, mtl_from_f32<T>(v));
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
// the 4 channels cc .. cc + 3 of stage S at fine pixel (y, x) from the stage's LDS image, whose first row is coarse row lo
__device__ __forceinline__ f32x4 df_tap(const float* img, const DfStage& S, int lo, int y, int x, int cc) {
    if (S.s == 1) return *reinterpret_cast<const f32x4*>(img + ((y - lo) * S.w + x) * S.pitch + cc);
    const float rs = 1.f / (float)S.s;
    int iy0, iy1, ix0, ix1;
    float fy, fx;
    df_src_index(y, rs, S.h, iy0, iy1, fy);
    df_src_index(x, rs, S.w, ix0, ix1, fx);
    const float* r0 = img + (iy0 - lo) * S.w * S.pitch + cc;
    const float* r1 = img + (iy1 - lo) * S.w * S.pitch + cc;
    const f32x4 a = *reinterpret_cast<const f32x4*>(r0 + ix0 * S.pitch), bq = *reinterpret_cast<const f32x4*>(r0 + ix1 * S.pitch);
    const f32x4 c = *reinterpret_cast<const f32x4*>(r1 + ix0 * S.pitch), d = *reinterpret_cast<const f32x4*>(r1 + ix1 * S.pitch);
    const float w00 = (1.f - fy) * (1.f - fx), w01 = (1.f - fy) * fx, w10 = fy * (1.f - fx), w11 = fy * fx;
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = w00 * a[e] + w01 * bq[e] + w10 * c[e] + w11 * d[e];
    return o;
}

template <typename T>
__global__ __launch_bounds__(DF_THREADS) void k_df_fwd(const DfParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char df_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, hh = lane >> 5;
    const int b = blockIdx.x / p.nbands, band = blockIdx.x - b * p.nbands;
    const int y0 = band * p.band, y1 = y0 + p.band < p.H ? y0 + p.band : p.H;

    // the projections of the band's coarse rows: fp32 accumulators -> the stages' LDS images
    int it = 0;
    for (int i = 0; i < p.n; ++i) {
        const DfStage& S = p.st[i];
        int lo, hi;
        df_rows(y0, y1, S.s, S.h, lo, hi);
        const int P = (hi - lo + 1) * S.w;                         // pixels: one contiguous run of tokens
        const int64_t tok0 = ((int64_t)b * S.h + lo) * S.w;
        const int nct = (S.c + 31) >> 5, nrt = (P + 31) >> 5, ks = S.C >> 4;
        float* img = reinterpret_cast<float*>(df_lds + S.lds_off);
        for (int ct = 0; ct < nct; ++ct)
            for (int r0 = 0; r0 < nrt; r0 += DF_RT, ++it) {
                if ((it & (DF_WAVES - 1)) != wave) continue;
                const int ch = 32 * ct + li;
                const bool ch_in = ch < S.c;
                const float* wq = S.W + (int64_t)(ch_in ? ch : 0) * S.C + 8 * hh;
                const T* xq[DF_RT];
                bool in[DF_RT];
                f32x16 acc[DF_RT];
#pragma unroll
                for (int rt = 0; rt < DF_RT; ++rt) {
                    const int pp = 32 * (r0 + rt) + li;
                    in[rt] = pp < P;
                    xq[rt] = reinterpret_cast<const T*>(S.x) + (tok0 + (in[rt] ? pp : 0)) * S.C + 8 * hh;
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[rt][r] = 0.f;
                }
                for (int s = 0; s < ks; ++s) {
                    u32x4 bw = {0u, 0u, 0u, 0u};
                    if (ch_in) {
                        const f32x4 w0 = *reinterpret_cast<const f32x4*>(wq + 16 * s), w1 = *reinterpret_cast<const f32x4*>(wq + 16 * s + 4);
                        bw = u32x4{mtl_pk2<T>(w0[0], w0[1]), mtl_pk2<T>(w0[2], w0[3]), mtl_pk2<T>(w1[0], w1[1]), mtl_pk2<T>(w1[2], w1[3])};
                    }
#pragma unroll
                    for (int rt = 0; rt < DF_RT; ++rt) {
                        if (32 * (r0 + rt) >= P) continue;  // (wave-uniform)
                        const u32x4 a = in[rt] ? *reinterpret_cast<const u32x4*>(xq[rt] + 16 * s) : u32x4{0u, 0u, 0u, 0u};
                        df_mma<T>(a, bw, acc[rt]);
                    }
                }
                // register r of tile rt: pixel 32 (r0 + rt) + mtl_d_row, channel ch; channels c .. pitch - 1 are +0 (zero operands)
                if (ch < S.pitch) {
#pragma unroll
                    for (int rt = 0; rt < DF_RT; ++rt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int pp = 32 * (r0 + rt) + mtl_d_row(lane, r);
                            if (pp < P) img[pp * S.pitch + ch] = acc[rt][r];
                        }
                }
            }
    }
    __syncthreads();

    // the fine pixels: 8 output columns per thread and step, complete rows
    const int nv = p.ld >> 3, total = (y1 - y0) * p.W * nv;
    int lo_s[DF_MAXS];  // first coarse row of each stage's image
#pragma unroll
    for (int i = 0; i < DF_MAXS; ++i) {
        int hi;
        lo_s[i] = 0;
        if (i < p.n) df_rows(y0, y1, p.st[i].s, p.st[i].h, lo_s[i], hi);
    }
    T* out = reinterpret_cast<T*>(p.out) + ((int64_t)b * p.H + y0) * p.W * p.ld;
    for (int e = tid; e < total; e += DF_THREADS) {
        const int px = e / nv, v = e - px * nv;
        const int yy = px / p.W, x = px - yy * p.W, y = y0 + yy;
        uint32_t o[4];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int col = 8 * v + 4 * half;
            f32x4 val = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < DF_MAXS; ++i) {
                if (i >= p.n) continue;
                const DfStage& S = p.st[i];
                const int cc = col - S.off;
                if (cc >= 0 && cc < S.pitch) val = df_tap(reinterpret_cast<const float*>(df_lds + S.lds_off), S, lo_s[i], y, x, cc);
            }
            o[2 * half] = mtl_pk2<T>(val[0], val[1]);
            o[2 * half + 1] = mtl_pk2<T>(val[2], val[3]);
        }
        *reinterpret_cast<u32x4*>(out + (int64_t)px * p.ld + 8 * v) = u32x4{o[0], o[1], o[2], o[3]};
    }
}

// ------------------------------------------------------------------------------------------------
// backward: gz on chip, dx, round(gz) to scratch
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(DF_THREADS) void k_df_bwd(const DfParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char df_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, hh = lane >> 5;
    const int b = blockIdx.x / p.nbands, band = blockIdx.x - b * p.nbands;
    const int y0 = band * p.band, y1 = y0 + p.band < p.H ? y0 + p.band : p.H;  // multiples of every scale
    const T* g = reinterpret_cast<const T*>(p.dout) + (int64_t)b * p.H * p.W * p.ld;

    // gz of the owned coarse pixels, 4 channels per thread and step (the gather of k_up_bwd), as the pair hi + lo
    for (int i = 0; i < p.n; ++i) {
        const DfStage& S = p.st[i];
        const int sc = S.s, q0 = y0 / sc, P = (y1 - y0) / sc * S.w, ng = (S.pitch - 16) >> 3;  // 4-channel groups of the padded k range
        const float rs = 1.f / (float)sc;
        unsigned char* hi_img = df_lds + S.lds_off;
        for (int e = tid; e < P * ng; e += DF_THREADS) {
            const int pp = e / ng, gq = e - pp * ng;
            const int qyl = pp / S.w, qx = pp - qyl * S.w, qy = q0 + qyl;
            const int nvalid = S.c - 4 * gq;  // channels of the group inside the slice
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            if (nvalid > 0) {
                const T* gs = g + S.off + 4 * gq;
                if (sc == 1) {
                    acc = df_ld4<T>(gs + ((int64_t)qy * p.W + qx) * p.ld);
                } else {
                    const int hs1 = (sc + 1) / 2 + 1;
                    const int oy_lo = sc * qy - hs1 < 0 ? 0 : sc * qy - hs1, oy_hi = sc * qy - hs1 + 2 * sc + 2 > p.H ? p.H : sc * qy - hs1 + 2 * sc + 2;
                    const int ox_lo = sc * qx - hs1 < 0 ? 0 : sc * qx - hs1, ox_hi = sc * qx - hs1 + 2 * sc + 2 > p.W ? p.W : sc * qx - hs1 + 2 * sc + 2;
                    for (int oy = oy_lo; oy < oy_hi; ++oy) {
                        int iy0, iy1;
                        float fy;
                        df_src_index(oy, rs, S.h, iy0, iy1, fy);
                        const float wy = (iy0 == qy ? 1.f - fy : 0.f) + (iy1 == qy ? fy : 0.f);
                        if (wy == 0.f) continue;
                        const T* row = gs + (int64_t)oy * p.W * p.ld;
                        for (int ox = ox_lo; ox < ox_hi; ++ox) {
                            int ix0, ix1;
                            float fx;
                            df_src_index(ox, rs, S.w, ix0, ix1, fx);
                            const float wq = wy * ((ix0 == qx ? 1.f - fx : 0.f) + (ix1 == qx ? fx : 0.f));
                            if (wq == 0.f) continue;
                            const f32x4 v = df_ld4<T>(row + (int64_t)ox * p.ld);
#pragma unroll
                            for (int k = 0; k < 4; ++k) acc[k] += wq * v[k];
                        }
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k >= nvalid) acc[k] = 0.f;  // pad columns of dout: ignored, whatever they hold
            }
            uint16_t hb[4], lb[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float hf = mtl_to_f32(mtl_from_f32<T>(acc[k]));
                hb[k] = df_bits<T>(acc[k]);
                lb[k] = (hf - hf == 0.f) ? df_bits<T>(acc[k] - hf) : (uint16_t)0;  // (a non-finite hi carries the value alone)
            }
            unsigned char* q = hi_img + pp * S.pitch + 8 * gq;
            *reinterpret_cast<u32x2*>(q) = u32x2{(uint32_t)hb[0] | (uint32_t)hb[1] << 16, (uint32_t)hb[2] | (uint32_t)hb[3] << 16};
            *reinterpret_cast<u32x2*>(q + S.img) = u32x2{(uint32_t)lb[0] | (uint32_t)lb[1] << 16, (uint32_t)lb[2] | (uint32_t)lb[3] << 16};
        }
    }
    __syncthreads();

    // round(gz) of stages >= 1 to scratch: rows of lda = c rounded up to 8 elements
    if (p.want_w) {
        for (int i = 1; i < p.n; ++i) {
            const DfStage& S = p.st[i];
            const int P = (y1 - y0) / S.s * S.w, nv = (int)(S.lda >> 3);
            T* gz = reinterpret_cast<T*>(S.gz) + (((int64_t)b * S.h + y0 / S.s) * S.w) * S.lda;
            for (int e = tid; e < P * nv; e += DF_THREADS) {
                const int pp = e / nv, v = e - pp * nv;
                *reinterpret_cast<u32x4*>(gz + (int64_t)pp * S.lda + 8 * v) = *reinterpret_cast<const u32x4*>(df_lds + S.lds_off + pp * S.pitch + 16 * v);
            }
        }
    }
    if (!p.want_x) return;

    // dx_i = (hi + lo) W_i: work items (stage, 32-column tile of C_i, group of DF_RT pixel tiles), round-robin over the waves
    int it = 0;
    for (int i = 0; i < p.n; ++i) {
        const DfStage& S = p.st[i];
        if (!S.dx) continue;
        const int P = (y1 - y0) / S.s * S.w;
        const int64_t tok0 = ((int64_t)b * S.h + y0 / S.s) * S.w;
        const int nct = (S.C + 31) >> 5, nrt = (P + 31) >> 5, ks = (S.pitch - 16) >> 5;
        const unsigned char* hi_img = df_lds + S.lds_off;
        for (int ct = 0; ct < nct; ++ct)
            for (int r0 = 0; r0 < nrt; r0 += DF_RT, ++it) {
                if ((it & (DF_WAVES - 1)) != wave) continue;
                const int col = 32 * ct + li;
                const bool col_in = col < S.C;
                const float* wq = S.W + (col_in ? col : 0);
                f32x16 acc[DF_RT];
                bool in[DF_RT];
#pragma unroll
                for (int rt = 0; rt < DF_RT; ++rt) {
                    in[rt] = 32 * (r0 + rt) + li < P;
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[rt][r] = 0.f;
                }
                for (int s = 0; s < ks; ++s) {
                    float wv[8];  // W_i^T: k = channel 16 s + 8 hh + e, row = column `col` of W_i
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int ch = 16 * s + 8 * hh + e;
                        wv[e] = (col_in && ch < S.c) ? wq[(int64_t)ch * S.C] : 0.f;
                    }
                    const u32x4 bw = {mtl_pk2<T>(wv[0], wv[1]), mtl_pk2<T>(wv[2], wv[3]), mtl_pk2<T>(wv[4], wv[5]), mtl_pk2<T>(wv[6], wv[7])};
#pragma unroll
                    for (int rt = 0; rt < DF_RT; ++rt) {
                        if (32 * (r0 + rt) >= P) continue;  // (wave-uniform)
                        const unsigned char* q = hi_img + (in[rt] ? 32 * (r0 + rt) + li : 0) * S.pitch + (16 * s + 8 * hh) * 2;
                        const u32x4 z = {0u, 0u, 0u, 0u};
                        const u32x4 ah = in[rt] ? *reinterpret_cast<const u32x4*>(q) : z, al = in[rt] ? *reinterpret_cast<const u32x4*>(q + S.img) : z;
                        df_mma<T>(ah, bw, acc[rt]);
                        df_mma<T>(al, bw, acc[rt]);
                    }
                }
                if (col_in) {
                    T* dx = reinterpret_cast<T*>(S.dx) + tok0 * S.C + col;
#pragma unroll
                    for (int rt = 0; rt < DF_RT; ++rt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int pp = 32 * (r0 + rt) + mtl_d_row(lane, r);
                            if (pp < P) dx[(int64_t)pp * S.C] = mtl_from_f32<T>(acc[rt][r]);
                        }
                }
            }
    }
}

// ------------------------------------------------------------------------------------------------
// backward: dW_i = gz_i^T x_i for all stages, split over rows
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(DF_THREADS) void k_df_dw(const DfParams p) {
    __shared__ __attribute__((aligned(16))) unsigned char sA[DF_DW_KE * DF_DW_LR], sB[DF_DW_KE * DF_DW_LR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int i = 0;
#pragma unroll
    for (int k = 1; k < DF_MAXS; ++k)
        if (k < p.n && (int)blockIdx.x >= p.st[k].item0) i = k;
    const DfStage& S = p.st[i];
    const int item = blockIdx.x - S.item0, nb = item / S.nsplit, sp = item - nb * S.nsplit;
    const int64_t M = p.B * S.h * S.w;
    const int64_t m_lo = (int64_t)sp * S.rps, m_hi = m_lo + S.rps < M ? m_lo + S.rps : M;
    const int nct = (S.c + 31) >> 5, nva = (S.c + 7) >> 3, nvz = 4 * nct;
    const bool wave_on = 128 * nb + 32 * wave < S.C;
    const T* A = reinterpret_cast<const T*>(S.gz);
    const T* X = reinterpret_cast<const T*>(S.x);
    f32x16 acc[DF_CT];
#pragma unroll
    for (int ct = 0; ct < DF_CT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;

    for (int64_t m0 = m_lo; m0 < m_hi; m0 += DF_DW_KE) {
        for (int v = tid; v < DF_DW_KE * nvz; v += DF_THREADS) {  // gz: columns at or past c are zeros
            const int row = v / nvz, vec = v - row * nvz;
            u32x4 a = {0u, 0u, 0u, 0u};
            if (vec < nva && m0 + row < m_hi) {
                a = *reinterpret_cast<const u32x4*>(A + (m0 + row) * S.lda + 8 * vec);
                const int nvalid = S.c - 8 * vec;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    if (2 * w >= nvalid) a[w] = 0u;
                    else if (2 * w + 1 >= nvalid) a[w] &= 0xFFFFu;
                }
            }
            *reinterpret_cast<u32x4*>(sA + row * DF_DW_LR + 16 * vec) = a;
        }
        for (int v = tid; v < DF_DW_KE * 16; v += DF_THREADS) {  // x: the panel's 128 columns
            const int row = v >> 4, vec = v & 15, col = 128 * nb + 8 * vec;
            u32x4 x = {0u, 0u, 0u, 0u};
            if (col < S.C && m0 + row < m_hi) x = *reinterpret_cast<const u32x4*>(X + (m0 + row) * S.C + col);
            *reinterpret_cast<u32x4*>(sB + row * DF_DW_LR + 16 * vec) = x;
        }
        __syncthreads();
        if (wave_on) {
            const Frag<T> fb = tn_frag16<T>(sB, 32 * wave, lane, DF_DW_LR);
#pragma unroll
            for (int ct = 0; ct < DF_CT; ++ct)
                if (ct < nct) mtl_mma(tn_frag16<T>(sA, 32 * ct, lane, DF_DW_LR), fb, acc[ct]);
        }
        __syncthreads();
    }
    if (!wave_on) return;
    const int col = 128 * nb + 32 * wave + mtl_d_col(lane);
    if (col >= S.C) return;
    float* part = S.part + (int64_t)sp * S.c * S.C + col;
#pragma unroll
    for (int ct = 0; ct < DF_CT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ch = 32 * ct + mtl_d_row(lane, r);
            if (ch < S.c) part[(int64_t)ch * S.C] = acc[ct][r];
        }
}

// element e of the concatenated dW_0 | dW_1 | ...: the sum of its splits in index order
__global__ __launch_bounds__(256) void k_df_dw_finish(const DfParams p) {
    int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= p.dw_total) return;
    int i = 0;
    for (; i < p.n - 1 && e >= p.st[i].c * p.st[i].C; ++i) e -= p.st[i].c * p.st[i].C;
    const DfStage& S = p.st[i];
    const int64_t per = (int64_t)S.c * S.C;
    float a = 0.f;
    for (int sp = 0; sp < S.nsplit; ++sp) a += S.part[sp * per + e];
    S.dW[e] = a;
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
int df_smax(const mtlora_decoder_front_desc* d) {
    int m = 1;
    for (int i = 0; i < d->n; ++i) m = d->s[i] > m ? d->s[i] : m;
    return m;
}
// LDS bytes of k_df_fwd with bands of R fine rows; the stages' offsets into lds_off when given
int64_t df_fwd_lds(const mtlora_decoder_front_desc* d, int R, int* lds_off) {
    const int H = d->h[0];
    int64_t at = 0;
    for (int i = 0; i < d->n; ++i) {
        int rows = 0;
        for (int y0 = 0; y0 < H; y0 += R) {
            int lo, hi;
            df_rows(y0, y0 + R < H ? y0 + R : H, d->s[i], d->h[i], lo, hi);
            rows = hi - lo + 1 > rows ? hi - lo + 1 : rows;
        }
        if (lds_off) lds_off[i] = (int)at;
        at += (int64_t)rows * d->w[i] * df_pad(d->c[i], 4) * 4;
    }
    return at;
}
int df_bwd_pitch(int c) { return df_pad(c, 16) * 2 + 16; }  // bytes per pixel of a hi / lo image: an odd number of 16-byte vectors
int64_t df_bwd_lds(const mtlora_decoder_front_desc* d, int R, int* lds_off) {
    int64_t at = 0;
    for (int i = 0; i < d->n; ++i) {
        if (lds_off) lds_off[i] = (int)at;
        at += 2 * (int64_t)(R / d->s[i]) * d->w[i] * df_bwd_pitch(d->c[i]);
    }
    return at;
}
// the band heights: the one asked for (default 4 forward, 8 backward), lowered until the LDS images fit; 0: none fits
int df_fwd_band(const mtlora_decoder_front_desc* d) {
    int R = d->band_rows > 0 ? d->band_rows : 4;
    R = R > d->h[0] ? d->h[0] : R;
    R = R > 64 ? 64 : R;
    while (R > 1 && df_fwd_lds(d, R, nullptr) > DF_LDS_MAX) --R;
    return df_fwd_lds(d, R, nullptr) <= DF_LDS_MAX ? R : 0;
}
int df_bwd_band(const mtlora_decoder_front_desc* d) {
    const int sm = df_smax(d);
    int R = (int)mtl_round_up(d->band_rows > 0 ? d->band_rows : 8, sm);
    R = R > d->h[0] ? d->h[0] : R;  // (H is a multiple of every scale)
    R = R > 64 ? 64 / sm * sm : R;
    while (R > sm && df_bwd_lds(d, R, nullptr) > DF_LDS_MAX) R -= sm;
    return df_bwd_lds(d, R, nullptr) <= DF_LDS_MAX ? R : 0;
}

// MTLORA_OK when the kernels take the descriptor, else the status every entry returns for it
int df_check(const mtlora_decoder_front_desc* d) {
    if (!d) return MTLORA_ERR_NULL;
    if (!mtl_dtype_in(d->dtype, MTL_DT_ALL)) return MTLORA_ERR_DTYPE;
    if (d->B < 0 || d->n < 2 || d->grad_flags < 0 || d->grad_flags > 3 || d->band_rows < 0 || d->ld < 1) return MTLORA_ERR_SHAPE;
    if (d->n > DF_MAXS) return MTLORA_ERR_UNSUPPORTED;
    for (int i = 0; i < d->n; ++i) {
        if (d->h[i] < 1 || d->w[i] < 1 || d->C[i] < 1 || d->c[i] < 1 || d->s[i] < 1 || d->off[i] < 0) return MTLORA_ERR_SHAPE;
        if ((int64_t)d->s[i] * d->h[i] != (int64_t)d->s[0] * d->h[0] || (int64_t)d->s[i] * d->w[i] != (int64_t)d->s[0] * d->w[0]) return MTLORA_ERR_SHAPE;
    }
    if (d->dtype == MTLORA_F32 || d->s[0] != 1) return MTLORA_ERR_UNSUPPORTED;
    int at = 0;
    for (int i = 0; i < d->n; ++i) {
        const int s = d->s[i];
        if (d->C[i] % 16 || (i && d->c[i] % 4) || d->c[i] > DF_MAX_C || s > DF_MAX_SCALE || (s & (s - 1)) || d->off[i] != at)
            return MTLORA_ERR_UNSUPPORTED;
        if ((int64_t)d->c[i] * d->C[i] >= ((int64_t)1 << 28)) return MTLORA_ERR_UNSUPPORTED;
        at += df_pad(d->c[i], 4);
    }
    if (d->ld != df_pad(at, 8)) return MTLORA_ERR_UNSUPPORTED;
    if (d->B * d->h[0] * (int64_t)d->w[0] >= ((int64_t)1 << 31)) return MTLORA_ERR_UNSUPPORTED;
    if (!df_fwd_band(d) || !df_bwd_band(d)) return MTLORA_ERR_UNSUPPORTED;
    return MTLORA_OK;
}

DfParams df_params(const mtlora_decoder_front_desc* d, const void* const* x, const float* const* W) {
    DfParams p = {};
    p.B = d->B;
    p.n = d->n;
    p.H = d->h[0];
    p.W = d->w[0];
    p.ld = d->ld;
    for (int i = 0; i < d->n; ++i) {
        DfStage& S = p.st[i];
        S.x = x[i];
        S.W = W[i];
        S.h = d->h[i];
        S.w = d->w[i];
        S.C = d->C[i];
        S.c = d->c[i];
        S.s = d->s[i];
        S.off = d->off[i];
    }
    return p;
}

// the row splits of k_df_dw and the scratch layout -- round(gz) of stages >= 1, then the partials -- into p (the parameter block of a
// launch, or a throw-away one for the size query); returns the bytes
int64_t df_plan_dw(const mtlora_decoder_front_desc* d, DfParams& p, unsigned char* scratch) {
    int64_t at = 0;
    p.n_items = p.dw_total = 0;
    for (int i = 0; i < d->n; ++i) {
        DfStage& S = p.st[i];
        const int64_t M = d->B * d->h[i] * d->w[i];
        int64_t ns = mtl_ceil_div(M, DF_DW_ROWS);
        ns = ns < 1 ? 1 : ns > 256 ? 256 : ns;
        S.rps = (int)mtl_round_up(mtl_ceil_div(M, ns), DF_DW_KE);
        S.nsplit = (int)mtl_ceil_div(M, S.rps);
        S.npanel = (d->C[i] + 127) / 128;
        S.item0 = p.n_items;
        S.lda = i ? df_pad(d->c[i], 8) : d->ld;
        S.gz = i && scratch ? scratch + at : nullptr;  // (stage 0: the caller points it at dout)
        if (i) at += mtl_round_up(M * S.lda * 2, 256);
        p.n_items += S.npanel * S.nsplit;
        p.dw_total += d->c[i] * d->C[i];
    }
    for (int i = 0; i < d->n; ++i) {
        p.st[i].part = scratch ? reinterpret_cast<float*>(scratch + at) : nullptr;
        at += mtl_round_up((int64_t)p.st[i].nsplit * d->c[i] * d->C[i] * 4, 256);
    }
    return at;
}

double df_bytes(const mtlora_decoder_front_desc* d) {
    double by = (double)d->B * d->h[0] * d->w[0] * d->ld * 2;
    for (int i = 0; i < d->n; ++i) by += (double)d->B * d->h[i] * d->w[i] * d->C[i] * 2;
    return by;
}

template <typename K>
void df_launch(K fn, int64_t grid, int lds, const DfParams& p, hipStream_t s) {
    if (lds > 48 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(DF_THREADS), lds, s, p);
}

}  // namespace

extern "C" {

int mtlora_decoder_front_supported(const mtlora_decoder_front_desc* d) { return df_check(d) == MTLORA_OK ? 1 : 0; }

int mtlora_decoder_front_fwd(const mtlora_decoder_front_desc* d, const void* const* x, const float* const* W, void* out, void* stream) {
    const int st = df_check(d);
    if (st != MTLORA_OK) return st;
    if (d->B == 0) return MTLORA_OK;
    if (mtl_any_null({out}, d->n, {x, mtl_arr(W)})) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({out}, d->n, {x, mtl_arr(W)})) return MTLORA_ERR_ALIGN;
    DfParams p = df_params(d, x, W);
    p.out = out;
    p.band = df_fwd_band(d);
    p.nbands = (int)mtl_ceil_div(p.H, p.band);
    int off[DF_MAXS];
    const int lds = (int)df_fwd_lds(d, p.band, off);
    for (int i = 0; i < d->n; ++i) {
        p.st[i].lds_off = off[i];
        p.st[i].pitch = df_pad(d->c[i], 4);
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    MtlProfScope prof(PK_UPSAMPLE, df_bytes(d), s);
    mtl_dispatch_dtype16(d->dtype, [&](auto tt) { df_launch(k_df_fwd<typename decltype(tt)::type>, d->B * p.nbands, lds, p, s); });
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

int64_t mtlora_decoder_front_bwd_scratch_bytes(const mtlora_decoder_front_desc* d) {
    if (df_check(d) != MTLORA_OK) return -1;
    DfParams p = {};
    const int64_t by = df_plan_dw(d, p, nullptr);
    return by < 16 ? 16 : by;
}

int mtlora_decoder_front_bwd(const mtlora_decoder_front_desc* d, const void* const* x, const float* const* W, const void* dout,
                             void* const* dx, float* const* dW, void* scratch, int64_t scratch_bytes, void* stream) {
    const int st = df_check(d);
    if (st != MTLORA_OK) return st;
    const bool want_w = d->grad_flags & MTLORA_DF_GRAD_W;
    bool want_x = false;
    if ((d->grad_flags & MTLORA_DF_GRAD_X) && dx)
        for (int i = 0; i < d->n; ++i) want_x = want_x || dx[i];
    if (d->B == 0 || !(want_x || want_w)) return MTLORA_OK;
    if (mtl_any_null({dout}, d->n, {x, mtl_arr(W)}) || (want_w && (mtl_any_null({scratch}, d->n, {mtl_arr(dW)})))) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({dout, scratch}, d->n, {x, mtl_arr(W), want_x ? mtl_arr(dx) : nullptr, want_w ? mtl_arr(dW) : nullptr}))
        return MTLORA_ERR_ALIGN;
    if (want_w && scratch_bytes < mtlora_decoder_front_bwd_scratch_bytes(d)) return MTLORA_ERR_WORKSPACE;
    DfParams p = df_params(d, x, W);
    p.dout = dout;
    p.want_x = want_x;
    p.want_w = want_w;
    p.band = df_bwd_band(d);
    p.nbands = (int)mtl_ceil_div(p.H, p.band);
    int off[DF_MAXS];
    const int lds = (int)df_bwd_lds(d, p.band, off);
    for (int i = 0; i < d->n; ++i) {
        DfStage& S = p.st[i];
        S.lds_off = off[i];
        S.pitch = df_bwd_pitch(d->c[i]);
        S.img = p.band / d->s[i] * d->w[i] * S.pitch;
        S.dx = want_x ? dx[i] : nullptr;
        S.dW = want_w ? dW[i] : nullptr;
    }
    if (want_w) {
        df_plan_dw(d, p, reinterpret_cast<unsigned char*>(scratch));
        p.st[0].gz = const_cast<void*>(dout);  // (off[0] is 0: stage 0's gz is the leading columns of dout)
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    MtlProfScope prof(PK_UPSAMPLE, df_bytes(d), s);
    mtl_dispatch_dtype16(d->dtype, [&](auto tt) { df_launch(k_df_bwd<typename decltype(tt)::type>, d->B * p.nbands, lds, p, s); });
    MTL_CHECK_LAUNCH();
    if (want_w) {
        mtl_dispatch_dtype16(d->dtype, [&](auto tt) { df_launch(k_df_dw<typename decltype(tt)::type>, p.n_items, 0, p, s); });
        MTL_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_df_dw_finish, dim3((unsigned)mtl_ceil_div(p.dw_total, 256)), dim3(256), 0, s, p);
        MTL_CHECK_LAUNCH();
    }
    return MTLORA_OK;
}

}  // extern "C"
