// predict.hip -- the predictions themselves (reference evaluation/evaluate_utils.py:20-38 get_output on the final F.interpolate
// of models/swin_mtl.py:245, what utils.py:405-439 save_imgs_mtl writes out), fused: the forward-only sibling of
// metrics.hip's k_up_metrics that STORES the processed pixel instead of counting it.  One pass over the LOW-resolution
// channels-last head output (B, h, w, C); every output pixel's C bilinear values are rebuilt in registers and only the processed
// prediction -- a class id, a [0, 255] image, the depth -- is written.  The (B, C, S*h, S*w) logits never exist.
//
// Tiling, staging and interpolation are k_up_metrics': one WAVE (a 64-thread workgroup) per tile of TQ x TR low-resolution
// pixels, TQ = 64 / S, lane = output column, the wave walks the TR S output rows; the (TR + 2) x (TQ + 2) neighbourhood is staged
// once as fp32 in LDS, the x-interpolated pair of a source cell stays in registers across the S rows of the cell, no workgroup
// barrier.  Index / weight arithmetic is PyTorch's (align_corners=False: src = max((dst + 0.5) * in/out - 0.5, 0),
// i1 = i0 + (i0 < in - 1), the formula of up_pixel.h's up_weight), per output pixel.  S <= 32.
//
// Precision.  The argmax kind evaluates the weights and the blend in fp32, operation for operation as k_up_metrics: the class id
// is the one the validation counters saw.  The kinds that store VALUES (C <= 4) evaluate the same formulas in fp64 and round the
// interpolated value to fp32 once; what follows (normalise, sigmoid) is fp32.  A stored value is held to 16 fp32 ulps of 255
// against an fp64 F.interpolate, and fp32 does not get there: at a scale that is no power of two the fp32 source index carries
// 1e-6 at column 80, times the difference of two logits, times the sigmoid's slope of 64 (3.4e-4 measured at scale 3), and a
// normal of small norm magnifies the blend's own rounding (3.3e-3 at scale 3, 2.5e-4 at scale 8).  At a power-of-two scale the
// weights are exact in either precision.  The kernel is store-bound; the fp64 blend of at most 4 channels is not what it waits for.
//
// Stores: the kernel is store-bound (21 classes: 0.2 MB read and 0.2 MB written per image), and a row of a tile is at most
// 64 pixels -- as uint8 one byte per lane.  So no result leaves from the lane that computed it: the wave collects NR rows of its
// tile in an LDS image whose rows sit at the SAME offset modulo 16 as their global addresses, then walks the image in 16-byte
// chunks, one chunk per lane: a chunk that lies inside the row is one 16-byte store, the (at most two) chunks at a row's
// unaligned ends are stored element by element.  Every element of the output is written exactly once, by exactly one lane;
// nothing outside it is written.  No atomics, no memset, no inline assembly.
//
//   kind 0  argmax     index of the FIRST maximum over C <= 48 (torch.max(dim)[1]); uint8 (B, H, W)
//   kind 1  normals    (up / max(|up|, 1e-12) + 1) * 255 / 2 (F.normalize's form), C <= 4; fp32 or uint8 (B, H, W, C)
//   kind 2  sigmoid    255 / (1 + exp(-up)), C = 1; fp32 or uint8 (B, H, W)
//   kind 3  identity   up, C = 1; fp32 (B, H, W, 1)
// uint8 is the fp32 value truncated, as tensor.to(torch.uint8) does for values in [0, 255].
#include "dispatch.h"

namespace {

struct UpPredParams {
    const void* low;     // (B, h, w, C)
    unsigned char* out;  // (B, H, W[, C])
    int B, h, w, C, S, TR;
    int NR, RS;          // rows and row stride (bytes, a multiple of 16) of the LDS output image
    int tiles;
};

constexpr int PRED_IMG_BYTES = 4096;  // the output image: small, so that many waves per CU keep stores in flight

// bytes of the widest row of a tile in the image: 64 / S * S pixels, shifted by up to 15 bytes, in whole 16-byte chunks
static inline int pred_row_stride(int S, int px_bytes) { return ((64 / S) * S * px_bytes + 15 + 15) & ~15; }
static __host__ __device__ inline int pred_stage_bytes(int C, int S, int TR) {
    return ((TR + 2) * (64 / S + 2) * (C | 1) * (int)sizeof(float) + 15) & ~15;
}
static inline int pred_nr(int S, int TR, int rs) {
    const int nr = PRED_IMG_BYTES / rs < 1 ? 1 : PRED_IMG_BYTES / rs;
    return nr < TR * S ? nr : TR * S;
}
static inline size_t pred_lds_bytes(int C, int S, int TR, int px_bytes) {
    const int rs = pred_row_stride(S, px_bytes);
    return (size_t)pred_stage_bytes(C, S, TR) + (size_t)pred_nr(S, TR, rs) * rs;
}
// low-res rows per tile: 4 as k_up_metrics, fewer where the staged neighbourhood would not fit (scale 1 with many classes)
static inline int pred_tr(int C, int S, int px_bytes) {
    int tr = 4;
    while (tr > 1 && pred_lds_bytes(C, S, tr, px_bytes) > 48 * 1024) tr >>= 1;
    return tr;
}

template <int PK>
struct PredAcc {  // the type the weights and the blend are evaluated in
    typedef double type;
};
template <>
struct PredAcc<0> {
    typedef float type;
};

__device__ __forceinline__ void pred_put(unsigned char* at, float v, float*) { *reinterpret_cast<float*>(at) = v; }
__device__ __forceinline__ void pred_put(unsigned char* at, float v, unsigned char*) { *at = (unsigned char)(unsigned int)v; }

template <typename T, int PK, int CMAX, int SC, typename OT>
__global__ __launch_bounds__(64) void k_up_predict(const UpPredParams p) {
    extern __shared__ float sm[];
    const int lane = threadIdx.x;
    const int S = SC ? SC : p.S;
    const int TR = p.TR, TQ = 64 / S;
    const int tiles_x = (p.w + TQ - 1) / TQ, tiles_y = (p.h + TR - 1) / TR;
    const int b = blockIdx.x / (tiles_x * tiles_y);
    const int trem = blockIdx.x % (tiles_x * tiles_y);
    const int qy0 = (trem / tiles_x) * TR, qx0 = (trem % tiles_x) * TQ;
    const int C = p.C, Cs = C | 1;
    const int RP = (TQ + 2) * Cs;
    const int H = p.h * S, W = p.w * S;
    float* lowt = sm;                                                                       // [TR + 2][TQ + 2][Cs]
    unsigned char* img = reinterpret_cast<unsigned char*>(sm) + pred_stage_bytes(C, S, TR);  // [NR][RS]
    const T* low = reinterpret_cast<const T*>(p.low);
    typedef typename PredAcc<PK>::type AT;
    const AT rs = (AT)p.h / (AT)H;  // in / out: 1/S rounded once (PyTorch's 1 / scale_factor)

    for (int i = lane; i < (TR + 2) * (TQ + 2) * C; i += 64) {
        const int pix = i / C, c = i - pix * C;
        const int py = pix / (TQ + 2), px = pix - py * (TQ + 2);
        int gy = qy0 - 1 + py, gx = qx0 - 1 + px;
        gy = gy < 0 ? 0 : (gy > p.h - 1 ? p.h - 1 : gy);
        gx = gx < 0 ? 0 : (gx > p.w - 1 ? p.w - 1 : gx);
        lowt[py * RP + px * Cs + c] = mtl_to_f32(low[(((int64_t)b * p.h + gy) * p.w + gx) * C + c]);
    }

    // this lane's output column
    const int ox0 = S * qx0;
    const int ncols = TQ * S < W - ox0 ? TQ * S : W - ox0;  // columns of this tile (wave-uniform)
    const bool col_ok = lane < ncols;
    const int oxc = col_ok ? ox0 + lane : W - 1;
    AT sx = ((AT)oxc + (AT)0.5) * rs - (AT)0.5;
    sx = sx < (AT)0 ? (AT)0 : sx;
    const int ix0 = (int)sx, ix1 = ix0 + (ix0 < p.w - 1 ? 1 : 0);
    const AT fx = sx - (AT)ix0;
    int lx0 = ix0 - qx0 + 1, lx1 = ix1 - qx0 + 1;
    lx0 = lx0 < 0 ? 0 : (lx0 > TQ + 1 ? TQ + 1 : lx0);
    lx1 = lx1 < 0 ? 0 : (lx1 > TQ + 1 ? TQ + 1 : lx1);
    const int oy_lo = S * qy0;
    const int oy_hi = S * (qy0 + TR) > H ? H : S * (qy0 + TR);
    const int PB = (int)sizeof(OT) * (PK == 1 ? C : 1);  // bytes of an output pixel
    const int nb = ncols * PB;                           // bytes of an output row of this tile
    const int NR = p.NR, RS = p.RS, CH = RS >> 4;
    unsigned char* const gtile = p.out + (((int64_t)b * H + oy_lo) * W + ox0) * PB;  // first row of the tile in the output
    const int64_t grow = (int64_t)W * PB;

    AT v0[CMAX], v1[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) v0[c] = v1[c] = (AT)0;
    int cell = -1;
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();

    // the processed pixel (this lane's column, row oy) into the image at `at`
    auto pixel = [&](int oy, unsigned char* at) __attribute__((always_inline)) {
        AT sy = ((AT)oy + (AT)0.5) * rs - (AT)0.5;
        sy = sy < (AT)0 ? (AT)0 : sy;
        const int iy0 = (int)sy, iy1 = iy0 + (iy0 < p.h - 1 ? 1 : 0);
        const AT fy = sy - (AT)iy0;
        if (iy0 != cell) {  // (wave-uniform) next source cell
            cell = iy0;
            int ly0 = iy0 - qy0 + 1, ly1 = iy1 - qy0 + 1;
            ly0 = ly0 < 0 ? 0 : (ly0 > TR + 1 ? TR + 1 : ly0);
            ly1 = ly1 < 0 ? 0 : (ly1 > TR + 1 ? TR + 1 : ly1);
            const float* r00 = lowt + ly0 * RP + lx0 * Cs;
            const float* r01 = lowt + ly0 * RP + lx1 * Cs;
            const float* r10 = lowt + ly1 * RP + lx0 * Cs;
            const float* r11 = lowt + ly1 * RP + lx1 * Cs;
#pragma unroll
            for (int c = 0; c < CMAX; ++c) {
                v0[c] = c < C ? ((AT)1 - fx) * (AT)r00[c] + fx * (AT)r01[c] : (AT)0;
                v1[c] = c < C ? ((AT)1 - fx) * (AT)r10[c] + fx * (AT)r11[c] : (AT)0;
            }
        }
        if (PK == 0) {
            int am = 0;
            float mv = (1.f - fy) * v0[0] + fy * v1[0];
#pragma unroll
            for (int c = 1; c < CMAX; ++c) {
                const float u = (1.f - fy) * v0[c] + fy * v1[c];
                if (c < C && u > mv) {
                    mv = u;
                    am = c;
                }
            }
            if (col_ok) *at = (unsigned char)am;
        } else if (PK == 1) {
            float up[CMAX];
            float r2 = 0.f;
#pragma unroll
            for (int c = 0; c < CMAX; ++c) {
                up[c] = (float)(((AT)1 - fy) * v0[c] + fy * v1[c]);
                r2 += up[c] * up[c];
            }
            const float den = fmaxf(sqrtf(r2), 1e-12f);
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (col_ok && c < C) pred_put(at + c * (int)sizeof(OT), (up[c] / den + 1.0f) * 255.f / 2.0f, (OT*)nullptr);
        } else {
            const float o = (float)(((AT)1 - fy) * v0[0] + fy * v1[0]);
            if (col_ok) pred_put(at, PK == 2 ? 255.f / (1.f + expf(-o)) : o, (OT*)nullptr);
        }
    };

    for (int ob = oy_lo; ob < oy_hi; ob += NR) {  // NR rows at a time through the image (all wave-uniform)
        const int nrow = oy_hi - ob < NR ? oy_hi - ob : NR;
        for (int r = 0; r < nrow; ++r) {
            const int sh = (int)(reinterpret_cast<uintptr_t>(gtile + (int64_t)(ob - oy_lo + r) * grow) & 15);
            pixel(ob + r, img + r * RS + sh + lane * PB);
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
        for (int i = lane; i < nrow * CH; i += 64) {
            const int r = i / CH, k16 = (i - r * CH) << 4;
            unsigned char* g = gtile + (int64_t)(ob - oy_lo + r) * grow;  // the row's first byte; its image is at [sh, sh + nb)
            const int sh = (int)(reinterpret_cast<uintptr_t>(g) & 15);
            const unsigned char* src = img + r * RS;
            g -= sh;
            const int lo = k16 > sh ? k16 : sh, hi = k16 + 16 < sh + nb ? k16 + 16 : sh + nb;
            if (hi - lo == 16) {
                *reinterpret_cast<u32x4*>(g + k16) = *reinterpret_cast<const u32x4*>(src + k16);
            } else {
                for (int j = lo; j < hi; j += (int)sizeof(OT)) *reinterpret_cast<OT*>(g + j) = *reinterpret_cast<const OT*>(src + j);
            }
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
    }
}

template <typename T, int PK, int CMAX, typename OT>
static void launch_pred(const UpPredParams& p, size_t lds, hipStream_t s) {
    if (p.S == 8)  // the scale of the models' heads
        hipLaunchKernelGGL((k_up_predict<T, PK, CMAX, 8, OT>), dim3((unsigned)p.tiles), dim3(64), lds, s, p);
    else
        hipLaunchKernelGGL((k_up_predict<T, PK, CMAX, 0, OT>), dim3((unsigned)p.tiles), dim3(64), lds, s, p);
}

template <typename T>
static void dispatch_pred(int kind, bool u8, const UpPredParams& p, size_t lds, hipStream_t s) {
    if (kind == 0) {
        if (p.C <= 8)
            launch_pred<T, 0, 8, unsigned char>(p, lds, s);
        else if (p.C <= 24)
            launch_pred<T, 0, 24, unsigned char>(p, lds, s);
        else
            launch_pred<T, 0, 48, unsigned char>(p, lds, s);
    } else if (kind == 1) {
        if (u8)
            launch_pred<T, 1, 4, unsigned char>(p, lds, s);
        else
            launch_pred<T, 1, 4, float>(p, lds, s);
    } else if (kind == 2) {
        if (u8)
            launch_pred<T, 2, 1, unsigned char>(p, lds, s);
        else
            launch_pred<T, 2, 1, float>(p, lds, s);
    } else {
        launch_pred<T, 3, 1, float>(p, lds, s);
    }
}

}  // namespace

extern "C" {

int mtlora_upsample_predict(int kind, const void* low, void* out, int64_t B, int h, int w, int C, int scale, int dtype, int out_dtype,
                            void* stream) {
    if (B < 0 || h <= 0 || w <= 0 || C <= 0) return MTLORA_ERR_SHAPE;
    if (kind < 0 || kind > 3 || scale < 1 || scale > 32) return MTLORA_ERR_UNSUPPORTED;
    if (kind == 0 ? C > 48 : kind == 1 ? C > 4 : C != 1) return MTLORA_ERR_UNSUPPORTED;
    const bool u8 = out_dtype == MTLORA_U8;
    if (!u8 && out_dtype != MTLORA_F32) return MTLORA_ERR_UNSUPPORTED;
    if ((kind == 0 && !u8) || (kind == 3 && u8)) return MTLORA_ERR_UNSUPPORTED;
    const int px_bytes = (u8 ? 1 : 4) * (kind == 1 ? C : 1);
    const int tr = pred_tr(C, scale, px_bytes);
    const size_t lds = pred_lds_bytes(C, scale, tr, px_bytes);
    if (lds > 64 * 1024) return MTLORA_ERR_UNSUPPORTED;
    if (!mtl_dtype_in(dtype, MTL_DT_ALL)) return MTLORA_ERR_DTYPE;
    if (B == 0) return MTLORA_OK;
    if (mtl_any_null({low, out})) return MTLORA_ERR_NULL;
    if (!u8 && mtl_any_misaligned({out}, 0, {}, 4)) return MTLORA_ERR_ALIGN;
    const int tq = 64 / scale;
    const int64_t tiles = B * (int64_t)((h + tr - 1) / tr) * ((w + tq - 1) / tq);
    if (tiles >= ((int64_t)1 << 31) || (int64_t)h * scale * (int64_t)w * scale >= ((int64_t)1 << 31)) return MTLORA_ERR_SHAPE;
    UpPredParams p;
    p.low = low;
    p.out = reinterpret_cast<unsigned char*>(out);
    p.B = (int)B;
    p.h = h;
    p.w = w;
    p.C = C;
    p.S = scale;
    p.TR = tr;
    p.RS = pred_row_stride(scale, px_bytes);
    p.NR = pred_nr(scale, tr, p.RS);
    p.tiles = (int)tiles;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    MtlProfScope prof(PK_UPSAMPLE, (double)B * h * w * C * mtl_elem_size(dtype) + (double)B * h * scale * w * scale * px_bytes, s);
    mtl_dispatch_dtype(dtype, [&](auto t) { dispatch_pred<typename decltype(t)::type>(kind, u8, p, lds, s); });
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

}  // extern "C"
