// augment.hip -- the geometric head of the reference's training pipeline on the device: ScaleNRotate (data/custom_transforms.py
// :24-88: cv2.getRotationMatrix2D about (w / 2, h / 2), cv2.warpAffine, the in-plane rotation of the normals :74-80, depth / sc
// :83-84) composed with FixedResize (:94-154: the resize to the training resolution and the renormalisation of the normals
// :144-150), as data/mtl_ds.py:846-859 chains them, for one batch of decoded, un-resampled samples stacked on a common canvas.
// In: uint8 HWC image, uint8 class / binary maps, fp32 HWC normals, fp32 depth, (B, Hc, Wc[, 3]) each, with the per-sample
// (h, w) in `size`.  Out: the same tensors at (Ho, Wo), the wire format mtlora_ingest_batch takes.  ONE resample where the
// reference has two (warp at source size, then resize): every output pixel is mapped back through both transforms at once.
// mtlora_amd/data.py:augment_batch_torch is the definition the tests hold this file to, bit for bit.
//
// Coordinates.  The host composes the two inverse maps in float64 (data.make_geometry) and hands over six integers per sample in
// Q24: the source coordinate of output pixel (u, v) is X = ax (2u + 1) + bx (2v + 1) + cx, Y likewise, evaluated in int64.
// Everything after that is integer too: nearest = (X + 2^23) >> 24 (round half up, arithmetic shift); cubic = (X + 2^18) >> 19,
// a coordinate in 1/32 pixel (cv2's INTER_BITS), integer part >> 5, fraction & 31.  A source pixel outside [0, w) x [0, h) of ITS
// sample is never read and counts as 0 (cv2's BORDER_CONSTANT 0); h and w are clamped to the canvas here, so no content of
// `size` or `geom` can make the kernel read outside the source tensors.
//
// Values.  IMAGE: 4 x 4 taps, Q15 weights (rows sum to 32768), horizontal sums in int32, the vertical sum in int64, then
// clamp((acc + 2^29) >> 30, 0, 255): exact.  NORMALS: the same taps in fp32, horizontal first (left to right), then vertical (top
// to bottom), every multiply and add rounded on its own (no contraction: the pragma below), then x' = x cos + y sin,
// y' = y cos - x sin with the fp32 (cos, sin) of the side table, then n / (sqrt(x^2 + y^2 + z^2) + 2^-52) with IEEE sqrt and
// division (a job flag skips this last step so that the stage before it can be tested for equality).  DEPTH: the nearest sample
// divided by the fp32 scale.  CLASS: the nearest sample.
//
// Work split.  One launch for all jobs (by value in the launch arguments, as the ingest's).  The output of a job is one flat HWC
// array; a wave owns AUG_PIX consecutive output pixels of it (a lane four adjacent ones), computes them into its own LDS image
// and then writes the image out in 16-byte chunks, lane k the chunk k: whole rows leave as contiguous 1 KiB wave stores whatever
// the pixel size (1, 3, 4 or 12 bytes), only the last chunk of a tensor can be partial.  The gathers have no reuse beyond the
// 4 x 4 footprint of neighbouring pixels: they go to global memory directly and the L1 / L2 absorb the overlap.  The two weight
// tables sit in LDS.  Every output element is written once, by one lane; plain vector stores, no atomics, no scratch, no
// inline assembly; deterministic.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int AUG_WAVES = 4;                     // waves of a workgroup
constexpr int AUG_PPL = 4;                       // adjacent output pixels of a lane
constexpr int AUG_PIX = MTL_WAVE * AUG_PPL;      // output pixels of a wave
constexpr int AUG_BLOCK_PIX = AUG_WAVES * AUG_PIX;
constexpr int AUG_Q = MTLORA_AUGMENT_GEOM_BITS;  // fraction bits of the geometry
constexpr float AUG_EPS = 2.220446049250313e-16f;  // 2^-52 (np.finfo(float).eps of FixedResize, an fp32 number too)

struct AugmentParams {
    mtlora_augment_job job[MTLORA_INGEST_MAX_JOBS];
    const int32_t* size;   // (B, 2): h, w
    const int64_t* geom;   // (B, 6): ax, bx, cx, ay, by, cy in Q24
    const float* side;     // (B, 3): cos, sin, sc
    const int32_t* cq;     // (32, 4) Q15
    const float* cf;       // (32, 4)
    int n_jobs, B, Hc, Wc, Ho, Wo, blocks_per_job;
};

struct AugSample {  // what a pixel needs of its sample
    int64_t ax, bx, cx, ay, by, cy;
    int h, w;
};

__device__ __forceinline__ AugSample aug_sample(const AugmentParams& p, int b) {
    AugSample s;
    const int64_t* g = p.geom + (int64_t)b * 6;
    s.ax = g[0], s.bx = g[1], s.cx = g[2], s.ay = g[3], s.by = g[4], s.cy = g[5];
    const int h = p.size[2 * b], w = p.size[2 * b + 1];
    s.h = h < 0 ? 0 : (h > p.Hc ? p.Hc : h);  // (whatever `size` holds, reads stay inside the canvas)
    s.w = w < 0 ? 0 : (w > p.Wc ? p.Wc : w);
    return s;
}

// a coordinate already shifted down, as an int that keeps "outside" outside: [-8, lim + 8] holds every tap decision
__device__ __forceinline__ int aug_narrow(int64_t v, int lim) {
    const int64_t lo = -8, hi = (int64_t)lim + 8;
    return (int)(v < lo ? lo : (v > hi ? hi : v));
}

// KIND-specific value of one output pixel (u, v) of sample b, written to the LDS image at `o`
template <int KIND>
__device__ __forceinline__ void aug_pixel(const AugmentParams& p, const mtlora_augment_job& J, const AugSample& s, int b, int u, int v,
                                          unsigned char* o, const int32_t* cq, const float* cf) {
    const int64_t X = s.ax * (int64_t)(2 * u + 1) + s.bx * (int64_t)(2 * v + 1) + s.cx;
    const int64_t Y = s.ay * (int64_t)(2 * u + 1) + s.by * (int64_t)(2 * v + 1) + s.cy;
    const int64_t base = (int64_t)b * p.Hc * p.Wc;  // first canvas pixel of the sample
    if (KIND == MTLORA_AUGMENT_CLASS_NEAREST_U8 || KIND == MTLORA_AUGMENT_DEPTH_NEAREST_F32) {
        const int x = aug_narrow((X + ((int64_t)1 << (AUG_Q - 1))) >> AUG_Q, s.w);
        const int y = aug_narrow((Y + ((int64_t)1 << (AUG_Q - 1))) >> AUG_Q, s.h);
        const bool in = x >= 0 && x < s.w && y >= 0 && y < s.h;
        const int64_t at = base + (int64_t)y * p.Wc + x;
        if (KIND == MTLORA_AUGMENT_CLASS_NEAREST_U8) {
            *o = in ? reinterpret_cast<const unsigned char*>(J.src)[at] : (unsigned char)0;
        } else {
            const float d = in ? reinterpret_cast<const float*>(J.src)[at] : 0.0f;
            *reinterpret_cast<float*>(o) = d / p.side[3 * b + 2];
        }
        return;
    }
    const int64_t X5 = (X + ((int64_t)1 << (AUG_Q - 6))) >> (AUG_Q - 5), Y5 = (Y + ((int64_t)1 << (AUG_Q - 6))) >> (AUG_Q - 5);
    const int fx = (int)(X5 & 31), fy = (int)(Y5 & 31);
    const int x0 = aug_narrow(X5 >> 5, s.w) - 1, y0 = aug_narrow(Y5 >> 5, s.h) - 1;  // the first tap
    if (KIND == MTLORA_AUGMENT_IMAGE_CUBIC_U8) {
        const unsigned char* src = reinterpret_cast<const unsigned char*>(J.src);
        const int wx[4] = {cq[4 * fx], cq[4 * fx + 1], cq[4 * fx + 2], cq[4 * fx + 3]};
        int64_t acc[3] = {0, 0, 0};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int y = y0 + r;
            const bool yin = y >= 0 && y < s.h;
            int hs[3] = {0, 0, 0};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int x = x0 + k;
                if (yin && x >= 0 && x < s.w) {
                    const unsigned char* q = src + (base + (int64_t)y * p.Wc + x) * 3;
                    hs[0] += wx[k] * (int)q[0];
                    hs[1] += wx[k] * (int)q[1];
                    hs[2] += wx[k] * (int)q[2];
                }
            }
            const int64_t wy = cq[4 * fy + r];
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += wy * (int64_t)hs[c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int64_t r = (acc[c] + ((int64_t)1 << 29)) >> 30;
            o[c] = (unsigned char)(r < 0 ? 0 : (r > 255 ? 255 : r));
        }
    } else {  // fp32 normals
        const float* src = reinterpret_cast<const float*>(J.src);
        const float wx[4] = {cf[4 * fx], cf[4 * fx + 1], cf[4 * fx + 2], cf[4 * fx + 3]};
        float n[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int y = y0 + r;
            const bool yin = y >= 0 && y < s.h;
            float hs[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int x = x0 + k;
                float t[3] = {0.0f, 0.0f, 0.0f};  // a tap outside the sample is 0 and is multiplied and added like any other
                if (yin && x >= 0 && x < s.w) {
                    const float* q = src + (base + (int64_t)y * p.Wc + x) * 3;
                    t[0] = q[0], t[1] = q[1], t[2] = q[2];
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float m = wx[k] * t[c];
                    hs[c] = k == 0 ? m : hs[c] + m;
                }
            }
            const float wy = cf[4 * fy + r];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float m = wy * hs[c];
                n[c] = r == 0 ? m : n[c] + m;
            }
        }
        const float cs = p.side[3 * b], sn = p.side[3 * b + 1];
        float x = n[0] * cs + n[1] * sn;
        float y = n[1] * cs - n[0] * sn;
        float z = n[2];
        if (!(J.flags & MTLORA_AUGMENT_FLAG_NO_RENORM)) {
            const float d = __builtin_sqrtf((x * x + y * y) + z * z) + AUG_EPS;
            x = x / d, y = y / d, z = z / d;
        }
        float* of = reinterpret_cast<float*>(o);
        of[0] = x, of[1] = y, of[2] = z;
    }
}

// the wave's AUG_PIX pixels from flat pixel p0 on: compute into `img`, then write [p0 * PB, ...) of dst in 16-byte chunks
template <int KIND, int PB>
__device__ __forceinline__ void aug_wave(const AugmentParams& p, const mtlora_augment_job& J, int64_t p0, unsigned char* img,
                                         const int32_t* cq, const float* cf) {
    const int lane = threadIdx.x & (MTL_WAVE - 1);
    const int64_t total = (int64_t)p.B * p.Ho * p.Wo;
    const int64_t first = p0 + (int64_t)lane * AUG_PPL;
    if (first < total) {
        const int HW = p.Ho * p.Wo;
        int b = (int)(first / HW);
        const int rem = (int)(first - (int64_t)b * HW);
        int v = rem / p.Wo, u = rem - v * p.Wo;
        AugSample s = aug_sample(p, b);
        for (int j = 0; j < AUG_PPL && first + j < total; ++j) {
            aug_pixel<KIND>(p, J, s, b, u, v, img + (lane * AUG_PPL + j) * PB, cq, cf);
            if (++u == p.Wo) {
                u = 0;
                if (++v == p.Ho) {
                    v = 0;
                    if (++b < p.B) s = aug_sample(p, b);
                }
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the wave's LDS writes are visible to all of its lanes
    __builtin_amdgcn_s_waitcnt(0xc07f);                       // lgkmcnt(0)
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int64_t left = (total - p0) * PB;  // bytes of the tensor from the wave's first on (> 0)
    const int nb = left < (int64_t)AUG_PIX * PB ? (int)left : AUG_PIX * PB;
    unsigned char* d = reinterpret_cast<unsigned char*>(J.dst) + p0 * PB;  // 16-byte aligned: dst is, and AUG_PIX * PB % 16 == 0
    for (int k = lane * 16; k < nb; k += MTL_WAVE * 16) {
        if (k + 16 <= nb) {
            *reinterpret_cast<u32x4*>(d + k) = *reinterpret_cast<const u32x4*>(img + k);
        } else if (PB % 4 == 0) {
            for (int i = k; i < nb; i += 4) *reinterpret_cast<uint32_t*>(d + i) = *reinterpret_cast<const uint32_t*>(img + i);
        } else {
            for (int i = k; i < nb; ++i) d[i] = img[i];
        }
    }
}

__global__ __launch_bounds__(AUG_WAVES* MTL_WAVE) void k_augment(const AugmentParams p) {
    __shared__ __attribute__((aligned(16))) int32_t s_cq[32 * 4];
    __shared__ __attribute__((aligned(16))) float s_cf[32 * 4];
    __shared__ __attribute__((aligned(16))) unsigned char s_img[AUG_WAVES][AUG_PIX * 12];
    const int j = blockIdx.x / p.blocks_per_job, blk = blockIdx.x - j * p.blocks_per_job;
    const mtlora_augment_job& J = p.job[j];
    const int wave = threadIdx.x >> 6;
    const int64_t p0 = (int64_t)blk * AUG_BLOCK_PIX + (int64_t)wave * AUG_PIX;
    const bool work = p0 < (int64_t)p.B * p.Ho * p.Wo;  // (wave-uniform)
    unsigned char* img = s_img[wave];
    switch (J.kind) {  // (uniform over the workgroup)
        case MTLORA_AUGMENT_IMAGE_CUBIC_U8:
            if (threadIdx.x < 32 * 4) s_cq[threadIdx.x] = p.cq[threadIdx.x];
            __syncthreads();
            if (work) aug_wave<MTLORA_AUGMENT_IMAGE_CUBIC_U8, 3>(p, J, p0, img, s_cq, s_cf);
            break;
        case MTLORA_AUGMENT_NORMALS_CUBIC_F32:
            if (threadIdx.x < 32 * 4) s_cf[threadIdx.x] = p.cf[threadIdx.x];
            __syncthreads();
            if (work) aug_wave<MTLORA_AUGMENT_NORMALS_CUBIC_F32, 12>(p, J, p0, img, s_cq, s_cf);
            break;
        case MTLORA_AUGMENT_CLASS_NEAREST_U8:
            if (work) aug_wave<MTLORA_AUGMENT_CLASS_NEAREST_U8, 1>(p, J, p0, img, s_cq, s_cf);
            break;
        default:
            if (work) aug_wave<MTLORA_AUGMENT_DEPTH_NEAREST_F32, 4>(p, J, p0, img, s_cq, s_cf);
            break;
    }
}

}  // namespace

extern "C" {

int mtlora_augment_batch(const mtlora_augment_job* jobs, int n_jobs, int64_t B, int32_t Hc, int32_t Wc, int32_t Ho, int32_t Wo,
                         const int32_t* size, const int64_t* geom, const float* side, const int32_t* cubic_q15,
                         const float* cubic_f32, void* stream) {
    if (n_jobs < 1 || n_jobs > MTLORA_INGEST_MAX_JOBS || !jobs) return MTLORA_ERR_UNSUPPORTED;
    if (B < 1 || Hc < 1 || Wc < 1 || Ho < 1 || Wo < 1) return MTLORA_ERR_UNSUPPORTED;
    if (!size || !geom) return MTLORA_ERR_UNSUPPORTED;
    for (int i = 0; i < n_jobs; ++i) {
        const mtlora_augment_job& J = jobs[i];
        uintptr_t es = 1;
        switch (J.kind) {
            case MTLORA_AUGMENT_IMAGE_CUBIC_U8:
                if (!cubic_q15) return MTLORA_ERR_UNSUPPORTED;
                break;
            case MTLORA_AUGMENT_CLASS_NEAREST_U8:
                break;
            case MTLORA_AUGMENT_NORMALS_CUBIC_F32:
                if (!cubic_f32 || !side) return MTLORA_ERR_UNSUPPORTED;
                es = 4;
                break;
            case MTLORA_AUGMENT_DEPTH_NEAREST_F32:
                if (!side) return MTLORA_ERR_UNSUPPORTED;
                es = 4;
                break;
            default:
                return MTLORA_ERR_UNSUPPORTED;
        }
        if (J.flags & ~MTLORA_AUGMENT_FLAG_NO_RENORM) return MTLORA_ERR_UNSUPPORTED;
        if (!J.src || !J.dst) return MTLORA_ERR_UNSUPPORTED;
        if ((reinterpret_cast<uintptr_t>(J.src) & (es - 1)) || (reinterpret_cast<uintptr_t>(J.dst) & 15)) return MTLORA_ERR_ALIGN;
    }
    if ((reinterpret_cast<uintptr_t>(size) & 3) || (reinterpret_cast<uintptr_t>(geom) & 7) || (reinterpret_cast<uintptr_t>(side) & 3) ||
        (reinterpret_cast<uintptr_t>(cubic_q15) & 3) || (reinterpret_cast<uintptr_t>(cubic_f32) & 3))
        return MTLORA_ERR_ALIGN;
    const int64_t out_pix = B * (int64_t)Ho * Wo;
    if (B > 65535 || (int64_t)Ho * Wo >= ((int64_t)1 << 31) || out_pix >= ((int64_t)1 << 40)) return MTLORA_ERR_SHAPE;
    const int64_t blocks_per_job = mtl_ceil_div(out_pix, AUG_BLOCK_PIX);
    if (blocks_per_job * n_jobs >= ((int64_t)1 << 31)) return MTLORA_ERR_SHAPE;
    AugmentParams p;
    for (int i = 0; i < MTLORA_INGEST_MAX_JOBS; ++i) p.job[i] = i < n_jobs ? jobs[i] : mtlora_augment_job{nullptr, nullptr, -1, 0};
    p.size = size;
    p.geom = geom;
    p.side = side;
    p.cq = cubic_q15;
    p.cf = cubic_f32;
    p.n_jobs = n_jobs;
    p.B = (int)B;
    p.Hc = Hc;
    p.Wc = Wc;
    p.Ho = Ho;
    p.Wo = Wo;
    p.blocks_per_job = (int)blocks_per_job;
    hipLaunchKernelGGL(k_augment, dim3((unsigned)(blocks_per_job * n_jobs)), dim3(AUG_WAVES * MTL_WAVE), 0,
                       reinterpret_cast<hipStream_t>(stream), p);
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

}  // extern "C"
