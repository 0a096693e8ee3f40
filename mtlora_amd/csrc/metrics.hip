// metrics.hip -- the validation end of an epoch (reference main.py:439-528 validate(): the final F.interpolate of
// models/swin_mtl.py:245 + evaluation/evaluate_utils.py get_output + the meters of evaluation/eval_*.py + the loss),
// fused: the forward-only sibling of loss.hip's k_up_loss.  One pass over the LOW-resolution channels-last head output
// (B, h, w, C) and the full-resolution label; every output pixel's C bilinear values are rebuilt in registers, the pixel is
// evaluated once, and only counters leave the kernel.  The (B, C, S*h, S*w) prediction, its argmax / sigmoid / normalised
// images and the meters' ~3 C boolean temporaries per class never exist, and nothing is copied to the host.
//
// One WAVE (a 64-thread workgroup) per tile of TQ x TR LOW-resolution pixels, TQ = 64 / S (8 at the models' S = 8): the tile
// owns the TQ S <= 64 output columns [S qx0, S (qx0 + TQ)) -- one per lane -- and the TR S output rows below S qy0, which the
// wave walks top to bottom.  No gradient, hence no rim: every output pixel belongs to exactly one tile, nothing is evaluated
// twice and there is no transpose-gather.  As in k_up_loss: the (TR + 2) x (TQ + 2) low-resolution neighbourhood is staged
// once as fp32 in LDS, the x-interpolated pair of a source cell stays in registers across the S rows of the cell, the labels
// of the next PF rows are in flight while the current ones are evaluated, and there is no workgroup barrier.
// Index / weight arithmetic is PyTorch's (align_corners=False: src = max((dst + 0.5) * in/out - 0.5, 0),
// i1 = i0 + (i0 < in - 1)), per output pixel, as loss.hip.  S <= 32.
//
// What leaves a tile:
//   integer counts   int64 atomicAdd on global memory, ADDED to the caller's array (a meter hands in its running state): the
//                    result does not depend on the order.  Per-lane register counters, one reduction per TILE (through an LDS
//                    image [64][n] summed by columns); the softmax kind, whose counters are indexed by class, keeps a per-wave
//                    LDS histogram instead (integer LDS atomics)
//   float sums       one fp32 partial per tile and quantity, fpartials[k * tiles + tile]; the caller sums them in a fixed order.
//                    No float atomics anywhere.
//
//   kind 0  softmax       argmax (first maximum) over C <= 48; valid = label != ignore
//                         counts[0..C) tp, [C..2C) predicted, [2C..3C) ground truth, [3C] valid;  floats: loss
//   kind 1  normals       n = up / (|up| + 1e-12), p = 2 ((n + 1) 255 / 2) / 255 - 1 in fp32 as get_output + the meters do
//                         V1 (eval_normals_v1.py:29-54) and V2 (eval_normals_v2.py:32-44)
//                         counts: n1, #<11.25, #<22.5, #<30, n2;  floats: loss, sum of V1 degrees, sum of V2 degrees
//   kind 2  saliency      q = (255 / (1 + exp(-up))) / 255 (get_output, then the meters' / 255)
//                         counts[0..57): for the 19 thresholds stat[16..35): tp, predicted, actual positives over
//                         label != ignore with sigmoid(q) >= t (eval_sal_beta.py:37-70: the second sigmoid is the reference's);
//                         counts[57 + (b 15 + j) 3 ..]: per image b and threshold stat[1 + j], j < 15: tp, fp, fn with q > t and
//                         label != 0 (eval_sal_no_beta.py:33-50, jaccard.py);  floats: loss (stat[0] = w)
//   kind 3  l1_masked     p = max(up, 1e-9); counts: valid;  floats: loss (unclamped up), sum (gt - p)^2,
//                         sum (log gt - log p)^2 over label != ignore (eval_depth.py:71-89)
//   kind 4  edge          floats: loss (kind 2's formula with the constant stat[0]), and the meter's value, which is the same
//                         formula applied to q (eval_edge.py:31-37 feeds the PROCESSED prediction to the loss)
//
// Partially labelled batches (mtlora_upsample_metrics_valid, VAL): a byte per sample says whether it carries a label, as in
// loss.hip.  A tile belongs to one sample, so the decision is wave-uniform: a tile of an unlabelled sample writes +0 to its
// float partials, adds to no counter and leaves before it loads anything of that sample.  stat holds the statistics over the
// labelled samples, and their number |V| behind the words of the unmasked launch (kinds 2 and 4 normalise by |V| H W).  VAL is
// a template parameter: the unmasked entry runs the code it ran before.
#include "dispatch.h"
#include "up_pixel.h"

namespace {

struct UpMetParams {
    const void* low;             // (B, h, w, C)
    const float* label;          // kind 1: (B, C, H, W); else (B, 1, H, W)
    const float* stat;           // device scalars, see above
    unsigned long long* counts;  // added to
    float* fpart;                // [NF][tiles]
    const unsigned char* valid;  // (B) non-zero: the sample has a label (VAL kernels only; NULL otherwise)
    int B, h, w, C, S, TR;
    int tiles;
    float ignore;
};

constexpr int MET_SAL_T1 = 15, MET_SAL_T2 = 19;
constexpr int MET_SAL_NC = 2 * MET_SAL_T1 + 1 + 2 * MET_SAL_T2 + 1;  // per-lane counters of the saliency kind
constexpr float MET_DEG = 57.29577951308232f;                          // 180 / pi
// VAL: the stat word that carries |V| -- behind the words of the unmasked launch
static __host__ __device__ constexpr int met_nv_word(int kind) { return kind == 2 ? 1 + MET_SAL_T1 + MET_SAL_T2 : 1; }

static __host__ __device__ inline int met_nfloat(int kind) { return kind == 1 || kind == 3 ? 3 : (kind == 4 ? 2 : 1); }
static inline int64_t met_nint(int kind, int64_t B, int C) {
    return kind == 0 ? 3 * (int64_t)C + 1 : kind == 1 ? 5 : kind == 2 ? 3 * MET_SAL_T2 + B * 3 * MET_SAL_T1 : kind == 3 ? 1 : 0;
}
// ints of LDS behind the staged neighbourhood
static __host__ __device__ inline int met_extra_lds(int kind, int C) {
    return kind == 0 ? 3 * C : kind == 2 ? 64 * (MET_SAL_NC | 1) + MET_SAL_NC : 0;
}
static inline size_t met_lds_bytes(int kind, int C, int S, int TR) {
    const int TQ = 64 / S;
    return ((size_t)(TR + 2) * (TQ + 2) * (C | 1) + met_extra_lds(kind, C)) * sizeof(float);
}
// low-res rows per tile: 4 as k_up_loss, fewer where the staged neighbourhood would not fit (scale 1 with many classes)
static inline int met_tr(int kind, int C, int S) {
    int tr = 4;
    while (tr > 1 && met_lds_bytes(kind, C, S, tr) > 48 * 1024) tr >>= 1;
    return tr;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <typename T, int MK, int CMAX, int SC, bool VAL>
__global__ __launch_bounds__(64) void k_up_metrics(const UpMetParams p) {
    extern __shared__ float sm[];
    constexpr int LK = MK == 4 ? 2 : MK;      // the loss formula of up_pixel
    constexpr int NL = MK == 1 ? CMAX : 1;    // label values per pixel
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
    float* lowt = sm;                                                // [TR + 2][TQ + 2][Cs]
    int* xl = reinterpret_cast<int*>(lowt + (TR + 2) * RP);          // kind 0: histogram [3C]; kind 2: [64][NC | 1] + [NC]
    const T* low = reinterpret_cast<const T*>(p.low);
    const float rs = (float)p.h / (float)H;  // in / out, exactly 1/S

    // a sample without a label (wave-uniform: b comes from blockIdx): +0 to the tile's partial of every float quantity, nothing
    // to any counter; neither low[b] nor label[b] is loaded
    if (VAL && __builtin_amdgcn_readfirstlane((int)p.valid[b]) == 0) {
        if (lane < met_nfloat(MK)) p.fpart[(int64_t)lane * p.tiles + blockIdx.x] = 0.f;
        return;
    }

    for (int i = lane; i < (TR + 2) * (TQ + 2) * C; i += 64) {
        const int pix = i / C, c = i - pix * C;
        const int py = pix / (TQ + 2), px = pix - py * (TQ + 2);
        int gy = qy0 - 1 + py, gx = qx0 - 1 + px;
        gy = gy < 0 ? 0 : (gy > p.h - 1 ? p.h - 1 : gy);
        gx = gx < 0 ? 0 : (gx > p.w - 1 ? p.w - 1 : gx);
        lowt[py * RP + px * Cs + c] = mtl_to_f32(low[(((int64_t)b * p.h + gy) * p.w + gx) * C + c]);
    }
    if (MK == 0)
        for (int i = lane; i < 3 * C; i += 64) xl[i] = 0;

    // 1 / normaliser of the mean, as k_up_loss.  VAL: stat[0] runs over the labelled samples; the formula of kinds 2 and 4 takes
    // |V| where it took B (the same expression: all labelled gives the same bits), and kind 0 guards a count of 0 as k_up_loss
    float norm;
    if (LK == 0)
        norm = (VAL && p.stat[0] == 0.f) ? 0.f : 1.f / p.stat[0];
    else if (LK == 1)
        norm = 1.f / fmaxf(p.stat[0], 1e-6f);
    else if (LK == 3)
        norm = 1.f / fmaxf(p.stat[0], 1.f);
    else
        norm = 1.f / ((VAL ? p.stat[met_nv_word(MK)] : (float)p.B) * (float)H * (float)W);
    const float wneg = LK == 2 ? p.stat[0] : 0.f;
    float th1[MK == 2 ? MET_SAL_T1 : 1], th2[MK == 2 ? MET_SAL_T2 : 1];  // (wave-uniform: scalar registers)
    if (MK == 2) {
#pragma unroll
        for (int j = 0; j < MET_SAL_T1; ++j) th1[MK == 2 ? j : 0] = p.stat[1 + j];
#pragma unroll
        for (int j = 0; j < MET_SAL_T2; ++j) th2[MK == 2 ? j : 0] = p.stat[1 + MET_SAL_T1 + j];
    }

    // this lane's output column
    const int ox = S * qx0 + lane;
    const bool col_ok = lane < TQ * S && ox < W;
    const int oxc = ox > W - 1 ? W - 1 : ox;
    float sx = ((float)oxc + 0.5f) * rs - 0.5f;
    sx = sx < 0.f ? 0.f : sx;
    const int ix0 = (int)sx, ix1 = ix0 + (ix0 < p.w - 1 ? 1 : 0);
    const float fx = sx - (float)ix0;
    int lx0 = ix0 - qx0 + 1, lx1 = ix1 - qx0 + 1;
    lx0 = lx0 < 0 ? 0 : (lx0 > TQ + 1 ? TQ + 1 : lx0);
    lx1 = lx1 < 0 ? 0 : (lx1 > TQ + 1 ? TQ + 1 : lx1);
    const int64_t HW = (int64_t)H * W;
    const float* lbase = p.label + (int64_t)b * (MK == 1 ? C : 1) * HW + oxc;
    const int oy_lo = S * qy0;
    const int oy_hi = S * (qy0 + TR) > H ? H : S * (qy0 + TR);

    float v0[CMAX], v1[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) v0[c] = v1[c] = 0.f;
    float fs[3] = {0.f, 0.f, 0.f};                 // this lane's float sums (fs[0]: loss)
    constexpr int NI = MK == 2 ? MET_SAL_NC : 5;
    int ic[NI];                                    // this lane's integer counters
#pragma unroll
    for (int i = 0; i < NI; ++i) ic[i] = 0;
    int cell = -1;
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();

    auto pixel = [&](int oy, const float (&lab)[NL]) __attribute__((always_inline)) {
        float sy = ((float)oy + 0.5f) * rs - 0.5f;
        sy = sy < 0.f ? 0.f : sy;
        const int iy0 = (int)sy, iy1 = iy0 + (iy0 < p.h - 1 ? 1 : 0);
        const float fy = sy - (float)iy0;
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
                v0[c] = c < C ? (1.f - fx) * r00[c] + fx * r01[c] : 0.f;
                v1[c] = c < C ? (1.f - fx) * r10[c] + fx * r11[c] : 0.f;
            }
        }
        float up[CMAX], g[CMAX];
#pragma unroll
        for (int c = 0; c < CMAX; ++c) up[c] = (1.f - fy) * v0[c] + fy * v1[c];

        if (MK == 0) {
            int am = 0;
            float mv = up[0];
#pragma unroll
            for (int c = 1; c < CMAX; ++c)
                if (c < C && up[c] > mv) {
                    mv = up[c];
                    am = c;
                }
            const float lv = up_pixel<LK, CMAX>(up, g, lab, C, p.ignore, norm, wneg);
            if (col_ok && lab[0] != p.ignore) {
                const int cls = (int)lab[0];
                fs[0] += lv;
                ic[0] += 1;
                atomicAdd(&xl[C + am], 1);
                if (cls >= 0 && cls < C) {
                    atomicAdd(&xl[2 * C + cls], 1);
                    if (cls == am) atomicAdd(&xl[cls], 1);
                }
            }
        } else if (MK == 1) {
            float r2 = 0.f;
#pragma unroll
            for (int c = 0; c < CMAX; ++c) r2 += up[c] * up[c];
            const float nrm = sqrtf(r2) + 1e-12f;
            float pr[CMAX], gt[CMAX];
            bool all_ok = true;
            float dot = 0.f, pn2 = 0.f, gn2 = 0.f;
#pragma unroll
            for (int c = 0; c < CMAX; ++c) {
                const float lc = lab[c < NL ? c : 0];
                const bool ok = lc != p.ignore;
                const float q = (up[c] / nrm + 1.0f) * 255.f / 2.0f;  // get_output
                pr[c] = c < C ? 2.f * q / 255.f - 1.f : 0.f;         // the meters
                gt[c] = c < C ? lc : 0.f;
                all_ok = all_ok && (c >= C || ok);
                dot += (c < C && ok) ? pr[c] * gt[c] : 0.f;           // V1 zeroes the invalid ENTRIES of both
                pn2 += pr[c] * pr[c];
                gn2 += gt[c] * gt[c];
            }
            const float deg1 = MET_DEG * acosf(fminf(fmaxf(dot, -1.f), 1.f));
            // V2: both re-normalised (a zero vector stays zero), 2 atan2(|p - g|, |p + g|)
            const float pn = sqrtf(pn2), gn = sqrtf(gn2);
            const float ip = pn == 0.f ? 1.f : pn, ig = gn == 0.f ? 1.f : gn;
            float dm = 0.f, dp = 0.f;
#pragma unroll
            for (int c = 0; c < CMAX; ++c) {
                const float a = pn == 0.f ? 0.f : pr[c] / ip, bq = gn == 0.f ? 0.f : gt[c] / ig;
                dm += (a - bq) * (a - bq);
                dp += (a + bq) * (a + bq);
            }
            const float deg2 = (2.f * atan2f(sqrtf(dm), sqrtf(dp))) * MET_DEG;
            const float lv = up_pixel<LK, CMAX>(up, g, lab, C, p.ignore, norm, wneg);
            if (col_ok) {
                fs[0] += lv;
                if (lab[0] != p.ignore) {
                    fs[1] += deg1;
                    ic[0] += 1;
                    ic[1] += deg1 < 11.25f ? 1 : 0;
                    ic[2] += deg1 < 22.5f ? 1 : 0;
                    ic[3] += deg1 < 30.f ? 1 : 0;
                }
                if (all_ok) {
                    fs[2] += deg2;
                    ic[4] += 1;
                }
            }
        } else if (MK == 2 || MK == 4) {
            const float o = up[0];
            const float q = (255.f / (1.f + expf(-o))) / 255.f;
            const float lv = up_pixel<LK, CMAX>(up, g, lab, C, p.ignore, norm, wneg);
            if (MK == 4) {
                float uq[CMAX];
                uq[0] = q;
                const float mv = up_pixel<LK, CMAX>(uq, g, lab, C, p.ignore, norm, wneg);
                if (col_ok) {
                    fs[0] += lv;
                    fs[1] += mv;
                }
            } else if (col_ok) {
                fs[0] += lv;
                const int gt1 = lab[0] != 0.f ? 1 : 0;
                ic[2 * MET_SAL_T1 < NI ? 2 * MET_SAL_T1 : 0] += gt1;
#pragma unroll
                for (int j = 0; j < MET_SAL_T1; ++j) {
                    const int pd = q > th1[MK == 2 ? j : 0] ? 1 : 0;
                    ic[j < NI ? j : 0] += pd & gt1;
                    ic[MET_SAL_T1 + j < NI ? MET_SAL_T1 + j : 0] += pd;
                }
                if (lab[0] != p.ignore) {
                    const float q2 = 1.f / (1.f + expf(-q));
                    const int tg = (int)lab[0];
                    constexpr int O2 = 2 * MET_SAL_T1 + 1;
                    ic[O2 + 2 * MET_SAL_T2 < NI ? O2 + 2 * MET_SAL_T2 : 0] += tg;
#pragma unroll
                    for (int j = 0; j < MET_SAL_T2; ++j) {
                        const int pd = q2 >= th2[MK == 2 ? j : 0] ? 1 : 0;
                        ic[O2 + j < NI ? O2 + j : 0] += pd * tg;
                        ic[O2 + MET_SAL_T2 + j < NI ? O2 + MET_SAL_T2 + j : 0] += pd;
                    }
                }
            }
        } else {  // MK == 3
            const float o = up[0];
            const float lv = up_pixel<LK, CMAX>(up, g, lab, C, p.ignore, norm, wneg);
            if (col_ok && lab[0] != p.ignore) {
                const float pc = fmaxf(o, 1e-9f);
                const float d = lab[0] - pc, dl = logf(lab[0]) - logf(pc);
                fs[0] += lv;
                fs[1] += d * d;
                fs[2] += dl * dl;
                ic[0] += 1;
            }
        }
    };

    // labels: PF rows in flight while the previous PF rows are evaluated (as k_up_loss)
    constexpr int PF = CMAX > 8 ? 1 : 4;
    float lab_next[PF][NL];
    auto fetch = [&](int oy0) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < PF; ++u)
#pragma unroll
            for (int c = 0; c < NL; ++c)
                lab_next[u][c] = (col_ok && oy0 + u < oy_hi && c < C) ? lbase[(int64_t)c * HW + (int64_t)(oy0 + u) * W] : 0.f;
    };
    fetch(oy_lo);
    for (int oyb = oy_lo; oyb < oy_hi; oyb += PF) {
        float labs[PF][NL];
#pragma unroll
        for (int u = 0; u < PF; ++u)
#pragma unroll
            for (int c = 0; c < NL; ++c) labs[u][c] = lab_next[u][c];
        if (oyb + PF < oy_hi) fetch(oyb + PF);
#pragma unroll
        for (int u = 0; u < PF; ++u)
            if (oyb + u < oy_hi) pixel(oyb + u, labs[u]);  // (wave-uniform)
    }

    // ---- one reduction per tile
    const int nf = met_nfloat(MK);
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (k < nf) {
            const float s = wave_sum(fs[k]);
            if (lane == 0) p.fpart[(int64_t)k * p.tiles + blockIdx.x] = s;
        }
    if (MK == 0) {
        const int nv = wave_sum(ic[0]);
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
        for (int i = lane; i < 3 * C; i += 64) {
            const int v = xl[i];
            if (v) atomicAdd(p.counts + i, (unsigned long long)v);
        }
        if (lane == 0 && nv) atomicAdd(p.counts + 3 * C, (unsigned long long)nv);
    } else if (MK == 1) {
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int v = wave_sum(ic[i < NI ? i : 0]);
            if (lane == 0 && v) atomicAdd(p.counts + i, (unsigned long long)v);
        }
    } else if (MK == 3) {
        const int v = wave_sum(ic[0]);
        if (lane == 0 && v) atomicAdd(p.counts, (unsigned long long)v);
    } else if (MK == 2) {
        constexpr int NC = MET_SAL_NC, LD = NC | 1;
        int* tot = xl + 64 * LD;
#pragma unroll
        for (int i = 0; i < NC; ++i) xl[lane * LD + i] = ic[i < NI ? i : 0];
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
        for (int i = lane; i < NC; i += 64) {
            int s = 0;
            for (int l = 0; l < 64; ++l) s += xl[l * LD + i];
            tot[i] = s;
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
        constexpr int O2 = 2 * MET_SAL_T1 + 1;
        for (int i = lane; i < 3 * MET_SAL_T2 + 3 * MET_SAL_T1; i += 64) {
            int v;
            int64_t at;
            if (i < 3 * MET_SAL_T2) {  // global, [j][tp, predicted, actual]
                const int j = i / 3, k = i - 3 * j;
                v = k == 0 ? tot[O2 + j] : k == 1 ? tot[O2 + MET_SAL_T2 + j] : tot[O2 + 2 * MET_SAL_T2];
                at = i;
            } else {  // this image, [j][tp, fp, fn]
                const int r = i - 3 * MET_SAL_T2, j = r / 3, k = r - 3 * j;
                const int tp = tot[j], pp = tot[MET_SAL_T1 + j], gp = tot[2 * MET_SAL_T1];
                v = k == 0 ? tp : k == 1 ? pp - tp : gp - tp;
                at = 3 * MET_SAL_T2 + (int64_t)b * 3 * MET_SAL_T1 + r;
            }
            if (v) atomicAdd(p.counts + at, (unsigned long long)v);
        }
    }
}

template <typename T, int MK, int CMAX, bool VAL>
static void launch_met(const UpMetParams& p, hipStream_t s) {
    const size_t lds = met_lds_bytes(MK, p.C, p.S, p.TR);
    if (p.S == 8)  // the scale of the models' heads
        hipLaunchKernelGGL((k_up_metrics<T, MK, CMAX, 8, VAL>), dim3((unsigned)p.tiles), dim3(64), lds, s, p);
    else
        hipLaunchKernelGGL((k_up_metrics<T, MK, CMAX, 0, VAL>), dim3((unsigned)p.tiles), dim3(64), lds, s, p);
}

template <typename T, bool VAL>
static int dispatch_met(int kind, const UpMetParams& p, hipStream_t s) {
    if (kind == 0) {
        if (p.C <= 8)
            launch_met<T, 0, 8, VAL>(p, s);
        else if (p.C <= 24)
            launch_met<T, 0, 24, VAL>(p, s);
        else if (p.C <= 48)
            launch_met<T, 0, 48, VAL>(p, s);
        else
            return MTLORA_ERR_UNSUPPORTED;
    } else if (kind == 1) {
        if (p.C > 4) return MTLORA_ERR_UNSUPPORTED;
        launch_met<T, 1, 4, VAL>(p, s);
    } else {
        if (p.C != 1) return MTLORA_ERR_UNSUPPORTED;
        if (kind == 2)
            launch_met<T, 2, 1, VAL>(p, s);
        else if (kind == 3)
            launch_met<T, 3, 1, VAL>(p, s);
        else
            launch_met<T, 4, 1, VAL>(p, s);
    }
    return MTLORA_OK;
}

static int64_t met_tiles(int kind, int64_t B, int h, int w, int C, int S) {
    const int tr = met_tr(kind, C, S), tq = 64 / S;
    return B * (int64_t)((h + tr - 1) / tr) * ((w + tq - 1) / tq);
}

}  // namespace

extern "C" {

int mtlora_upsample_metrics_sizes(int kind, int64_t B, int h, int w, int C, int scale, int64_t* n_int64, int64_t* n_float_partials) {
    if (kind < 0 || kind > 4 || B < 0 || h <= 0 || w <= 0 || C <= 0 || scale <= 0) return MTLORA_ERR_SHAPE;
    if (!n_int64 || !n_float_partials) return MTLORA_ERR_NULL;
    if (scale > 32 || C > 48 || (kind == 1 && C > 4) || (kind >= 2 && C != 1)) return MTLORA_ERR_UNSUPPORTED;
    if (met_lds_bytes(kind, C, scale, met_tr(kind, C, scale)) > 64 * 1024) return MTLORA_ERR_UNSUPPORTED;
    *n_int64 = met_nint(kind, B, C);
    *n_float_partials = met_nfloat(kind) * met_tiles(kind, B, h, w, C, scale);
    return MTLORA_OK;
}

// the launch behind both entries: mtlora_upsample_metrics hands in valid == NULL (need_valid false) and runs the VAL = false
// kernels
static int up_metrics_launch(int kind, const void* low, const float* label, const unsigned char* valid, bool need_valid,
                             const float* stat, int64_t* counts, float* fpartials, int64_t B, int h, int w, int C, int scale,
                             int dtype, float ignore_index, void* stream) {
    int64_t ni = 0, nfp = 0;
    const int rc0 = mtlora_upsample_metrics_sizes(kind, B, h, w, C, scale, &ni, &nfp);
    if (rc0 != MTLORA_OK) return rc0;
    if (!mtl_dtype_in(dtype, MTL_DT_F32_BF16)) return MTLORA_ERR_DTYPE;
    if (B == 0) return MTLORA_OK;
    if (mtl_any_null({low, label, stat, fpartials}) || (ni > 0 && !counts) || (need_valid && !valid)) return MTLORA_ERR_NULL;
    const int64_t tiles = met_tiles(kind, B, h, w, C, scale);
    if (tiles >= ((int64_t)1 << 31) || (int64_t)h * scale * (int64_t)w * scale >= ((int64_t)1 << 31)) return MTLORA_ERR_SHAPE;
    UpMetParams p;
    p.low = low;
    p.label = label;
    p.stat = stat;
    p.counts = reinterpret_cast<unsigned long long*>(counts);
    p.fpart = fpartials;
    p.valid = need_valid ? valid : nullptr;
    p.B = (int)B;
    p.h = h;
    p.w = w;
    p.C = C;
    p.S = scale;
    p.TR = met_tr(kind, C, scale);
    p.tiles = (int)tiles;
    p.ignore = ignore_index;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (need_valid) mtl_prof_tag("valid metrics k%d B%lld h%d w%d C%d S%d", kind, (long long)B, h, w, C, scale);
    MtlProfScope prof(PK_LOSS, (double)B * h * w * C * mtl_elem_size(dtype) +
                                   (double)B * h * scale * w * scale * 4.0 * (kind == 1 ? C : 1), s);
    const int rc = mtl_dispatch_f32_bf16(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        return need_valid ? dispatch_met<T, true>(kind, p, s) : dispatch_met<T, false>(kind, p, s);
    });
    if (rc != MTLORA_OK) return rc;
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

int mtlora_upsample_metrics(int kind, const void* low, const float* label, const float* stat, int64_t* counts, float* fpartials,
                            int64_t B, int h, int w, int C, int scale, int dtype, float ignore_index, void* stream) {
    return up_metrics_launch(kind, low, label, nullptr, false, stat, counts, fpartials, B, h, w, C, scale, dtype, ignore_index,
                             stream);
}

int mtlora_upsample_metrics_valid(int kind, const void* low, const float* label, const unsigned char* valid, const float* stat,
                                  int64_t* counts, float* fpartials, int64_t B, int h, int w, int C, int scale, int dtype,
                                  float ignore_index, void* stream) {
    return up_metrics_launch(kind, low, label, valid, true, stat, counts, fpartials, B, h, w, C, scale, dtype, ignore_index, stream);
}

}  // extern "C"
