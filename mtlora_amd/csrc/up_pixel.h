// up_pixel.h -- the per-output-pixel pieces shared by the fused upsample + loss kernel (loss.hip, k_up_loss) and its
// forward-only sibling (metrics.hip, k_up_metrics): the per-pixel loss formulas of mtl_loss_schemes.py and PyTorch's
// align_corners=False interpolation weight.  One copy, so the validation loss is the training loss bit for bit.
#pragma once
#include "common.h"

// per-output-pixel loss gradient g[c] = d loss / d up[c] (normalised), returns the pixel's share of the loss value;
// lab: the pixel's label (kinds 0, 2) or its C label channels (kind 1)
template <int KIND, int CMAX>
__device__ __forceinline__ float up_pixel(float (&up)[CMAX], float (&g)[CMAX], const float (&lab)[KIND == 1 ? CMAX : 1], int C,
                                          float ignore, float norm, float wneg) {
    float loss = 0.f;
    if (KIND == 0) {
#pragma unroll
        for (int c = 0; c < CMAX; ++c) g[c] = 0.f;
        if (lab[0] != ignore) {
            const int cls = (int)lab[0];
            float m = -3.0e38f;
#pragma unroll
            for (int c = 0; c < CMAX; ++c) m = c < C ? fmaxf(m, up[c]) : m;
            float sum = 0.f, ucls = 0.f;
#pragma unroll
            for (int c = 0; c < CMAX; ++c) {
                up[c] = c < C ? __expf(up[c] - m) : 0.f;
                sum += up[c];
            }
            const float inv = 1.f / sum;
#pragma unroll
            for (int c = 0; c < CMAX; ++c) {
                const float pc = up[c] * inv;
                ucls = c == cls ? pc : ucls;
                g[c] = norm * (pc - (c == cls ? 1.f : 0.f));
            }
            loss = -__logf(ucls) * norm;
        }
    } else if (KIND == 1) {
        float mk[CMAX];
        float r2 = 0.f;
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
            mk[c] = (c < C && lab[c < (KIND == 1 ? CMAX : 1) ? c : 0] != ignore) ? 1.f : 0.f;
            r2 += up[c] * up[c];
        }
        const float r = sqrtf(r2), n = r + 1e-12f;
        float gc[CMAX], dot = 0.f;
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
            const float d = up[c] / n - (c < C ? lab[c < (KIND == 1 ? CMAX : 1) ? c : 0] : 0.f);
            gc[c] = (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) * mk[c] * norm;
            dot += gc[c] * up[c];
            loss += fabsf(d) * mk[c] * norm;
        }
        const float k2 = r > 0.f ? dot / (r * n * n) : 0.f;
#pragma unroll
        for (int c = 0; c < CMAX; ++c) g[c] = gc[c] / n - k2 * up[c];
    } else if (KIND == 2) {
        const float lb = lab[0] >= 0.5f ? 1.f : 0.f;
        const float coef = (wneg * lb + (1.f - wneg) * (1.f - lb)) * norm;
        const float o = up[0], gz = o >= 0.f ? 1.f : 0.f;
        const float lv = o * (lb - gz) - log1pf(__expf(o - 2.f * o * gz));
        const float sg = 1.f / (1.f + __expf(-o));
        g[0] = -coef * (lb - sg);
        loss = -coef * lv;
    } else {  // KIND 3: |up - label| over label != ignore
        const float d = up[0] - lab[0];
        const float m = lab[0] != ignore ? norm : 0.f;
        g[0] = (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) * m;
        loss = fabsf(d) * m;
    }
    return loss;
}

// weight of output index o for low-res index q along one axis (PyTorch's source index arithmetic)
__device__ __forceinline__ float up_weight(int o, int q, float rs, int n_in) {
    float s = ((float)o + 0.5f) * rs - 0.5f;
    s = s < 0.f ? 0.f : s;
    const int i0 = (int)s, i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    const float f = s - (float)i0;
    return (i0 == q ? 1.f - f : 0.f) + (i1 == q ? f : 0.f);
}
