// act_dropout.h -- activation dropout (MODEL.DROP_RATE) generated inside the streaming kernels that consume it: act_dropout.hip
// (drop(act(h)) of the Mlp's hidden tensors, pos_drop) and the DROP instantiations of the residual + DropPath kernels of glue.hip
// (proj_drop / the Mlp's output drop, applied where the branch is added to the residual).  No mask is stored: forward and backward
// regenerate the same bits.
//
// Mask definition (restated by functional.act_dropout_torch / residual_droppath_drop_torch on oracle.dropout_keep_mask):
//   element (row m, channel c) of tensor k of a call  =  mtl_dropout_keep of common.h with
//       row     m                               (row of the (M, C) matrix, 32 bits: the host refuses M >= 2^32)
//       column  c
//       stream  site + MTL_ACT_DROP_TENSOR_STRIDE * k     (site: MTL_ACT_DROP_* of common.h; k = 0 shared tensor, 1 + i task i)
//   keep threshold floor(p * 65536) and the 1 / (1 - p) factor exactly as the linear and attention kernels use them
//   (mtl_make_dropout; a p below 2^-16 has threshold 0 and is "off").
// A lane owns 8 consecutive channels of one row per step: one row hash, then one mix32 per channel pair.
#pragma once
#include <cmath>

#include "common.h"

struct ActDrop {
    DropoutCfg cfg;
    uint32_t site;
    float inv_keep;  // 1 / (1 - p); 1 when off
};

// the checks of a dropout argument that follow the pointer checks of an entry (d is non-null): p in [0, 1), 32-bit rows
static inline int mtl_act_drop_make(const mtlora_attn_dropout* d, int site, int64_t M, ActDrop& o) {
    if (!std::isfinite(d->p) || d->p < 0.f || d->p >= 1.f) return MTLORA_ERR_SHAPE;
    if (M >= ((int64_t)1 << 32)) return MTLORA_ERR_SHAPE;
    o.cfg = mtl_make_dropout(d->p, d->seed, d->seed_offset);
    o.site = (uint32_t)site;
    o.inv_keep = o.cfg.enabled() ? 1.f / (1.f - d->p) : 1.f;
    return MTLORA_OK;
}

// bit e of the result: channel c0 + e of the row whose hash is `rowhash` is kept (c0 even)
__device__ __forceinline__ uint32_t mtl_act_keep8(const DropoutCfg& c, uint32_t rowhash, uint32_t c0) {
    uint32_t keep = 0u;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t h = mtl_dropout_pairbits(c, rowhash, c0 + 2 * w);
        keep |= ((h & 0xFFFFu) >= c.thr16 ? 1u : 0u) << (2 * w);
        keep |= ((h >> 16) >= c.thr16 ? 1u : 0u) << (2 * w + 1);
    }
    return keep;
}
__device__ __forceinline__ uint32_t mtl_act_rowhash(const DropoutCfg& c, uint32_t site, int k, int64_t row) {
    return mtl_dropout_rowhash(c, site + MTL_ACT_DROP_TENSOR_STRIDE * (uint32_t)k, (uint32_t)row);
}
