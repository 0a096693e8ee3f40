// attention_dropout.h -- attention dropout inside the window attention kernels (swin_transformer_mtlora.py:216, `self.attn_drop` on
// the softmax output):  P = softmax(..),  P' = keep . P / (1 - p),  O = P' V.
// Included by attention.hip inside its anonymous namespace.  The scores never leave registers, so the keep bits are generated where
// the probabilities are consumed -- forward and backward regenerate the same bits, no mask is stored.
//
// Mask definition (restated by the tests with oracle.dropout_keep_mask_t(seed, MTL_ATTN_DROP_STREAM, n_windows * nH * N, N, p)):
//   element (window w, head h, query i, key j)  =  mtl_dropout_keep of common.h with
//       row     m = (w * nH + h) * N + i        (w: index in the reference's (B_, nH, N, N) attention tensor -- image, window row,
//                                                window column; i, j: tokens of the window AFTER the cyclic shift, so both layouts
//                                                draw the same mask for the same logical window)
//       column  k = j
//       stream  MTL_ATTN_DROP_STREAM            (the linear layers' dropout is stream 0; the activation dropout sites: common.h)
//   keep threshold floor(p * 65536) and the 1 / (1 - p) factor exactly as the linear kernels use them (mtl_make_dropout; a p below
//   2^-16 has threshold 0 and is "off").  m must fit 32 bits: the host refuses n_windows * nH * N >= 2^32.
// One mix32 yields the bits of two adjacent keys (k >> 1).  Where a lane owns a QUERY its accumulator registers hold runs of four
// consecutive keys: two mix32 per run.  Where a lane owns a KEY (phase 2 of the wide backward) the partner key sits in lane ^ 1: the
// even lane hashes the even query rows, the odd lane the odd ones, and a quad-permute DPP move exchanges the words.
constexpr uint32_t MTL_ATTN_DROP_STREAM = 0x41u;

struct AttnDropParams : AttnParams {
    DropoutCfg drop;
    float keep_scale;  // 1 / (1 - p)
};

// The dropout kernels need the registers that the plain kernels spend on values a lane derives from its id alone (fragment addresses,
// clamped rows, validity masks: the optimiser hoists them out of the persistent loop and keeps them live across it).  Laundering the lane
// id once per window keeps those values short-lived, as wide_opaque does in attention_wide.h.  ON = false: the identity.
template <bool ON>
__device__ __forceinline__ int attn_opaque_lane(int v) {
    if constexpr (ON) asm volatile("" : "+v"(v));
    return v;
}
template <typename P>
__device__ __forceinline__ DropoutCfg attn_drop_cfg(const P& p) {
    DropoutCfg c = p.drop;
    mtl_dropout_resolve(c);
    return c;
}
// row hash of query i of (window w, head)
__device__ __forceinline__ uint32_t attn_drop_rowhash(const DropoutCfg& c, const AttnParams& p, int64_t w, int head, int i) {
    return mtl_dropout_rowhash(c, MTL_ATTN_DROP_STREAM, ((uint32_t)w * (uint32_t)p.nH + (uint32_t)head) * (uint32_t)p.N + (uint32_t)i);
}
// query-owned 32 x 32 accumulator tile: f(r, keep) for the 16 elements of a lane, element r <-> key j0 + (r & 3) + 8 (r >> 2)
// (j0 = 32 sj + 4 (lane >> 5): a multiple of 4)
template <typename F>
__device__ __forceinline__ void attn_keep_tile(const DropoutCfg& c, uint32_t rowhash, int j0, F&& f) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const uint32_t h = mtl_dropout_pairbits(c, rowhash, (uint32_t)(j0 + 8 * q + 2 * e));
            f(4 * q + 2 * e, (h & 0xFFFFu) >= c.thr16);
            f(4 * q + 2 * e + 1, (h >> 16) >= c.thr16);
        }
}
// key-owned tile (lane owns key j, lane ^ 1 owns j ^ 1): keep bits of the adjacent query rows (i0, i0 + 1) whose row hashes are
// rh0 / rh1.  Every lane of the wave must be active (DPP exchange).
__device__ __forceinline__ void attn_keep_keypair(const DropoutCfg& c, uint32_t rh0, uint32_t rh1, int j, bool& keep0, bool& keep1) {
    const bool odd = j & 1;
    const uint32_t own = mtl_dropout_pairbits(c, odd ? rh1 : rh0, (uint32_t)j);
    const uint32_t other = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)own, 0xB1, 0xF, 0xF, false);  // quad_perm [1, 0, 3, 2]
    const uint32_t h0 = odd ? other : own, h1 = odd ? own : other;
    keep0 = (odd ? h0 >> 16 : h0 & 0xFFFFu) >= c.thr16;
    keep1 = (odd ? h1 >> 16 : h1 & 0xFFFFu) >= c.thr16;
}
