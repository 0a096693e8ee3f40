// nt.h -- the tiled "NT" kernels of MTLoRALinear and what every kernel header shares: the segment table (Segs), the packed-factor
// layout (CtxLayout), k_pack / k_pack_table, NtParams, k_nt and its straight-line bf16 form k_ntl.  Included first by linear.hip
// (stream.h, dense.h and pq.h use its tile constants, nt_map, g_zero16, gelu_* and NlParams); linear.hip has the kernel overview.
#pragma once

#include "common.h"
#include "internal.h"

namespace {

constexpr int TILE = 128;    // rows per CTA tile, both operands
constexpr int SUBT = 3;             // 64-byte MFMA sub-tiles per staged k-tile: K = 96 bf16 is ONE round trip
constexpr int VPT = SUBT;           // 16-byte vectors per thread per tile row
constexpr int ROWB = 64 * SUBT;     // payload bytes per row per k-tile (96 bf16 / 48 f32)
constexpr int LDSB = ROWB + 16;     // padded LDS row stride (conflict-free ds_read_b128, 16-B aligned)
constexpr int EPI_ROW = 64 * 2 + 8;                      // row stride of a wave's bf16 output image (epilogue)
constexpr int EPI_BYTES = 4 * 64 * EPI_ROW;               // 4 waves x 64 rows = 8 waves x 32 rows
constexpr int STAGE_BYTES = 2 * TILE * LDSB > EPI_BYTES ? 2 * TILE * LDSB : EPI_BYTES;  // staging / epilogue region
constexpr int MAXO = MTLORA_MAX_TASKS + 1;

// ------------------------------------------------------------------------------------------------
// segment table: output o (0 = shared, 1..T = tasks) owns columns [off, off + rp) of the rank axis
// ------------------------------------------------------------------------------------------------
struct Segs {
    int n;  // 1 + T
    int r[MAXO], rp[MAXO], off[MAXO];
    int R;     // row stride of P / Q / the packed factors (columns), a multiple of 16
    int used;  // columns that belong to a segment: [used, R) is padding nobody writes
};
// packed factors (offsets relative to the pack base: the head of the ctx buffer, or the caller's persistent d->packed buffer) and
// P (offset relative to the ctx base)
struct CtxLayout {
    int64_t a_cat, b_cat, at_cat, bt_cat, alpha, a_proj, bt_proj, b_frag, at_frag, pack_total, p, total;
};

// ------------------------------------------------------------------------------------------------
// k_pack
// ------------------------------------------------------------------------------------------------
struct PackParams {
    const float* A[MAXO];
    const float* B[MAXO];
    float alpha[MAXO];
    const float* alpha_dev[MAXO];  // nullable: the segment's scale lives on the device (a trainable scale), alpha[o] then only holds
                                   // the host's factor f (dropout keep scale or 1) and the packed value is *alpha_dev[o] * f
    Segs s;
    int K, N;
};
// alpha of segment o as packed: the by-value product of the host, or the same fp32 product formed here from the device scale (one
// IEEE multiply either way: a device scale holding s packs bit for bit what scale = s packs by value)
template <typename PP>
__device__ __forceinline__ float pack_alpha(const PP& p, int o) {
    const float* __restrict__ sd = p.alpha_dev[o];
    return sd ? *sd * p.alpha[o] : p.alpha[o];
}

// The packing walks 64 x 64 TILES of the two concatenated factor matrices -- A_cat (R x K, rows = rank columns rr) and B_cat (N x R) -- one
// tile per workgroup pass: the fp32 masters are read along their contiguous axis (K for A, the segment's rank for B), the same-orientation
// copies (a_cat / a_proj, b_cat) are stored from registers, and the tile goes through LDS once for everything that is transposed or
// permuted (at_cat, bt_cat / bt_proj, the fragment-major at_frag / b_frag): every global access of the launch is a coalesced row segment.
// (Round 3's element-wise walk scattered 2-byte stores with a stride of R for the transposed copies and divided 64-bit indices per
// element: 1.07 ms for the 72 layers of Swin-B at rank 128, 30 x the time of the bytes it moves.)
constexpr int PK_T = 64;

template <typename PP>
__device__ __forceinline__ int pack_seg_of(const PP& p, int rr) {
    int o = 0;
#pragma unroll
    for (int q = 1; q < MAXO; ++q)
        if (q < p.s.n && rr >= p.s.off[q]) o = q;
    return o;
}

template <typename T, typename PP>
__device__ __forceinline__ void pack_body(const PP& p, T* a_cat, T* b_cat, T* at_cat, T* bt_cat, float* alpha, T* a_proj, T* bt_proj, T* b_frag,
                                          T* at_frag, int bid, int nblk) {
    __shared__ float tile[PK_T][PK_T + 1];
    constexpr bool FRAG = sizeof(T) == 2;  // fragment-major expansion factors: 16-bit types only (the wave-streaming kernels)
    const int R = p.s.R, K = p.K, N = p.N;
    const int tr = (R + PK_T - 1) / PK_T, tk = (K + PK_T - 1) / PK_T, tn = (N + PK_T - 1) / PK_T;
    const int na_t = tr * tk, nb_t = tn * tr;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int R16 = ((R + 31) >> 5) << 1, K32 = (K + 31) & ~31, N32 = (N + 31) & ~31;
    for (int job = bid; job < na_t + nb_t; job += nblk) {
        const bool isa = job < na_t;
        const int jb = isa ? job : job - na_t;
        // tile origin: rows r0 / cols c0 of A_cat (rr, k), or rows n0 / cols r0 of B_cat (n, rr)
        const int row0 = isa ? (jb / tk) * PK_T : (jb / tr) * PK_T;
        const int col0 = isa ? (jb % tk) * PK_T : (jb % tr) * PK_T;
        float v[PK_T / 4];  // all 16 loads of the tile are in flight before the first store (the stores may alias for all the compiler knows)
        if (isa) {
            const int c = col0 + tx;
            float al[PK_T / 4];
#pragma unroll
            for (int i = 0; i < PK_T / 4; ++i) {
                const int rr = row0 + ty + 4 * i;  // (wave-uniform)
                const int o = pack_seg_of(p, rr), lr = rr - p.s.off[o];
                al[i] = pack_alpha(p, o);
                v[i] = (rr < R && lr < p.s.r[o] && c < K && p.A[o]) ? p.A[o][(int64_t)lr * K + c] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < PK_T / 4; ++i) {
                const int row = ty + 4 * i, rr = row0 + row;
                tile[row][tx] = v[i];
                if (rr < R && c < K) {
                    a_cat[(int64_t)rr * K + c] = mtl_from_f32<T>(v[i]);
                    a_proj[(int64_t)rr * K + c] = mtl_from_f32<T>(v[i] * al[i]);
                }
            }
            if (col0 == 0 && threadIdx.x < PK_T && row0 + tx < R) alpha[row0 + tx] = pack_alpha(p, pack_seg_of(p, row0 + tx));
        } else {
            const int rr = col0 + tx;
            const int o = pack_seg_of(p, rr), lr = rr - p.s.off[o], ro = p.s.r[o];
            const bool live = rr < R && lr < ro && p.B[o];
            const float* __restrict__ Bo = p.B[o];
#pragma unroll
            for (int i = 0; i < PK_T / 4; ++i) {
                const int n = row0 + ty + 4 * i;
                v[i] = (live && n < N) ? Bo[(int64_t)n * ro + lr] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < PK_T / 4; ++i) {
                const int row = ty + 4 * i, n = row0 + row;
                tile[row][tx] = v[i];
                if (rr < R && n < N) b_cat[(int64_t)n * R + rr] = mtl_from_f32<T>(v[i]);
            }
        }
        __syncthreads();
        if (isa) {  // at_cat[k][rr]: lanes along rr
            const int rr = row0 + tx;
#pragma unroll 4
            for (int i = 0; i < PK_T / 4; ++i) {
                const int cl = ty + 4 * i, c = col0 + cl;
                if (rr < R && c < K) at_cat[(int64_t)c * R + rr] = mtl_from_f32<T>(tile[tx][cl]);
            }
        } else {    // bt_cat / bt_proj[rr][n]: lanes along n
            const int n = row0 + tx;
#pragma unroll 4
            for (int i = 0; i < PK_T / 4; ++i) {
                const int rl = ty + 4 * i, rr = col0 + rl;  // (wave-uniform)
                if (rr < R && n < N) {
                    const float v = tile[tx][rl];
                    bt_cat[(int64_t)rr * N + n] = mtl_from_f32<T>(v);
                    bt_proj[(int64_t)rr * N + n] = mtl_from_f32<T>(v * pack_alpha(p, pack_seg_of(p, rr)));
                }
            }
        }
        if constexpr (FRAG) {
            // fragment (32-row block blk of k or n, 16-wide rank step t) = 512 elements: lane l = (row blk * 32 + (l & 31), h = l >> 5)
            // holds rank columns 16 t + 8 (s >> 2) + 4 h + (s & 3), s = 0..7.  The tile holds 2 x 4 fragments; a thread writes two
            // (fragment, lane) groups of 8 elements = one 16-byte store each.
            T* __restrict__ dst = isa ? at_frag : b_frag;
            const int blk0 = (isa ? col0 : row0) >> 5, t0 = (isa ? row0 : col0) >> 4, nblk32 = (isa ? K32 : N32) >> 5;
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
                const int q = threadIdx.x + 256 * h2, fl = q >> 6, ln = q & 63;
                const int bl = fl >> 2, tl = fl & 3, rl = bl * 32 + (ln & 31);
                if (blk0 + bl < nblk32 && t0 + tl < R16) {
                    T tmp[8];
#pragma unroll
                    for (int sidx = 0; sidx < 8; ++sidx) {
                        const int kl = 16 * tl + 8 * (sidx >> 2) + 4 * (ln >> 5) + (sidx & 3);
                        tmp[sidx] = mtl_from_f32<T>(isa ? tile[kl][rl] : tile[rl][kl]);
                    }
                    const int64_t f = (int64_t)(blk0 + bl) * R16 + (t0 + tl);
                    *reinterpret_cast<uint4*>(dst + f * 512 + ln * 8) = *reinterpret_cast<const uint4*>(tmp);
                }
            }
        }
        __syncthreads();
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_pack(PackParams p, T* a_cat, T* b_cat, T* at_cat, T* bt_cat, float* alpha, T* a_proj,
                                              T* bt_proj, T* b_frag, T* at_frag) {
    pack_body<T>(p, a_cat, b_cat, at_cat, bt_cat, alpha, a_proj, bt_proj, b_frag, at_frag, (int)blockIdx.x, (int)gridDim.x);
}

// one launch for EVERY layer of a model (mtlora_linear_pack_table): blockIdx.y = table entry.  The factors change once per optimizer
// step, so a trainer refreshes all the packed buffers here instead of paying one k_pack launch per layer and forward call
// (48 launches per step at C2, 96 at C4).
struct PackEntry {
    PackParams pp;
    unsigned char* dst;  // the layer's packed buffer (device)
    int64_t off[9];      // a_cat, b_cat, at_cat, bt_cat, alpha, a_proj, bt_proj, b_frag, at_frag
};
template <typename T>
__global__ __launch_bounds__(256) void k_pack_table(const PackEntry* __restrict__ table) {
    const PackEntry& e = table[blockIdx.y];
    unsigned char* d = e.dst;
    pack_body<T>(e.pp, reinterpret_cast<T*>(d + e.off[0]), reinterpret_cast<T*>(d + e.off[1]), reinterpret_cast<T*>(d + e.off[2]),
                 reinterpret_cast<T*>(d + e.off[3]), reinterpret_cast<float*>(d + e.off[4]), reinterpret_cast<T*>(d + e.off[5]),
                 reinterpret_cast<T*>(d + e.off[6]), reinterpret_cast<T*>(d + e.off[7]), reinterpret_cast<T*>(d + e.off[8]), (int)blockIdx.x,
                 (int)gridDim.x);
}

// ------------------------------------------------------------------------------------------------
// k_nt
// ------------------------------------------------------------------------------------------------
struct NtOut {
    void* ptr;       // (M x ld_out) output, element type T
    int seg_lo, seg_hi;  // rank-column range of L/R chained onto this output ([lo,hi) empty -> none)
    int use_base;    // add the shared base accumulator
    int mask_lr;     // multiply the low-rank part by the dropout keep mask of (m, n)
    int fold;        // after storing: base += low-rank part ('matrixv2': tasks see the shared update)
    const void* gate;  // GATE kernels: out *= gelu'(gate[m][n]) (same shape / dtype / row stride as the output), nullable
    void* act;         // ACT kernels: second output gelu(out) (same shape / dtype / row stride), nullable
};

struct NtParams {
    // base GEMM
    const void* act[MAXO];  // (M x K) sources, summed while staging
    int n_act;
    int act_mask;           // dropout keep-mask applied to the staged activation
    int64_t ld_act;
    const void* wgt;        // (n_rows x K)
    int64_t ld_wgt;
    int64_t M;
    int n_rows;             // rows of wgt == output columns
    int K;                  // reduction length of the base GEMM (0 -> no base GEMM)
    const float* bias;      // per output column, nullable
    const float* alpha;     // per output column multiplier on the base GEMM, nullable
    // low-rank epilogue
    const void* L;          // (M x ldL)
    const void* Rm;         // (n_rows x ldR)
    int64_t ldL, ldR;
    int n_out;
    NtOut out[MAXO];
    int64_t ld_out;
    // batched form (gridDim.z = nz > 0): z selects activation / weight row slab / output column slab
    int nz;
    const void* zact[MAXO];
    int zrow0[MAXO], zrows[MAXO], zmask[MAXO];
    DropoutCfg drop;
};

// kernel parameters are read straight from the kernarg segment (constant address space): dynamic indexing of a
// by-value struct argument would make the compiler copy the whole struct to scratch
typedef const __attribute__((address_space(4))) NtParams* NtPtr;

// RI = tile rows per thread per operand: 2 with 256 threads (4 waves), 1 with 512 threads (8 waves)
// A thread stages 3 * RI 16-byte vectors per operand per k-tile.  Which (row, vector) a thread owns is chosen for the LDS
// STORE: ds_write_b128 is served 8 lanes (128 bytes = all 32 banks) at a time, so 8 consecutive lanes must write 8 pieces that
// are distinct mod 128 bytes.  With the 208-byte row stride (13 pieces: odd, which is what keeps the ds_read_b128 fragment
// reads conflict-free) the earlier 4-lanes-per-row map put (row r, piece 0) and (row r+1, piece 3) on the same banks in
// every group -- a 2-way conflict on every staging store (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.25,
// profiles/r01_pmc_sq.csv).  Now: slots 0 .. 2 RI - 1: 8 lanes x 16 B = the first 128 bytes of ONE row (also a 128-byte
// global-load segment instead of two 64-byte ones); the last RI slots: the remaining 64 bytes of rows r and r + 4 (52 pieces
// apart = 4 mod 8: the two halves interleave).
// The 4-wave variants (RI = 2: MULTI / row-panel / f32, already at 256 VGPRs) keep the 4-lanes-per-row map: six distinct row
// addresses per thread pushed their hot loop into scratch (8 -> 104 bytes per lane for the multi-output forward).
template <int RI>
__device__ __forceinline__ void nt_map(int tid, int slot, int& row, int& vec) {
    constexpr int NT = 512 / RI;
    if constexpr (RI == 2) {
        row = (tid >> 2) + (slot & 1) * 64;
        vec = (tid & 3) + 4 * (slot >> 1);
    } else if (slot < 2 * RI) {
        const int idx = tid + NT * slot;  // 0 .. 1023
        row = idx >> 3;
        vec = idx & 7;
    } else {
        const int idx = tid + NT * (slot - 2 * RI);  // 0 .. 511
        const int g = idx >> 3, l = idx & 7;
        row = (g >> 2) * 8 + (g & 3) + 4 * (l >> 2);
        vec = 8 + (l & 3);
    }
}

template <typename T, int RI>
struct TileRegs {
    u32x4 w[3 * RI], a[3 * RI];
    int mask;  // dropout keep-mask still to be applied to a[] (done at LDS-store time: applying it at load time
    int k0;    // would put an s_waitcnt vmcnt(0) behind every single load and serialise the tile's loads)
};

// stage one 128-row x ROWB-byte k-tile of the weight-like and activation-like operands into registers
template <typename T, bool MS, int RI>
__device__ __forceinline__ void nt_load(TileRegs<T, RI>& rg, int tid, const T* wgt, int64_t ld_w, int w_row0, int w_rows,
                                        const void* act0, NtPtr P, int n_act, int64_t ld_a, int64_t a_row0,
                                        int64_t a_rows, int k0, int k_hi, bool mask, int w_lo = 0) {
    constexpr int VEC = ET<T>::VEC;
    rg.mask = mask ? 1 : 0;
    rg.k0 = k0;
#pragma unroll
    for (int sl = 0; sl < 3 * RI; ++sl) {
        int r, v;
        nt_map<RI>(tid, sl, r, v);
        const int k = k0 + v * VEC;
        const bool kin = k < k_hi;
        const int wr = w_row0 + r;
        const bool wok = wr < w_rows && wr >= w_lo;
        rg.w[sl] = (kin && wok) ? *reinterpret_cast<const u32x4*>(wgt + (int64_t)wr * ld_w + k) : u32x4{0u, 0u, 0u, 0u};
        const int64_t ar = a_row0 + r;
        const bool aok = ar < a_rows && act0 != nullptr;
        const int64_t aoff = ar * ld_a;
        if (kin && aok) {
            u32x4 x = *reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(act0) + aoff + k);
            if (MS && n_act > 1) {
                if constexpr (sizeof(T) == 4) {
                    f32x4 fx = __builtin_bit_cast(f32x4, x);
#pragma unroll
                    for (int s = 1; s < MAXO; ++s) {
                        if (s < n_act) fx += *reinterpret_cast<const f32x4*>(reinterpret_cast<const T*>(P->act[s]) + aoff + k);
                    }
                    x = __builtin_bit_cast(u32x4, fx);
                } else {
                    float f[8];
                    VOps<T>::unpack(x, f);
#pragma unroll
                    for (int s = 1; s < MAXO; ++s) {
                        if (s < n_act) {
                            const u32x4 y = *reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(P->act[s]) + aoff + k);
                            float g[8];
                            VOps<T>::unpack(y, g);
#pragma unroll
                            for (int e = 0; e < 8; ++e) f[e] += g[e];
                        }
                    }
                    x = VOps<T>::pack(f);
                }
            }
            rg.a[sl] = x;
        } else {
            rg.a[sl] = u32x4{0u, 0u, 0u, 0u};
        }
    }
}

template <typename T, int RI>
__device__ __forceinline__ void nt_store_lds(TileRegs<T, RI>& rg, int tid, unsigned char* sW, unsigned char* sA,
                                             const DropoutCfg& dc, int64_t a_row0) {
    constexpr int VEC = ET<T>::VEC;
#pragma unroll
    for (int sl = 0; sl < 3 * RI; ++sl) {
        int r, v;
        nt_map<RI>(tid, sl, r, v);
        if (rg.mask) {  // wave-uniform
            const uint32_t rh = mtl_dropout_rowhash(dc, 0u, (uint32_t)(a_row0 + r));
            VOps<T>::drop(rg.a[sl], dc, rh, (uint32_t)(rg.k0 + v * VEC));
        }
        *reinterpret_cast<u32x4*>(sW + r * LDSB + v * 16) = rg.w[sl];
        *reinterpret_cast<u32x4*>(sA + r * LDSB + v * 16) = rg.a[sl];
    }
}

// multiply the staged tile; k_left = elements of the part's k range still ahead (sub-tiles past it are all zero
// and skipped -- wave-uniform)
// SM = 32-row m sub-blocks per wave: 2 (4 waves, wave tile 64 n x 64 m) or 1 (8 waves, wave tile 64 n x 32 m)
template <typename T, int SM>
__device__ __forceinline__ void nt_compute(f32x16 (&acc)[2][SM], const unsigned char* sW, const unsigned char* sA,
                                           int lane, int wn, int wm, int k_left, int a_stride = LDSB) {
    constexpr int KS = 64 / (int)sizeof(T);  // elements per 64-byte sub-tile
    const int h = lane >> 5, rl = lane & 31;
#pragma unroll
    for (int t = 0; t < SUBT; ++t) {
        if (t * KS >= k_left) break;
        Frag<T> fw[2], fa[SM];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const unsigned char* pw = sW + (wn * 64 + s * 32 + rl) * LDSB + t * 64;
            fw[s].v[0] = *reinterpret_cast<const u32x4*>(pw + h * 16);
            fw[s].v[1] = *reinterpret_cast<const u32x4*>(pw + (2 + h) * 16);
        }
#pragma unroll
        for (int s = 0; s < SM; ++s) {
            const unsigned char* pa = sA + (wm * (32 * SM) + s * 32 + rl) * a_stride + t * 64;
            fa[s].v[0] = *reinterpret_cast<const u32x4*>(pa + h * 16);
            fa[s].v[1] = *reinterpret_cast<const u32x4*>(pa + (2 + h) * 16);
        }
#pragma unroll
        for (int sn = 0; sn < 2; ++sn)
#pragma unroll
            for (int sm = 0; sm < SM; ++sm) mtl_mma(fw[sn], fa[sm], acc[sn][sm]);
    }
}

// ------------------------------------------------------------------------------------------------
// k_nt: one software-pipelined TILE STREAM per workgroup.
// The k-tiles of the base GEMM and of every output's rank segment are consumed as ONE sequence: the register
// prefetch of tile i+1 is issued before tile i is multiplied, ACROSS the boundaries between base / outputs, so a
// workgroup pays the global->LDS latency once instead of once per output (with K = 96 a base GEMM is only
// 3 k-tiles; cold starts per output were the dominant cost).
//   MULTI  (forward with task outputs):  base | out0: base+lr0 | out1: base+lr1 ...   (base kept in registers)
//   lean   (everything else):            per output: lr_o -> [mask] -> base -> store   (ONE accumulator set:
//          the low-rank part is formed first so the dropout mask of dX = G W + keep.(Q A) applies to it alone)
// ------------------------------------------------------------------------------------------------
struct NtCursor {
    int q;         // index in the part sequence
    int k0;        // current k-tile origin
    int k_hi;      // end of the part's k range
    int lr;        // 1: rank-segment part (L x Rm), 0: base part (act x wgt)
    int valid;
    int bn;        // n-tile of the workgroup
};

__device__ __forceinline__ NtOut nt_out(NtPtr P, int o) {
    NtOut O;
    O.ptr = P->out[o].ptr;
    O.seg_lo = P->out[o].seg_lo;
    O.seg_hi = P->out[o].seg_hi;
    O.use_base = P->out[o].use_base;
    O.mask_lr = P->out[o].mask_lr;
    O.fold = P->out[o].fold;
    O.gate = P->out[o].gate;
    O.act = P->out[o].act;
    return O;
}

// k range of part q.  MULTI: q = 0 base, q = 1 + o rank segment of output o.
// lean: q = 2 o rank segment of output o, q = 2 o + 1 base (if that output uses it).
template <bool MULTI>
__device__ __forceinline__ void nt_part(NtPtr P, int q, int& lr, int& k_lo, int& k_hi) {
    if (MULTI) {
        if (q == 0) {
            lr = 0;
            k_lo = 0;
            k_hi = P->K;
        } else {
            const NtOut O = nt_out(P, q - 1);
            lr = 1;
            k_lo = O.seg_lo;
            k_hi = O.seg_hi;
        }
    } else {
        const NtOut O = nt_out(P, q >> 1);
        if (q & 1) {
            lr = 0;
            k_lo = 0;
            k_hi = O.use_base ? P->K : 0;
        } else {
            lr = 1;
            k_lo = O.seg_lo;
            k_hi = O.seg_hi;
        }
    }
}

template <bool MULTI>
__device__ __forceinline__ NtCursor nt_seek(NtPtr P, int q, int nseq, int bn) {
    NtCursor c;
    c.valid = 0;
    c.q = q;
    c.k0 = c.k_hi = c.lr = 0;
    c.bn = bn;
    for (; q < nseq; ++q) {
        int lr, lo, hi;
        nt_part<MULTI>(P, q, lr, lo, hi);
        if (hi > lo) {
            c.q = q;
            c.k0 = lo;
            c.k_hi = hi;
            c.lr = lr;
            c.valid = 1;
            return c;
        }
    }
    return c;
}

// MLR: some output masks its low-rank part (dX = G W + keep .* (Q A)).  A template parameter, not a runtime test: the
// keep-mask hashes depend only on (m, n), so the compiler hoists all 64 of them (+ their SGPR-pair results, spilled to
// VGPR lanes) to the top of the kernel -- ~700 instructions per workgroup that the forward / P / Q launches never use.
// NW = waves per workgroup.  The 128 x 128 tile is unchanged; with 8 waves a wave owns 64 n x 32 m (half the
// accumulators, half the staging registers, half the loads / LDS traffic / MFMAs per step), fits 128 VGPRs and runs
// 4 waves per SIMD instead of 2 -- the kernel is latency- and issue-bound, not bandwidth-bound.
template <typename T, bool MULTI, bool MS, bool MLR, int NW, bool GATE = false, bool ACT = false>
__global__ __launch_bounds__(64 * NW, NW == 4 ? 2 : 4) void k_nt(const NtParams Pv) {
    constexpr int SM = 8 / NW;       // 32-row m sub-blocks per wave
    constexpr int MW = 32 * SM;      // m rows per wave
    constexpr int NT = 64 * NW;      // threads
    (void)Pv;
    NtPtr P = (NtPtr)__builtin_amdgcn_kernarg_segment_ptr();
    constexpr int KE = ROWB / (int)sizeof(T);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];  // staging (2 x 128 x LDSB)
    unsigned char* sW = smem;
    unsigned char* sA = smem + TILE * LDSB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = NW == 4 ? wave >> 1 : wave >> 2, wm = NW == 4 ? wave & 1 : wave & 3;

    // batched form
    const void* act0 = P->act[0];
    int row_off = 0, n_rows = P->n_rows;
    bool act_mask = P->act_mask != 0;
    if (P->nz > 0) {
        const int z = blockIdx.z;
        act0 = P->zact[z];
        row_off = P->zrow0[z];
        n_rows = P->zrows[z];
        act_mask = P->zmask[z] != 0;
    }
    if (n_rows <= 0) return;
    act_mask = act_mask && P->drop.thr16 != 0;

    // XCD-aware tile order: hardware places block b on XCD b % 8; give every XCD a contiguous run of
    // logical tiles so that the n-tiles sharing one activation row-block hit the same L2 (T1, bijective).
    const int n_tiles = (n_rows + TILE - 1) / TILE;
    const int64_t m_tiles = (P->M + TILE - 1) / TILE;
    const int64_t nwg = m_tiles * n_tiles;
    int64_t b = blockIdx.x;
    if (b >= nwg) return;
    {
        const int64_t q = nwg / 8, r = nwg % 8, xcd = b % 8;
        b = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + b / 8;
    }
    const int64_t bm = b / n_tiles;
    const int bn0 = (int)(b % n_tiles);
    const int64_t m0 = bm * TILE;
    const int n0 = bn0 * TILE;

    const T* wgt = reinterpret_cast<const T*>(P->wgt) + (int64_t)row_off * P->ld_wgt;
    DropoutCfg drop;
    drop.seed_lo = P->drop.seed_lo;
    drop.seed_hi = P->drop.seed_hi;
    drop.thr16 = P->drop.thr16;
    drop.off = P->drop.off;
    mtl_dropout_resolve(drop);
    const int nseq = MULTI ? 1 + P->n_out : 2 * P->n_out;

    // ---- loader side of the stream (register prefetch, one wide tile ahead)
    TileRegs<T, SM> rg;
    NtCursor ld = nt_seek<MULTI>(P, 0, nseq, bn0);
    auto issue = [&](const NtCursor& c) __attribute__((always_inline)) {
        if (c.lr)  // rank segment: weights = Rm, activation = L
            nt_load<T, false, SM>(rg, tid, reinterpret_cast<const T*>(P->Rm), P->ldR, c.bn * TILE, n_rows, P->L, P, 1, P->ldL, m0, P->M, c.k0,
                                  c.k_hi, false);
        else
            nt_load<T, MS, SM>(rg, tid, wgt, P->ld_wgt, c.bn * TILE, n_rows, act0, P, P->n_act, P->ld_act, m0, P->M, c.k0, c.k_hi, act_mask);
    };
    if (ld.valid) issue(ld);
    // consume one tile: registers -> LDS, prefetch the next tile of the stream, multiply
    auto step = [&](f32x16(&acc)[2][SM], int k_left) __attribute__((always_inline)) {
        nt_store_lds<T, SM>(rg, tid, sW, sA, drop, m0);
        __syncthreads();
        ld.k0 += KE;
        if (ld.k0 >= ld.k_hi) ld = nt_seek<MULTI>(P, ld.q + 1, nseq, bn0);
        if (ld.valid) issue(ld);
        // a wave whose 64 output columns lie entirely past n_rows (P / Q passes: <= 64 of the tile's 128 columns exist)
        // only helps staging: no LDS fragment reads, no MFMAs (wave-uniform test)
        if (n0 + wn * 64 < n_rows) nt_compute<T, SM>(acc, sW, sA, lane, wn, wm, k_left);
        __syncthreads();
    };
    auto run_part = [&](int q, f32x16(&acc)[2][SM]) __attribute__((always_inline)) {
        int lr, lo, hi;
        nt_part<MULTI>(P, q, lr, lo, hi);
        for (int k0 = lo; k0 < hi; k0 += KE) step(acc, hi - k0);
        return hi > lo;
    };
    auto zero = [](f32x16(&a)[2][SM]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < SM; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) a[i][j][r] = 0.f;
    };
    // acc = acc * alpha[n] + bias[n]
    auto affine = [&](f32x16(&a)[2][SM]) __attribute__((always_inline)) {
        if (!(P->alpha || P->bias)) return;
#pragma unroll
        for (int sn = 0; sn < 2; ++sn)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = n0 + wn * 64 + sn * 32 + 8 * q + 4 * (lane >> 5);
                if (n < n_rows) {
                    f32x4 al = {1.f, 1.f, 1.f, 1.f}, bi = {0.f, 0.f, 0.f, 0.f};
                    if (P->alpha) al = *reinterpret_cast<const f32x4*>(P->alpha + row_off + n);
                    if (P->bias) bi = *reinterpret_cast<const f32x4*>(P->bias + row_off + n);
#pragma unroll
                    for (int sm = 0; sm < SM; ++sm)
#pragma unroll
                        for (int e = 0; e < 4; ++e) a[sn][sm][q * 4 + e] = a[sn][sm][q * 4 + e] * al[e] + bi[e];
                }
            }
    };
    // acc *= keep(m, n)
    auto apply_mask = [&](f32x16(&a)[2][SM]) __attribute__((always_inline)) {
#pragma unroll
        for (int sm = 0; sm < SM; ++sm) {
            const int64_t m = m0 + wm * MW + sm * 32 + (lane & 31);
            const uint32_t rh = mtl_dropout_rowhash(drop, 0u, (uint32_t)m);
#pragma unroll
            for (int sn = 0; sn < 2; ++sn)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int n = n0 + wn * 64 + sn * 32 + 8 * q + 4 * (lane >> 5);
                    const uint32_t h0 = mtl_dropout_pairbits(drop, rh, (uint32_t)n);
                    const uint32_t h1 = mtl_dropout_pairbits(drop, rh, (uint32_t)(n + 2));
                    if ((h0 & 0xFFFFu) < drop.thr16) a[sn][sm][q * 4 + 0] = 0.f;
                    if ((h0 >> 16) < drop.thr16) a[sn][sm][q * 4 + 1] = 0.f;
                    if ((h1 & 0xFFFFu) < drop.thr16) a[sn][sm][q * 4 + 2] = 0.f;
                    if ((h1 >> 16) < drop.thr16) a[sn][sm][q * 4 + 3] = 0.f;
                }
        }
    };
    auto store = [&](const f32x16(&a)[2][SM], void* ptr, const void* gate_ptr, void* act_ptr) __attribute__((always_inline)) {
        T* outp = reinterpret_cast<T*>(ptr);
        const T* gate = reinterpret_cast<const T*>(gate_ptr);
        T* actp = reinterpret_cast<T*>(act_ptr);
        (void)gate;
        (void)actp;
        if (!outp || n0 + wn * 64 >= n_rows) return;  // (the per-wave LDS image needs no workgroup barrier)
        if constexpr (sizeof(T) == 2) {
            // bf16: transpose the wave's 64(n) x 64(m) accumulator tile through LDS so that every store instruction
            // writes whole 128-byte row segments (8 lanes x 16 B) instead of 16-byte pieces of 32 different rows.
            // The staging buffers are idle here (the trailing barrier of the last tile has passed).
            constexpr int ORS = EPI_ROW;  // row stride of the per-wave image (bytes): 2-way conflicts at most
            unsigned char* img = smem + wave * (MW * ORS);
#pragma unroll
            for (int sm = 0; sm < SM; ++sm)
#pragma unroll
                for (int sn = 0; sn < 2; ++sn)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int ml = sm * 32 + (lane & 31), nl = sn * 32 + 8 * q + 4 * (lane >> 5);
                        u32x2 pk = {mtl_pack2<T>(a[sn][sm][q * 4], a[sn][sm][q * 4 + 1]),
                                    mtl_pack2<T>(a[sn][sm][q * 4 + 2], a[sn][sm][q * 4 + 3])};
                        *reinterpret_cast<u32x2*>(img + ml * ORS + nl * 2) = pk;
                    }
            __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the image is private to this wave, no barrier needed
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int it = 0; it < 4 * SM; ++it) {
                const int ml = it * 8 + (lane >> 3), c16 = lane & 7;
                const int64_t m = m0 + wm * MW + ml;
                const int n = n0 + wn * 64 + c16 * 8;
                u32x4 v = *reinterpret_cast<const u32x4*>(img + ml * ORS + c16 * 16);
                if (m < P->M && n < n_rows) {
                    if constexpr (GATE) {
                        if (gate) {  // the bf16-rounded gradient times gelu'(pre-activation), rounded once (as ATen does)
                            const u32x4 hv = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(gate + m * P->ld_out + row_off + n));
                            v = mtl_gelu_gate_pk4<T, false>(v, hv);
                        }
                    }
                    // non-temporal: the 77 - 308 MB outputs of a launch outlive L2 / MALL anyway (+1 % on the step; the same hint
                    // on the glue kernels' stores costs 1.5 %: their consumers do hit in cache)
                    __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(outp + m * P->ld_out + row_off + n));
                    if constexpr (ACT) {
                        if (actp) {  // second output: GELU of the bf16-rounded value, rounded once (ATen's gelu on the bf16 tensor)
                            const u32x4 av = mtl_gelu_pk4<T, false>(v);
                            __builtin_nontemporal_store(av, reinterpret_cast<u32x4*>(actp + m * P->ld_out + row_off + n));
                        }
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
        } else {
#pragma unroll
            for (int sm = 0; sm < SM; ++sm) {
                const int64_t m = m0 + wm * MW + sm * 32 + (lane & 31);
#pragma unroll
                for (int sn = 0; sn < 2; ++sn)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int n = n0 + wn * 64 + sn * 32 + 8 * q + 4 * (lane >> 5);
                        if (m < P->M && n < n_rows) {
                            T* dst = outp + m * P->ld_out + row_off + n;
                            f32x4 o4 = {a[sn][sm][q * 4], a[sn][sm][q * 4 + 1], a[sn][sm][q * 4 + 2], a[sn][sm][q * 4 + 3]};
                            if constexpr (GATE) {
                                if (gate) {
                                    const f32x4 hv = *reinterpret_cast<const f32x4*>(gate + m * P->ld_out + row_off + n);
#pragma unroll
                                    for (int e = 0; e < 4; ++e) o4[e] *= gelu_grad(hv[e]);
                                }
                            }
                            *reinterpret_cast<f32x4*>(dst) = o4;
                            if constexpr (ACT) {
                                if (actp) {
                                    f32x4 a4;
#pragma unroll
                                    for (int e = 0; e < 4; ++e) a4[e] = gelu_fwd(o4[e]);
                                    *reinterpret_cast<f32x4*>(actp + m * P->ld_out + row_off + n) = a4;
                                }
                            }
                        }
                    }
            }
        }
    };

    if constexpr (MULTI) {
        f32x16 base[2][SM], acc[2][SM];
        zero(base);
        run_part(0, base);
        affine(base);
        for (int o = 0; o < P->n_out; ++o) {
            const NtOut O = nt_out(P, o);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < SM; ++j) acc[i][j] = base[i][j];
            run_part(1 + o, acc);
            if (O.fold) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < SM; ++j) base[i][j] = acc[i][j];
            }
            store(acc, O.ptr, O.gate, O.act);
            __syncthreads();  // the output image lives in the staging buffers
        }
    } else {
        f32x16 acc[2][SM];
        for (int o = 0; o < P->n_out; ++o) {
            const NtOut O = nt_out(P, o);
            zero(acc);
            const bool had_lr = run_part(2 * o, acc);
            if constexpr (MLR) {
                if (had_lr && O.mask_lr && drop.enabled()) apply_mask(acc);
            } else {
                (void)had_lr;
            }
            run_part(2 * o + 1, acc);
            if (O.use_base) affine(acc);
            store(acc, O.ptr, O.gate, O.act);
            __syncthreads();  // the output image lives in the staging buffers
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_ntl : the lean bf16 launches of k_nt (ONE output, one activation source, no batched / row-panel form: every P / Q pass,
// every T = 0 forward and dX) as straight-line code.
// Why a second kernel: an ablation of k_nt (profiles/r02_nt_ablate.txt; profiles/DESIGN_history_r01_r05.md 4.1c) showed that with
// loads, MFMAs, stores and the epilogue all switched OFF the s0.qkv forward still took 100 of its 164 us -- the generic
// kernel's bookkeeping.  Its prologue is a chain of ~15 DEPENDENT scalar loads from the 1 KB parameter block (each followed by
// s_waitcnt lgkmcnt(0)), three software 64-bit divisions (~130 SALU instructions each) for the XCD map, a part-sequence cursor
// that re-reads the output table per step, and every global load sits in its own exec-masked branch.  With only 2 - 4 k-steps
// per workgroup nothing amortises that.  Here:
//   * a compact parameter block (~200 B) read once; the XCD map and tile decomposition use 32-bit arithmetic and a host-side
//     magic multiplier instead of divisions;
//   * the step sequence is [rank-segment k-tiles | base k-tiles], both counts known up front: no cursor;
//   * loads are unconditional: out-of-range rows are CLAMPED (their products land in rows / columns that are never stored)
//     and out-of-range k vectors read a 16-byte zero page -- address selects, no branches;
//   * the bias is the accumulator's initial value (its loads overlap the first tile's) instead of a dependent load + FMA pass
//     after the last MFMA.
// Tile geometry, LDS layout, fragment reads and the transposing epilogue are k_nt's 8-wave variant (128 x 128 x 96, wave tile
// 64 n x 32 m), so results are bit-identical to k_nt's.
// ------------------------------------------------------------------------------------------------
__device__ __attribute__((aligned(16))) const uint32_t g_zero16[4] = {0u, 0u, 0u, 0u};

struct NlParams {
    const bf16* act;    // (M x K) activation-like operand of the base part
    const bf16* wgt;    // (n_rows x K)
    const bf16* L;      // (M x ldL) activation-like operand of the rank part
    const bf16* Rm;     // (n_rows x ldR)
    bf16* out;          // (M x ld_out)
    bf16* act2;         // ACT: second output gelu(out)
    const bf16* gate;   // GATE (k_ntd): out *= gelu'(gate[m][n]), same layout as out
    const float* bias;  // per output column, nullable
    const float* alpha; // per output column multiplier, nullable
    int64_t ld_act, ld_wgt, ldL, ldR, ld_out;
    int M, n_rows, K, seg_lo, seg_hi;
    int n_tiles;
    uint32_t nt_magic;  // floor(2^32 / n_tiles) + 1: b / n_tiles == umulhi(b, nt_magic) for b * n_tiles < 2^32 (n_tiles > 1)
    uint32_t q8, r8;    // workgroups / 8, workgroups % 8 (XCD map)
    int act_mask, use_base;
    DropoutCfg drop;
};

// SN = 32-column sub-blocks per wave: 2 (128 x 128 tile) or 3 (128 rows x 192 columns).  The wide tile exists for the launches
// whose 128 x 128 tile count lands just above a whole number of residency rounds (2 workgroups per CU = 512 slots): the
// N = 384 outputs of stage 2 (196 x 3 = 588 tiles = 1.15 rounds -> 2 rounds, the second one 15 % full) run as 196 x 2 = 392
// tiles of 1.5x the work in ONE round.  MLR: the low-rank part (rank tiles come first in the stream) is multiplied by the dropout
// keep-mask of (m, n) before the base tiles are added -- the dX launches (dX = keep .* (Q A) + dY W).
template <bool ACT, bool MLR, int SN>
__global__ __launch_bounds__(512, 4) void k_ntl(const NlParams P) {
    constexpr int KE = ROWB / 2;  // 96 elements per staged k-tile
    constexpr int TN = 64 * SN;   // tile columns
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* sW = smem;
    unsigned char* sA = smem + TN * LDSB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave >> 2, wm = wave & 3;

    // XCD-aware tile order (as k_nt): block b runs on XCD b % 8; every XCD gets a contiguous run of logical tiles
    uint32_t b = blockIdx.x;
    {
        const uint32_t xcd = b & 7u, q = P.q8, r = P.r8;
        b = (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + (b >> 3);
    }
    const uint32_t bm = P.n_tiles == 1 ? b : __umulhi(b, P.nt_magic);
    const int bn = (int)(b - bm * (uint32_t)P.n_tiles);
    const int m0 = (int)bm * TILE, n0 = bn * TN;
    const int M = P.M, n_rows = P.n_rows;

    DropoutCfg drop = P.drop;
    mtl_dropout_resolve(drop);
    const bool act_mask = P.act_mask != 0 && drop.thr16 != 0;

    const int n1 = P.seg_hi > P.seg_lo ? (P.seg_hi - P.seg_lo + KE - 1) / KE : 0;
    const int n2 = (P.use_base && P.K > 0) ? (P.K + KE - 1) / KE : 0;
    const int total = n1 + n2;

    f32x16 acc[SN];
    // accumulator start: the bias (when nothing multiplies the sum afterwards and no mask is applied to the running sum)
    const bool bias_first = !MLR && P.bias != nullptr && P.alpha == nullptr && P.use_base != 0;
#pragma unroll
    for (int sn = 0; sn < SN; ++sn)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x4 bi = {0.f, 0.f, 0.f, 0.f};
            if (bias_first) {
                int n = n0 + wn * (32 * SN) + sn * 32 + 8 * q + 4 * (lane >> 5);
                n = n < n_rows - 4 ? n : n_rows - 4;  // (columns >= n_rows are never stored)
                bi = *reinterpret_cast<const f32x4*>(P.bias + n);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[sn][q * 4 + e] = bi[e];
        }

    u32x4 rw[3], rw2[SN == 3 ? 3 : 1], ra[3];  // staged k-tile: weight rows 0..127, weight rows 128..191 (SN = 3), activation rows
    (void)rw2;
    int cur_mask = 0, cur_k0 = 0;  // of the tile sitting in the registers
    auto issue = [&](int i) __attribute__((always_inline)) {
        const bool lr = i < n1;
        const bf16* wp = lr ? P.Rm : P.wgt;
        const bf16* ap = lr ? P.L : P.act;
        const int64_t ldw = lr ? P.ldR : P.ld_wgt, lda = lr ? P.ldL : P.ld_act;
        const int k0 = lr ? P.seg_lo + i * KE : (i - n1) * KE;
        const int khi = lr ? P.seg_hi : P.K;
        cur_mask = (!lr && act_mask) ? 1 : 0;
        cur_k0 = k0;
        const bf16* zp = reinterpret_cast<const bf16*>(g_zero16);
#pragma unroll
        for (int sl = 0; sl < 3; ++sl) {
            int r, v;
            nt_map<1>(tid, sl, r, v);
            const int k = k0 + v * 8;
            const bool kin = k < khi;
            int wr = n0 + r, ar = m0 + r;
            wr = wr < n_rows ? wr : n_rows - 1;
            ar = ar < M ? ar : M - 1;
            rw[sl] = *reinterpret_cast<const u32x4*>(kin ? wp + (int64_t)wr * ldw + k : zp);
            ra[sl] = *reinterpret_cast<const u32x4*>(kin ? ap + (int64_t)ar * lda + k : zp);
            if constexpr (SN == 3) {  // weight rows 128 .. 191: the same map on a second 128-row panel, upper half unused
                int wr2 = n0 + 128 + r;
                wr2 = wr2 < n_rows ? wr2 : n_rows - 1;
                if (r < 64) rw2[sl] = *reinterpret_cast<const u32x4*>(kin ? wp + (int64_t)wr2 * ldw + k : zp);
            }
        }
    };
    auto stage = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int sl = 0; sl < 3; ++sl) {
            int r, v;
            nt_map<1>(tid, sl, r, v);
            if (cur_mask) {  // uniform
                const uint32_t rh = mtl_dropout_rowhash(drop, 0u, (uint32_t)(m0 + r));
                VOps<bf16>::drop(ra[sl], drop, rh, (uint32_t)(cur_k0 + v * 8));
            }
            *reinterpret_cast<u32x4*>(sW + r * LDSB + v * 16) = rw[sl];
            *reinterpret_cast<u32x4*>(sA + r * LDSB + v * 16) = ra[sl];
            if constexpr (SN == 3) {
                if (r < 64) *reinterpret_cast<u32x4*>(sW + (128 + r) * LDSB + v * 16) = rw2[sl];
            }
        }
    };
    auto compute = [&](int k_left) __attribute__((always_inline)) {
        const int h = lane >> 5, rl = lane & 31;
#pragma unroll
        for (int t = 0; t < SUBT; ++t) {
            if (t * 32 >= k_left) break;
            Frag<bf16> fw[SN], fa;
#pragma unroll
            for (int sn = 0; sn < SN; ++sn) {
                const unsigned char* pw = sW + (wn * (32 * SN) + sn * 32 + rl) * LDSB + t * 64;
                fw[sn].v[0] = *reinterpret_cast<const u32x4*>(pw + h * 16);
                fw[sn].v[1] = *reinterpret_cast<const u32x4*>(pw + (2 + h) * 16);
            }
            const unsigned char* pa = sA + (wm * 32 + rl) * LDSB + t * 64;
            fa.v[0] = *reinterpret_cast<const u32x4*>(pa + h * 16);
            fa.v[1] = *reinterpret_cast<const u32x4*>(pa + (2 + h) * 16);
#pragma unroll
            for (int sn = 0; sn < SN; ++sn) mtl_mma(fw[sn], fa, acc[sn]);
        }
    };
    const bool wave_live = n0 + wn * (32 * SN) < n_rows;  // P / Q passes: a wave whose columns do not exist only helps staging
    if (total > 0) issue(0);
    for (int i = 0; i < total; ++i) {
        const bool lr = i < n1;
        const int k_left = lr ? P.seg_hi - (P.seg_lo + i * KE) : P.K - (i - n1) * KE;
        stage();
        __syncthreads();
        if (i + 1 < total) issue(i + 1);
        if (wave_live) compute(k_left);
        if constexpr (MLR) {
            if (i + 1 == n1 && wave_live && drop.thr16 != 0) {  // the rank part is complete: acc *= keep(m, n)
                const uint32_t rh = mtl_dropout_rowhash(drop, 0u, (uint32_t)(m0 + wm * 32 + (lane & 31)));
#pragma unroll
                for (int sn = 0; sn < SN; ++sn)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int n = n0 + wn * (32 * SN) + sn * 32 + 8 * q + 4 * (lane >> 5);
                        const uint32_t h0 = mtl_dropout_pairbits(drop, rh, (uint32_t)n);
                        const uint32_t h1 = mtl_dropout_pairbits(drop, rh, (uint32_t)(n + 2));
                        if ((h0 & 0xFFFFu) < drop.thr16) acc[sn][q * 4 + 0] = 0.f;
                        if ((h0 >> 16) < drop.thr16) acc[sn][q * 4 + 1] = 0.f;
                        if ((h1 & 0xFFFFu) < drop.thr16) acc[sn][q * 4 + 2] = 0.f;
                        if ((h1 >> 16) < drop.thr16) acc[sn][q * 4 + 3] = 0.f;
                    }
            }
        }
        __syncthreads();
    }
    if (!wave_live) return;

    if (!bias_first && (P.alpha || P.bias) && P.use_base) {  // acc = acc * alpha[n] + bias[n]
#pragma unroll
        for (int sn = 0; sn < SN; ++sn)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                int n = n0 + wn * (32 * SN) + sn * 32 + 8 * q + 4 * (lane >> 5);
                n = n < n_rows - 4 ? n : n_rows - 4;
                f32x4 al = {1.f, 1.f, 1.f, 1.f}, bi = {0.f, 0.f, 0.f, 0.f};
                if (P.alpha) al = *reinterpret_cast<const f32x4*>(P.alpha + n);
                if (P.bias) bi = *reinterpret_cast<const f32x4*>(P.bias + n);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[sn][q * 4 + e] = acc[sn][q * 4 + e] * al[e] + bi[e];
            }
    }

    // epilogue: transpose the wave's (32 SN) (n) x 32 (m) tile through a private LDS image -> whole row-segment stores
    {
        constexpr int ORS = 64 * SN + 8;       // image row stride (bytes)
        constexpr int CPRW = 4 * SN;           // 16-byte chunks per image row
        unsigned char* img = smem + wave * (32 * ORS);
#pragma unroll
        for (int sn = 0; sn < SN; ++sn)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ml = lane & 31, nl = sn * 32 + 8 * q + 4 * (lane >> 5);
                u32x2 pk = {mtl_pack_bf16(acc[sn][q * 4], acc[sn][q * 4 + 1]), mtl_pack_bf16(acc[sn][q * 4 + 2], acc[sn][q * 4 + 3])};
                *reinterpret_cast<u32x2*>(img + ml * ORS + nl * 2) = pk;
            }
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the image is private to this wave
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int it = 0; it < 2 * SN; ++it) {
            const int idx = it * 64 + lane;
            const int ml = idx / CPRW, c16 = idx - ml * CPRW;
            const int m = m0 + wm * 32 + ml;
            const int n = n0 + wn * (32 * SN) + c16 * 8;
            u32x4 v = *reinterpret_cast<const u32x4*>(img + ml * ORS + c16 * 16);
            if (m < M && n < n_rows) {
                const int64_t o = (int64_t)m * P.ld_out + n;
                __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(P.out + o));
                if constexpr (ACT) {
                    if (P.act2) {
                        const u32x4 av = mtl_gelu_pk4<bf16, false>(v);
                        __builtin_nontemporal_store(av, reinterpret_cast<u32x4*>(P.act2 + o));
                    }
                }
            }
        }
    }
}

}  // namespace
