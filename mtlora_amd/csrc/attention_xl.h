// attention_xl.h -- window attention core for 144 < N = ws*ws <= 256 (ws 13..16), forward and backward, and the relative-position
// bias gather / scatter these windows use instead of the one-hot product.
// Included by attention.hip inside its anonymous namespace, after attention_wide.h: token addressing, LDS image geometry (N token rows
// + the shared zero row), fragment readers, accumulator-fed operands (accfrag / wide_mma_col) and the whole-row store path are shared.
//
// Keys and queries are padded to eight 32-token tiles.  The N <= 144 design (one workgroup, four images, dbias next to P^T in one wave)
// does not stretch this far, so the work is split by OWNERSHIP:
//   forward   k_attn_xl_fwd:  one workgroup per (window, head), 8 waves = one per 32-query block (blocks past N idle through the
//             barriers).  Q / K / V staged once in LDS; a wave holds S^T of its block against all keys as 8 accumulator tiles (128
//             registers, two waves on a SIMD), softmax over keys in the wave, O^T = V^T P^T.  No cross-wave traffic.
//   backward  two launches of 4-wave workgroups (one wave per SIMD, the whole register file); a workgroup takes every second 32-token
//             block of a window (blocks 2 wave + half) and walks its windows persistently.
//     k_attn_xl_bwd_q (wave = query block): K and V in LDS, its own Q / dO block straight from memory as MFMA fragments.  P^T (8 tiles),
//             D = sum_j P dP, dS^T tile by tile -> dbias (8 more tiles, accumulated in REGISTERS over the workgroup's windows) and
//             dQ^T = K^T dS^T.  Row maximum, 1 / sum and D go to a global statistics buffer of 3 N floats per (window, head).
//     k_attn_xl_bwd_k (wave = key block): Q and dO in LDS, its own K / V block as fragments.  S, P, dP recomputed in the other
//             orientation from the statistics -> dK^T = Q^T dS, dV^T = dO^T P.
// Every output element has exactly one owning lane; no atomics, no memset, no float accumulated across waves; the dbias partials are
// combined in fixed order by k_dbias_reduce.  Padded keys get probability exactly 0 by a select and stay out of the row maximum; padded
// queries are never stored and reach dK / dV / dbias as exact zeros (their Q / dO fragments are zero).  Bias and dense mask are added
// in fp32 straight from memory for every dtype.

constexpr int XT = 8;  // 32-token tiles: keys / queries padded to 256
constexpr int XN = 32 * XT;
constexpr int XF_THREADS = 64 * XT;  // forward: one wave per query block
constexpr int XB_WAVES = 4;          // backward: one wave per SIMD; a workgroup owns blocks 2 wave + half
constexpr int XB_THREADS = 64 * XB_WAVES;
constexpr int XL_MAX_N = XN;

struct XlParams : AttnParams {
    float* stats;  // [window][head][3][N]: row maximum, 1 / sum, D
};

// the 32 rows of block `blk` as the row operand of a product over head_dim: from an LDS image ...
template <typename T>
__device__ __forceinline__ void xl_lfrag(Frag<T> (&f)[AC<T>::KT_D], const unsigned char* img, int blk, int lane, int N) {
#pragma unroll
    for (int kt = 0; kt < AC<T>::KT_D; ++kt) f[kt] = rowfrag<T>(img, blk, kt, lane, N);
}
// ... or straight from memory (base: workgroup-uniform pointer at the head's slice, tokoff: the tokens' element offsets).  Same slot
// order as rowfrag; rows past N are zero, as the shared zero row of an image
template <typename T>
__device__ __forceinline__ void xl_gfrag(Frag<T> (&f)[AC<T>::KT_D], const T* base, const int* tokoff, int blk, int lane, int N) {
    const int row = blk * 32 + (lane & 31), h = lane >> 5;
    const bool v = row < N;
    const unsigned char* src = reinterpret_cast<const unsigned char*>(base + (uint32_t)tokoff[v ? row : 0]);
#pragma unroll
    for (int kt = 0; kt < AC<T>::KT_D; ++kt) {
        const u32x4 a = *reinterpret_cast<const u32x4*>(src + kt * 64 + h * 16);
        const u32x4 b = *reinterpret_cast<const u32x4*>(src + kt * 64 + (2 + h) * 16);
        f[kt].v[0] = v ? a : u32x4{0u, 0u, 0u, 0u};
        f[kt].v[1] = v ? b : u32x4{0u, 0u, 0u, 0u};
    }
}
// out[row of image tile ta][row of fb (lane)] += sum_d img[ta][d] * fb[d]
template <typename T>
__device__ __forceinline__ void xl_mma_rowf(f32x16& out, const unsigned char* img, int ta, const Frag<T> (&fb)[AC<T>::KT_D], int lane,
                                            int N) {
#pragma unroll
    for (int kt = 0; kt < AC<T>::KT_D; ++kt) {
        Frag<T> fa = rowfrag<T>(img, ta, kt, lane, N);
        mtl_mma(fa, fb[kt], out);
    }
}

__device__ __forceinline__ void xl_tables(const WideTabs& tb, const AttnParams& p, const WinPos& wq, int wm, int my_tyx, int tid) {
    if (tid < XN) {
        const bool v = tid < p.N;
        const int idx = v ? token_at(p, wq, tid, my_tyx) : 0;
        tb.tokC[tid] = idx * p.C;
        tb.tokC3[tid] = idx * 3 * p.C;
        tb.srid[tid] = (p.mask_ids && v) ? p.mask_ids[wm * p.N + tid] : 0;
    }
}
// rows of one (window, head) operand: global -> LDS image, 16 bytes per thread and step
template <typename T, int NT>
__device__ __forceinline__ void xl_stage(unsigned char* img, const T* base, const int* tokoff, int N, int tid) {
    constexpr int VPR = AC<T>::VPR, RS = AC<T>::RS;
    constexpr int IT = (XL_MAX_N * VPR + NT - 1) / NT;
    u32x4 v[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int idx = it * NT + tid;
        const int row = idx / VPR, vec = idx % VPR;
        v[it] = row < N ? *reinterpret_cast<const u32x4*>(base + (uint32_t)(tokoff[row] + vec * ET<T>::VEC)) : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int idx = it * NT + tid;
        const int row = idx / VPR, vec = idx % VPR;
        if (row < N) *reinterpret_cast<u32x4*>(img + row * RS + vec * 16) = v[it];
    }
}

// P^T of query block qb (fq: its Q rows): st[sj][r] = P[query qb*32 + (lane & 31)][key sj*32 + row(r, lane)], normalised; returns the
// row's maximum (m) and 1 / sum (inv) of the logits  q.k * scale + bias (+ mask)
template <typename T, bool DENSE>
__device__ __forceinline__ void xl_probs_t(f32x16 (&st)[XT], float& m_out, float& inv_out, const unsigned char* sK,
                                           const Frag<T> (&fq)[AC<T>::KT_D], int qb, int nt, const AttnParams& p, const float* bias_h,
                                           const int* srid, int wm, int lane) {
    const int N = p.N;
#pragma unroll
    for (int sj = 0; sj < XT; ++sj) {
        zero(st[sj]);
        if (sj < nt) xl_mma_rowf<T>(st[sj], sK, sj, fq, lane, N);
    }
    const int i = qb * 32 + (lane & 31);
    const int ic = i < N ? i : N - 1;
    int h4 = 4 * (lane >> 5);
    uint32_t boff = (uint32_t)(ic * N);
    asm volatile("" : "+v"(h4), "+v"(boff));  // (as wide_probs_t: the 128 element addresses stay out of the persistent loop's live set)
    const uint32_t moff = DENSE ? (uint32_t)((wm * N + ic) * N) : 0u;
    const bool ids = !DENSE && p.mask_ids != nullptr;
    const int rid_i = srid[ic];
    float m = -3.0e38f;
    constexpr int RC = DENSE ? 8 : 16;  // (a dense mask doubles the loads of an element)
    // per-lane row pointers: in a tile whose 32 keys are all real (every tile but the last one in use) an element is a constant offset
    // from them, i.e. an immediate of its load -- no address register per element; only the tile with padded keys clamps
    const float* brow = bias_h + boff + h4;
    const float* mrow = DENSE ? p.mask + moff + h4 : nullptr;
    const int* rrow = srid + h4;
    auto tile = [&](int sj, auto full) __attribute__((always_inline)) {
#pragma unroll
        for (int r0 = 0; r0 < 16; r0 += RC) {
            __builtin_amdgcn_sched_barrier(0);  // RC elements' loads in flight at a time (register pressure)
#pragma unroll
            for (int r = r0; r < r0 + RC; ++r) {
                const int j0 = sj * 32 + (r & 3) + 8 * (r >> 2);  // key j0 + h4
                const bool jv = decltype(full)::value || j0 + h4 < N;
                const int jo = decltype(full)::value ? j0 : (jv ? j0 : N - 1 - h4);
                float add = brow[jo];
                if constexpr (DENSE) add += mrow[jo];
                if (ids) add += rrow[jo] != rid_i ? p.mask_value : 0.f;
                const float v = st[sj][r] * p.scale + add;
                st[sj][r] = v;
                m = jv ? fmaxf(m, v) : m;  // padded keys stay out of the maximum
            }
        }
    };
#pragma unroll
    for (int sj = 0; sj < XT; ++sj) {
        if (sj < nt) {
            if (sj * 32 + 32 <= N)
                tile(sj, std::true_type{});
            else
                tile(sj, std::false_type{});
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    m = fmaxf(m, __shfl_xor(m, 32));
    float l = 0.f;
#pragma unroll
    for (int sj = 0; sj < XT; ++sj) {
        if (sj < nt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = sj * 32 + (r & 3) + 8 * (r >> 2) + h4;
                const float e = j < N ? __builtin_amdgcn_exp2f((st[sj][r] - m) * W_LOG2E) : 0.f;  // ... and get exactly 0
                st[sj][r] = e;
                l += e;
            }
        }
    }
    l += __shfl_xor(l, 32);
    const float inv = 1.f / l;
#pragma unroll
    for (int sj = 0; sj < XT; ++sj)
        if (sj < nt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) st[sj][r] *= inv;
        }
    m_out = m;
    inv_out = inv;
}

template <typename T, bool DENSE>
__global__ __launch_bounds__(XF_THREADS) void k_attn_xl_fwd(const AttnParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int N = p.N;
    const int IB = wide_img_bytes<T>(N);
    unsigned char* sQ = smem;
    unsigned char* sK = smem + IB;
    unsigned char* sV = smem + 2 * IB;
    WideTabs tb;
    tb.tokC = reinterpret_cast<int*>(smem + 3 * IB);
    tb.tokC3 = tb.tokC + XN;
    tb.srid = tb.tokC3 + XN;
    const int tid = threadIdx.x, lane0 = tid & 63, wv = tid >> 6;
    unsigned char* stg = reinterpret_cast<unsigned char*>(tb.srid + XN) + wv * STG<T>::BYTES;  // this wave's output staging image
    const int64_t L = xcd_remap(blockIdx.x, gridDim.x);
    const int head = (int)(L % p.nH);
    const int g = (int)(L / p.nH);
    const int nWimg = p.nWx * p.nWy;
    const int nt = (N + 31) >> 5;  // key / query tiles in use
    const T* qkv = reinterpret_cast<const T*>(p.qkv) + head * HD;
    T* out = reinterpret_cast<T*>(p.out) + head * HD;
    const float* bias_h = p.bias + (int64_t)head * N * N;
    const int C3 = 3 * p.C;
    const int my_tyx = pack_tyx(p, tid < N ? tid : 0);
    wide_zero_row(sQ, N, AC<T>::RS, tid);
    wide_zero_row(sK, N, AC<T>::RS, tid);
    wide_zero_row(sV, N, AC<T>::RS, tid);

    for (int64_t w = g; w < p.n_windows; w += p.G) {
        const int wm = (int)(w % nWimg);
        const WinPos wq = win_pos(p, w);
        __syncthreads();  // the previous window's LDS reads are done
        xl_tables(tb, p, wq, wm, my_tyx, tid);
        __syncthreads();
        const T* wb = qkv + wq.base * C3;
        xl_stage<T, XF_THREADS>(sQ, wb, tb.tokC3, N, tid);
        xl_stage<T, XF_THREADS>(sK, wb + p.C, tb.tokC3, N, tid);
        xl_stage<T, XF_THREADS>(sV, wb + 2 * p.C, tb.tokC3, N, tid);
        __syncthreads();
        const int qb = wv;
        if (qb < nt) {
            const int lane = wide_opaque(lane0);
            Frag<T> fq[AC<T>::KT_D];
            xl_lfrag<T>(fq, sQ, qb, lane, N);
            f32x16 st[XT];
            float m, inv;
            xl_probs_t<T, DENSE>(st, m, inv, sK, fq, qb, nt, p, bias_h, tb.srid, wm, lane);
            f32x16 o;
            zero(o);
#pragma unroll
            for (int sj = 0; sj < XT; ++sj)
                if (sj < nt) wide_mma_col<T>(o, sV, sj, st[sj], lane, N);
            store_dt_lds<T>(stg, out + wq.base * p.C, tb.tokC + qb * 32, N - qb * 32, o, 1.f, lane);
        }
    }
}

// backward, query-owner launch: dQ, dbias partials and the row statistics
template <typename T, bool DENSE>
__global__ __launch_bounds__(XB_THREADS) void k_attn_xl_bwd_q(const XlParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int N = p.N;
    const int IB = wide_img_bytes<T>(N);
    unsigned char* sK = smem;
    unsigned char* sV = smem + IB;
    WideTabs tb;
    tb.tokC = reinterpret_cast<int*>(smem + 2 * IB);
    tb.tokC3 = tb.tokC + XN;
    tb.srid = tb.tokC3 + XN;
    const int tid = threadIdx.x, lane0 = tid & 63, wv = tid >> 6;
    unsigned char* stg = reinterpret_cast<unsigned char*>(tb.srid + XN) + wv * STG<T>::BYTES;
    const int64_t L = xcd_remap(blockIdx.x, gridDim.x);
    const int half = (int)(L & 1);
    const int head = (int)((L >> 1) % p.nH);
    const int g = (int)((L >> 1) / p.nH);
    const int qb = 2 * wv + half;  // this wave's query block, the same for every window
    const int nWimg = p.nWx * p.nWy;
    const int nt = (N + 31) >> 5;
    const T* qkv = reinterpret_cast<const T*>(p.qkv) + head * HD;
    const T* dout = reinterpret_cast<const T*>(p.dout) + head * HD;
    T* dqkv = reinterpret_cast<T*>(p.dqkv) + head * HD;
    const float* bias_h = p.bias + (int64_t)head * N * N;
    const int C3 = 3 * p.C;
    const int my_tyx = pack_tyx(p, tid < N ? tid : 0);
    wide_zero_row(sK, N, AC<T>::RS, tid);
    wide_zero_row(sV, N, AC<T>::RS, tid);
    // dbias of this wave's query block: element (sj, r) of lane l is (key 32 sj + row(l, r), query 32 qb + l % 32) for every window
    f32x16 dbacc[XT];
#pragma unroll
    for (int sj = 0; sj < XT; ++sj) zero(dbacc[sj]);

    for (int64_t w = g; w < p.n_windows; w += p.G) {
        const int wm = (int)(w % nWimg);
        const WinPos wq = win_pos(p, w);
        __syncthreads();
        xl_tables(tb, p, wq, wm, my_tyx, tid);
        __syncthreads();
        const T* wb = qkv + wq.base * C3;
        xl_stage<T, XB_THREADS>(sK, wb + p.C, tb.tokC3, N, tid);
        xl_stage<T, XB_THREADS>(sV, wb + 2 * p.C, tb.tokC3, N, tid);
        __syncthreads();
        if (qb < nt) {
            const int lane = wide_opaque(lane0);
            const int il = lane & 31;
            f32x16 pt[XT];
            float m, inv;
            {
                Frag<T> fq[AC<T>::KT_D];
                xl_gfrag<T>(fq, wb, tb.tokC3, qb, lane, N);
                xl_probs_t<T, DENSE>(pt, m, inv, sK, fq, qb, nt, p, bias_h, tb.srid, wm, lane);
            }
            __builtin_amdgcn_sched_barrier(0);  // (dO's rows are loaded once the softmax's temporaries are gone)
            Frag<T> fo[AC<T>::KT_D];
            xl_gfrag<T>(fo, dout + wq.base * p.C, tb.tokC, qb, lane, N);
            float D = 0.f;
#pragma unroll
            for (int sj = 0; sj < XT; ++sj)
                if (sj < nt) {
                    __builtin_amdgcn_sched_barrier(0);  // one tile at a time
                    f32x16 dp;  // dP^T[j][i] = sum_d V[j][d] dO[i][d]
                    zero(dp);
                    xl_mma_rowf<T>(dp, sV, sj, fo, lane, N);
#pragma unroll
                    for (int r = 0; r < 16; ++r) D += pt[sj][r] * dp[r];
                }
            D += __shfl_xor(D, 32);
            const int i = qb * 32 + il;
            if (lane < 32 && i < N) {
                float* st = p.stats + ((int64_t)w * p.nH + head) * 3 * N;
                st[i] = m;
                st[N + i] = inv;
                st[2 * N + i] = D;
            }
            f32x16 dq;
            zero(dq);
#pragma unroll
            for (int sj = 0; sj < XT; ++sj)
                if (sj < nt) {
                    __builtin_amdgcn_sched_barrier(0);
                    f32x16 ds;
                    zero(ds);
                    xl_mma_rowf<T>(ds, sV, sj, fo, lane, N);
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float v = pt[sj][r] * (ds[r] - D);  // (padded keys: P = 0; padded queries: dO = 0, so D = 0 and v = 0)
                        ds[r] = v;
                        dbacc[sj][r] += v;
                    }
                    wide_mma_col<T>(dq, sK, sj, ds, lane, N);  // dQ^T[d][i] += sum_j K[j][d] dS^T[j][i]
                }
            store_dt_lds<T>(stg, dqkv + wq.base * C3, tb.tokC3 + qb * 32, N - qb * 32, dq, p.scale, lane);
        }
    }
    float* dst = p.dbias_part + ((int64_t)g * p.nH + head) * N * N;  // [j][i]
    const int i = qb * 32 + (lane0 & 31), h4 = 4 * (lane0 >> 5);
#pragma unroll
    for (int sj = 0; sj < XT; ++sj)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = sj * 32 + (r & 3) + 8 * (r >> 2) + h4;
            if (i < N && j < N) dst[j * N + i] = dbacc[sj][r];
        }
}

// backward, key-owner launch (after the query-owner launch on the same stream): dK and dV
template <typename T, bool DENSE>
__global__ __launch_bounds__(XB_THREADS) void k_attn_xl_bwd_k(const XlParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int N = p.N;
    const int IB = wide_img_bytes<T>(N);
    unsigned char* sQ = smem;
    unsigned char* sO = smem + IB;
    WideTabs tb;
    tb.tokC = reinterpret_cast<int*>(smem + 2 * IB);
    tb.tokC3 = tb.tokC + XN;
    tb.srid = tb.tokC3 + XN;
    float* sM = reinterpret_cast<float*>(tb.srid + XN);  // row statistics of the query-owner launch: maximum, 1 / sum, D
    float* sL = sM + XN;
    float* sD = sL + XN;
    const int tid = threadIdx.x, lane0 = tid & 63, wv = tid >> 6;
    unsigned char* stg = reinterpret_cast<unsigned char*>(sD + XN) + wv * STG<T>::BYTES;
    const int64_t L = xcd_remap(blockIdx.x, gridDim.x);
    const int half = (int)(L & 1);
    const int head = (int)((L >> 1) % p.nH);
    const int g = (int)((L >> 1) / p.nH);
    const int kb = 2 * wv + half;  // this wave's key block
    const int nWimg = p.nWx * p.nWy;
    const int nt = (N + 31) >> 5;
    const T* qkv = reinterpret_cast<const T*>(p.qkv) + head * HD;
    const T* dout = reinterpret_cast<const T*>(p.dout) + head * HD;
    T* dqkv = reinterpret_cast<T*>(p.dqkv) + head * HD;
    const float* bias_h = p.bias + (int64_t)head * N * N;
    const int C3 = 3 * p.C;
    const int my_tyx = pack_tyx(p, tid < N ? tid : 0);
    wide_zero_row(sQ, N, AC<T>::RS, tid);
    wide_zero_row(sO, N, AC<T>::RS, tid);

    for (int64_t w = g; w < p.n_windows; w += p.G) {
        const int wm = (int)(w % nWimg);
        const WinPos wq = win_pos(p, w);
        __syncthreads();
        xl_tables(tb, p, wq, wm, my_tyx, tid);
        if (tid < XN) {
            const float* st = p.stats + ((int64_t)w * p.nH + head) * 3 * N;
            const bool v = tid < N;
            sM[tid] = v ? st[tid] : 0.f;
            sL[tid] = v ? st[N + tid] : 0.f;
            sD[tid] = v ? st[2 * N + tid] : 0.f;
        }
        __syncthreads();
        const T* wb = qkv + wq.base * C3;
        T* gb = dqkv + wq.base * C3;
        xl_stage<T, XB_THREADS>(sQ, wb, tb.tokC3, N, tid);
        xl_stage<T, XB_THREADS>(sO, dout + wq.base * p.C, tb.tokC, N, tid);
        __syncthreads();
        if (kb < nt) {
            const int lane = wide_opaque(lane0);
            const int il = lane & 31, h4 = 4 * (lane >> 5);
            const int j = kb * 32 + il;
            const bool jv = j < N;
            const int jc = jv ? j : N - 1;
            const int rid_j = tb.srid[jc];
            const bool ids = !DENSE && p.mask_ids != nullptr;
            Frag<T> fk[AC<T>::KT_D], fv[AC<T>::KT_D];
            xl_gfrag<T>(fk, wb + p.C, tb.tokC3, kb, lane, N);
            xl_gfrag<T>(fv, wb + 2 * p.C, tb.tokC3, kb, lane, N);
            f32x16 dk, dv;
            zero(dk);
            zero(dv);
#pragma unroll 1
            for (int si = 0; si < nt; ++si) {
                f32x16 s, dp;  // [query i][key j]: lane owns the key
                zero(s);
                zero(dp);
                xl_mma_rowf<T>(s, sQ, si, fk, lane, N);
                xl_mma_rowf<T>(dp, sO, si, fv, lane, N);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = si * 32 + (r & 3) + 8 * (r >> 2) + h4;
                    const bool iv = i < N;
                    const int ic = iv ? i : N - 1;
                    float add = bias_h[(uint32_t)(ic * N + jc)];
                    if constexpr (DENSE) add += p.mask[(uint32_t)((wm * N + ic) * N + jc)];
                    if (ids) add += tb.srid[ic] != rid_j ? p.mask_value : 0.f;
                    const float v = s[r] * p.scale + add;
                    const float pr = (iv && jv) ? __builtin_amdgcn_exp2f((v - sM[ic]) * W_LOG2E) * sL[ic] : 0.f;
                    s[r] = pr;
                    dp[r] = pr * (dp[r] - sD[ic]);
                }
                wide_mma_col<T>(dk, sQ, si, dp, lane, N);  // dK^T[d][j] += sum_i Q[i][d] dS[i][j]
                wide_mma_col<T>(dv, sO, si, s, lane, N);   // dV^T[d][j] += sum_i dO[i][d] P[i][j]
            }
            store_dt_lds<T>(stg, gb + p.C, tb.tokC3 + kb * 32, N - kb * 32, dk, p.scale, lane);
            store_dt_lds<T>(stg, gb + 2 * p.C, tb.tokC3 + kb * 32, N - kb * 32, dv, 1.f, lane);
        }
    }
}

// ---- relative-position bias of these windows: bias[h][i][j] = table[index[i][j]][h] without the (2 ws - 1)^2 x N^2 one-hot matrix ----
__global__ __launch_bounds__(256) void k_rel_bias_gather(const float* table, const int* index, float* bias, int E, int nH, int NN) {
    const int pos = blockIdx.x * 256 + threadIdx.x;
    if (pos >= NN) return;
    const int e = index[pos];
    const bool ok = (unsigned)e < (unsigned)E;  // (an index outside the table contributes 0; the host rejects it when it builds the lists)
    for (int h = 0; h < nH; ++h) bias[(int64_t)h * NN + pos] = ok ? table[(int64_t)e * nH + h] : 0.f;
}
// d table[e][h] = sum of dbias[h][pos] over the positions of entry e (CSR lists in ascending position order): one wave per entry, lane l
// adds positions l, l + 64, ... of the list in that order, then one fixed butterfly across the lanes -- the same sums in the same order
// on every run, every element written (an entry no position uses gets 0)
__global__ __launch_bounds__(64) void k_rel_bias_scatter(const float* dbias, const int* off, const int* pos, float* dtable, int nH,
                                                         int NN) {
    const int e = blockIdx.x, lane = threadIdx.x;
    const int b = off[e], n = off[e + 1] - b;
    for (int h = 0; h < nH; ++h) {
        float a = 0.f;
        for (int k = lane; k < n; k += 64) {
            const int q = pos[b + k];
            a += (unsigned)q < (unsigned)NN ? dbias[(int64_t)h * NN + q] : 0.f;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
        if (lane == 0) dtable[(int64_t)e * nH + h] = a;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
enum { XL_FWD = 0, XL_BWD_Q = 1, XL_BWD_K = 2 };
static size_t xl_lds_bytes(int dtype, int N, int kind) {
    const AttnSizes z = attn_sizes(dtype);
    const size_t ib = (((size_t)(N + 1) * z.rs + 15) / 16) * 16;
    if (kind == XL_FWD) return 3 * ib + 3 * XN * 4 + XT * z.stg;
    return 2 * ib + (kind == XL_BWD_K ? 6 : 3) * XN * 4 + XB_WAVES * z.stg;
}
// persistent grids: one resident workgroup per CU; the backward's workgroups come in pairs (the two halves of a window's blocks)
static int xl_groups(const mtlora_attn_desc* d, bool bwd) {
    const int64_t nwin = d->B * (d->H / d->window_size) * (d->W / d->window_size);
    int64_t G = (bwd ? 128 : 256) / d->num_heads;
    if (G > nwin) G = nwin;
    if (G < 1) G = 1;
    return (int)G;
}
static int64_t xl_part_bytes(const mtlora_attn_desc* d) {
    const int64_t N = d->window_size * d->window_size;
    return (int64_t)xl_groups(d, true) * d->num_heads * N * N * 4;
}
static int64_t xl_stats_bytes(const mtlora_attn_desc* d) {
    const int64_t N = d->window_size * d->window_size;
    const int64_t nwin = d->B * (d->H / d->window_size) * (d->W / d->window_size);
    return nwin * d->num_heads * 3 * N * 4;
}
template <auto KERNEL, typename P>
static int xl_launch(const P& p, unsigned grid, unsigned threads, size_t lds, hipStream_t s) {
    static std::atomic<unsigned long long> done{0};  // (one per kernel instantiation)
    const void* kernel = reinterpret_cast<const void*>(KERNEL);
    if (lds > (size_t)WIDE_LDS_MAX || !wide_allow_lds(done, kernel, lds)) return MTLORA_ERR_HIP;
    void* args[] = {const_cast<P*>(&p)};
    if (hipLaunchKernel(kernel, dim3(grid), dim3(threads), args, lds, s) != hipSuccess) return MTLORA_ERR_HIP;
    return MTLORA_OK;
}
static int xl_fwd(const mtlora_attn_desc* d, AttnParams& p, hipStream_t s) {
    const bool dense = p.mask && !p.mask_ids;
    p.G = xl_groups(d, false);
    const unsigned grid = (unsigned)(p.G * p.nH);
    const size_t lds = xl_lds_bytes(d->dtype, p.N, XL_FWD);
    return mtl_dispatch_dtype(d->dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        return dense ? xl_launch<k_attn_xl_fwd<T, true>>(p, grid, XF_THREADS, lds, s) : xl_launch<k_attn_xl_fwd<T, false>>(p, grid, XF_THREADS, lds, s);
    });
}
static int xl_bwd(const mtlora_attn_desc* d, XlParams& p, hipStream_t s) {
    const bool dense = p.mask && !p.mask_ids;
    p.G = xl_groups(d, true);
    const unsigned grid = (unsigned)(p.G * p.nH * 2);
    const size_t lq = xl_lds_bytes(d->dtype, p.N, XL_BWD_Q), lk = xl_lds_bytes(d->dtype, p.N, XL_BWD_K);
    return mtl_dispatch_dtype(d->dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        const int st = dense ? xl_launch<k_attn_xl_bwd_q<T, true>>(p, grid, XB_THREADS, lq, s) : xl_launch<k_attn_xl_bwd_q<T, false>>(p, grid, XB_THREADS, lq, s);
        if (st != MTLORA_OK) return st;
        return dense ? xl_launch<k_attn_xl_bwd_k<T, true>>(p, grid, XB_THREADS, lk, s) : xl_launch<k_attn_xl_bwd_k<T, false>>(p, grid, XB_THREADS, lk, s);
    });
}
