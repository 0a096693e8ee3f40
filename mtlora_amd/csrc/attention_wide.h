// attention_wide.h -- window attention core for 64 < N = ws*ws <= 144 (ws 9..12), forward and backward.
// Included by attention.hip inside its anonymous namespace: the token addressing (win_pos / token_at), the LDS image geometry
// (AC<T>: N token rows + one shared zero row that every padded row reads), the fragment readers (rowfrag / colfrag) and the
// coalescing output path (store_dt_lds) are the narrow kernels' own.
//
// One wave cannot hold a 160 x 160 score block (400 accumulator registers), so ONE WORKGROUP serves a (window, head) pair with one
// wave per 32-query block (5 waves; blocks past N idle through the barriers).  The window's Q / K / V (/ dO) rows are staged in LDS
// once and shared by the waves.
//   forward:   wave qb:  S^T = K Q_qb^T as up to five 32 x 32 tiles (lane owns a query, registers span keys), + bias + mask,
//              softmax over keys inside the wave, O^T = V^T P^T.  No cross-wave traffic beyond the shared images.
//   backward:  phase 1 (wave = query block):  P^T as in the forward, D_i = sum_j P dP (one sweep of dP^T = V dO^T tiles), a second
//              sweep forms dS^T tile by tile -> dbias (REGISTER accumulate over the wave's windows, as in the narrow kernel) and
//              dQ^T = K^T dS^T; the row statistics (max, 1 / sum, D) go to LDS.
//              phase 2 (wave = key block):    S, P, dP recomputed in the other orientation (lane owns a key) from those statistics
//              -> dK^T = Q^T dS, dV^T = dO^T P.
//              No float is ever accumulated across waves: every output element has exactly one owner, so there is nothing whose
//              order could depend on timing, and no global scratch beyond the dbias partials of k_dbias_reduce.
// Padded keys (j >= N) are excluded from the row maximum and get probability exactly 0 (a select, not a large negative bias);
// padded queries are never stored and enter dK / dV / dbias as exact zeros.
// The bias (and the dense mask) are added in fp32 straight from memory for every dtype.

constexpr int WT = 5;               // 32-token tiles: keys / queries padded to 160
constexpr int WN = 32 * WT;
constexpr int W_THREADS = 64 * WT;  // one wave per query block
// backward: the dbias accumulator (80 registers per query block) lives across the persistent loop next to the 80 of P^T, which does not
// fit the 256 registers a wave has at two waves on a SIMD -- so 4 waves, one per SIMD with the whole 512-entry file, wave 0 taking the
// fifth block of a 12 x 12 window as well
constexpr int WB_WAVES = 4;
constexpr int WB_QPW = (WT + WB_WAVES - 1) / WB_WAVES;
constexpr int WB_THREADS = 64 * WB_WAVES;
constexpr float W_LOG2E = 1.4426950408889634f;

template <typename T>
__device__ __forceinline__ int wide_img_bytes(int N) {
    return (((N + 1) * AC<T>::RS + 15) / 16) * 16;
}

// accumulator tile as the B operand of the next product (k = the tile's rows); fp32 needs two 16-row k-tiles per tile
__device__ __forceinline__ Frag<bf16> accfrag(const f32x16& a, int, bf16*) {
    Frag<bf16> f;
    f.v[0] = u32x4{mtl_pk2<bf16>(a[0], a[1]), mtl_pk2<bf16>(a[2], a[3]), mtl_pk2<bf16>(a[4], a[5]), mtl_pk2<bf16>(a[6], a[7])};
    f.v[1] = u32x4{mtl_pk2<bf16>(a[8], a[9]), mtl_pk2<bf16>(a[10], a[11]), mtl_pk2<bf16>(a[12], a[13]), mtl_pk2<bf16>(a[14], a[15])};
    return f;
}
__device__ __forceinline__ Frag<f16> accfrag(const f32x16& a, int, f16*) {
    Frag<f16> f;
    f.v[0] = u32x4{mtl_pk2<f16>(a[0], a[1]), mtl_pk2<f16>(a[2], a[3]), mtl_pk2<f16>(a[4], a[5]), mtl_pk2<f16>(a[6], a[7])};
    f.v[1] = u32x4{mtl_pk2<f16>(a[8], a[9]), mtl_pk2<f16>(a[10], a[11]), mtl_pk2<f16>(a[12], a[13]), mtl_pk2<f16>(a[14], a[15])};
    return f;
}
__device__ __forceinline__ Frag<float> accfrag(const f32x16& a, int kk, float*) {
    Frag<float> f;
    const int o = kk * 8;
    f.v[0] = __builtin_bit_cast(u32x4, f32x4{a[o + 0], a[o + 1], a[o + 2], a[o + 3]});
    f.v[1] = __builtin_bit_cast(u32x4, f32x4{a[o + 4], a[o + 5], a[o + 6], a[o + 7]});
    return f;
}
// out[d][lane] += sum over the 32 rows of image tile `tile` of  img[row][d] * acc[row][lane]
template <typename T>
__device__ __forceinline__ void wide_mma_col(f32x16& out, const unsigned char* img, int tile, const f32x16& acc, int lane, int N) {
    constexpr int KK = sizeof(T) == 4 ? 2 : 1;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
        Frag<T> fa = colfrag(img, tile * KK + kk, lane, N, (T*)nullptr);
        Frag<T> fb = accfrag(acc, kk, (T*)nullptr);
        mtl_mma(fa, fb, out);
    }
}
// out[row of a][row of b (lane)] = sum_d imgA[tile ta][d] * imgB[tile tb][d]
template <typename T>
__device__ __forceinline__ void wide_mma_row(f32x16& out, const unsigned char* imgA, int ta, const unsigned char* imgB, int tb, int lane,
                                             int N) {
#pragma unroll
    for (int kt = 0; kt < AC<T>::KT_D; ++kt) {
        Frag<T> fa = rowfrag<T>(imgA, ta, kt, lane, N);
        Frag<T> fb = rowfrag<T>(imgB, tb, kt, lane, N);
        mtl_mma(fa, fb, out);
    }
}

// Everything a lane derives from its id alone (fragment addresses, clamped rows, validity masks) is the same for every window; left
// visible, the optimiser hoists all of it out of the persistent loop and keeps it live there (hundreds of registers, i.e. scratch).
// Laundering the lane id once per window and block keeps those values short-lived; recomputing them is a few VALU per fragment.
__device__ __forceinline__ int wide_opaque(int v) {
    asm volatile("" : "+v"(v));
    return v;
}

// per-window tables: element offsets of the tokens' rows in a C-wide and a 3C-wide tensor, and their region ids
struct WideTabs {
    int* tokC;
    int* tokC3;
    int* srid;
};
__device__ __forceinline__ void wide_tables(const WideTabs& tb, const AttnParams& p, const WinPos& wq, int wm, int my_tyx, int tid) {
    if (tid < WN) {
        const bool v = tid < p.N;
        const int idx = v ? token_at(p, wq, tid, my_tyx) : 0;
        tb.tokC[tid] = idx * p.C;
        tb.tokC3[tid] = idx * 3 * p.C;
        tb.srid[tid] = (p.mask_ids && v) ? p.mask_ids[wm * p.N + tid] : 0;
    }
}
// rows of one (window, head) operand: global -> LDS image, 16 bytes per thread and step.  base: workgroup-uniform pointer
template <typename T, int NT>
__device__ __forceinline__ void wide_stage(unsigned char* img, const T* base, const int* tokoff, int N, int tid) {
    constexpr int VPR = AC<T>::VPR, RS = AC<T>::RS;
    constexpr int IT = (144 * VPR + NT - 1) / NT;
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
__device__ __forceinline__ void wide_zero_row(unsigned char* img, int N, int rs, int tid) {
    if (tid * 16 < rs) *reinterpret_cast<u32x4*>(img + N * rs + tid * 16) = u32x4{0u, 0u, 0u, 0u};
}

// P^T of query block qb: st[sj][r] = P[query qb*32 + (lane & 31)][key sj*32 + row(r, lane)], normalised; returns the row's
// maximum (m) and 1 / sum (inv) of the logits  q.k * scale + bias (+ mask)
template <typename T, bool DENSE>
__device__ __forceinline__ void wide_probs_t(f32x16 (&st)[WT], float& m_out, float& inv_out, const unsigned char* sK,
                                             const unsigned char* sQ, int qb, int nt, const AttnParams& p, const float* bias_h,
                                             const int* srid, int wm, int lane) {
    const int N = p.N;
#pragma unroll
    for (int sj = 0; sj < WT; ++sj) {
        zero(st[sj]);
        if (sj < nt) wide_mma_row<T>(st[sj], sK, sj, sQ, qb, lane, N);
    }
    const int i = qb * 32 + (lane & 31);
    const int ic = i < N ? i : N - 1;
    int h4 = 4 * (lane >> 5);
    // bias / mask: workgroup-uniform base + 32-bit per-lane offset
    uint32_t boff = (uint32_t)(ic * N);
    // (the 80 element addresses and key-validity masks below are the same for every window: left visible, they are all hoisted out of
    // the persistent loop and live across it -- 160 registers and 80 lane masks, i.e. scratch.  Recomputing them is ~4 VALU an element)
    asm volatile("" : "+v"(h4), "+v"(boff));
    const uint32_t moff = DENSE ? (uint32_t)((wm * N + ic) * N) : 0u;
    const bool ids = !DENSE && p.mask_ids != nullptr;
    const int rid_i = srid[ic];
    float m = -3.0e38f;
#pragma unroll
    for (int sj = 0; sj < WT; ++sj) {
        __builtin_amdgcn_sched_barrier(0);  // one tile's 16 loads in flight at a time (register pressure)
        if (sj < nt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = sj * 32 + (r & 3) + 8 * (r >> 2) + h4;
                const bool jv = j < N;
                const uint32_t jc = (uint32_t)(jv ? j : N - 1);
                float add = bias_h[boff + jc];
                if constexpr (DENSE) add += p.mask[moff + jc];
                if (ids) add += srid[jc] != rid_i ? p.mask_value : 0.f;
                const float v = st[sj][r] * p.scale + add;
                st[sj][r] = v;
                m = jv ? fmaxf(m, v) : m;  // padded keys stay out of the maximum
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    m = fmaxf(m, __shfl_xor(m, 32));
    float l = 0.f;
#pragma unroll
    for (int sj = 0; sj < WT; ++sj) {
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
    for (int sj = 0; sj < WT; ++sj)
        if (sj < nt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) st[sj][r] *= inv;
        }
    m_out = m;
    inv_out = inv;
}

template <typename T, bool DENSE, bool DROP, typename P>
__device__ __forceinline__ void attn_wide_fwd_body(const P p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int N = p.N;
    const int IB = wide_img_bytes<T>(N);
    unsigned char* sQ = smem;
    unsigned char* sK = smem + IB;
    unsigned char* sV = smem + 2 * IB;
    WideTabs tb;
    tb.tokC = reinterpret_cast<int*>(smem + 3 * IB);
    tb.tokC3 = tb.tokC + WN;
    tb.srid = tb.tokC3 + WN;
    const int tid = threadIdx.x, lane0 = tid & 63, wv = tid >> 6;
    unsigned char* stg = reinterpret_cast<unsigned char*>(tb.srid + WN) + wv * STG<T>::BYTES;  // this wave's output staging image
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
    [[maybe_unused]] DropoutCfg dc;
    if constexpr (DROP) dc = attn_drop_cfg(p);

    for (int64_t w = g; w < p.n_windows; w += p.G) {
        const int wm = (int)(w % nWimg);
        const WinPos wq = win_pos(p, w);
        __syncthreads();  // the previous window's LDS reads are done
        wide_tables(tb, p, wq, wm, my_tyx, tid);
        __syncthreads();
        const T* wb = qkv + wq.base * C3;
        wide_stage<T, W_THREADS>(sQ, wb, tb.tokC3, N, tid);
        wide_stage<T, W_THREADS>(sK, wb + p.C, tb.tokC3, N, tid);
        wide_stage<T, W_THREADS>(sV, wb + 2 * p.C, tb.tokC3, N, tid);
        __syncthreads();
        const int qb = wv;
        if (qb < nt) {
            const int lane = wide_opaque(lane0);
            f32x16 st[WT];
            float m, inv;
            wide_probs_t<T, DENSE>(st, m, inv, sK, sQ, qb, nt, p, bias_h, tb.srid, wm, lane);
            float mul = 1.f;
            [[maybe_unused]] uint32_t rh = 0u;
            if constexpr (DROP) {  // P' = keep . P / (1 - p): the factor joins the output scale
                rh = attn_drop_rowhash(dc, p, w, head, qb * 32 + (lane & 31));
                mul = p.keep_scale;
            }
            f32x16 o;
            zero(o);
#pragma unroll
            for (int sj = 0; sj < WT; ++sj)
                if (sj < nt) {
                    if constexpr (DROP)  // the tile's bits, right where the tile is consumed
                        attn_keep_tile(dc, rh, sj * 32 + 4 * (lane >> 5), [&](int r, bool keep) __attribute__((always_inline)) {
                            st[sj][r] = keep ? st[sj][r] : 0.f;
                        });
                    wide_mma_col<T>(o, sV, sj, st[sj], lane, N);
                }
            store_dt_lds<T>(stg, out + wq.base * p.C, tb.tokC + qb * 32, N - qb * 32, o, mul, lane);
        }
    }
}
template <typename T, bool DENSE>
__global__ __launch_bounds__(W_THREADS) void k_attn_wide_fwd(const AttnParams p) {
    attn_wide_fwd_body<T, DENSE, false>(p);
}
template <typename T, bool DENSE>
__global__ __launch_bounds__(W_THREADS) void k_attn_drop_wide_fwd(const AttnDropParams p) {
    attn_wide_fwd_body<T, DENSE, true>(p);
}

template <typename T, bool DENSE, bool DROP, typename P>
__device__ __forceinline__ void attn_wide_bwd_body(const P p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int N = p.N;
    const int IB = wide_img_bytes<T>(N);
    unsigned char* sQ = smem;
    unsigned char* sK = smem + IB;
    unsigned char* sV = smem + 2 * IB;
    unsigned char* sO = smem + 3 * IB;
    WideTabs tb;
    tb.tokC = reinterpret_cast<int*>(smem + 4 * IB);
    tb.tokC3 = tb.tokC + WN;
    tb.srid = tb.tokC3 + WN;
    float* sM = reinterpret_cast<float*>(tb.srid + WN);  // row statistics of phase 1: maximum, 1 / sum, D
    float* sL = sM + WN;
    float* sD = sL + WN;
    const int tid = threadIdx.x, lane0 = tid & 63, wv = tid >> 6;
    unsigned char* stg = reinterpret_cast<unsigned char*>(sD + WN) + wv * STG<T>::BYTES;
    // DROP: row hashes of the window's queries for phase 2, where a lane's registers span the queries (behind the staging images)
    [[maybe_unused]] uint32_t* sRH = reinterpret_cast<uint32_t*>(reinterpret_cast<unsigned char*>(sD + WN) + WB_WAVES * STG<T>::BYTES);
    [[maybe_unused]] DropoutCfg dc;
    if constexpr (DROP) dc = attn_drop_cfg(p);
    const int64_t L = xcd_remap(blockIdx.x, gridDim.x);
    const int head = (int)(L % p.nH);
    const int g = (int)(L / p.nH);
    const int nWimg = p.nWx * p.nWy;
    const int nt = (N + 31) >> 5;
    const T* qkv = reinterpret_cast<const T*>(p.qkv) + head * HD;
    const T* dout = reinterpret_cast<const T*>(p.dout) + head * HD;
    T* dqkv = reinterpret_cast<T*>(p.dqkv) + head * HD;
    const float* bias_h = p.bias + (int64_t)head * N * N;
    const int C3 = 3 * p.C;
    const int my_tyx = pack_tyx(p, tid < N ? tid : 0);
    wide_zero_row(sQ, N, AC<T>::RS, tid);
    wide_zero_row(sK, N, AC<T>::RS, tid);
    wide_zero_row(sV, N, AC<T>::RS, tid);
    wide_zero_row(sO, N, AC<T>::RS, tid);
    // dbias of this wave's query blocks: element (qi, sj, r) of lane l is (key 32 sj + row(l, r), query 32 (wv + WB_WAVES qi) + l % 32)
    // for every window
    f32x16 dbacc[WB_QPW][WT];
#pragma unroll
    for (int qi = 0; qi < WB_QPW; ++qi)
#pragma unroll
        for (int sj = 0; sj < WT; ++sj) zero(dbacc[qi][sj]);

    for (int64_t w = g; w < p.n_windows; w += p.G) {
        const int wm = (int)(w % nWimg);
        const WinPos wq = win_pos(p, w);
        __syncthreads();
        wide_tables(tb, p, wq, wm, my_tyx, tid);
        if constexpr (DROP) {
            if (tid < WN) sRH[tid] = attn_drop_rowhash(dc, p, w, head, tid);
        }
        __syncthreads();
        const T* wb = qkv + wq.base * C3;
        T* gb = dqkv + wq.base * C3;
        wide_stage<T, WB_THREADS>(sQ, wb, tb.tokC3, N, tid);
        wide_stage<T, WB_THREADS>(sK, wb + p.C, tb.tokC3, N, tid);
        wide_stage<T, WB_THREADS>(sV, wb + 2 * p.C, tb.tokC3, N, tid);
        wide_stage<T, WB_THREADS>(sO, dout + wq.base * p.C, tb.tokC, N, tid);
        __syncthreads();
        // ---- phase 1: this wave's query blocks
#pragma unroll
        for (int qi = 0; qi < WB_QPW; ++qi) {
            const int qb = wv + WB_WAVES * qi;
            if (qb >= nt) continue;
            const int lane = wide_opaque(lane0);
            const int il = lane & 31;
            f32x16 pt[WT];
            float m, inv;
            wide_probs_t<T, DENSE>(pt, m, inv, sK, sQ, qb, nt, p, bias_h, tb.srid, wm, lane);
            float D = 0.f;
            // DROP: dP = keep . (dO V^T) / (1 - p).  The bits of a tile are drawn once, in the first sweep, and carried to the second as 16
            // bits per tile (three registers for the five tiles)
            [[maybe_unused]] uint32_t kept[(WT + 1) / 2] = {};
            [[maybe_unused]] uint32_t rh = 0u;
            if constexpr (DROP) rh = attn_drop_rowhash(dc, p, w, head, qb * 32 + il);
#pragma unroll
            for (int sj = 0; sj < WT; ++sj)
                if (sj < nt) {
                    f32x16 dp;  // dP^T[j][i] = sum_d V[j][d] dO[i][d]
                    zero(dp);
                    wide_mma_row<T>(dp, sV, sj, sO, qb, lane, N);
                    if constexpr (DROP) {
                        uint32_t kb = 0u;
                        attn_keep_tile(dc, rh, sj * 32 + 4 * (lane >> 5), [&](int r, bool keep) __attribute__((always_inline)) {
                            dp[r] = keep ? dp[r] : 0.f;
                            kb |= keep ? 1u << r : 0u;
                        });
                        kept[sj >> 1] |= kb << (16 * (sj & 1));
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) D += pt[sj][r] * dp[r];
                }
            if constexpr (DROP) D *= p.keep_scale;
            D += __shfl_xor(D, 32);
            if (lane < 32) {
                sM[qb * 32 + il] = m;
                sL[qb * 32 + il] = inv;
                sD[qb * 32 + il] = D;
            }
            f32x16 dq;
            zero(dq);
#pragma unroll
            for (int sj = 0; sj < WT; ++sj)
                if (sj < nt) {
                    f32x16 ds;
                    zero(ds);
                    wide_mma_row<T>(ds, sV, sj, sO, qb, lane, N);
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float dpr = ds[r];
                        if constexpr (DROP) dpr = ((kept[sj >> 1] >> (16 * (sj & 1) + r)) & 1u) ? dpr * p.keep_scale : 0.f;
                        const float v = pt[sj][r] * (dpr - D);  // (padded keys: P = 0)
                        ds[r] = v;
                        dbacc[qi][sj][r] += v;
                    }
                    wide_mma_col<T>(dq, sK, sj, ds, lane, N);  // dQ^T[d][i] += sum_j K[j][d] dS^T[j][i]
                }
            store_dt_lds<T>(stg, gb, tb.tokC3 + qb * 32, N - qb * 32, dq, p.scale, lane);
        }
        __syncthreads();  // the statistics of every query block are in LDS
        // ---- phase 2: this wave's key blocks
#pragma unroll 1
        for (int kb = wv; kb < nt; kb += WB_WAVES) {
            const int lane = wide_opaque(lane0);
            const int il = lane & 31, h4 = 4 * (lane >> 5);
            const int j = kb * 32 + il;
            const bool jv = j < N;
            const int jc = jv ? j : N - 1;
            const int rid_j = tb.srid[jc];
            const bool ids = !DENSE && p.mask_ids != nullptr;
            f32x16 dk, dv;
            zero(dk);
            zero(dv);
#pragma unroll 1
            for (int si = 0; si < nt; ++si) {
                f32x16 s, dp;  // [query i][key j]: lane owns the key
                zero(s);
                zero(dp);
                wide_mma_row<T>(s, sQ, si, sK, kb, lane, N);
                wide_mma_row<T>(dp, sO, si, sV, kb, lane, N);
                [[maybe_unused]] uint32_t kept = 0u;  // DROP: keep bit of query row r of this tile for the lane's key
                if constexpr (DROP) {
#pragma unroll
                    for (int t = 0; t < 8; ++t) {  // rows 2t, 2t + 1 are adjacent queries
                        const int i0 = si * 32 + ((2 * t) & 3) + 8 * (t >> 1) + h4;
                        bool k0, k1;
                        attn_keep_keypair(dc, sRH[i0], sRH[i0 + 1], j, k0, k1);  // (i0 + 1 < WN: the table spans the padded rows)
                        kept |= (k0 ? 1u : 0u) << (2 * t) | (k1 ? 2u : 0u) << (2 * t);
                    }
                }
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
                    if constexpr (DROP) {  // dS from dP = keep . dP / (1 - p); dV takes P'
                        const bool keep = (kept >> r) & 1u;
                        s[r] = keep ? pr * p.keep_scale : 0.f;
                        dp[r] = pr * ((keep ? dp[r] * p.keep_scale : 0.f) - sD[ic]);
                    } else {
                        s[r] = pr;
                        dp[r] = pr * (dp[r] - sD[ic]);
                    }
                }
                wide_mma_col<T>(dk, sQ, si, dp, lane, N);  // dK^T[d][j] += sum_i Q[i][d] dS[i][j]
                wide_mma_col<T>(dv, sO, si, s, lane, N);   // dV^T[d][j] += sum_i dO[i][d] P[i][j]
            }
            store_dt_lds<T>(stg, gb + p.C, tb.tokC3 + kb * 32, N - kb * 32, dk, p.scale, lane);
            store_dt_lds<T>(stg, gb + 2 * p.C, tb.tokC3 + kb * 32, N - kb * 32, dv, 1.f, lane);
        }
    }
    float* dst = p.dbias_part + ((int64_t)g * p.nH + head) * N * N;  // [j][i]
#pragma unroll
    for (int qi = 0; qi < WB_QPW; ++qi) {
        const int il = lane0 & 31, h4 = 4 * (lane0 >> 5);
        const int i = (wv + WB_WAVES * qi) * 32 + il;
#pragma unroll
        for (int sj = 0; sj < WT; ++sj)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = sj * 32 + (r & 3) + 8 * (r >> 2) + h4;
                if (i < N && j < N) dst[j * N + i] = dbacc[qi][sj][r];
            }
    }
}
template <typename T, bool DENSE>
__global__ __launch_bounds__(WB_THREADS) void k_attn_wide_bwd(const AttnParams p) {
    attn_wide_bwd_body<T, DENSE, false>(p);
}
template <typename T, bool DENSE>
__global__ __launch_bounds__(WB_THREADS) void k_attn_drop_wide_bwd(const AttnDropParams p) {
    attn_wide_bwd_body<T, DENSE, true>(p);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static size_t wide_lds_bytes(int dtype, int N, bool bwd, bool drop = false) {
    const AttnSizes z = attn_sizes(dtype);
    const size_t ib = (((size_t)(N + 1) * z.rs + 15) / 16) * 16;
    return (bwd ? 4 : 3) * ib + (bwd ? 6 : 3) * WN * 4 + (bwd ? WB_WAVES : WT) * z.stg + (bwd && drop ? WN * 4 : 0);  // (row hashes)
}
// persistent grid of `per_cu` resident workgroups per CU.  Backward: one (4 waves on the whole register file).  Forward: two where
// both the registers (151: three waves on a SIMD, i.e. two 5-wave workgroups) and the LDS (48 KB each) admit them -- the 16-bit
// kernels without a dense mask -- else one
static int wide_groups(const mtlora_attn_desc* d, int per_cu = 1) {
    const int64_t nwin = d->B * (d->H / d->window_size) * (d->W / d->window_size);
    int64_t G = (256 * per_cu) / d->num_heads;
    if (G > nwin) G = nwin;
    if (G < 1) G = 1;
    return (int)G;
}
constexpr size_t WIDE_LDS_DEFAULT = 64 * 1024;  // dynamic LDS a kernel may use without asking
constexpr int WIDE_LDS_MAX = 160 * 1024;        // what one gfx950 workgroup may use
// dynamic LDS above the default has to be allowed per kernel and device; false when the runtime refuses
static bool wide_allow_lds(std::atomic<unsigned long long>& done, const void* kernel, size_t bytes) {
    if (bytes <= WIDE_LDS_DEFAULT) return true;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    const bool cached = dev >= 0 && dev < 64;  // (devices past the bit mask ask every time)
    if (cached && ((done.load(std::memory_order_relaxed) >> dev) & 1ull)) return true;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, WIDE_LDS_MAX) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    if (cached) done.fetch_or(1ull << dev, std::memory_order_relaxed);
    return true;
}
// the kernel of a parameter block: plain (AttnParams) or attention dropout (AttnDropParams)
template <typename T, bool DENSE>
static const void* wide_kernel(const AttnParams&, bool bwd) {
    return bwd ? reinterpret_cast<const void*>(k_attn_wide_bwd<T, DENSE>) : reinterpret_cast<const void*>(k_attn_wide_fwd<T, DENSE>);
}
template <typename T, bool DENSE>
static const void* wide_kernel(const AttnDropParams&, bool bwd) {
    return bwd ? reinterpret_cast<const void*>(k_attn_drop_wide_bwd<T, DENSE>) : reinterpret_cast<const void*>(k_attn_drop_wide_fwd<T, DENSE>);
}
template <typename T, bool DENSE, bool BWD, typename P>
static int wide_launch(const P& p, unsigned grid, size_t lds, hipStream_t s) {
    static std::atomic<unsigned long long> done{0};  // (one per kernel instantiation)
    const void* kernel = wide_kernel<T, DENSE>(p, BWD);
    if (!wide_allow_lds(done, kernel, lds)) return MTLORA_ERR_HIP;
    void* args[] = {const_cast<P*>(&p)};
    if (hipLaunchKernel(kernel, dim3(grid), dim3(BWD ? WB_THREADS : W_THREADS), args, lds, s) != hipSuccess) return MTLORA_ERR_HIP;
    return MTLORA_OK;
}
template <bool BWD, typename P>
static int wide_dispatch(int dtype, bool dense, const P& p, unsigned grid, size_t lds, hipStream_t s) {
    return mtl_dispatch_dtype(dtype, [&](auto t) {
        return dense ? wide_launch<typename decltype(t)::type, true, BWD>(p, grid, lds, s) : wide_launch<typename decltype(t)::type, false, BWD>(p, grid, lds, s);
    });
}
template <typename P>
static int wide_fwd(const mtlora_attn_desc* d, P& p, hipStream_t s) {
    const bool dense = p.mask && !p.mask_ids;
    p.G = wide_groups(d, d->dtype != MTLORA_F32 && !dense ? 2 : 1);
    return wide_dispatch<false>(d->dtype, dense, p, (unsigned)(p.G * p.nH), wide_lds_bytes(d->dtype, p.N, false), s);
}
template <typename P>
static int wide_bwd(const mtlora_attn_desc* d, P& p, hipStream_t s) {
    p.G = wide_groups(d);
    const bool dense = p.mask && !p.mask_ids;
    return wide_dispatch<true>(d->dtype, dense, p, (unsigned)(p.G * p.nH), wide_lds_bytes(d->dtype, p.N, true, std::is_same<P, AttnDropParams>::value), s);
}
