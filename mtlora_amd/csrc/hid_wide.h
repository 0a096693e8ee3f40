// hid_wide.h -- k_hidr_*: the implicit task hidden tensors of hid.hip for task ranks 16 .. 128 (multiples of 16).  Included at the end of
// hid.hip (it uses its MFMA wrapper, GELU helpers and the swizzled [32][32] LDS images); launched by linear.hip through internal.h.
//
// At these ranks every product is GEMM work: the ranks are the k steps (r / 16) and the n tiles (r / 32, rounded up) of
// v_mfma_f32_32x32x16.  Everything is computed TRANSPOSED, "lane = row": the accumulator of the rank update is
//     h_t^T[c][m] = h_base^T + B1_t[c, :] P1_t[m, :]^T        A operand = b_cat rows (lane c), B operand = P rows (lane m)
// so lane (m = l & 31, hh = l >> 5) holds, of ROW m, the 16 hidden columns c(r) = (r & 3) + 8 (r >> 2) + 4 hh of the 32-column tile.
// Packed to 16 bits, registers 0..7 and 8..15 of that lane ARE the B operands of the two k steps of any product that contracts over the
// tile's columns (the k labelling of an MFMA is free as long as both operands agree): the other operand reads its 8 values per lane as two
// 8-byte runs (columns 4 kg .. + 3 and 8 + 4 kg .. + 3).  No trip through memory between GELU and the second product:
//     forward   P2_t^T[n][m] += A2_t[n, tile] a_t[m, tile]^T      backward   Q1_t^T[n][m] += B1_t[tile, n]^T dH_t[m, tile]^T
// and h_base / G enter and leave as 8-byte runs of their row.  The results come out as 4 consecutive rank columns per lane and register
// quad: 8-byte stores of P2, 16-byte fp32 rows of the Q1 table.
//
// k_hidr_fwd: one WAVE owns 32 rows and walks the whole hidden width, task by task: P2_t (<= 4 n tiles = 64 accumulator registers) leaves
//   the registers once, scaled by alpha2; no LDS, no barrier, no partials.  P1_t's k steps are held as fragments (<= 32 registers).
// k_hidr_bwd: ONE task per launch.  The factor gradients contract over ROWS, so their accumulators (dB1_t^T and dA2_t of the wave's 32
//   columns: 2 x 4 tiles x 16 registers) must stay with a fixed column slice through the persistent row loop: wave w of a 4-wave workgroup
//   owns columns 32 w of a 128-column chunk (grid y), the workgroup walks 32-row blocks (grid x).  Per block: P1 / Q2 rows -> swizzled LDS
//   images (zeros past M and past the rank); h_t^T and u^T = A2_t^T Q2_t^T by r / 16 MFMAs each; gelu, gelu', dH = u gelu'; G += dH (read
//   and written in place: the same lane owns the same addresses in every task's launch); Q1 tiles as above; then dH and a_t go through the
//   wave's image (row-major in, transposed out: hid_dl_store_t / hid_dl_raw) to become the B operands of the row contractions, whose A
//   operands are transposed reads of the P1 / Q2 images in the same row order.  Q1 of the four waves meets in an LDS table in a fixed
//   order ((w2 + w0) + (w3 + w1)), and goes unscaled to a (chunk, row) partial; k_hidr_rows_finish adds the chunks in order, scales by
//   alpha1 and stores 16-byte rank vectors.  The factor accumulators go to the workgroup's partial, k_hidr_reduce adds them in order.
// No atomics, no memset: bit-reproducible.

namespace {

template <typename T>
__device__ __forceinline__ void hidr_unpack4(const u32x2 w, f32x16& v, int q) {
    v[4 * q] = mtl_lo2<T>(w[0]);
    v[4 * q + 1] = mtl_hi2<T>(w[0]);
    v[4 * q + 2] = mtl_lo2<T>(w[1]);
    v[4 * q + 3] = mtl_hi2<T>(w[1]);
}
// the two k steps of a column-contracting operand: row `p` (H elements) at tile columns 4 kg + {0, 8} and 16 + 4 kg + {0, 8}
template <typename T>
__device__ __forceinline__ void hidr_col_frags(const T* p, bool on, u32x4& f0, u32x4& f1) {
    u32x2 a = {0u, 0u}, b = a, c = a, d = a;
    if (on) {
        a = *reinterpret_cast<const u32x2*>(p);
        b = *reinterpret_cast<const u32x2*>(p + 8);
        c = *reinterpret_cast<const u32x2*>(p + 16);
        d = *reinterpret_cast<const u32x2*>(p + 24);
    }
    f0 = u32x4{a[0], a[1], b[0], b[1]};
    f1 = u32x4{c[0], c[1], d[0], d[1]};
}

template <typename T>
__global__ __launch_bounds__(64) void k_hidr_fwd(const HidrFwdParams P) {
    const int lane = threadIdx.x, m = lane & 31, kg = lane >> 5;
    const int H = P.H;
    const T* hbase = reinterpret_cast<const T*>(P.hbase);
    const T* p1 = reinterpret_cast<const T*>(P.p1);
    const T* b1 = reinterpret_cast<const T*>(P.b1);
    const T* a2 = reinterpret_cast<const T*>(P.a2);
    T* p2 = reinterpret_cast<T*>(P.p2);
    const int64_t nblk = (P.M + 31) / 32;
    for (int64_t rb = blockIdx.x; rb < nblk; rb += gridDim.x) {
        const int64_t row = rb * 32 + m;
        const bool live = row < P.M;
        const int64_t rowc = live ? row : P.M - 1;
        for (int t = 0; t < P.nt; ++t) {
            const int o1 = P.off1[t], ks1 = P.r1[t] >> 4, o2 = P.off2[t], r2 = P.r2[t], nt2 = (r2 + 31) >> 5;
            u32x4 pf[8];
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                pf[ks] = u32x4{0u, 0u, 0u, 0u};
                if (ks < ks1 && live) pf[ks] = *reinterpret_cast<const u32x4*>(p1 + rowc * P.ld1 + o1 + 16 * ks + 8 * kg);
            }
            f32x16 acc[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
            const int n_l = m;  // (as the A operand's row: rank column n_l of tile j)
            for (int c0 = 0; c0 < H; c0 += 32) {
                f32x16 h;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    u32x2 w = {0u, 0u};
                    if (live) w = *reinterpret_cast<const u32x2*>(hbase + rowc * H + c0 + 8 * q + 4 * kg);
                    hidr_unpack4<T>(w, h, q);
                }
                const T* brow = b1 + (int64_t)(c0 + m) * P.ld1 + o1 + 8 * kg;  // (lane = column c0 + m of the tile)
#pragma unroll
                for (int ks = 0; ks < 8; ++ks)
                    if (ks < ks1) sp_mma1<T>(*reinterpret_cast<const u32x4*>(brow + 16 * ks), pf[ks], h);
                u32x4 x0, x1;
#pragma unroll
                for (int i4 = 0; i4 < 2; ++i4) {
                    f32x2 hv[4], av[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) hv[j] = f32x2{h[8 * i4 + 2 * j], h[8 * i4 + 2 * j + 1]};
                    hid_gelu2n_fwd<4>(hv, av);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t w = hid_pk<T>(av[j].x, av[j].y);
                        if (i4 == 0)
                            x0[j] = w;
                        else
                            x1[j] = w;
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < nt2) {
                        const int n = 32 * j + n_l;
                        const bool on = n < r2;
                        u32x4 f0, f1;
                        hidr_col_frags<T>(a2 + (int64_t)(o2 + (on ? n : 0)) * H + c0 + 4 * kg, on, f0, f1);
                        sp_mma1<T>(f0, x0, acc[j]);
                        sp_mma1<T>(f1, x1, acc[j]);
                    }
            }
            // lane (m, hh), tile j, register quad q: rank columns 32 j + 8 q + 4 hh .. + 3 of row m
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int n0 = 32 * j + 8 * q + 4 * kg;
                    if (live && n0 < r2) {
                        const f32x4 al = *reinterpret_cast<const f32x4*>(P.alpha2 + o2 + n0);
                        *reinterpret_cast<u32x2*>(p2 + row * P.ld2 + o2 + n0) =
                            u32x2{mtl_pack2<T>(acc[j][4 * q] * al[0], acc[j][4 * q + 1] * al[1]),
                                  mtl_pack2<T>(acc[j][4 * q + 2] * al[2], acc[j][4 * q + 3] * al[3])};
                    }
                }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_hidr_bwd(const HidrBwdParams P) {
    __shared__ __attribute__((aligned(16))) float red[2][32][HIDR_RS];
    __shared__ __attribute__((aligned(16))) unsigned char pimg[4 * 2048];   // P1 rows of the block: 4 rank tiles of [32][32]
    __shared__ __attribute__((aligned(16))) unsigned char qimg[4 * 2048];   // Q2 rows
    __shared__ __attribute__((aligned(16))) unsigned char wimgs[4 * 2048];  // one [32][32] image per wave
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = lane & 31, kg = lane >> 5;
    const int H = P.H, r1 = P.r1, r2 = P.r2, ks1 = r1 >> 4, ks2 = r2 >> 4, nt1 = (r1 + 31) >> 5, nt2 = (r2 + 31) >> 5;
    const int chunk = blockIdx.y, c0 = chunk * HIDR_HC + 32 * wave;
    const T* hbase = reinterpret_cast<const T*>(P.hbase);
    const T* gsrc = reinterpret_cast<const T*>(P.gsrc);
    T* gout = reinterpret_cast<T*>(P.g);
    const T* p1 = reinterpret_cast<const T*>(P.p1);
    const T* q2 = reinterpret_cast<const T*>(P.q2);
    unsigned char* wimg = wimgs + wave * 2048;
    // lane = hidden column c0 + m: its rank rows of b_cat (fc1) and at_cat (fc2), the A operands of the two rank updates
    const T* brow = reinterpret_cast<const T*>(P.b1) + (int64_t)(c0 + m) * P.ld1 + P.off1 + 8 * kg;
    const T* arow = reinterpret_cast<const T*>(P.a2t) + (int64_t)(c0 + m) * P.ld2 + P.off2 + 8 * kg;
    const T* b1t = reinterpret_cast<const T*>(P.b1t);
    f32x16 accB[4], accA[4];  // lane (c, hh): dB1^T / dA2 [rank 32 j + a(r)][column c0 + c]
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) accB[j][e] = accA[j][e] = 0.f;
    const int64_t nblk = (P.M + 31) / 32;
    for (int64_t rb = blockIdx.x; rb < nblk; rb += gridDim.x) {
        const int64_t m0 = rb * 32;
        for (int i = tid; i < 1024; i += 256) {  // (image, row, 16-byte vector 0..15 of the rank axis)
            const int img = i >> 9, row = (i >> 4) & 31, ch = i & 15;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (m0 + row < P.M && 8 * ch < (img ? r2 : r1))
                v = *reinterpret_cast<const u32x4*>(img ? q2 + (m0 + row) * P.ld2 + P.off2 + 8 * ch : p1 + (m0 + row) * P.ld1 + P.off1 + 8 * ch);
            *reinterpret_cast<u32x4*>((img ? qimg : pimg) + (ch >> 2) * 2048 + hid_off16(row, ch & 3)) = v;
        }
        __syncthreads();  // images complete; the previous block's reads of `red` are done
        const int64_t row = m0 + m;
        const bool live = row < P.M;
        const int64_t go = (live ? row : P.M - 1) * H + c0 + 4 * kg;
        f32x16 h, u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            u32x2 w = {0u, 0u};
            if (live) w = *reinterpret_cast<const u32x2*>(hbase + go + 8 * q);
            hidr_unpack4<T>(w, h, q);
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) u[e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const int io = (ks >> 1) * 2048 + hid_off16(m, (ks & 1) * 2 + kg);  // (lane = row m: rank columns 16 ks + 8 kg .. + 7)
            if (ks < ks1) sp_mma1<T>(*reinterpret_cast<const u32x4*>(brow + 16 * ks), *reinterpret_cast<const u32x4*>(pimg + io), h);
            if (ks < ks2) sp_mma1<T>(*reinterpret_cast<const u32x4*>(arow + 16 * ks), *reinterpret_cast<const u32x4*>(qimg + io), u);
        }
        u32x4 d0, d1, x0, x1;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            f32x2 av, gd;
            hid_gelu2(f32x2{h[2 * i], h[2 * i + 1]}, av, gd);
            const f32x2 dh = f32x2{u[2 * i], u[2 * i + 1]} * gd;
            u[2 * i] = dh.x;
            u[2 * i + 1] = dh.y;
            const uint32_t wd = hid_pk<T>(dh.x, dh.y), wa = hid_pk<T>(av.x, av.y);
            if (i < 4) {
                d0[i] = wd;
                x0[i] = wa;
            } else {
                d1[i - 4] = wd;
                x1[i - 4] = wa;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // G += dH_t, in place after the first task
            u32x2 w = {0u, 0u};
            if (gsrc && live) w = *reinterpret_cast<const u32x2*>(gsrc + go + 8 * q);
            const float g0 = mtl_lo2<T>(w[0]) + u[4 * q], g1 = mtl_hi2<T>(w[0]) + u[4 * q + 1];
            const float g2 = mtl_lo2<T>(w[1]) + u[4 * q + 2], g3 = mtl_hi2<T>(w[1]) + u[4 * q + 3];
            if (live) *reinterpret_cast<u32x2*>(gout + go + 8 * q) = u32x2{mtl_pack2<T>(g0, g1), mtl_pack2<T>(g2, g3)};
        }
        // Q1^T tiles of the wave's columns: lane (m, hh), register quad q = rank columns 32 j + 8 q + 4 hh .. + 3 of row m
        f32x16 accQ[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int e = 0; e < 16; ++e) accQ[j][e] = 0.f;
            if (j < nt1) {
                const int n = 32 * j + m;
                const bool on = n < r1;
                u32x4 f0, f1;
                hidr_col_frags<T>(b1t + (int64_t)(P.off1 + (on ? n : 0)) * H + c0 + 4 * kg, on, f0, f1);
                sp_mma1<T>(f0, d0, accQ[j]);
                sp_mma1<T>(f1, d1, accQ[j]);
            }
        }
        // row contractions: dH / a_t as [rows][columns] images, read back with the rows along the registers
        u32x4 t0, t1;
        hid_dl_store_t(wimg, lane, d0, d1);
        HID_LGKM0();
        __builtin_amdgcn_wave_barrier();
        hid_dl_raw(wimg, lane, t0, t1);
        HID_LGKM0();
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nt1) {
                u32x4 f0, f1;
                hid_dl_raw(pimg + j * 2048, lane, f0, f1);
                sp_mma1<T>(f0, t0, accB[j]);
                sp_mma1<T>(f1, t1, accB[j]);
            }
        hid_dl_store_t(wimg, lane, x0, x1);
        HID_LGKM0();
        __builtin_amdgcn_wave_barrier();
        hid_dl_raw(wimg, lane, t0, t1);
        HID_LGKM0();
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nt2) {
                u32x4 f0, f1;
                hid_dl_raw(qimg + j * 2048, lane, f0, f1);
                sp_mma1<T>(f0, t0, accA[j]);
                sp_mma1<T>(f1, t1, accA[j]);
            }
        // Q1 of the four waves: waves 2, 3 store, waves 0, 1 add theirs, then slot 0 + slot 1
        if (wave >= 2) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nt1)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        *reinterpret_cast<f32x4*>(&red[wave - 2][m][32 * j + 8 * q + 4 * kg]) =
                            f32x4{accQ[j][4 * q], accQ[j][4 * q + 1], accQ[j][4 * q + 2], accQ[j][4 * q + 3]};
        }
        __syncthreads();  // (also: every wave is done with the P1 / Q2 images)
        if (wave < 2) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nt1)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        f32x4* p = reinterpret_cast<f32x4*>(&red[wave][m][32 * j + 8 * q + 4 * kg]);
                        *p = *p + f32x4{accQ[j][4 * q], accQ[j][4 * q + 1], accQ[j][4 * q + 2], accQ[j][4 * q + 3]};
                    }
        }
        __syncthreads();
        const int r14 = r1 >> 2;
        for (int i = tid; i < 32 * r14; i += 256) {
            const int mm = i / r14, n4 = (i - mm * r14) * 4;
            if (m0 + mm < P.M)
                *reinterpret_cast<f32x4*>(P.rowpart + ((int64_t)chunk * P.M + m0 + mm) * r1 + n4) =
                    *reinterpret_cast<const f32x4*>(&red[0][mm][n4]) + *reinterpret_cast<const f32x4*>(&red[1][mm][n4]);
        }
    }
    // the wave's share of the factor gradients: lane (c, hh) holds rank rows 32 j + a(r) of column c0 + c
    float* part = P.part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (r1 + r2) * HIDR_HC + 32 * wave + m;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int n = 32 * j + (r & 3) + 8 * (r >> 2) + 4 * kg;
            if (n < r1) part[(int64_t)n * HIDR_HC] = accB[j][r];
            if (n < r2) part[(int64_t)(r1 + n) * HIDR_HC] = accA[j][r];
        }
}

// (chunk, row) partial row sums -> alpha-scaled 16-byte rank vectors of Q1
template <typename T>
__global__ __launch_bounds__(256) void k_hidr_rows_finish(const float* __restrict__ rowpart, int n_chunk, int64_t M, int r1, const float* alpha,
                                                          T* out, int ldo) {
    const int r8 = r1 >> 3;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * r8) return;
    const int64_t row = i / r8;
    const int n8 = (int)(i - row * r8) * 8;
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
    for (int ch = 0; ch < n_chunk; ++ch) {
        const float* p = rowpart + ((int64_t)ch * M + row) * r1 + n8;
        s0 += *reinterpret_cast<const f32x4*>(p);
        s1 += *reinterpret_cast<const f32x4*>(p + 4);
    }
    s0 *= *reinterpret_cast<const f32x4*>(alpha + n8);
    s1 *= *reinterpret_cast<const f32x4*>(alpha + n8 + 4);
    *reinterpret_cast<u32x4*>(out + row * ldo + n8) =
        u32x4{mtl_pack2<T>(s0[0], s0[1]), mtl_pack2<T>(s0[2], s0[3]), mtl_pack2<T>(s1[0], s1[1]), mtl_pack2<T>(s1[2], s1[3])};
}

__global__ __launch_bounds__(256) void k_hidr_reduce(const HidrRedParams P) {
    const int rr = P.r1 + P.r2;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)rr * P.H) return;
    const int n = (int)(i / P.H), c = (int)(i - (int64_t)n * P.H);
    float* dst = n < P.r1 ? P.dB1 : P.dA2;
    if (!dst) return;
    const int ch = c / HIDR_HC, cl = c - ch * HIDR_HC;
    const int64_t per_wg = (int64_t)rr * HIDR_HC;
    const float* src = P.part + (int64_t)ch * P.n_wg * per_wg + (int64_t)n * HIDR_HC + cl;
    float s0 = 0.f, s1 = 0.f;
    int w = 0;
    for (; w + 1 < P.n_wg; w += 2) {
        s0 += src[(int64_t)w * per_wg];
        s1 += src[(int64_t)(w + 1) * per_wg];
    }
    if (w < P.n_wg) s0 += src[(int64_t)w * per_wg];
    if (n < P.r1)
        dst[(int64_t)c * P.r1 + n] = s0 + s1;
    else
        dst[(int64_t)(n - P.r1) * P.H + c] = s0 + s1;
}

}  // namespace

MTL_INTERNAL void mtli_hidr_fwd(int dtype, const HidrFwdParams* q, int n_wg, void* stream) {
    mtl_dispatch_dtype16(dtype, [&](auto t) {
        hipLaunchKernelGGL(k_hidr_fwd<typename decltype(t)::type>, dim3((unsigned)n_wg), dim3(64), 0, (hipStream_t)stream, *q);
    });
}
MTL_INTERNAL void mtli_hidr_bwd(int dtype, const HidrBwdParams* q, int n_wg, int n_chunk, void* stream) {
    mtl_dispatch_dtype16(dtype, [&](auto t) {
        hipLaunchKernelGGL(k_hidr_bwd<typename decltype(t)::type>, dim3((unsigned)n_wg, (unsigned)n_chunk), dim3(256), 0, (hipStream_t)stream, *q);
    });
}
MTL_INTERNAL void mtli_hidr_rows_finish(int dtype, const float* rowpart, int n_chunk, int64_t M, int r1, const float* alpha, void* out, int ldo,
                                        void* stream) {
    const unsigned blocks = (unsigned)((M * (r1 >> 3) + 255) / 256);
    mtl_dispatch_dtype16(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(k_hidr_rows_finish<T>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, rowpart, n_chunk, M, r1, alpha,
                           reinterpret_cast<T*>(out), ldo);
    });
}
MTL_INTERNAL void mtli_hidr_reduce(const HidrRedParams* r, void* stream) {
    const int64_t per = (int64_t)(r->r1 + r->r2) * r->H;
    hipLaunchKernelGGL(k_hidr_reduce, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *r);
}
