// linear.hip -- MTLoRALinear forward / backward on CDNA4 (gfx950): the HOST side (validation, kernel selection, launchers, the C ABI).
// Replaces the ATen sequence of models/lora.py:253-284 and its autograd backward.
// The kernels live in the headers included below, all in this one translation unit: nt.h (k_pack, k_nt, k_ntl), stream.h (k_sp_*),
// dense.h (k_ntd / k_nte), pq.h (k_pq), tn.h (k_tn, k_sum, k_rank_out).
//
// Kernel families (all hand-written MFMA, 64-wide waves):
//
//   k_pack   fp32 LoRA masters -> compute-dtype packed factors: A_cat (R x K), B_cat (N x R), At_cat (K x R), Bt_cat (R x N),
//              alpha (R), the alpha-scaled projection rows a_proj / bt_proj and the fragment-major, k-permuted expansion
//              factors b_frag / at_frag of the wave-streaming kernels;   R = sum_o rp(o), every rank padded to 8 columns
//   k_sp_*   (stream.h) WAVE-STREAMING kernels, the default wherever a launch is eligible (16-bit types, stationary operands
//            fit in LDS): k_sp_xres / k_sp_ares = ONE launch per T = 0 layer and direction (projection kept in registers, no
//            P / Q pass, no re-read of X / dY; k_sp_xres also carries the GELU second output and the GELU' gate), k_sp_proj =
//            the P / Q passes of every other layer, k_sp_projsum = Q of all outputs + G = sum of the gradients in one pass
//            (T <= 4), k_sp_projk = P / Q with projection rows too large for LDS (single-round launches), k_sp_tn = the
//            factor gradients dA / dB with transposed LDS reads (large row counts)
//   k_ntd    (dense.h) single-output launches with a long reduction and well-filled residency rounds: 256 x 128 x 64 tiles,
//            global -> LDS ring of three stages running across the tiles of a persistent workgroup
//   k_rank_out  the task outputs of a dX launch with small task ranks (dX_t = Q_t A_t [.* gelu'(h_t)]) as a streaming kernel
//   k_nt     "NT" tile GEMM  D[n][m] = sum_k Wgt[n][k] * Act[m][k]  (128 x 128 tile, 4 or 8 waves per workgroup) run
//            as ONE software-pipelined stream of k-tiles over the base GEMM and every output's rank segment, with
//              - multi-source activation (sum of up to 1+T tensors formed while staging: G = dY_s + sum dY_t)
//              - optional dropout mask applied to the staged activation at LDS-store time (P = alpha * D(X) A^T)
//              - bias / per-row alpha epilogue, GELU second output (ACT), GELU' gate (GATE)
//              - multi-output low-rank parts: for each output o, extra k-tiles over the o-th rank segment of
//                L (M x R) and R (N x R) chained onto the base accumulator (Y_o = base + L_o R_o^T), optionally
//                masked (dX = G W + keep .* (Q A))
//            The MFMA "A" operand is the weight tile and "B" the activation tile, so a lane's four consecutive
//            accumulator registers are four consecutive output COLUMNS; the bf16 epilogue goes through LDS so that
//            stores are whole 128-byte row segments.   k_ntl = its single-output bf16 launches as straight-line code.
//   k_tn     "TN" split-M reduction  Out[a][b] = sum_m SrcA[m][a] * SrcB[m][b]  (dA = Q^T D(X), dB^T = P^T dY) with
//            64 (rank side) x 256 (wide side) tiles: both operands are read with the LDS transpose load
//            (ds_read_b64_tr_b16) for bf16; per-split partials (deterministic) + k_tn_reduce.
//   k_sum    G = sum of the output gradients (matrixv2 factors; pre-summed dX operand of wide outputs).
//
// Forward  = k_pack, then  k_sp_xres (T = 0, K <= 192)  |  k_sp_proj / k_sp_projk / k_nt (P), k_ntd / k_ntl / k_nt (all 1+T outputs).
// Backward = T = 0: k_sp_ares (narrow input) / k_sp_xres (wide input, short reduction, gate): Q + dX together
//            | else k_sp_projsum (Q + G, T <= 4) / [k_sum] k_sp_proj / k_sp_projk / k_nt (Q), then k_ntd / k_ntl / k_nt (dX) [+ k_rank_out (dX_t)];
//            k_sp_tn / k_tn + reduce for dA / dB.
// DESIGN.md section 4.1 / 4.3 has the measurements and the experiments that were tried and dropped.
#include <string.h>
#include <algorithm>
#include <atomic>
#include <type_traits>

#include "dispatch.h"
#include "internal.h"
#include "hid_params.h"
#include "nt.h"
#include "stream.h"
#include "dense.h"
#include "pq.h"
#include "tn.h"

namespace {

static Segs make_segs(const mtlora_linear_desc* d) {
    Segs s;
    s.n = 1 + d->T;
    int off = 0;
    for (int o = 0; o < s.n; ++o) {
        int r = (o == 0) ? d->r_s : d->r_t[o - 1];
        s.r[o] = r;
        // a segment is padded to ONE 16-byte vector of bf16 (8 columns), not to the 16-wide MFMA k granule: every consumer masks
        // per 16-byte vector (k_nt zero-fills the vectors past a part's k range on both operands, k_tn windows start on vector
        // boundaries), so r_t = 4 costs 8 columns of P / Q / factors instead of 16 -- R = 96 instead of 128 at C2's task layers,
        // 80 instead of 144 with 8 tasks of rank 4.  (Packing two 4-wide segments into one vector would need the P pass to merge
        // two different activation sources into one store: DESIGN.md 7.)
        s.rp[o] = (int)mtl_round_up(r, 8);
        s.off[o] = off;
        off += s.rp[o];
    }
    for (int o = s.n; o < MAXO; ++o) s.r[o] = s.rp[o] = s.off[o] = 0;
    s.used = off;
    s.R = (int)mtl_round_up(off, 16);  // row stride of P / Q: whole 32-byte pairs (the trailing pad columns are never read)
    return s;
}

static CtxLayout ctx_layout(const mtlora_linear_desc* d, const Segs& s) {
    const int es = mtl_elem_size(d->dtype);
    CtxLayout L;
    int64_t o = 0;
    auto take = [&](int64_t bytes) {
        int64_t at = o;
        o += mtl_round_up(bytes, 256);
        return at;
    };
    L.a_cat = take((int64_t)s.R * d->K * es);
    L.b_cat = take((int64_t)d->N * s.R * es);
    L.at_cat = take((int64_t)d->K * s.R * es);
    L.bt_cat = take((int64_t)s.R * d->N * es);
    L.alpha = take((int64_t)s.R * 4);
    L.a_proj = take((int64_t)s.R * d->K * es);   // alpha * A_cat   (projection rows of the wave-streaming forward / P pass)
    L.bt_proj = take((int64_t)s.R * d->N * es);  // alpha * Bt_cat  (projection rows of the wave-streaming dX / Q pass)
    // expansion factors of the wave-streaming kernels (stream.h), FRAGMENT-major and k-permuted: fragment (32-row block b,
    // 16-wide rank step t) = 1 KB, lane l = (row b*32 + (l & 31), h = l >> 5) holds the 8 rank columns
    // 16 t + 8 (s >> 2) + 4 h + (s & 3), s = 0..7 -- the order in which a lane holds P^T / Q^T after the projection MFMA
    // (rank steps padded to whole 32-row projection blocks: 2 * ceil(R / 32) steps per block, zero past the segments)
    L.b_frag = take(mtl_round_up(d->N, 32) * mtl_round_up(s.R, 32) * es);   // rows = output columns n:  B_cat[n][r]
    L.at_frag = take(mtl_round_up(d->K, 32) * mtl_round_up(s.R, 32) * es);  // rows = input columns k:   A_cat[r][k]
    L.pack_total = o;
    if (d->packed) o = 0;  // the factors live in the caller's buffer: ctx holds P alone
    L.p = take(d->M * s.R * es);
    L.total = o;
    return L;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static int check_desc(const mtlora_linear_desc* d) {
    if (!d) return MTLORA_ERR_NULL;
    if (!mtl_dtype_in(d->dtype, MTL_DT_ALL)) return MTLORA_ERR_DTYPE;
    if (d->M < 0 || d->K <= 0 || d->N <= 0 || d->T < 0 || d->T > MTLORA_MAX_TASKS || d->r_s < 0)
        return MTLORA_ERR_SHAPE;
    if (d->M >= ((int64_t)1 << 31)) return MTLORA_ERR_SHAPE;
    const int vec = mtl_vec_elems(d->dtype);
    if (d->K % vec || d->N % vec) return MTLORA_ERR_ALIGN;
    for (int t = 0; t < d->T; ++t)
        if (d->r_t[t] <= 0) return MTLORA_ERR_SHAPE;
    if (d->mode != 0 && d->mode != 1) return MTLORA_ERR_UNSUPPORTED;
    if (d->bwd_phase < 0 || d->bwd_phase > 2) return MTLORA_ERR_UNSUPPORTED;
    if (d->sel_stream < 0 || d->sel_stream > 1 || d->sel_dense < 0 || d->sel_dense > 4 || d->sel_tn < 0 || d->sel_tn > 2 || d->sel_projk < 0 ||
        d->sel_projk > 3 || d->max_cu < 0)
        return MTLORA_ERR_UNSUPPORTED;
    if (d->dropout_p < 0.f || d->dropout_p >= 1.f) return MTLORA_ERR_SHAPE;
    return MTLORA_OK;
}

static bool misaligned(const void* p) { return ((uintptr_t)p & 15u) != 0; }

// kernel selection of one call: a function of the descriptor alone (mtlora_linear_desc.sel_* / max_cu, ABI v6) -- the library reads
// no environment variables.  sp: wave-streaming family on; ntd / tn / projk: 0 never, 1 by heuristics, 2 whenever eligible (projk 3: k_pq
// whenever eligible).
struct Tune {
    int sp, ntd, tn, projk, max_cu;
};
static Tune make_tune(const mtlora_linear_desc* d) {
    auto tri = [](int v) { return v == 1 ? 0 : (v == 2 ? 2 : 1); };
    Tune t;
    t.sp = d->sel_stream == 1 ? 0 : 1;
    t.ntd = d->sel_dense >= 3 ? d->sel_dense : tri(d->sel_dense);  // (3: k_nte whenever eligible, 4: heuristics without k_nte)
    t.tn = tri(d->sel_tn);
    t.projk = d->sel_projk == 3 ? 3 : tri(d->sel_projk);  // (3: k_pq whenever eligible)
    t.max_cu = d->max_cu > 0 ? d->max_cu : 0;
    return t;
}
// per-device facts, cached (the only process-wide state next to the opt-in profiler): CU count and which kernels already had
// their dynamic-LDS limit raised on which device (hipFuncSetAttribute is per device)
constexpr int MTL_MAX_DEV = 64;
static int cur_dev() {
    int dev = 0;
    (void)hipGetDevice(&dev);
    return dev >= 0 && dev < MTL_MAX_DEV ? dev : 0;
}
static int dev_num_cu() {
    static std::atomic<int> cache[MTL_MAX_DEV];
    const int dev = cur_dev();
    int cu = cache[dev].load(std::memory_order_relaxed);
    if (cu == 0) {
        cu = 256;
        (void)hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev);
        if (cu <= 0) cu = 256;
        cache[dev].store(cu, std::memory_order_relaxed);
    }
    return cu;
}
static int num_cu(const Tune& tu) {
    const int cu = dev_num_cu();
    return tu.max_cu > 0 && tu.max_cu < cu ? tu.max_cu : cu;
}
// raise the dynamic-LDS limit of `fn` to `bytes` once per device; false when the runtime refuses (the caller falls back / reports)
static bool raise_lds(std::atomic<unsigned long long>& done, const void* fn, int bytes) {
    const int dev = cur_dev();
    if ((done.load(std::memory_order_relaxed) >> dev) & 1ull) return true;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    done.fetch_or(1ull << dev, std::memory_order_relaxed);
    return true;
}
// (a refusal is not an error here: the launch that follows fails with an invalid-configuration error, which the entry point's
// MTL_CHECK_LAUNCH reports as MTLORA_ERR_HIP)
#define MTL_RAISE_LDS(KERNEL, BYTES)                                        \
    do {                                                                    \
        static std::atomic<unsigned long long> done__{0};                   \
        (void)raise_lds(done__, (const void*)(KERNEL), (int)(BYTES));       \
    } while (0)

// k_nte (two 4-wave workgroups per CU) instead of k_ntd / k_ntl?  Measured per shape (tools/ntd_ab.sh, profiles/r04_ntd_ab.txt): it wins
// where a tile spends a large share of its life outside the k loop -- short reductions (<= 12 k-steps of 64) with at least 1.5 tiles per
// CU -- and where k_ntd's one-workgroup-per-CU rounds are badly filled (< 70 %) while every CU still gets a tile; it loses on long
// reductions with few tiles (stage 3 dX: half the waves per CU).
static bool nte_prefer(int64_t tiles, int ksteps, int64_t cus) {
    const double eff_d = (double)tiles / (double)(mtl_ceil_div(tiles, cus) * cus);
    return (ksteps >= 4 && ksteps <= 12 && tiles * 2 >= 3 * cus) || (ksteps >= 6 && eff_d < 0.7 && tiles >= cus);
}

// the compact parameter block of the single-output bf16 kernels (k_ntd / k_nte: dense, k_ntl) from the generic one.  `nt` column tiles
// per row of `mt` row tiles.  Only the dense kernels take a gate; they never see a masked activation (their eligibility excludes it).
static NlParams make_nl(const NtParams& P, int64_t mt, int64_t nt, bool dense) {
    NlParams q;
    q.act = reinterpret_cast<const bf16*>(P.act[0]);
    q.wgt = reinterpret_cast<const bf16*>(P.wgt);
    q.L = reinterpret_cast<const bf16*>(P.L);
    q.Rm = reinterpret_cast<const bf16*>(P.Rm);
    q.out = reinterpret_cast<bf16*>(P.out[0].ptr);
    q.act2 = reinterpret_cast<bf16*>(P.out[0].act);
    q.gate = dense ? reinterpret_cast<const bf16*>(P.out[0].gate) : nullptr;
    q.bias = P.bias;
    q.alpha = P.alpha;
    q.ld_act = P.ld_act;
    q.ld_wgt = P.ld_wgt;
    q.ldL = P.ldL;
    q.ldR = P.ldR;
    q.ld_out = P.ld_out;
    q.M = (int)P.M;
    q.n_rows = P.n_rows;
    q.K = P.act[0] ? P.K : 0;
    q.seg_lo = P.L ? P.out[0].seg_lo : 0;
    q.seg_hi = P.L ? P.out[0].seg_hi : 0;
    q.n_tiles = (int)nt;
    q.nt_magic = (uint32_t)(((uint64_t)1 << 32) / (uint64_t)nt) + 1u;
    const uint32_t nwg = (uint32_t)(mt * nt);
    q.q8 = nwg / 8u;
    q.r8 = nwg % 8u;
    q.act_mask = dense ? 0 : P.act_mask;
    q.use_base = P.out[0].use_base;
    q.drop = P.drop;
    return q;
}

// the <ACT, MLR, GATE> instance of a dense single-output kernel (k_ntd / k_nte): go(ACT, MLR, GATE) is called with the three as
// std::bool_constant values.  The GELU second output excludes the other two.  (k_ntl's ladder is over (act2, wide, ml0): on its own below.)
template <typename F>
static void nl_dispatch(const NlParams& q, bool ml0, F&& go) {
    using Y = std::true_type;
    using N = std::false_type;
    if (q.act2)
        go(Y{}, N{}, N{});
    else if (q.gate && ml0)
        go(N{}, Y{}, Y{});
    else if (q.gate)
        go(N{}, N{}, Y{});
    else if (ml0)
        go(N{}, Y{}, N{});
    else
        go(N{}, N{}, N{});
}

template <typename T>
static void launch_nt(const Tune& tu, const NtParams& P, hipStream_t s, int kind, double alg_bytes, double s8d_bytes = 0.0, double flops = 0.0) {
    mtl_prof_tag("M%lld K%d N%d ldL%lld no%d na%d nz%d", (long long)P.M, P.K, P.n_rows, (long long)P.ldL, P.n_out, P.n_act, P.nz);
    MtlProfScope prof(kind, alg_bytes, s, s8d_bytes, flops);
    int max_rows = P.n_rows;
    if (P.nz > 0) {
        max_rows = 0;
        for (int z = 0; z < P.nz; ++z) max_rows = P.zrows[z] > max_rows ? P.zrows[z] : max_rows;
    }
    const int64_t m_tiles = mtl_ceil_div(P.M, TILE);
    const int64_t n_tiles = mtl_ceil_div(max_rows, TILE);
    if (m_tiles * n_tiles == 0) return;
    dim3 g((unsigned)(m_tiles * n_tiles), 1, (unsigned)(P.nz > 0 ? P.nz : 1));
    int base_users = 0;
    for (int o = 0; o < P.n_out; ++o) base_users += P.out[o].use_base ? 1 : 0;
    const size_t lds = (size_t)STAGE_BYTES;
    // variant 0: several outputs share the base GEMM (MULTI: two accumulator sets, 4 waves); 1: multi-source activation (the dX
    // launch of a layer with task outputs); 2: one output, one source.  The 16-bit single-accumulator-set variants run 8 waves
    // per workgroup (<= 128 VGPRs, 4 waves per SIMD); MULTI and f32 (wider fragments) would spill at 128 and run 4.
    const int variant = base_users > 1 ? 0 : (P.n_act > 1 ? 1 : 2);
    constexpr bool W8 = sizeof(T) == 2;
    bool mlr = false, gated = false, acted = false;
    for (int o = 0; o < P.n_out; ++o) {
        mlr = mlr || P.out[o].mask_lr != 0;
        gated = gated || P.out[o].gate != nullptr;
        acted = acted || P.out[o].act != nullptr;
    }
    mlr = mlr && P.drop.enabled();
    if constexpr (std::is_same<T, bf16>::value) {
        // lean single-output bf16 launches (forward outputs, P / Q passes, rank-0 GEMMs, and the dX of layers without task
        // outputs -- masked rank part): the straight-line kernel
        // MFMA-dense launches (long reduction, enough tiles): k_ntd (dense.h).  MTLORA_NTD: 0 never, 2 whenever the shape allows
        const int ntd_mode = tu.ntd;  // 0 never, 1 by the heuristics below, 2 whenever the shape allows (the "[dense]" test variants)
        bool dense = false, use_e = false;
        int ksteps = 0;
        if (variant == 2 && P.n_out == 1 && P.nz == 0 && ntd_mode != 0 && P.act_mask == 0 && P.n_rows % 8 == 0 && P.n_rows >= 64 &&
            P.M < (int64_t)0x7FFFFF00 && P.out[0].ptr != nullptr && !(P.out[0].gate && P.out[0].act)) {
            const int seg = P.L ? P.out[0].seg_hi - P.out[0].seg_lo : 0;
            const int kk = (P.act[0] && P.out[0].use_base ? P.K : 0);
            ksteps = (seg + ND_KE - 1) / ND_KE + (kk + ND_KE - 1) / ND_KE;
            const int64_t tiles = mtl_ceil_div(P.M, ND_TM) * mtl_ceil_div(P.n_rows, ND_TN);
            const int64_t lim = ((int64_t)1 << 32) - 4096;
            const bool fits = P.M * P.ld_out * 2 < lim && P.M * P.ld_act * 2 < lim && P.M * P.ldL * 2 < lim && (int64_t)P.n_rows * P.ld_wgt * 2 < lim &&
                              (int64_t)P.n_rows * P.ldR * 2 < lim && P.K % 8 == 0 && seg % 8 == 0 && (P.ld_act % 8) == 0 && (P.ld_wgt % 8) == 0 &&
                              (P.ldL % 8) == 0 && (P.ldR % 8) == 0 && (P.L == nullptr || (P.out[0].seg_lo % 8) == 0);
            // where it wins (tools/ntd_ab.sh): a reduction of >= 6 k-tiles, residency rounds (one workgroup per CU) at least 70 % full or
            // a single round on at least half of the CUs, and no half-empty column tile
            const int64_t slots = num_cu(tu);
            const double eff = (double)tiles / (double)(mtl_ceil_div(tiles, slots) * slots);
            use_e = ntd_mode == 3 || (ntd_mode == 1 && nte_prefer(tiles, ksteps, slots) && (P.n_rows % ND_TN == 0 || P.n_rows > 2 * ND_TN));
            dense = fits && ksteps >= 1 &&
                    (ntd_mode == 2 || ntd_mode == 3 || use_e ||
                     (ksteps >= 6 && (eff >= 0.7 || (tiles <= slots && tiles >= slots / 2)) && (P.n_rows % ND_TN == 0 || P.n_rows > 2 * ND_TN)));
        }
        if (dense) {
            const int64_t mt = mtl_ceil_div(P.M, ND_TM), nt = mtl_ceil_div(P.n_rows, ND_TN);
            const NlParams q = make_nl(P, mt, nt, true);
            const bool ml0 = P.out[0].mask_lr != 0 && P.drop.enabled() && q.seg_hi > q.seg_lo;
            const uint32_t nwg = (uint32_t)(mt * nt), cus = (uint32_t)num_cu(tu);
            // k_nte: the same tile with two 4-wave workgroups per CU (dense.h); ntd_mode 3 forces it, 2 forces k_ntd
            nl_dispatch(q, ml0, [&](auto ac, auto ml, auto ga) {
                constexpr bool AC = decltype(ac)::value, ML = decltype(ml)::value, GA = decltype(ga)::value;
                if (use_e) {
                    MTL_RAISE_LDS((k_nte<AC, ML, GA>), SP_LDS_MAX);
                    hipLaunchKernelGGL((k_nte<AC, ML, GA>), dim3(nwg < 2u * cus ? nwg : 2u * cus), dim3(256), (size_t)NE_LDS, s, q);
                } else {
                    MTL_RAISE_LDS((k_ntd<AC, ML, GA>), SP_LDS_MAX);
                    hipLaunchKernelGGL((k_ntd<AC, ML, GA>), dim3(nwg < cus ? nwg : cus), dim3(512), (size_t)ND_LDS, s, q);
                }
            });
            return;
        }
        if (variant == 2 && P.n_out == 1 && P.out[0].gate == nullptr && P.nz == 0 && P.M < (int64_t)0x7FFFFF00 &&
            m_tiles * n_tiles < ((int64_t)1 << 28) && P.n_rows >= 8 && P.n_rows % 8 == 0) {
            if (P.out[0].ptr == nullptr) return;
            // tile width: 128 columns, or 192 when that saves residency rounds (512 workgroup slots at 128 columns, 2 per CU either way;
            // a 192-wide tile is 1.5x the work)
            const int64_t t128 = m_tiles * mtl_ceil_div(P.n_rows, 128), t192 = m_tiles * mtl_ceil_div(P.n_rows, 192);
            const int64_t slots = 2 * (int64_t)dev_num_cu();
            const double c128 = (double)mtl_ceil_div(t128, slots), c192 = 1.5 * (double)mtl_ceil_div(t192, slots);
            const bool wide = !P.out[0].act && P.n_rows >= 192 && c192 < c128 - 0.01;
            const int64_t nt = wide ? mtl_ceil_div(P.n_rows, 192) : n_tiles;
            const NlParams q = make_nl(P, m_tiles, nt, false);
            const bool ml0 = P.out[0].mask_lr != 0 && P.drop.enabled() && q.seg_hi > q.seg_lo;
            const uint32_t nwg = (uint32_t)(m_tiles * nt);
            constexpr size_t LDS192 = (size_t)(192 + 128) * LDSB;
#define MTL_NTL_GO(AC, ML, SNV, LDSV)                                                         \
    do {                                                                                      \
        if ((LDSV) > 64 * 1024) MTL_RAISE_LDS((k_ntl<AC, ML, SNV>), 160 * 1024 - 512);        \
        hipLaunchKernelGGL((k_ntl<AC, ML, SNV>), dim3(nwg), dim3(512), (size_t)(LDSV), s, q); \
    } while (0)
            if (q.act2)
                MTL_NTL_GO(true, false, 2, STAGE_BYTES);
            else if (wide && ml0)
                MTL_NTL_GO(false, true, 3, LDS192);
            else if (wide)
                MTL_NTL_GO(false, false, 3, LDS192);
            else if (ml0)
                MTL_NTL_GO(false, true, 2, STAGE_BYTES);
            else
                MTL_NTL_GO(false, false, 2, STAGE_BYTES);
#undef MTL_NTL_GO
            return;
        }
    }
#define MTL_NT_GO(MU, MSRC, ML, GA, AC)                                                                   \
    do {                                                                                                \
        if (W8 && !(MU))                                                                                \
            hipLaunchKernelGGL((k_nt<T, false, MSRC, ML, 8, GA, AC>), g, dim3(512), lds, s, P);         \
        else                                                                                            \
            hipLaunchKernelGGL((k_nt<T, MU, MSRC, ML, 4, GA, AC>), g, dim3(256), lds, s, P);            \
    } while (0)
    if (acted) {  // forward outputs with the GELU second output (fc1 of the Mlp): lean or MULTI
        if (variant == 0)
            MTL_NT_GO(true, false, false, false, true);
        else
            MTL_NT_GO(false, false, false, false, true);
    } else if (gated) {  // dX * gelu'(h) epilogue: the lean (single accumulator set) variants
        if (variant == 1)
            MTL_NT_GO(false, true, true, true, false);
        else if (mlr)
            MTL_NT_GO(false, false, true, true, false);
        else
            MTL_NT_GO(false, false, false, true, false);
    } else if (variant == 0) {
        MTL_NT_GO(true, false, false, false, false);
    } else if (variant == 1) {
        MTL_NT_GO(false, true, true, false, false);  // multi-source = the dX launch
    } else if (mlr) {
        MTL_NT_GO(false, false, true, false, false);
    } else {
        MTL_NT_GO(false, false, false, false, false);
    }
#undef MTL_NT_GO
}

// ---- wave-streaming projection (k_sp_proj, stream.h): the P = alpha D(X) A^T / Q = alpha dY B passes
// fills q.n_blk_total / n_slabs / n_items and returns the ring depth (0: not eligible).  Sources must be set.
template <typename T>
static int sp_proj_plan(const Tune& tu, SpProjParams& q, int& ch) {
    if (sizeof(T) != 2 || tu.sp == 0 || q.M <= 0 || q.n_src <= 0) return 0;
    ch = q.K % 96 == 0 ? 96 : (q.K % 64 == 0 ? 64 : 0);
    if (ch == 0 || q.M >= ((int64_t)1 << 31) - 64) return 0;
    q.n_blk_total = (q.Rw + 31) / 32;
    for (int s = 0; s < q.n_src; ++s) {
        if (q.src[s].n_blk > SP_MAXB || q.src[s].n_blk <= 0) return 0;
        if (((uintptr_t)q.src[s].act & 15u) != 0) return 0;
    }
    if ((q.ld_out % 8) != 0 || ((uintptr_t)q.out & 15u) != 0 || ((uintptr_t)q.wproj & 15u) != 0) return 0;
    if (q.M * q.ld_out * 2 >= ((int64_t)1 << 32) - 64) return 0;  // 32-bit store offsets (buffer descriptor)
    q.n_slabs = (int)mtl_ceil_div(q.M, 32);
    if ((int64_t)q.n_slabs * q.n_src >= ((int64_t)1 << 30)) return 0;
    q.n_items = q.n_slabs * q.n_src;
    const int64_t wbytes = (int64_t)q.n_blk_total * 32 * q.K * 2;
    const int64_t slot = 32 * ch * 2;
    for (int ns = 3; ns >= 1; --ns)
        if (wbytes + (int64_t)SP_WAVES * ns * slot <= SP_LDS_MAX) return ns;
    return 0;
}
template <typename T>
static void launch_sp_proj(const Tune& tu, const SpProjParams& q, int ch, int ns, hipStream_t s, int kind, double alg_bytes, double s8d, double flops) {
    mtl_prof_tag("sp_proj M%lld K%d R%d src%d ch%d ns%d", (long long)q.M, q.K, q.Rw, q.n_src, ch, ns);
    MtlProfScope prof(kind, alg_bytes, s, s8d, flops);
    const size_t lds = (size_t)q.n_blk_total * 32 * q.K * 2 + (size_t)SP_WAVES * ns * 32 * ch * 2;
    const int per_cu = lds * 2 <= (size_t)SP_LDS_MAX ? 2 : 1;
    int64_t wgs = mtl_ceil_div(q.n_items, SP_WAVES);
    if (wgs > (int64_t)num_cu(tu) * per_cu) wgs = (int64_t)num_cu(tu) * per_cu;
#define MTL_SP_PROJ(CHV, NSV)                                                                              \
    do {                                                                                                   \
        MTL_RAISE_LDS((k_sp_proj<T, CHV, NSV>), SP_LDS_MAX);                                               \
        hipLaunchKernelGGL((k_sp_proj<T, CHV, NSV>), dim3((unsigned)wgs), dim3(64 * SP_WAVES), lds, s, q); \
    } while (0)
    if constexpr (sizeof(T) == 2) {
        if (ch == 96) {
            if (ns == 3) MTL_SP_PROJ(96, 3);
            else if (ns == 2) MTL_SP_PROJ(96, 2);
            else MTL_SP_PROJ(96, 1);
        } else {
            if (ns == 3) MTL_SP_PROJ(64, 3);
            else if (ns == 2) MTL_SP_PROJ(64, 2);
            else MTL_SP_PROJ(64, 1);
        }
    }
#undef MTL_SP_PROJ
}

// ---- k_pq (pq.h): the P / Q passes whose projection rows do not fit in LDS: 64- or 128-row tiles with a deep LDS-DMA ring, one grid
// slice (blockIdx.z) per source with its column segment.  Fills `pq`, returns the row blocks per wave (1: 64-row tiles, 2: 128-row
// tiles; 0: not eligible).
template <typename T>
static int pq_plan(const Tune& tu, const SpProjParams& q, PqParams& pq) {
    if (sizeof(T) != 2 || tu.sp == 0 || tu.projk == 0 || tu.projk == 2 || q.M <= 0 || q.n_src < 1 || q.n_src > MAXO) return 0;
    if (q.Rw % 8 != 0 || q.K % 8 != 0 || q.K < 32 || (q.ld_out % 8) != 0) return 0;
    if ((((uintptr_t)q.wproj | (uintptr_t)q.out) & 15u) != 0) return 0;
    if (q.M >= ((int64_t)1 << 31) - 256 || q.M * q.ld_out * 2 >= ((int64_t)1 << 32) - 64) return 0;
    int wmax = 0;
    for (int s = 0; s < q.n_src; ++s) {
        const SpSrc& ss = q.src[s];
        if (((uintptr_t)ss.act & 15u) != 0 || ss.col_lo % 8 != 0 || ss.col_hi % 8 != 0 || ss.col_hi <= ss.col_lo || ss.col_hi > q.Rw) return 0;
        if (ss.col_hi - ss.col_lo > 1024) return 0;  // (<= 8 column tiles per source)
        pq.src[s].act = ss.act;
        pq.src[s].col_lo = ss.col_lo;
        pq.src[s].col_hi = ss.col_hi;
        pq.src[s].mask = ss.mask;
        pq.src[s].pad_ = 0;
        wmax = ss.col_hi - ss.col_lo > wmax ? ss.col_hi - ss.col_lo : wmax;
    }
    pq.n_src = q.n_src;
    pq.wproj = q.wproj;
    pq.out = q.out;
    pq.ld_out = q.ld_out;
    pq.M = (int)q.M;
    pq.K = q.K;
    pq.R = q.Rw;
    pq.drop = q.drop;
    // 64-row tiles while the launch is about one residency round (a workgroup per CU), 128-row tiles beyond
    const int64_t per_row_tile = (int64_t)q.n_src * mtl_ceil_div(wmax, wmax > 64 ? 128 : 64);
    return mtl_ceil_div(q.M, 64) * per_row_tile * 4 <= (int64_t)num_cu(tu) * 5 ? 1 : 2;
}
static bool pq_one_round(const Tune& tu, const PqParams& pq, int mb) {
    return pq.n_src == 1 && mtl_ceil_div(pq.M, 64 * mb) * 4 <= (int64_t)num_cu(tu) * 5;
}
template <typename T>
static void launch_pq(const PqParams& pq, int mb, hipStream_t s, int kind, double alg_bytes, double s8d, double flops) {
    int wmax = 0, any_mask = 0;
    for (int i = 0; i < pq.n_src; ++i) {
        wmax = pq.src[i].col_hi - pq.src[i].col_lo > wmax ? pq.src[i].col_hi - pq.src[i].col_lo : wmax;
        any_mask |= pq.src[i].mask;
    }
    mtl_prof_tag("pq M%d K%d R%d src%d w%d mb%d mask%d", pq.M, pq.K, pq.R, pq.n_src, wmax, mb, any_mask);
    MtlProfScope prof(kind, alg_bytes, s, s8d, flops);
    const bool wide = wmax > 64;
    const dim3 grid((unsigned)mtl_ceil_div(pq.M, 64 * mb), (unsigned)mtl_ceil_div(wmax, wide ? 128 : 64), (unsigned)pq.n_src);
#define MTL_PQ(WMV, NBV, NSTV, KSV)                                                                               \
    do {                                                                                                          \
        constexpr size_t lds = (size_t)NSTV * (32 * WMV + 32 * NBV) * 64;                                         \
        MTL_RAISE_LDS((k_pq<T, WMV, NBV, NSTV, KSV>), SP_LDS_MAX);                                                \
        hipLaunchKernelGGL((k_pq<T, WMV, NBV, NSTV, KSV>), grid, dim3(256), lds, s, pq);                          \
    } while (0)
    if constexpr (sizeof(T) == 2) {
        const bool ksp = any_mask != 0 && pq.drop.enabled();  // (masked: every activation fragment hashed by one wave)
        if (mb == 1 && wide && ksp) MTL_PQ(2, 4, 6, true);   // 64 x 128: 12 KB stages, 60 KB in flight
        else if (mb == 1 && wide) MTL_PQ(2, 4, 6, false);
        else if (mb == 1 && ksp) MTL_PQ(2, 2, 8, true);      // 64 x 64:   8 KB stages, 56 KB in flight
        else if (mb == 1) MTL_PQ(2, 2, 8, false);
        else if (wide) MTL_PQ(4, 4, 5, false);               // 128 x 128: 16 KB stages, 64 KB in flight
        else MTL_PQ(4, 2, 6, false);                         // 128 x 64: 12 KB stages, 60 KB in flight
    }
#undef MTL_PQ
}

// ---- k_sp_projk (stream.h): the P / Q passes whose projection rows do not fit in LDS, for small row counts (one work item per
// workgroup, reduction split over its waves).  Same parameter block as k_sp_proj; returns false when the shape is not eligible.
template <typename T>
static bool sp_projk_plan(const Tune& tu, SpProjParams& q, int& ch) {
    if (sizeof(T) != 2 || tu.sp == 0 || q.M <= 0 || q.n_src <= 0) return false;
    const int mode = tu.projk;
    if (mode == 0) return false;
    ch = q.K % 96 == 0 ? 96 : (q.K % 64 == 0 ? 64 : 0);
    if (ch == 0 || q.M >= ((int64_t)1 << 31) - 64) return false;
    q.n_blk_total = (q.Rw + 31) / 32;
    for (int s = 0; s < q.n_src; ++s) {
        if (q.src[s].n_blk > SP_MAXB || q.src[s].n_blk <= 0) return false;
        if (((uintptr_t)q.src[s].act & 15u) != 0) return false;
    }
    if ((q.ld_out % 8) != 0 || ((uintptr_t)q.out & 15u) != 0 || ((uintptr_t)q.wproj & 15u) != 0) return false;
    if (q.M * q.ld_out * 2 >= ((int64_t)1 << 32) - 64) return false;
    q.n_slabs = (int)mtl_ceil_div(q.M, 32);
    q.n_items = q.n_slabs * q.n_src;
    // every item re-reads the projection rows from L2 and pays three barriers: it wins while the whole launch is ONE residency round
    // (stage 3: 196 slabs; 42 - 62 us -> 20 - 24 us), ties at two to three rounds and loses beyond (tools/projk_ab.sh)
    return mode == 2 || (mode == 1 && (int64_t)q.n_items <= (int64_t)num_cu(tu) && q.K / ch >= SP_WAVES);
}
template <typename T>
static void launch_sp_projk(const Tune& tu, const SpProjParams& q, int ch, hipStream_t s, int kind, double alg_bytes, double s8d, double flops) {
    mtl_prof_tag("sp_projk M%lld K%d R%d src%d ch%d", (long long)q.M, q.K, q.Rw, q.n_src, ch);
    MtlProfScope prof(kind, alg_bytes, s, s8d, flops);
    int64_t wgs = q.n_items;
    if (wgs > (int64_t)num_cu(tu)) wgs = num_cu(tu);
#define MTL_SP_PROJK(CHV, NSLV)                                                                                   \
    do {                                                                                                          \
        constexpr size_t slots = (size_t)SP_WAVES * NSLV * 32 * CHV * 2, red = (size_t)SP_WAVES * SP_MAXB * 4096; \
        constexpr size_t lds = slots > red ? slots : red;                                                         \
        MTL_RAISE_LDS((k_sp_projk<T, CHV, NSLV>), SP_LDS_MAX);                                                    \
        hipLaunchKernelGGL((k_sp_projk<T, CHV, NSLV>), dim3((unsigned)wgs), dim3(64 * SP_WAVES), lds, s, q);      \
    } while (0)
    if constexpr (sizeof(T) == 2) {
        if (ch == 96)
            MTL_SP_PROJK(96, 3);
        else
            MTL_SP_PROJK(64, 4);
    }
#undef MTL_SP_PROJK
}

template <typename T>
static void launch_sp_projsum(const Tune& tu, const SpProjParams& q, int ch, int ns, T* gsum, hipStream_t s, int kind, double alg_bytes,
                              double s8d, double flops) {
    mtl_prof_tag("sp_projsum M%lld K%d R%d src%d ch%d ns%d", (long long)q.M, q.K, q.Rw, q.n_src, ch, ns);
    MtlProfScope prof(kind, alg_bytes, s, s8d, flops);
    const size_t lds = (size_t)q.n_blk_total * 32 * q.K * 2 + (size_t)SP_WAVES * ns * 32 * ch * 2;
    int64_t wgs = mtl_ceil_div(q.n_slabs, SP_WAVES);
    if (wgs > (int64_t)num_cu(tu)) wgs = num_cu(tu);
#define MTL_SP_PS(CHV, NSV)                                                                                         \
    do {                                                                                                            \
        MTL_RAISE_LDS((k_sp_projsum<T, CHV, NSV>), SP_LDS_MAX);                                                     \
        hipLaunchKernelGGL((k_sp_projsum<T, CHV, NSV>), dim3((unsigned)wgs), dim3(64 * SP_WAVES), lds, s, q, gsum); \
    } while (0)
    if constexpr (sizeof(T) == 2) {
        if (ch == 96) {
            if (ns >= 2) MTL_SP_PS(96, 2);
            else MTL_SP_PS(96, 1);
        } else {
            if (ns >= 2) MTL_SP_PS(64, 2);
            else MTL_SP_PS(64, 1);
        }
    }
#undef MTL_SP_PS
}

// ---- fused wave-streaming MTLoRALinear launch, activation-resident form (k_sp_xres, stream.h).  Fills the plan fields of q
// (n_parts, blk_per_part, n_slabs, estep) and the launch geometry; false: not eligible (weights do not fit / unsupported shape).
struct SpXresPlan {
    int ch, nkc, nrb;
    bool stg;
    unsigned grid;
    size_t lds;
};
// persistent grid of a fused wave-streaming launch: `parts` column parts x slab groups.  Normally the parts of one slab group sit on
// one XCD (blockIdx b -> XCD b % 8), so the groups come in eights (xsh = 3).  With fewer than 8 * parts CUs to use (desc.max_cu: the
// "[persist]" tests) the eight-fold grouping is dropped (xsh = 0): part = b % parts, group = b / parts.
static unsigned sp_lin_grid(const Tune& tu, int parts, int n_slabs, int& xsh) {
    const int64_t cu = num_cu(tu);
    const int64_t by_slabs = mtl_ceil_div(n_slabs, SP_WAVES);
    if (cu >= 8 * (int64_t)parts) {
        xsh = 3;
        int64_t g8 = mtl_ceil_div(by_slabs, 8);
        const int64_t g8_max = cu / (8 * parts);
        if (g8 > g8_max) g8 = g8_max;
        return (unsigned)(8 * parts * g8);
    }
    xsh = 0;
    int64_t g = cu / parts > 0 ? cu / parts : 1;
    if (g > by_slabs) g = by_slabs;
    return (unsigned)(parts * g);
}
template <typename T>
static bool sp_xres_plan(const Tune& tu, SpLinParams& q, int K, SpXresPlan& pl) {
    if (sizeof(T) != 2 || tu.sp == 0 || q.M <= 0 || q.M >= ((int64_t)1 << 31) - 64) return false;
    if (K == 96 || K == 192) {
        pl.ch = 96;
        pl.nkc = K / 96;
    } else if (K == 64 || K == 128) {
        pl.ch = 64;
        pl.nkc = K / 64;
    } else {
        return false;
    }
    if (q.R <= 0 || q.R > 128 || (q.R % 16) != 0) return false;
    pl.nrb = q.R <= 32 ? 1 : (q.R <= 64 ? 2 : 4);
    q.estep = 2 * ((q.R + 31) / 32);
    if ((q.n_cols % 8) != 0 || (q.ld_out % 8) != 0 || (q.ldp % 8) != 0) return false;
    if (q.M * q.ld_out * 2 >= ((int64_t)1 << 32) - 64 || q.M * q.ldp * 2 >= ((int64_t)1 << 32) - 64) return false;  // 32-bit store offsets
    const void* ptrs[] = {q.act, q.w, q.proj, q.expand, q.out, q.out2, q.pout, q.gate};
    for (const void* pp : ptrs)
        if (((uintptr_t)pp & 15u) != 0) return false;
    const int nb_all = (q.n_cols + 31) / 32;
    const int64_t slot = (int64_t)SP_WAVES * 32 * pl.ch * 2;
    auto fit = [&](bool stg, int& bpp_out, size_t& lds_out) -> int {
        const int64_t fixed = (int64_t)pl.nrb * 32 * K * 2 + slot + (stg ? (int64_t)SP_WAVES * SP_STG : 0);
        for (int np = 1; np <= nb_all && np <= 16; ++np) {
            const int bpp = (nb_all + np - 1) / np;
            if ((bpp * (np - 1)) >= nb_all) continue;  // an empty last part
            const int64_t need = fixed + (int64_t)bpp * (32 * K * 2 + 64 * pl.nrb * 32 * 2 / 2 + 128);
            if (need <= SP_LDS_MAX) {
                bpp_out = bpp;
                lds_out = (size_t)need;
                return np;
            }
        }
        return 0;
    };
    int bpp_d = 0, bpp_s = 0;
    size_t lds_d = 0, lds_s = 0;
    const int np_d = fit(false, bpp_d, lds_d), np_s = fit(true, bpp_s, lds_s);
    const bool stg = np_s > 0 && (np_d == 0 || np_s <= np_d + 1);
    const int parts = stg ? np_s : np_d;
    if (parts == 0) return false;
    pl.stg = stg;
    q.blk_per_part = stg ? bpp_s : bpp_d;
    pl.lds = stg ? lds_s : lds_d;
    q.n_parts = parts;
    q.n_slabs = (int)mtl_ceil_div(q.M, 32);
    pl.grid = sp_lin_grid(tu, parts, q.n_slabs, q.xsh);
    return true;
}
template <typename T>
static void launch_sp_xres(const SpLinParams& q, const SpXresPlan& pl, bool act, hipStream_t s, int kind, double alg_bytes, double s8d,
                           double flops, bool gate = false) {
    mtl_prof_tag("sp_xres M%lld K%d N%d R%d parts%d stg%d", (long long)q.M, pl.ch * pl.nkc, q.n_cols, q.R, q.n_parts, pl.stg ? 1 : 0);
    MtlProfScope prof(kind, alg_bytes, s, s8d, flops);
#define MTL_SP_X1(CHV, NKCV, NRBV, ACTV, STGV, GAV)                                                                             \
    do {                                                                                                                        \
        MTL_RAISE_LDS((k_sp_xres<T, CHV, NKCV, NRBV, ACTV, STGV, GAV>), SP_LDS_MAX);                                            \
        hipLaunchKernelGGL((k_sp_xres<T, CHV, NKCV, NRBV, ACTV, STGV, GAV>), dim3(pl.grid), dim3(64 * SP_WAVES), pl.lds, s, q); \
    } while (0)
#define MTL_SP_X(CHV, NKCV, NRBV, ACTV, STGV)                                    \
    do {                                                                         \
        if (!(ACTV) && gate) MTL_SP_X1(CHV, NKCV, NRBV, false, STGV, true);      \
        else MTL_SP_X1(CHV, NKCV, NRBV, ACTV, STGV, false);                      \
    } while (0)
#define MTL_SP_X_S(CHV, NKCV, NRBV, ACTV)                        \
    do {                                                         \
        if (pl.stg) MTL_SP_X(CHV, NKCV, NRBV, ACTV, true);       \
        else MTL_SP_X(CHV, NKCV, NRBV, ACTV, false);             \
    } while (0)
#define MTL_SP_X_R(CHV, NKCV, ACTV)                            \
    do {                                                       \
        if (pl.nrb == 1) MTL_SP_X_S(CHV, NKCV, 1, ACTV);       \
        else if (pl.nrb == 2) MTL_SP_X_S(CHV, NKCV, 2, ACTV);  \
        else MTL_SP_X_S(CHV, NKCV, 4, ACTV);                   \
    } while (0)
#define MTL_SP_X_K(ACTV)                                                  \
    do {                                                                  \
        if (pl.ch == 96 && pl.nkc == 1) MTL_SP_X_R(96, 1, ACTV);          \
        else if (pl.ch == 96) MTL_SP_X_R(96, 2, ACTV);                    \
        else if (pl.nkc == 1) MTL_SP_X_R(64, 1, ACTV);                    \
        else MTL_SP_X_R(64, 2, ACTV);                                     \
    } while (0)
    if constexpr (sizeof(T) == 2) {
        if (act) MTL_SP_X_K(true);
        else MTL_SP_X_K(false);
    }
#undef MTL_SP_X_K
#undef MTL_SP_X_R
#undef MTL_SP_X_S
#undef MTL_SP_X
#undef MTL_SP_X1
}

// ---- fused wave-streaming launch, accumulator-resident form (k_sp_ares, stream.h): few output columns, any reduction length
struct SpAresPlan {
    int ch, nob, nrb;
    bool expg;  // expansion fragments from global memory instead of LDS (k_sp_ares<..., EXPG>)
    unsigned grid;
    size_t lds;
};
template <typename T>
static bool sp_ares_plan(const Tune& tu, SpLinParams& q, int Kred, SpAresPlan& pl) {
    if (sizeof(T) != 2 || tu.sp == 0 || q.M <= 0 || q.M >= ((int64_t)1 << 31) - 64) return false;
    pl.ch = Kred % 96 == 0 ? 96 : (Kred % 64 == 0 ? 64 : 0);
    if (pl.ch == 0) return false;
    pl.nob = pl.ch == 96 ? 3 : 4;
    pl.expg = false;
    if (q.R <= 0 || q.R > 128 || (q.R % 16) != 0) return false;
    pl.nrb = q.R <= 64 ? 2 : 4;
    q.estep = 2 * ((q.R + 31) / 32);
    q.estep2 = Kred;
    if ((q.n_cols % 8) != 0 || (q.ld_out % 8) != 0 || (q.ldp % 8) != 0) return false;
    if (q.M * q.ld_out * 2 >= ((int64_t)1 << 32) - 64 || q.M * q.ldp * 2 >= ((int64_t)1 << 32) - 64) return false;
    const void* ptrs[] = {q.act, q.w, q.proj, q.expand, q.out, q.pout};
    for (const void* pp : ptrs)
        if (((uintptr_t)pp & 15u) != 0) return false;
    const int nb_all = (q.n_cols + 31) / 32;
    const int parts = (nb_all + pl.nob - 1) / pl.nob;
    if (parts > 2) return false;  // every part re-reads the activation: only worth it for narrow outputs
    const int64_t kst = Kred / 16;
    int64_t need = (int64_t)pl.nob * kst * 1024 + (int64_t)pl.nrb * kst * 1024 + (int64_t)pl.nob * 2 * pl.nrb * 1024 + pl.nob * 128 +
                   (int64_t)SP_WAVES * 32 * pl.ch * 2;
    if (need > SP_LDS_MAX && nb_all <= 3 && Kred % 64 == 0 && pl.nrb == 2) {
        // a long reduction with a 64-wide rank (stage-0 fc2 forward / fc1 dX: 384 -> 96): 64-wide slots, three output blocks and the
        // expansion fragments left in global memory (k_sp_ares<T, 64, 3, 2, EXPG>)
        pl.ch = 64;
        pl.nob = 3;
        pl.expg = true;
        need = (int64_t)pl.nob * kst * 1024 + (int64_t)pl.nrb * kst * 1024 + pl.nob * 128 + (int64_t)SP_WAVES * 32 * pl.ch * 2;
    }
    if (need > SP_LDS_MAX) return false;
    pl.lds = (size_t)need;
    q.n_parts = parts;
    q.blk_per_part = pl.nob;
    q.n_slabs = (int)mtl_ceil_div(q.M, 32);
    pl.grid = sp_lin_grid(tu, parts, q.n_slabs, q.xsh);
    return true;
}
template <typename T>
static void launch_sp_ares(const SpLinParams& q, const SpAresPlan& pl, hipStream_t s, int kind, double alg_bytes, double s8d, double flops) {
    mtl_prof_tag("sp_ares M%lld Kred%d N%d R%d parts%d", (long long)q.M, q.estep2, q.n_cols, q.R, q.n_parts);
    MtlProfScope prof(kind, alg_bytes, s, s8d, flops);
#define MTL_SP_A(CHV, NOBV, NRBV)                                                                              \
    do {                                                                                                       \
        MTL_RAISE_LDS((k_sp_ares<T, CHV, NOBV, NRBV>), SP_LDS_MAX);                                            \
        hipLaunchKernelGGL((k_sp_ares<T, CHV, NOBV, NRBV>), dim3(pl.grid), dim3(64 * SP_WAVES), pl.lds, s, q); \
    } while (0)
    if constexpr (sizeof(T) == 2) {
        if (pl.expg) {
            MTL_RAISE_LDS((k_sp_ares<T, 64, 3, 2, true>), SP_LDS_MAX);
            hipLaunchKernelGGL((k_sp_ares<T, 64, 3, 2, true>), dim3(pl.grid), dim3(64 * SP_WAVES), pl.lds, s, q);
        } else if (pl.ch == 96) {
            if (pl.nrb == 2) MTL_SP_A(96, 3, 2);
            else MTL_SP_A(96, 3, 4);
        } else {
            if (pl.nrb == 2) MTL_SP_A(64, 4, 2);
            else MTL_SP_A(64, 4, 4);
        }
    }
#undef MTL_SP_A
}

// k_pack of one layer into the packed-factor region at `pk` (the head of a forward's ctx buffer, or the caller's persistent
// buffer of mtlora_linear_pack)
// ---- wave-streaming factor gradients (k_sp_tn, stream.h).  Geometry is a function of the layer shape only (the scratch size
// must not depend on the device): part width 32 nb columns (nb = 4 when K and N are multiples of 128, 3 when multiples of 96),
// ~SP_TN_WGS workgroups dealt to the pps in row groups of 8.
constexpr int SP_TN_WGS = 256;
static int sp_tn_nb(const mtlora_linear_desc* d) {
    if (mtl_elem_size(d->dtype) != 2 || d->M <= 0 || d->M >= ((int64_t)1 << 31) - 64) return 0;
    if (d->K % 128 == 0 && d->N % 128 == 0) return 4;
    if (d->K % 96 == 0 && d->N % 96 == 0) return 3;
    return 0;
}
static int sp_tn_groups(const Tune& tu, int n_pp, int64_t M) {
    int G = SP_TN_WGS / (n_pp > 0 ? n_pp : 1);  // one resident round of workgroups, every workgroup the same number of rows
    if (tu.max_cu > 0) {  // (tests: as if the device had max_cu CUs -- fewer row groups, more slabs per wave)
        const int cap = tu.max_cu / (n_pp > 0 ? n_pp : 1);
        G = G < cap ? G : (cap > 0 ? cap : 1);
    }
    const int64_t by_rows = mtl_ceil_div(mtl_ceil_div(M, 32), SP_WAVES);  // no more waves than slabs
    if (G > by_rows) G = (int)by_rows;
    return G < 1 ? 1 : G;
}
// blockIdx -> (pp, row group).  Placement units are dealt largest first, each to the XCD with the least load so far.  coarse: a unit
// is every pp that reads the same narrow MATRIX for one row group (all dA problems read Q, all dB problems P: their column windows
// share cache lines); fine: one (problem, narrow tile).  Coarse is kept when no XCD gets more than its 32 CUs' worth of workgroups.
// Returns the grid size (0: does not fit the table).
static unsigned sp_tn_map_units(SpTnParams& q, bool coarse, int& max_load) {
    int load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    constexpr int CAP = SP_TN_MAP / 8;
    for (int i = 0; i < SP_TN_MAP; ++i) q.map[i] = 0xFFFFFFFFu;
    // unit list: [first problem, last problem] ranges over a problem order in which equal narrow matrices are adjacent
    int order[2 * MAXO], n = q.n_prob;
    for (int i = 0; i < n; ++i) order[i] = i;
    auto size_of = [&](int i) { return q.p[i].tiles_a * q.p[i].parts; };
    auto class_size = [&](int i) {
        int sz = 0;
        for (int j = 0; j < n; ++j)
            if (q.p[j].A == q.p[i].A) sz += size_of(j);
        return sz;
    };
    for (int i = 1; i < n; ++i)
        for (int j = i; j > 0; --j) {
            const int a = order[j], b = order[j - 1];
            const int ka = coarse ? class_size(a) : size_of(a), kb = coarse ? class_size(b) : size_of(b);
            const bool before = ka > kb || (ka == kb && coarse && q.p[a].A < q.p[b].A && q.p[a].A != q.p[b].A);
            if (!before) break;
            std::swap(order[j], order[j - 1]);
        }
    auto place = [&](int lo, int hi, int ta_lo, int ta_hi, int g) -> bool {  // problems order[lo..hi), narrow tiles [ta_lo, ta_hi)
        int sz = 0;
        for (int oi = lo; oi < hi; ++oi) sz += (std::min(ta_hi, q.p[order[oi]].tiles_a) - std::min(ta_lo, q.p[order[oi]].tiles_a)) * q.p[order[oi]].parts;
        int x = 0;
        for (int k = 1; k < 8; ++k)
            if (load[k] < load[x]) x = k;
        if (load[x] + sz > CAP) return false;
        for (int oi = lo; oi < hi; ++oi) {
            const SpTnProb& p = q.p[order[oi]];
            for (int ta = ta_lo; ta < ta_hi && ta < p.tiles_a; ++ta)
                for (int c = 0; c < p.parts; ++c) q.map[8 * (load[x]++) + x] = (uint32_t)(p.pp_lo + ta * p.parts + c) | ((uint32_t)g << 16);
        }
        return true;
    };
    for (int lo = 0; lo < n;) {
        int hi = lo + 1;
        if (coarse)
            while (hi < n && q.p[order[hi]].A == q.p[order[lo]].A) ++hi;
        int tmax = 0;
        for (int oi = lo; oi < hi; ++oi) tmax = std::max(tmax, q.p[order[oi]].tiles_a);
        for (int g = 0; g < q.G; ++g) {
            if (coarse) {
                if (!place(lo, hi, 0, tmax, g)) return 0;
            } else {
                for (int ta = 0; ta < tmax; ++ta)
                    if (!place(lo, hi, ta, ta + 1, g)) return 0;
            }
        }
        lo = hi;
    }
    max_load = 0;
    for (int k = 0; k < 8; ++k) max_load = std::max(max_load, load[k]);
    return (unsigned)(8 * max_load);
}
static unsigned sp_tn_map(SpTnParams& q) {
    // largest row-group count (from the one-round estimate down to 3 fewer) for which no XCD holds more than 32 workgroups (a
    // second residency round on one XCD doubles the launch); coarse units when they cost at most 5 % of the workgroups
    int mx = 0;
    const int G0 = q.G;
    int g_fine = 0, g_coarse = 0;
    for (int G = G0; G >= 1 && G >= G0 - 3 && g_fine == 0; --G) {
        q.G = G;
        if (sp_tn_map_units(q, false, mx) != 0 && mx <= 32) g_fine = G;
    }
    for (int G = G0; G >= 1 && G >= G0 - 3 && g_coarse == 0; --G) {
        q.G = G;
        if (sp_tn_map_units(q, true, mx) != 0 && mx <= 32) g_coarse = G;
    }
    if (g_coarse > 0 && g_coarse * 20 >= (g_fine > 0 ? g_fine : G0) * 19) {
        q.G = g_coarse;
        return sp_tn_map_units(q, true, mx);
    }
    q.G = g_fine > 0 ? g_fine : G0;
    return sp_tn_map_units(q, false, mx);
}
// Tune.tn (desc.sel_tn): 0 tiled k_tn only, 2 streaming whenever the shape allows, 1 (default): streaming when every wave gets
// >= 8 slabs (below that the launch is latency-bound and the tiled kernel's 64-row chunks win: measured on the stage-2 / 3 shapes)
static int64_t sp_tn_part_bytes(const mtlora_linear_desc* d, const Segs& sg) {
    const int nb = sp_tn_nb(d);
    if (nb == 0) return 0;
    int64_t n_pp = 0;
    for (int o = 0; o < sg.n; ++o)
        if (sg.rp[o] > 0) n_pp += mtl_ceil_div(sg.rp[o], 64) * (d->N / (32 * nb) + d->K / (32 * nb));
    const int64_t wgs = n_pp > SP_TN_WGS ? n_pp : SP_TN_WGS;
    return wgs * (2 * nb * 1024) * 4;
}
template <typename T>
static void launch_sp_tn(SpTnParams& q, int nb, hipStream_t s, double xb, double fl, const char* tag) {
    if constexpr (sizeof(T) == 2) {
        q.n_slabs = (int)mtl_ceil_div(q.M, 32);
        const unsigned grid = sp_tn_map(q);  // (q.G set by the caller; the caller checked that the table fits)
        {
            mtl_prof_tag("sp_tn %s np%d pp%d G%d nb%d", tag, q.n_prob, q.n_pp, q.G, nb);
            MtlProfScope prof(PK_TN, xb, s, xb, fl);
#define MTL_SP_TN(NBV, NSV)                                                                     \
    do {                                                                                        \
        constexpr size_t lds = (size_t)SP_WAVES * NSV * (SP_TN_NARROW + 32 * NBV * 64);         \
        MTL_RAISE_LDS((k_sp_tn<T, NBV, NSV>), SP_LDS_MAX);                                      \
        hipLaunchKernelGGL((k_sp_tn<T, NBV, NSV>), dim3(grid), dim3(64 * SP_WAVES), lds, s, q); \
    } while (0)
            if (nb == 4)
                MTL_SP_TN(4, 1);
            else
                MTL_SP_TN(3, 2);
#undef MTL_SP_TN
        }
        MtlProfScope prof(PK_REDUCE, 0.0, s);
        if (nb == 4)
            hipLaunchKernelGGL(k_sp_tn_reduce<4>, dim3(8, (unsigned)q.n_pp), dim3(256 * SP_TN_RG), 0, s, q);
        else
            hipLaunchKernelGGL(k_sp_tn_reduce<3>, dim3(6, (unsigned)q.n_pp), dim3(256 * SP_TN_RG), 0, s, q);
    }
}

// scale_dev (nullable; 1 + T entries, each nullable): a set entry makes k_pack read that segment's scale from the device and
// multiply it by the factor the host would have multiplied in; d->scale_* is read for the other segments only.  This is the ONLY
// place the library reads d->scale_s / d->scale_t: a call with d->packed set never packs, so it never looks at them.
static PackParams make_pack_params(const mtlora_linear_desc* d, const Segs& sg, const float* A_s, const float* B_s, const float* const* A_t,
                                   const float* const* B_t, const float* const* scale_dev = nullptr) {
    const float keep_scale = mtl_make_dropout(d->dropout_p, 0).enabled() ? 1.f / (1.f - d->dropout_p) : 1.f;
    PackParams pp;
    pp.s = sg;
    pp.K = (int)d->K;
    pp.N = (int)d->N;
    for (int o = 0; o < MAXO; ++o) {
        pp.A[o] = nullptr;
        pp.B[o] = nullptr;
        pp.alpha[o] = 0.f;
        pp.alpha_dev[o] = nullptr;
    }
    pp.A[0] = A_s;
    pp.B[0] = B_s;
    pp.alpha[0] = d->scale_s * keep_scale;
    for (int t = 0; t < d->T; ++t) {
        pp.A[t + 1] = A_t[t];
        pp.B[t + 1] = B_t[t];
        pp.alpha[t + 1] = d->scale_t[t] * (d->has_x_tasks ? 1.f : keep_scale);
    }
    for (int o = 0; scale_dev && o <= d->T; ++o)
        if (scale_dev[o]) {
            pp.alpha_dev[o] = scale_dev[o];
            pp.alpha[o] = (o == 0 || !d->has_x_tasks) ? keep_scale : 1.f;
        }
    return pp;
}
static unsigned pack_blocks(const mtlora_linear_desc* d, const Segs& sg) {
    const int64_t tr = mtl_ceil_div(sg.R, PK_T);
    int64_t blocks = tr * (mtl_ceil_div(d->K, PK_T) + mtl_ceil_div(d->N, PK_T));  // one 64 x 64 tile of A_cat / B_cat per workgroup
    if (blocks > 2048) blocks = 2048;
    return (unsigned)(blocks > 0 ? blocks : 1);
}
template <typename T>
static void launch_pack(const mtlora_linear_desc* d, const Segs& sg, const CtxLayout& L, unsigned char* pk, const float* A_s,
                        const float* B_s, const float* const* A_t, const float* const* B_t, hipStream_t s,
                        const float* const* scale_dev = nullptr) {
    const PackParams pp = make_pack_params(d, sg, A_s, B_s, A_t, B_t, scale_dev);
    MtlProfScope prof(PK_PACK, 0.0, s);
    hipLaunchKernelGGL(k_pack<T>, dim3(pack_blocks(d, sg)), dim3(256), 0, s, pp, reinterpret_cast<T*>(pk + L.a_cat),
                       reinterpret_cast<T*>(pk + L.b_cat), reinterpret_cast<T*>(pk + L.at_cat), reinterpret_cast<T*>(pk + L.bt_cat),
                       reinterpret_cast<float*>(pk + L.alpha), reinterpret_cast<T*>(pk + L.a_proj),
                       reinterpret_cast<T*>(pk + L.bt_proj), reinterpret_cast<T*>(pk + L.b_frag), reinterpret_cast<T*>(pk + L.at_frag));
}

// ---- the P / Q passes: Out[:, columns of source i] = alpha * f_i(Act_i) Wp^T   (P = alpha D(X) A^T per input, Q = alpha dY_o B_o per
// output).  One source list feeds every kernel that can run them.
struct ProjSrc {
    const void* act;     // (M x K) contiguous
    int col_lo, col_hi;  // columns of Out (rows of the factor) this source owns
    int mask;            // dropout keep-mask on the activation
};
static SpProjParams make_sp_proj(const ProjSrc* src, int n_src, const void* wproj, void* out, const Segs& sg, int64_t M, int K,
                                 const DropoutCfg& dc) {
    SpProjParams sp = {};
    sp.wproj = wproj;
    sp.out = out;
    sp.ld_out = sg.R;
    sp.M = M;
    sp.K = K;
    sp.Rw = sg.R;
    sp.drop = dc;
    for (int i = 0; i < n_src; ++i) {
        SpSrc& ss = sp.src[sp.n_src++];
        ss.act = src[i].act;
        ss.col_lo = src[i].col_lo;
        ss.col_hi = src[i].col_hi;
        ss.blk_lo = ss.col_lo / 32;
        ss.n_blk = (ss.col_hi - 1) / 32 - ss.blk_lo + 1;
        ss.mask = src[i].mask;
    }
    return sp;
}
// the factor side, the output and the profiler figures of one P / Q pass
template <typename T>
struct ProjJob {
    const void* wproj;   // (R x K) alpha-scaled factor rows (a_proj / bt_proj): the wave-streaming kernels and k_pq
    const T* wcat;       // the same rows unscaled ...
    const float* alpha;  // ... and their per-row alpha: k_nt
    T* out;              // (M x R)
    int64_t M;
    int K;
    bool one_panel;      // k_nt takes the single source as ONE (M x R) panel (pad columns included) instead of the batched form
    int kind;            // profiler kind
    double alg_bytes, s8d, flops;
};
template <typename T>
static void launch_proj(const Tune& tu, const Segs& sg, const DropoutCfg& dc, hipStream_t s, const ProjSrc* src, int n_src, const ProjJob<T>& j) {
    if (n_src == 0) return;
    // wave-streaming form (stream.h) when the alpha-scaled factor rows fit in LDS next to the slab ring
    SpProjParams sp = make_sp_proj(src, n_src, j.wproj, j.out, sg, j.M, j.K, dc);
    int ch = 0;
    const int ns = sp_proj_plan<T>(tu, sp, ch);
    PqParams pq = {};
    const int mb = pq_plan<T>(tu, sp, pq);
    // k_pq first: forced (3: the "[pq]" test family), instead of a one-slot k_sp_proj ring (which cannot overlap its loads), and
    // instead of k_sp_proj for launches of about one residency round (tools/pq_times.py: stage 2 of Swin-T 13 vs 16 us, Swin-B 14
    // vs 21 us); where k_sp_proj does not fit at all, k_sp_projk's single-round rule comes first (stage 3: 15 vs 21 us)
    if (mb > 0 && (tu.projk == 3 || ns == 1 || (ns > 1 && pq_one_round(tu, pq, mb)))) {
        launch_pq<T>(pq, mb, s, j.kind, j.alg_bytes, j.s8d, j.flops);
    } else if (ns > 0) {
        launch_sp_proj<T>(tu, sp, ch, ns, s, j.kind, j.alg_bytes, j.s8d, j.flops);
    } else if (sp_projk_plan<T>(tu, sp, ch)) {
        launch_sp_projk<T>(tu, sp, ch, s, j.kind, j.alg_bytes, j.s8d, j.flops);
    } else if (mb > 0) {
        launch_pq<T>(pq, mb, s, j.kind, j.alg_bytes, j.s8d, j.flops);
    } else {
        NtParams q = {};
        q.n_act = 1;
        q.ld_act = j.K;
        q.wgt = j.wcat;
        q.ld_wgt = j.K;
        q.M = j.M;
        q.K = j.K;
        q.alpha = j.alpha;
        q.n_out = 1;
        q.out[0].ptr = j.out;
        q.out[0].use_base = 1;
        q.ld_out = sg.R;
        q.drop = dc;
        if (j.one_panel) {
            q.act[0] = src[0].act;
            q.act_mask = src[0].mask;
            q.n_rows = sg.R;
        } else {
            for (int i = 0; i < n_src; ++i) {
                q.zact[i] = src[i].act;
                q.zrow0[i] = src[i].col_lo;
                q.zrows[i] = src[i].col_hi - src[i].col_lo;
                q.zmask[i] = src[i].mask;
            }
            q.nz = n_src;
        }
        launch_nt<T>(tu, q, s, j.kind, j.alg_bytes, j.s8d, j.flops);
    }
}

// sum of the un-padded ranks: of every output, or of the outputs o with a gradient (live[o] != null)
static double rank_sum(const Segs& sg, const void* const* live = nullptr) {
    double rsum = 0.0;
    for (int o = 0; o < sg.n; ++o)
        if (!live || (sg.rp[o] > 0 && live[o])) rsum += sg.r[o];
    return rsum;
}
// a T = 0 layer in ONE launch, either direction: 8(d) bytes (input + output) and the flops of the base GEMM and both rank GEMMs
static double fused_bytes(const mtlora_linear_desc* d, int es) { return (double)es * d->M * (d->K + (double)d->N); }
static double fused_flops(const mtlora_linear_desc* d, const Segs& sg) {
    return 2.0 * d->M * (double)d->K * d->N + 2.0 * d->M * (double)sg.r[0] * (d->K + d->N);
}

// T = 0 layers: ONE wave-streaming launch (projection kept in registers, stream.h) instead of the P pass + the output launch
template <typename T>
static bool fwd_one_pass(const mtlora_linear_desc* d, const Tune& tu, const Segs& sg, const CtxLayout& L, const unsigned char* pk, const void* x,
                         const void* W, const float* bias, void* y_s, void* a_s, T* Pm, const DropoutCfg& dc, hipStream_t s) {
    SpLinParams q = {};
    q.act = x;
    q.w = W;
    q.proj = pk + L.a_proj;
    q.expand = pk + L.b_frag;
    q.bias = bias;
    q.out = y_s;
    q.out2 = a_s;
    q.pout = Pm;
    q.ld_out = d->N;
    q.ldp = sg.R;
    q.M = d->M;
    q.n_cols = (int)d->N;
    q.R = sg.R;
    q.mask_act = 1;
    q.mask_lr = 0;
    q.drop = dc;
    SpXresPlan pl;
    const double b8d = fused_bytes(d, (int)sizeof(T)), fl = fused_flops(d, sg);
    // a short reduction: the activation-resident form
    if (sp_xres_plan<T>(tu, q, (int)d->K, pl)) {
        launch_sp_xres<T>(q, pl, a_s != nullptr, s, PK_NT_FWD_MAIN, b8d + (a_s ? (double)sizeof(T) * d->M * d->N : 0.0), b8d, fl);
        return true;
    }
    // a long reduction into few output columns (the Mlp's fc2 at stage 0: 384 -> 96): the accumulator-resident form, whose
    // projection sees the dropout-masked activation -- the P pass and its re-read of X disappear here too
    SpAresPlan pa;
    q.estep = q.estep2 = 0;
    if (a_s == nullptr && sp_ares_plan<T>(tu, q, (int)d->K, pa)) {
        launch_sp_ares<T>(q, pa, s, PK_NT_FWD_MAIN, b8d, b8d, fl);
        return true;
    }
    return false;
}

template <typename T>
static int fwd_impl(const mtlora_linear_desc* d, const void* x, const void* const* x_t, const void* W,
                    const float* bias, const float* A_s, const float* B_s, const float* const* A_t,
                    const float* const* B_t, void* y_s, void* const* y_t, void* ctx, hipStream_t s, void* a_s = nullptr,
                    void* const* a_t = nullptr) {
    const Segs sg = make_segs(d);
    const Tune tu = make_tune(d);
    const CtxLayout L = ctx_layout(d, sg);
    unsigned char* c = reinterpret_cast<unsigned char*>(ctx);
    unsigned char* pk = d->packed ? const_cast<unsigned char*>(reinterpret_cast<const unsigned char*>(d->packed)) : c;
    T* a_cat = reinterpret_cast<T*>(pk + L.a_cat);
    T* b_cat = reinterpret_cast<T*>(pk + L.b_cat);
    float* alpha = reinterpret_cast<float*>(pk + L.alpha);
    T* Pm = reinterpret_cast<T*>(c + L.p);
    const DropoutCfg dc = mtl_make_dropout(d->dropout_p, d->seed, d->seed_offset);

    if (sg.R > 0) {
        if (!d->packed) launch_pack<T>(d, sg, L, pk, A_s, B_s, A_t, B_t, s);
        if (d->T == 0 && d->mode == 0 && fwd_one_pass<T>(d, tu, sg, L, pk, x, W, bias, y_s, a_s, Pm, dc, s)) return MTLORA_OK;

        // P = alpha * D(X) A^T  (per source: x for every column, or x / the tasks' own inputs for their segments)
        const bool own = d->T > 0 && d->has_x_tasks;
        ProjSrc src[MAXO];
        int n_src = 0;
        if (!own) src[n_src++] = ProjSrc{x, 0, sg.used, 1};
        for (int o = 0; own && o < sg.n; ++o) {
            if (sg.rp[o] == 0) continue;
            if (o > 0 && (d->hid & MTLORA_HID_P_GIVEN)) continue;  // (task columns of P: mtlora_mlp_hid_proj wrote them)
            src[n_src++] = ProjSrc{o == 0 ? x : x_t[o - 1], sg.off[o], sg.off[o] + sg.rp[o], o == 0 ? 1 : 0};
        }
        // (HID_P_GIVEN: the tasks' own inputs are read -- implicitly -- by k_hid_proj, which carries their 8(d) bytes)
        const double xb = (double)sizeof(T) * ((d->has_x_tasks && !(d->hid & MTLORA_HID_P_GIVEN)) ? d->T : 0) * d->M * d->K;
        // (n_src == 0: r_s = 0 and the task columns are given -- nothing to launch)
        ProjJob<T> j = {};
        j.wproj = pk + L.a_proj;
        j.wcat = a_cat;
        j.alpha = alpha;
        j.out = Pm;
        j.M = d->M;
        j.K = (int)d->K;
        j.one_panel = !own;
        j.kind = PK_NT_FWD_P;
        j.alg_bytes = j.s8d = xb;
        j.flops = 2.0 * d->M * d->K * rank_sum(sg);
        launch_proj<T>(tu, sg, dc, s, src, n_src, j);
    }

    // all outputs
    NtParams m = {};
    m.act[0] = x;
    m.n_act = 1;
    m.ld_act = d->K;
    m.wgt = W;
    m.ld_wgt = d->K;
    m.M = d->M;
    m.n_rows = (int)d->N;
    m.K = (int)d->K;
    m.bias = bias;
    m.L = Pm;
    m.ldL = sg.R;
    m.Rm = b_cat;
    m.ldR = sg.R;
    m.ld_out = d->N;
    m.drop = dc;
    m.n_out = 1 + d->T;
    for (int o = 0; o < sg.n; ++o) {
        NtOut& O = m.out[o];
        O.ptr = (o == 0) ? y_s : y_t[o - 1];
        O.seg_lo = sg.off[o];
        O.seg_hi = sg.off[o] + sg.rp[o];
        O.use_base = 1;
        O.mask_lr = 0;
        O.fold = (o == 0 && d->mode == 1 && d->T > 0) ? 1 : 0;
        O.act = (o == 0) ? a_s : (a_t ? a_t[o - 1] : nullptr);
    }
    if (d->hid & MTLORA_HID_FWD_BASE) {  // the Mlp's fc1 with implicit task hiddens: the shared output and the bare pretrained product
        m.n_out = 2;
        NtOut& O = m.out[1];
        O.ptr = const_cast<void*>(d->hid_ptr);
        O.seg_lo = O.seg_hi = 0;
        O.use_base = 1;
        O.mask_lr = 0;
        O.fold = 0;
        O.act = nullptr;
    }
    int n_actout = 0;  // GELU second outputs: one more M x N write each
    for (int o = 0; o < m.n_out; ++o) n_actout += m.out[o].act ? 1 : 0;
    const double b8d = (double)sizeof(T) * d->M * (d->K + (double)(1 + d->T) * d->N);  // (SURVEY 8(d) counts every module output)
    const double fl = 2.0 * d->M * d->K * d->N + 2.0 * d->M * d->N * rank_sum(sg);
    const bool plain = sg.R == 0;
    launch_nt<T>(tu, m, s, plain ? PK_NT_PLAIN_FWD : PK_NT_FWD_MAIN, b8d + (double)sizeof(T) * d->M * (double)n_actout * d->N,
                 plain ? 0.0 : b8d, fl);
    return MTLORA_OK;
}

constexpr int64_t TN_TARGET_CTAS = 512;
struct BwdScratch {
    int64_t q, g, part, total;
    int nsplit;
    int64_t rows_per_split;
};
static BwdScratch bwd_scratch(const mtlora_linear_desc* d, const Segs& sg) {
    const int es = mtl_elem_size(d->dtype);
    BwdScratch S;
    int64_t o = 0;
    auto take = [&](int64_t bytes) {
        int64_t at = o;
        o += mtl_round_up(bytes, 256);
        return at;
    };
    S.q = take(d->M * sg.R * es);
    S.g = take(d->T > 0 ? d->M * d->N * es : 0);  // G = sum of the output gradients (matrixv2 factors; pre-summed dX operand)
    // TN tiles (rank side x wide side), dB and dA per output
    int64_t tiles = 0;
    for (int oo = 0; oo < sg.n; ++oo) {
        if (sg.rp[oo] == 0) continue;
        tiles += mtl_ceil_div(sg.rp[oo], TN_A) * mtl_ceil_div(d->N, TN_B);  // dB (as P^T dY)
        tiles += mtl_ceil_div(sg.rp[oo], TN_A) * mtl_ceil_div(d->K, TN_B);  // dA
    }
    // <= 512 workgroups = 2 per CU, all resident; >= 256 rows per split so that the fp32 partial tiles stay a small part of the traffic
    int nsplit = 1;
    if (tiles > 0) {
        nsplit = (int)(TN_TARGET_CTAS / tiles);  // floor: the whole grid is resident at once (no second round)
        const int64_t max_by_rows = mtl_ceil_div(d->M, 256);
        if (nsplit > max_by_rows) nsplit = (int)max_by_rows;
        if (nsplit > 256) nsplit = 256;
        if (nsplit < 1) nsplit = 1;
    }
    S.nsplit = nsplit;
    int64_t rps = mtl_ceil_div(d->M > 0 ? d->M : 1, nsplit);
    rps = mtl_round_up(rps, 64);
    S.rows_per_split = rps;
    {
        const int64_t tiled = tiles * nsplit * (int64_t)TN_TILE * 4, streamed = sp_tn_part_bytes(d, sg);
        S.part = take(tiled > streamed ? tiled : streamed);
    }
    S.total = o;
    return S;
}

// ---- backward: the state shared by its stages
template <typename T>
struct Bwd {
    const mtlora_linear_desc* d;
    Segs sg;
    Tune tu;
    CtxLayout L;
    BwdScratch S;
    hipStream_t s;
    DropoutCfg dc;
    const unsigned char* pk;  // packed factors
    const T *at_cat, *bt_cat, *Pm;
    const float* alpha;
    T *Qm, *Gm;
    float* part;
    const void* x;
    const void* const* x_t;
    const void* Wt;
    void* dx;
    void* const* dx_t;
    float *dA_s, *dB_s;
    float* const* dA_t;
    float* const* dB_t;
    const void* gate_s;
    const void* const* gate_t;
    const void* dy[MAXO];      // gradient of output o (null: none)
    const void* dy_all[MAXO];  // the n_dy gradients that exist
    int n_dy;
    const void* dyo[MAXO];     // gradient feeding factor o (matrixv2: the shared factors see G)
    bool do_dx;                // (bwd_phase 2 re-derives the same operand table without the dX launches)
    bool hid_q;                // fc1 of an Mlp with implicit task hiddens (hid.hip): Q task columns given
    bool presum;               // the dX launch reads G instead of re-summing the n_dy sources
    bool have_g;               // G is (to be) materialised in Gm
    bool q_done;               // Q came out of the k_sp_projsum pass
};

// G = sum of every output gradient, materialised when
//  * matrixv2: the shared factors see G, or
//  * the dX kernel would otherwise re-sum the n_dy sources once per output n-tile (it re-reads every dY panel for
//    each of the ceil(K/128) n-tiles: 3..24x for fc2): one k_sum pass + the single-source kernel moves
//    (n_dy + 1 + n_tiles) MN bytes instead of n_dy * n_tiles * MN.
// Fills dyo.
template <typename T>
static void bwd_grad_sum(Bwd<T>& b) {
    const mtlora_linear_desc* d = b.d;
    const Segs& sg = b.sg;
    const bool v2 = d->mode == 1 && d->T > 0;
    b.presum = b.n_dy > 1 && b.dx && mtl_ceil_div(d->K, TILE) >= 3;
    b.have_g = false;
    // layers with task outputs ('matrix' mode, every output has a gradient): ONE wave-streaming pass over the 1 + T gradient
    // tensors forms Q (all segments) AND G = sum_o dY_o (k_sp_projsum, stream.h); the dX launch then reads G alone
    b.q_done = false;
    if constexpr (sizeof(T) == 2) {
        if (d->T >= 1 && d->mode == 0 && b.do_dx && b.dx && b.n_dy == 1 + d->T && sg.rp[0] > 0 && sg.rp[0] <= 64) {
            ProjSrc src[MAXO];
            bool ok = true;
            for (int o = 0; o < sg.n; ++o) {
                if (sg.rp[o] == 0 || (o > 0 && sg.rp[o] > 32)) ok = false;
                src[o] = ProjSrc{b.dy[o], sg.off[o], sg.off[o] + sg.rp[o], 0};
            }
            SpProjParams sp = make_sp_proj(src, sg.n, b.pk + b.L.bt_proj, b.Qm, sg, d->M, (int)d->N, b.dc);
            for (int o = 1; o < sg.n; ++o)
                if (sp.src[o].n_blk != 1) ok = false;
            if (ok && sp.src[sp.n_src - 1].blk_lo - sp.src[1].blk_lo + 1 > SP_PS_MAXT) ok = false;  // task segments span too many blocks
            int ch = 0;
            const int ns = ok ? sp_proj_plan<T>(b.tu, sp, ch) : 0;
            if (ns > 0 && d->M * d->N * 2 < ((int64_t)1 << 32) - 64) {
                launch_sp_projsum<T>(b.tu, sp, ch, ns, b.Gm, b.s, PK_NT_BWD_Q, 0.0, 0.0, 2.0 * d->M * d->N * rank_sum(sg));
                b.q_done = true;
                b.presum = true;
                b.have_g = true;
            }
        }
    }
    if ((v2 || b.presum) && b.n_dy > 1) b.have_g = true;
    if (b.have_g && b.do_dx && !b.q_done) {
        SumParams sp;
        sp.n = b.n_dy;
        for (int i = 0; i < b.n_dy; ++i) sp.src[i] = b.dy_all[i];
        sp.nvec = d->M * d->N / ET<T>::VEC;
        int64_t blocks = mtl_ceil_div(sp.nvec, 256);
        if (blocks > 4096) blocks = 4096;
        if (blocks > 0) {
            MtlProfScope prof(PK_SUM, (double)sizeof(T) * d->M * d->N * (b.n_dy + 1), b.s);
            hipLaunchKernelGGL(k_sum<T>, dim3((unsigned)blocks), dim3(256), 0, b.s, sp, b.Gm);
        }
    }
    const void* dy_shared = b.dy[0];
    if (v2 && b.n_dy > 0) dy_shared = b.have_g ? (const void*)b.Gm : b.dy_all[0];
    for (int o = 0; o < sg.n; ++o) b.dyo[o] = (o == 0) ? dy_shared : b.dy[o];
}

// T = 0 layers: Q, the masked rank part and dY W in ONE wave-streaming pass over dY (stream.h); false: not eligible
template <typename T>
static bool bwd_one_pass(Bwd<T>& b) {
    const mtlora_linear_desc* d = b.d;
    const Segs& sg = b.sg;
    if (!(d->T == 0 && d->mode == 0 && b.do_dx && b.dx && b.dyo[0] && sg.R > 0)) return false;
    SpLinParams q = {};
    q.act = b.dyo[0];
    q.w = b.Wt;
    q.proj = b.pk + b.L.bt_proj;
    q.expand = b.pk + b.L.at_frag;
    q.out = b.dx;
    q.pout = b.Qm;
    q.ld_out = d->K;
    q.ldp = sg.R;
    q.M = d->M;
    q.n_cols = (int)d->K;
    q.R = sg.R;
    q.mask_act = 0;
    q.mask_lr = 1;
    q.drop = b.dc;
    const double b8d = fused_bytes(d, (int)sizeof(T)), fl = fused_flops(d, sg);
    // narrow input: the accumulator-resident form
    SpAresPlan pl;
    if (!b.gate_s && sp_ares_plan<T>(b.tu, q, (int)d->N, pl)) {
        launch_sp_ares<T>(q, pl, b.s, PK_NT_BWD_DX, b8d, b8d, fl);
        return true;
    }
    // wide input, short reduction (the Mlp's fc2: dX has 4 C columns, the reduction C <= 192): the activation-resident form,
    // with the GELU' gate of the fused Mlp in its epilogue
    SpXresPlan px;
    q.gate = b.gate_s;
    if (sp_xres_plan<T>(b.tu, q, (int)d->N, px)) {
        launch_sp_xres<T>(q, px, false, b.s, PK_NT_BWD_DX, b8d + (b.gate_s ? (double)sizeof(T) * d->M * d->K : 0.0), b8d, fl, b.gate_s != nullptr);
        return true;
    }
    return false;
}

// Q[:, seg_o] = alpha_o * dY_o B_o   (zero where the output got no gradient)
template <typename T>
static void bwd_q(Bwd<T>& b) {
    const mtlora_linear_desc* d = b.d;
    const Segs& sg = b.sg;
    if (!(sg.R > 0 && b.do_dx && !b.q_done)) return;
    bool any_missing = false;
    ProjSrc src[MAXO];
    int n_src = 0;
    for (int o = 0; o < sg.n; ++o) {
        if (sg.rp[o] == 0) continue;
        if (!b.dyo[o]) {
            any_missing = true;
            continue;
        }
        src[n_src++] = ProjSrc{b.dyo[o], sg.off[o], sg.off[o] + sg.rp[o], 0};
    }
    if (any_missing && !b.hid_q) mtl_zero_async(b.Qm, (size_t)(d->M * sg.R * sizeof(T)), b.s);  // (hid_q: the task columns are given)
    if (n_src > 0) {
        ProjJob<T> j = {};
        j.wproj = b.pk + b.L.bt_proj;
        j.wcat = b.bt_cat;
        j.alpha = b.alpha;
        j.out = b.Qm;
        j.M = d->M;
        j.K = (int)d->N;
        j.kind = PK_NT_BWD_Q;
        j.flops = 2.0 * d->M * d->N * rank_sum(sg, b.dyo);
        launch_proj<T>(b.tu, sg, b.dc, b.s, src, n_src, j);
    }
}

// dX = G W + keep .* (Q_s A_s [+ sum_t Q_t A_t]),  dX_t = Q_t A_t
template <typename T>
static void bwd_dx(Bwd<T>& b) {
    const mtlora_linear_desc* d = b.d;
    const Segs& sg = b.sg;
    const Tune& tu = b.tu;
    hipStream_t s = b.s;
    void* const* dx_t = b.dx_t;
    const void* const* gate_t = b.gate_t;
    if (!b.do_dx) return;
    NtParams m = {};
    RankOutParams rank_out = {};
    int rank_out_rp = 8;
    bool rank_out_gated = false;
    if (b.presum && b.have_g) {
        m.n_act = 1;
        m.act[0] = b.Gm;
    } else {
        m.n_act = b.n_dy;
        for (int i = 0; i < b.n_dy; ++i) m.act[i] = b.dy_all[i];
    }
    if (b.hid_q && d->hid_ptr) {  // G = dH_s + sum_t dH_t was formed by k_hid_bwd
        m.n_act = 1;
        m.act[0] = d->hid_ptr;
    }
    m.ld_act = d->N;
    m.wgt = b.Wt;
    m.ld_wgt = d->N;
    m.M = d->M;
    m.n_rows = (int)d->K;
    m.K = (b.n_dy > 0 || (b.hid_q && d->hid_ptr)) ? (int)d->N : 0;
    m.L = b.Qm;
    m.ldL = sg.R;
    m.Rm = b.at_cat;
    m.ldR = sg.R;
    m.ld_out = d->K;
    m.drop = b.dc;
    m.n_out = 1;
    NtOut& O = m.out[0];
    O.ptr = b.dx;
    O.use_base = 1;
    O.mask_lr = 1;
    O.gate = b.gate_s;
    if (d->T > 0 && d->has_x_tasks) {
        O.seg_lo = sg.off[0];
        O.seg_hi = sg.off[0] + sg.rp[0];
        // small task ranks: the task outputs are a streaming elementwise kernel of their own (k_rank_out), not tile passes
        if constexpr (sizeof(T) == 2) {
            bool ok = tu.sp != 0 && dx_t != nullptr && d->K % 8 == 0 && d->K / 8 <= 256 && d->M > 0;
            int rpm = 0, gates = 0, outs = 0;
            for (int t = 0; t < d->T; ++t) {
                if (!dx_t || !dx_t[t]) continue;
                ++outs;
                rpm = sg.rp[t + 1] > rpm ? sg.rp[t + 1] : rpm;
                gates += (gate_t && gate_t[t]) ? 1 : 0;
                ok = ok && sg.rp[t + 1] > 0 && !misaligned(dx_t[t]) && !(gate_t && gate_t[t] && misaligned(gate_t[t]));
            }
            for (int t = 0; t < d->T; ++t)
                if (dx_t && dx_t[t]) ok = ok && sg.rp[t + 1] == rpm;  // one register geometry per launch
            ok = ok && outs > 0 && rpm <= 16 && (gates == 0 || gates == outs) && !misaligned(b.Qm) && (sg.R % 8) == 0;
            if (ok) {
                rank_out.Q = b.Qm;
                rank_out.Acat = b.pk + b.L.a_cat;
                rank_out.ldq = sg.R;
                rank_out.M = d->M;
                rank_out.K = (int)d->K;
                for (int t = 0; t < d->T; ++t) {
                    if (!dx_t[t]) continue;
                    const int i = rank_out.n_t++;
                    rank_out.seg[i] = sg.off[t + 1];
                    rank_out.rp[i] = sg.rp[t + 1];
                    rank_out.out[i] = dx_t[t];
                    rank_out.gate[i] = gate_t ? gate_t[t] : nullptr;
                }
                rank_out_rp = rpm <= 8 ? 8 : 16;
                rank_out_gated = gates > 0;
            }
        }
        for (int t = 0; t < d->T && rank_out.n_t == 0; ++t) {
            if (!dx_t || !dx_t[t]) continue;
            NtOut& Ot = m.out[m.n_out++];
            Ot.ptr = dx_t[t];
            Ot.seg_lo = sg.off[t + 1];
            Ot.seg_hi = sg.off[t + 1] + sg.rp[t + 1];
            Ot.use_base = 0;
            Ot.mask_lr = 0;
            Ot.fold = 0;
            Ot.gate = gate_t ? gate_t[t] : nullptr;
        }
    } else {
        O.seg_lo = 0;
        O.seg_hi = sg.used;  // (not R: the Q pass writes segments only, the pad columns of Q hold whatever the scratch held)
    }
    if (b.dx) {
        int n_gate = 0;  // the fused GELU backward reads the pre-activation of every gated output (algorithmic: gelu'(h) needs h)
        for (int o = 0; o < m.n_out; ++o) n_gate += m.out[o].gate ? 1 : 0;
        const int n_xt = rank_out.n_t > 0 ? 0 : (d->has_x_tasks ? d->T : 0);  // task outputs written by THIS launch
        const double b8d = (double)sizeof(T) * d->M * ((double)b.n_dy * d->N + (double)(1 + n_xt) * d->K);
        const double fl = (b.n_dy > 0 ? 2.0 * d->M * d->N * d->K : 0.0) + 2.0 * d->M * d->K * rank_sum(sg, b.dyo);
        const bool plain = sg.R == 0;
        launch_nt<T>(tu, m, s, plain ? PK_NT_PLAIN_DX : PK_NT_BWD_DX, b8d + (double)sizeof(T) * d->M * (double)n_gate * d->K,
                     plain ? 0.0 : b8d, fl);
    }
    if constexpr (sizeof(T) == 2) {
        if (rank_out.n_t > 0) {
            const double ob = (double)sizeof(T) * d->M * (double)rank_out.n_t * d->K;
            mtl_prof_tag("rank_out M%lld K%lld nt%d rp%d gate%d", (long long)d->M, (long long)d->K, rank_out.n_t, rank_out_rp, rank_out_gated ? 1 : 0);
            MtlProfScope prof(PK_NT_BWD_DX, ob * (rank_out_gated ? 2.0 : 1.0), s, ob, 0.0);
            const int nchunk = (int)(d->K / 8), rpb = 256 / nchunk;
            int64_t bx = mtl_ceil_div(d->M, (int64_t)rpb * 4);
            const int64_t cap = (int64_t)num_cu(tu) * 8 / rank_out.n_t > 0 ? (int64_t)num_cu(tu) * 8 / rank_out.n_t : 1;
            if (bx > cap) bx = cap;
            const dim3 g((unsigned)bx, (unsigned)rank_out.n_t);
            if (rank_out_gated && rank_out_rp == 8)
                hipLaunchKernelGGL((k_rank_out<T, true, 8>), g, dim3(256), 0, s, rank_out);
            else if (rank_out_gated)
                hipLaunchKernelGGL((k_rank_out<T, true, 16>), g, dim3(256), 0, s, rank_out);
            else if (rank_out_rp == 8)
                hipLaunchKernelGGL((k_rank_out<T, false, 8>), g, dim3(256), 0, s, rank_out);
            else
                hipLaunchKernelGGL((k_rank_out<T, false, 16>), g, dim3(256), 0, s, rank_out);
        }
    }
}

// one factor-gradient problem  out (out_a x Nb) = A[:, a0 .. a0 + Na)^T B   (B is M x Nb, contiguous rows), stored transposed or not
static void add_tn_problem(TnParams& tp, float*& part, int nsplit, const void* A, int64_t lda, int a0, int Na, const void* B, int Nb, int b_mask,
                           float* out, int out_a, int ldo, int transpose) {
    TnProblem& p = tp.p[tp.n_prob++];
    p.A = A;
    p.lda = lda;
    p.a0 = a0;
    p.Na = Na;
    p.B = B;
    p.ldb = Nb;
    p.b0 = 0;
    p.Nb = Nb;
    p.b_mask = b_mask;
    p.tiles_a = (int)mtl_ceil_div(p.Na, TN_A);
    p.tiles_b = (int)mtl_ceil_div(p.Nb, TN_B);
    p.part = part;
    part += (int64_t)p.tiles_a * p.tiles_b * nsplit * TN_TILE;
    p.out = out;
    p.out_a = out_a;
    p.out_b = Nb;
    p.ldo = ldo;
    p.transpose = transpose;
}
// the same problems as the wave-streaming kernel's table (k_sp_tn, nb 32-column blocks per part); false: a problem does not fit its rules
static bool sp_tn_table(const TnParams& tp, int nb, SpTnParams& q) {
    bool ok = nb != 0 && tp.n_prob > 0;
    for (int i = 0; ok && i < tp.n_prob; ++i) {
        const TnProblem& p = tp.p[i];
        SpTnProb& r = q.p[i];
        ok = ok && p.b0 == 0 && p.Nb == p.ldb && p.Nb % (32 * nb) == 0 && !misaligned(p.A) && !misaligned(p.B) && (p.lda % 8) == 0 &&
             (p.a0 % 8) == 0;
        r.A = p.A;
        r.B = p.B;
        r.lda = p.lda;
        r.ldb = p.ldb;
        r.a0 = p.a0;
        r.Na = p.Na;
        r.Nb = p.Nb;
        r.b_mask = p.b_mask;
        r.tiles_a = (int)mtl_ceil_div(p.Na, 64);
        r.parts = p.Nb / (32 * nb);
        r.pp_lo = q.n_pp;
        r.transpose = p.transpose;
        r.out = p.out;
        r.out_a = p.out_a;
        r.out_b = p.out_b;
        r.ldo = p.ldo;
        q.n_pp += r.tiles_a * r.parts;
    }
    return ok;
}

// dA_o = Q_o^T D(X_o),  dB_o = dY_o^T P_o
template <typename T>
static void bwd_factors(Bwd<T>& b) {
    const mtlora_linear_desc* d = b.d;
    const Segs& sg = b.sg;
    const Tune& tu = b.tu;
    const BwdScratch& S = b.S;
    hipStream_t s = b.s;
    if (sg.R == 0) return;
    TnParams tp = {};
    tp.M = d->M;
    tp.nsplit = S.nsplit;
    tp.rows_per_split = S.rows_per_split;
    tp.drop = b.dc;
    float* pp = b.part;
    for (int o = 0; o < sg.n; ++o) {
        const bool q_given = b.hid_q && o > 0;  // Q[:, seg_o] came from k_hid_bwd (which also returns dB_o): dA_o only
        if (sg.rp[o] == 0 || (!b.dyo[o] && !q_given)) continue;
        float* dAo = (o == 0) ? b.dA_s : (b.dA_t ? b.dA_t[o - 1] : nullptr);
        float* dBo = (o == 0) ? b.dB_s : (b.dB_t ? b.dB_t[o - 1] : nullptr);
        if (!b.dyo[o]) dBo = nullptr;
        // (N x r_o) = dY_o^T P[:, seg_o], evaluated as its transpose P[:, seg_o]^T dY_o
        if (dBo) add_tn_problem(tp, pp, S.nsplit, b.Pm, sg.R, sg.off[o], sg.rp[o], b.dyo[o], (int)d->N, 0, dBo, sg.r[o], sg.r[o], 1);
        // (r_o x K) = Q[:, seg_o]^T . D(X_o)
        const bool own_x = (o > 0 && d->has_x_tasks);
        if (dAo) add_tn_problem(tp, pp, S.nsplit, b.Qm, sg.R, sg.off[o], sg.rp[o], own_x ? b.x_t[o - 1] : b.x, (int)d->K, own_x ? 0 : 1, dAo, sg.r[o], (int)d->K, 0);
    }
    int max_tiles = 0;
    double fl = 0.0;
    for (int i = 0; i < tp.n_prob; ++i) {
        max_tiles = std::max(max_tiles, tp.p[i].tiles_a * tp.p[i].tiles_b);
        fl += 2.0 * d->M * (double)tp.p[i].out_a * tp.p[i].out_b;
    }
    const double xb = (double)sizeof(T) * d->M * (double)(1 + (d->has_x_tasks ? d->T : 0)) * d->K;
    if constexpr (sizeof(T) == 2) {
        const int nb = (tu.sp != 0 && tu.tn != 0) ? sp_tn_nb(d) : 0;
        SpTnParams q = {};
        bool ok = sp_tn_table(tp, nb, q);
        if (ok) {
            const int mode = tu.tn;
            q.n_prob = tp.n_prob;
            q.G = sp_tn_groups(tu, q.n_pp, d->M);
            ok = q.n_pp <= SP_TN_WGS && q.G < 65536 && (mode == 2 || (mode == 1 && mtl_ceil_div(d->M, 32) >= (int64_t)8 * q.G * SP_WAVES));
            if (ok) {
                SpTnParams probe = q;
                ok = sp_tn_map(probe) != 0;
                q.G = probe.G;
            }
        }
        if (ok) {
            q.M = d->M;
            q.part = b.part;
            q.drop = b.dc;
            char tag[96];
            snprintf(tag, sizeof(tag), "M%lld K%lld N%lld T%d", (long long)d->M, (long long)d->K, (long long)d->N, d->T);
            launch_sp_tn<T>(q, nb, s, xb, fl, tag);
            return;
        }
    }
    if (tp.n_prob > 0 && d->M > 0) {
        {
            mtl_prof_tag("M%lld K%lld N%lld T%d np%d ns%d tiles%d", (long long)d->M, (long long)d->K, (long long)d->N, d->T, tp.n_prob,
                         S.nsplit, max_tiles);
            MtlProfScope prof(PK_TN, xb, s, xb, fl);
            hipLaunchKernelGGL(k_tn<T>, dim3((unsigned)S.nsplit, (unsigned)max_tiles, (unsigned)tp.n_prob),
                               dim3(256), 0, s, tp);
        }
        MtlProfScope prof(PK_REDUCE, 0.0, s);
        hipLaunchKernelGGL(k_tn_reduce<>, dim3(TN_TILE / 1024, (unsigned)max_tiles, (unsigned)tp.n_prob), dim3(256 * TN_RG), 0, s, tp);
    }
}

template <typename T>
static int bwd_impl(const mtlora_linear_desc* d, const void* x, const void* const* x_t, const void* Wt,
                    const void* dy_s, const void* const* dy_t, const void* ctx, void* dx, void* const* dx_t,
                    float* dA_s, float* dB_s, float* const* dA_t, float* const* dB_t, void* scratch, hipStream_t s,
                    const void* gate_s = nullptr, const void* const* gate_t = nullptr) {
    Bwd<T> b = {};
    b.d = d;
    b.sg = make_segs(d);
    b.tu = make_tune(d);
    b.L = ctx_layout(d, b.sg);
    b.S = bwd_scratch(d, b.sg);
    b.s = s;
    b.dc = mtl_make_dropout(d->dropout_p, d->seed, d->seed_offset);
    const unsigned char* c = reinterpret_cast<const unsigned char*>(ctx);
    unsigned char* sc = reinterpret_cast<unsigned char*>(scratch);
    b.pk = d->packed ? reinterpret_cast<const unsigned char*>(d->packed) : c;
    b.at_cat = reinterpret_cast<const T*>(b.pk + b.L.at_cat), b.bt_cat = reinterpret_cast<const T*>(b.pk + b.L.bt_cat);
    b.alpha = reinterpret_cast<const float*>(b.pk + b.L.alpha);
    b.Pm = reinterpret_cast<const T*>(c + b.L.p);
    b.Qm = reinterpret_cast<T*>(sc + b.S.q), b.Gm = reinterpret_cast<T*>(sc + b.S.g);
    b.part = reinterpret_cast<float*>(sc + b.S.part);
    b.x = x, b.x_t = x_t, b.Wt = Wt;
    b.dx = dx, b.dx_t = dx_t;
    b.dA_s = dA_s, b.dB_s = dB_s, b.dA_t = dA_t, b.dB_t = dB_t;
    b.gate_s = gate_s, b.gate_t = gate_t;
    b.do_dx = d->bwd_phase != 2;
    b.hid_q = (d->hid & MTLORA_HID_Q_GIVEN) != 0;
    b.dy[0] = dy_s;
    for (int t = 0; t < d->T; ++t) b.dy[t + 1] = dy_t ? dy_t[t] : nullptr;
    for (int o = 0; o < b.sg.n; ++o)
        if (b.dy[o]) b.dy_all[b.n_dy++] = b.dy[o];

    bwd_grad_sum(b);
    if (!bwd_one_pass(b)) {
        bwd_q(b);
        bwd_dx(b);
    }
    if (d->bwd_phase != 1) bwd_factors(b);
    return MTLORA_OK;
}

// ---- Mlp with implicit task hidden tensors (hid.hip): shape rules, launch geometry, the two launches
struct HidPlan {
    int tg, rr, nthr, nw, groups, n_wg;
};
static int hid_check(const mtlora_linear_desc* d1, const mtlora_linear_desc* d2) {
    int st = check_desc(d1);
    if (st != MTLORA_OK) return st;
    st = check_desc(d2);
    if (st != MTLORA_OK) return st;
    if (!mtl_dtype_in(d1->dtype, MTL_DT_16) || d1->dtype != d2->dtype) return MTLORA_ERR_UNSUPPORTED;
    if (d1->M != d2->M || d1->N != d2->K || d1->T != d2->T || d1->T < 1) return MTLORA_ERR_UNSUPPORTED;
    if (d1->mode != 0 || d2->mode != 0 || !d1->has_x_tasks || !d2->has_x_tasks) return MTLORA_ERR_UNSUPPORTED;
    if (d1->N % 128 != 0 || d1->M <= 0) return MTLORA_ERR_UNSUPPORTED;
    int rmax = 0;
    for (int t = 0; t < d1->T; ++t) {
        if (d1->r_t[t] < 1 || d1->r_t[t] > 8 || d2->r_t[t] < 1 || d2->r_t[t] > 8) return MTLORA_ERR_UNSUPPORTED;
        rmax = std::max(rmax, std::max(d1->r_t[t], d2->r_t[t]));
    }
    // the VALU forms hold a whole row per workgroup (two columns per thread: <= 2048 columns); the MFMA forms take any number of chunks
    const bool chunked = d1->sel_stream != 1 && rmax <= 4;  // (N % 128 == 0: a chunk width exists in both directions)
    if (d1->N > 2048 && !chunked) return MTLORA_ERR_UNSUPPORTED;
    return MTLORA_OK;
}
static HidPlan hid_plan(const mtlora_linear_desc* d1, const mtlora_linear_desc* d2) {
    HidPlan pl;
    int rmax = 0;
    for (int t = 0; t < d1->T; ++t) rmax = std::max(rmax, std::max(d1->r_t[t], d2->r_t[t]));
    pl.rr = rmax <= 4 ? 4 : 8;
    pl.nthr = (int)(d1->N / 2);
    pl.nw = pl.nthr / 64;
    // register budget: the backward kernel holds 8 * TG * RR factor + accumulator registers per lane: TG * RR = 16 needs the 256-register
    // budget of <= 512-thread workgroups (2 waves per SIMD), 8 fits the 168 registers of 768 threads, 1024 threads are capped at 128
    const int cap = pl.nthr <= 512 ? 16 : 8;
    pl.tg = std::max(1, cap / pl.rr);
    if (pl.nthr > 768 && pl.rr == 8) pl.tg = 1;
    pl.groups = (d1->T + pl.tg - 1) / pl.tg;
    const Tune tu = make_tune(d1);
    const int wg_per_cu = std::max(1, (8 + pl.nw - 1) / pl.nw);
    const int64_t nblk = (d1->M + HID_RB - 1) / HID_RB;
    pl.n_wg = (int)std::min<int64_t>(nblk, (int64_t)num_cu(tu) * wg_per_cu);
    return pl;
}
static int64_t hid_part_bytes(const mtlora_linear_desc* d1, const HidPlan& pl) {
    // (either form of the backward kernel: VALU n_wg x tg tasks, MFMA <= one workgroup per CU x HID_TG tasks)
    const Tune tu = make_tune(d1);
    const int64_t slots = std::max<int64_t>((int64_t)pl.n_wg * pl.tg, (int64_t)num_cu(tu) * HID_TG);
    return slots * 2 * pl.rr * d1->N * 4 + 256;
}

static void hid_launch_valu(int dtype, bool bwd, const HidPlan& pl, const HidParams& q, hipStream_t s) {
    HidLaunch L = {};
    L.kind = bwd ? 1 : 0;
    L.dtype = dtype;
    L.tg = pl.tg;
    L.rr = pl.rr;
    L.nthr = pl.nthr;
    L.n_wg = pl.n_wg;
    mtli_hid_launch(&L, &q, s);
}
// MFMA forms (hid.hip, k_hid_fwd_d / k_hid_bwd_d): rank <= 4, hidden width a multiple of 384 or 256 columns (one chunk per grid y)
struct HidDPlan {
    bool on;
    int hc, n_chunk, n_wg, groups;
    size_t lds_f, lds_b;
    int64_t rowpart_bytes;
};
static HidDPlan hid_d_plan(const mtlora_linear_desc* d1, const HidPlan& pl, bool bwd) {
    HidDPlan dp = {};
    const Tune tu = make_tune(d1);
    const int H = (int)d1->N;
    dp.hc = hid_d_chunk(H, bwd);
    dp.on = tu.sp != 0 && pl.rr == 4 && dp.hc != 0;
    if (!dp.on) return dp;
    dp.n_chunk = H / dp.hc;
    dp.groups = (d1->T + HID_TG - 1) / HID_TG;
    dp.lds_f = hid_d_lds_bytes(dp.hc, false);
    dp.lds_b = hid_d_lds_bytes(dp.hc, true);
    const int64_t nblk = (d1->M + 31) / 32;
    // workgroups per CU: as many as fit by LDS and by 12 waves of 168 registers
    const int per_cu = std::max(1, std::min((int)((size_t)(150 * 1024) / (bwd ? dp.lds_b : dp.lds_f)), (bwd ? 12 : 16) / (dp.hc / 32)));
    dp.n_wg = (int)std::min<int64_t>(nblk, std::max<int64_t>(1, (int64_t)num_cu(tu) * per_cu / dp.n_chunk));
    dp.rowpart_bytes = (int64_t)dp.n_chunk * d1->M * 16 * 4 + 256;
    return dp;
}
static void hid_launch_d(int dtype, bool bwd, const HidDPlan& dp, const HidParams& q, hipStream_t s) {
    HidLaunch L = {};
    L.kind = bwd ? 3 : 2;
    L.dtype = dtype;
    L.rr = 4;
    L.hc = dp.hc;
    L.n_chunk = dp.n_chunk;
    L.n_wg = dp.n_wg;
    L.nthr = dp.hc * 2;
    L.lds = bwd ? dp.lds_b : dp.lds_f;
    mtli_hid_launch(&L, &q, s);
}
static int64_t hid_fwd_scratch_bytes(const mtlora_linear_desc* d1, const mtlora_linear_desc* d2) {
    const HidPlan pl = hid_plan(d1, d2);
    const HidDPlan dp = hid_d_plan(d1, pl, false);
    return dp.on ? dp.rowpart_bytes : 256;
}
static int64_t hid_bwd_part_bytes(const mtlora_linear_desc* d1, const mtlora_linear_desc* d2) {
    const HidPlan pl = hid_plan(d1, d2);
    const HidDPlan dp = hid_d_plan(d1, pl, true);
    if (!dp.on) return hid_part_bytes(d1, pl);
    // [chunk][n_wg][nt <= 4][2][4][hc] factor-gradient partials, then the row-sum partials
    return (int64_t)dp.n_chunk * dp.n_wg * HID_TG * 2 * 4 * dp.hc * 4 + 256 + dp.rowpart_bytes;
}

template <typename T>
static int hid_proj_impl(const mtlora_linear_desc* d1, const mtlora_linear_desc* d2, const void* h_base, const void* ctx1, void* ctx2,
                         void* scratch, hipStream_t s) {
    const Segs s1 = make_segs(d1), s2 = make_segs(d2);
    const CtxLayout L1 = ctx_layout(d1, s1), L2 = ctx_layout(d2, s2);
    const unsigned char* c1 = reinterpret_cast<const unsigned char*>(ctx1);
    unsigned char* c2 = reinterpret_cast<unsigned char*>(ctx2);
    const unsigned char* pk1 = d1->packed ? reinterpret_cast<const unsigned char*>(d1->packed) : c1;
    const unsigned char* pk2 = reinterpret_cast<const unsigned char*>(d2->packed);
    const HidPlan pl = hid_plan(d1, d2);
    const HidDPlan dp = hid_d_plan(d1, pl, false);
    const int H = (int)d1->N;
    const int tg = dp.on ? HID_TG : pl.tg;
    const int groups = (d1->T + tg - 1) / tg;
    for (int gI = 0; gI < groups; ++gI) {
        HidParams q = {};
        q.hbase = h_base;
        q.p1 = c1 + L1.p;
        q.p2 = c2 + L2.p;
        q.b1t = pk1 + L1.bt_cat;
        q.a2 = pk2 + L2.a_cat;
        q.alpha1 = reinterpret_cast<const float*>(pk1 + L1.alpha);
        q.alpha2 = reinterpret_cast<const float*>(pk2 + L2.alpha);
        q.rowpart = reinterpret_cast<float*>(scratch);
        q.M = d1->M;
        q.H = H;
        q.ldp1 = s1.R;
        q.ldp2 = s2.R;
        q.nt = std::min(tg, d1->T - gI * tg);
        for (int i = 0; i < HID_TG; ++i) {  // (slots past nt: valid offsets, never stored -- hid.hip)
            const int t = gI * tg + (i < q.nt ? i : 0);
            q.off1[i] = s1.off[1 + t];
            q.off2[i] = s2.off[1 + t];
        }
        const double hb = (double)sizeof(T) * d1->M * H;
        mtl_prof_tag("hid_fwd%s M%lld H%d T%d nt%d rr%d", dp.on ? "_d" : "", (long long)d1->M, H, d1->T, q.nt, pl.rr);
        {
            MtlProfScope prof(PK_NT_FWD_P, hb, s, (double)sizeof(T) * d1->M * (double)q.nt * H, 0.0);
            if (dp.on)
                hid_launch_d(d1->dtype, false, dp, q, s);
            else
                hid_launch_valu(d1->dtype, false, pl, q, s);
        }
        if (dp.on) {  // (its own profiler record: one record per dispatch, tools/pmc_traffic.py zips the two lists)
            mtl_prof_tag("hid_rows_finish M%lld chunks%d", (long long)d1->M, dp.n_chunk);
            MtlProfScope prof(PK_REDUCE, 0.0, s);
            mtli_hid_rows_finish(d1->dtype, q.rowpart, dp.n_chunk, d1->M, q.nt, q.alpha2, q.off2, q.p2, q.ldp2, s);
        }
    }
    return MTLORA_OK;
}

template <typename T>
static int hid_bwd_impl(const mtlora_linear_desc* d1, const mtlora_linear_desc* d2, const void* h_base, const void* dh_s, const void* ctx1,
                        const void* ctx2, const void* scratch2, void* scratch1, void* g, float* const* dB1_t, float* const* dA2_t, void* part,
                        hipStream_t s) {
    const Segs s1 = make_segs(d1), s2 = make_segs(d2);
    const CtxLayout L1 = ctx_layout(d1, s1), L2 = ctx_layout(d2, s2);
    const BwdScratch S1 = bwd_scratch(d1, s1), S2 = bwd_scratch(d2, s2);
    const unsigned char* c1 = reinterpret_cast<const unsigned char*>(ctx1);
    const unsigned char* c2 = reinterpret_cast<const unsigned char*>(ctx2);
    const unsigned char* pk1 = d1->packed ? reinterpret_cast<const unsigned char*>(d1->packed) : c1;
    const unsigned char* pk2 = d2->packed ? reinterpret_cast<const unsigned char*>(d2->packed) : c2;
    const HidPlan pl = hid_plan(d1, d2);
    const HidDPlan dp = hid_d_plan(d1, pl, true);
    const int H = (int)d1->N;
    const int tg = dp.on ? HID_TG : pl.tg;
    const int groups = (d1->T + tg - 1) / tg;
    const int rr = pl.rr;
    const int64_t fact_bytes = dp.on ? (int64_t)dp.n_chunk * dp.n_wg * HID_TG * 2 * 4 * dp.hc * 4 + 256 : 0;
    for (int gI = 0; gI < groups; ++gI) {
        HidParams q = {};
        q.hbase = h_base;
        q.p1 = c1 + L1.p;
        q.q2 = reinterpret_cast<const unsigned char*>(scratch2) + S2.q;
        q.q1 = reinterpret_cast<unsigned char*>(scratch1) + S1.q;
        q.gsrc = gI == 0 ? dh_s : g;
        q.g = g;
        q.b1t = pk1 + L1.bt_cat;
        q.a2 = pk2 + L2.a_cat;
        q.alpha1 = reinterpret_cast<const float*>(pk1 + L1.alpha);
        q.alpha2 = reinterpret_cast<const float*>(pk2 + L2.alpha);
        q.part = reinterpret_cast<float*>(part);
        q.rowpart = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(part) + fact_bytes);
        q.M = d1->M;
        q.H = H;
        q.ldp1 = s1.R;
        q.ldq1 = s1.R;
        q.ldq2 = s2.R;
        q.nt = std::min(tg, d1->T - gI * tg);
        for (int i = 0; i < HID_TG; ++i) {  // (slots past nt: valid offsets, never stored -- hid.hip)
            const int t = gI * tg + (i < q.nt ? i : 0);
            q.off1[i] = s1.off[1 + t];
            q.off2[i] = s2.off[1 + t];
        }
        HidRedParams r = {};
        for (int i = 0; i < q.nt; ++i) {
            const int t = gI * tg + i;
            r.r[i] = 0;
            r.dB1[i] = dB1_t ? dB1_t[t] : nullptr;
            r.dA2[i] = dA2_t ? dA2_t[t] : nullptr;
        }
        {
            mtl_prof_tag("hid_bwd%s M%lld H%d T%d nt%d rr%d", dp.on ? "_d" : "", (long long)d1->M, H, d1->T, q.nt, rr);
            const double hb = (double)sizeof(T) * d1->M * H;
            MtlProfScope prof(PK_NT_BWD_DX, 3.0 * hb, s, (double)sizeof(T) * d1->M * (double)q.nt * H, 0.0);
            if (dp.on)
                hid_launch_d(d1->dtype, true, dp, q, s);
            else
                hid_launch_valu(d1->dtype, true, pl, q, s);
        }
        if (dp.on) {
            mtl_prof_tag("hid_rows_finish M%lld chunks%d", (long long)d1->M, dp.n_chunk);
            MtlProfScope prof(PK_REDUCE, 0.0, s);
            mtli_hid_rows_finish(d1->dtype, q.rowpart, dp.n_chunk, d1->M, q.nt, q.alpha1, q.off1, q.q1, q.ldq1, s);
        }
        // dB1_t (fc1's N x r_t, un-padded rank d1->r_t) and dA2_t (fc2's r_t x K) share one reduce: per kind the un-padded rank differs
        // only if the two layers were built with different task ranks -- reduce them separately then
        r.part = q.part;
        r.n_wg = dp.on ? dp.n_wg : pl.n_wg;
        r.nt = q.nt;
        r.RR = rr;
        r.H = H;
        r.chunk_cols = dp.on ? dp.hc : H;
        const int64_t per = (int64_t)q.nt * 2 * rr * H;
        bool same = true;
        for (int i = 0; i < q.nt; ++i) same = same && d1->r_t[gI * tg + i] == d2->r_t[gI * tg + i];
        MtlProfScope prof(PK_REDUCE, 0.0, s);
        if (same) {
            for (int i = 0; i < q.nt; ++i) r.r[i] = d1->r_t[gI * tg + i];
            mtli_hid_reduce(&r, per, s);
        } else {
            HidRedParams rb = r, ra = r;
            for (int i = 0; i < q.nt; ++i) {
                rb.r[i] = d1->r_t[gI * tg + i];
                rb.dA2[i] = nullptr;
                ra.r[i] = d2->r_t[gI * tg + i];
                ra.dB1[i] = nullptr;
            }
            mtli_hid_reduce(&rb, per, s);
            MtlProfScope prof2(PK_REDUCE, 0.0, s);
            mtli_hid_reduce(&ra, per, s);
        }
    }
    return MTLORA_OK;
}

}  // namespace

extern "C" {

int mtlora_mlp_hid_supported(const mtlora_linear_desc* d1, const mtlora_linear_desc* d2) {
    return (d1 && d2 && hid_check(d1, d2) == MTLORA_OK) ? 1 : 0;
}

int64_t mtlora_mlp_hid_fwd_scratch_bytes(const mtlora_linear_desc* d1, const mtlora_linear_desc* d2) {
    if (!d1 || !d2 || hid_check(d1, d2) != MTLORA_OK) return -1;
    return hid_fwd_scratch_bytes(d1, d2);
}

int64_t mtlora_mlp_hid_bwd_scratch_bytes(const mtlora_linear_desc* d1, const mtlora_linear_desc* d2) {
    if (!d1 || !d2 || hid_check(d1, d2) != MTLORA_OK) return -1;
    return hid_bwd_part_bytes(d1, d2);
}

int mtlora_mlp_hid_proj(const mtlora_linear_desc* d1, const mtlora_linear_desc* d2, const void* h_base, const void* ctx1, void* ctx2,
                        void* scratch, int64_t scratch_bytes, void* stream) {
    if (!d1 || !d2) return MTLORA_ERR_NULL;
    const int st = hid_check(d1, d2);
    if (st != MTLORA_OK) return st;
    if (!h_base || !ctx1 || !ctx2 || !d2->packed || !scratch) return MTLORA_ERR_NULL;
    if (misaligned(h_base) || misaligned(ctx1) || misaligned(ctx2) || misaligned(d2->packed) || misaligned(d1->packed) || misaligned(scratch))
        return MTLORA_ERR_ALIGN;
    if (scratch_bytes < hid_fwd_scratch_bytes(d1, d2)) return MTLORA_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int r = mtl_dispatch_dtype16(d1->dtype, [&](auto t) { return hid_proj_impl<typename decltype(t)::type>(d1, d2, h_base, ctx1, ctx2, scratch, s); });
    if (r != MTLORA_OK) return r;
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

int mtlora_mlp_hid_bwd(const mtlora_linear_desc* d1, const mtlora_linear_desc* d2, const void* h_base, const void* dh_s, const void* ctx1,
                       const void* ctx2, const void* scratch2, void* scratch1, void* g, float* const* dB1_t, float* const* dA2_t, void* part,
                       int64_t part_bytes, void* stream) {
    if (!d1 || !d2) return MTLORA_ERR_NULL;
    const int st = hid_check(d1, d2);
    if (st != MTLORA_OK) return st;
    if (!h_base || !ctx1 || !ctx2 || !scratch1 || !scratch2 || !g || !part) return MTLORA_ERR_NULL;
    if (misaligned(h_base) || misaligned(dh_s) || misaligned(ctx1) || misaligned(ctx2) || misaligned(scratch1) || misaligned(scratch2) ||
        misaligned(g) || misaligned(part))
        return MTLORA_ERR_ALIGN;
    if (part_bytes < hid_bwd_part_bytes(d1, d2)) return MTLORA_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int r = mtl_dispatch_dtype16(d1->dtype, [&](auto t) {
        return hid_bwd_impl<typename decltype(t)::type>(d1, d2, h_base, dh_s, ctx1, ctx2, scratch2, scratch1, g, dB1_t, dA2_t, part, s);
    });
    if (r != MTLORA_OK) return r;
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

int64_t mtlora_linear_ctx_bytes(const mtlora_linear_desc* d) {
    if (check_desc(d) != MTLORA_OK) return -1;
    const Segs sg = make_segs(d);
    return ctx_layout(d, sg).total + 256;
}

int64_t mtlora_linear_bwd_scratch_bytes(const mtlora_linear_desc* d) {
    if (check_desc(d) != MTLORA_OK) return -1;
    const Segs sg = make_segs(d);
    return bwd_scratch(d, sg).total + 256;
}

int64_t mtlora_linear_packed_bytes(const mtlora_linear_desc* d) {
    if (check_desc(d) != MTLORA_OK) return -1;
    const Segs sg = make_segs(d);
    return ctx_layout(d, sg).pack_total + 256;
}

static int pack_check(const mtlora_linear_desc* d, const float* A_s, const float* B_s, const float* const* A_t, const float* const* B_t,
                      const void* packed, int64_t packed_bytes) {
    const int st = check_desc(d);
    if (st != MTLORA_OK) return st;
    if (mtl_any_null({packed})) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({packed})) return MTLORA_ERR_ALIGN;
    if (d->r_s > 0 && mtl_any_null({A_s, B_s})) return MTLORA_ERR_NULL;
    if (d->T > 0 && mtl_any_null({}, d->T, {mtl_arr(A_t), mtl_arr(B_t)})) return MTLORA_ERR_NULL;
    const Segs sg = make_segs(d);
    if (packed_bytes < ctx_layout(d, sg).pack_total) return MTLORA_ERR_WORKSPACE;
    return MTLORA_OK;
}

// the device-scale argument of the *_dev entries: the array is required and has one slot per segment (shared, then the tasks); a
// null slot means "constant, the descriptor's value"; a scale is one aligned float
static int scale_dev_check(const mtlora_linear_desc* d, const float* const* scale_dev, int n_scale) {
    if (mtl_any_null({scale_dev})) return MTLORA_ERR_NULL;
    if (n_scale != d->T + 1) return MTLORA_ERR_SHAPE;
    if (mtl_any_misaligned({}, n_scale, {mtl_arr(scale_dev)}, 4)) return MTLORA_ERR_ALIGN;
    return MTLORA_OK;
}

static int linear_pack(const mtlora_linear_desc* d, const float* A_s, const float* B_s, const float* const* A_t, const float* const* B_t,
                       const float* const* scale_dev, void* packed, int64_t packed_bytes, void* stream) {
    const Segs sg = make_segs(d);
    if (sg.R == 0) return MTLORA_OK;
    const CtxLayout L = ctx_layout(d, sg);
    unsigned char* pk = reinterpret_cast<unsigned char*>(packed);
    hipStream_t s = (hipStream_t)stream;
    mtl_dispatch_dtype(d->dtype, [&](auto t) { launch_pack<typename decltype(t)::type>(d, sg, L, pk, A_s, B_s, A_t, B_t, s, scale_dev); });
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

int mtlora_linear_pack(const mtlora_linear_desc* d, const float* A_s, const float* B_s, const float* const* A_t,
                       const float* const* B_t, void* packed, int64_t packed_bytes, void* stream) {
    const int st = pack_check(d, A_s, B_s, A_t, B_t, packed, packed_bytes);
    if (st != MTLORA_OK) return st;
    return linear_pack(d, A_s, B_s, A_t, B_t, nullptr, packed, packed_bytes, stream);
}

int mtlora_linear_pack_dev(const mtlora_linear_desc* d, const float* A_s, const float* B_s, const float* const* A_t,
                           const float* const* B_t, const float* const* scale_dev, int n_scale, void* packed, int64_t packed_bytes,
                           void* stream) {
    int st = pack_check(d, A_s, B_s, A_t, B_t, packed, packed_bytes);
    if (st == MTLORA_OK) st = scale_dev_check(d, scale_dev, n_scale);
    if (st != MTLORA_OK) return st;
    return linear_pack(d, A_s, B_s, A_t, B_t, scale_dev, packed, packed_bytes, stream);
}

int64_t mtlora_linear_pack_entry_bytes(void) { return (int64_t)sizeof(PackEntry); }

static int linear_pack_entry(const mtlora_linear_desc* d, const float* A_s, const float* B_s, const float* const* A_t,
                             const float* const* B_t, const float* const* scale_dev, void* packed, void* entry_host) {
    if (!entry_host) return MTLORA_ERR_NULL;
    const Segs sg = make_segs(d);
    if (sg.R == 0) return MTLORA_ERR_SHAPE;  // nothing to pack: such a layer does not belong in a table
    const CtxLayout L = ctx_layout(d, sg);
    PackEntry e;
    memset(&e, 0, sizeof(e));
    e.pp = make_pack_params(d, sg, A_s, B_s, A_t, B_t, scale_dev);
    e.dst = reinterpret_cast<unsigned char*>(packed);
    const int64_t off[9] = {L.a_cat, L.b_cat, L.at_cat, L.bt_cat, L.alpha, L.a_proj, L.bt_proj, L.b_frag, L.at_frag};
    for (int i = 0; i < 9; ++i) e.off[i] = off[i];
    memcpy(entry_host, &e, sizeof(e));
    return MTLORA_OK;
}

int mtlora_linear_pack_entry(const mtlora_linear_desc* d, const float* A_s, const float* B_s, const float* const* A_t,
                             const float* const* B_t, void* packed, int64_t packed_bytes, void* entry_host) {
    const int st = pack_check(d, A_s, B_s, A_t, B_t, packed, packed_bytes);
    if (st != MTLORA_OK) return st;
    return linear_pack_entry(d, A_s, B_s, A_t, B_t, nullptr, packed, entry_host);
}

int mtlora_linear_pack_entry_dev(const mtlora_linear_desc* d, const float* A_s, const float* B_s, const float* const* A_t,
                                 const float* const* B_t, const float* const* scale_dev, int n_scale, void* packed,
                                 int64_t packed_bytes, void* entry_host) {
    int st = pack_check(d, A_s, B_s, A_t, B_t, packed, packed_bytes);
    if (st == MTLORA_OK) st = scale_dev_check(d, scale_dev, n_scale);
    if (st != MTLORA_OK) return st;
    return linear_pack_entry(d, A_s, B_s, A_t, B_t, scale_dev, packed, entry_host);
}

int64_t mtlora_linear_scale_grad_scratch_bytes(void) { return (int64_t)(MAXO * SG_BLOCKS * sizeof(float)); }

int mtlora_linear_scale_grad(const mtlora_linear_desc* d, const float* const* dB, const float* const* B, const float* const* scale_dev,
                             int n_scale, float* d_scale, void* scratch, int64_t scratch_bytes, void* stream) {
    int st = check_desc(d);
    if (st != MTLORA_OK) return st;
    if (mtl_any_null({dB, B, d_scale, scratch})) return MTLORA_ERR_NULL;
    st = scale_dev_check(d, scale_dev, n_scale);
    if (st != MTLORA_OK) return st;
    if (mtl_any_misaligned({d_scale, scratch}, n_scale, {mtl_arr(dB), mtl_arr(B)}, 4)) return MTLORA_ERR_ALIGN;
    if (scratch_bytes < mtlora_linear_scale_grad_scratch_bytes()) return MTLORA_ERR_WORKSPACE;
    ScaleGradParams P;
    memset(&P, 0, sizeof(P));
    P.nseg = n_scale;
    P.part = reinterpret_cast<float*>(scratch);
    P.d_scale = d_scale;
    bool any = false;
    for (int o = 0; o < n_scale; ++o) {
        const int64_t r = o == 0 ? d->r_s : d->r_t[o - 1];
        if (!dB[o] || !scale_dev[o] || r <= 0) continue;  // nothing to form for this segment
        if (!B[o]) return MTLORA_ERR_NULL;
        P.dB[o] = dB[o];
        P.B[o] = B[o];
        P.scale[o] = scale_dev[o];
        P.n[o] = d->N * r;
        any = true;
    }
    if (!any) return MTLORA_OK;
    hipStream_t s = (hipStream_t)stream;
    MtlProfScope prof(PK_REDUCE, 0.0, s);
    hipLaunchKernelGGL(k_scale_grad_part, dim3(SG_BLOCKS, (unsigned)n_scale), dim3(256), 0, s, P);
    hipLaunchKernelGGL(k_scale_grad_fin, dim3(1), dim3(64), 0, s, P);
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

int mtlora_linear_pack_table(const void* table_dev, int n_entries, int dtype, void* stream) {
    if (!mtl_dtype_in(dtype, MTL_DT_ALL)) return MTLORA_ERR_DTYPE;
    if (n_entries < 0 || n_entries > 65535) return MTLORA_ERR_SHAPE;
    if (n_entries == 0) return MTLORA_OK;
    if (mtl_any_null({table_dev})) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({table_dev}, 0, {}, 8)) return MTLORA_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    const PackEntry* tb = reinterpret_cast<const PackEntry*>(table_dev);
    MtlProfScope prof(PK_PACK, 0.0, s);
    const dim3 g(256, (unsigned)n_entries);  // up to 256 workgroups per layer walk its 20 - 800 tiles (the others leave at once)
    mtl_dispatch_dtype(dtype, [&](auto t) { hipLaunchKernelGGL(k_pack_table<typename decltype(t)::type>, g, dim3(256), 0, s, tb); });
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

static int linear_fwd_entry(const mtlora_linear_desc* d, const void* x, const void* const* x_t, const void* W,
                            const float* bias, const float* A_s, const float* B_s, const float* const* A_t,
                            const float* const* B_t, void* y_s, void* const* y_t, void* a_s, void* const* a_t, void* ctx,
                            int64_t ctx_bytes, void* stream) {
    int st = check_desc(d);
    if (st != MTLORA_OK) return st;
    if (!x || !W || !y_s) return MTLORA_ERR_NULL;
    if (d->r_s > 0 && !d->packed && (!A_s || !B_s)) return MTLORA_ERR_NULL;
    if (misaligned(x) || misaligned(W) || misaligned(y_s) || misaligned(bias) || misaligned(d->packed)) return MTLORA_ERR_ALIGN;
    const bool hid_base = (d->hid & MTLORA_HID_FWD_BASE) != 0, hid_p = (d->hid & MTLORA_HID_P_GIVEN) != 0;
    if (hid_base && (!d->hid_ptr || d->T < 1 || !d->has_x_tasks || d->mode != 0)) return MTLORA_ERR_NULL;
    if (hid_base && misaligned(d->hid_ptr)) return MTLORA_ERR_ALIGN;
    if (hid_p && (d->T < 1 || !d->has_x_tasks || d->mode != 0)) return MTLORA_ERR_UNSUPPORTED;
    for (int t = 0; t < d->T; ++t) {
        if (!hid_base && (!y_t || !y_t[t])) return MTLORA_ERR_NULL;  // (HID_FWD_BASE: no task outputs)
        if (!d->packed && (!A_t || !B_t || !A_t[t] || !B_t[t])) return MTLORA_ERR_NULL;
        if (!hid_base && misaligned(y_t[t])) return MTLORA_ERR_ALIGN;
        if (d->has_x_tasks && !hid_p && (!x_t || !x_t[t])) return MTLORA_ERR_NULL;  // (HID_P_GIVEN: x_t is not read)
        if (d->has_x_tasks && !hid_p && misaligned(x_t[t])) return MTLORA_ERR_ALIGN;
    }
    const Segs sg = make_segs(d);
    if (sg.R > 0) {
        if (!ctx) return MTLORA_ERR_NULL;
        if (misaligned(ctx)) return MTLORA_ERR_ALIGN;
        if (ctx_bytes < ctx_layout(d, sg).total) return MTLORA_ERR_WORKSPACE;
    }
    if (d->M == 0) return MTLORA_OK;
    hipStream_t s = (hipStream_t)stream;
    st = mtl_dispatch_dtype(d->dtype, [&](auto t) {
        return fwd_impl<typename decltype(t)::type>(d, x, x_t, W, bias, A_s, B_s, A_t, B_t, y_s, y_t, ctx, s, a_s, a_t);
    });
    if (st != MTLORA_OK) return st;
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

int mtlora_linear_fwd(const mtlora_linear_desc* d, const void* x, const void* const* x_t, const void* W,
                      const float* bias, const float* A_s, const float* B_s, const float* const* A_t,
                      const float* const* B_t, void* y_s, void* const* y_t, void* ctx, int64_t ctx_bytes,
                      void* stream) {
    return linear_fwd_entry(d, x, x_t, W, bias, A_s, B_s, A_t, B_t, y_s, y_t, nullptr, nullptr, ctx, ctx_bytes, stream);
}

int mtlora_linear_fwd_gelu(const mtlora_linear_desc* d, const void* x, const void* const* x_t, const void* W,
                           const float* bias, const float* A_s, const float* B_s, const float* const* A_t,
                           const float* const* B_t, void* y_s, void* const* y_t, void* a_s, void* const* a_t, void* ctx,
                           int64_t ctx_bytes, void* stream) {
    if (!a_s || !d) return MTLORA_ERR_NULL;
    if (misaligned(a_s)) return MTLORA_ERR_ALIGN;
    for (int t = 0; t < d->T && !(d->hid & MTLORA_HID_FWD_BASE); ++t) {  // (HID_FWD_BASE: no task outputs)
        if (!a_t || !a_t[t]) return MTLORA_ERR_NULL;
        if (misaligned(a_t[t])) return MTLORA_ERR_ALIGN;
    }
    return linear_fwd_entry(d, x, x_t, W, bias, A_s, B_s, A_t, B_t, y_s, y_t, a_s, a_t, ctx, ctx_bytes, stream);
}

static int linear_bwd_entry(const mtlora_linear_desc* d, const void* x, const void* const* x_t, const void* Wt,
                            const void* dy_s, const void* const* dy_t, const void* ctx, int64_t ctx_bytes, void* dx,
                            void* const* dx_t, float* dA_s, float* dB_s, float* const* dA_t, float* const* dB_t,
                            void* scratch, int64_t scratch_bytes, const void* gate_s, const void* const* gate_t,
                            void* stream) {
    int st = check_desc(d);
    if (st != MTLORA_OK) return st;
    if (!x || !Wt) return MTLORA_ERR_NULL;
    if (misaligned(x) || misaligned(Wt) || misaligned(dx) || misaligned(dy_s)) return MTLORA_ERR_ALIGN;
    const Segs sg = make_segs(d);
    if (sg.R > 0) {
        if (!ctx || !scratch) return MTLORA_ERR_NULL;
        if (misaligned(ctx) || misaligned(scratch)) return MTLORA_ERR_ALIGN;
        if (ctx_bytes < ctx_layout(d, sg).total) return MTLORA_ERR_WORKSPACE;
        if (scratch_bytes < bwd_scratch(d, sg).total) return MTLORA_ERR_WORKSPACE;
    }
    if ((d->hid & MTLORA_HID_Q_GIVEN) && (d->T < 1 || !d->has_x_tasks || d->mode != 0 || misaligned(d->hid_ptr))) return MTLORA_ERR_UNSUPPORTED;
    for (int t = 0; t < d->T; ++t) {
        // a task's own input is only read for its factor gradient dA_t (an Mlp with implicit task hiddens asks fc2 for none: hid.hip)
        if (d->has_x_tasks && dA_t && dA_t[t] && (!x_t || !x_t[t])) return MTLORA_ERR_NULL;
        if (d->has_x_tasks && x_t && misaligned(x_t[t])) return MTLORA_ERR_ALIGN;
        if (dy_t && misaligned(dy_t[t])) return MTLORA_ERR_ALIGN;
        if (dx_t && misaligned(dx_t[t])) return MTLORA_ERR_ALIGN;
    }
    if (d->M == 0) return MTLORA_OK;
    hipStream_t s = (hipStream_t)stream;
    st = mtl_dispatch_dtype(d->dtype, [&](auto t) {
        return bwd_impl<typename decltype(t)::type>(d, x, x_t, Wt, dy_s, dy_t, ctx, dx, dx_t, dA_s, dB_s, dA_t, dB_t, scratch, s, gate_s, gate_t);
    });
    if (st != MTLORA_OK) return st;
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

int mtlora_linear_bwd(const mtlora_linear_desc* d, const void* x, const void* const* x_t, const void* Wt,
                      const void* dy_s, const void* const* dy_t, const void* ctx, int64_t ctx_bytes, void* dx,
                      void* const* dx_t, float* dA_s, float* dB_s, float* const* dA_t, float* const* dB_t,
                      void* scratch, int64_t scratch_bytes, void* stream) {
    return linear_bwd_entry(d, x, x_t, Wt, dy_s, dy_t, ctx, ctx_bytes, dx, dx_t, dA_s, dB_s, dA_t, dB_t, scratch, scratch_bytes,
                            nullptr, nullptr, stream);
}

int mtlora_linear_bwd_gelu(const mtlora_linear_desc* d, const void* x, const void* const* x_t, const void* Wt,
                           const void* dy_s, const void* const* dy_t, const void* ctx, int64_t ctx_bytes, void* dx,
                           void* const* dx_t, float* dA_s, float* dB_s, float* const* dA_t, float* const* dB_t,
                           void* scratch, int64_t scratch_bytes, const void* h_s, const void* const* h_t, void* stream) {
    if (!h_s || !dx) return MTLORA_ERR_NULL;
    if (misaligned(h_s)) return MTLORA_ERR_ALIGN;
    for (int t = 0; t < d->T && d->has_x_tasks; ++t) {
        if (dx_t && dx_t[t] && (!h_t || !h_t[t])) return MTLORA_ERR_NULL;
        if (h_t && misaligned(h_t[t])) return MTLORA_ERR_ALIGN;
    }
    return linear_bwd_entry(d, x, x_t, Wt, dy_s, dy_t, ctx, ctx_bytes, dx, dx_t, dA_s, dB_s, dA_t, dB_t, scratch, scratch_bytes,
                            h_s, h_t, stream);
}

// ---- out (Na x Nb, fp32) = a^T b reduced over the M rows: the weight gradient dW = dY^T X of a plain linear layer whose
// output is narrow (the decoder heads' last 1x1 convolutions, seg_hrnet.py:518-526: Na = classes, Nb = 1080, M = B*H*W).
// Same split-M TN kernel as the LoRA factor gradients (k_tn + fixed-order k_tn_reduce: deterministic).
static int tn_plan(int64_t M, int Na, int Nb, int& tiles_a, int& tiles_b, int& nsplit, int64_t& rps) {
    tiles_a = (int)mtl_ceil_div(Na, TN_A);
    tiles_b = (int)mtl_ceil_div(Nb, TN_B);
    const int64_t tiles = (int64_t)tiles_a * tiles_b;
    nsplit = (int)(TN_TARGET_CTAS / (tiles > 0 ? tiles : 1));
    const int64_t max_by_rows = mtl_ceil_div(M, 256);
    if (nsplit > max_by_rows) nsplit = (int)max_by_rows;
    if (nsplit > 256) nsplit = 256;
    if (nsplit < 1) nsplit = 1;
    rps = mtl_round_up(mtl_ceil_div(M > 0 ? M : 1, nsplit), 64);
    return MTLORA_OK;
}

int64_t mtlora_gemm_tn_scratch_bytes(int64_t M, int Na, int Nb) {
    if (M < 0 || Na <= 0 || Nb <= 0) return -1;
    int ta, tb, ns;
    int64_t rps;
    tn_plan(M, Na, Nb, ta, tb, ns, rps);
    return (int64_t)ta * tb * ns * TN_TILE * 4 + 256;
}

int mtlora_gemm_tn(const void* a, const void* b, float* out, int64_t M, int Na, int Nb, int64_t lda, int64_t ldb,
                   int dtype, void* scratch, int64_t scratch_bytes, void* stream) {
    if (!mtl_dtype_in(dtype, MTL_DT_ALL)) return MTLORA_ERR_DTYPE;
    const int vec = mtl_vec_elems(dtype);
    if (M < 0 || M >= ((int64_t)1 << 31) || Na <= 0 || Nb <= 0 || lda < Na || ldb < Nb) return MTLORA_ERR_SHAPE;
    if (Na % vec || Nb % vec || lda % vec || ldb % vec) return MTLORA_ERR_ALIGN;
    if (Na > 1024) return MTLORA_ERR_UNSUPPORTED;  // narrow side only (every a-tile re-reads b)
    if (mtl_any_null({out, scratch}) || (M > 0 && mtl_any_null({a, b}))) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({a, b, scratch}) || mtl_any_misaligned({out}, 0, {}, 4)) return MTLORA_ERR_ALIGN;
    if (scratch_bytes < mtlora_gemm_tn_scratch_bytes(M, Na, Nb) - 256) return MTLORA_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (M == 0) {
        mtl_zero_async(out, (size_t)Na * Nb * 4, s);
        return MTLORA_OK;
    }
    TnParams tp = {};
    tp.M = M;
    int ta, tb;
    tn_plan(M, Na, Nb, ta, tb, tp.nsplit, tp.rows_per_split);
    tp.drop = mtl_make_dropout(0.f, 0, nullptr);
    tp.n_prob = 1;
    TnProblem& p = tp.p[0];
    p.A = a;
    p.B = b;
    p.lda = lda;
    p.ldb = ldb;
    p.a0 = 0;
    p.Na = Na;
    p.b0 = 0;
    p.Nb = Nb;
    p.b_mask = 0;
    p.tiles_a = ta;
    p.tiles_b = tb;
    p.part = reinterpret_cast<float*>(scratch);
    p.out = out;
    p.out_a = Na;
    p.out_b = Nb;
    p.ldo = Nb;
    p.transpose = 0;
    const int es = mtl_elem_size(dtype);
    {
        mtl_prof_tag("M%lld Na%d Nb%d", (long long)M, Na, Nb);
        MtlProfScope prof(PK_TN_PLAIN, (double)es * M * ((double)ta * Nb + Na), s, 0.0, 2.0 * M * (double)Na * Nb);
        mtl_dispatch_dtype(dtype, [&](auto t) {
            hipLaunchKernelGGL(k_tn<typename decltype(t)::type>, dim3((unsigned)tp.nsplit, (unsigned)(ta * tb), 1), dim3(256), 0, s, tp);
        });
    }
    MtlProfScope prof(PK_REDUCE, 0.0, s);
    hipLaunchKernelGGL(k_tn_reduce<>, dim3(TN_TILE / 1024, (unsigned)(ta * tb), 1), dim3(256 * TN_RG), 0, s, tp);
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}
}
