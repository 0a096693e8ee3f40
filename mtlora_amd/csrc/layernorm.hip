// layernorm.hip -- host side of the LayerNorm family (kernels: ln.h): the ten mtlora_*layernorm* entries, the two scratch-size
// queries and the two phased mtli_* entries of internal.h; and the three mtlora_sum_ln_add_* entries (kernels: sum_ln_add.h).
//
// Every entry is  validate -> fill LnParams -> plan -> launch:
//   validate   one helper per concern, always in this order (first failure wins):  ln_check status (dtypes, C) -> n range -> null
//              -> 16-byte alignment -> samples (B > 0, M % B == 0) -> workspace -> [M == 0 exit] -> merge geometry (ln_merge)
//   plan       ln_plan_fwd / ln_plan_bwd: LPR, vectors per lane, grid and LDS bytes from (M, C, x dtype); the scratch-size queries
//              are derived from ln_plan_bwd, so size and launch cannot disagree
//   launch     ln_run_fwd / ln_run_bwd through ln_dispatch, the one dtype x LPR x MAXV ladder
#include "dispatch.h"
#include "ln.h"
#include "sum_ln_add.h"

namespace {

constexpr int LN_MAXN = MTLORA_MAX_TASKS + 1;  // streams of the multi forms

int pick_lpr(int nvec) {
    int lpr = 8;
    while (lpr < 64 && (nvec + lpr - 1) / lpr > 3) lpr *= 2;
    return lpr;
}

int ln_grid(int64_t M, int lpr, int cap = 256 * 4, int unr = 1) {
    const int64_t rows_per_blk = 4 * (64 / lpr) * unr;
    int64_t g = mtl_ceil_div(M, rows_per_blk);
    if (g > cap) g = cap;  // also the number of dgamma/dbeta partials the second stage sums
    return (int)(g < 1 ? 1 : g);
}

// patch-merging gather: rows = B * (H/2) * (W/2), C = 4 * C_token, C_token a multiple of the vector width
int ln_merge(LnParams& p, int64_t M, int64_t C, int xdt, int mh, int mw) {
    p.mg_H = p.mg_W = 0;
    if (mh == 0 && mw == 0) return MTLORA_OK;
    const int ve = mtl_vec_elems(xdt);
    if (mh <= 0 || mw <= 0 || (mh & 1) || (mw & 1) || C % 4 || (C / 4) % ve) return MTLORA_ERR_SHAPE;
    if (M % ((int64_t)(mh / 2) * (mw / 2))) return MTLORA_ERR_SHAPE;
    p.mg_H = mh;
    p.mg_W = mw;
    return MTLORA_OK;
}

int ln_check(int64_t M, int64_t C, int xdt, int ydt) {
    if (!mtl_dtype_pair_ok(xdt, ydt)) return MTLORA_ERR_DTYPE;  // (bf16 <-> fp16 mixes: none)
    const int ve = mtl_vec_elems(xdt);
    if (M < 0 || C <= 0 || C % ve) return MTLORA_ERR_SHAPE;
    if (mtl_ceil_div(C / ve, 64) > LN_MAXV) return MTLORA_ERR_UNSUPPORTED;
    return MTLORA_OK;
}

bool ln_n_bad(int n) { return n < 1 || n > LN_MAXN; }

bool ln_samples_bad(int64_t M, int64_t B) { return B <= 0 || M % B; }

// ------------------------------------------------------------------------------------------------
// launch plan
// ------------------------------------------------------------------------------------------------
struct LnPlan {
    int lpr;           // lanes per row: 8 / 16 / 32 / 64
    int vpl;           // 16-byte vectors per lane per row: <= 3 -> the MAXV = 3 kernels, else MAXV = LN_MAXV
    int grid_x;        // workgroups along x (backward: also the dgamma / dbeta partials per stream)
    size_t lds_bytes;  // dynamic LDS of the main kernel
};

LnPlan ln_plan_row(int64_t C, int xdt) {
    const int nvec = (int)(C / mtl_vec_elems(xdt));
    LnPlan pl = {};
    pl.lpr = pick_lpr(nvec);
    pl.vpl = (nvec + pl.lpr - 1) / pl.lpr;
    return pl;
}

LnPlan ln_plan_fwd(int64_t M, int64_t C, int xdt) {
    LnPlan pl = ln_plan_row(C, xdt);
    const int g = (int)mtl_ceil_div(ln_grid(M, pl.lpr, 1 << 30), pl.vpl <= 3 ? 4 : 1);  // 4 row groups per wave iteration in the
    pl.grid_x = g < 256 * 8 ? g : 256 * 8;                                               // narrow-row kernels
    pl.lds_bytes = 0;
    return pl;
}

LnPlan ln_plan_bwd(int64_t M, int64_t C, int xdt) {
    LnPlan pl = ln_plan_row(C, xdt);
    pl.grid_x = ln_grid(M, pl.lpr);
    pl.lds_bytes = (size_t)4 * (64 / pl.lpr) * 2 * C * 4;  // [4 waves * 64/LPR row groups][2][C] column partials
    return pl;
}

// bytes of the [n][grid_x][2][C] fp32 partials the backward kernels write and k_ln_reduce reads
int64_t ln_part_bytes(int64_t M, int64_t C, int xdt, int n = 1) { return (int64_t)ln_plan_bwd(M, C, xdt).grid_x * 2 * C * 4 * n; }

// the ladder: f(MtlTag<TX>, MtlTag<TO>, MtlInt<LPR>, MtlInt<MAXV>) for the seven dtype pairs of mtl_dispatch_dtype_pair, the four LPR
// and MAXV 3 / LN_MAXV
template <typename F>
void ln_dispatch(int xdt, int odt, const LnPlan& pl, F&& f) {
    mtl_dispatch_dtype_pair(xdt, odt, [&](auto tx, auto to) {
        auto maxv = [&](auto lpr) {
            if (pl.vpl <= 3)
                f(tx, to, lpr, MtlInt<3>{});
            else
                f(tx, to, lpr, MtlInt<LN_MAXV>{});
        };
        switch (pl.lpr) {
            case 8: maxv(MtlInt<8>{}); break;
            case 16: maxv(MtlInt<16>{}); break;
            case 32: maxv(MtlInt<32>{}); break;
            default: maxv(MtlInt<64>{}); break;
        }
    });
}

// k_ln_fwd over (grid_x, ny) workgroups; res: the fused-residual instances.  prof_bytes: the entry's profiler byte figure
int ln_run_fwd(const LnParams& p, int xdt, int ydt, bool res, int ny, double prof_bytes, hipStream_t s) {
    const LnPlan pl = ln_plan_fwd(p.M, p.C, xdt);
    const dim3 grid((unsigned)pl.grid_x, (unsigned)ny);
    MtlProfScope prof(PK_LN_FWD, prof_bytes, s);
    ln_dispatch(xdt, ydt, pl, [&](auto tx, auto to, auto lpr, auto maxv) {
        using TX = typename decltype(tx)::type;
        using TO = typename decltype(to)::type;
        constexpr int LPR = decltype(lpr)::value, MAXV = decltype(maxv)::value;
        if (res)
            hipLaunchKernelGGL((k_ln_fwd<TX, TO, LPR, MAXV, true>), grid, dim3(256), pl.lds_bytes, s, p);
        else
            hipLaunchKernelGGL((k_ln_fwd<TX, TO, LPR, MAXV, false>), grid, dim3(256), pl.lds_bytes, s, p);
    });
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

// main backward kernel over (grid_x, ny) workgroups (shared_shortcut: k_resln_bwd_multi, else k_ln_bwd), then k_ln_reduce over its
// grid_x * ny partials.  phase (internal.h): 0 both, 1 main kernel only, 2 reduce only
int ln_run_bwd(const LnParams& p, int xdt, int gdt, bool shared_shortcut, int ny, float* dgamma, float* dbeta, int phase,
               double prof_bytes, hipStream_t s) {
    const LnPlan pl = ln_plan_bwd(p.M, p.C, xdt);
    const dim3 grid((unsigned)pl.grid_x, (unsigned)ny);
    if (phase != 2) {
        MtlProfScope prof(PK_LN_BWD, prof_bytes, s);
        ln_dispatch(xdt, gdt, pl, [&](auto tx, auto tg, auto lpr, auto maxv) {
            using TX = typename decltype(tx)::type;
            using TG = typename decltype(tg)::type;
            constexpr int LPR = decltype(lpr)::value, MAXV = decltype(maxv)::value;
            if (shared_shortcut)
                hipLaunchKernelGGL((k_resln_bwd_multi<TX, TG, LPR, MAXV>), grid, dim3(256), pl.lds_bytes, s, p);
            else
                hipLaunchKernelGGL((k_ln_bwd<TX, TG, LPR, MAXV>), grid, dim3(256), pl.lds_bytes, s, p);
        });
    }
    if (phase != 1)
        hipLaunchKernelGGL(k_ln_reduce, dim3((unsigned)mtl_ceil_div(2 * (int64_t)p.C, 64)), dim3(64 * LN_RW), 0, s,
                           (const float*)p.part, dgamma, dbeta, pl.grid_x * ny, p.C);
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

// backward with no rows: the parameter gradients are zero
int ln_bwd_empty(float* dgamma, float* dbeta, int64_t C, hipStream_t s) {
    mtl_zero_async(dgamma, (size_t)C * 4, s);
    mtl_zero_async(dbeta, (size_t)C * 4, s);
    return MTLORA_OK;
}

// ------------------------------------------------------------------------------------------------
// the three forms, forward and backward.  branch / d_branch null: the plain form (the public residual entries require them)
// ------------------------------------------------------------------------------------------------
int ln_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int64_t M, int64_t C, float eps,
           int x_dtype, int y_dtype, int merge_h, int merge_w, const void* branch, void* x_new, const float* scale, int64_t B,
           void* stream) {
    int st = ln_check(M, C, x_dtype, y_dtype);
    if (st != MTLORA_OK) return st;
    if (mtl_any_null({x, gamma, beta, y, mean, rstd})) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({x, y, branch, x_new})) return MTLORA_ERR_ALIGN;
    if (branch && ln_samples_bad(M, B)) return MTLORA_ERR_SHAPE;
    if (M == 0) return MTLORA_OK;
    LnParams p = {};
    p.rb = branch;
    p.xsum = x_new;
    p.rscale = scale;
    p.rows_per_sample = branch ? M / B : 1;
    p.x = x;
    p.gamma = gamma;
    p.beta = beta;
    p.y = y;
    p.mean = mean;
    p.rstd = rstd;
    p.M = M;
    p.C = (int)C;
    p.eps = eps;
    st = ln_merge(p, M, C, x_dtype, merge_h, merge_w);
    if (st != MTLORA_OK) return st;
    const int es_x = mtl_elem_size(x_dtype), es_y = mtl_elem_size(y_dtype);
    mtl_prof_tag("M%lld C%lld x%d y%d mg%d", (long long)M, (long long)C, x_dtype, y_dtype, merge_w);
    return ln_run_fwd(p, x_dtype, y_dtype, branch != nullptr, 1, (double)M * C * (es_x + es_y + (branch ? es_x + es_y : 0)),
                      (hipStream_t)stream);
}

int ln_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, void* dx, float* dgamma,
           float* dbeta, int64_t M, int64_t C, int x_dtype, int dy_dtype, void* scratch, int64_t scratch_bytes, const void* dx_addend,
           int merge_h, int merge_w, void* d_branch, const float* scale, int64_t B, void* stream, int phase = 0) {
    int st = ln_check(M, C, x_dtype, dy_dtype);
    if (st != MTLORA_OK) return st;
    if (mtl_any_null({dy, x, gamma, mean, rstd, dx, dgamma, dbeta, scratch})) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({x, dy, dx, scratch, dx_addend, d_branch})) return MTLORA_ERR_ALIGN;
    if (d_branch && ln_samples_bad(M, B)) return MTLORA_ERR_SHAPE;
    if (scratch_bytes < ln_part_bytes(M, C, x_dtype)) return MTLORA_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (M == 0) return ln_bwd_empty(dgamma, dbeta, C, s);
    LnParams p = {};
    p.x = x;
    p.dy = dy;
    p.gamma = gamma;
    p.mean = const_cast<float*>(mean);
    p.rstd = const_cast<float*>(rstd);
    p.dx = dx;
    p.add = dx_addend;
    p.dbr = d_branch;
    p.rscale = scale;
    p.rows_per_sample = d_branch ? M / B : 1;
    p.part = reinterpret_cast<float*>(scratch);
    p.M = M;
    p.C = (int)C;
    st = ln_merge(p, M, C, x_dtype, merge_h, merge_w);
    if (st != MTLORA_OK) return st;
    const int es_x = mtl_elem_size(x_dtype), es_g = mtl_elem_size(dy_dtype);
    if (phase != 2)
        mtl_prof_tag("M%lld C%lld x%d g%d mg%d add%d", (long long)M, (long long)C, x_dtype, dy_dtype, merge_w, dx_addend ? 1 : 0);
    return ln_run_bwd(p, x_dtype, dy_dtype, false, 1, dgamma, dbeta, phase,
                      (double)M * C * (2 * es_x + es_g + (dx_addend ? es_x : 0) + (d_branch ? es_g : 0)), s);
}

// n independent streams through the same LayerNorm (multi_x), each optionally with its own residual
int ln_streams_fwd(int n, const void* const* x, const float* gamma, const float* beta, void* const* y, float* const* mean,
                   float* const* rstd, int64_t M, int64_t C, float eps, int x_dtype, int y_dtype, int merge_h, int merge_w,
                   const void* const* branch, void* const* x_new, const float* scale, int64_t B, void* stream) {
    int st = ln_check(M, C, x_dtype, y_dtype);
    if (st != MTLORA_OK) return st;
    if (ln_n_bad(n)) return MTLORA_ERR_SHAPE;
    if (mtl_any_null({gamma, beta}, n, {x, mtl_arr(y), mtl_arr(mean), mtl_arr(rstd)})) return MTLORA_ERR_NULL;
    if (branch && mtl_any_null({}, n, {branch, mtl_arr(x_new)})) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({}, n, {x, mtl_arr(y), branch, mtl_arr(x_new)})) return MTLORA_ERR_ALIGN;
    if (branch && ln_samples_bad(M, B)) return MTLORA_ERR_SHAPE;
    if (M == 0) return MTLORA_OK;
    LnParams p = {};
    for (int k = 0; k < n; ++k) {
        p.x_k[k] = x[k];
        p.y_k[k] = y[k];
        p.mean_k[k] = mean[k];
        p.rstd_k[k] = rstd[k];
        if (branch) {
            p.rb_k[k] = branch[k];
            p.xsum_k[k] = x_new[k];
        }
    }
    if (branch) {
        p.rb = branch[0];
        p.xsum = x_new[0];
        p.rscale = scale;
    }
    p.multi_x = 1;
    p.x = x[0];
    p.y = y[0];
    p.mean = mean[0];
    p.rstd = rstd[0];
    p.gamma = gamma;
    p.beta = beta;
    p.M = M;
    p.C = (int)C;
    p.eps = eps;
    p.rows_per_sample = branch ? M / B : 1;
    st = ln_merge(p, M, C, x_dtype, merge_h, merge_w);
    if (st != MTLORA_OK) return st;
    const int es_x = mtl_elem_size(x_dtype), es_y = mtl_elem_size(y_dtype);
    mtl_prof_tag("M%lld C%lld x%d y%d mg%d n%d res%d", (long long)M, (long long)C, x_dtype, y_dtype, merge_w, n, branch ? 1 : 0);
    return ln_run_fwd(p, x_dtype, y_dtype, branch != nullptr, n, (double)n * M * C * (es_x + es_y + (branch ? es_x + es_y : 0)),
                      (hipStream_t)stream);
}

int ln_streams_bwd(int n, const void* const* dy, const void* const* x, const float* gamma, const float* const* mean,
                   const float* const* rstd, void* const* dx, float* dgamma, float* dbeta, int64_t M, int64_t C, int x_dtype,
                   int dy_dtype, void* scratch, int64_t scratch_bytes, const void* const* dx_addend, int merge_h, int merge_w,
                   void* const* d_branch, const float* scale, int64_t B, void* stream) {
    int st = ln_check(M, C, x_dtype, dy_dtype);
    if (st != MTLORA_OK) return st;
    if (ln_n_bad(n)) return MTLORA_ERR_SHAPE;
    if (mtl_any_null({gamma, dgamma, dbeta, scratch}, n, {dy, x, mtl_arr(mean), mtl_arr(rstd), mtl_arr(dx)})) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({scratch}, n, {dy, x, mtl_arr(dx), dx_addend, mtl_arr(d_branch)})) return MTLORA_ERR_ALIGN;
    if (d_branch && ln_samples_bad(M, B)) return MTLORA_ERR_SHAPE;
    if (scratch_bytes < ln_part_bytes(M, C, x_dtype, n)) return MTLORA_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (M == 0) return ln_bwd_empty(dgamma, dbeta, C, s);
    LnParams p = {};
    for (int k = 0; k < n; ++k) {
        p.dy_k[k] = dy[k];
        p.x_k[k] = x[k];
        p.dx_k[k] = dx[k];
        p.add_k[k] = dx_addend ? dx_addend[k] : nullptr;
        p.mean_k[k] = const_cast<float*>(mean[k]);
        p.rstd_k[k] = const_cast<float*>(rstd[k]);
        if (d_branch) p.dbr_k[k] = d_branch[k];
    }
    p.multi_x = 1;
    p.x = x[0];
    p.dy = dy[0];
    p.dx = dx[0];
    p.gamma = gamma;
    p.mean = const_cast<float*>(mean[0]);
    p.rstd = const_cast<float*>(rstd[0]);
    p.part = reinterpret_cast<float*>(scratch);
    p.M = M;
    p.C = (int)C;
    p.rscale = d_branch ? scale : nullptr;
    p.rows_per_sample = d_branch ? M / B : 1;
    st = ln_merge(p, M, C, x_dtype, merge_h, merge_w);
    if (st != MTLORA_OK) return st;
    const int es_x = mtl_elem_size(x_dtype), es_g = mtl_elem_size(dy_dtype);
    mtl_prof_tag("M%lld C%lld x%d g%d mg%d n%d", (long long)M, (long long)C, x_dtype, dy_dtype, merge_w, n);
    return ln_run_bwd(p, x_dtype, dy_dtype, false, n, dgamma, dbeta, 0, (double)n * M * C * (2 * es_x + es_g + (dx_addend ? es_x : 0)),
                      s);
}


// ------------------------------------------------------------------------------------------------
// SHARED_MODE "addition" (kernels: sum_ln_add.h): one tensor dtype, rows up to SNA_MAXV vectors per lane
// ------------------------------------------------------------------------------------------------
int sna_check(int n, int64_t M, int64_t N, int dtype) {
    if (!mtl_dtype_in(dtype, MTL_DT_ALL)) return MTLORA_ERR_DTYPE;
    const int ve = mtl_vec_elems(dtype);
    if (M < 0 || N <= 0 || N % ve) return MTLORA_ERR_SHAPE;
    if (mtl_ceil_div(N / ve, 64) > (dtype == MTLORA_F32 ? SNA_MAXV : LN_MAXV)) return MTLORA_ERR_UNSUPPORTED;
    if (n < 1 || n > MTLORA_MAX_TASKS) return MTLORA_ERR_SHAPE;
    return MTLORA_OK;
}

// f(MtlTag<T>, MtlInt<LPR>, MtlInt<MAXV>): MAXV 3 for the four LPR; 8, and 16 for fp32, at LPR 64 (pick_lpr leaves more than three
// vectors per lane only there)
template <typename F>
void sna_dispatch(int dtype, const LnPlan& pl, F&& f) {
    mtl_dispatch_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        if (pl.vpl > 3) {
            if constexpr (sizeof(T) == 4) {
                if (pl.vpl > LN_MAXV) {
                    f(t, MtlInt<64>{}, MtlInt<SNA_MAXV>{});
                    return;
                }
            }
            f(t, MtlInt<64>{}, MtlInt<LN_MAXV>{});
            return;
        }
        switch (pl.lpr) {
            case 8: f(t, MtlInt<8>{}, MtlInt<3>{}); break;
            case 16: f(t, MtlInt<16>{}, MtlInt<3>{}); break;
            case 32: f(t, MtlInt<32>{}, MtlInt<3>{}); break;
            default: f(t, MtlInt<64>{}, MtlInt<3>{}); break;
        }
    });
}

// workgroups of the backward launch = dgamma / dbeta partials; the forward takes up to twice as many
int sna_grid_bwd(int64_t M, int64_t N, int dtype) { return ln_grid(M, ln_plan_row(N, dtype).lpr); }
int64_t sna_part_bytes(int64_t M, int64_t N, int dtype) { return (int64_t)sna_grid_bwd(M, N, dtype) * 2 * N * 4; }

}  // namespace

extern "C" {

/* SHARED_MODE "addition" (reference lora.py:275-284): out = y + LayerNorm(sum_k y_t[k]) in one launch, tot never stored. */
int mtlora_sum_ln_add_fwd(int n, const void* const* y_t, const void* y, const float* gamma, const float* beta, void* out,
                                 float* mean, float* rstd, int64_t M, int64_t N, float eps, int dtype, void* stream) {
    int st = sna_check(n, M, N, dtype);
    if (st != MTLORA_OK) return st;
    if (M == 0) return MTLORA_OK;  // (before the pointers: tensors without rows have no address)
    if (mtl_any_null({y, gamma, beta, out, mean, rstd}, n, {y_t})) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({y, out, gamma, beta}, n, {y_t})) return MTLORA_ERR_ALIGN;
    SnaParams p = {};
    for (int k = 0; k < n; ++k) p.yt[k] = y_t[k];
    p.y = y;
    p.out = out;
    p.gamma = gamma;
    p.beta = beta;
    p.mean = mean;
    p.rstd = rstd;
    p.M = M;
    p.C = (int)N;
    p.n = n;
    p.eps = eps;
    const LnPlan pl = ln_plan_row(N, dtype);
    const int grid = ln_grid(M, pl.lpr, 256 * 8);
    hipStream_t s = (hipStream_t)stream;
    mtl_prof_tag("M%lld N%lld dt%d n%d", (long long)M, (long long)N, dtype, n);
    MtlProfScope prof(PK_SUM_LN_ADD_FWD, (double)M * N * mtl_elem_size(dtype) * (n + 2), s);
    sna_dispatch(dtype, pl, [&](auto t, auto lpr, auto maxv) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((k_sum_ln_add_fwd<T, decltype(lpr)::value, decltype(maxv)::value>), dim3((unsigned)grid), dim3(256), 0, s, p);
    });
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

int64_t mtlora_sum_ln_add_bwd_scratch_bytes(int n, int64_t M, int64_t N, int dtype) {
    if (sna_check(n, M, N, dtype) != MTLORA_OK) return -1;
    return sna_part_bytes(M, N, dtype) + 256;
}

/* backward of mtlora_sum_ln_add_fwd (reference lora.py:275-284): dy_t[k] = dy_t_addend[k] + LN-backward(dout) with tot formed
 * again from y_t; the gradient of y is dout itself and is not written here.  dgamma / dbeta: partials in scratch, fixed-order reduce. */
int mtlora_sum_ln_add_bwd(int n, const void* dout, const void* const* y_t, const float* gamma, const float* mean,
                                 const float* rstd, const void* const* dy_t_addend, void* const* dy_t, float* dgamma, float* dbeta,
                                 int64_t M, int64_t N, int dtype, void* scratch, int64_t scratch_bytes, void* stream) {
    int st = sna_check(n, M, N, dtype);
    if (st != MTLORA_OK) return st;
    if ((dgamma == nullptr) != (dbeta == nullptr)) return MTLORA_ERR_NULL;  // both, or neither (a frozen lora_norm: no reduce)
    hipStream_t s = (hipStream_t)stream;
    if (M == 0) return dgamma ? ln_bwd_empty(dgamma, dbeta, N, s) : MTLORA_OK;  // (before the row tensors' pointers, as the forward)
    if (mtl_any_null({dout, gamma, mean, rstd, scratch}, n, {y_t, mtl_arr(dy_t)})) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({dout, gamma, scratch}, n, {y_t, dy_t_addend, mtl_arr(dy_t)})) return MTLORA_ERR_ALIGN;
    if (scratch_bytes < sna_part_bytes(M, N, dtype)) return MTLORA_ERR_WORKSPACE;
    SnaParams p = {};
    int n_add = 0;
    for (int k = 0; k < n; ++k) {
        p.yt[k] = y_t[k];
        p.add[k] = dy_t_addend ? dy_t_addend[k] : nullptr;
        p.dyt[k] = dy_t[k];
        n_add += p.add[k] ? 1 : 0;
    }
    p.y = dout;
    p.gamma = gamma;
    p.mean = const_cast<float*>(mean);
    p.rstd = const_cast<float*>(rstd);
    p.part = reinterpret_cast<float*>(scratch);
    p.M = M;
    p.C = (int)N;
    p.n = n;
    const LnPlan pl = ln_plan_row(N, dtype);
    const int grid = sna_grid_bwd(M, N, dtype);
    mtl_prof_tag("M%lld N%lld dt%d n%d add%d", (long long)M, (long long)N, dtype, n, n_add);
    MtlProfScope prof(PK_SUM_LN_ADD_BWD, (double)M * N * mtl_elem_size(dtype) * (2 * n + 1 + n_add), s);
    sna_dispatch(dtype, pl, [&](auto t, auto lpr, auto maxv) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((k_sum_ln_add_bwd<T, decltype(lpr)::value, decltype(maxv)::value>), dim3((unsigned)grid), dim3(256), 0, s, p);
    });
    if (dgamma)
        hipLaunchKernelGGL(k_ln_reduce, dim3((unsigned)mtl_ceil_div(2 * N, 64)), dim3(64 * LN_RW), 0, s, (const float*)p.part, dgamma,
                           dbeta, grid, (int)N);
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

int64_t mtlora_layernorm_bwd_scratch_bytes(int64_t M, int64_t C, int x_dtype) {
    if (ln_check(M, C, x_dtype, MTLORA_F32) != MTLORA_OK) return -1;
    return ln_part_bytes(M, C, x_dtype) + 256;
}

int64_t mtlora_layernorm_multi_bwd_scratch_bytes(int n, int64_t M, int64_t C, int x_dtype) {
    if (ln_check(M, C, x_dtype, MTLORA_F32) != MTLORA_OK || ln_n_bad(n)) return -1;
    return ln_part_bytes(M, C, x_dtype, n) + 256;
}

int mtlora_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                         int64_t M, int64_t C, float eps, int x_dtype, int y_dtype, int merge_h, int merge_w, void* stream) {
    return ln_fwd(x, gamma, beta, y, mean, rstd, M, C, eps, x_dtype, y_dtype, merge_h, merge_w, nullptr, nullptr, nullptr, 1, stream);
}

int mtlora_residual_layernorm_fwd(const void* shortcut, const void* branch, const float* scale, int64_t B, const float* gamma,
                                  const float* beta, void* x_new, void* y, float* mean, float* rstd, int64_t M, int64_t C,
                                  float eps, int x_dtype, int y_dtype, void* stream) {
    if (!branch || !x_new) return MTLORA_ERR_NULL;
    return ln_fwd(shortcut, gamma, beta, y, mean, rstd, M, C, eps, x_dtype, y_dtype, 0, 0, branch, x_new, scale, B, stream);
}

int mtli_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, void* dx,
                       float* dgamma, float* dbeta, int64_t M, int64_t C, int x_dtype, int dy_dtype, void* scratch,
                       int64_t scratch_bytes, const void* dx_addend, int phase, void* stream) {
    return ln_bwd(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, M, C, x_dtype, dy_dtype, scratch, scratch_bytes, dx_addend, 0, 0,
                  nullptr, nullptr, 1, stream, phase);
}

int mtli_residual_layernorm_bwd(const void* dy, const void* x_new, const float* gamma, const float* mean, const float* rstd,
                                void* d_shortcut, void* d_branch, float* dgamma, float* dbeta, const float* scale, int64_t B,
                                int64_t M, int64_t C, int x_dtype, int dy_dtype, void* scratch, int64_t scratch_bytes,
                                const void* dx_addend, int phase, void* stream) {
    if (!d_branch) return MTLORA_ERR_NULL;
    return ln_bwd(dy, x_new, gamma, mean, rstd, d_shortcut, dgamma, dbeta, M, C, x_dtype, dy_dtype, scratch, scratch_bytes, dx_addend,
                  0, 0, d_branch, scale, B, stream, phase);
}

int mtlora_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                         void* dx, float* dgamma, float* dbeta, int64_t M, int64_t C, int x_dtype, int dy_dtype,
                         void* scratch, int64_t scratch_bytes, const void* dx_addend, int merge_h, int merge_w, void* stream) {
    return ln_bwd(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, M, C, x_dtype, dy_dtype, scratch, scratch_bytes, dx_addend, merge_h,
                  merge_w, nullptr, nullptr, 1, stream);
}

int mtlora_residual_layernorm_bwd(const void* dy, const void* x_new, const float* gamma, const float* mean, const float* rstd,
                                  void* d_shortcut, void* d_branch, float* dgamma, float* dbeta, const float* scale,
                                  int64_t B, int64_t M, int64_t C, int x_dtype, int dy_dtype, void* scratch,
                                  int64_t scratch_bytes, const void* dx_addend, void* stream) {
    if (!d_branch) return MTLORA_ERR_NULL;
    return ln_bwd(dy, x_new, gamma, mean, rstd, d_shortcut, dgamma, dbeta, M, C, x_dtype, dy_dtype, scratch, scratch_bytes, dx_addend,
                  0, 0, d_branch, scale, B, stream);
}

/* n independent inputs through the SAME LayerNorm in one launch each way (PatchMerging's norm applied to the shared tensor and
 * to every task tensor, swin_transformer_mtlora.py:543-551): dgamma / dbeta come out summed over the inputs. */
int mtlora_layernorm_multi_fwd(int n, const void* const* x, const float* gamma, const float* beta, void* const* y,
                               float* const* mean, float* const* rstd, int64_t M, int64_t C, float eps, int x_dtype, int y_dtype,
                               int merge_h, int merge_w, void* stream) {
    return ln_streams_fwd(n, x, gamma, beta, y, mean, rstd, M, C, eps, x_dtype, y_dtype, merge_h, merge_w, nullptr, nullptr, nullptr,
                          1, stream);
}

int mtlora_layernorm_multi_bwd(int n, const void* const* dy, const void* const* x, const float* gamma, const float* const* mean,
                               const float* const* rstd, void* const* dx, float* dgamma, float* dbeta, int64_t M, int64_t C,
                               int x_dtype, int dy_dtype, void* scratch, int64_t scratch_bytes, const void* const* dx_addend,
                               int merge_h, int merge_w, void* stream) {
    return ln_streams_bwd(n, dy, x, gamma, mean, rstd, dx, dgamma, dbeta, M, C, x_dtype, dy_dtype, scratch, scratch_bytes, dx_addend,
                          merge_h, merge_w, nullptr, nullptr, 1, stream);
}

/* n independent streams, each  x_new[k] = res[k] + scale[k][sample] * branch[k]  then the SAME LayerNorm (plain rows or the
 * PatchMerging gather): the MLP residual of the task-enabled block fused with the stage's PatchMerging norm. */
int mtlora_residual_layernorm_streams_fwd(int n, const void* const* res, const void* const* branch, const float* scale,
                                          int64_t B, const float* gamma, const float* beta, void* const* x_new, void* const* y,
                                          float* const* mean, float* const* rstd, int64_t M, int64_t C, float eps, int x_dtype,
                                          int y_dtype, int merge_h, int merge_w, void* stream) {
    if (!branch || !x_new) return MTLORA_ERR_NULL;
    return ln_streams_fwd(n, res, gamma, beta, y, mean, rstd, M, C, eps, x_dtype, y_dtype, merge_h, merge_w, branch, x_new, scale, B,
                          stream);
}

/* backward of mtlora_residual_layernorm_streams_fwd: d_res[k] = dx_addend[k] + LN-backward(dy[k]) (layout of res),
 * d_branch[k] = scale[k][sample] * d_res[k]; dgamma / dbeta summed over the streams. */
int mtlora_residual_layernorm_streams_bwd(int n, const void* const* dy, const void* const* x_new, const float* gamma,
                                          const float* const* mean, const float* const* rstd, void* const* d_res,
                                          void* const* d_branch, float* dgamma, float* dbeta, const float* scale, int64_t B,
                                          int64_t M, int64_t C, int x_dtype, int dy_dtype, void* scratch, int64_t scratch_bytes,
                                          const void* const* dx_addend, int merge_h, int merge_w, void* stream) {
    if (!d_branch) return MTLORA_ERR_NULL;
    return ln_streams_bwd(n, dy, x_new, gamma, mean, rstd, d_res, dgamma, dbeta, M, C, x_dtype, dy_dtype, scratch, scratch_bytes,
                          dx_addend, merge_h, merge_w, d_branch, scale, B, stream);
}

/* multi-stream forms: ONE shortcut, n branches -> n (x_new, y) pairs (task-enabled Swin block: swin_transformer_mtlora.py:389-396
 * for the shared stream and every task stream) */
int mtlora_residual_layernorm_multi_fwd(int n, const void* shortcut, const void* const* branch, const float* scale, int64_t B,
                                        const float* gamma, const float* beta, void* const* x_new, void* const* y,
                                        float* const* mean, float* const* rstd, int64_t M, int64_t C, float eps, int x_dtype,
                                        int y_dtype, void* stream) {
    int st = ln_check(M, C, x_dtype, y_dtype);
    if (st != MTLORA_OK) return st;
    if (ln_n_bad(n)) return MTLORA_ERR_SHAPE;
    if (mtl_any_null({shortcut, gamma, beta}, n, {branch, mtl_arr(x_new), mtl_arr(y), mtl_arr(mean), mtl_arr(rstd)})) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({shortcut}, n, {branch, mtl_arr(x_new), mtl_arr(y)})) return MTLORA_ERR_ALIGN;
    if (ln_samples_bad(M, B)) return MTLORA_ERR_SHAPE;
    if (M == 0) return MTLORA_OK;
    LnParams p = {};
    for (int k = 0; k < n; ++k) {
        p.rb_k[k] = branch[k];
        p.xsum_k[k] = x_new[k];
        p.y_k[k] = y[k];
        p.mean_k[k] = mean[k];
        p.rstd_k[k] = rstd[k];
    }
    p.nk = n;
    p.x = shortcut;
    p.gamma = gamma;
    p.beta = beta;
    p.rb = branch[0];
    p.xsum = x_new[0];
    p.y = y[0];
    p.mean = mean[0];
    p.rstd = rstd[0];
    p.rscale = scale;
    p.rows_per_sample = M / B;
    p.M = M;
    p.C = (int)C;
    p.eps = eps;
    const int es_x = mtl_elem_size(x_dtype), es_y = mtl_elem_size(y_dtype);
    mtl_prof_tag("M%lld C%lld x%d y%d n%d", (long long)M, (long long)C, x_dtype, y_dtype, n);
    return ln_run_fwd(p, x_dtype, y_dtype, true, n, (double)M * C * (es_x + (double)n * (es_x + 2 * es_y)), (hipStream_t)stream);
}

/* d_shortcut = sum_k (dx_addend[k] + LN-backward(dy[k]));  d_branch[k] = scale[k][sample] * (dx_addend[k] + LN-backward(dy[k]));
 * dgamma / dbeta summed over the streams.  dx_addend[k] / d_branch[k] may be NULL. */
int mtlora_residual_layernorm_multi_bwd(int n, const void* const* dy, const void* const* x_new, const float* gamma,
                                        const float* const* mean, const float* const* rstd, const void* const* dx_addend,
                                        void* d_shortcut, void* const* d_branch, float* dgamma, float* dbeta, const float* scale,
                                        int64_t B, int64_t M, int64_t C, int x_dtype, int dy_dtype, void* scratch,
                                        int64_t scratch_bytes, void* stream) {
    int st = ln_check(M, C, x_dtype, dy_dtype);
    if (st != MTLORA_OK) return st;
    if (ln_n_bad(n)) return MTLORA_ERR_SHAPE;
    if (mtl_any_null({gamma, d_shortcut, dgamma, dbeta, scratch}, n, {dy, x_new, mtl_arr(mean), mtl_arr(rstd)})) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({d_shortcut, scratch}, n, {dy, x_new, dx_addend, mtl_arr(d_branch)})) return MTLORA_ERR_ALIGN;
    if (ln_samples_bad(M, B)) return MTLORA_ERR_SHAPE;
    if (scratch_bytes < ln_part_bytes(M, C, x_dtype)) return MTLORA_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (M == 0) return ln_bwd_empty(dgamma, dbeta, C, s);
    LnParams p = {};
    for (int k = 0; k < n; ++k) {
        p.dy_k[k] = dy[k];
        p.xsum_k[k] = const_cast<void*>(x_new[k]);
        p.mean_k[k] = const_cast<float*>(mean[k]);
        p.rstd_k[k] = const_cast<float*>(rstd[k]);
        p.add_k[k] = dx_addend ? dx_addend[k] : nullptr;
        p.dbr_k[k] = d_branch ? d_branch[k] : nullptr;
    }
    p.nk = n;
    p.gamma = gamma;
    p.dx = d_shortcut;
    p.rscale = scale;
    p.rows_per_sample = M / B;
    p.part = reinterpret_cast<float*>(scratch);
    p.M = M;
    p.C = (int)C;
    const int es_x = mtl_elem_size(x_dtype), es_g = mtl_elem_size(dy_dtype);
    mtl_prof_tag("M%lld C%lld x%d g%d n%d", (long long)M, (long long)C, x_dtype, dy_dtype, n);
    return ln_run_bwd(p, x_dtype, dy_dtype, true, 1, dgamma, dbeta, 0, (double)M * C * (es_x + (double)n * (2 * es_x + 2 * es_g)), s);
}
}
