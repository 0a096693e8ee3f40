/*
 * mtlora_hip.h -- C ABI of libmtlora_hip.so, the MI355X (gfx950) implementation of the
 * MTLoRA data-parallel hot path.
 *
 * Boundary contract:
 *   - plain C, raw DEVICE pointers + sizes + a dtype enum + a hipStream_t passed as void*;
 *     no torch / ATen / pybind types anywhere;
 *   - the CALLER owns every buffer (inputs, outputs, ctx, scratch); the library never
 *     allocates, frees, retains a pointer or synchronises; every launch goes on `stream`;
 *   - re-entrant (safe from the autograd thread and across DDP ranks): nothing a call computes depends on state left by
 *     another call.  The only process-wide state is a per-device cache of device facts (CU count, "dynamic LDS limit raised"
 *     marks) and the opt-in profiler of mtlora_prof_begin/end; kernel selection is a function of the descriptor alone
 *     (ABI v6: no environment variable influences what the library computes or which kernel it picks; the
 *     opt-in profiler alone reads MTLORA_PROF_DUMP, a file name for its record dump, in mtlora_prof_end);
 *   - every function returns MTLORA_OK (0) or a negative mtlora_status; the Python shim
 *     (mtlora_amd/_lib.py) turns a non-zero status into RuntimeError -- the same observable
 *     behaviour as the reference's AT_ASSERTM -> RuntimeError (swin_window_process.cpp:64-66).
 *
 * Each entry point cites the reference interface it replaces.
 */
#ifndef MTLORA_HIP_H
#define MTLORA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTLORA_ABI_VERSION 12
#define MTLORA_MAX_TASKS 8

typedef enum mtlora_dtype {
    MTLORA_F32 = 0,  /* exact-f32 MFMA path (v_mfma_f32_32x32x2_f32) */
    MTLORA_BF16 = 1, /* bf16 in/out, fp32 accumulate (v_mfma_f32_32x32x16_bf16) */
    MTLORA_F16 = 2,  /* fp16 in/out, fp32 accumulate (v_mfma_f32_32x32x16_f16): MTLoRALinear, window attention, gemm_tn, the
                        window_process copies and the block glue (LayerNorm family, residual + DropPath, BatchNorm + ReLU) -- the
                        reference's default autocast dtype (main.py:341), and mtlora_upsample_cl_fwd / _bwd; loss / column-sum entries take
                        fp32 / bf16 */
    MTLORA_U8 = 3    /* OUTPUT dtype of mtlora_upsample_predict (ABI v11): class ids and [0, 255] images; SOURCE dtype of the
                        image and class-map jobs of mtlora_ingest_batch (ABI v12) */
} mtlora_dtype;

typedef enum mtlora_status {
    MTLORA_OK = 0,
    MTLORA_ERR_DTYPE = -1,
    MTLORA_ERR_SHAPE = -2,
    MTLORA_ERR_ALIGN = -3,
    MTLORA_ERR_NULL = -4,
    MTLORA_ERR_WORKSPACE = -5,
    MTLORA_ERR_HIP = -6,
    MTLORA_ERR_UNSUPPORTED = -7
} mtlora_status;

/* ABI version of the loaded library (== MTLORA_ABI_VERSION of the header it was built from). */
int mtlora_version(void);
const char* mtlora_error_string(int status);

/* ------------------------------------------------------------------------------------------
 * Window process -- replaces the pybind module `swin_window_process`
 * (kernels/window_process/swin_window_process.cpp:127-132) and its four CUDA kernels
 * (swin_window_process_kernel.cu:42,69,96,124).  Same argument meaning and SIGN CONVENTION:
 *   WindowProcess.apply(x,B,H,W,C,-shift,ws)         -> *_partition_forward (shift_size = -shift)
 *   WindowProcessReverse.apply(w,B,H,W,C,+shift,ws)  -> *_merge_and_roll_forward (shift_size = +shift)
 * Differences: output is caller-allocated; bf16 supported (reference: fp16/fp32 only,
 * .cu:170-175); correct for H != W (reference .cu:113-115 is only exact for square maps);
 * launches on `stream` (reference: default stream, .cu:178).
 * `image` is (B,H,W,C) contiguous, `windows` is (B*(H/ws)*(W/ws), ws, ws, C) contiguous.
 * ------------------------------------------------------------------------------------------ */
int mtlora_roll_and_window_partition_forward(const void* image, void* windows, int64_t B, int64_t H, int64_t W,
                                             int64_t C, int shift_size, int window_size, int dtype, void* stream);
int mtlora_roll_and_window_partition_backward(const void* grad_windows, void* grad_image, int64_t B, int64_t H,
                                              int64_t W, int64_t C, int shift_size, int window_size, int dtype,
                                              void* stream);
int mtlora_window_merge_and_roll_forward(const void* windows, void* image, int64_t B, int64_t H, int64_t W,
                                         int64_t C, int shift_size, int window_size, int dtype, void* stream);
int mtlora_window_merge_and_roll_backward(const void* grad_image, void* grad_windows, int64_t B, int64_t H,
                                          int64_t W, int64_t C, int shift_size, int window_size, int dtype,
                                          void* stream);

/* ------------------------------------------------------------------------------------------
 * MTLoRALinear -- replaces the ATen op sequence of models/lora.py:253-284 (forward) and its
 * autograd backward:
 *   Y_s = X W^T + b + s_s (D(X) A_s^T) B_s^T
 *   Y_t = X W^T + b [+ s_s(...) if mode==matrixv2] + s_t (X_t A_t^T) B_t^T,   X_t = x_tasks[t] or D(X)
 * D = dropout(p) (train only; counter-based generator `mtl_dropout_keep`, restated in
 * oracle/mtlora_oracle.py:dropout_keep_mask).  'addition' mode = r_s 0 + T>0 here; its
 * LayerNorm(sum_t) tail is applied by the host module.
 *
 * Layouts: X, X_t, Y_*: (M,K)/(M,N) row-major in `dtype`.  W (N,K), bias (N): `dtype` / fp32.
 * LoRA masters A_* (r,K), B_* (N,r): fp32 (the nn.Parameters themselves).  Parameter
 * gradients are fp32.  Wt is W transposed, (K,N) row-major in `dtype` (W is frozen; the host
 * caches it).
 * ------------------------------------------------------------------------------------------ */
typedef struct mtlora_linear_desc {
    int64_t M, K, N;
    int32_t dtype;      /* MTLORA_F32 | MTLORA_BF16 | MTLORA_F16 */
    int32_t mode;       /* 0 = 'matrix', 1 = 'matrixv2' (lora.py:259-274) */
    int32_t T;          /* number of task outputs, 0..MTLORA_MAX_TASKS (0 <=> tasks is None) */
    int32_t r_s;        /* shared rank, 0 = no shared update */
    int32_t r_t[MTLORA_MAX_TASKS];
    float scale_s;
    float scale_t[MTLORA_MAX_TASKS];
    int32_t has_x_tasks; /* 1: task t reads x_t[t] undropped; 0: task t reads D(X) (lora.py:262-263) */
    float dropout_p;     /* 0 in eval */
    uint64_t seed;       /* dropout seed of this call (same value for fwd and bwd) */
    const uint64_t* seed_offset; /* optional DEVICE pointer (null = none): the kernels use seed + *seed_offset (mod 2^64),
                                    read when they run -- a captured HIP graph draws fresh masks on every replay by
                                    bumping that one device word between replays (ABI v2) */
    int32_t bwd_phase;   /* backward only (ABI v3).  0: everything on `stream`.  1: dX / dX_t only (and the Q = alpha dY B
                            scratch the factor gradients need); 2: the factor gradients dA_* / dB_* only -- lets the caller
                            put them on a second stream next to the rest of the backward chain: call phase 1 on stream s1,
                            order s2 after it (event), call phase 2 with the SAME arguments on s2, and join s2 before the
                            gradients are read.  Nothing but dA / dB depends on phase 2. */
    /* ---- kernel selection (ABI v6; all 0 = the library's own choice).  Results are the same whatever is selected (the
     * kernel families are bit-compatible up to fp32 summation order); tests pin every family against the oracle by forcing
     * it on shapes far below the sizes at which the library would pick it, and A/B timing uses the same switches. */
    int32_t sel_stream;  /* wave-streaming kernels (csrc/stream.h): 0 wherever eligible, 1 never (tiled kernels only) */
    int32_t sel_dense;   /* k_ntd / k_nte (csrc/dense.h), single-output MFMA-dense launches: 0 by shape heuristics, 1 never, 2 k_ntd whenever
                            eligible, 3 k_nte (two 4-wave workgroups per CU) whenever eligible, 4 heuristics without k_nte (A/B) */
    int32_t sel_tn;      /* k_sp_tn, streaming factor gradients: 0 when every wave gets >= 8 slabs, 1 never, 2 whenever eligible */
    int32_t sel_projk;   /* P / Q passes whose projection rows do not fit in LDS: 0 heuristics (k_sp_projk on single-round launches, k_pq on
                            single-source passes, tiled otherwise), 1 tiled only, 2 k_sp_projk whenever eligible, 3 k_pq whenever eligible */
    int32_t max_cu;      /* 0: size persistent grids for the whole device; n > 0: as if the device had n CUs -- every wave /
                            workgroup of a persistent kernel then owns MANY work items even at test sizes (the steady state
                            of the slot rings and the vmcnt accounting, reached otherwise only at benchmark sizes) */
    const void* packed;  /* ABI v6, optional DEVICE pointer (null = none): the layer's packed low-rank factors, written earlier by
                            mtlora_linear_pack / mtlora_linear_pack_table from the SAME masters, scales, dropout_p and has_x_tasks.
                            fwd then skips its own packing launch and ctx only holds P; bwd must get the same pointer.  The masters
                            change once per optimizer step, so a trainer packs every layer in ONE launch per step instead of one
                            launch per layer and call. */
    int32_t hid;         /* ABI v8, 0 = none: role of this call inside an Mlp whose TASK hidden tensors stay implicit (MTLORA_HID_*, see
                            mtlora_mlp_hid_* below) */
    int32_t hid_pad_;
    const void* hid_ptr; /* ABI v8: MTLORA_HID_FWD_BASE: OUT (M x N), the pretrained product x W^T + b without any low-rank update;
                            MTLORA_HID_Q_GIVEN: IN (M x N), the summed output gradient G the dense part of dX is formed from (nullable) */
} mtlora_linear_desc;

/* d->hid flags (ABI v8) */
#define MTLORA_HID_FWD_BASE 1 /* fwd (the Mlp's fc1): writes y_s (+ a_s) and the base product to d->hid_ptr; NO task outputs (y_t / a_t are
                                 not touched) -- P (all segments) is written to ctx as usual */
#define MTLORA_HID_P_GIVEN 2  /* fwd (the Mlp's fc2): the TASK columns of P in ctx were written by mtlora_mlp_hid_proj before this call; the
                                 P pass runs for the shared source only, x_t is not read */
#define MTLORA_HID_Q_GIVEN 4  /* bwd (the Mlp's fc1): the TASK columns of Q (head of `scratch`) were written by mtlora_mlp_hid_bwd; dy_t is
                                 all-null, the dense part of dx comes from d->hid_ptr (G), dx_t / dA_t are formed from the given Q, dB_t
                                 must be null (mtlora_mlp_hid_bwd returns them) */

/* bytes of the context buffer written by fwd and read by bwd (packed low-rank factors + P; P alone when d->packed is set). */
int64_t mtlora_linear_ctx_bytes(const mtlora_linear_desc* d);

/* ---- packing the low-rank factors ahead of time (ABI v6).  fwd needs the fp32 masters A_* (r,K), B_* (N,r) of
 * models/lora.py:196-215 in the compute dtype and in several layouts (row-major, transposed, alpha-scaled projection rows,
 * fragment-major expansion factors): a small kernel per layer and call when done inside fwd.  The factors only change when the
 * optimizer steps, so a caller may keep one `packed` buffer per layer (mtlora_linear_packed_bytes) and refresh ALL of them with
 * one launch per step:
 *   mtlora_linear_pack            one layer, one launch (same arguments as fwd takes);
 *   mtlora_linear_pack_entry      writes one entry (mtlora_linear_pack_entry_bytes) of a HOST table describing a layer: master
 *                                 pointers, scales, geometry, destination; the caller copies the table to the device once (the
 *                                 pointers stay valid while parameters are updated in place);
 *   mtlora_linear_pack_table      ONE launch that packs every layer of a DEVICE table (entries of one dtype).
 * d->M is ignored by all of them; d->dropout_p / has_x_tasks / scales enter the alpha-scaled copies (train and eval differ). */
int64_t mtlora_linear_packed_bytes(const mtlora_linear_desc* d);
int mtlora_linear_pack(const mtlora_linear_desc* d, const float* A_s, const float* B_s, const float* const* A_t,
                       const float* const* B_t, void* packed, int64_t packed_bytes, void* stream);
int64_t mtlora_linear_pack_entry_bytes(void);
int mtlora_linear_pack_entry(const mtlora_linear_desc* d, const float* A_s, const float* B_s, const float* const* A_t,
                             const float* const* B_t, void* packed, int64_t packed_bytes, void* entry_host);
int mtlora_linear_pack_table(const void* table_dev, int n_entries, int dtype, void* stream);

/* ---- scales that live on the device (TRAINABLE_SCALE_SHARED / TRAINABLE_SCALE_PER_TASK of the reference, config.py:307-326,
 * lora.py:203-228: 1-element fp32 Parameters an optimizer moves every step).  Additive entries of ABI 12; the descriptor is
 * unchanged.  The scales reach the kernels through the packed factors alone (the alpha row and the alpha-scaled projection rows),
 * so a layer with such scales always runs with d->packed set, and the pack launch reads the scales when it RUNS: no host read of
 * a Parameter, and a captured graph that contains the pack launch follows the Parameter on every replay.
 *   scale_dev   HOST array of n_scale = 1 + d->T DEVICE pointers: [0] the shared scale, [1 + t] the scale of task t.  A null slot
 *               means "constant": that segment takes d->scale_s / d->scale_t[t] as the by-value entries do.  A set slot makes
 *               the kernel form  alpha = *scale_dev[o] * f  in fp32, f being the factor the host multiplies into a by-value
 *               scale (1 / (1 - dropout_p) for the shared segment and for task segments without x_tasks, 1 for task segments
 *               with x_tasks): a device scale holding the float s packs bit for bit what scale = s packs by value.
 *   mtlora_linear_pack_dev         mtlora_linear_pack with device scales;
 *   mtlora_linear_pack_entry_dev   mtlora_linear_pack_entry with device scales: one mtlora_linear_pack_table launch serves entries of
 *                                  both kinds (mtlora_linear_pack_entry_bytes is the size of either).
 * Rejected before any launch, after everything the by-value entry rejects: a null `scale_dev` array (MTLORA_ERR_NULL), n_scale !=
 * 1 + d->T (MTLORA_ERR_SHAPE), a scale pointer off 4 bytes (MTLORA_ERR_ALIGN).
 * d->scale_s / d->scale_t are read by the four packing entries and by a fwd that packs for itself (d->packed null), nowhere else: a
 * call with d->packed set never reads them (a host on this path fills them with 1.0). */
int mtlora_linear_pack_dev(const mtlora_linear_desc* d, const float* A_s, const float* B_s, const float* const* A_t,
                           const float* const* B_t, const float* const* scale_dev, int n_scale, void* packed, int64_t packed_bytes,
                           void* stream);
int mtlora_linear_pack_entry_dev(const mtlora_linear_desc* d, const float* A_s, const float* B_s, const float* const* A_t,
                                 const float* const* B_t, const float* const* scale_dev, int n_scale, void* packed,
                                 int64_t packed_bytes, void* entry_host);
/* d(loss)/d(scale) of the device scales of one layer in one call: d_scale[o] = <dB[o], B[o]> / *scale_dev[o] for o < n_scale =
 * 1 + d->T (segment order as scale_dev), dB[o] the fp32 factor gradient (N, r_o) mtlora_linear_bwd has just written on the same
 * stream, B[o] the fp32 master.  A segment whose scale_dev[o] or dB[o] is null (or whose rank is 0) is skipped: its d_scale word
 * is not written.  *scale_dev[o] == 0 writes 0.  Reduction in a fixed order (per-workgroup fp32 partials in `scratch`, summed in
 * double by a finishing launch behind it; no atomics): the same bits on every run.  d->M is ignored.  `d_scale`: 1 + d->T floats.
 * Rejected before any launch: a null dB / B / d_scale / scratch / scale_dev array or a null B[o] of a live segment
 * (MTLORA_ERR_NULL), n_scale != 1 + d->T (MTLORA_ERR_SHAPE), a pointer off 4 bytes (MTLORA_ERR_ALIGN), scratch_bytes below
 * mtlora_linear_scale_grad_scratch_bytes (MTLORA_ERR_WORKSPACE). */
int64_t mtlora_linear_scale_grad_scratch_bytes(void);
int mtlora_linear_scale_grad(const mtlora_linear_desc* d, const float* const* dB, const float* const* B,
                             const float* const* scale_dev, int n_scale, float* d_scale, void* scratch, int64_t scratch_bytes,
                             void* stream);
/* bytes of the backward scratch buffer. */
int64_t mtlora_linear_bwd_scratch_bytes(const mtlora_linear_desc* d);

int mtlora_linear_fwd(const mtlora_linear_desc* d, const void* x, const void* const* x_t, const void* W,
                      const float* bias, const float* A_s, const float* B_s, const float* const* A_t,
                      const float* const* B_t, void* y_s, void* const* y_t, void* ctx, int64_t ctx_bytes,
                      void* stream);

/* dy_s / dy_t[t] may be NULL (that output received no gradient).  dx_t is only written when
 * has_x_tasks; dA_x / dB_x may be NULL to skip a factor whose output got no gradient. */
int mtlora_linear_bwd(const mtlora_linear_desc* d, const void* x, const void* const* x_t, const void* Wt,
                      const void* dy_s, const void* const* dy_t, const void* ctx, int64_t ctx_bytes, void* dx,
                      void* const* dx_t, float* dA_s, float* dB_s, float* const* dA_t, float* const* dB_t,
                      void* scratch, int64_t scratch_bytes, void* stream);

/* mtlora_linear_fwd that ALSO writes a_s = gelu(y_s), a_t[t] = gelu(y_t[t]) (exact erf form; same shape / dtype as the
 * outputs) from the output epilogue -- the Mlp's fc1 followed by its activation (swin_transformer_mtlora.py:57-78):
 * replaces the separate aten::gelu pass (read h, write a) by one extra write. */
int mtlora_linear_fwd_gelu(const mtlora_linear_desc* d, const void* x, const void* const* x_t, const void* W,
                           const float* bias, const float* A_s, const float* B_s, const float* const* A_t,
                           const float* const* B_t, void* y_s, void* const* y_t, void* a_s, void* const* a_t, void* ctx,
                           int64_t ctx_bytes, void* stream);

/* mtlora_linear_bwd for a layer whose inputs are x = gelu(h_s), x_t[t] = gelu(h_t[t]) (the Mlp's fc2,
 * swin_transformer_mtlora.py:57-78: fc1 -> GELU -> fc2): dx and dx_t[t] are additionally multiplied by the exact-erf
 * GELU derivative gelu'(h) = Phi(h) + h phi(h) at the pre-activations (M x K, dtype of x), i.e. they are the gradients
 * w.r.t. h -- autograd's separate GeluBackward pass (read dX, read h, write dH) is folded into the dX epilogue.
 * h_t[t] is required wherever dx_t[t] is written. */
int mtlora_linear_bwd_gelu(const mtlora_linear_desc* d, const void* x, const void* const* x_t, const void* Wt,
                           const void* dy_s, const void* const* dy_t, const void* ctx, int64_t ctx_bytes, void* dx,
                           void* const* dx_t, float* dA_s, float* dB_s, float* const* dA_t, float* const* dB_t,
                           void* scratch, int64_t scratch_bytes, const void* h_s, const void* const* h_t, void* stream);

/* ------------------------------------------------------------------------------------------
 * Task-enabled Mlp with IMPLICIT task hidden tensors (ABI v8) -- replaces, for the T task streams of
 * `Mlp.forward` called with x_tasks (models/swin_transformer_mtlora.py:57-78: fc1 -> GELU -> fc2, both
 * MTLoRALinear with tasks, lora.py:262-266), the 3 T tensors of M x 4C elements the per-layer path writes
 * and re-reads (h_t = fc1 task outputs, gelu(h_t), and the gradients dH_t):
 *     h_t = h_base + P1_t B1_t^T   (h_base = x W1^T + b1, P1_t = s_t x_t A1_t^T: M x r_t)
 * enters fc2 ONLY through P2_t = s_t gelu(h_t) A2_t^T (M x r_t), and dH_t = (Q2_t A2_t) .* gelu'(h_t) is
 * consumed by G = dH_s + sum_t dH_t, Q1_t = s_t dH_t B1_t and the factor gradients dB1_t = dH_t^T P1_t,
 * dA2_t = Q2_t^T gelu(h_t).  Call sequence (d1 / d2 = descriptors of fc1 / fc2, same M, d1->N == d2->K):
 *   forward : mtlora_linear_fwd_gelu(d1 | HID_FWD_BASE) ; mtlora_mlp_hid_proj ; mtlora_linear_fwd(d2 | HID_P_GIVEN)
 *   backward: mtlora_linear_bwd_gelu(d2, dx_t = dA_t = null) ; mtlora_mlp_hid_bwd ; mtlora_linear_bwd(d1 | HID_Q_GIVEN)
 * Supported: 16-bit dtype, mode 'matrix', has_x_tasks, 1 <= T, every r_t <= 8, d1->N a multiple of 128; d1->N > 2048 only with
 * r_t <= 4 (the chunked MFMA kernels; mtlora_mlp_hid_supported returns 1).  Deterministic
 * (fixed-order partial sums).
 * ------------------------------------------------------------------------------------------ */
int mtlora_mlp_hid_supported(const mtlora_linear_desc* d1, const mtlora_linear_desc* d2);
/* bytes of the scratch buffers of mtlora_mlp_hid_proj / mtlora_mlp_hid_bwd (-1: unsupported shape) */
int64_t mtlora_mlp_hid_fwd_scratch_bytes(const mtlora_linear_desc* d1, const mtlora_linear_desc* d2);
int64_t mtlora_mlp_hid_bwd_scratch_bytes(const mtlora_linear_desc* d1, const mtlora_linear_desc* d2);
/* ctx1: fc1's context (P1; and the packed factors when d1->packed is null); ctx2: fc2's context, whose task columns of P are written;
 * d2->packed must be set (mtlora_linear_pack / _pack_table before the call). */
int mtlora_mlp_hid_proj(const mtlora_linear_desc* d1, const mtlora_linear_desc* d2, const void* h_base, const void* ctx1,
                        void* ctx2, void* scratch, int64_t scratch_bytes, void* stream);
/* dh_s: gradient w.r.t. the shared pre-activation (dx of fc2's bwd_gelu); scratch2: fc2's backward scratch after its phase 1 (holds
 * Q2); scratch1: fc1's backward scratch (its Q task columns are written); g: OUT (M x H) = dh_s + sum_t dH_t; dB1_t[t] (H x r_t) /
 * dA2_t[t] (r_t x H): fp32 OUT, nullable. */
int mtlora_mlp_hid_bwd(const mtlora_linear_desc* d1, const mtlora_linear_desc* d2, const void* h_base, const void* dh_s,
                       const void* ctx1, const void* ctx2, const void* scratch2, void* scratch1, void* g, float* const* dB1_t,
                       float* const* dA2_t, void* part, int64_t part_bytes, void* stream);

/* Weight gradient of a plain linear layer with a NARROW output (the decoder heads' final 1x1 convolutions,
 * models/seg_hrnet.py:518-526: nn.Conv2d(1080, num_classes, 1) on B*H*W pixels; autograd's dW = dY^T X):
 *   out (Na x Nb, fp32, row-major) = a^T b,  a = (M x Na, row stride lda), b = (M x Nb, row stride ldb).
 * Na, Nb, lda, ldb multiples of 8 (bf16) / 4 (f32); Na <= 1024.  Deterministic (fixed-order split-M partials). */
int64_t mtlora_gemm_tn_scratch_bytes(int64_t M, int Na, int Nb);
int mtlora_gemm_tn(const void* a, const void* b, float* out, int64_t M, int Na, int Nb, int64_t lda, int64_t ldb,
                   int dtype, void* scratch, int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Window attention core -- replaces swin_transformer_mtlora.py:194-220 (q*scale, q@k^T, + relative
 * position bias, + shift mask, softmax, @v, head merge) and, with image_layout = 1, also the
 * cyclic shift + window partition before it and the window merge + reverse shift after it
 * (:336-350, :365-377), by folding them into the kernel's load/store addressing.
 *
 * qkv: `dtype`, last dim laid out [3][num_heads][head_dim] (the reshape at :194-197).
 *   image_layout = 0: qkv is (n_windows, N, 3C) window-major exactly as the reference module sees it;
 *   image_layout = 1: qkv is (B, H, W, 3C) in natural token order; window w of image b covers
 *                     rows/cols ((wy*ws+ty+shift) mod H, (wx*ws+tx+shift) mod W).
 * out has the same token order as qkv, (.., C).  bias: dense (num_heads, N, N) fp32
 * (table[index] gathered by the host, :202-206).  mask: (nW_per_image, N, N) fp32 or NULL (:209-213).
 * N = ws*ws <= 144 (window sizes up to 12; N <= 64 runs one wave per (window, head), larger windows one workgroup),
 * head_dim == 32 (every Swin variant).  Larger windows return MTLORA_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------ */
typedef struct mtlora_attn_desc {
    int64_t B;            /* images */
    int32_t H, W;         /* token map */
    int32_t window_size;
    int32_t shift;        /* >= 0; only used for addressing when image_layout = 1 */
    int32_t num_heads;
    int32_t head_dim;
    int32_t image_layout;
    int32_t dtype;
    float scale;
    float mask_value;     /* value added where mask_ids differ (Swin: -100) */
} mtlora_attn_desc;

int64_t mtlora_window_attn_bwd_scratch_bytes(const mtlora_attn_desc* d);

/* bias: dense (num_heads, N, N) fp32, [h][i][j] added to score(query i, key j).  The shift mask can be given
 * either as region ids -- mask_ids (nW_per_image, N) int32: mask(i,j) = ids differ ? d->mask_value : 0, which is how
 * SW-MSA builds it (swin_transformer_mtlora.py:297-323); the fast path -- or as a general dense `mask`
 * (nW_per_image, N, N) fp32; both NULL = no mask.  When mask_ids is given, `mask` is ignored. */
int mtlora_window_attn_fwd(const mtlora_attn_desc* d, const void* qkv, const float* bias, const float* mask,
                           const int32_t* mask_ids, void* out, void* stream);
/* dbias: (num_heads, N, N) fp32 [h][i][j], overwritten.  dqkv: same shape/dtype as qkv, fully written. */
int mtlora_window_attn_bwd(const mtlora_attn_desc* d, const void* qkv, const float* bias, const float* mask,
                           const int32_t* mask_ids, const void* dout, void* dqkv, float* dbias, void* scratch,
                           int64_t scratch_bytes, void* stream);

/* Attention dropout (swin_transformer_mtlora.py:216, `attn_drop` on the softmax output):  P' = keep . P / (1 - p),  out = P' V.
 * The keep bits are generated inside the kernels, forward and backward alike; no mask is stored.  Element (window w, head h,
 * query i, key j) is the counter-based generator of the linear layers' dropout (oracle: dropout_keep_mask) with
 *     row m = (w * num_heads + h) * N + i,   column k = j,   stream 0x41  (the linear layers use stream 0)
 * where w counts windows as the reference's (B_, nH, N, N) attention tensor does (image, window row, window column) and i, j are
 * tokens of the window after the cyclic shift -- so both layouts draw the same mask.  keep <=> bits >= floor(p * 65536); a p below
 * 2^-16 is off.  seed_offset: optional DEVICE word added to `seed` when the kernels run (as mtlora_linear_desc.seed_offset: a
 * replayed graph draws fresh masks).  The backward must be given the forward's seed (and the same offset value).
 * Arguments, scratch size (mtlora_window_attn_bwd_scratch_bytes) and statuses as the plain entry points; in addition a NULL
 * dropout struct is MTLORA_ERR_NULL, a p outside [0, 1) or not finite MTLORA_ERR_SHAPE, and so is n_windows * num_heads * N >= 2^32
 * (the row index is 32 bits).  p == 0 runs the plain kernels. */
typedef struct mtlora_attn_dropout {
    float p;
    uint64_t seed;
    const uint64_t* seed_offset;
} mtlora_attn_dropout;
int mtlora_window_attn_drop_fwd(const mtlora_attn_desc* d, const mtlora_attn_dropout* drop, const void* qkv, const float* bias,
                                const float* mask, const int32_t* mask_ids, void* out, void* stream);
int mtlora_window_attn_drop_bwd(const mtlora_attn_desc* d, const mtlora_attn_dropout* drop, const void* qkv, const float* bias,
                                const float* mask, const int32_t* mask_ids, const void* dout, void* dqkv, float* dbias, void* scratch,
                                int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * LayerNorm over the last dim (block glue around the path: norm1 / norm2 / PatchMerging.norm,
 * swin_transformer_mtlora.py:331-333, 395-396, 469) -- replaces aten::native_layer_norm + the autocast cast:
 * reads x (fp32 or bf16) once and writes y directly in the dtype the following linear consumes; fp32 statistics
 * (mean, rstd: (M) fp32) are saved for backward.  bwd also writes dgamma / dbeta (C) fp32 (overwritten).
 * merge_h, merge_w (0, 0 = off): PatchMerging (swin_transformer_mtlora.py:429-481) in front of its LayerNorm: x (and dx,
 * dx_addend) are the (B, merge_h*merge_w, C/4) token tensor and row (b, y2, x2) of the normalised (M, C) matrix is the
 * 2x2 neighbourhood [x(2y2,2x2) | x(2y2+1,2x2) | x(2y2,2x2+1) | x(2y2+1,2x2+1)] gathered on the fly (backward scatters).
 * dx_addend (nullable, dtype and shape of x): dx = dx_addend + LN-backward(dy).  In a transformer block x feeds the
 * LayerNorm AND the skip connection; passing the skip path's gradient here replaces the framework's separate
 * full-size gradient add.
 * ------------------------------------------------------------------------------------------ */
int mtlora_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                         int64_t M, int64_t C, float eps, int x_dtype, int y_dtype, int merge_h, int merge_w, void* stream);
int64_t mtlora_layernorm_bwd_scratch_bytes(int64_t M, int64_t C, int x_dtype);
int mtlora_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                         void* dx, float* dgamma, float* dbeta, int64_t M, int64_t C, int x_dtype, int dy_dtype,
                         void* scratch, int64_t scratch_bytes, const void* dx_addend, int merge_h, int merge_w, void* stream);

/* Residual + DropPath fused with the LayerNorm that follows it (swin_transformer_mtlora.py:389-396: x = shortcut +
 * drop_path(attn(..)); then norm2(x); and :398-408 followed by the next block's norm1):
 *   fwd: x_new = shortcut + scale[sample] * branch  (written, dtype of shortcut = x_dtype);  y = LayerNorm(x_new) (y_dtype)
 *        branch has y_dtype; scale: (B) fp32 DropPath mask / keep, or NULL (= 1); rows M = B * tokens.
 *   bwd: d_shortcut = dx_addend + LN-backward(dy) (x_dtype);  d_branch = scale[sample] * d_shortcut (dy_dtype)
 * -- one pass each instead of residual kernel + LayerNorm kernel (saves re-reading the fp32 residual stream). */
int mtlora_residual_layernorm_fwd(const void* shortcut, const void* branch, const float* scale, int64_t B, const float* gamma,
                                  const float* beta, void* x_new, void* y, float* mean, float* rstd, int64_t M, int64_t C,
                                  float eps, int x_dtype, int y_dtype, void* stream);
int mtlora_residual_layernorm_bwd(const void* dy, const void* x_new, const float* gamma, const float* mean, const float* rstd,
                                  void* d_shortcut, void* d_branch, float* dgamma, float* dbeta, const float* scale,
                                  int64_t B, int64_t M, int64_t C, int x_dtype, int dy_dtype, void* scratch,
                                  int64_t scratch_bytes, const void* dx_addend, void* stream);

/* n independent inputs through the SAME LayerNorm, one launch each way (PatchMerging.norm applied to the shared tensor and to
 * every task tensor, swin_transformer_mtlora.py:543-551); y[k] may be slices of one stacked buffer; dgamma / dbeta are summed
 * over the inputs; dx_addend (array, nullable entries) as in mtlora_layernorm_bwd. */
int64_t mtlora_layernorm_multi_bwd_scratch_bytes(int n, int64_t M, int64_t C, int x_dtype);
int mtlora_layernorm_multi_fwd(int n, const void* const* x, const float* gamma, const float* beta, void* const* y,
                               float* const* mean, float* const* rstd, int64_t M, int64_t C, float eps, int x_dtype, int y_dtype,
                               int merge_h, int merge_w, void* stream);
int mtlora_layernorm_multi_bwd(int n, const void* const* dy, const void* const* x, const float* gamma, const float* const* mean,
                               const float* const* rstd, void* const* dx, float* dgamma, float* dbeta, int64_t M, int64_t C,
                               int x_dtype, int dy_dtype, void* scratch, int64_t scratch_bytes, const void* const* dx_addend,
                               int merge_h, int merge_w, void* stream);

/* n independent streams, each  x_new[k] = res[k] + scale[k][sample] * branch[k]  followed by the SAME LayerNorm (plain rows, or
 * the PatchMerging gather with merge_h / merge_w): the MLP residual of the task-enabled block (swin_transformer_mtlora.py:398-408)
 * fused with the stage's PatchMerging norm over the shared + task tensors (:543-551).  res / branch / x_new / d_res / d_branch are
 * token tensors in the layout of x; y[k] may be slices of one stacked buffer.  Backward: d_res[k] = dx_addend[k] + LN-backward,
 * d_branch[k] = scale[k] * d_res[k], dgamma / dbeta summed over the streams (scratch: mtlora_layernorm_multi_bwd_scratch_bytes). */
int mtlora_residual_layernorm_streams_fwd(int n, const void* const* res, const void* const* branch, const float* scale,
                                          int64_t B, const float* gamma, const float* beta, void* const* x_new, void* const* y,
                                          float* const* mean, float* const* rstd, int64_t M, int64_t C, float eps, int x_dtype,
                                          int y_dtype, int merge_h, int merge_w, void* stream);
int mtlora_residual_layernorm_streams_bwd(int n, const void* const* dy, const void* const* x_new, const float* gamma,
                                          const float* const* mean, const float* const* rstd, void* const* d_res,
                                          void* const* d_branch, float* dgamma, float* dbeta, const float* scale, int64_t B,
                                          int64_t M, int64_t C, int x_dtype, int dy_dtype, void* scratch, int64_t scratch_bytes,
                                          const void* const* dx_addend, int merge_h, int merge_w, void* stream);

/* The same for the task-enabled block (swin_transformer_mtlora.py:389-396 for the shared stream and each task stream): ONE
 * shortcut, n branches -> x_new[k] = shortcut + scale[k][sample] * branch[k], y[k] = LayerNorm(x_new[k]) (one launch), and
 * backward: d_branch[k] = scale[k] * (dx_addend[k] + LN-backward(dy[k])), d_shortcut = sum_k (dx_addend[k] + LN-backward(dy[k])),
 * dgamma / dbeta summed over the streams (one launch + reduce instead of n LayerNorm backwards and a residual backward).
 * scale: (n, B) fp32 or NULL; dx_addend[k], d_branch[k] nullable. */
int mtlora_residual_layernorm_multi_fwd(int n, const void* shortcut, const void* const* branch, const float* scale, int64_t B,
                                        const float* gamma, const float* beta, void* const* x_new, void* const* y,
                                        float* const* mean, float* const* rstd, int64_t M, int64_t C, float eps, int x_dtype,
                                        int y_dtype, void* stream);
int mtlora_residual_layernorm_multi_bwd(int n, const void* const* dy, const void* const* x_new, const float* gamma,
                                        const float* const* mean, const float* const* rstd, const void* const* dx_addend,
                                        void* d_shortcut, void* const* d_branch, float* dgamma, float* dbeta, const float* scale,
                                        int64_t B, int64_t M, int64_t C, int x_dtype, int dy_dtype, void* scratch,
                                        int64_t scratch_bytes, void* stream);

/* SHARED_MODE "addition" (reference lora.py:275-284): the LayerNorm of the SUM of the n task outputs of a linear layer, added to
 * its pretrained output, one launch:
 *   tot = sum_k y_t[k]  (fp32, in index order; never stored);  out = y + gamma (tot - mean) rstd + beta,  rounded to `dtype` once.
 * y_t[k], y, out: (M, N) of `dtype` (fp32 / bf16 / fp16), contiguous, 16-byte aligned; out may be y.  mean / rstd: (M) fp32, saved
 * for the backward.  n in 1 .. MTLORA_MAX_TASKS; N a multiple of 8 (16-bit) or 4 (fp32), up to 4096; M >= 0, and M == 0 returns
 * MTLORA_OK without a launch and without looking at the pointers.  A non-finite value in a row of any y_t makes that row of out non-finite and no other. */
int mtlora_sum_ln_add_fwd(int n, const void* const* y_t, const void* y, const float* gamma, const float* beta,
                                 void* out, float* mean, float* rstd, int64_t M, int64_t N, float eps, int dtype, void* stream);
/* Backward of mtlora_sum_ln_add_fwd (reference lora.py:275-284).  The gradient of y is dout itself: the caller passes it
 * through, nothing is written for it.  d_tot = LayerNorm-backward(dout) with tot formed again from y_t, and
 *   dy_t[k] = dy_t_addend[k] + d_tot
 * where dy_t_addend[k] (the array or any entry may be NULL) is the gradient that reached y_t[k] from downstream, as dx_addend of
 * mtlora_layernorm_bwd; dy_t[k] may be its addend.  dgamma / dbeta: (N) fp32, overwritten, deterministic (per-workgroup partials
 * in `scratch`, summed in a fixed order: no atomics, no memset); M == 0 zero-fills them; both NULL (a frozen norm): not computed.  scratch: at least
 * mtlora_sum_ln_add_bwd_scratch_bytes (-1: arguments outside the limits above). */
int64_t mtlora_sum_ln_add_bwd_scratch_bytes(int n, int64_t M, int64_t N, int dtype);
int mtlora_sum_ln_add_bwd(int n, const void* dout, const void* const* y_t, const float* gamma, const float* mean,
                                 const float* rstd, const void* const* dy_t_addend, void* const* dy_t, float* dgamma,
                                 float* dbeta, int64_t M, int64_t N, int dtype, void* scratch, int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training-mode BatchNorm + optional ReLU over a channels-last (R rows, C channels) matrix -- the decoder heads'
 * conv1x1 -> BatchNorm2d -> ReLU (seg_hrnet.py:498-526) on the (pixels, channels) matrix; replaces
 * aten::native_batch_norm(+backward) and the separate ReLU.  Biased variance for normalisation, unbiased for the
 * running_var update (momentum as nn.BatchNorm2d); running_* may be NULL.  save_* are (C) fp32 buffers written by
 * fwd and read by bwd (x is re-read by bwd; y is not needed).  dgamma / dbeta (C) fp32 are overwritten.
 * ------------------------------------------------------------------------------------------ */
int64_t mtlora_bn_scratch_bytes(int64_t R, int64_t C, int dtype);
int mtlora_bn_relu_fwd(const void* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                       float momentum, float eps, int relu, void* y, float* save_mean, float* save_rstd,
                       float* save_scale, float* save_shift, int64_t R, int64_t C, int dtype, void* scratch,
                       int64_t scratch_bytes, void* stream);
int mtlora_bn_relu_bwd(const void* dy, const void* x, const float* save_mean, const float* save_rstd,
                       const float* save_scale, const float* save_shift, int relu, void* dx, float* dgamma, float* dbeta,
                       int64_t R, int64_t C, int dtype, void* scratch, int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * residual + DropPath for the n = 1+T tensors of a block half (swin_transformer_mtlora.py:389-392, 398-408):
 *   out_k = res_k + scale[k][sample] * y_k      (scale = DropPath mask / keep_prob, (n, B) fp32, NULL = ones)
 * (M, C) row-major, M = B * tokens, C % 8 == 0; res / out in res_dtype, y in y_dtype.  Backward: dy_k = scale * g_k
 * (y_dtype) and, when the residual is shared by every k, dres = sum_k g_k (res_dtype); g[k] may be NULL.
 * ------------------------------------------------------------------------------------------ */
int mtlora_residual_droppath_fwd(int n, const void* const* res, const void* const* y, void* const* out,
                                 const float* scale, int64_t M, int64_t C, int64_t B, int res_dtype, int y_dtype,
                                 void* stream);
int mtlora_residual_droppath_bwd(int n, const void* const* g, void* const* dy, void* dres, const float* scale,
                                 int64_t M, int64_t C, int64_t B, int res_dtype, int y_dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Activation dropout (MODEL.DROP_RATE: Mlp.drop on the hidden tensors and on fc2's outputs, WindowAttention.proj_drop, pos_drop;
 * swin_transformer_mtlora.py:172-178, :274-279, :739) generated inside the kernels that consume the activation.  No mask is stored:
 * forward and backward regenerate the keep bits from the counter-based generator of the linear layers' dropout (oracle:
 * dropout_keep_mask).  Element (row m, channel c) of tensor k of a call uses
 *     row m (of the (M, C) row-major matrix),   column c,   stream  site + 0x100 * k
 * with site = 0x42 hidden, 0x43 projection, 0x44 Mlp output, 0x45 position, and k = 0 for the shared tensor, 1 + i for task i: every
 * tensor of a call has an independent mask.  keep <=> bits >= floor(p * 65536), kept values are scaled by 1 / (1 - p), a p below
 * 2^-16 is off.  The dropout argument is a mtlora_attn_dropout {p, seed, seed_offset}; seed_offset as there (a replayed graph draws
 * fresh masks); the backward must be given the forward's seed, site and offset value.
 *
 *   mtlora_act_dropout_fwd:  a[k]  = keep[k] . act(h[k]) / (1 - p)                      act: 0 identity, 1 exact (erf) GELU
 *   mtlora_act_dropout_bwd:  dh[k] = g[k] . keep[k] / (1 - p) . act'(h[k])              (h is not read, and may be NULL, for act 0)
 *   mtlora_residual_droppath_drop_fwd:  out[k] = res[k] + scale[k][sample] * keep[k] / (1 - p) * y[k]
 *   mtlora_residual_droppath_drop_bwd:  dy[k]  = scale[k][sample] * keep[k] / (1 - p) * g[k];  dres = sum_k g[k]
 * n <= 1 + MTLORA_MAX_TASKS tensors of (M, C), C % 8 == 0, one launch; fp32 / bf16 / fp16 (the residual pair as the plain entries);
 * products in fp32, rounded once.  The residual forms take the arguments of the plain entries (the dropped branch is never written);
 * p == 0 there runs the plain kernels.  Statuses, in the order they are checked: dtype; n (and act) out of range SHAPE; a NULL
 * pointer or dropout argument NULL; a tensor not 16-byte aligned ALIGN; C % 8, M % B, p outside [0, 1) or not finite, M >= 2^32
 * (the row index is 32 bits) SHAPE.  M == 0 returns OK without a launch.
 * ------------------------------------------------------------------------------------------ */
int mtlora_act_dropout_fwd(int n, const void* const* h, void* const* a, const mtlora_attn_dropout* drop, int site, int act,
                           int64_t M, int64_t C, int dtype, void* stream);
int mtlora_act_dropout_bwd(int n, const void* const* g, const void* const* h, void* const* dh, const mtlora_attn_dropout* drop,
                           int site, int act, int64_t M, int64_t C, int dtype, void* stream);
int mtlora_residual_droppath_drop_fwd(int n, const void* const* res, const void* const* y, void* const* out, const float* scale,
                                      const mtlora_attn_dropout* drop, int site, int64_t M, int64_t C, int64_t B, int res_dtype,
                                      int y_dtype, void* stream);
int mtlora_residual_droppath_drop_bwd(int n, const void* const* g, void* const* dy, void* dres, const float* scale,
                                      const mtlora_attn_dropout* drop, int site, int64_t M, int64_t C, int64_t B, int res_dtype,
                                      int y_dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Loss end of the train step, fused (callers): replaces the final
 * F.interpolate(pred, img_size, mode="bilinear") of models/swin_mtl.py:245 TOGETHER WITH the per-task loss of
 * mtl_loss_schemes.py and their autograd backward.
 *   kind 0  SoftMaxwithLoss (:22-39): cross entropy over C classes, ignore_index, mean over valid pixels;
 *           label (B,1,H,W) float class ids; stat[0] = number of valid pixels
 *   kind 1  NormalsLoss(normalize=True, L1, size_average) (:162-220): label (B,C,H,W), C <= 4;
 *           stat[0] = sum of the validity mask (label != ignore_index)
 *   kind 2  BalancedCrossEntropyLoss(size_average) (:42-89): C = 1, label (B,1,H,W);
 *           stat[0] = w = mean(1 - (label >= 0.5)), or the constant pos_weight (edge: 0.95, :243-245)
 *   kind 3  DepthLoss('l1') (:132-148): C = 1, label (B,1,H,W), |up - label| over label != ignore_index, mean over the
 *           valid pixels; stat[0] = number of valid pixels
 * low (B,h,w,C) is the channels-last low-resolution prediction, H = scale*h, W = scale*w (integer scale 1..32,
 * align_corners=False; larger scales: MTLORA_ERR_UNSUPPORTED / a negative count).  Writes dlow = d loss / d low (dtype of
 * low) and `mtlora_upsample_loss_partials(B, h, w, scale)` fp32 partial loss values (one per tile of the launch) whose sum
 * is the loss.  `stat` is a device pointer (label-only statistics).  Deterministic: no float atomics.
 * ------------------------------------------------------------------------------------------ */
int64_t mtlora_upsample_loss_partials(int64_t B, int h, int w, int scale);
int mtlora_upsample_loss(int kind, const void* low, const float* label, const float* stat, void* dlow, float* partials,
                         int64_t B, int h, int w, int C, int scale, int dtype, float ignore_index, void* stream);

/* ------------------------------------------------------------------------------------------
 * Partially labelled batches (additive under ABI 12): the same launch with a per-sample validity flag.  `valid` is a device
 * array of B bytes, non-zero = sample b carries a label for this task; V = the labelled samples.  The loss is the criterion
 * above applied to the sub-batch (up[V], label[V]):
 *   stat[0]  the statistic of mtlora_upsample_loss over the samples of V only (kind 2 with a constant weight: pos_weight)
 *   stat[1]  |V| as a float -- kind 2 normalises by |V| H W; both words are what mtlora_label_stat_valid writes
 * A tile of an unlabelled sample writes +0.0 to the elements of dlow it owns and 0 to its partial before it loads anything:
 * neither low[b] nor label[b] of such a sample is read (any bits, NaN and Inf included, may stand there), every element of
 * dlow is still written exactly once and the partial count is mtlora_upsample_loss_partials as before.  With V empty the
 * partials sum to +0.0 and dlow is all zero bytes.  With every sample labelled, loss partials and dlow have the bits of
 * mtlora_upsample_loss fed by mtlora_label_stat.  `valid` is read by the kernel, at launch or replay time: a captured launch
 * follows the buffer's content.  Checks and return codes as mtlora_upsample_loss; valid == NULL with B > 0 is
 * MTLORA_ERR_NULL.
 * ------------------------------------------------------------------------------------------ */
int mtlora_upsample_loss_valid(int kind, const void* low, const float* label, const unsigned char* valid, const float* stat,
                               void* dlow, float* partials, int64_t B, int h, int w, int C, int scale, int dtype,
                               float ignore_index, void* stream);

/* ------------------------------------------------------------------------------------------
 * Validation end of an epoch, fused (ABI v9): replaces, for one task and one batch, the final
 * F.interpolate(pred, img_size, mode="bilinear") of models/swin_mtl.py:245 TOGETHER WITH get_output
 * (evaluation/evaluate_utils.py:20-38), the task's meter update and the task's loss of main.py:439-528 validate().
 * Forward only; the upsampled prediction never exists and nothing is copied to the host.
 *   kind 0  softmax (SemsegMeter eval_semseg.py:109-120, HumanPartsMeter eval_human_parts.py:96-106, SoftMaxwithLoss), C <= 48
 *           counts: tp[C], predicted[C], ground truth[C] among label != ignore_index (fp = predicted - tp, fn = gt - tp),
 *           then the valid count: 3 C + 1.  float quantities: loss.  stat[0] = number of valid pixels
 *   kind 1  normals (NormalsMeterV1 eval_normals_v1.py:29-54, NormalsMeterV2 eval_normals_v2.py:32-44, NormalsLoss), C <= 4
 *           counts: n_v1, #{deg < 11.25}, #{deg < 22.5}, #{deg < 30}, n_v2.  float quantities: loss, sum of V1 degrees, sum
 *           of V2 degrees.  stat[0] = sum of the validity mask
 *   kind 2  saliency (SaliencyMeterWithBeta eval_sal_beta.py:29-70, SaliencyMeterWithNoBeta eval_sal_no_beta.py:33-50 with
 *           jaccard.py, BalancedCrossEntropyLoss), C = 1.  stat[0] = w, stat[1..16) the 15 per-image thresholds,
 *           stat[16..35) the 19 global thresholds (the caller builds them the way the meters do, so they are the same floats)
 *           counts: [19][tp, predicted, actual] over label != ignore_index, then [B][15][tp, fp, fn] per image: 57 + 45 B.
 *           float quantities: loss
 *   kind 3  depth (DepthMeter eval_depth.py:71-89, DepthLoss), C = 1.  counts: valid.  float quantities: loss,
 *           sum (gt - p)^2, sum (log gt - log p)^2 with p = max(up, 1e-9).  stat[0] = number of valid pixels
 *   kind 4  edge (EdgeMeter eval_edge.py:31-37, BalancedCrossEntropyLoss(pos_weight)), C = 1.  no counts.  float quantities:
 *           loss, and the meter's value (the same loss applied to the PROCESSED prediction, as the reference does).
 *           stat[0] = pos_weight
 * low, label, scale, dtype, ignore_index as mtlora_upsample_loss.  `counts` (n_int64 values) is ADDED to with integer
 * atomics -- zero it, or hand in a meter's running state; `fpartials` receives n_float_partials fp32 values laid out
 * [quantity][tile] (n_float_partials / number of quantities per row), to be summed by the caller in a fixed order.
 * Deterministic: no float atomics.  mtlora_upsample_metrics_sizes reports both sizes (pure host call).
 * ------------------------------------------------------------------------------------------ */
int mtlora_upsample_metrics_sizes(int kind, int64_t B, int h, int w, int C, int scale, int64_t* n_int64,
                                  int64_t* n_float_partials);
int mtlora_upsample_metrics(int kind, const void* low, const float* label, const float* stat, int64_t* counts,
                            float* fpartials, int64_t B, int h, int w, int C, int scale, int dtype, float ignore_index,
                            void* stream);

/* ------------------------------------------------------------------------------------------
 * Partially labelled batches at the validation end (additive under ABI 12): the same launch with the per-sample validity flag
 * of mtlora_upsample_loss_valid.  `valid` is a device array of B bytes, non-zero = sample b carries a label for this task;
 * V = the labelled samples.  The result is what mtlora_upsample_metrics gives for the sub-batch (low[V], label[V]):
 *   stat[0]  the statistic of mtlora_upsample_metrics over the samples of V only -- what mtlora_label_stat_valid writes to
 *            out[0] (kind 4: pos_weight), so the loss is the sub-batch's criterion
 *   |V|      as a float (out[1] of mtlora_label_stat_valid), in the word behind those of the unmasked launch: stat[1] for kinds
 *            0, 1, 3 (not read) and 4, stat[35] for kind 2, whose thresholds keep stat[1..35).  Kinds 2 and 4 normalise the loss
 *            (kind 4: and the meter's value) by |V| H W
 * A tile belongs to one sample.  A tile of an unlabelled sample decides on its flag before it loads anything: it adds nothing
 * to `counts` (kind 2: that image's [15][3] rows stay as they were), writes +0.0 to its partial of every float quantity and
 * reads neither low[b] nor label[b] (any bits, NaN and Inf included, may stand there).  Every element of `fpartials` is still
 * written exactly once; sizes and layouts are those of mtlora_upsample_metrics_sizes for the whole batch B, image b of kind 2
 * keeps row b.  With V empty, `counts` is unchanged and every partial is +0.0.  With every sample labelled, `counts` and
 * `fpartials` have the bits of mtlora_upsample_metrics fed by mtlora_label_stat.  `valid` is read by the kernel, at launch or
 * replay time: a captured launch follows the buffer's content.  No float atomics, no memset.  Checks and return codes as
 * mtlora_upsample_metrics; valid == NULL with B > 0 is MTLORA_ERR_NULL.
 * ------------------------------------------------------------------------------------------ */
int mtlora_upsample_metrics_valid(int kind, const void* low, const float* label, const unsigned char* valid, const float* stat,
                                  int64_t* counts, float* fpartials, int64_t B, int h, int w, int C, int scale, int dtype,
                                  float ignore_index, void* stream);

/* ------------------------------------------------------------------------------------------
 * Full-resolution predictions, fused (ABI v11): replaces, for one task and one batch, the final
 * F.interpolate(pred, img_size, mode="bilinear") of models/swin_mtl.py:245 TOGETHER WITH get_output
 * (evaluation/evaluate_utils.py:20-38) -- what utils.py:405-439 save_imgs_mtl and any offline scoring (the edge benchmark)
 * take.  Forward only, no label; the upsampled logits never exist, only the processed prediction is written.
 *   kind 0  argmax (semseg, human_parts), C <= 48: out (B,H,W) MTLORA_U8, the index of the FIRST maximum (torch.max(dim)[1])
 *   kind 1  normals, C <= 4: out (B,H,W,C), (up / max(|up|, 1e-12) + 1) * 255 / 2 (F.normalize's form)
 *   kind 2  sigmoid (sal, edge), C = 1: out (B,H,W), 255 / (1 + exp(-up))
 *   kind 3  identity (depth), C = 1: out (B,H,W,1) MTLORA_F32, up
 * out_dtype of kinds 1 and 2: MTLORA_F32 (get_output's value) or MTLORA_U8 (the same fp32 value truncated, as
 * tensor.to(torch.uint8) converts a value in [0, 255]).  low (B,h,w,C) channels-last fp32 / bf16 / fp16, H = scale*h,
 * W = scale*w, integer scale 1..32, align_corners=False as mtlora_upsample_loss.  A C or scale out of range, an unknown kind
 * or a kind / out_dtype pair not listed: MTLORA_ERR_UNSUPPORTED before any launch.  `out` is contiguous and aligned to its
 * element; every element of it is written exactly once and nothing else is.  Deterministic; no atomics, no memset.
 * ------------------------------------------------------------------------------------------ */
int mtlora_upsample_predict(int kind, const void* low, void* out, int64_t B, int h, int w, int C, int scale, int dtype,
                            int out_dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Small deterministic reductions of the callers (two launches each: per-block partials, fixed-order combine; no atomics and
 * no hipMemsetAsync, unlike ATen's multi-block reduce_kernel -- see csrc/reduce.hip and tools/find_memsets.py).
 *   mtlora_colsum      out[n] = sum_m x[m][n]  (fp32 out; x (M x N) row-major fp32 / bf16, N a multiple of the 16-byte vector):
 *                      replaces `grad.sum(0)` for the bias gradient of the heads' 1x1 convolutions
 *                      (reference models/seg_hrnet.py:498-526 layers under torch autograd)
 *   mtlora_label_stat  label-only statistics of the fused losses (`stat` of mtlora_upsample_loss), n fp32 labels:
 *                      kind 0: number of elements != ignore_index   (mtl_loss_schemes.py:22-39, :162-220)
 *                      kind 1: mean(1 - (label >= 0.5))             (mtl_loss_schemes.py:42-89)
 * ------------------------------------------------------------------------------------------ */
int64_t mtlora_colsum_scratch_bytes(int64_t M, int64_t N);
int mtlora_colsum(const void* x, int64_t M, int64_t N, int dtype, float* out, void* scratch, int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Gradient of a trainable `linear.bias` of an MTLoRALinear whose W stays frozen (additive under ABI 12) -- MODEL.MTLORA.BIAS 'all':
 * mark_only_lora_as_trainable(model, bias='all'), reference lora.py:606-624, sets requires_grad on every `*.bias`.  All 1 + T
 * outputs of the layer add the same x W^T + b (lora.py:255-284, every shared mode), so
 *   db[n] = sum_m ( dy_s[m][n] + sum_t dy_t[t][m][n] )     over the d->M rows
 * dy_s, dy_t[t]: (M, N) row-major in d->dtype (fp32, bf16 or fp16), T = d->T; a NULL source is an output that got no gradient and
 * is skipped (dy_t itself may be NULL when T == 0); with every source NULL, or M == 0, db is written as zeros.  db (N) fp32.
 * Only M, N, dtype and T of the descriptor are read.  N a multiple of the 16-byte vector of d->dtype and <= 2^20, sources and
 * scratch 16-byte aligned.  fp32 accumulation; every gradient element is read once, as 16-byte vectors, and no (M, N) intermediate
 * exists.  Two launches on `stream` (the column walk of mtlora_colsum over all sources, then its fixed-order combine): no
 * atomics, no memset, db fully overwritten, the same bits on every call with the same inputs.
 * ------------------------------------------------------------------------------------------ */
int64_t mtlora_linear_bias_grad_scratch_bytes(const mtlora_linear_desc* d);
int mtlora_linear_bias_grad(const mtlora_linear_desc* d, const void* dy_s, const void* const* dy_t, float* db, void* scratch,
                            int64_t scratch_bytes, void* stream);
int64_t mtlora_label_stat_scratch_bytes(int64_t n);
int mtlora_label_stat(const float* label, int64_t n, int kind, float ignore_index, float* out, void* scratch,
                      int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * mtlora_label_stat over the labelled samples of a batch (additive under ABI 12; `stat` of mtlora_upsample_loss_valid).
 * label: B samples of n_per_sample fp32 values each, contiguous; valid: B device bytes, non-zero = labelled, NULL = all.
 *   out[0]  kind 0: number of elements != ignore_index among the labelled samples; kind 1: mean(1 - (label >= 0.5)) over
 *           them; kind 2: 0 -- only the count below is wanted (a constant pos_weight), `label` is not read and may be NULL.
 *           0 when no sample is labelled.  With valid == NULL or all non-zero: the bits of mtlora_label_stat(label, B * n_per_sample).
 *   out[1]  the number of labelled samples, as a float
 * Two launches (kind 2: the second only): per-sample, per-block counts, then a fixed-order combine that skips the partials
 * of unlabelled samples; the labels of an unlabelled sample are never read.  No atomics, no memset; `valid` is read on the
 * device.  out: 2 floats, 4-byte aligned.  MTLORA_ERR_UNSUPPORTED: kind outside 0..2; SHAPE: B <= 0, n_per_sample <= 0 or
 * >= 2^31, B >= 2^21; NULL: out, scratch, or label with kind != 2; ALIGN: label or scratch not 16-byte aligned; WORKSPACE:
 * scratch_bytes below mtlora_label_stat_valid_scratch_bytes(B, n_per_sample) (-1 for a shape the entry rejects).
 * ------------------------------------------------------------------------------------------ */
int64_t mtlora_label_stat_valid_scratch_bytes(int64_t B, int64_t n_per_sample);
int mtlora_label_stat_valid(const float* label, const unsigned char* valid, int64_t B, int64_t n_per_sample, int kind,
                            float ignore_index, float* out, void* scratch, int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Full fine-tuning (additive under ABI 12) -- MODEL.MTLORA.FREEZE_PRETRAINED False (reference config.py:317): main.py:254-262 then
 * skips mark_only_lora_as_trainable, so every `linear.weight` of the MTLoRALinear layers trains next to the LoRA factors.
 *
 * mtlora_linear_weight_grad: the dense gradient of `linear.weight`.  All 1 + T outputs of the layer add the same x W^T + b, and the
 * task inputs and the dropout mask touch only the low-rank branches (lora.py:255-284, every shared mode), so
 *   dW[n][k] = sum_m ( dy_s[m][n] + sum_t dy_t[t][m][n] ) * x[m][k]          (N x K) fp32 row-major, the master's layout
 * x (M, K): the shared input the forward's dense product read (un-dropped; gelu(h) for a layer fed through a GELU gate);
 * dy_s, dy_t[t] (M, N); all row-major in d->dtype (fp32, bf16 or fp16), T = d->T.  Only M, K, N, dtype and T of the descriptor are
 * read.  A NULL source is an output that got no gradient and is skipped (dy_t itself may be NULL when T == 0); with every source
 * NULL, or M == 0, dW is written as zeros.  dW is fully overwritten on every call.  N and K multiples of the 16-byte vector of
 * d->dtype, N x K at most 65535 tiles of 128 x 128, every pointer 16-byte aligned; the size query answers -1 for a refused shape.
 * fp32 accumulation on the matrix pipe (MFMA for all three types); the sources extend the reduction dimension (sum_o dy_o^T x), so
 * no (M, N) intermediate exists.  One launch over 128 x 128 tiles x splits of M, then (when M is split) the fixed-order combine of
 * the partial tiles: no atomics, no memset, the same bits on every call with the same inputs.
 *
 * mtlora_linear_weight_cast: the per-step refresh of the compute-dtype copies of a trainable fp32 master W (N, K), one launch that
 * reads W once and writes Wc (N, K) and Wt (K, N) = Wc^T in `dtype` (rounding of W.to(dtype): to nearest even; fp32: a copy and a
 * transpose) -- the two operands MTLoRALinear's forward and backward read (lora.py:255, F.linear(x, self.linear.weight)).
 * ------------------------------------------------------------------------------------------ */
int64_t mtlora_linear_weight_grad_scratch_bytes(const mtlora_linear_desc* d);
int mtlora_linear_weight_grad(const mtlora_linear_desc* d, const void* x, const void* dy_s, const void* const* dy_t, float* dW,
                              void* scratch, int64_t scratch_bytes, void* stream);
int mtlora_linear_weight_cast(const float* W, int N, int K, int dtype, void* Wc, void* Wt, void* stream);

/* ------------------------------------------------------------------------------------------
 * Channels-last bilinear upsampling by an integer factor (align_corners=False) for the HRNet head of the callers
 * (models/seg_hrnet.py:498-526: F.interpolate of the coarse maps + torch.cat).  coarse (B,h,w,C) contiguous; the fine
 * tensor (B, scale*h, scale*w, .) is addressed with `ld_fine` elements per pixel, its pointer already offset to the
 * first channel of this map -- i.e. a channel slice of the concatenated matrix.  C and ld_fine multiples of 4,
 * pointers 8-byte (bf16, fp16) / 16-byte (fp32) aligned.  bwd = exact transpose (gather form, deterministic: ATen's
 * bilinear backward adds with atomics, which in fp16 with scaled gradients differs from run to run).
 * ------------------------------------------------------------------------------------------ */
int mtlora_upsample_cl_fwd(const void* coarse, void* fine, int64_t B, int h, int w, int C, int scale, int64_t ld_fine,
                           int dtype, void* stream);
int mtlora_upsample_cl_bwd(const void* grad_fine, void* grad_coarse, int64_t B, int h, int w, int C, int scale,
                           int64_t ld_fine, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * One whole SwinTransformerBlock WITHOUT task outputs, forward and backward, as ONE call each (ABI v7) -- replaces the
 * tasks-free path of SwinTransformerBlock.forward, models/swin_transformer_mtlora.py:326-408 (norm1 :331, shift / partition
 * :336-350, WindowAttention :353 = :186-227, merge / reverse shift :365-377, residual + DropPath :389, norm2 + Mlp :395-396
 * = :68-81, residual :398) with the four MTLoRALinear layers of lora.py:253-284 inside.  Nothing new is computed: the call
 * issues the launches of the entry points above in the block's order (LayerNorm -> qkv -> window attention -> proj ->
 * residual + DropPath + norm2 -> fc1 (+ GELU) -> fc2 -> residual + DropPath + the NEXT block's norm1), so its results are bit
 * identical to calling them one by one; what it removes is the caller's per-launch work (one host crossing and one autograd
 * node per block and direction instead of ~10: the train step of the reference's Swin-B config was bound by exactly that).
 * Every stage of a Swin backbone is `depth - 1` such blocks followed by one task-enabled block (:523-531), so a block of
 * this kind always hands over to another block: x_out AND normed_out = LayerNorm_next(x_out) are produced together.
 *
 * Tensors (M = B*H*W rows, token order (B, H*W) as everywhere in this library):
 *   x (M,C) x_dtype: the residual stream entering the block;  normed (M,C) dtype: norm1(x) when has_norm1 == 0 (it came out of
 *   the previous block's call), ignored otherwise;  x_out (M,C) x_dtype, normed_out (M,C) dtype.
 *   save: ONE caller-owned buffer of mtlora_block_save_bytes() that fwd fills and bwd reads (normalised tensors, qkv, attention
 *   output, the linears' ctx = P, the mid-block residual stream, fc1's pre-activation and activation, LayerNorm statistics);
 *   tmp: scratch of mtlora_block_fwd_tmp_bytes(), dead when fwd returns (stream-ordered).
 * bwd: g_x_out (M,C) x_dtype and g_normed_out (M,C) dtype are the gradients of the two outputs (g_x_out may be NULL);
 *   it writes g_x (x_dtype) and, when has_norm1 == 0, g_normed (dtype), the LayerNorm gradients, the eight factor gradients
 *   (fp32, shapes of the masters), dbias (num_heads, N, N) fp32 and, where asked for, the gradients of the four linears'
 *   biases: one mtlora_linear_bias_grad each on the buffer that linear's backward reads as dy, issued with the factor gradients
 *   (phases 0 and 2) and bit identical to the stand-alone call.  phase as mtlora_linear_desc.bwd_phase: 0 everything on
 *   `stream`; 1 everything but the factor gradients; 2 the factor gradients only (same arguments, a second stream ordered
 *   behind phase 1).  scratch: mtlora_block_bwd_scratch_bytes(), must stay valid until phase 2 has run.
 * ------------------------------------------------------------------------------------------ */
typedef struct mtlora_block_desc {
    int64_t B;
    int32_t H, W, C, hidden;   /* token map, channels, Mlp hidden width */
    int32_t num_heads, window_size, shift;
    int32_t dtype;             /* compute dtype: the linears, the normalised tensors, attention */
    int32_t x_dtype;           /* dtype of the residual stream (fp32 under autocast) */
    int32_t has_norm1;         /* 1: the call applies norm1 itself (first block of a stage); 0: `normed` is an input */
    float eps1, eps2, eps_next;
    float attn_scale, mask_value;
    mtlora_linear_desc lin[4]; /* qkv (C -> 3C), proj (C -> C), fc1 (C -> hidden, + GELU), fc2 (hidden -> C); T = 0, M = B*H*W;
                                  seed / dropout_p / packed / sel_* as for a stand-alone call (bwd_phase is set by the block call) */
} mtlora_block_desc;

typedef struct mtlora_block_params {   /* device pointers, caller-owned; fp32 unless noted */
    const float *norm1_g, *norm1_b;    /* has_norm1 only */
    const float *norm2_g, *norm2_b, *next_g, *next_b;
    const void* W[4];                  /* (N,K) dtype */
    const void* Wt[4];                 /* (K,N) dtype (bwd) */
    const float* bias[4];              /* (N) or NULL */
    const float* A[4];                 /* (r,K) masters */
    const float* Bf[4];                /* (N,r) masters */
    const float* attn_bias;            /* dense (num_heads, N, N) */
    const int32_t* mask_ids;           /* (nW, N) region ids of SW-MSA or NULL */
    const float* mask;                 /* general dense mask or NULL (ignored when mask_ids is given) */
    const float *scale1, *scale2;      /* DropPath mask / keep of the two residuals, (B) each, or NULL (= 1) */
} mtlora_block_params;

typedef struct mtlora_block_grads {    /* outputs of bwd, fp32 unless noted, all overwritten */
    void* g_x;                         /* (M,C) x_dtype */
    void* g_normed;                    /* (M,C) dtype; has_norm1 == 0 only */
    float *d_norm1_g, *d_norm1_b;      /* has_norm1 only */
    float *d_norm2_g, *d_norm2_b, *d_next_g, *d_next_b;
    float* dA[4];
    float* dB[4];
    float* dbias;                      /* (num_heads, N, N) */
    float* dlin_bias[4];               /* (N) gradient of the bias of qkv, proj, fc1, fc2; NULL = not wanted.  Appended under ABI 12: a library
                                          from before it lacks mtlora_linear_bias_grad, which the binding looks up when it loads */
} mtlora_block_grads;

int64_t mtlora_block_save_bytes(const mtlora_block_desc* d);
int64_t mtlora_block_fwd_tmp_bytes(const mtlora_block_desc* d);
int64_t mtlora_block_bwd_scratch_bytes(const mtlora_block_desc* d);
int mtlora_block_fwd(const mtlora_block_desc* d, const mtlora_block_params* p, const void* x, const void* normed, void* x_out,
                     void* normed_out, void* save, int64_t save_bytes, void* tmp, int64_t tmp_bytes, void* stream);
int mtlora_block_bwd(const mtlora_block_desc* d, const mtlora_block_params* p, const void* x, const void* normed,
                     const void* x_out, const void* g_x_out, const void* g_normed_out, const void* save, int64_t save_bytes,
                     const mtlora_block_grads* g, void* scratch, int64_t scratch_bytes, int phase, void* stream);

/* ------------------------------------------------------------------------------------------
 * The parameter update of the train step, fused (ABI v10): replaces, for ALL trainable tensors at once, what the
 * reference's NativeScalerWithGradNormCount.__call__ does after backward (utils.py:348-375, called at main.py:347-353):
 * GradScaler.unscale_, torch.nn.utils.clip_grad_norm_, the AdamW step over the decay / no-decay groups of
 * optimizer.py:71-85, and GradScaler.update -- three launches on `stream`, no host synchronisation, nothing read back.
 * fp32 parameters, gradients and state only; no amsgrad, no maximize.
 *
 * Tensors are cut into chunks of MTLORA_ADAMW_CHUNK elements, one workgroup per chunk.
 *   mtlora_adamw_sizes   pure host call: for n_tensors element counts, the number of chunks, the bytes of the device table
 *                        and the bytes of per-call scratch (two words per chunk).
 *   mtlora_adamw_table   pure host call: fills `host_table` (table_bytes of HOST memory) from the tensors' DEVICE pointers
 *                        p / m (exp_avg) / v (exp_avg_sq), element counts and parameter-group indices
 *                        (< MTLORA_ADAMW_MAX_GROUPS); the caller copies it to the device once.  Pointers 4-byte aligned; the
 *                        kernels use 16-byte accesses where a tensor's pointers are 16-byte aligned and scalar ones elsewhere.
 *   mtlora_adamw_update  one optimizer step.  `table`: the device copy of that table.  `grads`: DEVICE array of n_tensors
 *                        gradient pointers, re-uploaded by the caller whenever they change (autograd allocates fresh
 *                        gradients after zero_grad(set_to_none=True)); a null entry = no gradient this step: that tensor,
 *                        its state and nothing else of it is read or written (torch skips such parameters too).
 *                        `groups`: n_groups HOST structs, passed on to the kernels by value (lr moves every step under a
 *                        scheduler).  max_norm <= 0: no clipping.  `scale` / `growth_tracker`: DEVICE words of a GradScaler
 *                        (fp32 / int32), both null = no loss scaling; the gradients are multiplied by 1 / *scale, then
 *                        the scale is updated with growth_factor / backoff_factor / growth_interval as
 *                        torch.amp.GradScaler.update does.  `norm_out`: optional DEVICE fp32 word, receives the total norm.
 *                        `ctrl`: MTLORA_ADAMW_CTRL_WORDS fp32 DEVICE words owned by the optimizer, zero before the first
 *                        step, persistent:
 *                            [0] total 2-norm of the UNSCALED gradients before clipping   [1] found_inf (0 / 1)
 *                            [2] clip coefficient min(1, max_norm / (norm + 1e-6))         [3] [2] / *scale
 *                            [4] the step counter t (counts the steps that were not skipped)
 *                            [8 + 2 g], [9 + 2 g]  1 - beta1^t and sqrt(1 - beta2^t) of group g
 *                        A gradient holding inf / nan sets found_inf: the step is skipped ON THE DEVICE (parameters, state
 *                        and t stay bitwise unchanged; with a scaler the scale backs off) -- with or without a scaler.
 *                        Otherwise, per element: g' = g [3]; p *= 1 - lr wd; m = b1 m + (1 - b1) g';
 *                        v = b2 v + (1 - b2) g'^2; p -= lr / (1 - b1^t) m / (sqrt(v) / sqrt(1 - b2^t) + eps).
 *   mtlora_adamw_update_dev  the same step with the hyper-parameters read from DEVICE memory, for a step captured in a HIP
 *                        graph (additive, ABI stays 12): launch arguments are frozen at capture, so a replay of
 *                        mtlora_adamw_update would use the capture step's lr forever; here only pointers are baked in.
 *                        `groups_dev`: DEVICE buffer of MTLORA_ADAMW_GROUPS_DEV_BYTES, 8-byte aligned.  The caller writes
 *                        the n_groups records at its start (an ordinary copy on `stream` before the step / the replay,
 *                        whenever a value changes) and never touches the rest: the tail behind
 *                        MTLORA_ADAMW_MAX_GROUPS records is the library's, it holds what the kernels derive from the
 *                        records each step -- (float)lr, (float)(1 - lr wd), (float)beta, (float)(1 - beta), (float)eps,
 *                        formed in double exactly as the host forms them for mtlora_adamw_update, so with equal
 *                        hyper-parameters the two entries give bit-identical results.  growth_factor / backoff_factor are
 *                        doubles here and are rounded to fp32 once.  Pointer and count checks are made on the host before
 *                        any launch, as above.  The VALUES of the records cannot be checked on the host: a record that
 *                        mtlora_adamw_update rejects with MTLORA_ERR_SHAPE (lr, eps or weight_decay negative, a beta outside
 *                        [0, 1), any nan) sets found_inf on the device instead -- the step is skipped exactly like one with
 *                        an inf gradient (parameters, state and t bitwise unchanged; with a scaler the scale backs off)
 *                        and the norm in ctrl[0] / norm_out is nan.
 *   mtlora_adamw_accum_update_dev  ONE MICRO-STEP of gradient accumulation over k = accum_steps calls (the reference's
 *                        TRAIN.ACCUMULATION_STEPS, main.py:347-353; additive, ABI stays 12), for a graph that is replayed
 *                        once per micro-step.  Arguments as mtlora_adamw_update_dev, plus:
 *                        `acc`: persistent fp32 DEVICE accumulator the caller owns, 16-byte aligned, of the `acc_elems`
 *                        elements mtlora_adamw_accum_layout returns; never memset, by anyone (its first use overwrites it).
 *                        `acc_offsets`: DEVICE copy of the n_tensors int64 element offsets that call fills (tensor i's slice
 *                        is acc + acc_offsets[i], numel[i] elements, every slice 16-byte aligned); uploaded once.
 *                        `accum_steps`: 1 .. MTLORA_ADAMW_MAX_ACCUM_STEPS.  It is a LAUNCH ARGUMENT: a captured graph keeps
 *                        the k of its capture.
 *                        Two more words of `ctrl` (zero before first use, like the rest):
 *                            [MTLORA_ADAMW_CTRL_MICRO]    c, the micro-step counter, 0 <= c < k
 *                            [MTLORA_ADAMW_CTRL_UPDATED]  1 if the last call was an update micro-step, else 0
 *                        Every decision is taken on the device from c; nothing is read back.  Per call, still three launches:
 *                          accumulate   for every tensor with a non-null gradient entry: acc = g if c == 0 (what acc held is
 *                                       not read: a cycle poisoned by inf / nan cannot leak into the next), else
 *                                       acc = acc + g -- one fp32 add per element, in micro-step order, the bits autograd
 *                                       gives when it accumulates into .grad.  Fused into the norm pass: the value stored is
 *                                       the value squared.  A tensor's entry must be null or non-null for a WHOLE cycle.
 *                          c < k - 1    c = c + 1, [UPDATED] = 0.  Parameters, state, t, the bias corrections, ctrl[0..4],
 *                                       *scale, *growth_tracker and *norm_out stay bitwise unchanged: the update launch is
 *                                       still issued, and every workgroup leaves on [UPDATED] == 0 before it writes.
 *                          c == k - 1   the step of mtlora_adamw_update_dev with acc's slices as the gradients (norm,
 *                                       found_inf, clip, unscale, AdamW, scaler update, bad records -> skip and nan norm),
 *                                       then c = 0, [UPDATED] = 1 -- also when the step was skipped.
 *                        The loss is NOT divided by k (main.py:341-349): acc is the plain sum.  accum_steps == 1: every
 *                        call updates straight from `grads` (acc and acc_offsets are checked but not dereferenced), p, m, v
 *                        and ctrl[0..4] have the bits mtlora_adamw_update_dev gives, and [UPDATED] = 1.
 *   mtlora_adamw_accum_layout  pure host call: the accumulator's layout for n_tensors element counts -- `host_offsets`
 *                        (n_tensors int64, HOST memory, may be null) and the total `acc_elems`; slices are rounded up to 4.
 * Deterministic: no float atomics; the norm is summed in a fixed order (per-chunk fp32 partials, combined in double).
 * ------------------------------------------------------------------------------------------ */
#define MTLORA_ADAMW_CHUNK 4096
#define MTLORA_ADAMW_MAX_GROUPS 16
#define MTLORA_ADAMW_CTRL_WORDS 64
#define MTLORA_ADAMW_GROUPS_DEV_BYTES 1152 /* MAX_GROUPS 40-byte records, then 512 bytes for what is derived from them */
typedef struct mtlora_adamw_group {
    double lr, beta1, beta2, eps, weight_decay; /* doubles, as torch holds them: 1 - beta, 1 - lr wd and the powers are formed in
                                                   double and rounded once */
} mtlora_adamw_group;
int mtlora_adamw_sizes(int64_t n_tensors, const int64_t* numel, int64_t* n_chunks, int64_t* table_bytes,
                       int64_t* scratch_bytes);
int mtlora_adamw_table(int64_t n_tensors, const int64_t* numel, const int32_t* group, void* const* p, void* const* m,
                       void* const* v, void* host_table, int64_t table_bytes);
int mtlora_adamw_update(const void* table, const void* grads, int64_t n_tensors, int64_t n_chunks,
                        const mtlora_adamw_group* groups, int n_groups, float max_norm, float* ctrl, float* norm_out,
                        float* scale, int32_t* growth_tracker, float growth_factor, float backoff_factor,
                        int growth_interval, void* scratch, int64_t scratch_bytes, void* stream);
int mtlora_adamw_update_dev(const void* table, const void* grads, int64_t n_tensors, int64_t n_chunks,
                            const mtlora_adamw_group* groups_dev, int n_groups, float max_norm, float* ctrl,
                            float* norm_out, float* scale, int32_t* growth_tracker, double growth_factor,
                            double backoff_factor, int growth_interval, void* scratch, int64_t scratch_bytes,
                            void* stream);
#define MTLORA_ADAMW_CTRL_MICRO 5
#define MTLORA_ADAMW_CTRL_UPDATED 6
#define MTLORA_ADAMW_MAX_ACCUM_STEPS (1 << 24) /* c lives in an fp32 word */
int mtlora_adamw_accum_layout(int64_t n_tensors, const int64_t* numel, int64_t* host_offsets, int64_t* acc_elems);
int mtlora_adamw_accum_update_dev(const void* table, const void* grads, int64_t n_tensors, int64_t n_chunks,
                                  const mtlora_adamw_group* groups_dev, int n_groups, float max_norm, float* ctrl,
                                  float* norm_out, float* scale, int32_t* growth_tracker, double growth_factor,
                                  double backoff_factor, int growth_interval, void* scratch, int64_t scratch_bytes,
                                  float* acc, const int64_t* acc_offsets, int accum_steps, void* stream);

/* The learning-rate schedule INSIDE the fused update (additive, ABI stays 12): the reference's last per-step host action,
 * lr_scheduler.step_update((epoch * num_steps + idx) // ACCUMULATION_STEPS) (main.py:350-353, lr_scheduler.py), done by
 * k_optim_finish from a call counter in device memory, so that a replayed train step needs nothing from the host but the next batch.
 *   mtlora_lr_schedule   a plain record the host fills once: the four schedules of the reference's build_scheduler, counted in
 *                        update calls (t_in_epochs = False).  For group g with base value v = base_lr[g], at count t, in double,
 *                        without contraction, in exactly this order of operations (the order of the Python classes):
 *                          t < warmup_t (all kinds)   warmup_lr_init + t * ((v - warmup_lr_init) / warmup_t)
 *                          MTLORA_LR_COSINE     t -= warmup_t if warmup_prefix; i = t / t_initial; t_curr = t - t_initial * i;
 *                                               i < 1: lr_min + 0.5 * (v - lr_min) * (1 + cos(pi * t_curr / t_initial)), else lr_min
 *                          MTLORA_LR_STEP       v * pow(decay_rate, t / decay_t)                     (integer quotient)
 *                          MTLORA_LR_LINEAR     t -= warmup_t; v - (v - v * lr_min_rate) * (t / (t_initial - warmup_t))
 *                          MTLORA_LR_MULTISTEP  v * pow(gamma, the number of milestones <= t)        (milestones ascending)
 *                        Warm-up, the linear kind and the lr_min plateau use + - * / only and equal the host's Python floats bit
 *                        for bit; cos and pow are the device math library's.
 *   the schedule buffer  MTLORA_ADAMW_SCHED_DEV_BYTES of DEVICE memory the optimizer owns, 8-byte aligned: the record, then
 *                        at byte MTLORA_ADAMW_SCHED_COUNT_OFFSET an int64 u, the number of UPDATE CALLS made so far (a real
 *                        integer: a schedule counts past 2^24, which the fp32 control words cannot), then at byte
 *                        MTLORA_ADAMW_SCHED_LR_OFFSET double lr_used[MTLORA_ADAMW_MAX_GROUPS], the values the last update used.
 *                        The caller uploads record and u with an ordinary copy; the kernels own them from then on.
 *   mtlora_adamw_sched_update_dev  mtlora_adamw_accum_update_dev (same parameters, same three launches on every call) plus
 *                        `sched_dev`, that buffer.  accum_steps == 1: every call is an update call, acc and acc_offsets may be
 *                        null.  On an update call (c == k - 1) the per-group threads of k_optim_finish read u, form
 *                        lr = L_g(max(u - 1, 0)), store it to lr_used[g] and use it IN PLACE OF the group record's lr (betas,
 *                        eps and weight decay still come from `groups_dev`); u + 1 is written.  On an accumulating micro-step
 *                        u and lr_used stay bitwise unchanged.  u follows CALLS, not Adam steps: a call that found_inf skips
 *                        advances u (as the reference's idx advances) and not ctrl[4].  Why u - 1: the reference steps its
 *                        scheduler AFTER the optimizer, so update 0 runs at the constructor's value, which is L(0) for all four
 *                        kinds (milestones >= 1), and update n >= 1 at L(n - 1).  This reproduces the reference whenever
 *                        num_steps % ACCUMULATION_STEPS == 0 (otherwise its (epoch * num_steps + idx) // k repeats or skips a
 *                        count at an epoch boundary).  A record mtlora_lr_schedule_check rejects, a negative u or a value that
 *                        comes out negative or nan sets found_inf on the device, exactly as a bad hyper-parameter record does:
 *                        the step is skipped, the norm is nan, lr_used is nan.
 *   mtlora_lr_schedule_check  pure host call: MTLORA_OK if the kernels accept the record for n_groups groups, else
 *                        MTLORA_ERR_SHAPE -- unknown kind, n_milestones outside 0 .. MTLORA_LR_MAX_MILESTONES, milestones < 1 or
 *                        not ascending or in front of warmup_t, warmup_t < 0, a nan or negative warmup_lr_init / base_lr /
 *                        lr_min / lr_min_rate / decay_rate / gamma, t_initial <= 0 (cosine), t_initial <= warmup_t
 *                        (linear), decay_t <= 0 (step).  The kernels run the same function on the device record.
 *   mtlora_lr_schedule_value  pure host call: *lr = L_group(t) by the very function the kernel runs (the host compiler's cos
 *                        and pow), for checks without a device; MTLORA_ERR_SHAPE if the record is rejected or t < 0. */
#define MTLORA_LR_MAX_MILESTONES 16
#define MTLORA_LR_COSINE 1
#define MTLORA_LR_STEP 2
#define MTLORA_LR_LINEAR 3
#define MTLORA_LR_MULTISTEP 4
typedef struct mtlora_lr_schedule {
    int64_t kind, warmup_t, warmup_prefix, t_initial, decay_t, n_milestones; /* counts are int64, values are doubles */
    int64_t milestones[MTLORA_LR_MAX_MILESTONES];
    double warmup_lr_init, lr_min, lr_min_rate, decay_rate, gamma;
    double base_lr[MTLORA_ADAMW_MAX_GROUPS];
} mtlora_lr_schedule;
#define MTLORA_ADAMW_SCHED_COUNT_OFFSET 344 /* sizeof(mtlora_lr_schedule) */
#define MTLORA_ADAMW_SCHED_LR_OFFSET 352
#define MTLORA_ADAMW_SCHED_DEV_BYTES 480
int mtlora_lr_schedule_check(const mtlora_lr_schedule* host_record, int n_groups);
int mtlora_lr_schedule_value(const mtlora_lr_schedule* host_record, int n_groups, int group, int64_t t, double* lr);
int mtlora_adamw_sched_update_dev(const void* table, const void* grads, int64_t n_tensors, int64_t n_chunks,
                                  const mtlora_adamw_group* groups_dev, int n_groups, float max_norm, float* ctrl,
                                  float* norm_out, float* scale, int32_t* growth_tracker, double growth_factor,
                                  double backoff_factor, int growth_interval, void* scratch, int64_t scratch_bytes,
                                  float* acc, const int64_t* acc_offsets, int accum_steps, void* sched_dev, void* stream);

/* The other two optimizers of the reference's optimizer.py:53-66 on the same machinery (additive, ABI stays 12): the table of
 * mtlora_adamw_sizes / mtlora_adamw_table, the gradient-pointer array, the norm and finish launches, the control block (words
 * [0..4] as above), the skip on inf / nan, the GradScaler words and the fixed-order reductions are those of mtlora_adamw_update;
 * only what follows the finish launch differs.  Every argument that mtlora_adamw_update has means the same here.  Each has a
 * by-value entry (`groups`: HOST records) and a _dev entry (`groups_dev`: a DEVICE buffer of MTLORA_ADAMW_GROUPS_DEV_BYTES whose
 * first n_groups records the caller writes and whose tail is the library's; a record the by-value entry rejects sets found_inf
 * on the device: the step is skipped, the norm is nan).  With equal records the two entries give bit-identical results.
 *   mtlora_sgd_update[_dev]   torch.optim.SGD(momentum, dampening=0, weight_decay, nesterov) -- optimizer.py:56 -- in THREE
 *                        launches (norm, finish, step).  Only `m` of the table is used: the momentum buffer (`v` must still
 *                        be non-null; pass m).  With g the unscaled, clipped gradient (g_stored * ctrl[3]), per element:
 *                            g' = g + wd p;  m = mu m + g';  p -= lr (g' + mu m) if nesterov, else p -= lr m
 *                        A zero-initialised m gives torch's first step (m = g') because dampening is 0.  mu == 0: plain SGD,
 *                        p -= lr g', and m is neither read nor written.  Rejected records: lr, momentum or weight_decay
 *                        negative or nan, nesterov not 0 or 1.
 *   mtlora_lamb_update[_dev]  apex FusedLAMB(bias_correction, grad_averaging, adam_w_mode all True) in FOUR launches (norm,
 *                        finish, moments + partials, apply).  The records are mtlora_adamw_group.  `scratch`: TWICE the
 *                        scratch_bytes mtlora_adamw_sizes reports (four words per chunk).  `max_grad_norm` <= 0 disables
 *                        LAMB's own clip.  With n = ctrl[0] * ctrl[2], the norm of the gradients after the max_norm clip:
 *                            c = n / max_grad_norm if n > max_grad_norm else 1   (ctrl[MTLORA_LAMB_CTRL_CLIP]);  ctrl[3] = ctrl[2] / *scale / c
 *                            g = g_stored * ctrl[3];  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2        (launch 3, stored)
 *                            u = (m / (1 - b1^t)) / (sqrt(v) / sqrt(1 - b2^t) + eps) + wd p                    (never stored)
 *                            per tensor |p| and |u|: launch 3 writes one fp32 partial of each per chunk, launch 4 adds a
 *                            tensor's partials in double in a fixed order (no float atomics; a chunk never spans tensors)
 *                            ratio = lr |p| / |u| if (wd != 0 or use_nvlamb) and |p| != 0 and |u| != 0, else lr
 *                            p -= ratio u     (launch 4 forms u again from the stored m, v and the still unmodified p)
 *                        A skipped step leaves p, m, v and t bitwise unchanged: launches 3 and 4 read found_inf before they
 *                        write.  max_grad_norm and use_nvlamb are launch arguments: a captured graph keeps those of its capture. */
#define MTLORA_LAMB_CTRL_CLIP 7
typedef struct mtlora_sgd_group {
    double lr, momentum, nesterov, reserved, weight_decay; /* nesterov: 0.0 or 1.0; reserved: 0.0 */
} mtlora_sgd_group;
int mtlora_sgd_update(const void* table, const void* grads, int64_t n_tensors, int64_t n_chunks, const mtlora_sgd_group* groups,
                      int n_groups, float max_norm, float* ctrl, float* norm_out, float* scale, int32_t* growth_tracker,
                      float growth_factor, float backoff_factor, int growth_interval, void* scratch, int64_t scratch_bytes,
                      void* stream);
int mtlora_sgd_update_dev(const void* table, const void* grads, int64_t n_tensors, int64_t n_chunks,
                          const mtlora_sgd_group* groups_dev, int n_groups, float max_norm, float* ctrl, float* norm_out,
                          float* scale, int32_t* growth_tracker, double growth_factor, double backoff_factor,
                          int growth_interval, void* scratch, int64_t scratch_bytes, void* stream);
int mtlora_lamb_update(const void* table, const void* grads, int64_t n_tensors, int64_t n_chunks,
                       const mtlora_adamw_group* groups, int n_groups, float max_norm, float max_grad_norm, int use_nvlamb,
                       float* ctrl, float* norm_out, float* scale, int32_t* growth_tracker, float growth_factor,
                       float backoff_factor, int growth_interval, void* scratch, int64_t scratch_bytes, void* stream);
int mtlora_lamb_update_dev(const void* table, const void* grads, int64_t n_tensors, int64_t n_chunks,
                           const mtlora_adamw_group* groups_dev, int n_groups, float max_norm, float max_grad_norm,
                           int use_nvlamb, float* ctrl, float* norm_out, float* scale, int32_t* growth_tracker,
                           double growth_factor, double backoff_factor, int growth_interval, void* scratch,
                           int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Batch ingest (ABI v12): the tail of the reference's loader pipelines on the device -- RandomHorizontalFlip,
 * AddIgnoreRegions, ToTensor and Normalize of data/custom_transforms.py:192-209 and :266-341 -- for one batch in the
 * narrowest lossless host format ("wire format": uint8 HWC image, uint8 class / binary maps, fp32 or fp16 HWC normals,
 * fp32 depth), written as the fp32 (B, C, H, W) tensors the train, validation and prediction steps take.
 *
 * One job per tensor, at most MTLORA_INGEST_MAX_JOBS, passed by value in the launch arguments.  Per sample b, in this order:
 *   flip[b] != 0: mirror along W; normals channel 0 changes sign
 *   MTLORA_INGEST_IMAGE                 u8 (B,H,W,3) -> f32 (B,3,H,W), dst = lut[c * 256 + src]; `lut` is the caller's
 *                                       (3, 256) table ((v / 255) - mean[c]) / std[c], so no division happens here
 *   MTLORA_INGEST_CLASS                 u8 (B,H,W)   -> f32 (B,1,H,W), the value itself
 *   MTLORA_INGEST_CLASS_ALLZERO_IGNORE  as CLASS; a sample that is 0 everywhere becomes 255 everywhere (human_parts)
 *   MTLORA_INGEST_NORMALS               f32 or f16 (B,H,W,3) -> f32 (B,3,H,W); a pixel whose three components are all +-0
 *                                       becomes 255 in all three channels
 *   MTLORA_INGEST_DEPTH                 f32 (B,H,W)  -> f32 (B,1,H,W); +-0 becomes 255
 * `C` is the channel count of the job (3 for IMAGE and NORMALS, 1 otherwise), `src_dtype` MTLORA_U8 / MTLORA_F32 /
 * MTLORA_F16 as listed, `reserved` is ignored.  `src` may sit at any multiple of its element size (a uint8 source at any
 * byte), `dst` is contiguous and 4-byte aligned; no input is written, every element of every dst is written exactly once.
 *
 * At most three launches on `stream`, no host synchronisation: with a CLASS_ALLZERO_IGNORE job a zeroing launch for the
 * per-sample flag words in `scratch` and a pass that ORs "any non-zero" into them (integer atomic OR), then the main launch
 * over all jobs.  Without such a job `scratch` is not touched (it may be NULL).  Deterministic; no float atomics.
 * mtlora_ingest_scratch_bytes is a pure host call (negative status for arguments out of range).
 *
 * Rejected before any launch: n_jobs outside 1..8, an unknown kind, a C the kind does not take, B, H or W < 1, a null
 * `jobs`, src or dst, an IMAGE job without `lut` (all MTLORA_ERR_UNSUPPORTED); a src_dtype the kind does not take
 * (MTLORA_ERR_DTYPE); a src or dst off its element's alignment (MTLORA_ERR_ALIGN); a `scratch` that is needed and
 * missing or too small (MTLORA_ERR_WORKSPACE).
 * ------------------------------------------------------------------------------------------ */
#define MTLORA_INGEST_MAX_JOBS 8
typedef enum mtlora_ingest_kind {
    MTLORA_INGEST_IMAGE = 0,
    MTLORA_INGEST_CLASS = 1,
    MTLORA_INGEST_CLASS_ALLZERO_IGNORE = 2,
    MTLORA_INGEST_NORMALS = 3,
    MTLORA_INGEST_DEPTH = 4
} mtlora_ingest_kind;
typedef struct mtlora_ingest_job {
    const void* src;
    void* dst;
    int32_t kind, src_dtype, C, reserved;
} mtlora_ingest_job;
int64_t mtlora_ingest_scratch_bytes(int n_jobs, int64_t B);
int mtlora_ingest_batch(const mtlora_ingest_job* jobs, int n_jobs, int64_t B, int32_t H, int32_t W, const uint8_t* flip,
                        const float* lut, void* scratch, int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Geometric augmentation (added under ABI v12, additive): the head of the reference's training pipeline on the device --
 * ScaleNRotate (data/custom_transforms.py:24-88: cv2.getRotationMatrix2D about (w / 2, h / 2), cv2.warpAffine with
 * BORDER_CONSTANT 0, the in-plane rotation of the normals :74-80, depth / sc :83-84) composed with FixedResize (:94-154, the
 * renormalisation of the normals :144-150), as data/mtl_ds.py:846-859 chains them (and :866-867 for the resize-only test
 * pipeline: rotation 0, scale 1) -- for one batch of decoded, un-resampled samples in "canvas format": every tensor stacked as
 * (B, Hc, Wc[, 3]) with the dtypes of the wire format, sample b occupying the top-left size[b] = (h, w) rectangle of its
 * canvas.  The outputs are the wire-format tensors at (Ho, Wo) that the batch ingest above takes.  ONE resample per pixel
 * where the reference has two (it warps at source size and resizes afterwards).
 *
 * `size`  int32 (B, 2): h, w with 1 <= h <= Hc, 1 <= w <= Wc (clamped to the canvas on the device: no value makes the kernel
 *         read outside a source).  Canvas pixels outside the rectangle are never read; they count as border (0).
 * `geom`  int64 (B, 6): ax, bx, cx, ay, by, cy with MTLORA_AUGMENT_GEOM_BITS fraction bits; the source coordinate of output
 *         pixel (u, v) is X = ax (2u + 1) + bx (2v + 1) + cx and Y likewise, in int64.  The caller composes them in float64.
 * `side`  fp32 (B, 3): cos(rot), sin(rot), sc.  Needed by NORMALS and DEPTH jobs.
 * `cubic_q15` int32 (32, 4), `cubic_f32` fp32 (32, 4): the four cubic weights (Keys, a = -0.75) at the fractions f / 32, rows
 *         of the Q15 form summing to 32768.  Needed by IMAGE (q15) and NORMALS (f32) jobs.
 *
 * One job per tensor, at most MTLORA_INGEST_MAX_JOBS, passed by value in the launch arguments:
 *   MTLORA_AUGMENT_IMAGE_CUBIC_U8     u8 (B,Hc,Wc,3) -> u8 (B,Ho,Wo,3); coordinate rounded to 1/32 pixel, 4 x 4 taps, integer
 *                                     accumulation, clamp((acc + 2^29) >> 30, 0, 255)
 *   MTLORA_AUGMENT_CLASS_NEAREST_U8   u8 (B,Hc,Wc) -> u8 (B,Ho,Wo); coordinate rounded half up to the source pixel
 *   MTLORA_AUGMENT_NORMALS_CUBIC_F32  f32 (B,Hc,Wc,3) -> f32 (B,Ho,Wo,3); the same taps in fp32 (horizontal left to right, then
 *                                     vertical top to bottom, no contraction), x' = x cos + y sin, y' = y cos - x sin, then
 *                                     n / (|n| + 2^-52) unless MTLORA_AUGMENT_FLAG_NO_RENORM is set in `flags`
 *   MTLORA_AUGMENT_DEPTH_NEAREST_F32  f32 (B,Hc,Wc) -> f32 (B,Ho,Wo); the nearest sample divided by sc
 * A tap or a nearest sample outside [0, w) x [0, h) counts as 0.  `src` may sit at any multiple of its element size (a uint8
 * source at any byte), `dst` is contiguous and 16-byte aligned; no input is written, every element of every dst is written
 * exactly once.  One launch on `stream`, no host synchronisation, no scratch buffer; deterministic, plain vector stores.
 *
 * Rejected before any launch: n_jobs outside 1..8, an unknown kind or flag, B, Hc, Wc, Ho or Wo < 1, a null `jobs`, src, dst,
 * `size` or `geom`, a job without the table or the side table it needs (all MTLORA_ERR_UNSUPPORTED); a src off its element's
 * alignment, a dst off 16 bytes, a table off its element's alignment (MTLORA_ERR_ALIGN); more than 65535 samples or 2^31
 * output pixels per sample (MTLORA_ERR_SHAPE).
 * ------------------------------------------------------------------------------------------ */
#define MTLORA_AUGMENT_GEOM_BITS 24
#define MTLORA_AUGMENT_FLAG_NO_RENORM 1
typedef enum mtlora_augment_kind {
    MTLORA_AUGMENT_IMAGE_CUBIC_U8 = 0,
    MTLORA_AUGMENT_CLASS_NEAREST_U8 = 1,
    MTLORA_AUGMENT_NORMALS_CUBIC_F32 = 2,
    MTLORA_AUGMENT_DEPTH_NEAREST_F32 = 3
} mtlora_augment_kind;
typedef struct mtlora_augment_job {
    const void* src;
    void* dst;
    int32_t kind, flags;
} mtlora_augment_job;
int mtlora_augment_batch(const mtlora_augment_job* jobs, int n_jobs, int64_t B, int32_t Hc, int32_t Wc, int32_t Ho, int32_t Wo,
                         const int32_t* size, const int64_t* geom, const float* side, const int32_t* cubic_q15,
                         const float* cubic_f32, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training meters (added under ABI v12, additive): replaces timm's AverageMeter.update as the reference's train loop uses it
 * (main.py:318-321 the meters, :354-365 loss scale, loss, gradient norm, :384-386 the per-task losses) -- there one .item() /
 * state_dict() read-back per value and step, here ONE launch at the end of the step that reads every value where it already
 * sits in device memory.
 *
 * `bank`     n_slots x {val, sum, count, skipped}, doubles, 16-byte aligned.  avg = sum / count is the reader's division.
 * `table`    n_slots records in device memory: `src` a device address holding one fp32 (MTLORA_METER_F32) or fp64
 *            (MTLORA_METER_F64) value, aligned to it; `weight` AverageMeter's n; `period` k >= 1 (a smaller value counts as 1).
 *            A record whose src is null is never served.
 * `counter`  one device int64, owned by the bank: the number of update calls so far.
 * A call that finds the counter at c serves slot i iff (c + 1) % period == 0 (an untouched slot is not written): v = *src;
 * v finite: val = v, sum += v * weight, count += weight (product and sum rounded separately); v inf or nan: val = v,
 * skipped += 1, sum and count stay -- unlike AverageMeter, where one overflowed fp16 step would turn the epoch's average into
 * inf / nan.  Then counter = c + 1.
 * One launch of one 64-lane workgroup on `stream`, lane i serving slot i; plain loads and vector stores, no atomics, no
 * memset, nothing allocated, retained or synchronised: every pointer is a launch argument, so a captured launch replays as is.
 * The reset is a zero-fill kernel over the bank (a captured memset does not replay reliably, see the train-step notes);
 * keep_phase == 0 zeroes the counter as well, keep_phase != 0 keeps the position inside the periods.
 * Rejected before any launch: n_slots outside 1 .. MTLORA_METER_MAX_SLOTS (MTLORA_ERR_SHAPE, before any pointer is looked at);
 * a null bank, table or counter (MTLORA_ERR_NULL); a bank off 16 bytes, a table or counter off 8 (MTLORA_ERR_ALIGN).
 * ------------------------------------------------------------------------------------------ */
#define MTLORA_METER_MAX_SLOTS 64
#define MTLORA_METER_F32 0
#define MTLORA_METER_F64 1
typedef struct mtlora_meter_source {
    const void* src;
    int32_t dtype, reserved;
    double weight;
    int64_t period;
} mtlora_meter_source;
int mtlora_meter_update(double* bank, const mtlora_meter_source* table, int n_slots, int64_t* counter, void* stream);
int mtlora_meter_reset(double* bank, int n_slots, int64_t* counter, int keep_phase, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training-state snapshot (added under ABI v12, additive): the device half of the reference's save_checkpoint and
 * auto_resume_helper (utils.py:280-321).  There the checkpoint is model.state_dict() / optimizer.state_dict() /
 * loss_scaler.state_dict(): one device-to-host copy per tensor and a host synchronisation.  Here every tensor a train step mutates
 * is gathered into one contiguous `packed` buffer by ONE launch between two replays of the step, and scattered back by one.
 *
 * `table`   n entries of mtlora_snapshot_entry_bytes each: a device address, a byte count (0 is legal) and the entry's offset in
 *           `packed`.  Entries ascend in `packed`, every offset a multiple of 16, none reaching into the next; the bytes between
 *           entries are never written.  Tensors are opaque bytes at ANY address alignment: 16-byte vector accesses where the
 *           address is 16-byte aligned, dwords where it is 4-byte aligned, bytes otherwise; nothing outside
 *           [address, address + bytes) is read or written.  The caller builds the table once on the host, uploads it and keeps
 *           it (8-byte aligned); it holds raw addresses, valid while the tensors live and are only updated in place.
 * Work is cut into chunks of MTLORA_SNAPSHOT_CHUNK bytes of `packed`; one workgroup owns one chunk.
 *
 *   mtlora_snapshot_entry_bytes   utils.py:280-321 has no counterpart: size of one table entry.
 *   mtlora_snapshot_entry         fills one entry of a HOST table (what utils.py:280-321 names by state_dict key).  MTLORA_ERR_NULL
 *                                 for a null entry or a null address with bytes > 0, MTLORA_ERR_SHAPE for a negative size or
 *                                 offset, MTLORA_ERR_ALIGN for an offset that is no multiple of 16.
 *   mtlora_snapshot_chunks        the number of chunks a HOST table of n entries needs (ceil(extent / MTLORA_SNAPSHOT_CHUNK), the
 *                                 extent being the end of the last entry; 0 for an empty table), or a negative status: what
 *                                 mtlora_snapshot_entry rejects, found per entry, MTLORA_ERR_NULL for a null table with n > 0 and
 *                                 MTLORA_ERR_SHAPE for an entry that begins before the previous one ends.  Pure host call, for the
 *                                 save of utils.py:280-321.
 *   mtlora_snapshot_check         the same validation plus MTLORA_ERR_WORKSPACE if packed_bytes is smaller than the extent; pure
 *                                 host call, made once when the table is built (utils.py:280-321: before the first save).
 *   mtlora_snapshot_pack          tensors -> packed: the copy behind save_checkpoint (utils.py:280-321), one launch on `stream`.
 *   mtlora_snapshot_unpack        packed -> tensors through the same table: the copy behind a resume (auto_resume_helper and
 *                                 load_checkpoint, utils.py:280-321 and :41-176), one launch on `stream`.
 * Both launches reject, before anything runs: negative n, n_chunks or packed_bytes (MTLORA_ERR_SHAPE); a null table with n > 0
 * or a null `packed` with n_chunks > 0 (MTLORA_ERR_NULL); a table off 8 bytes or a `packed` off 16 (MTLORA_ERR_ALIGN); a
 * packed_bytes that n_chunks chunks cannot fit in, packed_bytes <= (n_chunks - 1) * MTLORA_SNAPSHOT_CHUNK (MTLORA_ERR_WORKSPACE; the
 * table is device memory at this point, the exact comparison is mtlora_snapshot_check's).  The kernel touches no byte of `packed`
 * at or behind packed_bytes whatever the table says.  n == 0 or n_chunks == 0 launches nothing.  Plain vector loads and stores,
 * no atomics, no scratch, no memset; nothing is allocated, retained or synchronised and every pointer is a launch argument or
 * sits in the table, so a captured launch replays as it is.
 * ------------------------------------------------------------------------------------------ */
#define MTLORA_SNAPSHOT_CHUNK 32768
int64_t mtlora_snapshot_entry_bytes(void);
int mtlora_snapshot_entry(void* host_entry, const void* ptr, int64_t bytes, int64_t packed_offset);
int64_t mtlora_snapshot_chunks(const void* host_table, int64_t n);
int mtlora_snapshot_check(const void* host_table, int64_t n, int64_t packed_bytes);
int mtlora_snapshot_pack(const void* dev_table, int64_t n, int64_t n_chunks, void* packed, int64_t packed_bytes, void* stream);
int mtlora_snapshot_unpack(const void* dev_table, int64_t n, int64_t n_chunks, const void* packed, int64_t packed_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Hardware self-test: writes the lane->element maps of the MFMA / LDS-transpose primitives the
 * kernels rely on into `out` (int32[4096]) so a GPU test can assert them (tests/test_gpu_layouts.py).
 * ------------------------------------------------------------------------------------------ */
int mtlora_selftest_layouts(int32_t* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Opt-in per-launch timing for the roofline report (bench.py): between begin and end every kernel
 * launch of this library is bracketed by two HIP events recorded on ITS launch stream and tagged with
 * a kind and the algorithmic bytes of that launch.  `end` must be called after the streams
 * were synchronised.  A process-wide diagnostic switch -- the only global state in the library; the
 * compute entry points stay re-entrant.
 * ------------------------------------------------------------------------------------------ */
#define MTLORA_PROF_KINDS 24
typedef struct mtlora_prof_summary {
    int64_t count[MTLORA_PROF_KINDS];
    double ms[MTLORA_PROF_KINDS];        /* sum of launch durations */
    double alg_bytes[MTLORA_PROF_KINDS]; /* sum of the useful bytes of the launches as issued (incl. the fused GELU write /
                                            gate read riding on the MTLoRALinear kernels) */
    double s8d_bytes[MTLORA_PROF_KINDS]; /* sum of the SURVEY 8(d) algorithmic bytes: the MTLoRALinear / attention-core formulas
                                            only (no GELU traffic); 0 for kinds outside the hot path (ABI v3) */
    double flops[MTLORA_PROF_KINDS];     /* sum of algorithmic FLOPs, un-padded ranks (GEMM kinds only; ABI v3) */
} mtlora_prof_summary;
int mtlora_prof_begin(int max_records);
int mtlora_prof_end(mtlora_prof_summary* out);
const char* mtlora_prof_kind_name(int kind);

#ifdef __cplusplus
}
#endif
#endif /* MTLORA_HIP_H */
