// optim.hip -- the parameter update of the reference train step (main.py:347-353 with utils.py:348-375 and the AdamW of
// optimizer.py:71-85), fused: GradScaler.unscale_ + clip_grad_norm_ + AdamW.step + GradScaler.update over ALL trainable
// tensors as three launches, with no host synchronisation and no per-tensor work on the host.  fp32 parameters, gradients and state.
//
// The tensors are cut into chunks of MTLORA_ADAMW_CHUNK elements; one 256-thread workgroup owns one chunk.  A device table
// (built on the host by mtlora_adamw_table, uploaded once) maps chunk -> (tensor, chunk index inside it) and tensor ->
// (p, m, v, numel, group).  The gradient pointers live in a table of their own, because they change from step to step
// (zero_grad(set_to_none=True) lets autograd allocate fresh gradients): the caller re-uploads that one array per step.  A null
// gradient pointer switches the tensor's chunks off: nothing of it is read or written.
//
//   k_optim_norm    partials[chunk] = sum of g^2 over the chunk, of the gradients AS STORED (still multiplied by the loss scale);
//                   flags[chunk] = 1 if a value of the chunk is inf / nan.  No float atomics: every workgroup owns its two words.
//   k_optim_finish  ONE workgroup: partials summed in a fixed order in double (thread t takes t, t + 256, ...; then a fixed
//                   tree), so the norm is bit-reproducible from run to run.  Writes the control block (unscaled norm, found_inf,
//                   clip coefficient, the factor coef / scale the update applies to the raw gradients, the step counter --
//                   incremented only when the step is not skipped -- and each group's bias corrections, powers in double) and
//                   performs GradScaler.update: on found_inf scale *= backoff and the growth tracker returns to 0; otherwise the
//                   tracker counts up and at growth_interval scale *= growth (kept only if finite, as ATen) and the tracker resets.
//   k_optim_step    the same chunk grid.  found_inf set: returns before touching memory -- parameters and state stay bitwise
//                   unchanged.  Otherwise torch's AdamW, decoupled weight decay, per element:
//                       g' = g * (coef / scale);  p *= 1 - lr wd;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;
//                       p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)
//                   lr, wd, betas, eps per parameter group, BY VALUE in the launch arguments (lr moves every step under a
//                   scheduler; nothing to upload).
// Every chunk kernel of this file finds its chunk with opt_slice and -- k_optim_step apart, see there -- walks it with opt_stream:
// 16-byte accesses where every pointer in use is 16-byte aligned, the last n % 4 elements and every element of a misaligned tensor
// scalar.  Every update entry is opt_check, the entry's own checks, then opt_update<algorithm, groups type>, the one launcher.
//
// mtlora_adamw_update_dev is the same three launches with the hyper-parameters in DEVICE memory, for a step that is captured in a
// HIP graph: launch arguments are frozen at capture, device memory is read at replay.  The group records (doubles) sit in a buffer
// of MTLORA_ADAMW_GROUPS_DEV_BYTES; k_optim_finish's one-thread-per-group part derives from them, in double, what the host derives
// for the by-value entry ((float)lr, (float)(1 - lr wd), (float)b, (float)(1 - b), (float)eps -- the same IEEE operations, no
// contraction, so the two entries are bit-identical) and stores it in that buffer's tail, where k_optim_step reads it.  A record
// the host entry would reject (negative lr, beta >= 1, nan) raises found_inf: the step is skipped and the norm is nan.
//
// mtlora_adamw_accum_update_dev is one MICRO-step of gradient accumulation (main.py:347-353 with ACCUMULATION_STEPS = k), still three
// launches, for a graph that is replayed once per micro-step.  Two more control words: c, the micro-step counter, and `updated`.
//   k_optim_norm<true>    the accumulate pass and the norm pass are ONE kernel: acc = g (c == 0) or acc + g (one fp32 add, in micro-step
//                         order: the bits autograd's accumulation into .grad gives), stored, and the partial / flag formed from the
//                         value just stored.  acc is read once and written once per micro-step and not read again for the norm.
//   k_optim_finish<G, true>  c < k - 1: c = c + 1, updated = 0, and nothing else is written.  c == k - 1: the finish above, then
//                         c = 0, updated = 1.
//   k_optim_step<G, OptGradAcc>  the same launch every micro-step (a graph replays a fixed launch list); every workgroup leaves on
//                         updated == 0 before it reads or writes anything else; otherwise the step above with acc's slices as gradients.
//
// mtlora_adamw_sched_update_dev is that micro-step (k >= 1) with the learning-rate schedule of the reference's lr_scheduler.py on the
// device: the last thing the host did between two replays (lr_scheduler.step_update, main.py:350-353).  A buffer of
// MTLORA_ADAMW_SCHED_DEV_BYTES holds the mtlora_lr_schedule record, an int64 count u of UPDATE CALLS (not of Adam steps: a skipped
// call counts, as the reference's idx does; and a real integer, a schedule runs past the 2^24 an fp32 word counts to) and the
// doubles lr_used[g].
//   k_optim_finish<OptGroupsDev, true, true>  on an update call the one-thread-per-group part reads u, forms lr = L_g(max(u - 1, 0))
//                         (opt_sched_lr: double, no contraction, the Python classes' order of operations, so warm-up, the linear
//                         kind and the lr_min plateau are the host's bits), stores it to lr_used[g] and hands it to opt_derive in
//                         place of the record's lr; thread 0 writes u + 1.  A record opt_sched_ok rejects raises found_inf like a
//                         bad hyper-parameter record.  An accumulating micro-step leaves before any of this.
//   k_optim_norm, k_optim_step  the instantiations above, unchanged: what they read of the schedule is h.lr[g] in the groups' tail.
//
// mtlora_sgd_update[_dev] and mtlora_lamb_update[_dev] run the reference's other two optimizers on the same table, norm and finish
// launches: see "SGD and LAMB" below.
#include "common.h"

namespace {

constexpr int OPT_CHUNK = MTLORA_ADAMW_CHUNK;
constexpr int OPT_THREADS = 256;
constexpr int OPT_VPT = OPT_CHUNK / (4 * OPT_THREADS);  // 16-byte vectors per thread and chunk
constexpr int OPT_MAXG = MTLORA_ADAMW_MAX_GROUPS;
static_assert(OPT_CHUNK % (4 * OPT_THREADS) == 0, "chunk = whole vectors per thread");

// the device table: [n_tensors] OptTensor, then [n_chunks] OptChunk
struct OptTensor {
    float* p;
    float* m;
    float* v;
    int64_t n;
    int32_t group;
    int32_t pad_;
};
struct OptChunk {
    int32_t tensor;
    int32_t index;  // element offset = index * OPT_CHUNK
};
static_assert(sizeof(OptTensor) == 40 && sizeof(OptChunk) == 8, "table layout");

struct OptHyperArr {  // what k_optim_step needs of the groups: 448 bytes
    float lr[OPT_MAXG], decay[OPT_MAXG], b1[OPT_MAXG], omb1[OPT_MAXG], b2[OPT_MAXG], omb2[OPT_MAXG], eps[OPT_MAXG];
};
struct OptGroups {  // kernel argument.  The hyper-parameters arrive as doubles (as torch holds them); what is derived from them is
    // formed in double on the host and rounded once: 1 - 0.999f is 1.3e-5 away from 1 - 0.999
    OptHyperArr h;
    double b1d[OPT_MAXG], b2d[OPT_MAXG];
    int n;
};
struct OptGroupsDev {  // kernel argument of the _dev entry: [OPT_MAXG] records the caller uploads; behind them the OptHyperArr that
    const mtlora_adamw_group* rec;  // k_optim_finish derives from them -- the same arrays, indexed the same way, as the by-value
    OptHyperArr* hyp;               // argument holds, so that k_optim_step is the same code on both paths
    int n;
};
struct OptHyper {  // one group's derived values
    float lr, decay, b1, omb1, b2, omb2, eps;
};
static_assert(sizeof(mtlora_adamw_group) == 40 && sizeof(OptHyperArr) == 28 * OPT_MAXG, "group buffer layout");
static_assert(OPT_MAXG * sizeof(mtlora_adamw_group) + sizeof(OptHyperArr) <= MTLORA_ADAMW_GROUPS_DEV_BYTES, "group buffer size");

__device__ __forceinline__ const OptHyperArr& opt_hyper(const OptGroups& g) { return g.h; }
__device__ __forceinline__ const OptHyperArr& opt_hyper(const OptGroupsDev& g) { return *g.hyp; }
__host__ __device__ inline void opt_put(OptHyperArr& a, int i, const OptHyper& h) {
    a.lr[i] = h.lr;
    a.decay[i] = h.decay;
    a.b1[i] = h.b1;
    a.omb1[i] = h.omb1;
    a.b2[i] = h.b2;
    a.omb2[i] = h.omb2;
    a.eps[i] = h.eps;
}

// host and device form the derived values with the same expression; on the device the product and the difference must stay two
// roundings (the host has no fused multiply-add to contract them into)
__host__ __device__ inline bool opt_derive(const mtlora_adamw_group& s, OptHyper& h) {
#pragma clang fp contract(off)
    h.lr = (float)s.lr;
    h.decay = (float)(1.0 - s.lr * s.weight_decay);
    h.b1 = (float)s.beta1;
    h.omb1 = (float)(1.0 - s.beta1);
    h.b2 = (float)s.beta2;
    h.omb2 = (float)(1.0 - s.beta2);
    h.eps = (float)s.eps;
    return s.lr >= 0.0 && s.eps >= 0.0 && s.weight_decay >= 0.0 && s.beta1 >= 0.0 && s.beta1 < 1.0 && s.beta2 >= 0.0 && s.beta2 < 1.0;
}

// the other optimizers on this machinery (see "SGD and LAMB" below).  Their derived values use the same arrays: SGD keeps the
// weight decay itself in `decay`, the momentum in b1 and nesterov (0 / 1) in b2; LAMB is AdamW's set with the weight decay itself
enum { OPT_ADAMW = 0, OPT_SGD = 1, OPT_LAMB = 2 };
static_assert(sizeof(mtlora_sgd_group) == sizeof(mtlora_adamw_group) && __builtin_offsetof(mtlora_sgd_group, momentum) == __builtin_offsetof(mtlora_adamw_group, beta1) &&
                  __builtin_offsetof(mtlora_sgd_group, nesterov) == __builtin_offsetof(mtlora_adamw_group, beta2) &&
                  __builtin_offsetof(mtlora_sgd_group, weight_decay) == __builtin_offsetof(mtlora_adamw_group, weight_decay),
              "an SGD record is read through the AdamW record's fields: beta1 = momentum, beta2 = nesterov");
template <int ALG>
__host__ __device__ inline bool opt_derive_as(const mtlora_adamw_group& s, OptHyper& h) {
    if constexpr (ALG == OPT_ADAMW) return opt_derive(s, h);
    if constexpr (ALG == OPT_SGD) {
        h.lr = (float)s.lr;
        h.decay = (float)s.weight_decay;
        h.b1 = (float)s.beta1;
        h.b2 = s.beta2 != 0.0 ? 1.f : 0.f;
        h.omb1 = h.omb2 = h.eps = 0.f;
        return s.lr >= 0.0 && s.weight_decay >= 0.0 && s.beta1 >= 0.0 && (s.beta2 == 0.0 || s.beta2 == 1.0);
    }
    const bool ok = opt_derive(s, h);  // LAMB
    h.decay = (float)s.weight_decay;
    return ok;
}

// the schedule buffer of mtlora_adamw_sched_update_dev
struct OptSched {
    mtlora_lr_schedule rec;
    int64_t u;  // update calls made so far
    double lr_used[OPT_MAXG];
};
static_assert(sizeof(mtlora_lr_schedule) == MTLORA_ADAMW_SCHED_COUNT_OFFSET && __builtin_offsetof(OptSched, u) == MTLORA_ADAMW_SCHED_COUNT_OFFSET &&
                  __builtin_offsetof(OptSched, lr_used) == MTLORA_ADAMW_SCHED_LR_OFFSET && sizeof(OptSched) == MTLORA_ADAMW_SCHED_DEV_BYTES,
              "schedule buffer layout");

// what the host checks before it uploads a record and the kernel checks again on the record it finds (fields are read in place:
// the record is never copied into registers, so the milestone loop indexes memory, not a private array)
__host__ __device__ inline bool opt_sched_ok(const mtlora_lr_schedule& s, int n_groups) {
    bool ok = s.warmup_t >= 0 && s.warmup_lr_init >= 0.0;  // (a comparison with nan is false)
    for (int g = 0; g < n_groups; ++g) ok = ok && s.base_lr[g] >= 0.0;
    switch (s.kind) {
        case MTLORA_LR_COSINE: return ok && s.t_initial > 0 && s.lr_min >= 0.0;
        case MTLORA_LR_STEP: return ok && s.decay_t > 0 && s.decay_rate >= 0.0;
        case MTLORA_LR_LINEAR: return ok && s.t_initial > s.warmup_t && s.lr_min_rate >= 0.0;
        case MTLORA_LR_MULTISTEP: {
            if (!(ok && s.gamma >= 0.0 && s.n_milestones >= 0 && s.n_milestones <= MTLORA_LR_MAX_MILESTONES)) return false;
            int64_t prev = s.warmup_t > 1 ? s.warmup_t : 1;  // milestones >= 1 (L(0) is the constructor's value) and >= warmup_t
            for (int64_t i = 0; i < s.n_milestones; ++i) {
                if (s.milestones[i] < prev) return false;
                prev = s.milestones[i];
            }
            return true;
        }
        default: return false;
    }
}

// L_g(t), t >= 0, of a record opt_sched_ok accepts.  Every expression is the Python class's, operation for operation
// (mtlora_amd/lr_scheduler.py); integer counts become doubles exactly (< 2^53)
__host__ __device__ inline double opt_sched_lr(const mtlora_lr_schedule& s, int g, int64_t t) {
#pragma clang fp contract(off)
    const double v = s.base_lr[g];
    if (t < s.warmup_t) return s.warmup_lr_init + (double)t * ((v - s.warmup_lr_init) / (double)s.warmup_t);
    switch (s.kind) {
        case MTLORA_LR_COSINE: {
            if (s.warmup_prefix) t -= s.warmup_t;
            const int64_t i = t / s.t_initial, t_curr = t - s.t_initial * i;
            if (i >= 1) return s.lr_min;
            return s.lr_min + 0.5 * (v - s.lr_min) * (1.0 + cos(3.141592653589793 * (double)t_curr / (double)s.t_initial));
        }
        case MTLORA_LR_STEP: return v * pow(s.decay_rate, (double)(t / s.decay_t));
        case MTLORA_LR_LINEAR: {
            t -= s.warmup_t;
            return v - ((v - v * s.lr_min_rate) * ((double)t / (double)(s.t_initial - s.warmup_t)));
        }
        default: {  // MTLORA_LR_MULTISTEP
            int passed = 0;
            for (int64_t i = 0; i < s.n_milestones; ++i) passed += s.milestones[i] <= t ? 1 : 0;
            return v * pow(s.gamma, (double)passed);
        }
    }
}

// control block words (floats), MTLORA_ADAMW_CTRL_WORDS of them
enum { OC_NORM = 0, OC_FOUND_INF = 1, OC_COEF = 2, OC_GMUL = 3, OC_STEP = 4, OC_BC = 8 };  // OC_BC + 2 g: bc1, sqrt(bc2) of group g
enum { OC_MICRO = MTLORA_ADAMW_CTRL_MICRO, OC_UPDATED = MTLORA_ADAMW_CTRL_UPDATED };  // gradient accumulation only
static_assert(OC_MICRO > OC_STEP && OC_UPDATED > OC_MICRO && OC_UPDATED < OC_BC, "control block");
static_assert(OC_BC + 2 * OPT_MAXG <= MTLORA_ADAMW_CTRL_WORDS, "control block");
enum { OC_LAMB_CLIP = MTLORA_LAMB_CTRL_CLIP };  // LAMB only: the divisor of its own max_grad_norm clip
static_assert(OC_LAMB_CLIP > OC_UPDATED && OC_LAMB_CLIP < OC_BC, "control block");

// where k_optim_step finds a tensor's gradient, and whether this launch may write at all
struct OptGradPtrs {  // the caller's gradient pointers
    const float* const* grads;
    __device__ __forceinline__ bool live(const float*) const { return true; }
    __device__ __forceinline__ const float* at(int t) const { return grads[t]; }
};
struct OptGradAcc {  // the accumulator's slices; a null gradient pointer still switches the tensor off
    const float* const* grads;
    const float* acc;
    const int64_t* off;
    __device__ __forceinline__ bool live(const float* ctrl) const { return ctrl[OC_UPDATED] != 0.f; }
    __device__ __forceinline__ const float* at(int t) const { return grads[t] ? acc + off[t] : nullptr; }
};

__device__ __forceinline__ bool opt_nonfinite(float x) { return (__builtin_bit_cast(uint32_t, x) & 0x7F800000u) == 0x7F800000u; }

// fixed-order sum (float or double) over the workgroup's 4 waves; every thread gets the same bits.  `red`: 4 words of LDS per call
template <class T>
__device__ __forceinline__ T opt_block_sum(T s, T* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// what the walk below needs of every pointer it uses to take 16-byte accesses (OR the addresses), and what the accumulating
// entries therefore ask of `acc`, whose slices all start at multiples of 4 elements
__host__ __device__ inline bool opt_aligned16(uintptr_t bits) { return (bits & 15u) == 0; }

// THE walk over one chunk, element by element: f(g, p, m, v) on registers.  A: which of g / p / m / v are read and which of
// p / m / v are written; a pointer A does not name may be null.  16-byte accesses where every pointer in use is 16-byte aligned,
// with the last n % 4 elements scalar on threads 0..3; scalar else.  A thread visits its elements in a fixed order (vector k
// ascending, lane e ascending, then the tail element): a sum f accumulates is reproducible.
enum { OS_G = 1, OS_P = 2, OS_M = 4, OS_V = 8, OS_WP = 16, OS_WM = 32, OS_WV = 64 };
template <int A, class F>
__device__ __forceinline__ void opt_stream(int n, const float* __restrict__ g, float* __restrict__ p, float* __restrict__ m,
                                           float* __restrict__ v, F f) {
    const int tid = threadIdx.x;
    uintptr_t al = 0;
    if constexpr ((A & (OS_P | OS_WP)) != 0) al |= (uintptr_t)p;
    if constexpr ((A & OS_G) != 0) al |= (uintptr_t)g;
    if constexpr ((A & (OS_M | OS_WM)) != 0) al |= (uintptr_t)m;
    if constexpr ((A & (OS_V | OS_WV)) != 0) al |= (uintptr_t)v;
    auto one = [&](int i) {
        float gg = 0.f, pp = 0.f, mm = 0.f, vv = 0.f;
        if constexpr ((A & OS_P) != 0) pp = p[i];
        if constexpr ((A & OS_G) != 0) gg = g[i];
        if constexpr ((A & OS_M) != 0) mm = m[i];
        if constexpr ((A & OS_V) != 0) vv = v[i];
        f(gg, pp, mm, vv);
        if constexpr ((A & OS_WP) != 0) p[i] = pp;
        if constexpr ((A & OS_WM) != 0) m[i] = mm;
        if constexpr ((A & OS_WV) != 0) v[i] = vv;
    };
    if (opt_aligned16(al)) {
        const int nv = n >> 2;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        f32x4 xg[OPT_VPT], xp[OPT_VPT], xm[OPT_VPT], xv[OPT_VPT];
#pragma unroll
        for (int k = 0; k < OPT_VPT; ++k) {
            const int i = k * OPT_THREADS + tid;
            xg[k] = xp[k] = xm[k] = xv[k] = zero;
            if (i < nv) {
                if constexpr ((A & OS_P) != 0) xp[k] = *reinterpret_cast<const f32x4*>(p + 4 * i);
                if constexpr ((A & OS_G) != 0) xg[k] = *reinterpret_cast<const f32x4*>(g + 4 * i);
                if constexpr ((A & OS_M) != 0) xm[k] = *reinterpret_cast<const f32x4*>(m + 4 * i);
                if constexpr ((A & OS_V) != 0) xv[k] = *reinterpret_cast<const f32x4*>(v + 4 * i);
            }
        }
#pragma unroll
        for (int k = 0; k < OPT_VPT; ++k) {
            const int i = k * OPT_THREADS + tid;
            if (i < nv) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float pp = xp[k][e], mm = xm[k][e], vv = xv[k][e];
                    f(xg[k][e], pp, mm, vv);
                    xp[k][e] = pp;
                    xm[k][e] = mm;
                    xv[k][e] = vv;
                }
                if constexpr ((A & OS_WP) != 0) *reinterpret_cast<f32x4*>(p + 4 * i) = xp[k];
                if constexpr ((A & OS_WM) != 0) *reinterpret_cast<f32x4*>(m + 4 * i) = xm[k];
                if constexpr ((A & OS_WV) != 0) *reinterpret_cast<f32x4*>(v + 4 * i) = xv[k];
            }
        }
        const int i = 4 * nv + tid;  // the last n % 4 elements
        if (tid < 4 && i < n) one(i);
    } else {
        for (int i = tid; i < n; i += OPT_THREADS) one(i);
    }
}

// the chunk this workgroup owns, of the tensor whose gradient starts at `g`: false if it has none this step (workgroup-uniform)
struct OptSlice {
    const float* g;
    float *p, *m, *v;
    int n, group;
    int64_t off, numel;  // the chunk's first element in its tensor; the tensor's size
};
__device__ __forceinline__ bool opt_slice(const OptTensor* __restrict__ tens, const OptChunk& ck, const float* g, OptSlice& s) {
    if (!g) return false;
    const OptTensor t = tens[ck.tensor];
    s.off = (int64_t)ck.index * OPT_CHUNK;
    const int64_t left = t.n - s.off;
    s.n = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
    s.g = g + s.off;
    s.p = t.p + s.off;
    s.m = t.m + s.off;
    s.v = t.v + s.off;
    s.group = t.group;
    s.numel = t.n;
    return true;
}

// partials[chunk] / flags[chunk] of the gradients as stored.  ACC: gradient accumulation -- the chunk of acc (at acc +
// acc_off[tensor]; it rides in the walk's p slot) becomes g (ctrl[OC_MICRO] == 0: whatever acc held is overwritten, never read)
// or acc + g, and the partial / flag are those of the value stored.  Each element of acc has one writer.  (waves_per_eu: the
// walk has all of a thread's g and acc vectors in flight at once; the attribute holds that within 64 VGPRs, 8 waves per SIMD.)
template <bool ACC>
__global__ __launch_bounds__(OPT_THREADS) __attribute__((amdgpu_waves_per_eu(8))) void k_optim_norm(const OptTensor* __restrict__ tens, const OptChunk* __restrict__ chunks,
                                                            const float* const* __restrict__ grads, float* __restrict__ partials,
                                                            uint32_t* __restrict__ flags, float* __restrict__ acc,
                                                            const int64_t* __restrict__ acc_off, const float* __restrict__ ctrl) {
    __shared__ float red[4];
    __shared__ int bad_any;
    const int tid = threadIdx.x;
    const OptChunk ck = chunks[blockIdx.x];
    OptSlice sl;
    if (!opt_slice(tens, ck, grads[ck.tensor], sl)) {  // no gradient this step
        if (tid == 0) {
            partials[blockIdx.x] = 0.f;
            flags[blockIdx.x] = 0u;
        }
        return;
    }
    if (tid == 0) bad_any = 0;
    float s = 0.f;
    bool bad = false;
    auto add = [&](float x) {
        s += x * x;
        bad |= opt_nonfinite(x);
    };
    if constexpr (ACC) {
        float* a = acc + acc_off[ck.tensor] + sl.off;
        if (ctrl[OC_MICRO] == 0.f)  // (workgroup-uniform; k_optim_finish, the next launch, is the one that moves it)
            opt_stream<OS_G | OS_WP>(sl.n, sl.g, a, nullptr, nullptr, [&](float g, float& x, float&, float&) { add(x = g); });
        else
            opt_stream<OS_G | OS_P | OS_WP>(sl.n, sl.g, a, nullptr, nullptr, [&](float g, float& x, float&, float&) { add(x = x + g); });
    } else {
        opt_stream<OS_G>(sl.n, sl.g, nullptr, nullptr, nullptr, [&](float g, float&, float&, float&) { add(g); });
    }
    __syncthreads();  // bad_any = 0 is visible
    if (bad) bad_any = 1;  // (LDS; every writer stores the same value)
    const float tot = opt_block_sum(s, red);  // (its barrier also orders bad_any)
    if (tid == 0) {
        partials[blockIdx.x] = tot;
        flags[blockIdx.x] = bad_any ? 1u : 0u;
    }
}

// G: OptGroups (by value) or OptGroupsDev.  ACC: gradient accumulation over accum_steps micro-steps -- ctrl[OC_MICRO] decides, on
// the device, whether this call is the cycle's last; if it is not, the counter moves and NOTHING else is written.  SCHED (with
// OptGroupsDev and ACC): an update call takes each group's lr from the schedule in `sch` and counts itself there.  ALG: whose
// records these are -- SGD has no bias corrections; LAMB folds its own clip at `lamb_max_norm` (of the norm AFTER the max_norm
// clip) into ctrl[OC_GMUL].
template <class G, bool ACC, bool SCHED = false, int ALG = OPT_ADAMW>
__global__ __launch_bounds__(OPT_THREADS) void k_optim_finish(const float* __restrict__ partials, const uint32_t* __restrict__ flags,
                                                              int n_chunks, const G grp, float max_norm, float* __restrict__ ctrl,
                                                              float* __restrict__ norm_out, float* __restrict__ scale,
                                                              int32_t* __restrict__ tracker, float growth, float backoff, int interval,
                                                              int accum_steps, OptSched* __restrict__ sch, float lamb_max_norm) {
    static_assert(!SCHED || (ACC && __is_same(G, OptGroupsDev)), "the schedule rides on the accumulating device-record entry");
    static_assert(ALG == OPT_ADAMW || (!ACC && !SCHED), "accumulation and the schedule are AdamW's");
    __shared__ double red[OPT_THREADS];
    __shared__ uint32_t fl[OPT_THREADS];
    __shared__ float step_new;
    const int tid = threadIdx.x;
    if constexpr (ACC) {
        const float c = ctrl[OC_MICRO];
        __syncthreads();  // every thread has read c before thread 0 moves it
        if (c + 1.f < (float)accum_steps) {  // (workgroup-uniform; accum_steps <= 2^24, so the floats are exact)
            if (tid == 0) {
                ctrl[OC_MICRO] = c + 1.f;
                ctrl[OC_UPDATED] = 0.f;
            }
            return;
        }
    }
    double s = 0.0;
    uint32_t f = 0u;
    double b1d = 0.0, b2d = 0.0;
    int64_t u = 0;
    if (tid < grp.n) {
        if constexpr (__is_same(G, OptGroupsDev)) {
            mtlora_adamw_group r = grp.rec[tid];
            if constexpr (SCHED) {  // the reference steps its scheduler AFTER the optimizer: update n >= 1 runs at L(n - 1), update 0 at L(0)
                u = sch->u;  // (thread 0 moves it behind the barrier below)
                const bool ok = u >= 0 && opt_sched_ok(sch->rec, grp.n);
                r.lr = ok ? opt_sched_lr(sch->rec, tid, u > 0 ? u - 1 : 0) : (double)__builtin_nanf("");  // nan: opt_derive rejects it
                sch->lr_used[tid] = r.lr;
            }
            OptHyper h;
            if (!opt_derive_as<ALG>(r, h)) f = 1u;  // what the host entry rejects: found_inf, a skipped step
            opt_put(*grp.hyp, tid, h);
            b1d = r.beta1;
            b2d = r.beta2;
        } else {
            b1d = grp.b1d[tid];
            b2d = grp.b2d[tid];
        }
    }
    const uint32_t bad_hyper = f;
    for (int i = tid; i < n_chunks; i += OPT_THREADS) {
        s += (double)partials[i];
        f |= flags[i];
    }
    red[tid] = s;
    fl[tid] = f | (bad_hyper << 1);
    __syncthreads();
    for (int w = OPT_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) {
            red[tid] += red[tid + w];
            fl[tid] |= fl[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const bool found = fl[0] != 0u;
        const float sc = scale ? *scale : 1.f;
        const float inv = (float)(1.0 / (double)sc);  // GradScaler.unscale_: the reciprocal in double, applied in fp32
        const float norm = (fl[0] & 2u) ? __builtin_nanf("") : (float)(sqrt(red[0]) * (double)inv);
        const float coef = max_norm > 0.f ? fminf(1.f, max_norm / (norm + 1e-6f)) : 1.f;  // clip_grad_norm_
        const float st = ctrl[OC_STEP] + (found ? 0.f : 1.f);
        ctrl[OC_NORM] = norm;
        ctrl[OC_FOUND_INF] = found ? 1.f : 0.f;
        ctrl[OC_COEF] = coef;
        if constexpr (ALG == OPT_LAMB) {
            const float n2 = norm * coef;  // (a nan norm compares false: c = 1, and the step is skipped anyway)
            const float c = lamb_max_norm > 0.f && n2 > lamb_max_norm ? n2 / lamb_max_norm : 1.f;
            ctrl[OC_LAMB_CLIP] = c;
            ctrl[OC_GMUL] = coef * inv / c;
        } else {
            ctrl[OC_GMUL] = coef * inv;
        }
        ctrl[OC_STEP] = st;
        if constexpr (ACC) {  // the cycle ends here, whether the step was taken or skipped
            ctrl[OC_MICRO] = 0.f;
            ctrl[OC_UPDATED] = 1.f;
        }
        if constexpr (SCHED) sch->u = u + 1;  // an update CALL, taken or skipped
        step_new = st;
        if (norm_out) *norm_out = norm;
        if (scale) {  // GradScaler.update (ATen amp_update_scale)
            if (found) {
                *scale = sc * backoff;
                *tracker = 0;
            } else {
                const int ok = *tracker + 1;
                if (ok == interval) {
                    const float grown = sc * growth;
                    if (!opt_nonfinite(grown)) *scale = grown;
                    *tracker = 0;
                } else {
                    *tracker = ok;
                }
            }
        }
    }
    if constexpr (ALG == OPT_SGD) return;  // no bias corrections
    __syncthreads();
    if (tid < grp.n) {
        const double t = (double)step_new;
        ctrl[OC_BC + 2 * tid] = (float)(1.0 - pow(b1d, t));
        ctrl[OC_BC + 2 * tid + 1] = (float)sqrt(1.0 - pow(b2d, t));
    }
}

struct OptCoef {
    float gmul, decay, b1, omb1, b2, omb2, step_size, inv_bc2s, eps;
};

__device__ __forceinline__ void opt_adamw(float& p, float g, float& m, float& v, const OptCoef& c) {
    g *= c.gmul;
    p *= c.decay;
    m = c.b1 * m + c.omb1 * g;
    v = c.b2 * v + c.omb2 * g * g;
    p -= c.step_size * (m / (sqrtf(v) * c.inv_bc2s + c.eps));
}

template <class G, class S>  // S: OptGradPtrs or OptGradAcc
__global__ __launch_bounds__(OPT_THREADS) void k_optim_step(const OptTensor* __restrict__ tens, const OptChunk* __restrict__ chunks,
                                                            const S src, const float* __restrict__ ctrl, const G grp) {
    if (!src.live(ctrl)) return;            // an accumulating micro-step: nothing is written (ctrl[OC_FOUND_INF] is the last update's)
    if (ctrl[OC_FOUND_INF] != 0.f) return;  // skipped step: nothing is written
    const OptChunk ck = chunks[blockIdx.x];
    OptSlice s;
    if (!opt_slice(tens, ck, src.at(ck.tensor), s)) return;
    const int gi = s.group;
    const OptHyperArr& h = opt_hyper(grp);
    OptCoef c;
    c.gmul = ctrl[OC_GMUL];
    c.decay = h.decay[gi];
    c.b1 = h.b1[gi];
    c.omb1 = h.omb1[gi];
    c.b2 = h.b2[gi];
    c.omb2 = h.omb2[gi];
    c.step_size = h.lr[gi] / ctrl[OC_BC + 2 * gi];
    c.inv_bc2s = 1.f / ctrl[OC_BC + 2 * gi + 1];
    c.eps = h.eps[gi];
    // NOT on opt_stream: there the compiler contracts opt_adamw's multiplies and adds into other fused multiply-adds than here
    // (m, v and p then differ in the last bits from the second step on: tools/optim_digest.py).  The walk below is
    // opt_stream<OS_G | OS_P | OS_M | OS_V | OS_WP | OS_WM | OS_WV>'s, statement for statement
    const int tid = threadIdx.x, n = s.n;
    const float* g = s.g;
    float *p = s.p, *m = s.m, *v = s.v;
    if (opt_aligned16((uintptr_t)g | (uintptr_t)p | (uintptr_t)m | (uintptr_t)v)) {
        const int nv = n >> 2;
        f32x4 xg[OPT_VPT], xp[OPT_VPT], xm[OPT_VPT], xv[OPT_VPT];
#pragma unroll
        for (int k = 0; k < OPT_VPT; ++k) {
            const int i = k * OPT_THREADS + tid;
            if (i < nv) {
                xg[k] = *reinterpret_cast<const f32x4*>(g + 4 * i);
                xp[k] = *reinterpret_cast<const f32x4*>(p + 4 * i);
                xm[k] = *reinterpret_cast<const f32x4*>(m + 4 * i);
                xv[k] = *reinterpret_cast<const f32x4*>(v + 4 * i);
            }
        }
#pragma unroll
        for (int k = 0; k < OPT_VPT; ++k) {
            const int i = k * OPT_THREADS + tid;
            if (i < nv) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float pp = xp[k][e], mm = xm[k][e], vv = xv[k][e];
                    opt_adamw(pp, xg[k][e], mm, vv, c);
                    xp[k][e] = pp;
                    xm[k][e] = mm;
                    xv[k][e] = vv;
                }
                *reinterpret_cast<f32x4*>(p + 4 * i) = xp[k];
                *reinterpret_cast<f32x4*>(m + 4 * i) = xm[k];
                *reinterpret_cast<f32x4*>(v + 4 * i) = xv[k];
            }
        }
        const int i = 4 * nv + tid;  // the last n % 4 elements
        if (tid < 4 && i < n) {
            float pp = p[i], mm = m[i], vv = v[i];
            opt_adamw(pp, g[i], mm, vv, c);
            p[i] = pp;
            m[i] = mm;
            v[i] = vv;
        }
    } else {
        for (int i = tid; i < n; i += OPT_THREADS) {
            float pp = p[i], mm = m[i], vv = v[i];
            opt_adamw(pp, g[i], mm, vv, c);
            p[i] = pp;
            m[i] = mm;
            v[i] = vv;
        }
    }
}

// ---- SGD and LAMB (optimizer.py:53-66: the reference's `sgd` and `fused_lamb`) -----------------------------------------------
// The same table, chunk grid, gradient-pointer array, k_optim_norm and k_optim_finish (ALG picks the record's meaning); what
// follows the finish launch is:
//   k_sgd_step      torch.optim.SGD(momentum = mu, dampening = 0, nesterov): g' = g gmul + wd p;  m = mu m + g';
//                   p -= lr (nesterov ? g' + mu m : m).  mu == 0: p -= lr g' and m is not touched.  v is never touched.
//   k_lamb_moments  g = g gmul (gmul carries both clips);  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2, stored;
//                   u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps) + wd p;  pn[chunk] = sum p^2, un[chunk] = sum u^2 (one workgroup
//                   owns both words).  p is only read.
//   k_lamb_apply    every workgroup adds the partials of ITS tensor's chunks (a tensor's chunks are consecutive and a chunk never
//                   spans tensors) in double in a fixed order -- all workgroups of a tensor get the same bits --, forms the trust
//                   ratio, forms u AGAIN from the stored m, v and the p that nothing has written yet (12 bytes read per element
//                   instead of 4 written and 4 read for a stored u, and no buffer the size of the parameters), and p -= ratio u.
// All three leave on found_inf before they read or write anything else.

template <class G>
__global__ __launch_bounds__(OPT_THREADS) void k_sgd_step(const OptTensor* __restrict__ tens, const OptChunk* __restrict__ chunks,
                                                          const float* const* __restrict__ grads, const float* __restrict__ ctrl,
                                                          const G grp) {
    if (ctrl[OC_FOUND_INF] != 0.f) return;  // skipped step: nothing is written
    const OptChunk ck = chunks[blockIdx.x];
    OptSlice s;
    if (!opt_slice(tens, ck, grads[ck.tensor], s)) return;
    const OptHyperArr& h = opt_hyper(grp);
    const float gmul = ctrl[OC_GMUL], lr = h.lr[s.group], wd = h.decay[s.group], mu = h.b1[s.group];
    const bool nesterov = h.b2[s.group] != 0.f;
    if (mu == 0.f) {  // (workgroup-uniform) no momentum: no buffer
        opt_stream<OS_G | OS_P | OS_WP>(s.n, s.g, s.p, nullptr, nullptr, [&](float g, float& p, float&, float&) {
            g = g * gmul + wd * p;
            p -= lr * g;
        });
    } else {
        opt_stream<OS_G | OS_P | OS_M | OS_WP | OS_WM>(s.n, s.g, s.p, s.m, nullptr, [&](float g, float& p, float& m, float&) {
            g = g * gmul + wd * p;
            m = mu * m + g;
            p -= lr * (nesterov ? g + mu * m : m);
        });
    }
}

struct LambCoef {
    float gmul, wd, b1, omb1, b2, omb2, inv_bc1, inv_bc2s, eps;
};
template <class G>
__device__ __forceinline__ LambCoef lamb_coef(const float* __restrict__ ctrl, const G& grp, int gi) {
    const OptHyperArr& h = opt_hyper(grp);
    LambCoef c;
    c.gmul = ctrl[OC_GMUL];
    c.wd = h.decay[gi];
    c.b1 = h.b1[gi];
    c.omb1 = h.omb1[gi];
    c.b2 = h.b2[gi];
    c.omb2 = h.omb2[gi];
    c.inv_bc1 = 1.f / ctrl[OC_BC + 2 * gi];
    c.inv_bc2s = 1.f / ctrl[OC_BC + 2 * gi + 1];
    c.eps = h.eps[gi];
    return c;
}
// the one expression both LAMB kernels form u with
__device__ __forceinline__ float lamb_u(float p, float m, float v, const LambCoef& c) {
    return (m * c.inv_bc1) / (sqrtf(v) * c.inv_bc2s + c.eps) + c.wd * p;
}

template <class G>
__global__ __launch_bounds__(OPT_THREADS) void k_lamb_moments(const OptTensor* __restrict__ tens, const OptChunk* __restrict__ chunks,
                                                              const float* const* __restrict__ grads, const float* __restrict__ ctrl,
                                                              const G grp, float* __restrict__ pn, float* __restrict__ un) {
    __shared__ float red_p[4], red_u[4];
    if (ctrl[OC_FOUND_INF] != 0.f) return;  // skipped step: m and v stay as they are (and launch 4 reads no partial)
    const OptChunk ck = chunks[blockIdx.x];
    OptSlice s;
    if (!opt_slice(tens, ck, grads[ck.tensor], s)) return;
    const LambCoef c = lamb_coef(ctrl, grp, s.group);
    float sp = 0.f, su = 0.f;
    opt_stream<OS_G | OS_P | OS_M | OS_V | OS_WM | OS_WV>(s.n, s.g, s.p, s.m, s.v, [&](float g, float& p, float& m, float& v) {
        g *= c.gmul;
        m = c.b1 * m + c.omb1 * g;
        v = c.b2 * v + c.omb2 * g * g;
        const float u = lamb_u(p, m, v, c);
        sp += p * p;
        su += u * u;
    });
    const float tp = opt_block_sum(sp, red_p), tu = opt_block_sum(su, red_u);
    if (threadIdx.x == 0) {
        pn[blockIdx.x] = tp;
        un[blockIdx.x] = tu;
    }
}

template <class G>
__global__ __launch_bounds__(OPT_THREADS) void k_lamb_apply(const OptTensor* __restrict__ tens, const OptChunk* __restrict__ chunks,
                                                            const float* const* __restrict__ grads, const float* __restrict__ ctrl,
                                                            const G grp, const float* __restrict__ pn, const float* __restrict__ un,
                                                            int use_nvlamb) {
    __shared__ double red_p[4], red_u[4];
    if (ctrl[OC_FOUND_INF] != 0.f) return;
    const OptChunk ck = chunks[blockIdx.x];
    OptSlice s;
    if (!opt_slice(tens, ck, grads[ck.tensor], s)) return;
    const int first = (int)blockIdx.x - ck.index;                  // the tensor's chunks are [first, first + cnt)
    const int cnt = (int)((s.numel + OPT_CHUNK - 1) / OPT_CHUNK);  // (< 2^31: opt_count)
    double sp = 0.0, su = 0.0;
    for (int i = threadIdx.x; i < cnt; i += OPT_THREADS) {
        sp += (double)pn[first + i];
        su += (double)un[first + i];
    }
    const float pnorm = (float)sqrt(opt_block_sum(sp, red_p)), unorm = (float)sqrt(opt_block_sum(su, red_u));
    const LambCoef c = lamb_coef(ctrl, grp, s.group);
    const float lr = opt_hyper(grp).lr[s.group];
    const float ratio = ((c.wd != 0.f || use_nvlamb) && pnorm != 0.f && unorm != 0.f) ? lr * (pnorm / unorm) : lr;
    opt_stream<OS_P | OS_M | OS_V | OS_WP>(s.n, nullptr, s.p, s.m, s.v,
                                    [&](float, float& p, float& m, float& v) { p -= ratio * lamb_u(p, m, v, c); });
}

static int opt_count(int64_t n_tensors, const int64_t* numel, int64_t* n_chunks) {
    if (n_tensors <= 0 || n_tensors >= ((int64_t)1 << 31)) return MTLORA_ERR_SHAPE;
    if (!numel) return MTLORA_ERR_NULL;
    int64_t nc = 0;
    for (int64_t i = 0; i < n_tensors; ++i) {
        if (numel[i] < 0 || numel[i] >= ((int64_t)1 << 42)) return MTLORA_ERR_SHAPE;
        nc += mtl_ceil_div(numel[i], OPT_CHUNK);
    }
    if (nc >= ((int64_t)1 << 31)) return MTLORA_ERR_SHAPE;
    *n_chunks = nc;
    return MTLORA_OK;
}

// the arguments of an update entry: what all seven have, then LAMB's two, then the accumulating entries' (accum_steps >= 1; 0: the
// entry does not accumulate) and the scheduled entry's buffer
struct OptCall {
    const void *table, *grads;
    int64_t n_tensors, n_chunks;
    const mtlora_adamw_group* groups;  // host records, or device records (an SGD record is read through the AdamW record's fields)
    int n_groups;
    float max_norm, *ctrl, *norm_out, *scale;
    int32_t* tracker;
    float growth, backoff;
    int interval;
    void* scratch;
    int64_t scratch_bytes;
    void* stream;
    float lamb_max_norm = 0.f;
    int use_nvlamb = 0;
    float* acc = nullptr;
    const int64_t* acc_off = nullptr;
    int accum_steps = 0;
    OptSched* sch = nullptr;
};

// argument checks shared by the update entries, before any launch
template <int ALG>
static int opt_check(const OptCall& a) {
    if (a.n_tensors <= 0 || a.n_tensors >= ((int64_t)1 << 31) || a.n_chunks < 0 || a.n_chunks >= ((int64_t)1 << 31)) return MTLORA_ERR_SHAPE;
    if (a.n_groups < 1 || a.n_groups > OPT_MAXG) return MTLORA_ERR_UNSUPPORTED;
    if (!a.table || !a.grads || !a.groups || !a.ctrl || !a.scratch) return MTLORA_ERR_NULL;
    if ((a.scale == nullptr) != (a.tracker == nullptr)) return MTLORA_ERR_NULL;
    if (((uintptr_t)a.table | (uintptr_t)a.grads | (uintptr_t)a.scratch) & 7u) return MTLORA_ERR_ALIGN;
    if (((uintptr_t)a.ctrl | (uintptr_t)a.norm_out | (uintptr_t)a.scale | (uintptr_t)a.tracker) & 3u) return MTLORA_ERR_ALIGN;
    if (a.scratch_bytes < a.n_chunks * 8) return MTLORA_ERR_WORKSPACE;
    if (a.scale && (a.interval < 1 || !(a.growth > 1.f) || !(a.backoff > 0.f && a.backoff < 1.f))) return MTLORA_ERR_SHAPE;
    if constexpr (ALG == OPT_LAMB) {
        if (a.scratch_bytes < a.n_chunks * 16) return MTLORA_ERR_WORKSPACE;  // two more words per chunk: |p|^2, |u|^2
        if (!(a.lamb_max_norm == a.lamb_max_norm)) return MTLORA_ERR_SHAPE;
    }
    return MTLORA_OK;
}

// THE host path of the update entries, behind opt_check and the entry's own checks: the kernels' groups argument G -- OptGroups,
// derived here from the host records, or OptGroupsDev, the device records k_optim_finish derives from -- and the launches of
// algorithm ALG: norm, finish, and its step kernel(s).  a.accum_steps >= 1 (AdamW on device records only): one micro-step of a
// cycle of accum_steps.  With accum_steps == 1 every call is the cycle's last and updates straight from the caller's gradients:
// acc is not touched, and the bits are the plain entry's.  a.sch: the schedule buffer, or null -- the same launches either way,
// only k_optim_finish differs.
template <int ALG, class G>
static int opt_update(const OptCall& a) {
    G g = {};
    g.n = a.n_groups;
    if constexpr (__is_same(G, OptGroupsDev)) {
        if ((uintptr_t)a.groups & 7u) return MTLORA_ERR_ALIGN;
        g.rec = a.groups;  // the records are only read; the tail behind them is the library's
        g.hyp = reinterpret_cast<OptHyperArr*>(const_cast<mtlora_adamw_group*>(a.groups) + OPT_MAXG);
    } else {
        for (int i = 0; i < a.n_groups; ++i) {
            OptHyper h;
            if (!opt_derive_as<ALG>(a.groups[i], h)) return MTLORA_ERR_SHAPE;
            opt_put(g.h, i, h);
            g.b1d[i] = a.groups[i].beta1;  // (the bias corrections; SGD's finish does not read them)
            g.b2d[i] = a.groups[i].beta2;
        }
    }
    constexpr bool CYCLE = ALG == OPT_ADAMW && __is_same(G, OptGroupsDev);  // the entries with a micro-step counter
    hipStream_t s = reinterpret_cast<hipStream_t>(a.stream);
    const OptTensor* te = reinterpret_cast<const OptTensor*>(a.table);
    const OptChunk* ce = reinterpret_cast<const OptChunk*>(te + a.n_tensors);
    const float* const* gp = reinterpret_cast<const float* const*>(a.grads);
    float* partials = reinterpret_cast<float*>(a.scratch);
    uint32_t* flags = reinterpret_cast<uint32_t*>(partials + a.n_chunks);
    const float* ctrl = a.ctrl;
    const dim3 grid((unsigned)a.n_chunks), block(OPT_THREADS);
    const bool sum = a.accum_steps > 1;
    if (a.n_chunks > 0) {
        if (sum)
            hipLaunchKernelGGL(k_optim_norm<true>, grid, block, 0, s, te, ce, gp, partials, flags, a.acc, a.acc_off, ctrl);
        else
            hipLaunchKernelGGL(k_optim_norm<false>, grid, block, 0, s, te, ce, gp, partials, flags, (float*)nullptr, (const int64_t*)nullptr,
                               (const float*)nullptr);
    }
    auto* finish = k_optim_finish<G, false, false, ALG>;
    if constexpr (CYCLE) {
        if (a.sch)
            finish = k_optim_finish<G, true, true>;
        else if (a.accum_steps > 0)
            finish = k_optim_finish<G, true>;
    }
    hipLaunchKernelGGL(finish, dim3(1), block, 0, s, partials, flags, (int)a.n_chunks, g, a.max_norm, a.ctrl, a.norm_out, a.scale, a.tracker,
                       a.growth, a.backoff, a.interval, a.accum_steps, a.sch, a.lamb_max_norm);
    if (a.n_chunks > 0) {
        if constexpr (ALG == OPT_SGD) {
            hipLaunchKernelGGL((k_sgd_step<G>), grid, block, 0, s, te, ce, gp, ctrl, g);
        } else if constexpr (ALG == OPT_LAMB) {
            float* pn = reinterpret_cast<float*>(flags + a.n_chunks);  // the scratch's second half: [n_chunks] |p|^2, [n_chunks] |u|^2
            float* un = pn + a.n_chunks;
            hipLaunchKernelGGL((k_lamb_moments<G>), grid, block, 0, s, te, ce, gp, ctrl, g, pn, un);
            hipLaunchKernelGGL((k_lamb_apply<G>), grid, block, 0, s, te, ce, gp, ctrl, g, (const float*)pn, (const float*)un, a.use_nvlamb);
        } else {
            if constexpr (CYCLE)
                if (sum) hipLaunchKernelGGL((k_optim_step<G, OptGradAcc>), grid, block, 0, s, te, ce, OptGradAcc{gp, a.acc, a.acc_off}, ctrl, g);
            if (!sum) hipLaunchKernelGGL((k_optim_step<G, OptGradPtrs>), grid, block, 0, s, te, ce, OptGradPtrs{gp}, ctrl, g);
        }
    }
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

}  // namespace

extern "C" {

int mtlora_adamw_sizes(int64_t n_tensors, const int64_t* numel, int64_t* n_chunks, int64_t* table_bytes, int64_t* scratch_bytes) {
    if (!n_chunks || !table_bytes || !scratch_bytes) return MTLORA_ERR_NULL;
    int64_t nc = 0;
    const int rc = opt_count(n_tensors, numel, &nc);
    if (rc != MTLORA_OK) return rc;
    *n_chunks = nc;
    *table_bytes = n_tensors * (int64_t)sizeof(OptTensor) + nc * (int64_t)sizeof(OptChunk);
    *scratch_bytes = nc * 8;  // partials (fp32) + flags
    return MTLORA_OK;
}

int mtlora_adamw_table(int64_t n_tensors, const int64_t* numel, const int32_t* group, void* const* p, void* const* m, void* const* v,
                       void* host_table, int64_t table_bytes) {
    int64_t nc = 0;
    const int rc = opt_count(n_tensors, numel, &nc);
    if (rc != MTLORA_OK) return rc;
    if (!group || !p || !m || !v || !host_table) return MTLORA_ERR_NULL;
    if (table_bytes < n_tensors * (int64_t)sizeof(OptTensor) + nc * (int64_t)sizeof(OptChunk)) return MTLORA_ERR_WORKSPACE;
    OptTensor* te = reinterpret_cast<OptTensor*>(host_table);
    OptChunk* ce = reinterpret_cast<OptChunk*>(te + n_tensors);
    int64_t c = 0;
    for (int64_t i = 0; i < n_tensors; ++i) {
        if (group[i] < 0 || group[i] >= OPT_MAXG) return MTLORA_ERR_SHAPE;
        if (numel[i] > 0 && (!p[i] || !m[i] || !v[i])) return MTLORA_ERR_NULL;
        if (((uintptr_t)p[i] | (uintptr_t)m[i] | (uintptr_t)v[i]) & 3u) return MTLORA_ERR_ALIGN;
        te[i].p = reinterpret_cast<float*>(p[i]);
        te[i].m = reinterpret_cast<float*>(m[i]);
        te[i].v = reinterpret_cast<float*>(v[i]);
        te[i].n = numel[i];
        te[i].group = group[i];
        te[i].pad_ = 0;
        const int64_t k = mtl_ceil_div(numel[i], OPT_CHUNK);
        for (int64_t j = 0; j < k; ++j, ++c) {
            ce[c].tensor = (int32_t)i;
            ce[c].index = (int32_t)j;
        }
    }
    return MTLORA_OK;
}

int mtlora_adamw_update(const void* table, const void* grads, int64_t n_tensors, int64_t n_chunks, const mtlora_adamw_group* groups,
                        int n_groups, float max_norm, float* ctrl, float* norm_out, float* scale, int32_t* growth_tracker,
                        float growth_factor, float backoff_factor, int growth_interval, void* scratch, int64_t scratch_bytes,
                        void* stream) {
    const OptCall a = {table, grads, n_tensors, n_chunks, groups, n_groups, max_norm, ctrl, norm_out, scale, growth_tracker,
                       growth_factor, backoff_factor, growth_interval, scratch, scratch_bytes, stream};
    const int rc = opt_check<OPT_ADAMW>(a);
    return rc != MTLORA_OK ? rc : opt_update<OPT_ADAMW, OptGroups>(a);
}

int mtlora_adamw_update_dev(const void* table, const void* grads, int64_t n_tensors, int64_t n_chunks,
                            const mtlora_adamw_group* groups_dev, int n_groups, float max_norm, float* ctrl, float* norm_out, float* scale,
                            int32_t* growth_tracker, double growth_factor, double backoff_factor, int growth_interval, void* scratch,
                            int64_t scratch_bytes, void* stream) {
    const OptCall a = {table, grads, n_tensors, n_chunks, groups_dev, n_groups, max_norm, ctrl, norm_out, scale, growth_tracker,
                       (float)growth_factor, (float)backoff_factor, growth_interval, scratch, scratch_bytes, stream};
    const int rc = opt_check<OPT_ADAMW>(a);
    return rc != MTLORA_OK ? rc : opt_update<OPT_ADAMW, OptGroupsDev>(a);
}

// SGD's records have the AdamW record's layout (see opt_derive_as)
int mtlora_sgd_update(const void* table, const void* grads, int64_t n_tensors, int64_t n_chunks, const mtlora_sgd_group* groups,
                      int n_groups, float max_norm, float* ctrl, float* norm_out, float* scale, int32_t* growth_tracker,
                      float growth_factor, float backoff_factor, int growth_interval, void* scratch, int64_t scratch_bytes, void* stream) {
    const OptCall a = {table, grads, n_tensors, n_chunks, reinterpret_cast<const mtlora_adamw_group*>(groups), n_groups, max_norm, ctrl,
                       norm_out, scale, growth_tracker, growth_factor, backoff_factor, growth_interval, scratch, scratch_bytes, stream};
    const int rc = opt_check<OPT_SGD>(a);
    return rc != MTLORA_OK ? rc : opt_update<OPT_SGD, OptGroups>(a);
}

int mtlora_sgd_update_dev(const void* table, const void* grads, int64_t n_tensors, int64_t n_chunks, const mtlora_sgd_group* groups_dev,
                          int n_groups, float max_norm, float* ctrl, float* norm_out, float* scale, int32_t* growth_tracker,
                          double growth_factor, double backoff_factor, int growth_interval, void* scratch, int64_t scratch_bytes,
                          void* stream) {
    const OptCall a = {table, grads, n_tensors, n_chunks, reinterpret_cast<const mtlora_adamw_group*>(groups_dev), n_groups, max_norm, ctrl,
                       norm_out, scale, growth_tracker, (float)growth_factor, (float)backoff_factor, growth_interval, scratch, scratch_bytes,
                       stream};
    const int rc = opt_check<OPT_SGD>(a);
    return rc != MTLORA_OK ? rc : opt_update<OPT_SGD, OptGroupsDev>(a);
}

int mtlora_lamb_update(const void* table, const void* grads, int64_t n_tensors, int64_t n_chunks, const mtlora_adamw_group* groups,
                       int n_groups, float max_norm, float max_grad_norm, int use_nvlamb, float* ctrl, float* norm_out, float* scale,
                       int32_t* growth_tracker, float growth_factor, float backoff_factor, int growth_interval, void* scratch,
                       int64_t scratch_bytes, void* stream) {
    const OptCall a = {table, grads, n_tensors, n_chunks, groups, n_groups, max_norm, ctrl, norm_out, scale, growth_tracker,
                       growth_factor, backoff_factor, growth_interval, scratch, scratch_bytes, stream, max_grad_norm, use_nvlamb != 0};
    const int rc = opt_check<OPT_LAMB>(a);
    return rc != MTLORA_OK ? rc : opt_update<OPT_LAMB, OptGroups>(a);
}

int mtlora_lamb_update_dev(const void* table, const void* grads, int64_t n_tensors, int64_t n_chunks, const mtlora_adamw_group* groups_dev,
                           int n_groups, float max_norm, float max_grad_norm, int use_nvlamb, float* ctrl, float* norm_out, float* scale,
                           int32_t* growth_tracker, double growth_factor, double backoff_factor, int growth_interval, void* scratch,
                           int64_t scratch_bytes, void* stream) {
    const OptCall a = {table, grads, n_tensors, n_chunks, groups_dev, n_groups, max_norm, ctrl, norm_out, scale, growth_tracker,
                       (float)growth_factor, (float)backoff_factor, growth_interval, scratch, scratch_bytes, stream, max_grad_norm,
                       use_nvlamb != 0};
    const int rc = opt_check<OPT_LAMB>(a);
    return rc != MTLORA_OK ? rc : opt_update<OPT_LAMB, OptGroupsDev>(a);
}

int mtlora_adamw_accum_layout(int64_t n_tensors, const int64_t* numel, int64_t* host_offsets, int64_t* acc_elems) {
    if (!acc_elems) return MTLORA_ERR_NULL;
    int64_t nc = 0;
    const int rc = opt_count(n_tensors, numel, &nc);
    if (rc != MTLORA_OK) return rc;
    int64_t total = 0;
    for (int64_t i = 0; i < n_tensors; ++i) {
        if (host_offsets) host_offsets[i] = total;
        total += mtl_ceil_div(numel[i], (int64_t)4) * 4;  // every slice starts 16-byte aligned
    }
    *acc_elems = total;
    return MTLORA_OK;
}

int mtlora_adamw_accum_update_dev(const void* table, const void* grads, int64_t n_tensors, int64_t n_chunks,
                                  const mtlora_adamw_group* groups_dev, int n_groups, float max_norm, float* ctrl, float* norm_out,
                                  float* scale, int32_t* growth_tracker, double growth_factor, double backoff_factor, int growth_interval,
                                  void* scratch, int64_t scratch_bytes, float* acc, const int64_t* acc_offsets, int accum_steps,
                                  void* stream) {
    const OptCall a = {table, grads, n_tensors, n_chunks, groups_dev, n_groups, max_norm, ctrl, norm_out, scale, growth_tracker,
                       (float)growth_factor, (float)backoff_factor, growth_interval, scratch, scratch_bytes, stream, 0.f, 0, acc, acc_offsets,
                       accum_steps};
    const int rc = opt_check<OPT_ADAMW>(a);
    if (rc != MTLORA_OK) return rc;
    if (!acc || !acc_offsets) return MTLORA_ERR_NULL;
    if (accum_steps < 1 || accum_steps > MTLORA_ADAMW_MAX_ACCUM_STEPS) return MTLORA_ERR_SHAPE;
    if (((uintptr_t)groups_dev | (uintptr_t)acc_offsets) & 7u) return MTLORA_ERR_ALIGN;
    if (!opt_aligned16((uintptr_t)acc)) return MTLORA_ERR_ALIGN;
    return opt_update<OPT_ADAMW, OptGroupsDev>(a);
}

int mtlora_lr_schedule_check(const mtlora_lr_schedule* host_record, int n_groups) {
    if (!host_record) return MTLORA_ERR_NULL;
    if (n_groups < 1 || n_groups > OPT_MAXG) return MTLORA_ERR_UNSUPPORTED;
    return opt_sched_ok(*host_record, n_groups) ? MTLORA_OK : MTLORA_ERR_SHAPE;
}

int mtlora_lr_schedule_value(const mtlora_lr_schedule* host_record, int n_groups, int group, int64_t t, double* lr) {
    if (!lr) return MTLORA_ERR_NULL;
    const int rc = mtlora_lr_schedule_check(host_record, n_groups);
    if (rc != MTLORA_OK) return rc;
    if (group < 0 || group >= n_groups || t < 0) return MTLORA_ERR_SHAPE;
    *lr = opt_sched_lr(*host_record, group, t);
    return MTLORA_OK;
}

int mtlora_adamw_sched_update_dev(const void* table, const void* grads, int64_t n_tensors, int64_t n_chunks,
                                  const mtlora_adamw_group* groups_dev, int n_groups, float max_norm, float* ctrl, float* norm_out,
                                  float* scale, int32_t* growth_tracker, double growth_factor, double backoff_factor, int growth_interval,
                                  void* scratch, int64_t scratch_bytes, float* acc, const int64_t* acc_offsets, int accum_steps,
                                  void* sched_dev, void* stream) {
    const OptCall a = {table, grads, n_tensors, n_chunks, groups_dev, n_groups, max_norm, ctrl, norm_out, scale, growth_tracker,
                       (float)growth_factor, (float)backoff_factor, growth_interval, scratch, scratch_bytes, stream, 0.f, 0, acc, acc_offsets,
                       accum_steps, reinterpret_cast<OptSched*>(sched_dev)};
    const int rc = opt_check<OPT_ADAMW>(a);
    if (rc != MTLORA_OK) return rc;
    if (!sched_dev) return MTLORA_ERR_NULL;
    if (accum_steps < 1 || accum_steps > MTLORA_ADAMW_MAX_ACCUM_STEPS) return MTLORA_ERR_SHAPE;
    if (accum_steps > 1 && (!acc || !acc_offsets)) return MTLORA_ERR_NULL;  // (k = 1 updates straight from `grads`)
    if (((uintptr_t)groups_dev | (uintptr_t)acc_offsets | (uintptr_t)sched_dev) & 7u) return MTLORA_ERR_ALIGN;
    if (!opt_aligned16((uintptr_t)acc)) return MTLORA_ERR_ALIGN;
    return opt_update<OPT_ADAMW, OptGroupsDev>(a);
}

}  // extern "C"
