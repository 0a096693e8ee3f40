// reduce.hip -- small deterministic reductions of the train step's callers that ATen would run as multi-block
// reduce_kernels: those zero a semaphore buffer with hipMemsetAsync first, and on this ROCm stack a CAPTURED small memset stops
// taking effect from the second graph replay on (mtl_harness.GraphedTrainStep) -- the nine memsets per step listed by
// tools/find_memsets.py were exactly these sums.  Two launches each (per-block partials in a fixed order, then one combine
// kernel): no atomics, no memset, bit-reproducible.
//
//   mtlora_colsum       out[n] = sum_m x[m][n]                     bias gradient of the heads' big-M 1x1 convolutions
//                                                                  (dL/db of reference models/seg_hrnet.py:498-526 layers)
//   mtlora_linear_bias_grad  db[n] = sum_m (dy_s[m][n] + sum_t dy_t[t][m][n])   gradient of a trainable `linear.bias` of an MTLoRALinear
//                                                                  (MTLORA.BIAS 'all', reference lora.py:606-624): the same walk over
//                                                                  up to 1 + T sources, no (M, N) intermediate
//   mtlora_label_stat   kind 0: #{ lab != ignore }                 valid-pixel count / mask sum of mtl_loss_schemes.py:22-39,
//                       kind 1: mean(1 - (lab >= 0.5))             :162-220; class balance w of :42-89
//   mtlora_label_stat_valid  the same over the labelled samples of a batch (a byte per sample), plus their number: the `stat`
//                       of mtlora_upsample_loss_valid; an unlabelled sample's labels are not read
#include "dispatch.h"

namespace {

constexpr int RD_MAXBLK = 1024;

// stage 1: block b sums rows b, b + G, ... (256 / nvec rows per sweep) of the 16-byte column vectors of EVERY source -> part[b][N].
// The sources travel by value (SumParams of tn.h is the pattern); a row batch issues its four loads per source before the adds,
// which keep the order row-major then source-major: one source gives the bits of the single-pointer kernel this one replaced.
constexpr int CS_MAXSRC = 1 + MTLORA_MAX_TASKS;
struct ColsumParams {
    const void* src[CS_MAXSRC];
    int n;
};
template <typename T>
__global__ __launch_bounds__(256) void k_colsum_part(ColsumParams P, int64_t M, int N, float* part) {
    constexpr int VE = ET<T>::VEC;
    __shared__ float sm[256][VE + 1];
    const int nvec = N / VE;
    const int tid = threadIdx.x;
    for (int v0 = 0; v0 < nvec; v0 += 256) {  // column-vector chunks (one pass for N <= 256 * VE)
        const int cv = nvec - v0 < 256 ? nvec - v0 : 256;  // vectors in this chunk
        const int rps = 256 / cv;                          // rows per sweep
        const int r = tid / cv, v = tid - r * cv;
        float acc[VE];
#pragma unroll
        for (int e = 0; e < VE; ++e) acc[e] = 0.f;
        if (r < rps) {
            const int64_t step = (int64_t)gridDim.x * rps, col = (int64_t)(v0 + v) * VE;
            int64_t m = (int64_t)blockIdx.x * rps + r;
            for (; m + 3 * step < M; m += 4 * step) {  // four rows in flight per source
                for (int s = 0; s < P.n; ++s) {
                    const T* x = reinterpret_cast<const T*>(P.src[s]) + col;
                    Vec16<T> q[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) q[j] = mtl_ld16<T>(x + (m + j * step) * N);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int e = 0; e < VE; ++e) acc[e] += mtl_to_f32(q[j].e[e]);
                }
            }
            for (; m < M; m += step)
                for (int s = 0; s < P.n; ++s) {
                    const Vec16<T> q = mtl_ld16<T>(reinterpret_cast<const T*>(P.src[s]) + col + m * N);
#pragma unroll
                    for (int e = 0; e < VE; ++e) acc[e] += mtl_to_f32(q.e[e]);
                }
        }
#pragma unroll
        for (int e = 0; e < VE; ++e) sm[tid][e] = (r < rps) ? acc[e] : 0.f;
        __syncthreads();
        if (tid < cv) {  // fixed-order combine over the rows of the sweep
            float t[VE];
#pragma unroll
            for (int e = 0; e < VE; ++e) t[e] = 0.f;
            for (int rr = 0; rr < rps; ++rr)
#pragma unroll
                for (int e = 0; e < VE; ++e) t[e] += sm[rr * cv + tid][e];
#pragma unroll
            for (int e = 0; e < VE; ++e) part[(int64_t)blockIdx.x * N + (int64_t)(v0 + tid) * VE + e] = t[e];
        }
        __syncthreads();
    }
}

// stage 2: out[c] = scale * sum_b part[b][c]  (16 waves share the partials round-robin, 4 independent chains each)
constexpr int RD_RW = 16;
__global__ __launch_bounds__(64 * RD_RW) void k_colsum_combine(const float* part, float* out, int nblk, int N, float scale) {
    __shared__ float sm[RD_RW][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (c < N) {
        int b = wave;
        for (; b + 3 * RD_RW < nblk; b += 4 * RD_RW) {
            a0 += part[(int64_t)b * N + c];
            a1 += part[(int64_t)(b + RD_RW) * N + c];
            a2 += part[(int64_t)(b + 2 * RD_RW) * N + c];
            a3 += part[(int64_t)(b + 3 * RD_RW) * N + c];
        }
        for (; b < nblk; b += RD_RW) a0 += part[(int64_t)b * N + c];
    }
    sm[wave][lane] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (wave == 0 && c < N) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < RD_RW; ++w) t += sm[w][lane];
        out[c] = t * scale;
    }
}

// label statistics, stage 1: per-block count (exact in fp32: a block sees < 2^24 elements)
__global__ __launch_bounds__(256) void k_label_stat_part(const float* lab, int64_t n, int kind, float ignore, float* part) {
    __shared__ float sm[256];
    float c = 0.f;
    const int64_t nv = n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (int64_t)gridDim.x * 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(lab + i * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) c += kind == 0 ? (v[e] != ignore ? 1.f : 0.f) : (v[e] >= 0.5f ? 0.f : 1.f);
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(n & 3)) {  // tail elements
        const float v = lab[(nv << 2) + threadIdx.x];
        c += kind == 0 ? (v != ignore ? 1.f : 0.f) : (v >= 0.5f ? 0.f : 1.f);
    }
    sm[threadIdx.x] = c;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sm[0];
}

// label statistics, stage 2: the per-block counts are exact integers < 2^24; their total may exceed 2^24, so it is formed in
// double and rounded once (what ATen's int64 sum followed by .float() gives)
__global__ __launch_bounds__(256) void k_label_stat_combine(const float* part, float* out, int nblk, double scale) {
    __shared__ double sm[256];
    double t = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 256) t += (double)part[b];
    sm[threadIdx.x] = t;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)(sm[0] * scale);
}

// label statistics over the LABELLED samples of a batch (valid[b] != 0; NULL: all), stage 1: block (b, j) = blockIdx.x / g,
// blockIdx.x % g counts its share of sample b into part[b * g + j].  A block of an unlabelled sample returns before it reads
// anything of that sample and leaves its partial unwritten: stage 2 does not read it.  Samples whose first element is not
// 16-byte aligned (n_per_sample % 4 != 0) are walked element by element; counts are integers, so the walk does not matter.
__global__ __launch_bounds__(256) void k_label_stat_valid_part(const float* lab, const unsigned char* valid, int64_t nps, int g, int kind,
                                                               float ignore, float* part) {
    __shared__ float sm[256];
    const int b = blockIdx.x / g, j = blockIdx.x - b * g;
    if (valid != nullptr && valid[b] == 0) return;  // (block-uniform)
    const float* x = lab + (int64_t)b * nps;
    float c = 0.f;
    if ((nps & 3) == 0) {
        const int64_t nv = nps >> 2;
        for (int64_t i = (int64_t)j * 256 + threadIdx.x; i < nv; i += (int64_t)g * 256) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(x + i * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) c += kind == 0 ? (v[e] != ignore ? 1.f : 0.f) : (v[e] >= 0.5f ? 0.f : 1.f);
        }
    } else {
        for (int64_t i = (int64_t)j * 256 + threadIdx.x; i < nps; i += (int64_t)g * 256) {
            const float v = x[i];
            c += kind == 0 ? (v != ignore ? 1.f : 0.f) : (v >= 0.5f ? 0.f : 1.f);
        }
    }
    sm[threadIdx.x] = c;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sm[0];
}

// stage 2: the labelled samples' partials (exact integers) in double, in a fixed order, and their number |V|:
// out[0] = kind 0: the count; kind 1: count / (|V| n_per_sample), the mean, formed as k_label_stat_combine forms count / n
// (all labelled: the same bits); kind 2: 0 (nothing was counted).  0 when no sample is labelled.  out[1] = |V|.
__global__ __launch_bounds__(256) void k_label_stat_valid_combine(const float* part, const unsigned char* valid, float* out, int B, int g,
                                                                  int64_t nps, int kind) {
    __shared__ double sm[256];
    __shared__ int sv[256];
    double t = 0.0;
    int nv = 0;
    if (kind != 2)
        for (int i = threadIdx.x; i < B * g; i += 256)
            if (valid == nullptr || valid[i / g] != 0) t += (double)part[i];
    for (int b = threadIdx.x; b < B; b += 256) nv += (valid == nullptr || valid[b] != 0) ? 1 : 0;
    sm[threadIdx.x] = t;
    sv[threadIdx.x] = nv;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            sm[threadIdx.x] += sm[threadIdx.x + s];
            sv[threadIdx.x] += sv[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double scale = kind == 0 ? 1.0 : (sv[0] > 0 ? 1.0 / (double)((int64_t)sv[0] * nps) : 0.0);
        out[0] = (float)(sm[0] * scale);
        out[1] = (float)sv[0];
    }
}

int rd_blocks(int64_t work_items) {
    int64_t g = mtl_ceil_div(work_items, 256 * 8);
    if (g > RD_MAXBLK) g = RD_MAXBLK;
    return (int)(g < 1 ? 1 : g);
}

bool colsum_shape_ok(int64_t M, int64_t N, int dtype) { return M >= 0 && N > 0 && N % mtl_vec_elems(dtype) == 0 && N <= (1 << 20); }

// >= 8 sweeps per block, at most RD_MAXBLK blocks
int colsum_blocks(int64_t M, int64_t N, int dtype) {
    const int nvec = (int)(N / mtl_vec_elems(dtype));
    const int rps = nvec >= 256 ? 1 : 256 / nvec;
    int64_t g = mtl_ceil_div(M, (int64_t)rps * 8);
    if (g > RD_MAXBLK) g = RD_MAXBLK;
    return (int)(g < 1 ? 1 : g);
}

// the two launches of a column sum over P's sources; `part` holds colsum_blocks() x N floats
int colsum_launch(const ColsumParams& P, int64_t M, int64_t N, int dtype, float* out, float* part, hipStream_t s) {
    const int g = colsum_blocks(M, N, dtype);
    mtl_dispatch_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(k_colsum_part<T>, dim3((unsigned)g), dim3(256), 0, s, P, M, (int)N, part);
    });
    hipLaunchKernelGGL(k_colsum_combine, dim3((unsigned)mtl_ceil_div(N, 64)), dim3(64 * RD_RW), 0, s, (const float*)part, out, g, (int)N,
                       1.f);
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

}  // namespace

extern "C" {

int64_t mtlora_colsum_scratch_bytes(int64_t M, int64_t N) {
    if (M < 0 || N <= 0) return -1;
    return (int64_t)RD_MAXBLK * N * 4 + 256;
}

int mtlora_colsum(const void* x, int64_t M, int64_t N, int dtype, float* out, void* scratch, int64_t scratch_bytes, void* stream) {
    if (!mtl_dtype_in(dtype, MTL_DT_F32_BF16)) return MTLORA_ERR_DTYPE;
    if (!colsum_shape_ok(M, N, dtype)) return MTLORA_ERR_SHAPE;
    if (mtl_any_null({x, out, scratch})) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({x, scratch})) return MTLORA_ERR_ALIGN;
    if (scratch_bytes < mtlora_colsum_scratch_bytes(M, N)) return MTLORA_ERR_WORKSPACE;
    ColsumParams P = {};
    P.src[P.n++] = x;
    return colsum_launch(P, M, N, dtype, out, reinterpret_cast<float*>(scratch), (hipStream_t)stream);
}

int64_t mtlora_linear_bias_grad_scratch_bytes(const mtlora_linear_desc* d) {
    if (!d || !mtl_dtype_in(d->dtype, MTL_DT_ALL) || d->T < 0 || d->T > MTLORA_MAX_TASKS || !colsum_shape_ok(d->M, d->N, d->dtype)) return -1;
    return (int64_t)colsum_blocks(d->M, d->N, d->dtype) * d->N * 4 + 256;
}

int mtlora_linear_bias_grad(const mtlora_linear_desc* d, const void* dy_s, const void* const* dy_t, float* db, void* scratch,
                            int64_t scratch_bytes, void* stream) {
    if (!d) return MTLORA_ERR_NULL;
    if (!mtl_dtype_in(d->dtype, MTL_DT_ALL)) return MTLORA_ERR_DTYPE;
    if (d->T < 0 || d->T > MTLORA_MAX_TASKS || !colsum_shape_ok(d->M, d->N, d->dtype)) return MTLORA_ERR_SHAPE;
    if (mtl_any_null({db, scratch}) || (d->T > 0 && !dy_t)) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({dy_s, scratch}, d->T, {dy_t}) || ((uintptr_t)db & 3)) return MTLORA_ERR_ALIGN;
    if (scratch_bytes < mtlora_linear_bias_grad_scratch_bytes(d)) return MTLORA_ERR_WORKSPACE;
    ColsumParams P = {};  // an output that got no gradient (NULL) is skipped; no source at all: the kernels write zeros
    if (dy_s) P.src[P.n++] = dy_s;
    for (int t = 0; t < d->T; ++t)
        if (dy_t[t]) P.src[P.n++] = dy_t[t];
    return colsum_launch(P, d->M, d->N, d->dtype, db, reinterpret_cast<float*>(scratch), (hipStream_t)stream);
}

int64_t mtlora_label_stat_scratch_bytes(int64_t n) {
    if (n < 0) return -1;
    return (int64_t)RD_MAXBLK * 4 + 256;
}

int mtlora_label_stat(const float* label, int64_t n, int kind, float ignore_index, float* out, void* scratch,
                      int64_t scratch_bytes, void* stream) {
    if (kind != 0 && kind != 1) return MTLORA_ERR_UNSUPPORTED;
    if (n <= 0) return MTLORA_ERR_SHAPE;
    if (mtl_any_null({label, out, scratch})) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({label})) return MTLORA_ERR_ALIGN;
    if (scratch_bytes < mtlora_label_stat_scratch_bytes(n)) return MTLORA_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int g = rd_blocks(n / 4 + 1);
    float* part = reinterpret_cast<float*>(scratch);
    hipLaunchKernelGGL(k_label_stat_part, dim3((unsigned)g), dim3(256), 0, s, label, n, kind, ignore_index, part);
    hipLaunchKernelGGL(k_label_stat_combine, dim3(1), dim3(256), 0, s, (const float*)part, out, g, kind == 0 ? 1.0 : 1.0 / (double)n);
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

// blocks per sample of mtlora_label_stat_valid (a block sees < 2^24 elements: n_per_sample < 2^31)
static int label_stat_valid_blocks(int64_t n_per_sample) { return rd_blocks(n_per_sample / 4 + 1); }

static bool label_stat_valid_shape_ok(int64_t B, int64_t n_per_sample) {
    return B > 0 && n_per_sample > 0 && n_per_sample < ((int64_t)1 << 31) && B * (int64_t)RD_MAXBLK < ((int64_t)1 << 31);
}

int64_t mtlora_label_stat_valid_scratch_bytes(int64_t B, int64_t n_per_sample) {
    if (!label_stat_valid_shape_ok(B, n_per_sample)) return -1;
    return B * (int64_t)label_stat_valid_blocks(n_per_sample) * 4 + 256;
}

int mtlora_label_stat_valid(const float* label, const unsigned char* valid, int64_t B, int64_t n_per_sample, int kind,
                            float ignore_index, float* out, void* scratch, int64_t scratch_bytes, void* stream) {
    if (kind != 0 && kind != 1 && kind != 2) return MTLORA_ERR_UNSUPPORTED;
    if (!label_stat_valid_shape_ok(B, n_per_sample)) return MTLORA_ERR_SHAPE;
    if (mtl_any_null({out, scratch}) || (kind != 2 && !label)) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({label, scratch}) || ((uintptr_t)out & 3)) return MTLORA_ERR_ALIGN;
    if (scratch_bytes < mtlora_label_stat_valid_scratch_bytes(B, n_per_sample)) return MTLORA_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int g = label_stat_valid_blocks(n_per_sample);
    float* part = reinterpret_cast<float*>(scratch);
    mtl_prof_tag("part B%lld n%lld k%d g%d", (long long)B, (long long)n_per_sample, kind, g);
    if (kind != 2) {
        MtlProfScope prof(PK_LABEL_STAT_VALID, (double)B * n_per_sample * 4.0, s);
        hipLaunchKernelGGL(k_label_stat_valid_part, dim3((unsigned)(B * g)), dim3(256), 0, s, label, valid, n_per_sample, g, kind,
                           ignore_index, part);
    }
    {
        mtl_prof_tag("combine B%lld k%d g%d", (long long)B, kind, g);
        MtlProfScope prof(PK_LABEL_STAT_VALID, (double)B * g * 4.0, s);
        hipLaunchKernelGGL(k_label_stat_valid_combine, dim3(1), dim3(256), 0, s, (const float*)part, valid, out, (int)B, g, n_per_sample,
                           kind);
    }
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

}  // extern "C"
