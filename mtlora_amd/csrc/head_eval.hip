// head_eval.hip -- the decoder head in eval mode as ONE kernel (reference models/seg_hrnet.py:498-526: conv1x1 -> BatchNorm2d ->
// ReLU -> conv1x1 on the (pixels, channels) matrix, BatchNorm with its running statistics):
//
//   mtlora_head_eval_fwd   O (M x ncp) = act((X W1^T) .* a + c) W2^T + b2        k_head_eval, one launch
//
// a = gamma / sqrt(running_var + eps), c = beta + (b1 - running_mean) a (formed by the caller on the device), act = ReLU or identity.
// The Hd-wide intermediate (1080 channels in every shipped head) never leaves the chip:
//
//   work split  a wave owns 32 rows of X for a whole row block: its X operand covers ALL of K and is loaded ONCE, straight from global
//               memory into fragment registers (ceil(ldx / 16) steps x 4 registers; 68 at ldx = 272).  A workgroup is HE_WAVES waves
//               (8 -> 256 rows; 4 at ldx > 272, where the X operand alone is up to 128 registers) that share the weight stream; the
//               grid is persistent: workgroup g takes row blocks g, g + grid, ...
//   chunks      the hidden axis is walked in chunks of 32 columns.  Per chunk the 32 x ldx slab of W1, the 32 matching columns of W2
//               and 32 values each of a and c go through a two-slot LDS ring: the next chunk's global loads are issued before the
//               current chunk's MFMAs and land in LDS after them, ONE barrier per chunk.  The ring runs on across row blocks (after
//               the last chunk of a block comes chunk 0 of the next), so it drains once per workgroup.  W1 comes from L2: 587 KB at
//               1080 x 272, re-read once per row block.
//   GEMM 1      transposed: H^T_chunk (32 hidden x 32 rows) = W1_chunk (A operand, from LDS) . X^T (B operand, the resident
//               fragments), v_mfma_f32_32x32x16_{bf16,f16}.  Lane (row m = lane & 31, hh = lane >> 5) then holds, in accumulator
//               register r, hidden column  h(r) = (r & 3) + 8 (r >> 2) + 4 hh  of row m: 16 fp32 values.
//   epilogue 1  v = acc * a[h] + c[h], ReLU as (v < 0 ? 0 : v) -- a NaN stays a NaN, as ATen's relu keeps it -- and a pack to 16 bits.
//   GEMM 2      O^T (classes x rows) += W2_chunk . H^T_chunk, and the packed accumulator IS the B operand: registers 8t .. 8t + 7 are
//               the lane's eight k-slots of MFMA t (t = 0, 1).  A dot product does not care about the order of its terms as long as
//               both operands agree on it, so W2's chunk is laid out in LDS in the accumulator's order: slot e of lane half hh of MFMA
//               t, position p = 16 t + 8 hh + e of a class row, holds hidden column (e & 3) + 8 (2 t + (e >> 2)) + 4 hh.  The
//               staging threads do that permutation on their way into LDS (a 16-byte global vector, hidden 8 q .. 8 q + 7, becomes two
//               8-byte LDS writes at p = 16 (q >> 1) + 4 (q & 1) and p + 8).  No shuffle, no LDS round trip of H.
//   tails       the chunk past Hd (1080 = 33 * 32 + 24) has zero W1 rows, zero W2 columns and zero a, c: no address at or past row
//               Hd of W1 / column Hd of W2 is formed into a load.  A k tail (ldx % 16 == 8) and rows past M are zero X fragments
//               (never loaded) and zero A operands; class rows past ncp are zero A operands of GEMM 2.
//   epilogue 2  + b2, pack, one exchange between the two lane halves (each holds 4 of every 8 consecutive classes) and whole
//               16-byte segments of O's rows are stored; rows past M are not.
//   LDS rows    the W1 slab's row pitch is an ODD number of 16-byte vectors ((ldx / 8) | 1) and the W2 rows' 80 bytes (5 vectors), so
//               that 16 lanes reading one vector each of 16 consecutive rows cover all 64 banks once.
//
// Rows share nothing but the weights: a non-finite value in a row of X stays in that row of O.  No atomics, no workspace, no memset;
// every output element is produced once in a fixed order: results are bit-reproducible, and the launch is capturable as it is.
#include "common.h"
#include "dispatch.h"

namespace {

constexpr int HE_CH = 32;          // hidden columns per chunk
constexpr int HE_W2_PITCH = 80;    // bytes per class row of a W2 chunk in LDS (64 used)
constexpr int HE_MAX_LDX = 512, HE_MAX_NCP = 64;

struct HeadEvalParams {
    const void* X;
    const void* W1;
    const float* a;
    const float* c;
    const void* W2;
    const float* b2;
    void* O;
    int64_t M;
    int ldx, Hd, ncp, relu, n_blocks, w1_pitch;  // w1_pitch: bytes per row of a W1 chunk in LDS
};

template <int NT>
__host__ __device__ constexpr int he_slot_bytes(int w1_pitch) {
    return HE_CH * w1_pitch + NT * 32 * HE_W2_PITCH + 2 * HE_CH * 4;
}

template <typename T>
__device__ __forceinline__ f32x16 he_mfma(const u32x4& a, const u32x4& b, const f32x16& c) {
    if constexpr (__is_same(T, f16))
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// NK: steps of 16 along K the X fragments are sized for (ceil(ldx / 16) <= NK); NT: class tiles of 32 (ncp <= 32 NT)
template <typename T, int NK, int NT, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void k_head_eval(const HeadEvalParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char he_lds[];
    constexpr int NTH = WAVES * 64;
    constexpr int VW1 = (HE_CH * 2 * NK + NTH - 1) / NTH;  // 16-byte vectors of a W1 chunk per staging thread, at most
    constexpr u32x4 Z4 = {0u, 0u, 0u, 0u};
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, hh = lane >> 5;
    const int ldx = p.ldx, Hd = p.Hd, ncp = p.ncp;
    const int nv = ldx >> 3;                                // vectors per row of W1 / X
    const int n_chunks = (Hd + HE_CH - 1) / HE_CH;
    const int slot_bytes = he_slot_bytes<NT>(p.w1_pitch);
    const int w2_base = HE_CH * p.w1_pitch, ac_base = w2_base + NT * 32 * HE_W2_PITCH;
    const T* __restrict__ W1 = reinterpret_cast<const T*>(p.W1);
    const T* __restrict__ W2 = reinterpret_cast<const T*>(p.W2);
    const T* __restrict__ X = reinterpret_cast<const T*>(p.X);
    T* __restrict__ O = reinterpret_cast<T*>(p.O);

    // ---- what this thread stages of every chunk (chunk-independent: worked out once) ----
    int w1_row[VW1], w1_src[VW1], w1_dst[VW1];  // row of the chunk (HE_CH: nothing), element offset inside W1's chunk, LDS byte offset
#pragma unroll
    for (int i = 0; i < VW1; ++i) {
        const int v = tid + i * NTH;
        const int row = v / nv, col = v - row * nv;
        w1_row[i] = row < HE_CH ? row : HE_CH;
        w1_src[i] = row * ldx + col * 8;
        w1_dst[i] = row * p.w1_pitch + col * 16;
    }
    const int w2_n = tid >> 2, w2_q = tid & 3;  // class row and 16-byte vector (hidden 8 q .. 8 q + 7) of the W2 chunk
    const bool w2_mine = tid < NT * 128 && w2_n < ncp;
    const int w2_dst = w2_base + w2_n * HE_W2_PITCH + 2 * (16 * (w2_q >> 1) + 4 * (w2_q & 1));
    const bool ac_mine = tid < 16;              // threads 0 .. 7: a, 8 .. 15: c, four floats each
    const float* __restrict__ ac_src = (tid & 8) ? p.c : p.a;
    const int ac_i = 4 * (tid & 7);

    // a vector that lies outside its matrix is a ZERO, and its load is aimed at the matrix's first vector instead (always there):
    // no branch around a load, no address outside a matrix
    u32x4 sw1[VW1], sw2, sac;
    auto stage_load = [&](int chunk) {  // global -> registers; everything at or past Hd is zero and never addressed
        const int j0 = chunk * HE_CH;
#pragma unroll
        for (int i = 0; i < VW1; ++i) {
            const bool in = w1_row[i] < HE_CH && j0 + w1_row[i] < Hd;
            const u32x4 v = *reinterpret_cast<const u32x4*>(W1 + (in ? (int64_t)j0 * ldx + w1_src[i] : 0));
            sw1[i] = in ? v : Z4;
        }
        const bool in2 = w2_mine && j0 + 8 * w2_q < Hd, in3 = ac_mine && j0 + ac_i < Hd;
        const u32x4 v2 = *reinterpret_cast<const u32x4*>(W2 + (in2 ? (int64_t)w2_n * Hd + j0 + 8 * w2_q : 0));
        const u32x4 v3 = *reinterpret_cast<const u32x4*>(ac_src + (in3 ? j0 + ac_i : 0));
        sw2 = in2 ? v2 : Z4;
        sac = in3 ? v3 : Z4;
    };
    auto stage_store = [&](int slot) {  // registers -> LDS slot
        unsigned char* s = he_lds + slot * slot_bytes;
#pragma unroll
        for (int i = 0; i < VW1; ++i)
            if (w1_row[i] < HE_CH) *reinterpret_cast<u32x4*>(s + w1_dst[i]) = sw1[i];
        if (tid < NT * 128) {  // (class rows past ncp are written as zeros: sw2 is zero there)
            *reinterpret_cast<u32x2*>(s + w2_dst) = u32x2{sw2[0], sw2[1]};
            *reinterpret_cast<u32x2*>(s + w2_dst + 16) = u32x2{sw2[2], sw2[3]};
        }
        if (ac_mine) *reinterpret_cast<u32x4*>(s + ac_base + ((tid & 8) ? HE_CH * 4 : 0) + ac_i * 4) = sac;
    };

    int slot = 0;
    if ((int)blockIdx.x < p.n_blocks) {
        stage_load(0);
        stage_store(0);
    }
    __syncthreads();

    for (int blk = blockIdx.x; blk < p.n_blocks; blk += gridDim.x) {
        const int64_t row = (int64_t)blk * (WAVES * 32) + wave * 32 + li;
        const bool row_in = row < p.M;
        // the wave's X operand, all of K: element 16 s + 8 hh .. + 7 of the lane's row per step
        u32x4 xf[NK];
#pragma unroll
        for (int s = 0; s < NK; ++s) {
            const bool in = row_in && 16 * s + 8 * hh < ldx;
            const u32x4 v = *reinterpret_cast<const u32x4*>(X + (in ? row * ldx + 16 * s + 8 * hh : 0));
            xf[s] = in ? v : Z4;
        }
        f32x16 o[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
        const bool more_blocks = blk + (int)gridDim.x < p.n_blocks;

        for (int ch = 0; ch < n_chunks; ++ch) {
            const bool last = ch + 1 == n_chunks;
            const bool has_next = !last || more_blocks;
            if (has_next) stage_load(last ? 0 : ch + 1);

            const unsigned char* s = he_lds + slot * slot_bytes;
            // GEMM 1: H^T = W1_chunk . X^T
            f32x16 h;
#pragma unroll
            for (int r = 0; r < 16; ++r) h[r] = 0.f;
            const unsigned char* w1l = s + li * p.w1_pitch + 16 * hh;
#pragma unroll
            for (int k = 0; k < NK; ++k) {  // all NK steps, branch-free: a step at or past ldx has zero operands on both sides
                const bool in = 16 * k + 8 * hh < ldx;
                const u32x4 wa = *reinterpret_cast<const u32x4*>(w1l + (in ? 32 * k : 0));
                h = he_mfma<T>(in ? wa : Z4, xf[k], h);
            }
            // epilogue 1: the eval-mode BatchNorm as an affine map, ReLU, pack: registers 8 t .. 8 t + 7 -> the B operand of MFMA t
            const float* acl = reinterpret_cast<const float*>(s + ac_base) + 4 * hh;
            u32x4 hb[2];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 av = *reinterpret_cast<const f32x4*>(acl + 8 * g), cv = *reinterpret_cast<const f32x4*>(acl + HE_CH + 8 * g);
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[e] = h[4 * g + e] * av[e] + cv[e];
                    if (p.relu) v[e] = v[e] < 0.f ? 0.f : v[e];
                }
                hb[g >> 1][2 * (g & 1)] = mtl_pk2<T>(v[0], v[1]);
                hb[g >> 1][2 * (g & 1) + 1] = mtl_pk2<T>(v[2], v[3]);
            }
            // GEMM 2: O^T += W2_chunk . H^T
            const unsigned char* w2l = s + w2_base + li * HE_W2_PITCH + 16 * hh;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int k = 0; k < 2; ++k)
                    o[t] = he_mfma<T>(*reinterpret_cast<const u32x4*>(w2l + t * 32 * HE_W2_PITCH + 32 * k), hb[k], o[t]);

            if (has_next) stage_store(slot ^ 1);
            __syncthreads();
            slot ^= 1;
        }

        // epilogue 2: lane (row, hh) holds classes 32 t + 8 g + 4 hh + 0 .. 3 in registers 4 g .. 4 g + 3
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            u32x4 lo, hi;  // packed classes of segments g = 0, 1 and g = 2, 3: this lane's half (4 hh .. 4 hh + 3) of each
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int cls = 32 * t + 8 * g + 4 * hh;
                f32x4 b = {0.f, 0.f, 0.f, 0.f};
                if (cls < ncp) b = *reinterpret_cast<const f32x4*>(p.b2 + cls);
                const uint32_t w0 = mtl_pk2<T>(o[t][4 * g] + b[0], o[t][4 * g + 1] + b[1]);
                const uint32_t w1 = mtl_pk2<T>(o[t][4 * g + 2] + b[2], o[t][4 * g + 3] + b[3]);
                if (g < 2) {
                    lo[2 * g] = w0;
                    lo[2 * g + 1] = w1;
                } else {
                    hi[2 * g - 4] = w0;
                    hi[2 * g - 3] = w1;
                }
            }
            // the lower lane half stores segments g = 0, 1, the upper g = 2, 3: each hands the other its halves of those
            u32x4 got;
#pragma unroll
            for (int w = 0; w < 4; ++w) got[w] = (uint32_t)__shfl_xor((int)(hh ? lo[w] : hi[w]), 32, 64);
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const int seg = 32 * t + 8 * (g + 2 * hh);
                const u32x4 upper = {got[2 * g], got[2 * g + 1], hi[2 * g], hi[2 * g + 1]}, lower = {lo[2 * g], lo[2 * g + 1], got[2 * g], got[2 * g + 1]};
                const u32x4 out = hh ? upper : lower;
                if (row_in && seg < ncp) *reinterpret_cast<u32x4*>(O + row * ncp + seg) = out;
            }
        }
    }
}

template <typename T, int NK, int NT, int WAVES>
void he_launch(const HeadEvalParams& q, int cus, hipStream_t s) {
    HeadEvalParams p = q;
    const int64_t n_blocks = mtl_ceil_div(p.M, WAVES * 32);
    p.n_blocks = (int)n_blocks;
    const int lds = 2 * he_slot_bytes<NT>(p.w1_pitch);
    auto fn = k_head_eval<T, NK, NT, WAVES>;
    if (lds > 48 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    const unsigned grid = (unsigned)(n_blocks < cus ? n_blocks : cus);
    hipLaunchKernelGGL(fn, dim3(grid), dim3(WAVES * 64), lds, s, p);
}

template <typename T, int NT>
void he_launch_k(const HeadEvalParams& p, int cus, hipStream_t s) {
    if (p.ldx <= 64)
        he_launch<T, 4, NT, 8>(p, cus, s);
    else if (p.ldx <= 272)
        he_launch<T, 17, NT, 8>(p, cus, s);
    else
        he_launch<T, 32, NT, 4>(p, cus, s);
}

// MTLORA_OK when the kernel takes the shape, else the code mtlora_head_eval_fwd returns for it
int he_shape(int64_t M, int ldx, int Hd, int ncp) {
    if (M < 0 || ldx <= 0 || Hd <= 0 || ncp <= 0 || ldx % 8 || ncp % 8) return MTLORA_ERR_SHAPE;
    if (ldx > HE_MAX_LDX || Hd % 8 || ncp > HE_MAX_NCP || mtl_ceil_div(M, 128) >= ((int64_t)1 << 31)) return MTLORA_ERR_UNSUPPORTED;
    return MTLORA_OK;
}

}  // namespace

extern "C" {

int mtlora_head_eval_supported(int64_t M, int ldx, int Hd, int ncp, int dtype) {
    return mtl_dtype_in(dtype, MTL_DT_16) && he_shape(M, ldx, Hd, ncp) == MTLORA_OK ? 1 : 0;
}

int mtlora_head_eval_fwd(const void* X, const void* W1, const float* a, const float* c, const void* W2, const float* b2, void* O, int64_t M,
                         int ldx, int Hd, int ncp, int relu, int dtype, void* stream) {
    if (!mtl_dtype_in(dtype, MTL_DT_ALL)) return MTLORA_ERR_DTYPE;
    if (!mtl_dtype_in(dtype, MTL_DT_16)) return MTLORA_ERR_UNSUPPORTED;  // (fp32: the callers keep their four-step route)
    if (M == 0) return MTLORA_OK;
    if (mtl_any_null({X, W1, a, c, W2, b2, O})) return MTLORA_ERR_NULL;
    if (mtl_any_misaligned({X, W1, a, c, W2, b2, O})) return MTLORA_ERR_ALIGN;
    const int st = he_shape(M, ldx, Hd, ncp);
    if (st != MTLORA_OK) return st;
    HeadEvalParams p = {};
    p.X = X;
    p.W1 = W1;
    p.a = a;
    p.c = c;
    p.W2 = W2;
    p.b2 = b2;
    p.O = O;
    p.M = M;
    p.ldx = ldx;
    p.Hd = Hd;
    p.ncp = ncp;
    p.relu = relu ? 1 : 0;
    p.w1_pitch = ((ldx / 8) | 1) * 16;
    int dev = 0, cus = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    mtl_dispatch_dtype16(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        if (ncp <= 32)
            he_launch_k<T, 1>(p, cus, s);
        else
            he_launch_k<T, 2>(p, cus, s);
    });
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

}  // extern "C"
