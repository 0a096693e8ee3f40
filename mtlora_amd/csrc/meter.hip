// meter.hip -- the reference's training meters on the device: timm's AverageMeter.update (val / sum / count, avg = sum / count) for
// the loss, the per-task losses, the gradient norm, the loss scale and the learning rate of main.py:318-321, 354-365, 384-386,
// updated by ONE launch at the end of the train step from values that already sit in device memory.  The reference reads each of
// them back with .item() / state_dict() every step; here nothing leaves the device until the caller copies the bank out.
// mtlora_amd/meters.py:TrainMeters.update_torch is the definition the tests hold this file to, bit for bit.
//
// Bank: n_slots x {val, sum, count, skipped}, doubles.  Table: n_slots x mtlora_meter_source.  Counter: one int64, the number of
// update calls made so far.  A call with counter value c serves slot i iff (c + 1) % period[i] == 0: it reads v = *src[i] (fp32
// values widen exactly) and, v finite, sets val = v, sum += v * weight, count += weight; v not finite, sets val = v and
// skipped += 1 and leaves sum and count alone (AverageMeter would carry the inf / nan in sum for the rest of the epoch; the fp16
// recipe produces such a step whenever the scale grows too far).  Then the counter becomes c + 1.
//
// One workgroup of one wave, lane i serves slot i: every slot is read and written by one lane only, the counter is read by every
// lane before the barrier and written by lane 0 after it.  Plain loads, 16-byte vector stores, no atomics, no memset, no scratch;
// the product and the sum are rounded separately (no contraction: the pragma below), as the definition's are.  All pointers are
// launch arguments and the host code keeps no state, so a captured launch replays as it is.
#include "common.h"

#pragma clang fp contract(off)

namespace {

typedef __attribute__((ext_vector_type(2))) double f64x2;

__device__ __forceinline__ bool meter_finite(double v) {  // exponent not all ones (no reliance on the floating-point mode flags)
    return (__builtin_bit_cast(uint64_t, v) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
}

__global__ __launch_bounds__(MTLORA_METER_MAX_SLOTS) void k_meter_update(double* bank, const mtlora_meter_source* table, int n_slots,
                                                                         int64_t* counter) {
    const int i = threadIdx.x;
    const int64_t c1 = *counter + 1;
    if (i < n_slots) {
        const mtlora_meter_source s = table[i];
        const int64_t period = s.period < 1 ? 1 : s.period;
        if (s.src && c1 % period == 0) {  // (a record without a source is never served: no table content makes the kernel read null)
            const double v = s.dtype == MTLORA_METER_F64 ? *reinterpret_cast<const double*>(s.src)
                                                         : (double)*reinterpret_cast<const float*>(s.src);
            f64x2* slot = reinterpret_cast<f64x2*>(bank + 4 * i);
            const f64x2 a = slot[0], b = slot[1];  // val, sum | count, skipped
            if (meter_finite(v)) {
                const double vn = v * s.weight;
                slot[0] = f64x2{v, a.y + vn};
                slot[1] = f64x2{b.x + s.weight, b.y};
            } else {
                slot[0] = f64x2{v, a.y};
                slot[1] = f64x2{b.x, b.y + 1.0};
            }
        }
    }
    __syncthreads();  // every lane has read the counter
    if (i == 0) *counter = c1;
}

// zero-fill as a kernel (common.h:mtl_zero_async says why), with the counter as one more optional word
__global__ __launch_bounds__(256) void k_meter_reset(double* bank, int n_words, int64_t* counter) {
    for (int i = threadIdx.x; i < n_words; i += blockDim.x) bank[i] = 0.0;
    if (counter && threadIdx.x == 0) *counter = 0;
}

int meter_check(const void* bank, int n_slots, const void* counter) {
    if (n_slots < 1 || n_slots > MTLORA_METER_MAX_SLOTS) return MTLORA_ERR_SHAPE;  // before any pointer is looked at
    if (!bank || !counter) return MTLORA_ERR_NULL;
    if ((reinterpret_cast<uintptr_t>(bank) & 15) || (reinterpret_cast<uintptr_t>(counter) & 7)) return MTLORA_ERR_ALIGN;
    return MTLORA_OK;
}

}  // namespace

extern "C" {

int mtlora_meter_update(double* bank, const mtlora_meter_source* table, int n_slots, int64_t* counter, void* stream) {
    const int st = meter_check(bank, n_slots, counter);
    if (st != MTLORA_OK) return st;
    if (!table) return MTLORA_ERR_NULL;
    if (reinterpret_cast<uintptr_t>(table) & 7) return MTLORA_ERR_ALIGN;
    hipLaunchKernelGGL(k_meter_update, dim3(1), dim3(MTLORA_METER_MAX_SLOTS), 0, reinterpret_cast<hipStream_t>(stream), bank, table,
                       n_slots, counter);
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

int mtlora_meter_reset(double* bank, int n_slots, int64_t* counter, int keep_phase, void* stream) {
    const int st = meter_check(bank, n_slots, counter);
    if (st != MTLORA_OK) return st;
    hipLaunchKernelGGL(k_meter_reset, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), bank, 4 * n_slots,
                       keep_phase ? nullptr : counter);
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

}  // extern "C"
