// snapshot.hip -- everything a train step mutates (trainable parameters, module buffers, the optimizer's moments and control
// words, the loss scaler's two words) gathered into ONE contiguous buffer by ONE launch, and scattered back by one: the device
// half of the reference's save_checkpoint / auto_resume_helper (utils.py:280-321), which there is a state_dict() walk with one
// device-to-host copy per tensor.  A replayed train loop cannot afford that walk between two replays; one launch into a staging
// buffer it can (mtlora_amd/checkpoint.py:TrainState takes it from there: one asynchronous copy to pinned memory).
//
// Table: n entries {address, bytes, packed offset}, built once on the host (mtlora_snapshot_entry), uploaded and kept.  Entries
// come in ascending packed order, every packed offset 16-byte aligned, no entry reaching into the next (mtlora_snapshot_chunks /
// mtlora_snapshot_check reject anything else on the host).  Tensors are opaque bytes.
//
// Work is cut in the PACKED space, not per tensor: workgroup c owns packed bytes [c * CHUNK, (c + 1) * CHUNK).  optim.hip keeps a
// second table chunk -> (tensor, index) because its chunks are per tensor; here the packed offsets are already a sorted key, so a
// workgroup finds its first entry with a binary search over the entry table (about ten uniform loads for a thousand tensors) and
// walks on until an entry begins behind its range.  That needs no second table, balances a set of one 30 MB buffer and hundreds of
// 64-byte vectors by construction, and a chunk boundary inside an entry keeps the 16-byte phase: CHUNK is a multiple of 16, so
// the live address of a chunk's first byte is misaligned exactly as the tensor's base is.
//
// Per (entry, chunk) range: whole 16-byte units first -- 16-byte vector loads and stores when the live address is 16-byte aligned,
// four dwords per unit when it is 4-byte aligned, sixteen bytes per unit otherwise (any alignment down to 1) -- the packed side is a
// 16-byte vector access in all three; then the last bytes % 16 one byte per lane.  Only bytes inside an entry are ever read or
// written on either side: the alignment gaps of `packed` keep what they held, and a tensor that ends on the last byte of its
// allocation is not read past.  Plain C++, vector stores, no atomics, no scratch, no memset; every pointer is a launch argument or
// sits in the table, and the host code allocates, keeps and synchronises nothing, so a captured launch replays as it is.
#include "common.h"

namespace {

constexpr int64_t SNAP_CHUNK = MTLORA_SNAPSHOT_CHUNK;
constexpr int SNAP_THREADS = 256;
constexpr int SNAP_INFLIGHT = 4;  // 16-byte units a lane loads before it stores the first
static_assert(SNAP_CHUNK % 16 == 0 && SNAP_CHUNK % (16 * SNAP_THREADS) == 0, "chunk = whole vectors per lane");

struct SnapEntry {
    uint8_t* ptr;    // the live tensor
    int64_t bytes;
    int64_t offset;  // in the packed buffer, a multiple of 16
    int64_t reserved;
};
static_assert(sizeof(SnapEntry) == 32, "table layout");

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

// one 16-byte unit of a live tensor at any alignment: A = 16 (one vector), 4 (dwords) or 1 (bytes)
template <int A>
__device__ __forceinline__ u32x4 snap_load(const uint8_t* p) {
    if constexpr (A == 16) {
        return *reinterpret_cast<const u32x4*>(p);
    } else if constexpr (A == 4) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
        return u32x4{q[0], q[1], q[2], q[3]};
    } else {
        u32x4 v;
#pragma unroll
        for (int w = 0; w < 4; ++w)
            v[w] = (uint32_t)p[4 * w] | ((uint32_t)p[4 * w + 1] << 8) | ((uint32_t)p[4 * w + 2] << 16) | ((uint32_t)p[4 * w + 3] << 24);
        return v;
    }
}
template <int A>
__device__ __forceinline__ void snap_store(uint8_t* p, u32x4 v) {
    if constexpr (A == 16) {
        *reinterpret_cast<u32x4*>(p) = v;
    } else if constexpr (A == 4) {
        uint32_t* q = reinterpret_cast<uint32_t*>(p);
        q[0] = v[0], q[1] = v[1], q[2] = v[2], q[3] = v[3];
    } else {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            p[4 * w] = (uint8_t)v[w], p[4 * w + 1] = (uint8_t)(v[w] >> 8);
            p[4 * w + 2] = (uint8_t)(v[w] >> 16), p[4 * w + 3] = (uint8_t)(v[w] >> 24);
        }
    }
}

// nv whole units between a live range (alignment class A) and a packed range (16-byte aligned); UNPACK: packed -> live
template <bool UNPACK, int A>
__device__ __forceinline__ void snap_units(uint8_t* live, uint8_t* packed, int nv) {
    for (int i = threadIdx.x; i < nv; i += SNAP_INFLIGHT * SNAP_THREADS) {
        u32x4 v[SNAP_INFLIGHT];
#pragma unroll
        for (int j = 0; j < SNAP_INFLIGHT; ++j) {
            const int u = i + j * SNAP_THREADS;
            if (u < nv) v[j] = UNPACK ? snap_load<16>(packed + 16 * (int64_t)u) : snap_load<A>(live + 16 * (int64_t)u);
        }
#pragma unroll
        for (int j = 0; j < SNAP_INFLIGHT; ++j) {
            const int u = i + j * SNAP_THREADS;
            if (u < nv) {
                if (UNPACK)
                    snap_store<A>(live + 16 * (int64_t)u, v[j]);
                else
                    snap_store<16>(packed + 16 * (int64_t)u, v[j]);
            }
        }
    }
}

template <bool UNPACK>
__global__ __launch_bounds__(SNAP_THREADS) void k_snapshot(const SnapEntry* __restrict__ table, int n, uint8_t* packed,
                                                           int64_t packed_bytes) {
    const int64_t lo = (int64_t)blockIdx.x * SNAP_CHUNK;
    const int64_t hi = lo + SNAP_CHUNK < packed_bytes ? lo + SNAP_CHUNK : packed_bytes;  // nothing of `packed` behind its end
    int a = 0, b = n;  // the first entry that ends behind lo (the ends ascend: entries are sorted and do not overlap)
    while (a < b) {
        const int m = (a + b) >> 1;
        if (table[m].offset + table[m].bytes > lo)
            b = m;
        else
            a = m + 1;
    }
    for (int e = a; e < n; ++e) {
        const SnapEntry t = table[e];
        if (t.offset >= hi) break;
        const int64_t s = t.offset > lo ? t.offset : lo;
        const int64_t f = t.offset + t.bytes < hi ? t.offset + t.bytes : hi;
        if (f <= s) continue;  // a zero-byte tensor
        uint8_t* live = t.ptr + (s - t.offset);
        uint8_t* pk = packed + s;  // 16-byte aligned: s is t.offset or lo
        const int len = (int)(f - s), nv = len >> 4;
        const uintptr_t al = reinterpret_cast<uintptr_t>(live);
        if ((al & 15) == 0)
            snap_units<UNPACK, 16>(live, pk, nv);
        else if ((al & 3) == 0)
            snap_units<UNPACK, 4>(live, pk, nv);
        else
            snap_units<UNPACK, 1>(live, pk, nv);
        const int at = (nv << 4) + (int)threadIdx.x;  // the last len % 16 bytes: one per lane, bytes on both sides
        if (at < len) {
            if (UNPACK)
                live[at] = pk[at];
            else
                pk[at] = live[at];
        }
    }
}

// the host table: sorted, aligned, not overlapping; *extent = the end of the last byte any entry owns
int snap_scan(const void* host_table, int64_t n, int64_t* extent) {
    if (n < 0 || n >= ((int64_t)1 << 31)) return MTLORA_ERR_SHAPE;
    if (n > 0 && !host_table) return MTLORA_ERR_NULL;
    const SnapEntry* t = reinterpret_cast<const SnapEntry*>(host_table);
    int64_t end = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (t[i].bytes < 0 || t[i].offset < 0 || t[i].bytes >= ((int64_t)1 << 46) || t[i].offset >= ((int64_t)1 << 46)) return MTLORA_ERR_SHAPE;
        if (t[i].offset & 15) return MTLORA_ERR_ALIGN;
        if (t[i].offset < end) return MTLORA_ERR_SHAPE;  // reaches into the previous entry (or the table is not sorted)
        if (t[i].bytes > 0 && !t[i].ptr) return MTLORA_ERR_NULL;
        end = t[i].offset + t[i].bytes;
    }
    *extent = end;
    return MTLORA_OK;
}

int snap_launch_check(const void* dev_table, int64_t n, int64_t n_chunks, const void* packed, int64_t packed_bytes) {
    if (n < 0 || n >= ((int64_t)1 << 31) || n_chunks < 0 || n_chunks >= ((int64_t)1 << 31) || packed_bytes < 0) return MTLORA_ERR_SHAPE;
    if (n > 0 && !dev_table) return MTLORA_ERR_NULL;
    if (n_chunks > 0 && !packed) return MTLORA_ERR_NULL;
    if ((reinterpret_cast<uintptr_t>(dev_table) & 7) || (reinterpret_cast<uintptr_t>(packed) & 15)) return MTLORA_ERR_ALIGN;
    // the table is device memory here: what can be said without it is that n_chunks chunks hold more than n_chunks - 1 whole ones
    // (mtlora_snapshot_check compares against the exact extent); the kernel never touches `packed` at or behind packed_bytes
    if (n_chunks > 0 && packed_bytes <= (n_chunks - 1) * SNAP_CHUNK) return MTLORA_ERR_WORKSPACE;
    return MTLORA_OK;
}

}  // namespace

extern "C" {

int64_t mtlora_snapshot_entry_bytes(void) { return (int64_t)sizeof(SnapEntry); }

int mtlora_snapshot_entry(void* host_entry, const void* ptr, int64_t bytes, int64_t packed_offset) {
    if (!host_entry) return MTLORA_ERR_NULL;
    if (bytes < 0 || packed_offset < 0 || bytes >= ((int64_t)1 << 46) || packed_offset >= ((int64_t)1 << 46)) return MTLORA_ERR_SHAPE;
    if (packed_offset & 15) return MTLORA_ERR_ALIGN;
    if (bytes > 0 && !ptr) return MTLORA_ERR_NULL;
    SnapEntry* e = reinterpret_cast<SnapEntry*>(host_entry);
    e->ptr = reinterpret_cast<uint8_t*>(const_cast<void*>(ptr));
    e->bytes = bytes;
    e->offset = packed_offset;
    e->reserved = 0;
    return MTLORA_OK;
}

int64_t mtlora_snapshot_chunks(const void* host_table, int64_t n) {
    int64_t extent = 0;
    const int rc = snap_scan(host_table, n, &extent);
    if (rc != MTLORA_OK) return rc;
    const int64_t nc = mtl_ceil_div(extent, SNAP_CHUNK);
    return nc >= ((int64_t)1 << 31) ? (int64_t)MTLORA_ERR_SHAPE : nc;
}

int mtlora_snapshot_check(const void* host_table, int64_t n, int64_t packed_bytes) {
    int64_t extent = 0;
    const int rc = snap_scan(host_table, n, &extent);
    if (rc != MTLORA_OK) return rc;
    if (packed_bytes < 0) return MTLORA_ERR_SHAPE;
    return packed_bytes < extent ? MTLORA_ERR_WORKSPACE : MTLORA_OK;
}

int mtlora_snapshot_pack(const void* dev_table, int64_t n, int64_t n_chunks, void* packed, int64_t packed_bytes, void* stream) {
    const int rc = snap_launch_check(dev_table, n, n_chunks, packed, packed_bytes);
    if (rc != MTLORA_OK) return rc;
    if (n == 0 || n_chunks == 0) return MTLORA_OK;
    hipLaunchKernelGGL(k_snapshot<false>, dim3((unsigned)n_chunks), dim3(SNAP_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const SnapEntry*>(dev_table), (int)n, reinterpret_cast<uint8_t*>(packed), packed_bytes);
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

int mtlora_snapshot_unpack(const void* dev_table, int64_t n, int64_t n_chunks, const void* packed, int64_t packed_bytes, void* stream) {
    const int rc = snap_launch_check(dev_table, n, n_chunks, packed, packed_bytes);
    if (rc != MTLORA_OK) return rc;
    if (n == 0 || n_chunks == 0) return MTLORA_OK;
    hipLaunchKernelGGL(k_snapshot<true>, dim3((unsigned)n_chunks), dim3(SNAP_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const SnapEntry*>(dev_table), (int)n, reinterpret_cast<uint8_t*>(const_cast<void*>(packed)),
                       packed_bytes);
    MTL_CHECK_LAUNCH();
    return MTLORA_OK;
}

}  // extern "C"
