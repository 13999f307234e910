// Pieces shared by the mesh kernels (meshmetrics.hip, meshcontains.hip): order-preserving fp64 keys for atomic min / max, the counter
// hash of the samplers, the scratch carver and the synchronising status read.
#pragma once
#include <string.h>

#include "common.h"

namespace {

__device__ __forceinline__ unsigned long long f64_key(double x) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
inline double f64_unkey(unsigned long long k) {
    const unsigned long long u = (k & 0x8000000000000000ull) ? (k & 0x7fffffffffffffffull) : ~k;
    double d;
    memcpy(&d, &u, 8);
    return d;
}

// min / max keys: per thread, then per wave, then one atomic per wave and axis
template <typename K>
__device__ __forceinline__ void wave_minmax_atomic(K lo, K hi, K* dlo, K* dhi) {
    for (int o = 32; o > 0; o >>= 1) {
        const K a = __shfl_xor(lo, o), b = __shfl_xor(hi, o);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
    if (lane_id() == 0) {
        if (lo != (K)~(K)0) atomicMin(dlo, lo);
        if (hi != (K)0) atomicMax(dhi, hi);
    }
}

__device__ __forceinline__ uint64_t mm_hash(uint64_t seed, uint64_t ctr) {
    uint64_t z = seed + ctr * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ double mm_u01(uint64_t h) { return (double)(h >> 11) * 0x1p-53; }           // [0, 1)
__device__ __forceinline__ double mm_u01_open0(uint64_t h) { return (double)((h >> 11) + 1) * 0x1p-53; }   // (0, 1]

// carves 256-byte aligned arrays out of one scratch buffer (p == nullptr: only counts the bytes)
struct Take {
    char* p;
    int64_t off;
    template <typename T>
    T* take(int64_t elems) {
        T* q = (T*)(p ? p + off : nullptr);
        off += (((elems > 0 ? elems : 1) * (int64_t)sizeof(T) + 255) / 256) * 256;
        return q;
    }
};

inline int mm_read(void* dst, const void* src, size_t bytes, hipStream_t stream, const char* what) {
    if (hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
        dgnn_set_error("%s: %s", what, hipGetErrorString(hipGetLastError()));
        return DGNN_E_LAUNCH;
    }
    return DGNN_OK;
}

}  // namespace
