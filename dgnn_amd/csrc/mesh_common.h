// Pieces shared by the mesh, scene and triangulation kernels: the launch grid, the id range check, order-preserving fp64 keys for atomic
// min / max and the bounding box of the referenced vertices, the wave reductions, the counter hash of the samplers, the scratch carver and
// the synchronising status read.
#pragma once
#include <string.h>

#include "common.h"
#include "mix64.h"

namespace {

constexpr int MESH_THREADS = 256;
dim3 mesh_launch_grid(int64_t items) { return dim3(dgnn_grid_cap(dgnn_cdiv(items > 0 ? items : 1, MESH_THREADS))); }

// ids read through later are checked first: every ids[i] in [0, bound), else `bit` into the status word
__global__ void k_check_ids(const int32_t* __restrict__ ids, int64_t n, int64_t bound, int32_t* err, int32_t bit) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        if (ids[i] < 0 || ids[i] >= bound) atomicOr(err, bit);
}

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

// (ids validated) min / max over the vertices that `ids` references, as integer keys: order-free.  refuse(x) = the status bits of a
// coordinate that does not count (0: it counts).  lo[3] preset to ~0, hi[3] to 0.
template <typename Refuse>
__global__ void k_bbox_referenced(const double* __restrict__ v, const int32_t* __restrict__ ids, int64_t n, Refuse refuse, int32_t* err,
                                  unsigned long long* dlo, unsigned long long* dhi) {
    unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0, 0, 0};
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t id = ids[i];
        for (int a = 0; a < 3; ++a) {
            const double x = v[3 * id + a];
            const int32_t e = refuse(x);
            if (e) { atomicOr(err, e); continue; }
            const unsigned long long k = f64_key(x);
            lo[a] = k < lo[a] ? k : lo[a];
            hi[a] = k > hi[a] ? k : hi[a];
        }
    }
    for (int a = 0; a < 3; ++a) wave_minmax_atomic(lo[a], hi[a], dlo + a, dhi + a);
}
inline void bbox_unkey(const unsigned long long* klo, const unsigned long long* khi, double* lo, double* hi) {
    for (int a = 0; a < 3; ++a) { lo[a] = f64_unkey(klo[a]); hi[a] = f64_unkey(khi[a]); }
}

// sums over the wave (every lane of the wave arrives).  wave_add_atomic: lane 0 adds a non-zero sum to *dst; integer sums: order-free
template <typename T>
__device__ __forceinline__ T wave_sum(T x) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}
template <typename T>
__device__ __forceinline__ void wave_add_atomic(T x, unsigned long long* dst) {
    x = wave_sum(x);
    if (lane_id() == 0 && x) atomicAdd(dst, (unsigned long long)x);
}
// the same over a block of MESH_THREADS: one atomic per block
__device__ __forceinline__ void block_add_atomic(unsigned long long* dst, long long v) {
    __shared__ long long part[MESH_THREADS / DGNN_WAVE];
    v = wave_sum(v);
    if (lane_id() == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long s = 0;
        for (int k = 0; k < MESH_THREADS / DGNN_WAVE; ++k) s += part[k];
        if (s) atomicAdd(dst, (unsigned long long)s);
    }
    __syncthreads();
}

__device__ __forceinline__ uint64_t mm_hash(uint64_t seed, uint64_t ctr) {
    return mix64(seed + ctr * 0x9E3779B97F4A7C15ull);
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
