// Fixed-order fp64 sums / inclusive scans of a device array (meshmetrics.hip: cumulative areas, distance sums; cutterms.hip: the mean facet
// area): the result depends on the data alone, not on the launch.
#pragma once
#include "common.h"

// chunk t = [t C, (t + 1) C): a serial inclusive scan in place (scan != 0) or a serial sum; chunk totals -> part[t]
constexpr int FIXED_SUM_CHUNK = 256;   // elements per serial partial sum / scan chunk
constexpr int FIXED_SUM_THREADS = 256;

namespace {

template <typename T>
__global__ void k_chunk(T* __restrict__ x, int64_t n, int scan, double* __restrict__ part) {
    const int64_t nch = (n + FIXED_SUM_CHUNK - 1) / FIXED_SUM_CHUNK;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < nch; t += (int64_t)gridDim.x * blockDim.x) {
        double s = 0;
        const int64_t e = (t + 1) * FIXED_SUM_CHUNK < n ? (t + 1) * FIXED_SUM_CHUNK : n;
        for (int64_t i = t * FIXED_SUM_CHUNK; i < e; ++i) {
            s += (double)x[i];
            if (scan) x[i] = (T)s;
        }
        part[t] = s;
    }
}

// part[] -> exclusive offsets in place, serially (so a scan is monotone and its last element equals *total bit for bit)
__global__ void k_chunk_offsets(double* __restrict__ part, int64_t nch, double* __restrict__ total) {
    if (threadIdx.x != 0) return;
    double acc = 0;
    for (int64_t t = 0; t < nch; ++t) { const double r = part[t]; part[t] = acc; acc += r; }
    *total = acc;
}

// fixed-order fp64 sum of x[0, n) -> *total (device); part: dgnn_cdiv(n, FIXED_SUM_CHUNK) + 1 doubles
template <typename T>
void fixed_sum(T* x, int64_t n, int scan, double* part, double* total, hipStream_t stream) {
    const int64_t nch = dgnn_cdiv(n, FIXED_SUM_CHUNK);
    hipLaunchKernelGGL(k_chunk<T>, dim3(dgnn_grid_cap(dgnn_cdiv(nch > 0 ? nch : 1, FIXED_SUM_THREADS))), dim3(FIXED_SUM_THREADS), 0, stream, x, n, scan,
                       part);
    hipLaunchKernelGGL(k_chunk_offsets, dim3(1), dim3(64), 0, stream, part, nch, total);
}

}  // namespace
