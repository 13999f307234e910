// A point set binned in mesh_grid.h's frame over its own box, shared by knn.hip and scansub.hip (§35): the box with the refusal of
// non-finite coordinates, the (x, y, z, index) records binned cell after cell (z fastest) by count / scan / fill, and the fp64 squared distance
// both files state.  Everything rounds on its own (-ffp-contract=off).
#pragma once
#include "mesh_grid.h"

namespace {

constexpr int32_t KNN_NONFINITE = 1, KNN_BAD_ID = 2;
constexpr int KNN_MAX_R = 1024;

struct PointBox {
    int32_t err, pad;
    unsigned long long lo[3], hi[3];          // bbox of the points (f64_key); lo preset to ~0, hi to 0
};

struct KnnPoint { double x, y, z; int32_t id, pad; };          // a binned record; pad: the caller's word (knn: 0; thinning: the point's rank)

__global__ void __launch_bounds__(MESH_THREADS) k_knn_bbox(const double* __restrict__ p, int64_t n, PointBox* st) {
    unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0, 0, 0};
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        for (int a = 0; a < 3; ++a) {
            const double x = p[3 * i + a];
            if (!isfinite(x)) { atomicOr(&st->err, KNN_NONFINITE); continue; }
            const unsigned long long k = f64_key(x);
            lo[a] = k < lo[a] ? k : lo[a];
            hi[a] = k > hi[a] ? k : hi[a];
        }
    for (int a = 0; a < 3; ++a) wave_minmax_atomic(lo[a], hi[a], st->lo + a, st->hi + a);
}

// fill == 0: ccnt[cell] += 1; fill != 0: rec[cursor[cell]++] = (x, y, z, i, pad[i] or 0).  Both passes map a point to the same cell, so a
// cursor never leaves its cell's run and every slot is below n.
__global__ void k_knn_bin(const double* __restrict__ p, int64_t n, CellGrid g, int fill, int32_t* __restrict__ ccnt, KnnPoint* __restrict__ rec,
                          const int32_t* __restrict__ pad) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
        const int64_t cell = ((int64_t)grid_cell(g, 0, x) * g.n[1] + grid_cell(g, 1, y)) * g.n[2] + grid_cell(g, 2, z);
        const int32_t slot = atomicAdd(ccnt + cell, 1);
        if (fill) rec[slot] = KnnPoint{x, y, z, (int32_t)i, pad ? pad[i] : 0};
    }
}

__device__ __forceinline__ double knn_d2(const double (&q)[3], double x, double y, double z) {
    const double dx = q[0] - x, dy = q[1] - y, dz = q[2] - z;
    return (dx * dx + dy * dy) + dz * dz;
}

// the bins of n points in a grid of at most R^3 cells
struct PointBins { int32_t *ccnt, *rowptr, *sums; KnnPoint* rec; };
inline PointBins take_point_bins(Take& t, int64_t n, int64_t R) {
    const int64_t cells = R * R * R;
    PointBins B{};
    B.ccnt = t.take<int32_t>(cells + 1);
    B.rowptr = t.take<int32_t>(cells + 1);
    B.sums = t.take<int32_t>(dgnn_cdiv(cells + 1, 2048) + 2);
    B.rec = t.take<KnnPoint>(n);
    return B;
}

// the box read back (finite, n > 0) -> the frame at resolution R and the records of the points in it; pad: per point, or NULL
inline int bin_points(const double* points, int64_t n, const PointBox& box, int32_t R, const PointBins& B, const int32_t* pad, CellGrid* g_out,
                      hipStream_t stream) {
    double lo[3], hi[3];
    bbox_unkey(box.lo, box.hi, lo, hi);
    const CellGrid g = cell_grid_frame(lo, hi, R);
    const int64_t cells = (int64_t)g.n[0] * g.n[1] * g.n[2];
    const dim3 block(MESH_THREADS);
    (void)hipMemsetAsync(B.ccnt, 0, sizeof(int32_t) * (cells + 1), stream);
    hipLaunchKernelGGL(k_knn_bin, mesh_launch_grid(n), block, 0, stream, points, n, g, 0, B.ccnt, (KnnPoint*)nullptr, (const int32_t*)nullptr);
    const int rc = dgnn_exclusive_scan_i32(B.ccnt, cells, B.rowptr, B.sums, stream);
    if (rc) return rc;
    (void)hipMemcpyAsync(B.ccnt, B.rowptr, sizeof(int32_t) * (cells + 1), hipMemcpyDeviceToDevice, stream);   // the fill's cursors
    hipLaunchKernelGGL(k_knn_bin, mesh_launch_grid(n), block, 0, stream, points, n, g, 1, B.ccnt, B.rec, pad);
    *g_out = g;
    return DGNN_OK;
}

inline bool knn_resolution_ok(int32_t R) { return R >= 0 && R <= KNN_MAX_R; }

}  // namespace
