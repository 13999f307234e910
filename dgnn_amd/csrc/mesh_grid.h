// The candidate grid of meshcontains.hip (xy cells), raycast.hip and meshdist.hip (3D cells): every box t of a list (a face's
// bounding box in cells) is entered in every cell it touches, by count / scan / fill through a cursor with ONE WORK ITEM PER (box, cell)
// ENTRY, so a box over the whole grid costs what its entries cost, spread over the machine.  The user supplies tcnt[t] = the cells of box
// t and a by-value policy with cell(t, k) = the cell of the k-th entry of box t (its own order, its own index width).
#pragma once
#include <math.h>

#include "mesh_common.h"
#include "vec3.h"

int dgnn_exclusive_scan_i32(const int32_t* in, int64_t n, int32_t* out, int32_t* sums_scratch, hipStream_t stream);   // plan.hip

namespace {

struct GridBufs { int32_t *tcnt, *toff, *ccnt, *rowptr, *sums; };
inline GridBufs take_grid(Take& t, int64_t n_boxes, int64_t max_cells) {
    GridBufs B{};
    const int64_t m = n_boxes > max_cells ? n_boxes : max_cells;
    B.tcnt = t.take<int32_t>(n_boxes + 1);
    B.toff = t.take<int32_t>(n_boxes + 1);
    B.ccnt = t.take<int32_t>(max_cells + 1);
    B.rowptr = t.take<int32_t>(max_cells + 1);
    B.sums = t.take<int32_t>(dgnn_cdiv(m + 1, 2048) + 2);
    return B;
}

// entry e belongs to the box t with toff[t] <= e < toff[t + 1] (toff ascending, toff[n] = n_entries: the search ends inside [0, n))
__device__ __forceinline__ int64_t grid_entry_box(const int32_t* __restrict__ toff, int64_t n, int32_t e) {
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (toff[mid] <= e) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// fill == 0: ccnt[cell] += 1; fill != 0: entries[cursor[cell]++] = t (the order inside a cell is whatever the atomics give: no reader of
// the grid depends on it)
template <typename Cells>
__global__ void k_grid_entries(const int32_t* __restrict__ toff, int64_t n, Cells cells, int64_t n_entries, int fill, int32_t* __restrict__ ccnt,
                               int32_t* __restrict__ entries) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n_entries; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = grid_entry_box(toff, n, (int32_t)e);
        const int32_t slot = atomicAdd(ccnt + cells.cell(t, (int32_t)e - toff[t]), 1);
        if (fill) entries[slot] = (int32_t)t;
    }
}

// B.tcnt filled -> B.rowptr over n_cells cells and `entries` (ne of them)
template <typename Cells>
int build_entry_grid(const GridBufs& B, const Cells& cells, int64_t n, int64_t n_cells, int64_t ne, int32_t* entries, hipStream_t stream) {
    const dim3 block(MESH_THREADS);
    int rc;
    if ((rc = dgnn_exclusive_scan_i32(B.tcnt, n, B.toff, B.sums, stream))) return rc;
    (void)hipMemsetAsync(B.ccnt, 0, sizeof(int32_t) * (n_cells + 1), stream);
    hipLaunchKernelGGL(k_grid_entries<Cells>, mesh_launch_grid(ne), block, 0, stream, B.toff, n, cells, ne, 0, B.ccnt, (int32_t*)nullptr);
    if ((rc = dgnn_exclusive_scan_i32(B.ccnt, n_cells, B.rowptr, B.sums, stream))) return rc;
    (void)hipMemcpyAsync(B.ccnt, B.rowptr, sizeof(int32_t) * (n_cells + 1), hipMemcpyDeviceToDevice, stream);   // the fill's cursors
    hipLaunchKernelGGL(k_grid_entries<Cells>, mesh_launch_grid(ne), block, 0, stream, B.toff, n, cells, ne, 1, B.ccnt, entries);
    return DGNN_OK;
}

// ---- the 3D frame of raycast.hip and meshdist.hip: a uniform grid over a box, every face entered in the cells of its bounding box ------
struct CellGrid {          // by value to the kernels
    double lo[3], hi[3], inv[3], h[3];        // cells per unit length (0 on an axis without extent) and the cell's edge
    int32_t n[3];
    double mag;                               // the largest |coordinate| of the box
};

// about cubic cells over [lo, hi]: R along the longest axis, one where there is no extent
inline CellGrid cell_grid_frame(const double* lo, const double* hi, int32_t R) {
    CellGrid g{};
    double longest = 0.0;
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = lo[a];
        g.hi[a] = hi[a];
        longest = fmax(longest, hi[a] - lo[a]);
        g.mag = fmax(g.mag, fmax(fabs(lo[a]), fabs(hi[a])));
    }
    for (int a = 0; a < 3; ++a) {
        const double ext = hi[a] - lo[a];
        double cells = longest > 0 ? ceil(ext / (longest / R)) : 1.0;
        cells = cells < 1 ? 1 : (cells > R ? R : cells);
        g.n[a] = (int32_t)cells;
        g.h[a] = ext / cells;
        g.inv[a] = ext > 0 ? cells / ext : 0.0;
        if (!isfinite(g.inv[a]) || !isfinite(ext)) { g.n[a] = 1; g.h[a] = ext; g.inv[a] = 0.0; }          // an extent below 2^-1022 or so, or above 2^1024: one cell
    }
    return g;
}

// the cell of coordinate x on axis a: a chain of monotone steps (difference, product, truncation, clamp), so x <= y gives cell(x) <= cell(y)
__device__ __forceinline__ int32_t grid_cell(const CellGrid& g, int a, double x) {
    const double f = (x - g.lo[a]) * g.inv[a];
    return !(f > 0) ? 0 : (f >= (double)g.n[a] ? g.n[a] - 1 : (int32_t)f);
}

struct CellBox { int32_t lo[3], hi[3]; };

// tbox[t] = the cells of the face's bounding box; tcnt[t] = their number; the total -> *total (an integer sum: order-free)
__global__ void __launch_bounds__(MESH_THREADS) k_cell_boxes(const double* __restrict__ v, const int32_t* __restrict__ faces, int64_t nf, CellGrid g,
                                                           CellBox* __restrict__ tbox, int32_t* __restrict__ tcnt, unsigned long long* total) {
    using namespace dgnn_exact;
    unsigned long long tot = 0;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < nf; t += (int64_t)gridDim.x * blockDim.x) {
        const V3 a = load_v3(v, faces[3 * t]), b = load_v3(v, faces[3 * t + 1]), c = load_v3(v, faces[3 * t + 2]);
        CellBox bx;
        int64_t cnt = 1;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            bx.lo[k] = grid_cell(g, k, fmin(fmin(get(a, k), get(b, k)), get(c, k)));
            bx.hi[k] = grid_cell(g, k, fmax(fmax(get(a, k), get(b, k)), get(c, k)));
            cnt *= bx.hi[k] - bx.lo[k] + 1;
        }
        tbox[t] = bx;
        tcnt[t] = (int32_t)cnt;          // <= 1024^3 = 2^30
        tot += (unsigned long long)cnt;
    }
    wave_add_atomic(tot, total);
}

// the cell policy of build_entry_grid: the cells of box t, z fastest (the order inside a cell is whatever the builder's atomics give: the
// readers take a minimum under a total order)
struct BoxCells {
    const CellBox* tbox;
    int32_t n1, n2;          // the grid's cells along y and z
    __device__ int64_t cell(int64_t t, int32_t k) const {
        const CellBox b = tbox[t];
        const int32_t nz = b.hi[2] - b.lo[2] + 1, ny = b.hi[1] - b.lo[1] + 1;
        const int32_t z = b.lo[2] + k % nz;
        k /= nz;
        const int32_t y = b.lo[1] + k % ny, x = b.lo[0] + k / ny;
        return ((int64_t)x * n1 + y) * n2 + z;
    }
};

}  // namespace
