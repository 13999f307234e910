// The candidate grid of meshcontains.hip (xy cells) and raycast.hip (3D cells): every box t of a list (a face's
// bounding box in cells) is entered in every cell it touches, by count / scan / fill through a cursor with ONE WORK ITEM PER (box, cell)
// ENTRY, so a box over the whole grid costs what its entries cost, spread over the machine.  The user supplies tcnt[t] = the cells of box
// t and a by-value policy with cell(t, k) = the cell of the k-th entry of box t (its own order, its own index width).
#pragma once
#include "mesh_common.h"

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

}  // namespace
