// A row of a cell list (`tetrahedra` [T, 4], `neighbors` [T, 4]): its load, slot -> id, slot -> the ids around it, the id range test, and the
// one rule for "this facet is a face of this cell".  (Not in mesh_faces.h: that is about triangle lists and brings their kernels, which
// cutterms.hip and facetgeom.hip do not want.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// ---- a row as the kernel holds it: four ids behind a pointer, or one 16-byte load (the caller has checked the alignment) -----------
__device__ __forceinline__ int4 load_row(const int32_t* __restrict__ rows, int64_t c) { return *reinterpret_cast<const int4*>(rows + 4 * c); }
__device__ __forceinline__ int32_t row_at(int32_t t0, int32_t t1, int32_t t2, int32_t t3, int k) { return k == 0 ? t0 : (k == 1 ? t1 : (k == 2 ? t2 : t3)); }
__device__ __forceinline__ int32_t row_at(const int4& r, int k) { return k == 0 ? r.x : (k == 1 ? r.y : (k == 2 ? r.z : r.w)); }
__device__ __forceinline__ int32_t row_at(const int32_t t[4], int k) { return row_at(t[0], t[1], t[2], t[3], k); }

// the ids of the other three vertices around slot k, in slot order
__device__ __forceinline__ void row_others(const int4& r, int k, int32_t& a, int32_t& b, int32_t& c) {
    a = k <= 0 ? r.y : r.x;
    b = k <= 1 ? r.z : r.y;
    c = k <= 2 ? r.w : r.z;
}
__device__ __forceinline__ void row_others(const int32_t* __restrict__ row, int k, int32_t& a, int32_t& b, int32_t& c) {
    a = row[k <= 0];
    b = row[1 + (k <= 1)];
    c = row[2 + (k <= 2)];
}

// every id of the row in [0, nv)
__device__ __forceinline__ bool tet_ids_ok(int32_t i0, int32_t i1, int32_t i2, int32_t i3, int64_t nv) {
    return !(i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv || i3 < 0 || i3 >= nv);
}
__device__ __forceinline__ bool tet_ids_ok(const int32_t t[4], int64_t nv) { return tet_ids_ok(t[0], t[1], t[2], t[3], nv); }

// ---- the facet / slot rule -------------------------------------------------------------------------------------------------------
// The facet (ia, ib, ic) is a face of the cell t[0..3] when exactly three slots of the cell hold a vertex of the facet AND each vertex of
// the facet occurs in the cell.  (The second half matters for a cell that repeats a vertex: (0, 0, 1, 3) has three slots on the facet
// (0, 1, 2) and is not a cell of it.)  Returns the slot of the cell's one vertex that is not on the facet, -1 when the facet is no face.
__device__ __forceinline__ int facet_opposite_slot(const int32_t t[4], int32_t ia, int32_t ib, int32_t ic) {
    int in = 0, slot = -1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (t[k] == ia || t[k] == ib || t[k] == ic) ++in;
        else slot = k;
    }
    const bool has = (t[0] == ia || t[1] == ia || t[2] == ia || t[3] == ia) && (t[0] == ib || t[1] == ib || t[2] == ib || t[3] == ib) &&
                     (t[0] == ic || t[1] == ic || t[2] == ic || t[3] == ic);
    return in == 3 && has ? slot : -1;
}
__device__ __forceinline__ int facet_opposite_slot(const int4& r, int32_t ia, int32_t ib, int32_t ic) {
    const int32_t t[4] = {r.x, r.y, r.z, r.w};
    return facet_opposite_slot(t, ia, ib, ic);
}

}  // namespace
