// The steps that the two vertex-ray operations share (scenefeat.hip: dgnn_vertex_rays; raywalk.hip: dgnn_ray_walk): the first-ray kernel and
// the preset of its array, the incident-corner prologue over a row of dgnn_vertex_incidence, the unit direction and the plane distance (in
// the operation order include/dgnn_hip.h states), the runs of a sorted key array and the accumulator that folds a run.
#pragma once
#include "exact_orient.h"
#include "mesh_faces.h"
#include "tet_common.h"

namespace {

using dgnn_exact::V3;
using dgnn_exact::load_v3;

// ---- first[v] = the lowest ray index of vertex v ----------------------------------------------------------------------------------
// first[] is preset bytewise to 0x7f7f7f7f, which has to lie above every ray index: each operation bounds its ray count by this or less
constexpr int64_t RAY_FIRST_NONE = 0x7f7f7f7f;
inline void ray_first_preset(int32_t* first, int64_t nv, hipStream_t stream) {
    if (nv > 0) (void)hipMemsetAsync(first, 0x7f, sizeof(int32_t) * nv, stream);
}

// checks the ids of the rays; with `unique`, first[v] = the lowest ray index of vertex v
__global__ void k_ray_first(const int32_t* __restrict__ ray_vertex, int64_t nr, int64_t nv, int unique, int32_t* first, int32_t* err) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < nr; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t a = ray_vertex[r];
        if (a < 0 || a >= nv) atomicOr(err, MT_BAD_ID);
        else if (unique) atomicMin(first + a, (int32_t)r);
    }
}

// ---- the incident corners of a ray's vertex ---------------------------------------------------------------------------------------
// the row [b, e) of vertex vid in the incidence; false and MT_BAD_ID when it does not lie in the 4 nt corners
__device__ __forceinline__ bool corner_row(const int32_t* __restrict__ rowptr, int32_t vid, int64_t nt, int64_t& b, int64_t& e, MtState* st) {
    b = rowptr[vid];
    e = rowptr[vid + 1];
    if (b < 0 || e < b || e > 4 * nt) { atomicOr(&st->err, MT_BAD_ID); return false; }
    return true;
}
// an entry of that row as (tet, slot); false and MT_BAD_ID when it is not a corner of this vertex
__device__ __forceinline__ bool corner_of(const int32_t* __restrict__ tets, int64_t nt, int32_t ent, int32_t vid, int32_t& t, int& k, MtState* st) {
    if (ent < 0 || ent >= 4 * nt || tets[ent] != vid) { atomicOr(&st->err, MT_BAD_ID); return false; }
    t = ent >> 2;
    k = ent & 3;
    return true;
}

// ---- lengths along a ray ----------------------------------------------------------------------------------------------------------
// e / |e| (flip = 0) or its negative (flip = 1): the square root, three divisions, then the negation; len = |e|
__device__ __forceinline__ V3 unit_ray(const V3& e, int flip, double& len) {
    len = sqrt(dot(e, e));
    V3 d{e.x / len, e.y / len, e.z / len};
    if (flip) d = V3{-d.x, -d.y, -d.z};
    return d;
}
// the length from p along the unit direction d to the plane of (q0, q1, q2): n = (q1 - q0) X (q2 - q0), den = n . d, n . (q0 - p) / den
__device__ __forceinline__ double plane_distance(const V3& p, const V3& d, const V3& q0, const V3& q1, const V3& q2, double& den) {
    const V3 n = cross(sub(q1, q0), sub(q2, q0));
    den = dot(n, d);
    return dot(n, sub(q0, p)) / den;
}

// ---- runs and folds ---------------------------------------------------------------------------------------------------------------
// sorted keys -> per key below n_keys the run [run_begin, run_end) of its elements (the caller zeroes both: no element, an empty run)
__global__ void k_ray_runs(const uint64_t* __restrict__ keys, int64_t n, int64_t n_keys, int32_t* __restrict__ run_begin, int32_t* __restrict__ run_end) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t c = keys[i];
        if (c >= (uint64_t)n_keys) continue;
        if (i == 0 || keys[i - 1] != c) run_begin[c] = (int32_t)i;
        if (i == n - 1 || keys[i + 1] != c) run_end[c] = (int32_t)(i + 1);
    }
}

// min, max and sum of one column, from nothing or continuing from memory (stat[0], stat[stride], stat[2 stride]).  The count stays with the
// caller -- several columns share one -- and add() takes the count before the value.
struct Fold {
    double lo = 0.0, hi = 0.0, sum = 0.0;
    __device__ __forceinline__ void load(const double* stat, int64_t stride) { lo = stat[0]; hi = stat[stride]; sum = stat[2 * stride]; }
    __device__ __forceinline__ void store(double* stat, int64_t stride) const { stat[0] = lo; stat[stride] = hi; stat[2 * stride] = sum; }
    __device__ __forceinline__ void add(int32_t n, double d) {
        lo = n == 0 ? d : (d < lo ? d : lo);
        hi = n == 0 ? d : (d > hi ? d : hi);
        sum = sum + d;
    }
};

}  // namespace
