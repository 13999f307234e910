// Pieces shared by the kernels that read a triangle list (meshtopo.hip, meshcomp.hip) and by the scene kernels that report through the same
// status word: the status word and its synchronising read, the face check, the sorted undirected-edge keys, the lock-free union-find and the
// radix-sort workspace.
#pragma once
#include "mesh_common.h"

int dgnn_exclusive_scan_i32(const int32_t* in, int64_t n, int32_t* out, int32_t* sums_scratch, hipStream_t stream);   // plan.hip
int64_t dgnn_radix_sort_hist_elems(int64_t n);                                                                       // reorder.hip
int dgnn_radix_sort_u64_i32(uint64_t* const keys[2], int32_t* const vals[2], int64_t n, int bits, int32_t* hist, int32_t* scanned, int32_t* sums,
                            hipStream_t stream, int* cur);

namespace {

// status bits
constexpr int32_t MT_BAD_ID = 1, MT_NONFINITE = 2, MT_NOT_FACE = 4, MT_NOT_INTERFACE = 8, MT_RANGE = 16, MT_DEGENERATE = 32, MT_PASSES = 64;

struct MtState {
    int32_t err, exact_used, pad[2];
    unsigned long long undetermined;
};

__global__ void k_check_faces(const int32_t* __restrict__ faces, int64_t n, int64_t nv, MtState* st) {
    for (int64_t f = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; f < n; f += (int64_t)gridDim.x * blockDim.x) {
        const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        if (a < 0 || a >= nv || b < 0 || b >= nv || c < 0 || c >= nv) atomicOr(&st->err, MT_BAD_ID);
        else if (a == b || b == c || a == c) atomicOr(&st->err, MT_DEGENERATE);
    }
}

// edge e = 3 f + k runs from corner k to corner k + 1 of face f: key (min, max); value: the face f when face_vals != 0, else +1 when the
// edge runs from min to max and -1 when it runs from max to min
__global__ void k_edge_keys(const int32_t* __restrict__ faces, int64_t n3, int vb, int face_vals, uint64_t* __restrict__ keys,
                            int32_t* __restrict__ vals) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n3; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = e / 3;
        const int k = (int)(e - 3 * f);
        const uint32_t u = (uint32_t)faces[3 * f + k], v = (uint32_t)faces[3 * f + (k + 1) % 3];
        const uint32_t lo = u < v ? u : v, hi = u < v ? v : u;
        keys[e] = ((uint64_t)lo << vb) | hi;
        vals[e] = face_vals ? (int32_t)f : (u < v ? 1 : -1);
    }
}

__device__ __forceinline__ int32_t uf_load(int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x (parent pointers only ever move to an ancestor: path halving is a benign race)
__device__ __forceinline__ int32_t uf_find(int32_t* parent, int32_t x) {
    for (;;) {
        const int32_t p = uf_load(parent + x);
        if (p == x) return x;
        const int32_t g = uf_load(parent + p);
        if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
    }
}

// joins the sets of a and b: the larger root is hooked under the smaller one; a failed compare-and-swap (the root was hooked meanwhile) retries
__device__ __forceinline__ void uf_union(int32_t* parent, int32_t a, int32_t b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a < b) { const int32_t t = a; a = b; b = t; }
        int32_t expected = a;
        if (__hip_atomic_compare_exchange_strong(parent + a, &expected, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    }
}

// elements with equal keys are joined, each with its predecessor in the sorted order
__global__ void k_link_union(const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals, int64_t n, int32_t* parent) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        if (i > 0 && keys[i - 1] == keys[i]) uf_union(parent, vals[i - 1], vals[i]);
}

int mt_read_status(MtState* hs, const MtState* st, hipStream_t stream, const char* what) {
    int rc = dgnn_check_launch(what);
    if (rc || (rc = mm_read(hs, st, sizeof(MtState), stream, what))) return rc;
    if (!hs->err) return DGNN_OK;
    const int32_t e = hs->err;
    dgnn_set_error("%s: %s%s%s%s%s%s%s", what, e & MT_BAD_ID ? "an id out of range; " : "", e & MT_NONFINITE ? "non-finite coordinates; " : "",
                   e & MT_NOT_FACE ? "a facet that is not a face of the cell nfacets names; " : "",
                   e & MT_NOT_INTERFACE ? "a facet that does not separate an inside cell from an outside one; " : "",
                   e & MT_RANGE ? "a coordinate magnitude outside [2^-300, 2^300] (the exact predicate's range); " : "",
                   e & MT_DEGENERATE ? "a face with a repeated vertex; " : "",
                   e & MT_PASSES ? "the counting and the filling pass disagree (the inputs changed during the call?); " : "");
    return e == MT_RANGE ? DGNN_E_UNSUPPORTED : DGNN_E_INVALID;
}

// the workspace of dgnn_radix_sort_u64_i32 for m elements: the two key and value buffers it ping-pongs between, its histogram and scan
struct SortBufs { uint64_t* keys[2]; int32_t *vals[2], *hist, *scanned, *sums; };
void take_sort(Take& t, int64_t m, SortBufs& S) {
    const int64_t h = dgnn_radix_sort_hist_elems(m);
    S.keys[0] = t.take<uint64_t>(m);
    S.keys[1] = t.take<uint64_t>(m);
    S.vals[0] = t.take<int32_t>(m);
    S.vals[1] = t.take<int32_t>(m);
    S.hist = t.take<int32_t>(h);
    S.scanned = t.take<int32_t>(h);
    S.sums = t.take<int32_t>(dgnn_cdiv(h, 2048) + 4);
}
// sorts S.keys[0] / S.vals[0]; the result is in S.keys[*cur] / S.vals[*cur]
int sort_pairs(const SortBufs& S, int64_t n, int bits, hipStream_t stream, int* cur) {
    return dgnn_radix_sort_u64_i32(S.keys, S.vals, n, bits, S.hist, S.scanned, S.sums, stream, cur);
}

int key_bits(int64_t nv) {
    int b = 1;
    while (b < 31 && ((int64_t)1 << b) < nv) ++b;
    return b;
}

}  // namespace
