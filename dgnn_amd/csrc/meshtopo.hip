// The mesh `generate` returns (reference processing/generate_mesh.py:107-124: trimesh.Trimesh(process=True), fix_normals, Open3D's
// is_watertight), built on the device.  DESIGN §15.
//
//   orient     every interface facet wound so that its normal points away from its inside cell: the exact sign of
//              det[b - a, c - a, d - a] for the inside cell's opposite vertex d (exact_orient.h), the outside cell's when the inside
//              cell is flat, the stored winding (counted) when both are flat or the outside cell is the infinite one.  One thread per facet.
//   compact    the referenced vertices in ascending id (flags, then dgnn_compact_i32) and the faces renumbered onto them.
//   topology   edge counts from the sorted undirected edge keys (one thread per run of equal keys); vertex fans from the sorted
//              (vertex, link vertex) keys of every face corner: corners that share a key are joined in a union-find (hooking the larger
//              root under the smaller by compare-and-swap), and a vertex is non-manifold when its corners keep two or more roots.
//              Integer sums only: the counts do not depend on the schedule.
#include "exact_orient.h"
#include "mesh_faces.h"
#include "tet_common.h"

namespace {

using dgnn_exact::V3;
using dgnn_exact::load_v3;

// the status bits of a point whose coordinates the exact predicate cannot take
__device__ __forceinline__ int32_t coord_bits(const V3& p) {
    int32_t e = 0;
    const double c[3] = {p.x, p.y, p.z};
    for (int k = 0; k < 3; ++k) {
        const dgnn_exact::CoordClass cls = dgnn_exact::coord_class(c[k]);
        if (cls == dgnn_exact::COORD_NONFINITE) e |= MT_NONFINITE;
        else if (cls == dgnn_exact::COORD_RANGE) e |= MT_RANGE;
    }
    return e;
}

// the vertex of cell c that is not x, y or z; -1 when (x, y, z) is not a face of c (tet_common.h: the facet / slot rule)
__device__ __forceinline__ int32_t opposite_vertex(const int32_t* __restrict__ tets, int32_t c, int32_t x, int32_t y, int32_t z) {
    const int32_t* const row = tets + 4 * (int64_t)c;
    const int slot = facet_opposite_slot(row, x, y, z);
    return slot < 0 ? -1 : row[slot];
}

// ---- orientation -------------------------------------------------------------------------------------------------------------
__global__ void k_orient(const double* __restrict__ vert, int64_t nv, const int32_t* __restrict__ tets, int64_t nc,
                         const int32_t* __restrict__ facets, const int32_t* __restrict__ nfacets, int64_t nf, const int32_t* __restrict__ labels,
                         const int32_t* __restrict__ ids, int64_t n, int orient, int32_t* __restrict__ out, MtState* st) {
    unsigned long long n_und = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t f = ids[i];
        int32_t err = 0, und = 0, used = 0;
        int32_t x = 0, y = 0, z = 0;
        if (f < 0 || f >= nf) err = MT_BAD_ID;
        else {
            x = facets[3 * (int64_t)f];
            y = facets[3 * (int64_t)f + 1];
            z = facets[3 * (int64_t)f + 2];
            const int32_t c0 = nfacets[2 * (int64_t)f], c1 = nfacets[2 * (int64_t)f + 1];
            if (x < 0 || x >= nv || y < 0 || y >= nv || z < 0 || z >= nv || c0 < -1 || c0 >= nc || c1 < -1 || c1 >= nc) err = MT_BAD_ID;
            else {
                const bool in0 = c0 >= 0 && labels[c0] == 0, in1 = c1 >= 0 && labels[c1] == 0;   // -1 = the infinite cell = outside
                const int32_t ci = in0 ? c0 : c1, co = in0 ? c1 : c0;
                int32_t d_in = -1, d_out = -1;
                if (in0 == in1) err = MT_NOT_INTERFACE;
                else if ((d_in = opposite_vertex(tets, ci, x, y, z)) < 0 || (co >= 0 && (d_out = opposite_vertex(tets, co, x, y, z)) < 0)) err = MT_NOT_FACE;
                else if (d_in >= nv || d_out >= nv) err = MT_BAD_ID;
                else if (orient) {
                    const V3 a = load_v3(vert, x), b = load_v3(vert, y), c = load_v3(vert, z), din = load_v3(vert, d_in);
                    err = coord_bits(a) | coord_bits(b) | coord_bits(c) | coord_bits(din);
                    if (co >= 0) err |= coord_bits(load_v3(vert, d_out));
                    if (!err) {
                        int s = dgnn_exact::orient_sign(a, b, c, din, &used);
                        if (s == 0 && co >= 0) s = -dgnn_exact::orient_sign(a, b, c, load_v3(vert, d_out), &used);
                        if (s > 0) { const int32_t t = y; y = z; z = t; }
                        und = s == 0;
                    }
                }
            }
        }
        if (err) atomicOr(&st->err, err);
        if (used) atomicOr(&st->exact_used, 1);
        n_und += und;
        out[3 * i] = x;
        out[3 * i + 1] = y;
        out[3 * i + 2] = z;
    }
    wave_add_atomic(n_und, &st->undetermined);   // every lane is here: the loop has ended for all of them
}

// ---- vertex compaction ---------------------------------------------------------------------------------------------------------
__global__ void k_mark_vertices(const int32_t* __restrict__ faces, int64_t n3, int64_t nv, int32_t* __restrict__ flags, MtState* st) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n3; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t v = faces[i];
        if (v < 0 || v >= nv) atomicOr(&st->err, MT_BAD_ID);
        else flags[v] = 1;   // every writer stores the same value
    }
}

__global__ void k_new_ids(const int32_t* __restrict__ kept, const int32_t* __restrict__ n_kept, int32_t* __restrict__ new_id) {
    const int64_t m = *n_kept;
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) new_id[kept[j]] = (int32_t)j;
}

__global__ void k_renumber(const int32_t* __restrict__ faces, int64_t n3, const int32_t* __restrict__ new_id, int32_t* __restrict__ out) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n3; i += (int64_t)gridDim.x * blockDim.x) out[i] = new_id[faces[i]];
}

// ---- topology (the face check, the edge keys and the union-find: mesh_faces.h) ---------------------------------------------------
// one thread per run of equal keys (its first element): faces on the edge = run length, directed balance = sum of the values
__global__ void k_edge_runs(const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals, int64_t n, long long* __restrict__ counts) {
    unsigned long long edges = 0, boundary = 0, nonmanifold = 0, mismatch = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (i > 0 && keys[i - 1] == keys[i]) continue;
        int64_t len = 0, bal = 0;
        for (int64_t j = i; j < n && keys[j] == keys[i]; ++j) { ++len; bal += vals[j]; }
        ++edges;
        boundary += len == 1;
        nonmanifold += len >= 3;
        mismatch += bal != 0;
    }
    edges = wave_sum(edges);
    boundary = wave_sum(boundary);
    nonmanifold = wave_sum(nonmanifold);
    mismatch = wave_sum(mismatch);
    if (lane_id() == 0) {
        if (edges) atomicAdd((unsigned long long*)&counts[0], edges);
        if (boundary) atomicAdd((unsigned long long*)&counts[1], boundary);
        if (nonmanifold) atomicAdd((unsigned long long*)&counts[2], nonmanifold);
        if (mismatch) atomicAdd((unsigned long long*)&counts[4], mismatch);
    }
}

// corner c = 3 f + k (vertex v = faces[c]) gives keys (v, x) and (v, y) for the face's two other vertices x, y; value c.  parent[c] = c.
__global__ void k_link_keys(const int32_t* __restrict__ faces, int64_t n3, int vb, uint64_t* __restrict__ keys, int32_t* __restrict__ vals,
                            int32_t* __restrict__ parent) {
    for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < n3; c += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = c / 3;
        const int k = (int)(c - 3 * f);
        const uint64_t v = (uint32_t)faces[c], x = (uint32_t)faces[3 * f + (k + 1) % 3], y = (uint32_t)faces[3 * f + (k + 2) % 3];
        keys[2 * c] = (v << vb) | x;
        keys[2 * c + 1] = (v << vb) | y;
        vals[2 * c] = vals[2 * c + 1] = (int32_t)c;
        parent[c] = (int32_t)c;
    }
}

// after every union: one root per fan; roots[v] = number of fans of v
__global__ void k_fan_roots(const int32_t* __restrict__ faces, const int32_t* __restrict__ parent, int64_t n3, int32_t* __restrict__ roots) {
    for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < n3; c += (int64_t)gridDim.x * blockDim.x)
        if (parent[c] == (int32_t)c) atomicAdd(roots + faces[c], 1);
}

__global__ void k_fan_count(const int32_t* __restrict__ roots, int64_t nv, long long* __restrict__ counts) {
    unsigned long long bad = 0;
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < nv; v += (int64_t)gridDim.x * blockDim.x) bad += roots[v] >= 2;
    bad = wave_sum(bad);
    if (lane_id() == 0 && bad) atomicAdd((unsigned long long*)&counts[3], bad);
}

// ---- scratch layouts, status ---------------------------------------------------------------------------------------------------
struct CompactLayout { MtState* st; int32_t *flags, *new_id, *cscratch; int64_t bytes; };
CompactLayout compact_layout(void* base, int64_t nv) {
    Take t{(char*)base, 256};
    CompactLayout L{};
    L.st = (MtState*)base;
    L.flags = t.take<int32_t>(nv);
    L.new_id = t.take<int32_t>(nv);
    L.cscratch = t.take<int32_t>(dgnn_compact_scratch_elems(nv));
    L.bytes = t.off;
    return L;
}

struct TopoLayout { MtState* st; SortBufs S; int32_t *parent, *roots; int64_t bytes; };
TopoLayout topo_layout(void* base, int64_t nfc, int64_t nv) {
    Take t{(char*)base, 256};
    TopoLayout L{};
    L.st = (MtState*)base;
    take_sort(t, 6 * nfc, L.S);   // link keys; the 3 nfc edge keys use the front
    L.parent = t.take<int32_t>(3 * nfc);
    L.roots = t.take<int32_t>(nv);
    L.bytes = t.off;
    return L;
}

}  // namespace

// ================================================================================================================================
extern "C" int64_t dgnn_orient_interface_scratch_bytes(void) { return 256; }

extern "C" int dgnn_orient_interface(const double* vertices, int64_t n_vertices, const int32_t* tets, int64_t n_cells, const int32_t* facets,
                                     const int32_t* nfacets, int64_t n_facets, const int32_t* labels, const int32_t* face_ids, int64_t n_faces,
                                     int orient, int32_t* faces_out, int64_t* n_undetermined_out, int32_t* exact_used_out, void* scratch,
                                     void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(n_vertices >= 0 && n_cells >= 0 && n_facets >= 0 && n_faces >= 0 && scratch &&
                     (n_faces == 0 || (vertices && tets && facets && nfacets && labels && face_ids && faces_out)),
                 DGNN_E_INVALID, "orient_interface: bad args");
    DGNN_REQUIRE(n_cells < INT32_MAX / 4 && n_vertices < INT32_MAX && n_facets < INT32_MAX && n_faces < INT32_MAX / 3, DGNN_E_UNSUPPORTED,
                 "orient_interface: sizes exceed the int32 indexing");
    MtState* st = (MtState*)scratch;
    (void)hipMemsetAsync(st, 0, sizeof(MtState), stream);
    if (n_faces > 0)
        hipLaunchKernelGGL(k_orient, mesh_launch_grid(n_faces), dim3(MESH_THREADS), 0, stream, vertices, n_vertices, tets, n_cells, facets, nfacets, n_facets,
                           labels, face_ids, n_faces, orient, faces_out, st);
    if (n_undetermined_out) (void)hipMemcpyAsync(n_undetermined_out, &st->undetermined, sizeof(int64_t), hipMemcpyDeviceToDevice, stream);
    if (exact_used_out) (void)hipMemcpyAsync(exact_used_out, &st->exact_used, sizeof(int32_t), hipMemcpyDeviceToDevice, stream);
    MtState hs{};
    return mt_read_status(&hs, st, stream, "orient_interface");
}

extern "C" int64_t dgnn_compact_vertices_scratch_bytes(int64_t n_vertices) {
    if (n_vertices < 0) return 0;
    return compact_layout(nullptr, n_vertices).bytes;
}

extern "C" int dgnn_compact_vertices(const int32_t* faces, int64_t n_faces, int64_t n_vertices, int32_t* faces_out, int32_t* kept_out,
                                     int32_t* n_kept_out, void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(n_faces >= 0 && n_vertices >= 0 && scratch && n_kept_out && (n_faces == 0 || (faces && faces_out)) && (n_vertices == 0 || kept_out),
                 DGNN_E_INVALID, "compact_vertices: bad args");
    DGNN_REQUIRE(n_faces < INT32_MAX / 3 && n_vertices < INT32_MAX, DGNN_E_UNSUPPORTED, "compact_vertices: sizes exceed the int32 indexing");
    const CompactLayout L = compact_layout(scratch, n_vertices);
    (void)hipMemsetAsync(L.st, 0, sizeof(MtState), stream);
    (void)hipMemsetAsync(L.flags, 0, sizeof(int32_t) * (n_vertices > 0 ? n_vertices : 1), stream);
    if (n_faces > 0) hipLaunchKernelGGL(k_mark_vertices, mesh_launch_grid(3 * n_faces), dim3(MESH_THREADS), 0, stream, faces, 3 * n_faces, n_vertices, L.flags, L.st);
    MtState hs{};
    int rc = mt_read_status(&hs, L.st, stream, "compact_vertices");
    if (rc) return rc;
    if ((rc = dgnn_compact_i32(nullptr, L.flags, 0, n_vertices, kept_out, n_kept_out, L.cscratch, stream))) return rc;
    if (n_faces > 0) {
        hipLaunchKernelGGL(k_new_ids, mesh_launch_grid(n_vertices), dim3(MESH_THREADS), 0, stream, kept_out, n_kept_out, L.new_id);
        hipLaunchKernelGGL(k_renumber, mesh_launch_grid(3 * n_faces), dim3(MESH_THREADS), 0, stream, faces, 3 * n_faces, L.new_id, faces_out);
    }
    return dgnn_check_launch("compact_vertices");
}

extern "C" int64_t dgnn_mesh_topology_scratch_bytes(int64_t n_faces, int64_t n_vertices) {
    if (n_faces < 0 || n_vertices < 0) return 0;
    return topo_layout(nullptr, n_faces, n_vertices).bytes;
}

extern "C" int dgnn_mesh_topology(const int32_t* faces, int64_t n_faces, int64_t n_vertices, int64_t* counts_out, void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(n_faces >= 0 && n_vertices >= 0 && scratch && counts_out && (n_faces == 0 || faces), DGNN_E_INVALID, "mesh_topology: bad args");
    DGNN_REQUIRE(n_faces < INT32_MAX / 6 && n_vertices < INT32_MAX, DGNN_E_UNSUPPORTED, "mesh_topology: sizes exceed the int32 indexing");
    const TopoLayout L = topo_layout(scratch, n_faces, n_vertices);
    const dim3 block(MESH_THREADS);
    (void)hipMemsetAsync(L.st, 0, sizeof(MtState), stream);
    (void)hipMemsetAsync(counts_out, 0, 5 * sizeof(int64_t), stream);
    if (n_faces > 0) hipLaunchKernelGGL(k_check_faces, mesh_launch_grid(n_faces), block, 0, stream, faces, n_faces, n_vertices, L.st);
    MtState hs{};
    int rc = mt_read_status(&hs, L.st, stream, "mesh_topology");
    if (rc || n_faces == 0) return rc;
    const int vb = key_bits(n_vertices);
    const int64_t n3 = 3 * n_faces;
    int cur = 0;
    long long* counts = (long long*)counts_out;
    // edges
    hipLaunchKernelGGL(k_edge_keys, mesh_launch_grid(n3), block, 0, stream, faces, n3, vb, 0, L.S.keys[0], L.S.vals[0]);
    if ((rc = sort_pairs(L.S, n3, 2 * vb, stream, &cur))) return rc;
    hipLaunchKernelGGL(k_edge_runs, mesh_launch_grid(n3), block, 0, stream, L.S.keys[cur], L.S.vals[cur], n3, counts);
    // vertex fans
    hipLaunchKernelGGL(k_link_keys, mesh_launch_grid(n3), block, 0, stream, faces, n3, vb, L.S.keys[0], L.S.vals[0], L.parent);
    if ((rc = sort_pairs(L.S, 2 * n3, 2 * vb, stream, &cur))) return rc;
    hipLaunchKernelGGL(k_link_union, mesh_launch_grid(2 * n3), block, 0, stream, L.S.keys[cur], L.S.vals[cur], 2 * n3, L.parent);
    (void)hipMemsetAsync(L.roots, 0, sizeof(int32_t) * (n_vertices > 0 ? n_vertices : 1), stream);
    hipLaunchKernelGGL(k_fan_roots, mesh_launch_grid(n3), block, 0, stream, faces, L.parent, n3, L.roots);
    hipLaunchKernelGGL(k_fan_count, mesh_launch_grid(n_vertices), block, 0, stream, L.roots, n_vertices, counts);
    return dgnn_check_launch("mesh_topology");
}
