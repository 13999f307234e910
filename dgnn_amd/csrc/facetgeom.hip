// The facet geometry columns of `<scene>_fgeom.npz` from the arrays of `<scene>_3dt.npz` (include/dgnn_hip.h: dgnn_cell_circumspheres,
// dgnn_facet_geometry): per directed facet row 4 t + k (the facet of tet t opposite its vertex k) the facet's area, the cosine
// of the angle between the facet and the circumsphere of the cell on its own side, the same for the cell across, and the beta-skeleton term
// 1 - min of the two.  The arithmetic is §23's (facet_geom.h, shared with cutterms.hip), in two passes instead of that file's recompute:
//
//   k_cell_spheres     one thread per tet: (o.x, o.y, o.z, R), one 32-byte record per cell
//   k_facet_geometry   one thread per facet: the plane once, per side the cell's row of `tetrahedra` (slot, opposite vertex, validation) and
//                      its sphere record; the four values go to the row of either side that has a cell.  The infinite side's cosine is 1.
// Every row has one writer (a facet of a cell is named once by a well-formed `_3dt`), the output is zero-filled first, the counters are
// integer atomics per wave: reruns are bit-identical.  All fp64, no contraction (the build's -ffp-contract=off).
#include "common.h"
#include "mesh_common.h"
#include "facet_geom.h"
#include "tet_common.h"

namespace {

using dgnn_exact::FacetPlane;
using dgnn_exact::V3;
using dgnn_exact::load_v3;

constexpr int32_t FG_BAD_ID = 1, FG_MALFORMED = 2;

struct FgState {
    int32_t err, pad[3];
    unsigned long long rows, hull, neutral, flat;
};

struct alignas(32) SphereRec { double ox, oy, oz, R; };

__global__ void __launch_bounds__(MESH_THREADS) k_cell_spheres(const double* __restrict__ v, int64_t nv, const int32_t* __restrict__ tets, int64_t nt,
                                                             SphereRec* __restrict__ out, FgState* st) {
    int32_t flat = 0;
    for (int64_t t0 = blockIdx.x * (int64_t)blockDim.x; t0 < nt; t0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = t0 + threadIdx.x;
        if (t >= nt) continue;
        const int32_t i0 = tets[4 * t], i1 = tets[4 * t + 1], i2 = tets[4 * t + 2], i3 = tets[4 * t + 3];
        if (!tet_ids_ok(i0, i1, i2, i3, nv)) {
            atomicOr(&st->err, FG_BAD_ID);
            out[t] = SphereRec{0.0, 0.0, 0.0, 0.0};
            continue;
        }
        const dgnn_exact::Sphere s = dgnn_exact::cell_sphere(load_v3(v, i0), load_v3(v, i1), load_v3(v, i2), load_v3(v, i3));
        flat += s.det == 0;
        out[t] = SphereRec{s.o.x, s.o.y, s.o.z, s.R};
    }
    flat = wave_sum(flat);
    if (lane_id() == 0 && flat) atomicAdd(&st->flat, (unsigned long long)flat);
}

// out: four columns of n4 = 4 nc rows each (area, cos_own, cos_neighbor, beta), zero-filled by the caller
__global__ void __launch_bounds__(MESH_THREADS) k_facet_geometry(const double* __restrict__ v, int64_t nv, const int32_t* __restrict__ tets, int64_t nc,
                                                               const int32_t* __restrict__ facets, const int32_t* __restrict__ nfacets, int64_t nf,
                                                               const SphereRec* __restrict__ spheres, double* __restrict__ out, FgState* st) {
    const int64_t n4 = 4 * nc;
    int32_t rows = 0, hull = 0, neutral = 0;
    for (int64_t f0 = blockIdx.x * (int64_t)blockDim.x; f0 < nf; f0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = f0 + threadIdx.x;
        if (f >= nf) continue;
        const int32_t cell[2] = {nfacets[2 * f], nfacets[2 * f + 1]};
        const int32_t ia = facets[3 * f], ib = facets[3 * f + 1], ic = facets[3 * f + 2];
        if (cell[0] >= nc || cell[1] >= nc || ia < 0 || ia >= nv || ib < 0 || ib >= nv || ic < 0 || ic >= nv) {
            atomicOr(&st->err, FG_BAD_ID);
            continue;
        }
        if (cell[0] < 0 && cell[1] < 0) continue;
        const FacetPlane p = dgnn_exact::facet_plane(load_v3(v, ia), load_v3(v, ib), load_v3(v, ic));
        double cosine[2] = {1.0, 1.0};          // the infinite cell: its sphere is the half-space beyond the facet, h / R -> 1
        int slot[2] = {0, 0}, side_neutral = 0;
        bool ok = true;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (cell[s] < 0 || !ok) continue;
            int32_t t[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) t[k] = tets[4 * (int64_t)cell[s] + k];
            if (!tet_ids_ok(t, nv)) {
                atomicOr(&st->err, FG_BAD_ID);
                ok = false;
                continue;
            }
            slot[s] = facet_opposite_slot(t, ia, ib, ic);
            if (slot[s] < 0) {
                atomicOr(&st->err, FG_MALFORMED);
                ok = false;
                continue;
            }
            const SphereRec r = spheres[cell[s]];
            cosine[s] = dgnn_exact::sphere_cosine(V3{r.ox, r.oy, r.oz}, r.R, p, load_v3(v, row_at(t, slot[s])), &side_neutral);
        }
        if (!ok) continue;
        neutral += side_neutral;
        const double area = 0.5 * p.nn, beta = 1.0 - (cosine[0] < cosine[1] ? cosine[0] : cosine[1]);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (cell[s] < 0) continue;
            const int64_t row = 4 * (int64_t)cell[s] + slot[s];
            out[row] = area;
            out[n4 + row] = cosine[s];
            out[2 * n4 + row] = cosine[1 - s];
            out[3 * n4 + row] = beta;
            ++rows;
            hull += cell[1 - s] < 0;
        }
    }
    rows = wave_sum(rows);
    hull = wave_sum(hull);
    neutral = wave_sum(neutral);
    if (lane_id() != 0) return;
    if (rows) atomicAdd(&st->rows, (unsigned long long)rows);
    if (hull) atomicAdd(&st->hull, (unsigned long long)hull);
    if (neutral) atomicAdd(&st->neutral, (unsigned long long)neutral);
}

__global__ void k_geometry_stats(const FgState* st, int64_t* stats_out) {
    if (threadIdx.x == 0) {
        stats_out[0] = (int64_t)st->rows;
        stats_out[1] = (int64_t)st->hull;
        stats_out[2] = (int64_t)st->neutral;
        stats_out[3] = (int64_t)st->flat;
    }
}

bool fg_sizes_ok(int64_t nc, int64_t nv, int64_t nf) { return nc < INT32_MAX / 4 && nv < INT32_MAX && nf < INT32_MAX / 3; }

int fg_read_status(FgState* hs, const FgState* st, hipStream_t stream, const char* what) {
    int rc = dgnn_check_launch(what);
    if (rc || (rc = mm_read(hs, st, sizeof(FgState), stream, what))) return rc;
    if (!hs->err) return DGNN_OK;
    dgnn_set_error("%s: %s%s", what, hs->err & FG_BAD_ID ? "an id out of range; " : "",
                   hs->err & FG_MALFORMED ? "a facet is not a face of the cell its nfacets row names; " : "");
    return DGNN_E_INVALID;
}

struct FgLayout { FgState* st; SphereRec* spheres; int64_t bytes; };
FgLayout fg_layout(void* base, int64_t nc) {
    Take t{(char*)base, 256};
    FgLayout L{};
    L.st = (FgState*)base;
    L.spheres = t.take<SphereRec>(nc);
    L.bytes = t.off;
    return L;
}

}  // namespace

extern "C" int64_t dgnn_cell_circumspheres_scratch_bytes(void) { return 256; }

extern "C" int dgnn_cell_circumspheres(const double* vertices, int64_t n_vertices, const int32_t* tets, int64_t n_cells, double* centre_radius_out,
                                       int64_t* stats_out, void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(n_vertices >= 0 && n_cells >= 0 && scratch && (n_cells == 0 || (tets && centre_radius_out)) && (n_vertices == 0 || vertices) &&
                     (uintptr_t)centre_radius_out % sizeof(SphereRec) == 0,
                 DGNN_E_INVALID, "cell_circumspheres: bad args (centre_radius_out is 32-byte aligned)");
    DGNN_REQUIRE(fg_sizes_ok(n_cells, n_vertices, 0), DGNN_E_UNSUPPORTED, "cell_circumspheres: sizes exceed the int32 indexing");
    FgState* st = (FgState*)scratch;
    (void)hipMemsetAsync(st, 0, sizeof(FgState), stream);
    if (n_cells > 0)
        hipLaunchKernelGGL(k_cell_spheres, mesh_launch_grid(n_cells), dim3(MESH_THREADS), 0, stream, vertices, n_vertices, tets, n_cells,
                           (SphereRec*)centre_radius_out, st);
    if (stats_out) hipLaunchKernelGGL(k_geometry_stats, dim3(1), dim3(64), 0, stream, st, stats_out);
    FgState hs{};
    return fg_read_status(&hs, st, stream, "cell_circumspheres");
}

extern "C" int64_t dgnn_facet_geometry_scratch_bytes(int64_t n_cells) {
    if (n_cells < 0) return 0;
    return fg_layout(nullptr, n_cells).bytes;
}

extern "C" int dgnn_facet_geometry(const double* vertices, int64_t n_vertices, const int32_t* tets, int64_t n_cells, const int32_t* facets,
                                   const int32_t* nfacets, int64_t n_facets, const double* spheres, double* out, int64_t* stats_out, void* scratch,
                                   void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(n_vertices >= 0 && n_cells >= 0 && n_facets >= 0 && scratch && (n_facets == 0 || (facets && nfacets)) && (n_vertices == 0 || vertices) &&
                     (n_cells == 0 || (tets && out)) && (uintptr_t)spheres % sizeof(SphereRec) == 0,
                 DGNN_E_INVALID, "facet_geometry: bad args (spheres is 32-byte aligned)");
    DGNN_REQUIRE(fg_sizes_ok(n_cells, n_vertices, n_facets), DGNN_E_UNSUPPORTED, "facet_geometry: sizes exceed the int32 indexing");
    const FgLayout L = fg_layout(scratch, n_cells);
    (void)hipMemsetAsync(L.st, 0, sizeof(FgState), stream);
    if (n_cells > 0) (void)hipMemsetAsync(out, 0, sizeof(double) * 16 * n_cells, stream);
    if (n_cells > 0 && !spheres)
        hipLaunchKernelGGL(k_cell_spheres, mesh_launch_grid(n_cells), dim3(MESH_THREADS), 0, stream, vertices, n_vertices, tets, n_cells, L.spheres, L.st);
    if (n_facets > 0)
        hipLaunchKernelGGL(k_facet_geometry, mesh_launch_grid(n_facets), dim3(MESH_THREADS), 0, stream, vertices, n_vertices, tets, n_cells, facets, nfacets,
                           n_facets, spheres ? (const SphereRec*)spheres : L.spheres, out, L.st);
    if (stats_out) hipLaunchKernelGGL(k_geometry_stats, dim3(1), dim3(64), 0, stream, L.st, stats_out);
    FgState hs{};
    return fg_read_status(&hs, L.st, stream, "facet_geometry");
}
