// Point-in-mesh occupancy of an arbitrary triangle mesh (reference utils/libmesh: inside_mesh.py MeshIntersector.query with
// triangle_hash.pyx as its candidate generator) and the three small generators of the evaluation-sample builder.  DESIGN §21.
//
//   rescale    vertices and points go to the hash frame in fp64: r(a) = scale * a + translate, two roundings, with scale = (R - 1) /
//              (max - min) and translate = 0.5 - scale * min over the vertices the faces reference (host fp64, the same two expressions).
//   candidates a uniform xy grid of ((R - 1) >> shift) + 1 cells per axis on int(coord) >> shift: a triangle is entered in every cell its
//              xy bounding box touches (cells clamped to [0, R - 1] before the shift), a point reads the list of its own cell.  A point
//              that passes the strict barycentric test of a triangle lies inside that triangle's box, so any shift offers a superset of
//              the triangles that count and the answer is the all-pairs answer; shift = the smallest with at most max_entries entries.
//              Built by the entry-grid builder of mesh_grid.h: one work item per (triangle, cell) entry.
//   query      one lane per point (DESIGN §21 says why), every loop bounded by a list length; per candidate the reference's 2D test and
//              depth, operand for operand; the two parities are integer counts, so the order inside a cell does not matter.
//   generators box points, Gaussian jitter (Box-Muller) and face normals, all fp64, randomness from mm_hash (mesh_common.h).
//   labels     the share of each tet of a triangulation inside the mesh (the training target): k counter-hash samples per tet,
//              made in registers and put through the query's own per-point function; a wavefront owns whole tets and counts with
//              popcount(ballot): integer counts, no atomics.  The sampler alone is the second entry point.
#include <math.h>

#include "common.h"
#include "mesh_grid.h"

namespace {

constexpr int MC_MAX_R = 4096;     // hash_resolution; (MC_MAX_R - 1) >> (MC_SHIFTS - 1) == 0: the coarsest grid is one cell
constexpr int MC_SHIFTS = 13;
constexpr int32_t MC_BAD_ID = 1, MC_NONFINITE = 2, MC_BAD_TET = 4;

struct McState {
    int32_t err, pad;
    unsigned long long lo[3], hi[3];          // bbox of the referenced vertices (f64_key)
    unsigned long long totals[MC_SHIFTS];     // (triangle, cell) entries at every shift
    unsigned long long n_disagree;
};

struct Frame {          // by value to the kernels
    double scale[3], translate[3];
    int32_t R, shift, G;   // G cells per axis at `shift`
};

// the bounding box (k_bbox_referenced) leaves out a coordinate that is not finite
struct McRefuse {
    __device__ int32_t operator()(double x) const { return isfinite(x) ? 0 : MC_NONFINITE; }
};

// rv = scale * v + translate (a multiply, then an add: the library is built without contraction)
__global__ void k_mc_rescale(const double* __restrict__ v, int64_t nv, Frame f, double* __restrict__ rv) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < 3 * nv; i += (int64_t)gridDim.x * blockDim.x) {
        const int a = (int)(i % 3);
        const double m = f.scale[a] * v[i];
        rv[i] = m + f.translate[a];
    }
}

// the reference's int(coord) clamped to [0, R - 1]; clamping first keeps the cast defined for any value
__device__ __forceinline__ int32_t mc_cell(double x, int32_t R) { return !(x > 0) ? 0 : (x >= (double)(R - 1) ? R - 1 : (int32_t)x); }

// tbox[t] = (x0, y0, x1, y1): the cells at full resolution of the triangle's xy bounding box; entries at every shift -> totals
__global__ void __launch_bounds__(MESH_THREADS) k_mc_tri_box(const double* __restrict__ rv, const int32_t* __restrict__ faces, int64_t nf, int32_t R,
                                                           int4* __restrict__ tbox, McState* st) {
    long long tot[MC_SHIFTS];
#pragma unroll
    for (int s = 0; s < MC_SHIFTS; ++s) tot[s] = 0;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < nf; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t a = faces[3 * t], b = faces[3 * t + 1], c = faces[3 * t + 2];
        const double ax = rv[3 * a], ay = rv[3 * a + 1], bx = rv[3 * b], by = rv[3 * b + 1], cx = rv[3 * c], cy = rv[3 * c + 1];
        const int32_t x0 = mc_cell(fmin(fmin(ax, bx), cx), R), x1 = mc_cell(fmax(fmax(ax, bx), cx), R);
        const int32_t y0 = mc_cell(fmin(fmin(ay, by), cy), R), y1 = mc_cell(fmax(fmax(ay, by), cy), R);
        tbox[t] = make_int4(x0, y0, x1, y1);
#pragma unroll
        for (int s = 0; s < MC_SHIFTS; ++s) tot[s] += (long long)((x1 >> s) - (x0 >> s) + 1) * ((y1 >> s) - (y0 >> s) + 1);
    }
#pragma unroll
    for (int s = 0; s < MC_SHIFTS; ++s) wave_add_atomic(tot[s], &st->totals[s]);
}

// ---- the grid (mesh_grid.h): the cells of a triangle's box at `shift`, row-major ------------------------------------------------------
struct McCells {
    const int4* tbox;
    int32_t shift, G;
    __device__ int32_t count(int64_t t) const {
        const int4 b = tbox[t];
        return ((b.z >> shift) - (b.x >> shift) + 1) * ((b.w >> shift) - (b.y >> shift) + 1);
    }
    __device__ int32_t cell(int64_t t, int32_t k) const {
        const int4 b = tbox[t];
        const int32_t y0 = b.y >> shift, ny = (b.w >> shift) - y0 + 1;
        return G * ((b.x >> shift) + k / ny) + y0 + k % ny;
    }
};

__global__ void k_mc_tri_count(McCells cells, int64_t nf, int32_t* __restrict__ tcnt) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < nf; t += (int64_t)gridDim.x * blockDim.x) tcnt[t] = cells.count(t);
}

// ---- the query -----------------------------------------------------------------------------------------------------------------
// The per-point work, stated once for k_mc_query and k_cl_count: the rescale to the hash frame, the cell lookup and the candidate loop.
// -> bit 0 = (above odd), bit 1 = (below odd); 3 = contained, 1 or 2 = the two parities disagree.
__device__ __forceinline__ uint32_t mc_point_parities(const double* __restrict__ rv, const int32_t* __restrict__ faces, const int32_t* __restrict__ rowptr,
                                                      const int32_t* __restrict__ entries, const Frame& f, double px, double py, double pz) {
    const double Rd = (double)f.R;
    const double in[3] = {px, py, pz};
    double p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double m = f.scale[a] * in[a];
        p[a] = m + f.translate[a];
    }
    uint32_t above = 0, below = 0;
    // the box test is false for NaN; x, y < R as the hash's own test (a coordinate equal to R is in no cell)
    if (0 <= p[0] && p[0] < Rd && 0 <= p[1] && p[1] < Rd && 0 <= p[2] && p[2] <= Rd) {
        const int32_t cell = f.G * ((int32_t)p[0] >> f.shift) + ((int32_t)p[1] >> f.shift);
        for (int32_t s = rowptr[cell], e = rowptr[cell + 1]; s < e; ++s) {
            const int64_t t = entries[s];
            const double* t1 = rv + 3 * (int64_t)faces[3 * t];
            const double* t2 = rv + 3 * (int64_t)faces[3 * t + 1];
            const double* t3 = rv + 3 * (int64_t)faces[3 * t + 2];
            const double t1x = t1[0], t1y = t1[1], t1z = t1[2], t2x = t2[0], t2y = t2[1], t2z = t2[2], t3x = t3[0], t3y = t3[1], t3z = t3[2];
            // check_triangles: A = [t1 - t3, t2 - t3] as columns, y = p - t3
            const double a00 = t1x - t3x, a01 = t2x - t3x, a10 = t1y - t3y, a11 = t2y - t3y;
            const double y0 = p[0] - t3x, y1 = p[1] - t3y;
            const double det = a00 * a11 - a01 * a10;
            if (!(fabs(det) != 0.)) continue;
            const double sd = det > 0 ? 1.0 : (det < 0 ? -1.0 : det), ad = fabs(det);   // np.sign (nan stays nan)
            const double u = (a11 * y0 - a01 * y1) * sd;
            const double v = (-a10 * y0 + a00 * y1) * sd;
            const double uv = u + v;
            if (!(0 < u && u < ad && 0 < v && v < ad && 0 < uv && uv < ad)) continue;
            // compute_intersection_depth: normals = cross(t3 - t1, t2 - t1)
            const double v1x = t3x - t1x, v1y = t3y - t1y, v1z = t3z - t1z, v2x = t2x - t1x, v2y = t2y - t1y, v2z = t2z - t1z;
            const double n0 = v1y * v2z - v1z * v2y, n1 = v1z * v2x - v1x * v2z, n2 = v1x * v2y - v1y * v2x;
            const double alpha = n0 * (t1x - p[0]) + n1 * (t1y - p[1]);
            const double an = fabs(n2);
            if (!(an != 0)) continue;                                 // depth = nan: neither above nor below
            const double sn = n2 > 0 ? 1.0 : (n2 < 0 ? -1.0 : n2);
            const double depth = t1z * an + alpha * sn, rhs = p[2] * an;
            above += depth >= rhs;
            below += depth < rhs;
        }
    }
    return (above & 1) | ((below & 1) << 1);
}

__global__ void __launch_bounds__(MESH_THREADS) k_mc_query(const double* __restrict__ rv, const int32_t* __restrict__ faces,
                                                         const int32_t* __restrict__ rowptr, const int32_t* __restrict__ entries, Frame f,
                                                         const double* __restrict__ pts, int64_t np, uint8_t* __restrict__ out, McState* st) {
    long long dis = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < np; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t par = mc_point_parities(rv, faces, rowptr, entries, f, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
        const uint32_t c1 = par & 1, c2 = par >> 1;
        out[i] = (uint8_t)(c1 & c2);
        dis += c1 != c2;
    }
    wave_add_atomic(dis, &st->n_disagree);
}

__global__ void k_mc_disagree_out(const McState* st, int64_t* out) {
    if (threadIdx.x == 0) *out = (int64_t)st->n_disagree;
}

// ---- generators ------------------------------------------------------------------------------------------------------------------
__global__ void k_box_points(int64_t n3, double boxsize, uint64_t seed, double* __restrict__ out) {
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n3; j += (int64_t)gridDim.x * blockDim.x)
        out[j] = boxsize * (mm_u01(mm_hash(seed, (uint64_t)j + 1)) - 0.5);
}

// out[j] = pts[j] + sigma * (sqrt(-2 log u1) cos(2 pi u2)), u1 in (0, 1] from counter 2 j + 1, u2 in [0, 1) from 2 j + 2
__global__ void k_jitter_points(const double* __restrict__ pts, int64_t n3, double sigma, uint64_t seed, double* __restrict__ out) {
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n3; j += (int64_t)gridDim.x * blockDim.x) {
        const double u1 = mm_u01_open0(mm_hash(seed, 2 * (uint64_t)j + 1)), u2 = mm_u01(mm_hash(seed, 2 * (uint64_t)j + 2));
        const double z = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
        out[j] = pts[j] + sigma * z;
    }
}

__global__ void k_face_normals(const double* __restrict__ v, int64_t nv, const int32_t* __restrict__ faces, int64_t nf, double* __restrict__ out,
                               McState* st) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < nf; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t a = faces[3 * t], b = faces[3 * t + 1], c = faces[3 * t + 2];
        double nx = 0, ny = 0, nz = 0;
        if (a < 0 || a >= nv || b < 0 || b >= nv || c < 0 || c >= nv) {
            atomicOr(&st->err, MC_BAD_ID);
        } else {
            const double ux = v[3 * b] - v[3 * a], uy = v[3 * b + 1] - v[3 * a + 1], uz = v[3 * b + 2] - v[3 * a + 2];
            const double wx = v[3 * c] - v[3 * a], wy = v[3 * c + 1] - v[3 * a + 1], wz = v[3 * c + 2] - v[3 * a + 2];
            const double cx = uy * wz - uz * wy, cy = uz * wx - ux * wz, cz = ux * wy - uy * wx;
            const double len = sqrt(cx * cx + cy * cy + cz * cz);
            if (len > 0 && isfinite(len)) { nx = cx / len; ny = cy / len; nz = cz / len; }   // a degenerate face: zeros
        }
        out[3 * t] = nx; out[3 * t + 1] = ny; out[3 * t + 2] = nz;
    }
}

// ---- cell labels: the share of each tet inside the mesh, by sampling -----------------------------------------------------
// sample j of tet t (ids validated): three draws from the counters c, c + 1, c + 2 with c = 3 ((tet_offset + t) k + j) + 1 (mod 2^64),
// folded from the unit cube onto the unit tet, then x = ((s e1 + t e2) + u e3) + p0 per coordinate; one rounding per operation
__device__ __forceinline__ void cl_sample(const double (&p)[4][3], uint64_t seed, uint64_t c, double* x) {
    double s = mm_u01(mm_hash(seed, c)), t = mm_u01(mm_hash(seed, c + 1)), u = mm_u01(mm_hash(seed, c + 2));
    if (s + t > 1) { s = 1 - s; t = 1 - t; }
    const double st = s + t;
    if (t + u > 1) {
        const double t0 = t;
        t = 1 - u;
        u = (1 - s) - t0;
    } else if (st + u > 1) {
        s = (1 - t) - u;
        u = (st + u) - 1;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double e1 = p[1][a] - p[0][a], e2 = p[2][a] - p[0][a], e3 = p[3][a] - p[0][a];
        x[a] = ((s * e1 + t * e2) + u * e3) + p[0][a];
    }
}

__device__ __forceinline__ void cl_load_tet(const double* __restrict__ v, const int32_t* __restrict__ tets, int64_t t, double (&p)[4][3]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int64_t id = tets[4 * t + c];
#pragma unroll
        for (int a = 0; a < 3; ++a) p[c][a] = v[3 * id + a];
    }
}

// the sampler alone: one lane per sample, points_out row t k + j
__global__ void __launch_bounds__(MESH_THREADS) k_tet_sample(const double* __restrict__ v, const int32_t* __restrict__ tets, int64_t nt, int64_t k,
                                                           uint64_t seed, uint64_t tet_offset, double* __restrict__ out) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nt * k; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = i / k, j = i - t * k;
        double p[4][3], x[3];
        cl_load_tet(v, tets, t, p);
        cl_sample(p, seed, 3 * ((tet_offset + (uint64_t)t) * (uint64_t)k + (uint64_t)j) + 1, x);
        out[3 * i] = x[0]; out[3 * i + 1] = x[1]; out[3 * i + 2] = x[2];
    }
}

// The fused path: a wavefront owns 64 >> LG whole tets, 1 << LG lanes each (LG = 6: one tet, its ids and vertices wave-uniform, so they
// come by scalar loads; LG < 6: k <= 1 << LG <= 32, tets packed so that a small k does not idle the lanes).  A lane strides over its
// tet's samples, makes each in registers and tests it; count[t] = popcount of the tet's bits of ballot(inside), summed over the rounds
// and stored by the tet's first lane.  Integer counts without atomics: the same bits on every run.  Every loop has a wave-uniform trip
// count, so all 64 lanes reach each ballot.
template <int LG>
__global__ void __launch_bounds__(MESH_THREADS) k_cl_count(const double* __restrict__ rv, const int32_t* __restrict__ faces,
                                                         const int32_t* __restrict__ rowptr, const int32_t* __restrict__ entries, Frame f,
                                                         const double* __restrict__ v, const int32_t* __restrict__ tets, int64_t nt, int64_t k,
                                                         uint64_t seed, uint64_t tet_offset, int32_t* __restrict__ count, McState* st) {
    constexpr int G = 1 << LG, PER = 64 >> LG;
    constexpr uint64_t MASK = LG == 6 ? ~0ull : (1ull << (G & 63)) - 1;
    const int lane = lane_id(), sub = lane >> LG, j0 = lane & (G - 1);
    const int64_t n_groups = (nt + PER - 1) / PER, n_waves = (int64_t)gridDim.x * (MESH_THREADS / 64);
    long long dis = 0;
    for (int64_t grp = (int64_t)blockIdx.x * (MESH_THREADS / 64) + wave_id_uniform(); grp < n_groups; grp += n_waves) {
        const int64_t t = grp * PER + sub;
        const bool live = t < nt;
        double p[4][3];
        cl_load_tet(v, tets, live ? t : nt - 1, p);
        const uint64_t c0 = (tet_offset + (uint64_t)t) * (uint64_t)k;
        int32_t cnt = 0;
        for (int64_t base = 0; base < k; base += G) {
            const int64_t j = base + j0;
            uint32_t par = 0;
            if (live && j < k) {
                double x[3];
                cl_sample(p, seed, 3 * (c0 + (uint64_t)j) + 1, x);
                par = mc_point_parities(rv, faces, rowptr, entries, f, x[0], x[1], x[2]);
            }
            dis += par == 1 || par == 2;
            const uint64_t inside = __ballot(par == 3);
            cnt += __popcll((inside >> (sub * G)) & MASK);
        }
        if (live && j0 == 0) count[t] = cnt;
    }
    wave_add_atomic(dis, &st->n_disagree);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
struct McLayout { McState* st; double* rv; int4* tbox; GridBufs g; int64_t bytes; };
McLayout mc_layout(void* base, int64_t nv, int64_t nf, int64_t R) {
    Take t{(char*)base, 256};
    McLayout L{};
    L.st = (McState*)base;
    L.rv = t.take<double>(3 * nv);
    L.tbox = t.take<int4>(nf);
    L.g = take_grid(t, nf, R * R);
    L.bytes = t.off;
    return L;
}

int mc_status(const McState& hs, const char* what) {
    if (!hs.err) return DGNN_OK;
    dgnn_set_error("%s: %s%s%s", what, hs.err & MC_BAD_ID ? "a face's vertex id out of range; " : "",
                   hs.err & MC_NONFINITE ? "a non-finite coordinate of a referenced vertex; " : "",
                   hs.err & MC_BAD_TET ? "a tetrahedron's vertex id out of range; " : "");
    return DGNN_E_INVALID;
}

// validation, bounding box, rescaled vertices, per-triangle boxes and the choice of the shift.  On success rv / tbox of L are filled, *fr is
// the frame and *n_entries the entries at fr->shift.  Synchronises three times.
int mc_plan(const double* vertices, int64_t nv, const int32_t* faces, int64_t nf, int32_t R, int64_t max_entries, const McLayout& L, Frame* fr,
            int64_t* n_entries, hipStream_t stream, const char* what) {
    DGNN_REQUIRE(nv >= 0 && nf >= 0 && (nv == 0 || vertices) && (nf == 0 || faces) && L.st, DGNN_E_INVALID, "%s: bad args", what);
    DGNN_REQUIRE(nf > 0, DGNN_E_INVALID, "%s: a mesh without faces", what);
    DGNN_REQUIRE(R >= 2, DGNN_E_INVALID, "%s: hash_resolution %d < 2", what, R);
    DGNN_REQUIRE(R <= MC_MAX_R, DGNN_E_UNSUPPORTED, "%s: hash_resolution %d above %d", what, R, MC_MAX_R);
    DGNN_REQUIRE(max_entries >= 1, DGNN_E_INVALID, "%s: max_entries < 1", what);
    DGNN_REQUIRE(nf < INT32_MAX / 4 && nv < INT32_MAX, DGNN_E_UNSUPPORTED, "%s: sizes exceed the int32 indexing", what);
    const dim3 block(MESH_THREADS);
    McState hs{};
    hs.lo[0] = hs.lo[1] = hs.lo[2] = ~0ull;
    (void)hipMemcpyAsync(L.st, &hs, sizeof(McState), hipMemcpyHostToDevice, stream);
    hipLaunchKernelGGL(k_check_ids, mesh_launch_grid(3 * nf), block, 0, stream, faces, 3 * nf, nv, &L.st->err, MC_BAD_ID);
    int rc = dgnn_check_launch(what);
    if (rc || (rc = mm_read(&hs, L.st, sizeof(McState), stream, what)) || (rc = mc_status(hs, what))) return rc;   // ids are read below: checked first
    hipLaunchKernelGGL(k_bbox_referenced<McRefuse>, mesh_launch_grid(3 * nf), block, 0, stream, vertices, faces, 3 * nf, McRefuse{}, &L.st->err, L.st->lo,
                       L.st->hi);
    if ((rc = dgnn_check_launch(what)) || (rc = mm_read(&hs, L.st, sizeof(McState), stream, what)) || (rc = mc_status(hs, what))) return rc;
    Frame f{};
    f.R = R;
    double lo[3], hi[3];
    bbox_unkey(hs.lo, hs.hi, lo, hi);
    for (int a = 0; a < 3; ++a) {
        const double ext = hi[a] - lo[a];
        DGNN_REQUIRE(ext > 0, DGNN_E_INVALID, "%s: the mesh has no extent on axis %d", what, a);
        f.scale[a] = (double)(R - 1) / ext;
        const double m = f.scale[a] * lo[a];
        f.translate[a] = 0.5 - m;
        DGNN_REQUIRE(isfinite(f.scale[a]) && isfinite(f.translate[a]), DGNN_E_INVALID, "%s: the extent %g of axis %d does not rescale", what, ext, a);
    }
    hipLaunchKernelGGL(k_mc_rescale, mesh_launch_grid(3 * nv), block, 0, stream, vertices, nv, f, L.rv);
    hipLaunchKernelGGL(k_mc_tri_box, mesh_launch_grid(nf), block, 0, stream, L.rv, faces, nf, R, L.tbox, L.st);
    if ((rc = dgnn_check_launch(what)) || (rc = mm_read(&hs, L.st, sizeof(McState), stream, what))) return rc;
    int s = 0;
    while (s < MC_SHIFTS && hs.totals[s] > (unsigned long long)max_entries) ++s;
    DGNN_REQUIRE(s < MC_SHIFTS, DGNN_E_UNSUPPORTED, "%s: max_entries %lld is below the number of faces %lld", what, (long long)max_entries, (long long)nf);
    DGNN_REQUIRE(hs.totals[s] < (unsigned long long)INT32_MAX, DGNN_E_UNSUPPORTED, "%s: %llu hash entries exceed the int32 indexing", what, hs.totals[s]);
    f.shift = s;
    f.G = ((R - 1) >> s) + 1;
    *fr = f;
    *n_entries = (int64_t)hs.totals[s];
    return DGNN_OK;
}

// the candidate grid of the planned frame into L.g.rowptr and `entries` (ne of them): the counts at the chosen shift (only the plan's
// totals over all shifts told which), then the shared builder
int mc_build_grid(const McLayout& L, const Frame& f, int64_t n_faces, int64_t ne, int32_t* entries, hipStream_t stream) {
    const McCells cells{L.tbox, f.shift, f.G};
    hipLaunchKernelGGL(k_mc_tri_count, mesh_launch_grid(n_faces), dim3(MESH_THREADS), 0, stream, cells, n_faces, L.g.tcnt);
    return build_entry_grid(L.g, cells, n_faces, (int64_t)f.G * f.G, ne, entries, stream);
}

// ids of the tets in [0, nv), checked on the device before any kernel reads through them.  `st` is zero in err on entry.  Synchronises once.
int cl_check_tets(const int32_t* tets, int64_t nt, int64_t nv, McState* st, hipStream_t stream, const char* what) {
    McState hs{};
    hipLaunchKernelGGL(k_check_ids, mesh_launch_grid(4 * nt), dim3(MESH_THREADS), 0, stream, tets, 4 * nt, nv, &st->err, MC_BAD_TET);
    int rc = dgnn_check_launch(what);
    if (rc || (rc = mm_read(&hs, st, sizeof(McState), stream, what))) return rc;
    return mc_status(hs, what);
}

template <int LG>
void cl_launch(const McLayout& L, const Frame& f, const int32_t* faces, const int32_t* entries, const double* v, const int32_t* tets, int64_t nt, int64_t k,
               uint64_t seed, uint64_t tet_offset, int32_t* count, hipStream_t stream) {
    const int64_t waves = dgnn_cdiv(nt, 64 >> LG);
    hipLaunchKernelGGL(k_cl_count<LG>, dim3(dgnn_grid_cap(dgnn_cdiv(waves, MESH_THREADS / 64))), dim3(MESH_THREADS), 0, stream, L.rv, faces, L.g.rowptr, entries, f, v,
                       tets, nt, k, seed, tet_offset, count, L.st);
}

}  // namespace

// ================================================================================================================================
extern "C" int64_t dgnn_mesh_contains_scratch_bytes(int64_t n_vertices, int64_t n_faces, int32_t hash_resolution) {
    if (n_vertices < 0 || n_faces < 0 || hash_resolution < 2 || hash_resolution > MC_MAX_R) return 256;
    return mc_layout(nullptr, n_vertices, n_faces, hash_resolution).bytes;
}

extern "C" int dgnn_mesh_contains_plan(const double* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int32_t hash_resolution,
                                       int64_t max_entries, int32_t* shift_out, int64_t* n_entries_out, void* scratch, void* stream_) {
    DGNN_REQUIRE(scratch && shift_out && n_entries_out, DGNN_E_INVALID, "mesh_contains_plan: bad args");
    Frame f{};
    const McLayout L = mc_layout(scratch, n_vertices > 0 ? n_vertices : 0, n_faces > 0 ? n_faces : 0,
                                 hash_resolution >= 2 && hash_resolution <= MC_MAX_R ? hash_resolution : 2);
    const int rc = mc_plan(vertices, n_vertices, faces, n_faces, hash_resolution, max_entries, L, &f, n_entries_out, (hipStream_t)stream_, "mesh_contains_plan");
    if (rc) return rc;
    *shift_out = f.shift;
    return DGNN_OK;
}

extern "C" int dgnn_mesh_contains(const double* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int32_t hash_resolution,
                                  int64_t max_entries, const double* points, int64_t n_points, uint8_t* contains_out, int64_t* n_disagree_out,
                                  int32_t* entries, int64_t entry_capacity, void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(scratch && n_points >= 0 && entry_capacity >= 0 && (n_points == 0 || (points && contains_out)), DGNN_E_INVALID, "mesh_contains: bad args");
    DGNN_REQUIRE(n_points < INT32_MAX, DGNN_E_UNSUPPORTED, "mesh_contains: sizes exceed the int32 indexing");
    Frame f{};
    int64_t ne = 0;
    const McLayout L = mc_layout(scratch, n_vertices > 0 ? n_vertices : 0, n_faces > 0 ? n_faces : 0,
                                 hash_resolution >= 2 && hash_resolution <= MC_MAX_R ? hash_resolution : 2);
    int rc = mc_plan(vertices, n_vertices, faces, n_faces, hash_resolution, max_entries, L, &f, &ne, stream, "mesh_contains");
    if (rc) return rc;
    DGNN_REQUIRE(entries && ne <= entry_capacity, DGNN_E_INVALID, "mesh_contains: %lld hash entries, room for %lld (dgnn_mesh_contains_plan gives the number)",
                 (long long)ne, (long long)entry_capacity);
    if (n_disagree_out) (void)hipMemsetAsync(n_disagree_out, 0, sizeof(int64_t), stream);
    if (n_points == 0) return dgnn_check_launch("mesh_contains");
    if ((rc = mc_build_grid(L, f, n_faces, ne, entries, stream))) return rc;
    hipLaunchKernelGGL(k_mc_query, mesh_launch_grid(n_points), dim3(MESH_THREADS), 0, stream, L.rv, faces, L.g.rowptr, entries, f, points, n_points, contains_out, L.st);
    if (n_disagree_out) hipLaunchKernelGGL(k_mc_disagree_out, dim3(1), dim3(64), 0, stream, L.st, n_disagree_out);
    return dgnn_check_launch("mesh_contains");
}

extern "C" int dgnn_box_points(int64_t n_points, double boxsize, uint64_t seed, double* points_out, void* stream_) {
    DGNN_REQUIRE(n_points >= 0 && (n_points == 0 || points_out), DGNN_E_INVALID, "box_points: bad args");
    if (n_points > 0) hipLaunchKernelGGL(k_box_points, mesh_launch_grid(3 * n_points), dim3(MESH_THREADS), 0, (hipStream_t)stream_, 3 * n_points, boxsize, seed, points_out);
    return dgnn_check_launch("box_points");
}

extern "C" int dgnn_jitter_points(const double* points, int64_t n_points, double sigma, uint64_t seed, double* points_out, void* stream_) {
    DGNN_REQUIRE(n_points >= 0 && (n_points == 0 || (points && points_out)), DGNN_E_INVALID, "jitter_points: bad args");
    if (n_points > 0)
        hipLaunchKernelGGL(k_jitter_points, mesh_launch_grid(3 * n_points), dim3(MESH_THREADS), 0, (hipStream_t)stream_, points, 3 * n_points, sigma, seed, points_out);
    return dgnn_check_launch("jitter_points");
}

extern "C" int dgnn_face_normals(const double* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, double* normals_out, void* scratch,
                                 void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(n_vertices >= 0 && n_faces >= 0 && scratch && (n_faces == 0 || (faces && normals_out)) && (n_vertices == 0 || vertices), DGNN_E_INVALID,
                 "face_normals: bad args");
    McState* st = (McState*)scratch;
    McState hs{};
    (void)hipMemsetAsync(st, 0, sizeof(McState), stream);
    if (n_faces > 0) hipLaunchKernelGGL(k_face_normals, mesh_launch_grid(n_faces), dim3(MESH_THREADS), 0, stream, vertices, n_vertices, faces, n_faces, normals_out, st);
    int rc = dgnn_check_launch("face_normals");
    if (rc || (rc = mm_read(&hs, st, sizeof(McState), stream, "face_normals"))) return rc;
    return mc_status(hs, "face_normals");
}

extern "C" int64_t dgnn_cell_labels_scratch_bytes(int64_t n_mesh_vertices, int64_t n_faces, int32_t hash_resolution) {
    return dgnn_mesh_contains_scratch_bytes(n_mesh_vertices, n_faces, hash_resolution);
}

extern "C" int dgnn_cell_labels(const double* mesh_vertices, int64_t n_mesh_vertices, const int32_t* faces, int64_t n_faces, int32_t hash_resolution,
                                int64_t max_entries, int32_t* entries, int64_t entry_capacity, const double* vertices, int64_t n_vertices,
                                const int32_t* tetrahedra, int64_t n_tets, int64_t n_samples, uint64_t seed, uint64_t tet_offset, int32_t* count_out,
                                int64_t* n_disagree_out, void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(scratch && n_tets >= 0 && n_vertices >= 0 && entry_capacity >= 0 && (n_tets == 0 || (tetrahedra && count_out)) && (n_vertices == 0 || vertices),
                 DGNN_E_INVALID, "cell_labels: bad args");
    DGNN_REQUIRE(n_samples >= 1, DGNN_E_INVALID, "cell_labels: n_samples %lld < 1", (long long)n_samples);
    DGNN_REQUIRE(n_samples <= INT32_MAX, DGNN_E_UNSUPPORTED, "cell_labels: n_samples %lld above the int32 counts", (long long)n_samples);
    Frame f{};
    int64_t ne = 0;
    const McLayout L = mc_layout(scratch, n_mesh_vertices > 0 ? n_mesh_vertices : 0, n_faces > 0 ? n_faces : 0,
                                 hash_resolution >= 2 && hash_resolution <= MC_MAX_R ? hash_resolution : 2);
    int rc = mc_plan(mesh_vertices, n_mesh_vertices, faces, n_faces, hash_resolution, max_entries, L, &f, &ne, stream, "cell_labels");
    if (rc) return rc;
    DGNN_REQUIRE(entries && ne <= entry_capacity, DGNN_E_INVALID, "cell_labels: %lld hash entries, room for %lld (dgnn_mesh_contains_plan gives the number)",
                 (long long)ne, (long long)entry_capacity);
    if (n_disagree_out) (void)hipMemsetAsync(n_disagree_out, 0, sizeof(int64_t), stream);
    if (n_tets == 0) return dgnn_check_launch("cell_labels");
    if ((rc = cl_check_tets(tetrahedra, n_tets, n_vertices, L.st, stream, "cell_labels"))) return rc;   // ids are read below: checked first
    if ((rc = mc_build_grid(L, f, n_faces, ne, entries, stream))) return rc;
    int lg = 0;
    while (lg < 6 && (n_samples > 32 || ((int64_t)1 << lg) < n_samples)) ++lg;   // 1 << lg = pow2ceil(k) for k <= 32, else 64
#define CL_CASE(LG) case LG: cl_launch<LG>(L, f, faces, entries, vertices, tetrahedra, n_tets, n_samples, seed, tet_offset, count_out, stream); break
    switch (lg) { CL_CASE(0); CL_CASE(1); CL_CASE(2); CL_CASE(3); CL_CASE(4); CL_CASE(5); default: CL_CASE(6); }
#undef CL_CASE
    if (n_disagree_out) hipLaunchKernelGGL(k_mc_disagree_out, dim3(1), dim3(64), 0, stream, L.st, n_disagree_out);
    return dgnn_check_launch("cell_labels");
}

extern "C" int64_t dgnn_tet_sample_points_scratch_bytes(void) { return 256; }

extern "C" int dgnn_tet_sample_points(const double* vertices, int64_t n_vertices, const int32_t* tetrahedra, int64_t n_tets, int64_t n_samples, uint64_t seed,
                                      uint64_t tet_offset, double* points_out, void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(scratch && n_tets >= 0 && n_vertices >= 0 && (n_tets == 0 || (tetrahedra && points_out)) && (n_vertices == 0 || vertices), DGNN_E_INVALID,
                 "tet_sample_points: bad args");
    DGNN_REQUIRE(n_samples >= 1, DGNN_E_INVALID, "tet_sample_points: n_samples %lld < 1", (long long)n_samples);
    DGNN_REQUIRE(n_tets == 0 || n_samples <= INT64_MAX / 24 / n_tets, DGNN_E_UNSUPPORTED, "tet_sample_points: %lld x %lld points exceed the int64 indexing",
                 (long long)n_tets, (long long)n_samples);
    if (n_tets == 0) return DGNN_OK;
    McState* st = (McState*)scratch;
    (void)hipMemsetAsync(st, 0, sizeof(McState), stream);
    int rc = cl_check_tets(tetrahedra, n_tets, n_vertices, st, stream, "tet_sample_points");
    if (rc) return rc;
    hipLaunchKernelGGL(k_tet_sample, mesh_launch_grid(n_tets * n_samples), dim3(MESH_THREADS), 0, stream, vertices, tetrahedra, n_tets, n_samples, seed, tet_offset,
                       points_out);
    return dgnn_check_launch("tet_sample_points");
}
