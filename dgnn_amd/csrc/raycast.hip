// First-hit ray casting over a triangle mesh: the primitive of the virtual scanner (processing/scan_mesh.py).  DESIGN §27; the contract is
// in include/dgnn_hip.h.  Everything is fp64 and every product, sum and division rounds on its own (-ffp-contract=off).
//
//   rule       ray r is o + t d, d = g - o.  A face (a, b, c) is crossed when the three exact signs det[g - o, a - o, b - o], det[g - o, b - o,
//              c - o], det[g - o, c - o, a - o] (exact_orient.h: filter, then expansion) are all >= 0 or all <= 0 and not all 0; its
//              parameter is t = n . (a - o) / (n . d), n = (b - a) x (c - a); the answer is the smallest t above t_min, ties to the lowest face.
//   grid       a uniform 3D grid over the box of the referenced vertices, built by the entry-grid builder of mesh_grid.h (which
//              meshcontains.hip uses for its xy grid): one work item per (face, cell) entry.  A face is entered in every cell its
//              bounding box touches, through the one monotone map rc_cell.
//   traversal  one lane per ray.  The computed t of a sliver says nothing about where the sliver is, so no hit is ever final before the
//              whole line has been walked: the line is clipped to the box and walked slab by slab along its fastest axis (in cells); per
//              slab the two other coordinates at the slab's two ends give a rectangle of cells.  Every bound is widened by eps_w = 2^-46
//              of the largest coordinate magnitude M in play (128 u M, u = 2^-53; the roundings behind a bound add up to less than 34 u M)
//              and goes through rc_cell as the faces' boxes did: the cell of the true crossing point is therefore in both sets (DESIGN
//              §27 has the argument).  The answer is a minimum over a set that contains every crossed face, under a total order: the
//              grid resolution, the order inside a cell and the number of times a face is met do not matter.  A face that spans several
//              visited cells is tested in the first of them only (its box against the slab's rectangle and the one before): that saves
//              work, most of all the exact stage's, and cannot lose a face.
//   stats      hits and skipped rays; the signs of the HIT faces that the exact stage decided; crossings dropped as degenerate, each face
//              once: a ray that meets one recounts over all faces (out of line, rare), since the walk may meet a face in several cells.
#include "exact_orient.h"
#include "mesh_grid.h"

namespace {

using dgnn_exact::V3;
using dgnn_exact::load_v3;

constexpr int RC_MAX_R = 1024;
constexpr double RC_MARGIN = 0x1p-46;          // of the largest coordinate magnitude M of the box and the ray: 128 u M, u = 2^-53
constexpr int32_t RC_BAD_ID = 1, RC_NONFINITE = 2, RC_RANGE = 4;
enum { RC_HITS = 0, RC_SKIPPED, RC_DEGENERATE, RC_EXACT, RC_N_STATS };

struct RcState {
    int32_t err, pad;
    unsigned long long lo[3], hi[3];          // bbox of the referenced vertices (f64_key)
    unsigned long long n_entries;
    unsigned long long stats[RC_N_STATS];
};
static_assert(sizeof(RcState) <= 256, "RcState must fit the first scratch slot");

using RcGrid = CellGrid;          // the frame, the cell map, the faces' boxes and the cell policy are mesh_grid.h's
using RcBox = CellBox;
using RcCells = BoxCells;

__device__ __forceinline__ int32_t rc_pick(const int32_t (&p)[3], int k) { return k == 0 ? p[0] : (k == 1 ? p[1] : p[2]); }
// the status bits of a coordinate that is not finite or outside the exact predicate's range; the bounding box (k_bbox_referenced) leaves it out
struct RcCoordErr {
    __device__ int32_t operator()(double x) const {
        const dgnn_exact::CoordClass k = dgnn_exact::coord_class(x);
        return k == dgnn_exact::COORD_FINE ? 0 : (k == dgnn_exact::COORD_NONFINITE ? RC_NONFINITE : RC_RANGE);
    }
};

__device__ __forceinline__ int32_t rc_cell(const RcGrid& g, int a, double x) { return grid_cell(g, a, x); }

// ---- validation ------------------------------------------------------------------------------------------------------------------
__global__ void k_rc_check_rays(const double* __restrict__ origins, const double* __restrict__ aims, int64_t n3, RcState* st) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n3; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t e = RcCoordErr{}(origins[i]) | RcCoordErr{}(aims[i]);
        if (e) atomicOr(&st->err, e);
    }
}

// ---- the rays --------------------------------------------------------------------------------------------------------------------
struct RcBest { double t; int32_t face, exact; };

// 0: the line does not cross the face; 1: it does and *t is its parameter; 2: it does and the parameter is degenerate.  *exact = the signs
// the exact stage decided.
__device__ __forceinline__ int rc_face(const double* __restrict__ v, const int32_t* __restrict__ faces, int64_t f, const V3& o, const V3& g, const V3& d,
                                       double* t, int* exact) {
    const V3 a = load_v3(v, faces[3 * f]), b = load_v3(v, faces[3 * f + 1]), c = load_v3(v, faces[3 * f + 2]);
    int ex[3] = {0, 0, 0};
    const int s1 = dgnn_exact::orient_sign(o, g, a, b, &ex[0]);
    const int s2 = dgnn_exact::orient_sign(o, g, b, c, &ex[1]);
    const int s3 = dgnn_exact::orient_sign(o, g, c, a, &ex[2]);
    *exact = ex[0] + ex[1] + ex[2];
    const bool nonneg = s1 >= 0 && s2 >= 0 && s3 >= 0, nonpos = s1 <= 0 && s2 <= 0 && s3 <= 0;
    if (!(nonneg || nonpos) || (nonneg && nonpos)) return 0;
    const V3 n = cross(sub(b, a), sub(c, a));
    const double num = dot(n, sub(a, o)), den = dot(n, d);
    if (den == 0.0) return 2;
    *t = num / den;
    return isfinite(*t) ? 1 : 2;
}

// the degenerate crossings of one ray over ALL faces, each once (the walk may meet a face in several cells)
__device__ __noinline__ int64_t rc_count_degenerate(const double* __restrict__ v, const int32_t* __restrict__ faces, int64_t nf, V3 o, V3 g, V3 d) {
    int64_t n = 0;
    for (int64_t f = 0; f < nf; ++f) {
        double t;
        int ex;
        n += rc_face(v, faces, f, o, g, d, &t, &ex) == 2;
    }
    return n;
}

__global__ void __launch_bounds__(MESH_THREADS) k_rc_rays(const double* __restrict__ v, const int32_t* __restrict__ faces, int64_t nf,
                                                        const int32_t* __restrict__ rowptr, const int32_t* __restrict__ entries,
                                                        const RcBox* __restrict__ tbox, RcGrid G, const double* __restrict__ origins, const double* __restrict__ aims, int64_t nr, double t_min,
                                                        int32_t* __restrict__ hit_face, double* __restrict__ hit_t, double* __restrict__ hit_point,
                                                        RcState* st) {
    unsigned long long cnt[RC_N_STATS] = {0, 0, 0, 0};
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < nr; r += (int64_t)gridDim.x * blockDim.x) {
        const V3 o = load_v3(origins, r), g = load_v3(aims, r);
        const V3 d = sub(g, o);
        RcBest best{0.0, -1, 0};
        bool degenerate = false;
        if (o.x == g.x && o.y == g.y && o.z == g.z) {
            ++cnt[RC_SKIPPED];
        } else {
            const double oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
            double mag = G.mag;
#pragma unroll
            for (int a = 0; a < 3; ++a) mag = fmax(mag, fmax(fabs(oo[a]), fabs(get(g, a))));
            const double eps = RC_MARGIN * mag;
            // the line clipped to the widened box: [t_in, t_out]; the fastest axis in cells
            double t_in = -INFINITY, t_out = INFINITY, speed = -1.0;
            bool miss = false;
            int m = 0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (dd[a] != 0.0) {
                    const double ta = ((G.lo[a] - eps) - oo[a]) / dd[a], tb = ((G.hi[a] + eps) - oo[a]) / dd[a];
                    t_in = fmax(t_in, fmin(ta, tb));
                    t_out = fmin(t_out, fmax(ta, tb));
                } else if (oo[a] < G.lo[a] - eps || oo[a] > G.hi[a] + eps) {
                    miss = true;
                }
                const double s = G.n[a] > 1 ? fabs(dd[a]) * G.inv[a] : 0.0;
                if (s > speed) { speed = s; m = a; }
            }
            if (speed == 0.0) m = fabs(dd[1]) > fabs(dd[0]) ? (fabs(dd[2]) > fabs(dd[1]) ? 2 : 1) : (fabs(dd[2]) > fabs(dd[0]) ? 2 : 0);
            if (!miss && t_in <= t_out) {
                const int a1 = m == 0 ? 1 : 0, a2 = m == 2 ? 1 : 2;
                const double om = oo[m], dm = dd[m];
                const double pm0 = om + t_in * dm, pm1 = om + t_out * dm;
                const int32_t k0 = rc_cell(G, m, fmin(pm0, pm1) - eps), k1 = rc_cell(G, m, fmax(pm0, pm1) + eps);
                int32_t q10 = 0, q11 = -1, q20 = 0, q21 = -1;          // the rectangle of the slab before (empty: none)
                for (int32_t k = k0; k <= k1; ++k) {
                    // the slab's span of t, widened, within [t_in, t_out]
                    const double x0 = (G.lo[m] + (double)k * G.h[m]) - eps, x1 = (G.lo[m] + (double)(k + 1) * G.h[m]) + eps;
                    const double ta = (x0 - om) / dm, tb = (x1 - om) / dm;
                    const double ts = fmax(fmin(ta, tb), t_in), te = fmin(fmax(ta, tb), t_out);
                    if (!(ts <= te)) { q11 = q21 = -1; q10 = q20 = 0; continue; }
                    const double p10 = oo[a1] + ts * dd[a1], p11 = oo[a1] + te * dd[a1];
                    const double p20 = oo[a2] + ts * dd[a2], p21 = oo[a2] + te * dd[a2];
                    const int32_t c10 = rc_cell(G, a1, fmin(p10, p11) - eps), c11 = rc_cell(G, a1, fmax(p10, p11) + eps);
                    const int32_t c20 = rc_cell(G, a2, fmin(p20, p21) - eps), c21 = rc_cell(G, a2, fmax(p20, p21) + eps);
                    for (int32_t c1 = c10; c1 <= c11; ++c1)
                        for (int32_t c2 = c20; c2 <= c21; ++c2) {
                            const int32_t cx = m == 0 ? k : c1, cy = m == 1 ? k : (m == 0 ? c1 : c2), cz = m == 2 ? k : c2;
                            const int64_t cell = ((int64_t)cx * G.n[1] + cy) * G.n[2] + cz;
                            for (int32_t s = rowptr[cell], e = rowptr[cell + 1]; s < e; ++s) {
                                const int32_t f = entries[s];
                                // a face whose box holds an earlier cell of this slab's rectangle, or a cell of the rectangle before, was met
                                // there; the first cell of the walk that lists a face always tests it (by induction), so no face is lost
                                const RcBox b = tbox[f];
                                const int32_t bl1 = rc_pick(b.lo, a1), bh1 = rc_pick(b.hi, a1), bl2 = rc_pick(b.lo, a2), bh2 = rc_pick(b.hi, a2);
                                if (c1 != (bl1 > c10 ? bl1 : c10) || c2 != (bl2 > c20 ? bl2 : c20)) continue;
                                if (k > rc_pick(b.lo, m) && (bl1 > q10 ? bl1 : q10) <= (bh1 < q11 ? bh1 : q11) && (bl2 > q20 ? bl2 : q20) <= (bh2 < q21 ? bh2 : q21))
                                    continue;
                                double t;
                                int ex;
                                const int kind = rc_face(v, faces, f, o, g, d, &t, &ex);
                                if (kind == 2) degenerate = true;
                                if (kind == 1 && t > t_min && (best.face < 0 || t < best.t || (t == best.t && f < best.face))) best = RcBest{t, f, ex};
                            }
                        }
                    q10 = c10; q11 = c11; q20 = c20; q21 = c21;
                }
            }
            if (degenerate) cnt[RC_DEGENERATE] += (unsigned long long)rc_count_degenerate(v, faces, nf, o, g, d);
        }
        if (best.face >= 0) {
            ++cnt[RC_HITS];
            cnt[RC_EXACT] += best.exact;
        }
        hit_face[r] = best.face;
        hit_t[r] = best.t;
        if (hit_point) {
            const bool hit = best.face >= 0;
            const double mx = best.t * d.x, my = best.t * d.y, mz = best.t * d.z;
            hit_point[3 * r] = hit ? o.x + mx : 0.0;
            hit_point[3 * r + 1] = hit ? o.y + my : 0.0;
            hit_point[3 * r + 2] = hit ? o.z + mz : 0.0;
        }
    }
#pragma unroll
    for (int j = 0; j < RC_N_STATS; ++j) wave_add_atomic(cnt[j], &st->stats[j]);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
struct RcLayout { RcState* st; RcBox* tbox; GridBufs g; int64_t bytes; };
RcLayout rc_layout(void* base, int64_t nf, int64_t R) {
    Take t{(char*)base, 256};
    RcLayout L{};
    L.st = (RcState*)base;
    L.tbox = t.take<RcBox>(nf);
    L.g = take_grid(t, nf, R * R * R);
    L.bytes = t.off;
    return L;
}

int rc_status(const RcState& hs, const char* what) {
    if (!hs.err) return DGNN_OK;
    dgnn_set_error("%s: %s%s%s", what, hs.err & RC_BAD_ID ? "a face's vertex id out of range; " : "",
                   hs.err & RC_NONFINITE ? "a non-finite coordinate of a referenced vertex, an origin or an aim; " : "",
                   hs.err & RC_RANGE ? "a coordinate magnitude outside [2^-300, 2^300] (the exact predicate's range); " : "");
    return hs.err == RC_RANGE ? DGNN_E_UNSUPPORTED : DGNN_E_INVALID;
}

bool rc_resolution_ok(int32_t R) { return R >= 1 && R <= RC_MAX_R; }

// validation, bounding box, the grid's frame, per-face boxes and their total.  On success tbox / tcnt of L are filled, *grid is the frame
// and *n_entries the (face, cell) entries.  Synchronises three times; with rays (n_rays > 0) they are validated with the vertices.
int rc_plan(const double* vertices, int64_t nv, const int32_t* faces, int64_t nf, int32_t R, const double* origins, const double* aims, int64_t n_rays,
            const RcLayout& L, RcGrid* grid, int64_t* n_entries, hipStream_t stream, const char* what) {
    DGNN_REQUIRE(nv >= 0 && nf >= 0 && (nv == 0 || vertices) && (nf == 0 || faces) && L.st, DGNN_E_INVALID, "%s: bad args", what);
    DGNN_REQUIRE(nf > 0, DGNN_E_INVALID, "%s: a mesh without faces", what);
    DGNN_REQUIRE(rc_resolution_ok(R), DGNN_E_UNSUPPORTED, "%s: grid_resolution %d outside [1, %d]", what, R, RC_MAX_R);
    DGNN_REQUIRE(nf < INT32_MAX / 4 && nv < INT32_MAX, DGNN_E_UNSUPPORTED, "%s: sizes exceed the int32 indexing", what);
    const dim3 block(MESH_THREADS);
    RcState hs{};
    hs.lo[0] = hs.lo[1] = hs.lo[2] = ~0ull;
    (void)hipMemcpyAsync(L.st, &hs, sizeof(RcState), hipMemcpyHostToDevice, stream);
    hipLaunchKernelGGL(k_check_ids, mesh_launch_grid(3 * nf), block, 0, stream, faces, 3 * nf, nv, &L.st->err, RC_BAD_ID);
    int rc = dgnn_check_launch(what);
    if (rc || (rc = mm_read(&hs, L.st, sizeof(RcState), stream, what)) || (rc = rc_status(hs, what))) return rc;   // ids are read below: checked first
    hipLaunchKernelGGL(k_bbox_referenced<RcCoordErr>, mesh_launch_grid(3 * nf), block, 0, stream, vertices, faces, 3 * nf, RcCoordErr{}, &L.st->err, L.st->lo,
                       L.st->hi);
    if (n_rays > 0) hipLaunchKernelGGL(k_rc_check_rays, mesh_launch_grid(3 * n_rays), block, 0, stream, origins, aims, 3 * n_rays, L.st);
    if ((rc = dgnn_check_launch(what)) || (rc = mm_read(&hs, L.st, sizeof(RcState), stream, what)) || (rc = rc_status(hs, what))) return rc;
    double lo[3], hi[3];
    bbox_unkey(hs.lo, hs.hi, lo, hi);
    const RcGrid g = cell_grid_frame(lo, hi, R);
    hipLaunchKernelGGL(k_cell_boxes, mesh_launch_grid(nf), block, 0, stream, vertices, faces, nf, g, L.tbox, L.g.tcnt, &L.st->n_entries);
    if ((rc = dgnn_check_launch(what)) || (rc = mm_read(&hs, L.st, sizeof(RcState), stream, what))) return rc;
    DGNN_REQUIRE(hs.n_entries < (unsigned long long)INT32_MAX, DGNN_E_UNSUPPORTED, "%s: %llu grid entries exceed the int32 indexing (lower grid_resolution)", what,
                 hs.n_entries);
    *grid = g;
    *n_entries = (int64_t)hs.n_entries;
    return DGNN_OK;
}

}  // namespace

// ================================================================================================================================
extern "C" int64_t dgnn_ray_first_hit_scratch_bytes(int64_t n_faces, int32_t grid_resolution) {
    if (n_faces < 0 || !rc_resolution_ok(grid_resolution)) return 256;
    return rc_layout(nullptr, n_faces, grid_resolution).bytes;
}

extern "C" int dgnn_ray_first_hit_plan(const double* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int32_t grid_resolution,
                                       int64_t* n_entries_out, int32_t* cells_out, void* scratch, void* stream_) {
    DGNN_REQUIRE(scratch && n_entries_out, DGNN_E_INVALID, "ray_first_hit_plan: bad args");
    RcGrid g{};
    const RcLayout L = rc_layout(scratch, n_faces > 0 ? n_faces : 0, rc_resolution_ok(grid_resolution) ? grid_resolution : 1);
    const int rc = rc_plan(vertices, n_vertices, faces, n_faces, grid_resolution, nullptr, nullptr, 0, L, &g, n_entries_out, (hipStream_t)stream_,
                           "ray_first_hit_plan");
    if (rc) return rc;
    if (cells_out)
        for (int a = 0; a < 3; ++a) cells_out[a] = g.n[a];
    return DGNN_OK;
}

extern "C" int dgnn_ray_first_hit(const double* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int32_t grid_resolution,
                                  const double* origins, const double* aims, int64_t n_rays, double t_min, int32_t* hit_face_out, double* hit_t_out,
                                  double* hit_point_out, int64_t* stats_out, int32_t* entries, int64_t entry_capacity, void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(scratch && stats_out && n_rays >= 0 && entry_capacity >= 0 && (n_rays == 0 || (origins && aims && hit_face_out && hit_t_out)), DGNN_E_INVALID,
                 "ray_first_hit: bad args");
    DGNN_REQUIRE(t_min >= 0.0, DGNN_E_INVALID, "ray_first_hit: t_min %g is negative or NaN", t_min);
    DGNN_REQUIRE(n_rays <= INT64_MAX / 24, DGNN_E_UNSUPPORTED, "ray_first_hit: %lld rays exceed the int64 indexing", (long long)n_rays);
    RcGrid g{};
    int64_t ne = 0;
    const RcLayout L = rc_layout(scratch, n_faces > 0 ? n_faces : 0, rc_resolution_ok(grid_resolution) ? grid_resolution : 1);
    int rc = rc_plan(vertices, n_vertices, faces, n_faces, grid_resolution, origins, aims, n_rays, L, &g, &ne, stream, "ray_first_hit");
    if (rc) return rc;
    DGNN_REQUIRE(entries && ne <= entry_capacity, DGNN_E_INVALID, "ray_first_hit: %lld grid entries, room for %lld (dgnn_ray_first_hit_plan gives the number)",
                 (long long)ne, (long long)entry_capacity);
    if (n_rays > 0) {
        if ((rc = build_entry_grid(L.g, RcCells{L.tbox, g.n[1], g.n[2]}, n_faces, (int64_t)g.n[0] * g.n[1] * g.n[2], ne, entries, stream))) return rc;
        hipLaunchKernelGGL(k_rc_rays, mesh_launch_grid(n_rays), dim3(MESH_THREADS), 0, stream, vertices, faces, n_faces, L.g.rowptr, entries, L.tbox, g, origins,
                           aims, n_rays, t_min, hit_face_out, hit_t_out, hit_point_out, L.st);
    }
    (void)hipMemcpyAsync(stats_out, L.st->stats, sizeof(int64_t) * RC_N_STATS, hipMemcpyDeviceToDevice, stream);
    return dgnn_check_launch("ray_first_hit");
}
