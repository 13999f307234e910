// Distance from points to a triangle mesh, with the closest face, point and region, and the fold of such distances into the sums, the
// maximum and the threshold counts of the surface metrics (ops.surface_metrics).  DESIGN §30; the contract is in include/dgnn_hip.h.
// Everything is fp64 and every product, sum, difference and division rounds on its own (-ffp-contract=off).
//
//   rule       md_face below, operation for operation the header's text: three segments in ascending vertex id, then the plane candidate;
//              d2 is always |p - closest|^2 of the closest point that is reported.  The answer is the minimum of (d2, face) over ALL faces.
//   grid       a uniform 3D grid over the box of the referenced vertices, built by mesh_grid.h: a face is entered in every cell its bounding
//              box touches, through the one monotone map grid_cell (the frame, the boxes and the cell policy are the ray caster's).
//   search     one lane per query: Chebyshev shells of cells about the (clamped) cell of the point.  After shell s the cells of the block
//              B = [c - s, c + s]^3 (cut to the grid) have been read.  A face without an entry in B has its whole cell box beyond one of
//              B's sides that is not at the grid's edge, say below B's low side k on axis a: every coordinate x of it has
//              fl(fl(x - lo) inv) < k, so x < X + 4 u M for the side's plane X = lo + k h (u = 2^-53, M the largest coordinate magnitude
//              of the box).  The reported closest point of EVERY candidate lies in its face's bounding box up to 2 u M (a segment's u + t e
//              with 0 < t < 1; the plane candidate's is clamped to the box), so for such a face
//              p_a - closest_a >= p_a - X - 6 u M, and its computed d2, a sum of three rounded squares, has sqrt(d2) >= (p_a - closest_a)
//              (1 - 3 u).  The side's plane as computed, fl(lo + fl(k h)), and the difference fl(p_a - plane) add less than 4 u (M + |p_a|).
//              So with b = max(fl(|p_a - plane|) - MD_MARGIN max(M, |p|_inf), 0), MD_MARGIN = 2^-46 = 128 u against a need below 20 u,
//              such a face has |p_a - closest_a| >= b.  On the two other axes the closest point lies in the mesh's box (up to the same
//              2 u M), so there |p_k - closest_k| >= o_k = max(lo_k - p_k, p_k - hi_k) - the margin, or 0: the term that lets a query far
//              outside the box stop after a few shells, not after the whole grid.  Every face not yet read therefore has computed
//              d2 >= (b^2 + o_k^2 + o_l^2) (1 - 4 u), and B2 = the minimum of fl(b b + (o_k^2 + o_l^2)) over the sides that are not at the
//              grid's edge is within (1 + 3 u) of that sum: the search stops when best d2 < B2 (1 - 2^-50), strictly, so that a tie in d2
//              with a lower face further out is still found.  The bound holds for a point outside the box as well: its clamped cell is at
//              the grid's edge on that side, that side never counts, and the other sides' planes lie between the point and the faces beyond
//              them all the same.  When every side is at the grid's edge the whole grid was read (kept as a flag, not read off B2: for
//              coordinates so large that the squares overflow, B2 is inf and the search simply reads on to the last shell).
//   repeats    a face is entered in every cell of its box: one whose box meets the block of the shell before was evaluated then (by
//              induction every entry of that block was) and is skipped; within a shell it may be evaluated more than once, which a
//              lexicographic minimum does not see.
//   cliff      a query deep inside an empty region, at about the same distance from much of the mesh (the centre of a sphere), reads
//              O(s^2) cells per shell and in the end nearly the whole grid: §14's empty-shell cliff, measured in profiles/mesh_distance.md.
//              For such queries grid_resolution = 0 is the faster call; a coarse occupancy level is not built.
//   stats      entries of the grid; shells read (the largest per query and their total); (point, face) evaluations.
#include <math.h>

#include "fixed_sum.h"
#include "mesh_grid.h"
#include "vec3.h"

namespace {

using dgnn_exact::V3;
using dgnn_exact::load_v3;

constexpr int MD_MAX_R = 1024;
constexpr double MD_MARGIN = 0x1p-46;          // of max(M, |p|_inf): 128 u, u = 2^-53 (the derivation is above)
constexpr double MD_SHRINK = 1.0 - 0x1p-50;
constexpr int32_t MD_BAD_ID = 1, MD_NONFINITE = 2;
enum { MD_SHELL_MAX = 0, MD_SHELL_SUM, MD_EVALS, MD_N_STATS };

struct MdState {
    int32_t err, pad;
    unsigned long long lo[3], hi[3];          // bbox of the referenced vertices (f64_key)
    unsigned long long n_entries;
    unsigned long long stats[MD_N_STATS];
};
static_assert(sizeof(MdState) <= 256, "MdState must fit the first scratch slot");

using MdGrid = CellGrid;          // the frame, the cell map, the faces' boxes and the cell policy are mesh_grid.h's
using MdBox = CellBox;

struct MdNonFinite {
    __device__ int32_t operator()(double x) const { return isfinite(x) ? 0 : MD_NONFINITE; }
};

// ---- the rule ----------------------------------------------------------------------------------------------------------------------
struct MdBest { double d2; V3 c; int32_t face, region; };

// segment (u, v), u the lower vertex id: -> d2, *c the closest point, *code 0 = inside the segment, 1 = at u, 2 = at v
__device__ __forceinline__ double md_segment(const V3& p, const V3& u, const V3& v, V3* c, int* code) {
    const V3 e = sub(v, u), w = sub(p, u);
    const double ee = dot(e, e), we = dot(w, e);
    if (we <= 0.0 || ee == 0.0) {
        *c = u;
        *code = 1;
    } else if (we >= ee) {
        *c = v;
        *code = 2;
    } else {
        const double t = we / ee;
        *c = V3{u.x + t * e.x, u.y + t * e.y, u.z + t * e.z};
        *code = 0;
    }
    const V3 d = sub(p, *c);
    return dot(d, d);
}

// face f against point p: (d2, closest, region) of the face -> best when (d2, f) is lexicographically below it
__device__ __forceinline__ void md_face(const double* __restrict__ v, const int32_t* __restrict__ faces, int32_t f, const V3& p, MdBest& best) {
    const int32_t id[3] = {faces[3 * (int64_t)f], faces[3 * (int64_t)f + 1], faces[3 * (int64_t)f + 2]};
    const V3 t[3] = {load_v3(v, id[0]), load_v3(v, id[1]), load_v3(v, id[2])};
    double d2 = 0.0;
    V3 c{};
    int region = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int j = k == 2 ? 0 : k + 1;
        const bool swap = id[k] > id[j];
        const int iu = swap ? j : k, iv = swap ? k : j;
        const V3 u = swap ? t[j] : t[k], w = swap ? t[k] : t[j];
        V3 ck;
        int code;
        const double dk = md_segment(p, u, w, &ck, &code);
        if (k == 0 || dk < d2) {
            d2 = dk;
            c = ck;
            region = code == 0 ? 1 + k : 4 + (code == 1 ? iu : iv);
        }
    }
    const V3 n = cross(sub(t[1], t[0]), sub(t[2], t[0]));
    const double nn = dot(n, n);
    if (nn > 0.0 && dot(cross(sub(t[1], t[0]), sub(p, t[0])), n) > 0.0 && dot(cross(sub(t[2], t[1]), sub(p, t[1])), n) > 0.0 &&
        dot(cross(sub(t[0], t[2]), sub(p, t[2])), n) > 0.0) {
        const double s = dot(sub(p, t[0]), n) / nn;
        // the foot of the perpendicular, clamped per axis to the face's bounding box: a rounding for a sound normal (exactly onto the plane
        // of an axis-aligned face), and for a sliver's unsound one still a point of the box
        const V3 cp{fmin(fmax(p.x - s * n.x, fmin(fmin(t[0].x, t[1].x), t[2].x)), fmax(fmax(t[0].x, t[1].x), t[2].x)),
                    fmin(fmax(p.y - s * n.y, fmin(fmin(t[0].y, t[1].y), t[2].y)), fmax(fmax(t[0].y, t[1].y), t[2].y)),
                    fmin(fmax(p.z - s * n.z, fmin(fmin(t[0].z, t[1].z), t[2].z)), fmax(fmax(t[0].z, t[1].z), t[2].z))};
        const V3 d = sub(p, cp);
        const double dp = dot(d, d);
        if (dp < d2) {
            d2 = dp;
            c = cp;
            region = 0;
        }
    }
    if (best.face < 0 || d2 < best.d2 || (d2 == best.d2 && f < best.face)) best = MdBest{d2, c, f, region};
}

struct MdOut { double *d2, *dist; int32_t* face; double* closest; uint8_t* region; };          // dist = sqrt(d2), correctly rounded; NULL: not written

__device__ __forceinline__ void md_store(const MdBest& b, int64_t i, const MdOut& o) {
    double* __restrict__ d2 = o.d2;
    int32_t* __restrict__ face = o.face;
    double* __restrict__ closest = o.closest;
    uint8_t* __restrict__ region = o.region;
    d2[i] = b.d2;
    if (o.dist) o.dist[i] = sqrt(b.d2);
    face[i] = b.face;
    closest[3 * i] = b.c.x;
    closest[3 * i + 1] = b.c.y;
    closest[3 * i + 2] = b.c.z;
    region[i] = (uint8_t)b.region;
}

__global__ void k_md_check_points(const double* __restrict__ p, int64_t n3, MdState* st) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n3; i += (int64_t)gridDim.x * blockDim.x)
        if (!isfinite(p[i])) atomicOr(&st->err, MD_NONFINITE);
}

// ---- all pairs: every face per lane ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MESH_THREADS) k_md_all_pairs(const double* __restrict__ v, const int32_t* __restrict__ faces, int32_t nf,
                                                             const double* __restrict__ points, int64_t n, MdOut out, MdState* st) {
    unsigned long long evals = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const V3 p = load_v3(points, i);
        MdBest best{0.0, V3{0.0, 0.0, 0.0}, -1, 0};
        for (int32_t f = 0; f < nf; ++f) md_face(v, faces, f, p, best);
        evals += (unsigned long long)nf;
        md_store(best, i, out);
    }
    wave_add_atomic(evals, &st->stats[MD_EVALS]);
}

// ---- the search ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int32_t md_max(int32_t a, int32_t b) { return a > b ? a : b; }
__device__ __forceinline__ int32_t md_min(int32_t a, int32_t b) { return a < b ? a : b; }

__global__ void __launch_bounds__(MESH_THREADS) k_md_search(const double* __restrict__ v, const int32_t* __restrict__ faces,
                                                          const int32_t* __restrict__ rowptr, const int32_t* __restrict__ entries,
                                                          const MdBox* __restrict__ tbox, MdGrid G, const double* __restrict__ points, int64_t n,
                                                          MdOut out, MdState* st) {
    unsigned long long evals = 0, shell_sum = 0;
    int32_t shell_max = 0;
    const int32_t s_end = md_max(G.n[0], md_max(G.n[1], G.n[2]));          // shells <= the resolution
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const V3 p = load_v3(points, i);
        const double pp[3] = {p.x, p.y, p.z};
        int32_t c[3];
        double mag = G.mag;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            c[a] = grid_cell(G, a, pp[a]);
            mag = fmax(mag, fabs(pp[a]));
        }
        const double eps = MD_MARGIN * mag;
        double out2[3];          // per axis, the squared distance from the point to the box's span (0 inside it), shrunk by the margin
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double o = fmax(fmax(G.lo[a] - pp[a], pp[a] - G.hi[a]) - eps, 0.0);
            out2[a] = o * o;
        }
        MdBest best{0.0, V3{0.0, 0.0, 0.0}, -1, 0};
        int32_t s = 0;
        for (; s < s_end; ++s) {
            const int32_t x0 = md_max(c[0] - s, 0), x1 = md_min(c[0] + s, G.n[0] - 1);
            const int32_t y0 = md_max(c[1] - s, 0), y1 = md_min(c[1] + s, G.n[1] - 1);
            const int32_t z0 = md_max(c[2] - s, 0), z1 = md_min(c[2] + s, G.n[2] - 1);
            for (int32_t x = x0; x <= x1; ++x)
                for (int32_t y = y0; y <= y1; ++y) {
                    // the cells of the column at Chebyshev distance s: all of it when x or y is on the shell, else its two ends
                    const bool whole = x == c[0] - s || x == c[0] + s || y == c[1] - s || y == c[1] + s;
                    const int32_t step = whole ? 1 : 2 * s;
                    for (int32_t z = whole ? z0 : c[2] - s; z <= (whole ? z1 : c[2] + s); z += step) {
                        if (z < z0 || z > z1) continue;
                        const int64_t cell = ((int64_t)x * G.n[1] + y) * G.n[2] + z;
                        for (int32_t k = rowptr[cell], e = rowptr[cell + 1]; k < e; ++k) {
                            const int32_t f = entries[k];
                            if (s > 0) {          // met in the block of the shell before: evaluated then
                                const MdBox b = tbox[f];
                                if (md_max(b.lo[0], c[0] - s + 1) <= md_min(b.hi[0], c[0] + s - 1) && md_max(b.lo[1], c[1] - s + 1) <= md_min(b.hi[1], c[1] + s - 1) &&
                                    md_max(b.lo[2], c[2] - s + 1) <= md_min(b.hi[2], c[2] + s - 1))
                                    continue;
                            }
                            md_face(v, faces, f, p, best);
                            ++evals;
                        }
                    }
                }
            // the squared distance to everything not yet read: the nearest side of the block that is not at the grid's edge
            double b2 = INFINITY;
            bool open_side = false;
            const int32_t blo[3] = {x0, y0, z0}, bhi[3] = {x1, y1, z1};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double rest = out2[a == 0 ? 1 : 0] + out2[a == 2 ? 1 : 2];
                if (blo[a] > 0) {
                    open_side = true;
                    const double b = fmax((pp[a] - (G.lo[a] + (double)blo[a] * G.h[a])) - eps, 0.0);
                    b2 = fmin(b2, b * b + rest);
                }
                if (bhi[a] < G.n[a] - 1) {
                    open_side = true;
                    const double b = fmax(((G.lo[a] + (double)(bhi[a] + 1) * G.h[a]) - pp[a]) - eps, 0.0);
                    b2 = fmin(b2, b * b + rest);
                }
            }
            if (!open_side) { ++s; break; }          // every side at the grid's edge: the whole grid was read
            if (best.face >= 0 && best.d2 < b2 * MD_SHRINK) { ++s; break; }
        }
        shell_sum += (unsigned long long)s;
        shell_max = md_max(shell_max, s);
        md_store(best, i, out);
    }
    wave_add_atomic(evals, &st->stats[MD_EVALS]);
    wave_add_atomic(shell_sum, &st->stats[MD_SHELL_SUM]);
    for (int o = 32; o > 0; o >>= 1) shell_max = md_max(shell_max, __shfl_xor(shell_max, o));
    if (lane_id() == 0 && shell_max) atomicMax(&st->stats[MD_SHELL_MAX], (unsigned long long)shell_max);
}

// ---- the fold ------------------------------------------------------------------------------------------------------------------------
// chunk t = [t C, (t + 1) C) of fixed_sum.h: serial sums of dist and |cosine| and the maximum of dist -> part[0 / 1 / 2][t]
__global__ void k_md_fold_chunks(const double* __restrict__ dist, const double* __restrict__ cosine, int64_t n, int64_t nch, double* __restrict__ part) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < nch; t += (int64_t)gridDim.x * blockDim.x) {
        double s = 0.0, sc = 0.0, m = 0.0;
        const int64_t e = (t + 1) * FIXED_SUM_CHUNK < n ? (t + 1) * FIXED_SUM_CHUNK : n;
        for (int64_t i = t * FIXED_SUM_CHUNK; i < e; ++i) {
            const double d = dist[i];
            s += d;
            m = d > m ? d : m;
            if (cosine) sc += fabs(cosine[i]);
        }
        part[t] = s;
        part[nch + t] = sc;
        part[2 * nch + t] = m;
    }
}

// the chunk results serially, in chunk order -> out[0] = sum of dist, out[1] = sum of |cosine|, out[2] = max of dist
__global__ void k_md_fold_total(const double* __restrict__ part, int64_t nch, double* __restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double s = 0.0, sc = 0.0, m = 0.0;
    for (int64_t t = 0; t < nch; ++t) {
        s += part[t];
        sc += part[nch + t];
        m = part[2 * nch + t] > m ? part[2 * nch + t] : m;
    }
    out[0] = s;
    out[1] = sc;
    out[2] = m;
}

// counts[t] = #{dist <= thresholds[t]}: integer sums, order-free (counts zeroed by the caller)
__global__ void __launch_bounds__(MESH_THREADS) k_md_fold_counts(const double* __restrict__ dist, int64_t n, const double* __restrict__ thresholds, int32_t nt,
                                                               unsigned long long* __restrict__ counts) {
    for (int32_t t = 0; t < nt; ++t) {
        const double thr = thresholds[t];
        unsigned long long c = 0;
        for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) c += dist[i] <= thr;
        wave_add_atomic(c, counts + t);
    }
}

__global__ void k_md_row_dot3(const double* __restrict__ a, const int32_t* __restrict__ ia, const double* __restrict__ b, const int32_t* __restrict__ ib,
                              int64_t n, double* __restrict__ out) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = dot(load_v3(a, ia[i]), load_v3(b, ib[i]));
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
struct MdLayout { MdState* st; MdBox* tbox; GridBufs g; int64_t bytes; };
MdLayout md_layout(void* base, int64_t nf, int64_t R) {
    Take t{(char*)base, 256};
    MdLayout L{};
    L.st = (MdState*)base;
    if (R > 0) {
        L.tbox = t.take<MdBox>(nf);
        L.g = take_grid(t, nf, R * R * R);
    }
    L.bytes = t.off;
    return L;
}

int md_status(const MdState& hs, const char* what) {
    if (!hs.err) return DGNN_OK;
    dgnn_set_error("%s: %s%s", what, hs.err & MD_BAD_ID ? "a face's vertex id out of range; " : "",
                   hs.err & MD_NONFINITE ? "a non-finite coordinate of a referenced vertex or of a point; " : "");
    return DGNN_E_INVALID;
}

bool md_resolution_ok(int32_t R) { return R >= 0 && R <= MD_MAX_R; }

// validation (ids, then the referenced vertices and the points) and, with R > 0, the grid's frame, the faces' boxes and their total.
// Synchronises twice, three times with a grid.
int md_plan(const double* vertices, int64_t nv, const int32_t* faces, int64_t nf, int32_t R, const double* points, int64_t n, const MdLayout& L,
            MdGrid* grid, int64_t* n_entries, hipStream_t stream, const char* what) {
    DGNN_REQUIRE(nv >= 0 && nf >= 0 && (nv == 0 || vertices) && (nf == 0 || faces) && L.st, DGNN_E_INVALID, "%s: bad args", what);
    DGNN_REQUIRE(nf > 0, DGNN_E_INVALID, "%s: a mesh without faces", what);
    DGNN_REQUIRE(md_resolution_ok(R), DGNN_E_UNSUPPORTED, "%s: grid_resolution %d outside [0, %d]", what, R, MD_MAX_R);
    DGNN_REQUIRE(nf < INT32_MAX / 4 && nv < INT32_MAX, DGNN_E_UNSUPPORTED, "%s: sizes exceed the int32 indexing", what);
    const dim3 block(MESH_THREADS);
    MdState hs{};
    hs.lo[0] = hs.lo[1] = hs.lo[2] = ~0ull;
    (void)hipMemcpyAsync(L.st, &hs, sizeof(MdState), hipMemcpyHostToDevice, stream);
    hipLaunchKernelGGL(k_check_ids, mesh_launch_grid(3 * nf), block, 0, stream, faces, 3 * nf, nv, &L.st->err, MD_BAD_ID);
    int rc = dgnn_check_launch(what);
    if (rc || (rc = mm_read(&hs, L.st, sizeof(MdState), stream, what)) || (rc = md_status(hs, what))) return rc;   // ids are read below: checked first
    hipLaunchKernelGGL(k_bbox_referenced<MdNonFinite>, mesh_launch_grid(3 * nf), block, 0, stream, vertices, faces, 3 * nf, MdNonFinite{}, &L.st->err,
                       L.st->lo, L.st->hi);
    if (n > 0) hipLaunchKernelGGL(k_md_check_points, mesh_launch_grid(3 * n), block, 0, stream, points, 3 * n, L.st);
    if ((rc = dgnn_check_launch(what)) || (rc = mm_read(&hs, L.st, sizeof(MdState), stream, what)) || (rc = md_status(hs, what))) return rc;
    *n_entries = 0;
    if (R == 0) return DGNN_OK;
    double lo[3], hi[3];
    bbox_unkey(hs.lo, hs.hi, lo, hi);
    const MdGrid g = cell_grid_frame(lo, hi, R);
    hipLaunchKernelGGL(k_cell_boxes, mesh_launch_grid(nf), block, 0, stream, vertices, faces, nf, g, L.tbox, L.g.tcnt, &L.st->n_entries);
    if ((rc = dgnn_check_launch(what)) || (rc = mm_read(&hs, L.st, sizeof(MdState), stream, what))) return rc;
    DGNN_REQUIRE(hs.n_entries < (unsigned long long)INT32_MAX, DGNN_E_UNSUPPORTED, "%s: %llu grid entries exceed the int32 indexing (lower grid_resolution)", what,
                 hs.n_entries);
    *grid = g;
    *n_entries = (int64_t)hs.n_entries;
    return DGNN_OK;
}

}  // namespace

// ================================================================================================================================
extern "C" int64_t dgnn_point_mesh_distance_scratch_bytes(int64_t n_faces, int32_t grid_resolution) {
    if (n_faces < 0 || !md_resolution_ok(grid_resolution)) return 256;
    return md_layout(nullptr, n_faces, grid_resolution).bytes;
}

extern "C" int dgnn_point_mesh_distance_plan(const double* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int32_t grid_resolution,
                                             int64_t* n_entries_out, void* scratch, void* stream_) {
    DGNN_REQUIRE(scratch && n_entries_out, DGNN_E_INVALID, "point_mesh_distance_plan: bad args");
    MdGrid g{};
    const MdLayout L = md_layout(scratch, n_faces > 0 ? n_faces : 0, md_resolution_ok(grid_resolution) ? grid_resolution : 0);
    return md_plan(vertices, n_vertices, faces, n_faces, grid_resolution, nullptr, 0, L, &g, n_entries_out, (hipStream_t)stream_, "point_mesh_distance_plan");
}

extern "C" int dgnn_point_mesh_distance(const double* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int32_t grid_resolution,
                                        const double* points, int64_t n_points, double* d2_out, double* dist_out, int32_t* face_out,
                                        double* closest_out, uint8_t* region_out, int64_t* stats_out, int32_t* entries, int64_t entry_capacity, void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(scratch && stats_out && n_points >= 0 && entry_capacity >= 0 && (n_points == 0 || (points && d2_out && face_out && closest_out && region_out)),
                 DGNN_E_INVALID, "point_mesh_distance: bad args");
    DGNN_REQUIRE(n_points <= INT64_MAX / 24, DGNN_E_UNSUPPORTED, "point_mesh_distance: %lld points exceed the int64 indexing", (long long)n_points);
    MdGrid g{};
    int64_t ne = 0;
    const int32_t R = grid_resolution;
    const MdLayout L = md_layout(scratch, n_faces > 0 ? n_faces : 0, md_resolution_ok(R) ? R : 0);
    int rc = md_plan(vertices, n_vertices, faces, n_faces, R, points, n_points, L, &g, &ne, stream, "point_mesh_distance");
    if (rc) return rc;
    DGNN_REQUIRE(R == 0 || (entries && ne <= entry_capacity), DGNN_E_INVALID,
                 "point_mesh_distance: %lld grid entries, room for %lld (dgnn_point_mesh_distance_plan gives the number)", (long long)ne, (long long)entry_capacity);
    const MdOut out{d2_out, dist_out, face_out, closest_out, region_out};
    if (n_points > 0) {
        if (R == 0) {
            hipLaunchKernelGGL(k_md_all_pairs, mesh_launch_grid(n_points), dim3(MESH_THREADS), 0, stream, vertices, faces, (int32_t)n_faces, points, n_points, out, L.st);
        } else {
            if ((rc = build_entry_grid(L.g, BoxCells{L.tbox, g.n[1], g.n[2]}, n_faces, (int64_t)g.n[0] * g.n[1] * g.n[2], ne, entries, stream))) return rc;
            hipLaunchKernelGGL(k_md_search, mesh_launch_grid(n_points), dim3(MESH_THREADS), 0, stream, vertices, faces, L.g.rowptr, entries, L.tbox, g, points, n_points,
                               out, L.st);
        }
    }
    // stats: entries, the largest shell count, the shells' total, the evaluations
    (void)hipMemcpyAsync(stats_out, &L.st->n_entries, sizeof(int64_t) * (1 + MD_N_STATS), hipMemcpyDeviceToDevice, stream);
    return dgnn_check_launch("point_mesh_distance");
}

extern "C" int64_t dgnn_distance_fold_scratch_bytes(int64_t n) {
    if (n < 0) return 256;
    return 256 + (3 * dgnn_cdiv(n, FIXED_SUM_CHUNK) + 3) * (int64_t)sizeof(double);
}

extern "C" int dgnn_distance_fold(const double* dist, const double* cosine, int64_t n, const double* thresholds, int32_t n_thresholds, double* sums_out,
                                  int64_t* counts_out, void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(scratch && sums_out && n >= 0 && n_thresholds >= 0 && (n == 0 || dist) && (n_thresholds == 0 || (thresholds && counts_out)), DGNN_E_INVALID,
                 "distance_fold: bad args");
    const int64_t nch = dgnn_cdiv(n, FIXED_SUM_CHUNK);
    double* part = (double*)((char*)scratch + 256);
    if (nch > 0)
        hipLaunchKernelGGL(k_md_fold_chunks, dim3(dgnn_grid_cap(dgnn_cdiv(nch, FIXED_SUM_THREADS))), dim3(FIXED_SUM_THREADS), 0, stream, dist, cosine, n, nch, part);
    hipLaunchKernelGGL(k_md_fold_total, dim3(1), dim3(64), 0, stream, part, nch, sums_out);
    if (n_thresholds > 0) {
        (void)hipMemsetAsync(counts_out, 0, sizeof(int64_t) * n_thresholds, stream);
        if (n > 0)
            hipLaunchKernelGGL(k_md_fold_counts, mesh_launch_grid(n), dim3(MESH_THREADS), 0, stream, dist, n, thresholds, n_thresholds, (unsigned long long*)counts_out);
    }
    return dgnn_check_launch("distance_fold");
}

extern "C" int dgnn_row_dot3(const double* a, int64_t n_a, const int32_t* ia, const double* b, int64_t n_b, const int32_t* ib, int64_t n, double* out,
                             void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(scratch && n >= 0 && n_a >= 0 && n_b >= 0 && (n == 0 || (a && b && ia && ib && out)), DGNN_E_INVALID, "row_dot3: bad args");
    if (n == 0) return DGNN_OK;
    int32_t* err = (int32_t*)scratch;
    int32_t herr = 0;
    (void)hipMemsetAsync(err, 0, sizeof(int32_t), stream);
    hipLaunchKernelGGL(k_check_ids, mesh_launch_grid(n), dim3(MESH_THREADS), 0, stream, ia, n, n_a, err, 1);
    hipLaunchKernelGGL(k_check_ids, mesh_launch_grid(n), dim3(MESH_THREADS), 0, stream, ib, n, n_b, err, 1);
    int rc = dgnn_check_launch("row_dot3");
    if (rc || (rc = mm_read(&herr, err, sizeof(int32_t), stream, "row_dot3"))) return rc;   // ids are read below: checked first
    DGNN_REQUIRE(!herr, DGNN_E_INVALID, "row_dot3: a row index out of range");
    hipLaunchKernelGGL(k_md_row_dot3, mesh_launch_grid(n), dim3(MESH_THREADS), 0, stream, a, ia, b, ib, n, out);
    return dgnn_check_launch("row_dot3");
}
