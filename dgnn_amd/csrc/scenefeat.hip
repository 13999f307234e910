// The scene front end on the device: what a triangulation (`_3dt.npz`) and a scan (points + sensor positions) give before the model runs --
// cell adjacency by slot, cell geometry (`_cgeom`) and the vertex-ray visibility aggregates (`_cbvf`, `_fbvf`).  DESIGN §25; the contract
// is in include/dgnn_hip.h.  Every kernel is fp64 and every product, sum, division and square root rounds on its own (-ffp-contract=off).
//
//   neighbours  one thread per (facet, side): the slot of the cell's one vertex that is not on the facet gets the cell on the other side.
//   geometry    one thread per tet; the two column sums of the loader's mean_edge in the fixed order of fixed_sum.h.
//   incidence   vertex -> (tet, slot): count (one atomic per corner), exclusive scan, fill through a cursor per vertex.  The order inside a
//               row is whatever the fill gives; no consumer depends on it.
//   rays        one thread per ray scans the tets incident to its vertex with the exact orientation predicate and keeps, per side, the
//               lowest qualifying tet: a minimum over a set, so the row order does not matter.  The (tet, slot, dist) record of either
//               side is stored per ray; per side the ray ids are sorted stably by tet, so every tet owns a run of ray ids in ascending
//               order, and one thread per tet folds its run serially: counts, min / max and the sums in ascending ray index, for the tet
//               and for each of its four slots.  No floating-point atomics: reruns are bit-identical.  The steps that the facet-ray walk
//               (raywalk.hip) takes as well -- first ray per vertex, the incident-corner prologue, ray lengths, runs, the fold -- are
//               tet_rays.h's; the facet / slot rule and the row helpers are tet_common.h's.
#include "fixed_sum.h"
#include "tet_rays.h"

namespace {

constexpr int SF_SIDES = 2;          // 0 = outside (towards the sensor), 1 = inside (away from it)
constexpr int64_t SF_MAX_RAYS = RAY_FIRST_NONE;
enum { SF_USED = 0, SF_DUPLICATE, SF_DEGENERATE, SF_NO_OUTSIDE, SF_NO_INSIDE, SF_EXACT, SF_N_STATS };

using dgnn_exact::orient_coords_ok;

// ---- neighbours ----------------------------------------------------------------------------------------------------------------
__global__ void k_neighbors(const int32_t* __restrict__ tets, int64_t nt, const int32_t* __restrict__ facets, const int32_t* __restrict__ nfacets,
                            int64_t nf2, int32_t* __restrict__ nbr, unsigned long long* n_bad, MtState* st) {
    unsigned long long bad = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nf2; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = i >> 1;
        const int32_t c = nfacets[i], other = nfacets[i ^ 1];
        if (c < -1 || c >= nt || other < -1 || other >= nt) { atomicOr(&st->err, MT_BAD_ID); continue; }
        if (c < 0) continue;
        const int32_t f0 = facets[3 * f], f1 = facets[3 * f + 1], f2 = facets[3 * f + 2];
        const int slot = facet_opposite_slot(tets + 4 * (int64_t)c, f0, f1, f2);
        if (slot >= 0) nbr[4 * (int64_t)c + slot] = other;
        else ++bad;
    }
    wave_add_atomic(bad, n_bad);
}

// ---- geometry ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double edge_len(const V3& a, const V3& b) {
    const V3 d = sub(b, a);
    return sqrt(dot(d, d));
}

__global__ void k_cell_geometry(const double* __restrict__ v, int64_t nv, const int32_t* __restrict__ tets, int64_t nt, double* __restrict__ radius,
                                double* __restrict__ vol, double* __restrict__ longest, double* __restrict__ shortest, unsigned long long* n_flat,
                                MtState* st) {
    unsigned long long flat = 0;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < nt; t += (int64_t)gridDim.x * blockDim.x) {
        const int32_t i0 = tets[4 * t], i1 = tets[4 * t + 1], i2 = tets[4 * t + 2], i3 = tets[4 * t + 3];
        if (!tet_ids_ok(i0, i1, i2, i3, nv)) {
            atomicOr(&st->err, MT_BAD_ID);
            radius[t] = vol[t] = longest[t] = shortest[t] = 0.0;
            continue;
        }
        const V3 p0 = load_v3(v, i0), p1 = load_v3(v, i1), p2 = load_v3(v, i2), p3 = load_v3(v, i3);
        const V3 u = sub(p1, p0), w1 = sub(p2, p0), w2 = sub(p3, p0);
        const V3 c_vw = cross(w1, w2), c_wu = cross(w2, u), c_uv = cross(u, w1);
        const double det = dot(u, c_vw), u2 = dot(u, u), v2 = dot(w1, w1), w2n = dot(w2, w2);
        const V3 r{(u2 * c_vw.x + v2 * c_wu.x) + w2n * c_uv.x, (u2 * c_vw.y + v2 * c_wu.y) + w2n * c_uv.y, (u2 * c_vw.z + v2 * c_wu.z) + w2n * c_uv.z};
        flat += det == 0.0;
        radius[t] = det == 0.0 ? (double)INFINITY : sqrt(dot(r, r)) / (2.0 * fabs(det));
        vol[t] = fabs(det) / 6.0;
        const double e[6] = {edge_len(p0, p1), edge_len(p0, p2), edge_len(p0, p3), edge_len(p1, p2), edge_len(p1, p3), edge_len(p2, p3)};
        double hi = e[0], lo = e[0];
#pragma unroll
        for (int j = 1; j < 6; ++j) {
            hi = e[j] > hi ? e[j] : hi;
            lo = e[j] < lo ? e[j] : lo;
        }
        longest[t] = hi;
        shortest[t] = lo;
    }
    wave_add_atomic(flat, n_flat);
}

// ---- incidence -----------------------------------------------------------------------------------------------------------------
__global__ void k_incidence_count(const int32_t* __restrict__ tets, int64_t n4, int64_t nv, int32_t* count, MtState* st) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t a = tets[i];
        if (a < 0 || a >= nv) atomicOr(&st->err, MT_BAD_ID);
        else atomicAdd(count + a, 1);
    }
}

// (after the ids have passed k_incidence_count) entry 4 t + k goes to the next free place of its vertex's row
__global__ void k_incidence_fill(const int32_t* __restrict__ tets, int64_t n4, int32_t* cursor, int32_t* __restrict__ entries) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x)
        entries[atomicAdd(cursor + tets[i], 1)] = (int32_t)i;
}

// ---- rays ----------------------------------------------------------------------------------------------------------------------
// the other three vertices of tet t around slot k, in slot order
__device__ __forceinline__ void other_vertices(const double* __restrict__ v, const int32_t* __restrict__ tets, int64_t t, int k, V3& q0, V3& q1, V3& q2) {
    int32_t i0, i1, i2;
    row_others(tets + 4 * t, k, i0, i1, i2);
    q0 = load_v3(v, i0);
    q1 = load_v3(v, i1);
    q2 = load_v3(v, i2);
}

// the ray length from p to the plane of (q0, q1, q2) along e / |e| (flip = 0) or its negative (flip = 1)
__device__ __forceinline__ double ray_length(const V3& p, const V3& e, int flip, const V3& q0, const V3& q1, const V3& q2) {
    double len, den;
    const V3 d = unit_ray(e, flip, len);
    return plane_distance(p, d, q0, q1, q2, den);
}

__global__ void __launch_bounds__(MESH_THREADS)
k_rays(const double* __restrict__ v, int64_t nv, const int32_t* __restrict__ tets, int64_t nt, const int32_t* __restrict__ rowptr,
       const int32_t* __restrict__ entries, const int32_t* __restrict__ ray_vertex, const double* __restrict__ sensors, int64_t nr, int unique,
       const int32_t* __restrict__ first, int32_t* __restrict__ ray_tet, int32_t* __restrict__ ray_slot, double* __restrict__ ray_dist,
       unsigned long long* stats, MtState* st) {
    unsigned long long cnt[SF_N_STATS] = {0, 0, 0, 0, 0, 0};
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < nr; r += (int64_t)gridDim.x * blockDim.x) {
        int32_t best[SF_SIDES] = {INT32_MAX, INT32_MAX}, best_slot[SF_SIDES] = {-1, -1};
        double dist[SF_SIDES] = {0.0, 0.0};
        const int32_t vid = ray_vertex[r];          // in range: k_ray_first has passed
        const V3 p = load_v3(v, vid), s = load_v3(sensors, r);
        bool live = true;
        if (s.x == p.x && s.y == p.y && s.z == p.z) { ++cnt[SF_DEGENERATE]; live = false; }
        else if (unique && first[vid] != (int32_t)r) { ++cnt[SF_DUPLICATE]; live = false; }
        else if (!orient_coords_ok(p) || !orient_coords_ok(s)) { atomicOr(&st->err, s.x == s.x && s.y == s.y && s.z == s.z ? MT_RANGE : MT_NONFINITE); live = false; }
        if (live) {
            ++cnt[SF_USED];
            int64_t b, e;
            if (corner_row(rowptr, vid, nt, b, e, st))
                for (int64_t i = b; i < e; ++i) {
                    int32_t t;
                    int k;
                    if (!corner_of(tets, nt, entries[i], vid, t, k, st)) continue;
                    V3 q0, q1, q2;
                    other_vertices(v, tets, t, k, q0, q1, q2);
                    if (!orient_coords_ok(q0) || !orient_coords_ok(q1) || !orient_coords_ok(q2)) { atomicOr(&st->err, MT_RANGE); continue; }
                    // det[q0 - p, q1 - p, q2 - p] is the orientation of each facet (p, qa, qb) through p against the remaining vertex, the
                    // facets taken cyclically; the sensor qualifies on a side when it agrees with it (or lies on the plane) on all three
                    int ex[4] = {0, 0, 0, 0};
                    const int d = dgnn_exact::orient_sign(p, q0, q1, q2, &ex[0]);
                    const int a0 = d * dgnn_exact::orient_sign(p, q0, q1, s, &ex[1]);
                    const int a1 = d * dgnn_exact::orient_sign(p, q1, q2, s, &ex[2]);
                    const int a2 = d * dgnn_exact::orient_sign(p, q2, q0, s, &ex[3]);
                    cnt[SF_EXACT] += ex[0] + ex[1] + ex[2] + ex[3];
                    if (d == 0) continue;          // a flat tet holds no ray
                    if (a0 >= 0 && a1 >= 0 && a2 >= 0 && t < best[0]) { best[0] = t; best_slot[0] = k; }
                    if (a0 <= 0 && a1 <= 0 && a2 <= 0 && t < best[1]) { best[1] = t; best_slot[1] = k; }
                }
            const V3 e3 = sub(s, p);
#pragma unroll
            for (int side = 0; side < SF_SIDES; ++side) {
                if (best[side] == INT32_MAX) { ++cnt[side == 0 ? SF_NO_OUTSIDE : SF_NO_INSIDE]; continue; }
                V3 q0, q1, q2;
                other_vertices(v, tets, best[side], best_slot[side], q0, q1, q2);
                dist[side] = ray_length(p, e3, side, q0, q1, q2);
            }
        }
#pragma unroll
        for (int side = 0; side < SF_SIDES; ++side) {
            ray_tet[SF_SIDES * r + side] = best[side] == INT32_MAX ? -1 : best[side];
            ray_slot[SF_SIDES * r + side] = best_slot[side];
            ray_dist[SF_SIDES * r + side] = dist[side];
        }
    }
#pragma unroll
    for (int j = 0; j < SF_N_STATS; ++j) wave_add_atomic(cnt[j], stats + j);
}

// sort keys of one side: the ray's tet, rays without one behind every tet
__global__ void k_ray_keys(const int32_t* __restrict__ ray_tet, int64_t nr, int side, int64_t nt, uint64_t* __restrict__ keys, int32_t* __restrict__ vals) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < nr; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t t = ray_tet[SF_SIDES * r + side];
        keys[r] = t < 0 ? (uint64_t)nt : (uint64_t)t;
        vals[r] = (int32_t)r;
    }
}

// one thread per tet: its run of ray ids (ascending) folded serially.  count [T], stat [3, T] = min, max, sum; the same per slot with T -> 4 T.
__global__ void k_ray_fold(const int32_t* __restrict__ order, const int32_t* __restrict__ run_begin, const int32_t* __restrict__ run_end, int64_t nt,
                           int side, const int32_t* __restrict__ ray_slot, const double* __restrict__ ray_dist, int32_t* __restrict__ tet_count,
                           double* __restrict__ tet_stat, int32_t* __restrict__ slot_count, double* __restrict__ slot_stat) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < nt; t += (int64_t)gridDim.x * blockDim.x) {
        Fold all, s0, s1, s2, s3;
        int32_t n = 0, n0 = 0, n1 = 0, n2 = 0, n3 = 0;
        for (int64_t i = run_begin[t]; i < run_end[t]; ++i) {
            const int64_t r = order[i];
            const int k = ray_slot[SF_SIDES * r + side];
            const double d = ray_dist[SF_SIDES * r + side];
            all.add(n++, d);
            if (k == 0) s0.add(n0++, d);
            else if (k == 1) s1.add(n1++, d);
            else if (k == 2) s2.add(n2++, d);
            else s3.add(n3++, d);
        }
        tet_count[t] = n;
        all.store(tet_stat + t, nt);
        const Fold* const f[4] = {&s0, &s1, &s2, &s3};
        const int32_t fn[4] = {n0, n1, n2, n3};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            slot_count[4 * t + k] = fn[k];
            f[k]->store(slot_stat + 4 * t + k, 4 * nt);
        }
    }
}

// ---- scratch layouts -----------------------------------------------------------------------------------------------------------
// the first 256 bytes of every scratch: the status word, then the counters
struct Head { MtState st; unsigned long long counters[8]; };
static_assert(sizeof(Head) <= 256, "Head must fit the first scratch slot");

struct IncLayout { Head* head; int32_t *count, *cursor, *sums; int64_t bytes; };
IncLayout inc_layout(void* base, int64_t nv) {
    Take t{(char*)base, 256};
    IncLayout L{};
    L.head = (Head*)base;
    L.count = t.take<int32_t>(nv);
    L.cursor = t.take<int32_t>(nv);
    L.sums = t.take<int32_t>(dgnn_cdiv(nv, 2048) + 4);
    L.bytes = t.off;
    return L;
}

struct RayLayout { Head* head; SortBufs S; int32_t *first, *run_begin, *run_end; int64_t bytes; };
RayLayout ray_layout(void* base, int64_t nr, int64_t nt, int64_t nv) {
    Take t{(char*)base, 256};
    RayLayout L{};
    L.head = (Head*)base;
    take_sort(t, nr, L.S);
    L.first = t.take<int32_t>(nv);
    L.run_begin = t.take<int32_t>(nt);
    L.run_end = t.take<int32_t>(nt);
    L.bytes = t.off;
    return L;
}

bool sizes_ok(int64_t nt, int64_t nv) { return nt >= 0 && nv >= 0 && nt < INT32_MAX / 4 && nv < INT32_MAX; }

}  // namespace

// ================================================================================================================================
extern "C" int64_t dgnn_tet_neighbors_scratch_bytes(void) { return 256; }

extern "C" int dgnn_tet_neighbors(const int32_t* tetrahedra, int64_t n_tets, const int32_t* facets, const int32_t* nfacets, int64_t n_facets,
                                  int32_t* neighbors_out, int64_t* n_bad_out, void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(n_tets >= 0 && n_tets < INT32_MAX / 4 && n_facets >= 0 && n_facets < INT32_MAX / 3, DGNN_E_UNSUPPORTED,
                 "tet_neighbors: sizes exceed the int32 indexing");
    DGNN_REQUIRE(scratch && n_bad_out && (n_tets == 0 || (tetrahedra && neighbors_out)) && (n_facets == 0 || (facets && nfacets)), DGNN_E_INVALID,
                 "tet_neighbors: bad args");
    Head* head = (Head*)scratch;
    (void)hipMemsetAsync(head, 0, sizeof(Head), stream);
    if (n_tets > 0) (void)hipMemsetAsync(neighbors_out, 0xff, sizeof(int32_t) * 4 * n_tets, stream);   // -1: the infinite cell
    if (n_facets > 0)
        hipLaunchKernelGGL(k_neighbors, mesh_launch_grid(2 * n_facets), dim3(MESH_THREADS), 0, stream, tetrahedra, n_tets, facets, nfacets, 2 * n_facets,
                           neighbors_out, head->counters, &head->st);
    (void)hipMemcpyAsync(n_bad_out, head->counters, sizeof(int64_t), hipMemcpyDeviceToDevice, stream);
    MtState hs{};
    return mt_read_status(&hs, &head->st, stream, "tet_neighbors");
}

extern "C" int64_t dgnn_cell_geometry_scratch_bytes(int64_t n_tets) {
    if (n_tets < 0) return 0;
    Take t{nullptr, 256};
    t.take<double>(dgnn_cdiv(n_tets, FIXED_SUM_CHUNK) + 1);
    return t.off;
}

extern "C" int dgnn_cell_geometry(const double* vertices, int64_t n_vertices, const int32_t* tetrahedra, int64_t n_tets, double* radius_out,
                                  double* vol_out, double* longest_out, double* shortest_out, double* edge_sums_out, int64_t* n_flat_out, void* scratch,
                                  void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(sizes_ok(n_tets, n_vertices), DGNN_E_UNSUPPORTED, "cell_geometry: sizes exceed the int32 indexing");
    DGNN_REQUIRE(scratch && edge_sums_out && n_flat_out && (n_tets == 0 || (vertices && tetrahedra && radius_out && vol_out && longest_out && shortest_out)),
                 DGNN_E_INVALID, "cell_geometry: bad args");
    Head* head = (Head*)scratch;
    double* part = (double*)((char*)scratch + 256);
    (void)hipMemsetAsync(head, 0, sizeof(Head), stream);
    if (n_tets > 0)
        hipLaunchKernelGGL(k_cell_geometry, mesh_launch_grid(n_tets), dim3(MESH_THREADS), 0, stream, vertices, n_vertices, tetrahedra, n_tets, radius_out, vol_out,
                           longest_out, shortest_out, head->counters, &head->st);
    fixed_sum(longest_out, n_tets, 0, part, edge_sums_out, stream);          // (the stream orders the two uses of part)
    fixed_sum(shortest_out, n_tets, 0, part, edge_sums_out + 1, stream);
    (void)hipMemcpyAsync(n_flat_out, head->counters, sizeof(int64_t), hipMemcpyDeviceToDevice, stream);
    MtState hs{};
    return mt_read_status(&hs, &head->st, stream, "cell_geometry");
}

extern "C" int64_t dgnn_vertex_incidence_scratch_bytes(int64_t n_vertices) { return n_vertices < 0 ? 0 : inc_layout(nullptr, n_vertices).bytes; }

extern "C" int dgnn_vertex_incidence(const int32_t* tetrahedra, int64_t n_tets, int64_t n_vertices, int32_t* rowptr_out, int32_t* entries_out,
                                     void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(sizes_ok(n_tets, n_vertices), DGNN_E_UNSUPPORTED, "vertex_incidence: sizes exceed the int32 indexing");
    DGNN_REQUIRE(scratch && rowptr_out && (n_tets == 0 || (tetrahedra && entries_out)), DGNN_E_INVALID, "vertex_incidence: bad args");
    const IncLayout L = inc_layout(scratch, n_vertices);
    const int64_t n4 = 4 * n_tets;
    (void)hipMemsetAsync(L.head, 0, sizeof(Head), stream);
    if (n_vertices > 0) (void)hipMemsetAsync(L.count, 0, sizeof(int32_t) * n_vertices, stream);
    if (n4 > 0) hipLaunchKernelGGL(k_incidence_count, mesh_launch_grid(n4), dim3(MESH_THREADS), 0, stream, tetrahedra, n4, n_vertices, L.count, &L.head->st);
    MtState hs{};
    int rc = mt_read_status(&hs, &L.head->st, stream, "vertex_incidence");
    if (rc) return rc;
    if ((rc = dgnn_exclusive_scan_i32(L.count, n_vertices, rowptr_out, L.sums, stream))) return rc;
    if (n4 > 0) {
        (void)hipMemcpyAsync(L.cursor, rowptr_out, sizeof(int32_t) * n_vertices, hipMemcpyDeviceToDevice, stream);
        hipLaunchKernelGGL(k_incidence_fill, mesh_launch_grid(n4), dim3(MESH_THREADS), 0, stream, tetrahedra, n4, L.cursor, entries_out);
    }
    return dgnn_check_launch("vertex_incidence");
}

extern "C" int64_t dgnn_vertex_rays_scratch_bytes(int64_t n_rays, int64_t n_tets, int64_t n_vertices) {
    if (n_rays < 0 || n_rays >= SF_MAX_RAYS || !sizes_ok(n_tets, n_vertices)) return 0;
    return ray_layout(nullptr, n_rays, n_tets, n_vertices).bytes;
}

extern "C" int dgnn_vertex_rays(const double* vertices, int64_t n_vertices, const int32_t* tetrahedra, int64_t n_tets, const int32_t* rowptr,
                                const int32_t* entries, const int32_t* ray_vertex, const double* sensors, int64_t n_rays, int unique, int32_t* ray_tet_out,
                                int32_t* ray_slot_out, double* ray_dist_out, int32_t* tet_count_out, double* tet_stat_out, int32_t* slot_count_out,
                                double* slot_stat_out, int64_t* stats_out, void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(n_rays >= 0 && n_rays < SF_MAX_RAYS && sizes_ok(n_tets, n_vertices), DGNN_E_UNSUPPORTED, "vertex_rays: sizes exceed the int32 indexing");
    DGNN_REQUIRE(scratch && stats_out && rowptr && (n_tets == 0 || (vertices && tetrahedra && entries && tet_count_out && tet_stat_out && slot_count_out &&
                                                                     slot_stat_out)) &&
                     (n_rays == 0 || (ray_vertex && sensors && ray_tet_out && ray_slot_out && ray_dist_out)),
                 DGNN_E_INVALID, "vertex_rays: bad args");
    const RayLayout L = ray_layout(scratch, n_rays, n_tets, n_vertices);
    const dim3 block(MESH_THREADS);
    (void)hipMemsetAsync(L.head, 0, sizeof(Head), stream);
    ray_first_preset(L.first, n_vertices, stream);
    if (n_tets > 0) hipLaunchKernelGGL(k_check_ids, mesh_launch_grid(4 * n_tets), block, 0, stream, tetrahedra, 4 * n_tets, n_vertices, &L.head->st.err, MT_BAD_ID);
    if (n_rays > 0) hipLaunchKernelGGL(k_ray_first, mesh_launch_grid(n_rays), block, 0, stream, ray_vertex, n_rays, n_vertices, unique, L.first, &L.head->st.err);
    MtState hs{};
    int rc = mt_read_status(&hs, &L.head->st, stream, "vertex_rays");
    if (rc) return rc;
    if (n_rays > 0)
        hipLaunchKernelGGL(k_rays, mesh_launch_grid(n_rays), block, 0, stream, vertices, n_vertices, tetrahedra, n_tets, rowptr, entries, ray_vertex, sensors, n_rays,
                           unique, L.first, ray_tet_out, ray_slot_out, ray_dist_out, L.head->counters, &L.head->st);
    for (int side = 0; side < SF_SIDES && n_tets > 0; ++side) {
        int cur = 0;
        if (n_rays > 0) {
            hipLaunchKernelGGL(k_ray_keys, mesh_launch_grid(n_rays), block, 0, stream, ray_tet_out, n_rays, side, n_tets, L.S.keys[0], L.S.vals[0]);
            if ((rc = sort_pairs(L.S, n_rays, key_bits(n_tets + 1), stream, &cur))) return rc;
        }
        (void)hipMemsetAsync(L.run_begin, 0, sizeof(int32_t) * n_tets, stream);          // a tet without rays: an empty run
        (void)hipMemsetAsync(L.run_end, 0, sizeof(int32_t) * n_tets, stream);
        if (n_rays > 0) hipLaunchKernelGGL(k_ray_runs, mesh_launch_grid(n_rays), block, 0, stream, L.S.keys[cur], n_rays, n_tets, L.run_begin, L.run_end);
        hipLaunchKernelGGL(k_ray_fold, mesh_launch_grid(n_tets), block, 0, stream, L.S.vals[cur], L.run_begin, L.run_end, n_tets, side, ray_slot_out, ray_dist_out,
                           tet_count_out + side * n_tets, tet_stat_out + side * 3 * n_tets, slot_count_out + side * 4 * n_tets,
                           slot_stat_out + side * 12 * n_tets);
    }
    (void)hipMemcpyAsync(stats_out, L.head->counters, sizeof(int64_t) * SF_N_STATS, hipMemcpyDeviceToDevice, stream);
    return mt_read_status(&hs, &L.head->st, stream, "vertex_rays");
}
