// The facet-ray walk: every sensor ray followed through ALL the cells it crosses, towards the sensor and behind the surface point, and the
// aggregates of what it meets (`_cbff`, `_fbff`).  DESIGN §29; the rule is in include/dgnn_hip.h, operation by operation.  Every sign is exact
// (exact_orient.h), every distance plain fp64 with each operation rounding on its own (-ffp-contract=off).
//
//   start    one thread per ray scans the tets incident to its vertex through the prologue of tet_rays.h, which k_rays of scenefeat.hip
//            runs too, here with the perturbed side test sigma; per side the lowest qualifying tet (a minimum over a set: the row order of the incidence does not matter), its slot and the three
//            edge signs of its exit facet.
//   walk     one lane per (ray, side).  A step is a chain of two dependent gathers: the tet row and the neighbour row of the new cell are
//            read together (both addresses follow from the cell id, 16 bytes each), then the one apex vertex.  Three new signs decide the exit;
//            the entry facet's three carry over.  The filter of orient_sign is inline, its exact stage and the axis terms of the perturbation
//            are out of line (the exact stage holds a 97-double expansion in scratch memory, as in k_rays and raycast.hip).  The lanes run in
//            ray order: rays of one scan come in the order of its points, and no result depends on the order.
//   stream   the walk runs twice.  The first pass counts the records of every lane and decides status and stats; the host cuts the lanes
//            into ascending chunks of at most max_records records (64-bit sums: no int32 limit on rays x crossings); per chunk an
//            exclusive scan places every lane, the second pass repeats the walk and writes its records, and the records are sorted stably
//            by (side, cell) with the radix sort of reorder.hip.
//   fold     one thread per (side, cell) folds its run serially, for the cell and for each of its four slots, continuing from the values the
//            earlier chunks left in the outputs: ascending (ray, step) whatever max_records is.  No floating-point atomics.
// Every device loop is capped (the scan by the incidence row, the walk by n_tets steps); trouble goes to the status word.
#include <chrono>

#include "tet_rays.h"

namespace {

enum { RW_NONE = 0, RW_SENSOR, RW_HULL, RW_DEPTH, RW_STUCK, RW_CAPPED, RW_N_STATUS };
enum { RW_USED = 0, RW_SKIPPED, RW_PERTURBED, RW_EXACT, RW_DEGENERATE, RW_STATUS0, RW_RECORDS = RW_STATUS0 + RW_N_STATUS, RW_LONGEST, RW_N_STATS };
static_assert(RW_N_STATS == 13, "the layout of stats_out in include/dgnn_hip.h");
constexpr int64_t RW_MAX_RAYS = (int64_t)1 << 30;          // 2 n_rays lanes in int32
static_assert(RW_MAX_RAYS <= RAY_FIRST_NONE, "the preset of first[] has to lie above every ray index");

struct RwHead { MtState st; unsigned long long counters[RW_N_STATS]; };
static_assert(sizeof(RwHead) <= 256, "RwHead must fit the first scratch slot");

// ---- the side test -----------------------------------------------------------------------------------------------------------------
// a representable coordinate above x (|x| <= 2^300, so 2 x <= 2^301 and every triple product of the exact stage stays below 2^902)
__device__ __forceinline__ double axis_up(double x) { return x < 0.0 ? 0.0 : (x == 0.0 ? 1.0 : 2.0 * x); }

// the axis terms of sigma: det[e_a, u - p, v - p] for a = x, y, z as the orientation of (p, p moved up its axis a, u, v); the first non-zero
__device__ __noinline__ int sigma_axes(V3 p, V3 u, V3 v, int* exact) {
    for (int a = 0; a < 3; ++a) {
        const V3 m{a == 0 ? axis_up(p.x) : p.x, a == 1 ? axis_up(p.y) : p.y, a == 2 ? axis_up(p.z) : p.z};
        int ex = 0;
        const int g = dgnn_exact::orient_sign(p, m, u, v, &ex);
        *exact += ex;
        if (g) return g;
    }
    return 0;
}

// sigma(u, v) = sign det[s' - p, u - p, v - p] with s' = s + (eps, eps^2, eps^3): 0 only when p, u, v are collinear
__device__ __forceinline__ int sigma(const V3& p, const V3& s, const V3& u, const V3& v, int& exact, int& perturbed) {
    int ex = 0;
    const int g = dgnn_exact::orient_sign(p, s, u, v, &ex);
    exact += ex;
    if (g) return g;
    perturbed = 1;
    return sigma_axes(p, u, v, &exact);
}

// the common sign of the three edge signs of a facet, 0 when the ray does not cross it
__device__ __forceinline__ int crossing(int x, int y, int z) {
    const bool any = (x | y | z) != 0;
    if (any && x >= 0 && y >= 0 && z >= 0) return 1;
    if (any && x <= 0 && y <= 0 && z <= 0) return -1;
    return 0;
}

__device__ __forceinline__ int32_t pack_start(int k, int s0, int s1, int s2) { return k | ((s0 + 1) << 2) | ((s1 + 1) << 4) | ((s2 + 1) << 6); }

// ---- checks ------------------------------------------------------------------------------------------------------------------------
__global__ void k_walk_check_neighbors(const int32_t* __restrict__ nbr, int64_t n4, int64_t nt, int32_t* err) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x)
        if (nbr[i] < -1 || nbr[i] >= nt) atomicOr(err, MT_BAD_ID);
}

__global__ void k_walk_check_coords(const double* __restrict__ x, int64_t n3, int32_t* err) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n3; i += (int64_t)gridDim.x * blockDim.x) {
        const dgnn_exact::CoordClass k = dgnn_exact::coord_class(x[i]);
        if (k != dgnn_exact::COORD_FINE) atomicOr(err, k == dgnn_exact::COORD_NONFINITE ? MT_NONFINITE : MT_RANGE);
    }
}

// ---- the start cells ---------------------------------------------------------------------------------------------------------------
// (ids and coordinates have passed the checks) start_tet [R, 2] (-1 = none), start_info [R, 2] = pack_start(slot, the facet's edge signs)
__global__ void __launch_bounds__(MESH_THREADS)
k_walk_start(const double* __restrict__ v, const int32_t* __restrict__ tets, int64_t nt, const int32_t* __restrict__ rowptr,
             const int32_t* __restrict__ entries, const int32_t* __restrict__ ray_vertex, const double* __restrict__ sensors, int64_t nr, int unique,
             const int32_t* __restrict__ first, int32_t* __restrict__ start_tet, int32_t* __restrict__ start_info, int32_t* __restrict__ pert,
             unsigned long long* counters, MtState* st) {
    unsigned long long n_used = 0, n_skipped = 0, n_exact = 0;
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < nr; r += (int64_t)gridDim.x * blockDim.x) {
        int32_t best[2] = {INT32_MAX, INT32_MAX}, info[2] = {0, 0};
        int exact = 0, perturbed = 0;
        const int32_t vid = ray_vertex[r];
        const V3 p = load_v3(v, vid), s = load_v3(sensors, r);
        if ((s.x == p.x && s.y == p.y && s.z == p.z) || (unique && first[vid] != (int32_t)r)) ++n_skipped;
        else {
            ++n_used;
            int64_t b, e;
            if (corner_row(rowptr, vid, nt, b, e, st))
                for (int64_t i = b; i < e; ++i) {
                    int32_t t;
                    int k;
                    if (!corner_of(tets, nt, entries[i], vid, t, k, st)) continue;
                    int32_t i0, i1, i2;
                    row_others(load_row(tets, t), k, i0, i1, i2);
                    const V3 q0 = load_v3(v, i0), q1 = load_v3(v, i1), q2 = load_v3(v, i2);
                    int ex = 0;
                    const int d = dgnn_exact::orient_sign(p, q0, q1, q2, &ex);
                    exact += ex;
                    const int s0 = sigma(p, s, q0, q1, exact, perturbed), s1 = sigma(p, s, q1, q2, exact, perturbed), s2 = sigma(p, s, q2, q0, exact, perturbed);
                    const int c = crossing(s0, s1, s2);
                    if (d == 0 || c == 0) continue;          // a flat tet starts no walk
                    const int side = c == d ? 0 : 1;          // forwards with the tet's sign, backwards against it
                    if (t < best[side]) { best[side] = t; info[side] = pack_start(k, s0, s1, s2); }
                }
        }
        n_exact += exact;
        pert[r] = perturbed;
        for (int side = 0; side < 2; ++side) {
            start_tet[2 * r + side] = best[side] == INT32_MAX ? -1 : best[side];
            start_info[2 * r + side] = info[side];
        }
    }
    wave_add_atomic(n_used, counters + RW_USED);
    wave_add_atomic(n_skipped, counters + RW_SKIPPED);
    wave_add_atomic(n_exact, counters + RW_EXACT);
}

// ---- the walk ----------------------------------------------------------------------------------------------------------------------
struct WalkIn {
    const double* v;
    const int32_t *tets, *nbr;
    int64_t nt;
    const int32_t* ray_vertex;
    const double* sensors;
    const int32_t *start_tet, *start_info;
    int64_t lane0, lane1;          // the lanes of this launch
    int32_t depth[2];
};
struct WalkRec {          // the chunk's record stream (fill pass)
    const int32_t* offs;          // [lane1 - lane0 + 1]
    int64_t cap;
    int32_t *lane, *cell, *slot;
    double *first, *second;
};

__device__ __forceinline__ V3 pick(int32_t id, int32_t f0, int32_t f1, const V3& P0, const V3& P1, const V3& P2) {
    return id == f0 ? P0 : (id == f1 ? P1 : P2);
}

// FILL = false: counts the records of every lane, writes ray_cells / ray_status, adds to the counters and to pert[].
// FILL = true: the same walk again, writing record i of lane l to offs[l - lane0] + i; ray_cells holds the counts of the first pass.
template <bool FILL>
__global__ void __launch_bounds__(MESH_THREADS)
k_walk(WalkIn in, WalkRec rec, int32_t* __restrict__ ray_cells, int32_t* __restrict__ ray_status, int32_t* __restrict__ pert,
       unsigned long long* counters, MtState* st) {
    unsigned long long n_exact = 0, n_degenerate = 0;
    for (int64_t lane = in.lane0 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; lane < in.lane1; lane += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = lane >> 1;
        const int side = (int)(lane & 1);
        int32_t c = in.start_tet[lane];
        int status = RW_NONE, n_cells = 0, exact = 0, perturbed = 0;
        if (c >= 0) {
            const int32_t info = in.start_info[lane];
            int k = info & 3, sg0 = ((info >> 2) & 3) - 1, sg1 = ((info >> 4) & 3) - 1, sg2 = ((info >> 6) & 3) - 1;
            const V3 p = load_v3(in.v, in.ray_vertex[r]), s = load_v3(in.sensors, r);
            double len;
            const V3 d = unit_ray(sub(s, p), side, len);
            const int32_t depth = in.depth[side];
            const int32_t expect = FILL ? ray_cells[lane] : 0;
            const int64_t base = FILL ? rec.offs[lane - in.lane0] : 0;
            int4 row = load_row(in.tets, c), nrow = load_row(in.nbr, c);
            int32_t f0, f1, f2;          // the exit facet, with sg0 = sigma(f0, f1), sg1 = sigma(f1, f2), sg2 = sigma(f2, f0)
            row_others(row, k, f0, f1, f2);
            V3 P0 = load_v3(in.v, f0), P1 = load_v3(in.v, f1), P2 = load_v3(in.v, f2);
            double prev = 0.0, first = 0.0;
            bool recorded = false;          // the start cell is the vertex family's: not recorded
            auto put = [&](int32_t slot, double second) {
                if (FILL) {
                    const int64_t i = base + n_cells;
                    if (n_cells < expect && i < rec.cap) {
                        rec.lane[i] = (int32_t)lane;
                        rec.cell[i] = c;
                        rec.slot[i] = slot;
                        rec.first[i] = first;
                        rec.second[i] = second;
                    } else atomicOr(&st->err, MT_PASSES);          // the two passes disagree
                }
                ++n_cells;
            };
            for (int64_t steps = 0;;) {
                if (side == 0) {          // the sensor's cell: s is not strictly beyond the exit facet
                    int ex = 0;
                    const int g = dgnn_exact::orient_sign(P0, P1, P2, s, &ex);
                    exact += ex;
                    if (g != crossing(sg0, sg1, sg2)) {
                        if (recorded) put(-1, len);
                        status = RW_SENSOR;
                        break;
                    }
                }
                {          // the distance to the exit facet, its vertices in the slot order of the cell the ray leaves
                    int32_t i0, i1, i2;
                    row_others(row, k, i0, i1, i2);
                    const V3 q0 = pick(i0, f0, f1, P0, P1, P2), q1 = pick(i1, f0, f1, P0, P1, P2), q2 = pick(i2, f0, f1, P0, P1, P2);
                    double den;
                    double dist = plane_distance(p, d, q0, q1, q2, den);
                    if (den == 0.0 || !dgnn_exact::coord_finite(dist)) { dist = prev; ++n_degenerate; }
                    prev = dist;
                }
                if (recorded) {
                    put(k, prev);
                    if (depth && n_cells == depth) { status = RW_DEPTH; break; }
                }
                const int32_t nxt = row_at(nrow, k);
                if (nxt < 0) { status = RW_HULL; break; }
                if (++steps > in.nt) { status = RW_CAPPED; break; }
                row = load_row(in.tets, nxt);
                nrow = load_row(in.nbr, nxt);
                const int apex = facet_opposite_slot(row, f0, f1, f2);
                if (apex < 0) { atomicOr(&st->err, MT_NOT_FACE); status = RW_STUCK; break; }   // not the cell across the facet
                const int32_t w = row_at(row, apex);
                const V3 W = load_v3(in.v, w);
                const int a0 = sigma(p, s, W, P0, exact, perturbed), a1 = sigma(p, s, W, P1, exact, perturbed), a2 = sigma(p, s, W, P2, exact, perturbed);
                // the facet opposite f_m is (w, f_m+1, f_m+2) with the signs (a_m+1, sg_m+1, -a_m+2)
                const int c0 = crossing(a1, sg1, -a2), c1 = crossing(a2, sg2, -a0), c2 = crossing(a0, sg0, -a1);
                if ((c0 != 0) + (c1 != 0) + (c2 != 0) != 1) { status = RW_STUCK; break; }
                int32_t out;          // the vertex the ray leaves behind; its slot is the exit slot
                if (c0) { out = f0; sg0 = a1; sg2 = -a2; /* sg1 stays */ f0 = w; P0 = W; }
                else if (c1) { out = f1; const int t1 = sg2; sg0 = a2; sg2 = -a0; sg1 = t1; const int32_t g0 = f0; const V3 G0 = P0; f0 = w; f1 = f2; f2 = g0; P0 = W; P1 = P2; P2 = G0; }
                else { out = f2; const int t1 = sg0; sg0 = a0; sg2 = -a1; sg1 = t1; const int32_t g0 = f0; const V3 G0 = P0; f2 = f1; f1 = g0; f0 = w; P2 = P1; P1 = G0; P0 = W; }
                c = nxt;
                k = row.x == out ? 0 : (row.y == out ? 1 : (row.z == out ? 2 : 3));
                first = prev;
                recorded = true;
            }
        }
        if (!FILL) {
            ray_cells[lane] = n_cells;
            ray_status[lane] = status;
            if (perturbed) atomicOr(pert + r, 1);
            n_exact += exact;
        } else if (c >= 0 && n_cells != ray_cells[lane]) atomicOr(&st->err, MT_PASSES);
    }
    if (!FILL) {
        wave_add_atomic(n_exact, counters + RW_EXACT);
        wave_add_atomic(n_degenerate, counters + RW_DEGENERATE);
    }
}

__global__ void k_walk_stats(const int32_t* __restrict__ ray_status, const int32_t* __restrict__ pert, int64_t nr, unsigned long long* counters) {
    unsigned long long n[RW_N_STATUS] = {0, 0, 0, 0, 0, 0}, np = 0;
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < nr; r += (int64_t)gridDim.x * blockDim.x) {
        np += pert[r] != 0;
        for (int side = 0; side < 2; ++side) {
            const int32_t s = ray_status[2 * r + side];
#pragma unroll
            for (int j = 0; j < RW_N_STATUS; ++j) n[j] += s == j;
        }
    }
    wave_add_atomic(np, counters + RW_PERTURBED);
#pragma unroll
    for (int j = 0; j < RW_N_STATUS; ++j) wave_add_atomic(n[j], counters + RW_STATUS0 + j);
}

// ---- sort and fold -----------------------------------------------------------------------------------------------------------------
__global__ void k_walk_keys(const int32_t* __restrict__ lane, const int32_t* __restrict__ cell, int64_t n, int64_t nt, uint64_t* __restrict__ keys,
                            int32_t* __restrict__ vals) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        keys[i] = (uint64_t)(lane[i] & 1) * (uint64_t)nt + (uint64_t)cell[i];
        vals[i] = (int32_t)i;
    }
}

// one thread per (side, cell): its run of records, ascending (ray, step), folded serially onto what the earlier chunks left.
// cell_count [2, T], cell_stat [2, 6, T] = first min / max / sum, second min / max / sum; slot_count [2, T, 4], slot_stat [2, 3, T, 4].
__global__ void k_walk_fold(const int32_t* __restrict__ order, const int32_t* __restrict__ run_begin, const int32_t* __restrict__ run_end, int64_t nt,
                            const int32_t* __restrict__ rec_slot, const double* __restrict__ rec_first, const double* __restrict__ rec_second,
                            int32_t* __restrict__ cell_count, double* __restrict__ cell_stat, int32_t* __restrict__ slot_count,
                            double* __restrict__ slot_stat) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < 2 * nt; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = run_begin[i], e = run_end[i];
        if (b >= e) continue;
        const int64_t side = i >= nt, t = i - side * nt;
        double* const cs = cell_stat + side * 6 * nt + t;
        double* const ss = slot_stat + side * 12 * nt + 4 * t;
        int32_t n = cell_count[i], n0 = slot_count[4 * i], n1 = slot_count[4 * i + 1], n2 = slot_count[4 * i + 2], n3 = slot_count[4 * i + 3];
        Fold fa, fb, s0, s1, s2, s3;
        fa.load(cs, nt);
        fb.load(cs + 3 * nt, nt);
        s0.load(ss, 4 * nt);
        s1.load(ss + 1, 4 * nt);
        s2.load(ss + 2, 4 * nt);
        s3.load(ss + 3, 4 * nt);
        for (int64_t j = b; j < e; ++j) {
            const int64_t q = order[j];
            const int k = rec_slot[q];
            const double d1 = rec_first[q], d2 = rec_second[q];
            fa.add(n, d1);
            fb.add(n, d2);
            ++n;
            if (k == 0) s0.add(n0++, d2);
            else if (k == 1) s1.add(n1++, d2);
            else if (k == 2) s2.add(n2++, d2);
            else if (k == 3) s3.add(n3++, d2);
        }
        cell_count[i] = n;
        slot_count[4 * i] = n0;
        slot_count[4 * i + 1] = n1;
        slot_count[4 * i + 2] = n2;
        slot_count[4 * i + 3] = n3;
        fa.store(cs, nt);
        fb.store(cs + 3 * nt, nt);
        s0.store(ss, 4 * nt);
        s1.store(ss + 1, 4 * nt);
        s2.store(ss + 2, 4 * nt);
        s3.store(ss + 3, 4 * nt);
    }
}

// the chunk's records into the caller's stream at `at`: ids [5, cap] = ray, side, step, cell, slot; dist [2, cap] = first, second
__global__ void k_walk_copy_records(const int32_t* __restrict__ lane, const int32_t* __restrict__ cell, const int32_t* __restrict__ slot,
                                    const double* __restrict__ first, const double* __restrict__ second, const int32_t* __restrict__ offs, int64_t lane0,
                                    int64_t n, int64_t at, int64_t cap, int32_t* __restrict__ ids, double* __restrict__ dist) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t o = at + i;
        if (o >= cap) continue;
        const int32_t l = lane[i];
        ids[o] = l >> 1;
        ids[cap + o] = l & 1;
        ids[2 * cap + o] = (int32_t)(i - offs[l - lane0]);
        ids[3 * cap + o] = cell[i];
        ids[4 * cap + o] = slot[i];
        dist[o] = first[i];
        dist[cap + o] = second[i];
    }
}

// ---- scratch -----------------------------------------------------------------------------------------------------------------------
struct WalkLayout {
    RwHead* head;
    int32_t *first, *start_tet, *start_info, *pert, *offs, *scan_sums, *run_begin, *run_end;
    int32_t *rec_lane, *rec_cell, *rec_slot;
    double *rec_first, *rec_second;
    SortBufs S;
    int64_t bytes;
};
WalkLayout walk_layout(void* base, int64_t nr, int64_t nt, int64_t nv, int64_t m) {
    Take t{(char*)base, 256};
    WalkLayout L{};
    L.head = (RwHead*)base;
    L.first = t.take<int32_t>(nv);
    L.start_tet = t.take<int32_t>(2 * nr);
    L.start_info = t.take<int32_t>(2 * nr);
    L.pert = t.take<int32_t>(nr);
    L.offs = t.take<int32_t>(2 * nr + 1);
    L.scan_sums = t.take<int32_t>(dgnn_cdiv(2 * nr, 2048) + 4);
    L.run_begin = t.take<int32_t>(2 * nt);
    L.run_end = t.take<int32_t>(2 * nt);
    L.rec_lane = t.take<int32_t>(m);
    L.rec_cell = t.take<int32_t>(m);
    L.rec_slot = t.take<int32_t>(m);
    L.rec_first = t.take<double>(m);
    L.rec_second = t.take<double>(m);
    take_sort(t, m, L.S);
    L.bytes = t.off;
    return L;
}

// Stage times for tools/bench_ray_walk.py.  Off by default; when on, dgnn_ray_walk synchronises the stream at every stage boundary (so the
// call as a whole is slower) and adds the host time of each stage: 0 checks, start cells and the counting walk, 1 the filling walk with
// its scan, 2 keys and sort, 3 runs and fold.
bool g_walk_timing = false;
double g_walk_ms[4] = {0, 0, 0, 0};
struct StageClock {
    hipStream_t stream;
    std::chrono::steady_clock::time_point t0;
    explicit StageClock(hipStream_t s) : stream(s) {
        if (g_walk_timing) { (void)hipStreamSynchronize(stream); t0 = std::chrono::steady_clock::now(); }
    }
    void lap(int stage) {
        if (!g_walk_timing) return;
        (void)hipStreamSynchronize(stream);
        const auto t1 = std::chrono::steady_clock::now();
        g_walk_ms[stage] += std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
    }
};

bool walk_sizes_ok(int64_t nr, int64_t nt, int64_t nv, int64_t m) {
    return nr >= 0 && nr < RW_MAX_RAYS && nt >= 0 && nt < INT32_MAX / 8 && nv >= 0 && nv < INT32_MAX && m >= 1 && m < INT32_MAX / 2;
}

}  // namespace

// ================================================================================================================================
extern "C" int dgnn_ray_walk_timing(int on, double* stage_ms_out) {
    if (stage_ms_out) memcpy(stage_ms_out, g_walk_ms, sizeof(g_walk_ms));
    memset(g_walk_ms, 0, sizeof(g_walk_ms));
    g_walk_timing = on != 0;
    return DGNN_OK;
}

extern "C" int64_t dgnn_ray_walk_scratch_bytes(int64_t n_rays, int64_t n_tets, int64_t n_vertices, int64_t max_records) {
    if (!walk_sizes_ok(n_rays, n_tets, n_vertices, max_records)) return 0;
    return walk_layout(nullptr, n_rays, n_tets, n_vertices, max_records).bytes;
}

extern "C" int dgnn_ray_walk(const double* vertices, int64_t n_vertices, const int32_t* tetrahedra, int64_t n_tets, const int32_t* neighbors,
                             const int32_t* rowptr, const int32_t* entries, const int32_t* ray_vertex, const double* sensors, int64_t n_rays, int unique,
                             int64_t outside_depth, int64_t inside_depth, int64_t max_records, int32_t* ray_status_out, int32_t* ray_cells_out,
                             int32_t* cell_count_out, double* cell_stat_out, int32_t* slot_count_out, double* slot_stat_out, int64_t* stats_out,
                             int64_t records_capacity, int32_t* record_ids_out, double* record_dist_out, void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(walk_sizes_ok(n_rays, n_tets, n_vertices, max_records), DGNN_E_UNSUPPORTED,
                 "ray_walk: sizes exceed the int32 indexing (rays < 2^30, 8 n_tets and 2 max_records within int32, max_records >= 1)");
    DGNN_REQUIRE(outside_depth >= 0 && inside_depth >= 0 && outside_depth < INT32_MAX && inside_depth < INT32_MAX && records_capacity >= 0, DGNN_E_INVALID,
                 "ray_walk: a negative depth or capacity");
    DGNN_REQUIRE(scratch && stats_out && rowptr &&
                     (n_tets == 0 || (vertices && tetrahedra && neighbors && entries && cell_count_out && cell_stat_out && slot_count_out && slot_stat_out)) &&
                     (n_rays == 0 || (ray_vertex && sensors && ray_status_out && ray_cells_out)) &&
                     (records_capacity == 0 || (record_ids_out && record_dist_out)),
                 DGNN_E_INVALID, "ray_walk: bad args");
    DGNN_REQUIRE(((uintptr_t)tetrahedra % 16) == 0 && ((uintptr_t)neighbors % 16) == 0, DGNN_E_INVALID, "ray_walk: tetrahedra and neighbors must be 16-byte aligned");
    const WalkLayout L = walk_layout(scratch, n_rays, n_tets, n_vertices, max_records);
    const dim3 block(MESH_THREADS);
    const int64_t n_lanes = 2 * n_rays;
    int32_t* const err = &L.head->st.err;
    StageClock clock(stream);
    (void)hipMemsetAsync(L.head, 0, sizeof(RwHead), stream);
    ray_first_preset(L.first, n_vertices, stream);
    if (n_tets > 0) {
        (void)hipMemsetAsync(cell_count_out, 0, sizeof(int32_t) * 2 * n_tets, stream);
        (void)hipMemsetAsync(cell_stat_out, 0, sizeof(double) * 12 * n_tets, stream);
        (void)hipMemsetAsync(slot_count_out, 0, sizeof(int32_t) * 8 * n_tets, stream);
        (void)hipMemsetAsync(slot_stat_out, 0, sizeof(double) * 24 * n_tets, stream);
        hipLaunchKernelGGL(k_check_ids, mesh_launch_grid(4 * n_tets), block, 0, stream, tetrahedra, 4 * n_tets, n_vertices, err, MT_BAD_ID);
        hipLaunchKernelGGL(k_walk_check_neighbors, mesh_launch_grid(4 * n_tets), block, 0, stream, neighbors, 4 * n_tets, n_tets, err);
    }
    if (n_vertices > 0) hipLaunchKernelGGL(k_walk_check_coords, mesh_launch_grid(3 * n_vertices), block, 0, stream, vertices, 3 * n_vertices, err);
    if (n_rays > 0) {
        hipLaunchKernelGGL(k_walk_check_coords, mesh_launch_grid(3 * n_rays), block, 0, stream, sensors, 3 * n_rays, err);
        hipLaunchKernelGGL(k_ray_first, mesh_launch_grid(n_rays), block, 0, stream, ray_vertex, n_rays, n_vertices, unique, L.first, err);
    }
    MtState hs{};
    int rc = mt_read_status(&hs, &L.head->st, stream, "ray_walk");
    if (rc) return rc;

    int64_t stats[RW_N_STATS] = {0};
    int32_t* counts = nullptr;          // host copy of ray_cells_out
    if (n_rays > 0) {
        WalkIn in{vertices, tetrahedra, neighbors, n_tets, ray_vertex, sensors, L.start_tet, L.start_info, 0, n_lanes, {(int32_t)outside_depth, (int32_t)inside_depth}};
        hipLaunchKernelGGL(k_walk_start, mesh_launch_grid(n_rays), block, 0, stream, vertices, tetrahedra, n_tets, rowptr, entries, ray_vertex, sensors, n_rays,
                           unique, L.first, L.start_tet, L.start_info, L.pert, L.head->counters, &L.head->st);
        hipLaunchKernelGGL((k_walk<false>), mesh_launch_grid(n_lanes), block, 0, stream, in, WalkRec{}, ray_cells_out, ray_status_out, L.pert, L.head->counters,
                           &L.head->st);
        hipLaunchKernelGGL(k_walk_stats, mesh_launch_grid(n_rays), block, 0, stream, ray_status_out, L.pert, n_rays, L.head->counters);
        if ((rc = mt_read_status(&hs, &L.head->st, stream, "ray_walk"))) return rc;
        counts = (int32_t*)malloc(sizeof(int32_t) * n_lanes);
        DGNN_REQUIRE(counts, DGNN_E_INVALID, "ray_walk: no host memory for %lld counts", (long long)n_lanes);
        if ((rc = mm_read(counts, ray_cells_out, sizeof(int32_t) * n_lanes, stream, "ray_walk")) ||
            (rc = mm_read(stats, L.head->counters, sizeof(int64_t) * RW_N_STATS, stream, "ray_walk"))) {
            free(counts);
            return rc;
        }
        for (int64_t l = 0; l < n_lanes; ++l) {
            stats[RW_RECORDS] += counts[l];
            if (counts[l] > stats[RW_LONGEST]) stats[RW_LONGEST] = counts[l];
        }
    }
    if (hipMemcpyAsync(stats_out, stats, sizeof(stats), hipMemcpyHostToDevice, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
        free(counts);
        dgnn_set_error("ray_walk: %s", hipGetErrorString(hipGetLastError()));
        return DGNN_E_LAUNCH;
    }
    if (stats[RW_LONGEST] > max_records || (records_capacity > 0 && records_capacity < stats[RW_RECORDS])) {
        free(counts);
        dgnn_set_error("ray_walk: the longest walk has %lld records and all walks %lld; max_records is %lld and the record capacity %lld",
                       (long long)stats[RW_LONGEST], (long long)stats[RW_RECORDS], (long long)max_records, (long long)records_capacity);
        return DGNN_E_UNSUPPORTED;
    }

    clock.lap(0);
    // ascending chunks of lanes whose records fit max_records
    int64_t at = 0;          // records before this chunk
    for (int64_t l0 = 0; l0 < n_lanes && n_tets > 0;) {
        int64_t l1 = l0, m = 0;
        while (l1 < n_lanes && m + counts[l1] <= max_records) m += counts[l1++];
        if (m > 0) {
            WalkIn in{vertices, tetrahedra, neighbors, n_tets, ray_vertex, sensors, L.start_tet, L.start_info, l0, l1, {(int32_t)outside_depth, (int32_t)inside_depth}};
            const WalkRec rec{L.offs, m, L.rec_lane, L.rec_cell, L.rec_slot, L.rec_first, L.rec_second};
            int cur = 0;
            if ((rc = dgnn_exclusive_scan_i32(ray_cells_out + l0, l1 - l0, L.offs, L.scan_sums, stream))) break;
            hipLaunchKernelGGL((k_walk<true>), mesh_launch_grid(l1 - l0), block, 0, stream, in, rec, ray_cells_out, ray_status_out, L.pert, L.head->counters, &L.head->st);
            clock.lap(1);
            hipLaunchKernelGGL(k_walk_keys, mesh_launch_grid(m), block, 0, stream, L.rec_lane, L.rec_cell, m, n_tets, L.S.keys[0], L.S.vals[0]);
            if ((rc = sort_pairs(L.S, m, key_bits(2 * n_tets + 1), stream, &cur))) break;
            clock.lap(2);
            (void)hipMemsetAsync(L.run_begin, 0, sizeof(int32_t) * 2 * n_tets, stream);          // a cell without records: an empty run
            (void)hipMemsetAsync(L.run_end, 0, sizeof(int32_t) * 2 * n_tets, stream);
            hipLaunchKernelGGL(k_ray_runs, mesh_launch_grid(m), block, 0, stream, L.S.keys[cur], m, 2 * n_tets, L.run_begin, L.run_end);
            hipLaunchKernelGGL(k_walk_fold, mesh_launch_grid(2 * n_tets), block, 0, stream, L.S.vals[cur], L.run_begin, L.run_end, n_tets, L.rec_slot, L.rec_first,
                               L.rec_second, cell_count_out, cell_stat_out, slot_count_out, slot_stat_out);
            if (records_capacity > 0)
                hipLaunchKernelGGL(k_walk_copy_records, mesh_launch_grid(m), block, 0, stream, L.rec_lane, L.rec_cell, L.rec_slot, L.rec_first, L.rec_second, L.offs,
                                   l0, m, at, records_capacity, record_ids_out, record_dist_out);
            clock.lap(3);
            at += m;
        }
        l0 = l1;
    }
    free(counts);
    if (rc) return rc;
    return mt_read_status(&hs, &L.head->st, stream, "ray_walk");
}
