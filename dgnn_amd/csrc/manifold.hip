// Singular vertices of a labelled tetrahedralization and their repair by relabelling cells (`mesh.manifold: repair` of `generate`).
// DESIGN §31; the criterion and the rule are stated operation by operation in include/dgnn_hip.h.  Everything is integer.
//
//   nodes      corner 4 c + k of cell c (vertex v = tetrahedra[c][k]) stands for c in v's star; node 4 T + v for the infinite cell at v.
//   joins      one thread per cell: across each facet to a neighbour with the same label, the three corner pairs of the shared vertices; an
//              outside cell that faces the infinite cell, its three corners on the facet with their vertices' infinite nodes.  The
//              union-find of mesh_faces.h: the larger root is hooked under the smaller by compare-and-swap, parents only decrease, so every
//              retry loop ends and no thread waits for another.
//              A component's root is its smallest corner, 4 (its smallest cell) + slot; the root of an infinite node that was joined is a corner.
//   roots      per corner its root; per root the int64 sum of cost (integer atomic add: order-free), and the OR of `holds a flipped cell`
//              and `holds the infinite node`.
//   select     per vertex over its row of dgnn_vertex_incidence: the roots counted by side, the lone infinite component of a hull vertex
//              added, and per side the root with the smallest (cost, corner) among those that hold neither the infinite node nor a flipped
//              cell -- sums, counts and minima, so the row's order does not matter.  A row of up to a wavefront is walked by one lane; a
//              longer one is put on a list and walked by a whole wavefront in a second launch (a star has no size limit).
//   claim      every corner whose vertex has a move: atomicMin(claim[c], v).  A vertex that finds another id on a cell of its star loses.
//   apply      every corner of a winner whose root is the winner's move flips its cell and marks it.  Winners' stars are disjoint: one
//              writer per cell.
// The host loop reads one small record per round and ends when a round had no move.
#include "mesh_faces.h"
#include "tet_common.h"

namespace {

constexpr int32_t MR_BAD_ID = 1, MR_NEIGHBOR = 2, MR_COST = 4, MR_LABEL = 8, MR_DEGENERATE = 16, MR_LIST = 32;
constexpr int32_t MR_F_FLIPPED = 1, MR_F_INF = 2;
constexpr int MR_LONG_ROW = DGNN_WAVE;   // rows longer than this are walked by a wavefront

struct MrState {
    int32_t err, n_long, pad[2];
    unsigned long long singular, movers;                                        // this round's detection
    unsigned long long moves, to_inside, to_outside, flipped_cost;              // the whole call
};

struct MrBest {
    long long sum;
    int32_t root;   // -1: none
};
__device__ __forceinline__ void best_take(MrBest& b, long long s, int32_t r) {
    if (r >= 0 && (b.root < 0 || s < b.sum || (s == b.sum && r < b.root))) { b.sum = s; b.root = r; }
}

// the input the later kernels read through: neighbour ids in [-1, T), no cell twice its own vertex, every neighbour holding the three
// shared vertices and naming the cell back across them, labels in {0, 1}, cost >= 0.  (The vertex ids have passed k_check_ids.)
__global__ void k_mr_check(const int32_t* __restrict__ tets, const int32_t* __restrict__ nbr, const int32_t* __restrict__ labels,
                           const int32_t* __restrict__ cost, int64_t nt, int32_t* __restrict__ hull, MrState* st) {
    for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < nt; c += (int64_t)gridDim.x * blockDim.x) {
        int32_t err = 0;
        int32_t v[4], n[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[k] = tets[4 * c + k]; n[k] = nbr[4 * c + k]; }
        if (v[0] == v[1] || v[0] == v[2] || v[0] == v[3] || v[1] == v[2] || v[1] == v[3] || v[2] == v[3]) err |= MR_DEGENERATE;
        if (labels[c] != 0 && labels[c] != 1) err |= MR_LABEL;
        if (cost && cost[c] < 0) err |= MR_COST;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (n[j] < -1 || n[j] >= nt) { err |= MR_BAD_ID; continue; }
            if (n[j] < 0) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k != j) hull[v[k]] = 1;   // every writer stores the same value
                continue;
            }
            int32_t f0, f1, f2;   // the facet shared with n[j]: the cell's vertices other than slot j
            row_others(v, j, f0, f1, f2);
            const int back = facet_opposite_slot(tets + 4 * (int64_t)n[j], f0, f1, f2);
            if (n[j] == (int32_t)c || back < 0 || nbr[4 * (int64_t)n[j] + back] != (int32_t)c) err |= MR_NEIGHBOR;
        }
        if (err) atomicOr(&st->err, err);
    }
}

// one launch resets what a round builds: every node its own parent, the sums and flags of the corners, the claims, the lost marks
__global__ void k_mr_reset(int64_t n4, int64_t nv, int32_t* __restrict__ parent, long long* __restrict__ sum, int32_t* __restrict__ flag,
                           int32_t* __restrict__ claim, int32_t* __restrict__ lost) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4 + nv; i += (int64_t)gridDim.x * blockDim.x) {
        parent[i] = (int32_t)i;
        if (i < n4) {
            sum[i] = 0;
            flag[i] = 0;
            if ((i & 3) == 0) claim[i >> 2] = INT32_MAX;
        } else {
            lost[i - n4] = 0;
        }
    }
}

// one thread per cell: its row and its neighbour's are read once (16 bytes each) for the three corner pairs of a shared facet
__global__ void k_mr_join(const int4* __restrict__ tets, const int4* __restrict__ nbr, const int32_t* __restrict__ labels, int64_t nt,
                          int32_t* parent) {
    const int64_t n4 = 4 * nt;
    for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < nt; c += (int64_t)gridDim.x * blockDim.x) {
        const int4 tv = tets[c], tn = nbr[c];
        const int32_t v[4] = {tv.x, tv.y, tv.z, tv.w}, n[4] = {tn.x, tn.y, tn.z, tn.w};
        const int32_t lab = labels[c];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (n[j] < 0) {
                if (lab == 1) {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (k != j) uf_union(parent, (int32_t)(4 * c + k), (int32_t)(n4 + v[k]));
                }
            } else if (n[j] > (int32_t)c && labels[n[j]] == lab) {   // (each pair once, from its lower cell)
                const int4 tw = tets[n[j]];
                const int32_t w[4] = {tw.x, tw.y, tw.z, tw.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (k == j) continue;
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        if (w[s] == v[k]) uf_union(parent, (int32_t)(4 * c + k), 4 * n[j] + s);
                }
            }
        }
    }
}

// (after every join) items [0, 4 T): root[e], the cost and the flipped mark of e's cell into its root; items [4 T, 4 T + V): the vertex's
// infinite node -- its root is flagged, or, when nothing was joined to it at a hull vertex, it is a component of its own (lone[v] = 1)
__global__ void k_mr_roots(const int32_t* __restrict__ cost, const int32_t* __restrict__ flipped, const int32_t* __restrict__ hull, int64_t n4,
                           int64_t nv, int select, int32_t* parent, int32_t* __restrict__ root, long long* __restrict__ sum,
                           int32_t* __restrict__ flag, int32_t* __restrict__ lone) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4 + nv; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t r = uf_find(parent, (int32_t)i);
        if (i < n4) {
            root[i] = r;
            if (select) {
                atomicAdd((unsigned long long*)(sum + r), (unsigned long long)(cost ? cost[i >> 2] : 1));
                if (flipped[i >> 2]) atomicOr(flag + r, MR_F_FLIPPED);
            }
        } else {
            if (r < n4) atomicOr(flag + r, MR_F_INF);
            lone[i - n4] = r >= n4 && hull[i - n4];
        }
    }
}

struct MrRow {
    int32_t a, b;
    MrBest in, out;
};
// entries [begin + first, end) of a row, every `step`-th
__device__ __forceinline__ MrRow row_walk(const int32_t* __restrict__ entries, const int32_t* __restrict__ labels, const int32_t* __restrict__ root,
                                          const long long* __restrict__ sum, const int32_t* __restrict__ flag, int32_t begin, int32_t end, int first,
                                          int step) {
    MrRow w{0, 0, {0, -1}, {0, -1}};
    for (int32_t i = begin + first; i < end; i += step) {
        const int32_t e = entries[i];
        if (root[e] != e) continue;
        const bool outside = labels[e >> 2] == 1;
        w.a += !outside;
        w.b += outside;
        if (flag[e] == 0) best_take(outside ? w.out : w.in, sum[e], e);
    }
    return w;
}

// the row's verdict: a(v), b(v) with the lone infinite component, singular or not, and the move = the candidate with the smallest
// (cost, corner) on the sides that have two components or more
__device__ __forceinline__ void row_verdict(const MrRow& w, int32_t v, int32_t lone, int select, int32_t* __restrict__ n_in, int32_t* __restrict__ n_out,
                                            int32_t* __restrict__ move, unsigned long long& singular, unsigned long long& movers) {
    const int32_t a = w.a, b = w.b + lone;
    n_in[v] = a;
    n_out[v] = b;
    MrBest m{0, -1};
    if (a > 1) best_take(m, w.in.sum, w.in.root);
    if (b > 1) best_take(m, w.out.sum, w.out.root);
    singular += a > 1 || b > 1;
    if (select) {
        move[v] = m.root;
        movers += m.root >= 0;
    }
}

__global__ void k_mr_select(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ entries, const int32_t* __restrict__ labels,
                            const int32_t* __restrict__ root, const long long* __restrict__ sum, const int32_t* __restrict__ flag,
                            const int32_t* __restrict__ lone, int64_t nv, int select, int32_t* __restrict__ n_in, int32_t* __restrict__ n_out,
                            int32_t* __restrict__ move, int32_t* __restrict__ long_list, MrState* st) {
    unsigned long long singular = 0, movers = 0;
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < nv; v += (int64_t)gridDim.x * blockDim.x) {
        const int32_t begin = rowptr[v], end = rowptr[v + 1];
        if (end - begin > MR_LONG_ROW) {
            const int32_t at = atomicAdd(&st->n_long, 1);
            if (at < nv) long_list[at] = (int32_t)v;
            else atomicOr(&st->err, MR_LIST);
            continue;
        }
        row_verdict(row_walk(entries, labels, root, sum, flag, begin, end, 0, 1), (int32_t)v, lone[v], select, n_in, n_out, move, singular, movers);
    }
    wave_add_atomic(singular, &st->singular);   // every lane is here: the loop has ended for all of them
    wave_add_atomic(movers, &st->movers);
}

// one wavefront per listed vertex: the lanes take every 64th entry, the counts are summed and the minima taken over the wavefront
__global__ void __launch_bounds__(MESH_THREADS) k_mr_select_long(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ entries,
                                                                 const int32_t* __restrict__ labels, const int32_t* __restrict__ root,
                                                                 const long long* __restrict__ sum, const int32_t* __restrict__ flag,
                                                                 const int32_t* __restrict__ lone, int64_t nv, int select,
                                                                 int32_t* __restrict__ n_in, int32_t* __restrict__ n_out, int32_t* __restrict__ move,
                                                                 const int32_t* __restrict__ long_list, MrState* st) {
    const int64_t n_long = st->n_long < nv ? st->n_long : nv;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    unsigned long long singular = 0, movers = 0;
    for (int64_t i = wave; i < n_long; i += n_waves) {   // (uniform over the wavefront)
        const int32_t v = long_list[i];
        MrRow w = row_walk(entries, labels, root, sum, flag, rowptr[v], rowptr[v + 1], lane_id(), DGNN_WAVE);
        for (int o = 32; o > 0; o >>= 1) {
            w.a += __shfl_xor(w.a, o);
            w.b += __shfl_xor(w.b, o);
            best_take(w.in, __shfl_xor(w.in.sum, o), __shfl_xor(w.in.root, o));
            best_take(w.out, __shfl_xor(w.out.sum, o), __shfl_xor(w.out.root, o));
        }
        if (lane_id() == 0) row_verdict(w, v, lone[v], select, n_in, n_out, move, singular, movers);
    }
    if (lane_id() == 0) {
        if (singular) atomicAdd(&st->singular, singular);
        if (movers) atomicAdd(&st->movers, movers);
    }
}

__global__ void k_mr_claim(const int32_t* __restrict__ tets, const int32_t* __restrict__ move, int64_t n4, int32_t* claim) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n4; e += (int64_t)gridDim.x * blockDim.x) {
        const int32_t v = tets[e];
        if (move[v] >= 0) atomicMin(claim + (e >> 2), v);
    }
}

__global__ void k_mr_lose(const int32_t* __restrict__ tets, const int32_t* __restrict__ move, const int32_t* __restrict__ claim, int64_t n4,
                          int32_t* __restrict__ lost) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n4; e += (int64_t)gridDim.x * blockDim.x) {
        const int32_t v = tets[e];
        if (move[v] >= 0 && claim[e >> 2] != v) lost[v] = 1;   // every writer stores the same value
    }
}

__global__ void k_mr_apply(const int32_t* __restrict__ tets, const int32_t* __restrict__ move, const int32_t* __restrict__ lost,
                           const int32_t* __restrict__ root, const int32_t* __restrict__ cost, int64_t n4, int32_t* __restrict__ labels,
                           int32_t* __restrict__ flipped, MrState* st) {
    unsigned long long moves = 0, to_in = 0, to_out = 0, fcost = 0;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n4; e += (int64_t)gridDim.x * blockDim.x) {
        const int32_t v = tets[e], m = move[v];
        if (m < 0 || lost[v] || root[e] != m) continue;
        const int64_t c = e >> 2;
        const int32_t lab = labels[c];   // the one writer of cell c: no other winner's star holds it
        labels[c] = lab ^ 1;
        flipped[c] = 1;
        moves += m == (int32_t)e;
        to_in += lab == 1;
        to_out += lab == 0;
        fcost += (unsigned long long)(cost ? cost[c] : 1);
    }
    wave_add_atomic(moves, &st->moves);
    wave_add_atomic(to_in, &st->to_inside);
    wave_add_atomic(to_out, &st->to_outside);
    wave_add_atomic(fcost, &st->flipped_cost);
}

// ---- scratch layout ------------------------------------------------------------------------------------------------------------
struct MrLayout {
    MrState* st;
    int32_t *parent, *root, *flag, *hull, *lone, *move, *lost, *claim, *flipped, *rowptr, *entries, *long_list, *n_in, *n_out;
    long long* sum;
    void* inc_scratch;
    int64_t bytes;
};
MrLayout mr_layout(void* base, int64_t nt, int64_t nv) {
    Take t{(char*)base, 256};
    MrLayout L{};
    L.st = (MrState*)base;
    L.parent = t.take<int32_t>(4 * nt + nv);
    L.root = t.take<int32_t>(4 * nt);
    L.sum = t.take<long long>(4 * nt);
    L.flag = t.take<int32_t>(4 * nt);
    L.hull = t.take<int32_t>(nv);
    L.lone = t.take<int32_t>(nv);
    L.move = t.take<int32_t>(nv);
    L.lost = t.take<int32_t>(nv);
    L.claim = t.take<int32_t>(nt);
    L.flipped = t.take<int32_t>(nt);
    L.rowptr = t.take<int32_t>(nv + 1);
    L.entries = t.take<int32_t>(4 * nt);
    L.long_list = t.take<int32_t>(nv);
    L.n_in = t.take<int32_t>(nv);
    L.n_out = t.take<int32_t>(nv);
    L.inc_scratch = t.take<char>(dgnn_vertex_incidence_scratch_bytes(nv));
    L.bytes = t.off;
    return L;
}

bool mr_rows_aligned(const void* tets, const void* nbr) { return (((uintptr_t)tets | (uintptr_t)nbr) & 15) == 0; }   // rows are read as int4
bool mr_sizes_ok(int64_t nt, int64_t nv) { return nt >= 0 && nv >= 0 && nt < INT32_MAX / 4 && nv < INT32_MAX && 4 * nt + nv < (int64_t)INT32_MAX; }

int mr_read_state(MrState* hs, const MrState* st, hipStream_t stream, const char* what) {
    int rc = dgnn_check_launch(what);
    if (rc || (rc = mm_read(hs, st, sizeof(MrState), stream, what))) return rc;
    if (!hs->err) return DGNN_OK;
    const int32_t e = hs->err;
    dgnn_set_error("%s: %s%s%s%s%s%s", what, e & MR_BAD_ID ? "an id out of range; " : "",
                   e & MR_NEIGHBOR ? "a neighbour that does not hold the shared facet or does not name the cell back; " : "",
                   e & MR_COST ? "a negative cost; " : "", e & MR_LABEL ? "a label outside {0, 1}; " : "",
                   e & MR_DEGENERATE ? "a cell with a repeated vertex; " : "", e & MR_LIST ? "the list of long rows overflowed; " : "");
    return DGNN_E_INVALID;
}

#define MR_LAUNCH(kernel, items, ...) hipLaunchKernelGGL(kernel, mesh_launch_grid(items), dim3(MESH_THREADS), 0, stream, __VA_ARGS__)

// the checks and what does not change between rounds: the hull flags and the incidence rows.  SYNCHRONISES.
int mr_prepare(const MrLayout& L, const int32_t* tets, const int32_t* nbr, const int32_t* labels, const int32_t* cost, int64_t nt, int64_t nv,
               hipStream_t stream, const char* what) {
    (void)hipMemsetAsync(L.st, 0, sizeof(MrState), stream);
    (void)hipMemsetAsync(L.hull, 0, sizeof(int32_t) * (nv > 0 ? nv : 1), stream);
    (void)hipMemsetAsync(L.flipped, 0, sizeof(int32_t) * (nt > 0 ? nt : 1), stream);
    MrState hs{};
    int rc;
    if (nt > 0) MR_LAUNCH(k_check_ids, 4 * nt, tets, 4 * nt, nv, &L.st->err, MR_BAD_ID);
    if ((rc = mr_read_state(&hs, L.st, stream, what))) return rc;
    if (nt > 0) MR_LAUNCH(k_mr_check, nt, tets, nbr, labels, cost, nt, L.hull, L.st);
    if ((rc = mr_read_state(&hs, L.st, stream, what))) return rc;
    return dgnn_vertex_incidence(tets, nt, nv, L.rowptr, L.entries, L.inc_scratch, stream);
}

// steps 1 and 2 of a round on the current labels: components, a(v), b(v), the singular count and (select != 0) the moves
void mr_detect(const MrLayout& L, const int32_t* tets, const int32_t* nbr, const int32_t* labels, const int32_t* cost, int64_t nt, int64_t nv,
               int select, int32_t* n_in, int32_t* n_out, hipStream_t stream) {
    const int64_t n4 = 4 * nt;
    (void)hipMemsetAsync(&L.st->n_long, 0, sizeof(int32_t), stream);
    (void)hipMemsetAsync(&L.st->singular, 0, 2 * sizeof(unsigned long long), stream);
    MR_LAUNCH(k_mr_reset, n4 + nv, n4, nv, L.parent, L.sum, L.flag, L.claim, L.lost);
    if (nt > 0) MR_LAUNCH(k_mr_join, nt, (const int4*)tets, (const int4*)nbr, labels, nt, L.parent);
    MR_LAUNCH(k_mr_roots, n4 + nv, cost, L.flipped, L.hull, n4, nv, select, L.parent, L.root, L.sum, L.flag, L.lone);
    MR_LAUNCH(k_mr_select, nv, L.rowptr, L.entries, labels, L.root, L.sum, L.flag, L.lone, nv, select, n_in, n_out, L.move, L.long_list, L.st);
    // the long rows: the list's length is on the device; the grid covers a few hundred rows at a time
    hipLaunchKernelGGL(k_mr_select_long, dim3(dgnn_grid_cap(dgnn_cdiv(nv, 64), 1)), dim3(MESH_THREADS), 0, stream, L.rowptr, L.entries, labels, L.root,
                       L.sum, L.flag, L.lone, nv, select, n_in, n_out, L.move, L.long_list, L.st);
}

}  // namespace

// ================================================================================================================================
extern "C" int64_t dgnn_vertex_components_scratch_bytes(int64_t n_tets, int64_t n_vertices) {
    if (!mr_sizes_ok(n_tets, n_vertices)) return 0;
    return mr_layout(nullptr, n_tets, n_vertices).bytes;
}

extern "C" int dgnn_vertex_components(const int32_t* tetrahedra, const int32_t* neighbors, const int32_t* labels, int64_t n_tets, int64_t n_vertices,
                                      int32_t* n_inside_out, int32_t* n_outside_out, int64_t* n_singular_out, void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(mr_sizes_ok(n_tets, n_vertices), DGNN_E_UNSUPPORTED, "vertex_components: sizes exceed the int32 indexing");
    DGNN_REQUIRE(scratch && n_singular_out && (n_tets == 0 || (tetrahedra && neighbors && labels)) && (n_vertices == 0 || (n_inside_out && n_outside_out)),
                 DGNN_E_INVALID, "vertex_components: bad args");
    DGNN_REQUIRE(mr_rows_aligned(tetrahedra, neighbors), DGNN_E_INVALID, "vertex_components: tetrahedra and neighbors must be 16-byte aligned");
    const MrLayout L = mr_layout(scratch, n_tets, n_vertices);
    int rc = mr_prepare(L, tetrahedra, neighbors, labels, nullptr, n_tets, n_vertices, stream, "vertex_components");
    if (rc) return rc;
    mr_detect(L, tetrahedra, neighbors, labels, nullptr, n_tets, n_vertices, 0, n_inside_out, n_outside_out, stream);
    MrState hs{};
    if ((rc = mr_read_state(&hs, L.st, stream, "vertex_components"))) return rc;
    *n_singular_out = (int64_t)hs.singular;
    return DGNN_OK;
}

extern "C" int64_t dgnn_manifold_repair_scratch_bytes(int64_t n_tets, int64_t n_vertices) {
    return dgnn_vertex_components_scratch_bytes(n_tets, n_vertices);
}

extern "C" int dgnn_manifold_repair(const int32_t* tetrahedra, const int32_t* neighbors, int32_t* labels, const int32_t* cost, int64_t n_tets,
                                    int64_t n_vertices, int64_t max_rounds, int32_t* flipped_out, int64_t* stats_out, void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(mr_sizes_ok(n_tets, n_vertices), DGNN_E_UNSUPPORTED, "manifold_repair: sizes exceed the int32 indexing");
    DGNN_REQUIRE(scratch && stats_out && (n_tets == 0 || (tetrahedra && neighbors && labels)), DGNN_E_INVALID, "manifold_repair: bad args");
    DGNN_REQUIRE(mr_rows_aligned(tetrahedra, neighbors), DGNN_E_INVALID, "manifold_repair: tetrahedra and neighbors must be 16-byte aligned");
    const MrLayout L = mr_layout(scratch, n_tets, n_vertices);
    const int64_t n4 = 4 * n_tets;
    for (int i = 0; i < DGNN_MANIFOLD_N_STATS; ++i) stats_out[i] = 0;
    int rc = mr_prepare(L, tetrahedra, neighbors, labels, cost, n_tets, n_vertices, stream, "manifold_repair");
    if (rc) return rc;
    MrState hs{};
    int64_t rounds = 0;
    for (;;) {   // a cell flips at most once and every round with a move flips one: at most n_tets rounds apply something
        const bool last = (max_rounds >= 0 && rounds >= max_rounds) || rounds > n_tets;
        mr_detect(L, tetrahedra, neighbors, labels, cost, n_tets, n_vertices, last ? 0 : 1, L.n_in, L.n_out, stream);
        if (!last && n_tets > 0) {
            MR_LAUNCH(k_mr_claim, n4, tetrahedra, L.move, n4, L.claim);
            MR_LAUNCH(k_mr_lose, n4, tetrahedra, L.move, L.claim, n4, L.lost);
            MR_LAUNCH(k_mr_apply, n4, tetrahedra, L.move, L.lost, L.root, cost, n4, labels, L.flipped, L.st);
        }
        if ((rc = mr_read_state(&hs, L.st, stream, "manifold_repair"))) return rc;
        if (rounds == 0) stats_out[DGNN_MANIFOLD_SINGULAR_BEFORE] = (int64_t)hs.singular;
        stats_out[DGNN_MANIFOLD_SINGULAR_AFTER] = (int64_t)hs.singular;   // of the labels this round began with: final when it moved nothing
        if (last || hs.movers == 0) break;
        ++rounds;
    }
    stats_out[DGNN_MANIFOLD_ROUNDS] = rounds;
    stats_out[DGNN_MANIFOLD_MOVES] = (int64_t)hs.moves;
    stats_out[DGNN_MANIFOLD_TO_INSIDE] = (int64_t)hs.to_inside;
    stats_out[DGNN_MANIFOLD_TO_OUTSIDE] = (int64_t)hs.to_outside;
    stats_out[DGNN_MANIFOLD_FLIPPED_CELLS] = (int64_t)(hs.to_inside + hs.to_outside);
    stats_out[DGNN_MANIFOLD_FLIPPED_COST] = (int64_t)hs.flipped_cost;
    if (flipped_out && n_tets > 0) (void)hipMemcpyAsync(flipped_out, L.flipped, sizeof(int32_t) * n_tets, hipMemcpyDeviceToDevice, stream);
    return dgnn_check_launch("manifold_repair");
}
