// Exact binary graph cut of the per-cell labels (reference processing/generate_mesh.py:15-58, the gco alpha-expansion with
// two labels and a Potts term).  Two labels + non-negative Potts weights = a submodular energy whose global minimum is one
// s-t minimum cut; a converged alpha-expansion reaches the same energy.  The cut is found by push-relabel:
//
//   costs      D_i(0) = rint(pred[i,1] * uw), D_i(1) = rint(pred[i,0] * uw) (fp32 product, half to even), terminal capacities
//   graph      CSR of the undirected facet graph (count / scan / fill, each node's arcs sorted by arc id = deterministic),
//              reverse-slot index per arc
//   phase 1    synchronous (Jacobi) push-relabel steps: k_push decides from a snapshot of the heights and writes the amounts
//              into the node's OWN outgoing arc slots; k_gather takes them in through the reverse slots.  A node pushes only
//              to neighbours lower than itself in (height, id), so two opposite pushes never meet in one step: no atomics,
//              the preflow stays valid and reruns are bit-identical.
//   relabel    level-synchronous BFS from t over residual arcs (frontier queues) every few steps; unreached nodes get
//              height n + 1 (above any distance) and drop out
//   stop       an exact BFS from t reaches no node with positive excess: the preflow is maximum, and the nodes that BFS
//              reached are label 1 (outside) -- the minimal sink side, i.e. the minimiser with the fewest outside cells.
//              Heights only steer the pushes; the answer comes from the BFS alone.
//   energy     int64 sums: E = sum D_i(l_i) + sum over rows w_r [l_i != l_j]; flow = sum of what reached t.  E == flow + sum min D_i
//              is checked before returning (the max-flow / min-cut identity).
//   weights    one Potts weight for every row (dgnn_graph_cut_binary) or one capacity per row (dgnn_graph_cut_weighted): the same body
//              (gc_solve), the four kernels that read a weight (k_count, k_rev, k_check_caps, k_pair_energy) templated on where it comes from.  A row of weight 0 keeps its arcs
//              (the CSR does not depend on the weights) and carries nothing.
#include "common.h"
#include "mesh_common.h"

int dgnn_exclusive_scan_i32(const int32_t* in, int64_t n, int32_t* out, int32_t* sums_scratch, hipStream_t stream);  // plan.hip

namespace {

// error bits of the status word (checked once after the costs and graph are built)
constexpr int32_t GC_BAD_EDGE = 1, GC_NONFINITE = 2, GC_COST_RANGE = 4, GC_CAP_OVERFLOW = 8, GC_NEG_WEIGHT = 16;
constexpr int GC_BFS_GRID = 1024;      // blocks of a BFS level launch (grid-stride over the frontier)
constexpr int GC_BFS_BATCH = 8;        // BFS levels queued between two reads of the frontier size
constexpr int64_t GC_MAX_STEPS = 1 << 19;
constexpr int GC_MAX_RELABELS = 1 << 14;
constexpr int GC_SORT_INLINE = 8;      // segments up to this length are sorted in registers

// status words at the front of the scratch: [0] error bits, [1] excess reached by the BFS, [2..4] frontier counters (ring of 3)
struct GcState {
    int32_t err, excess_hit, cnt[3], pad[3];
    unsigned long long sums[4];        // sum D_i(l_i), sum over rows w [l_i != l_j], flow into t, sum min D_i
};

__global__ void k_costs(const float* __restrict__ logits, int64_t ld, int64_t n, float uw, int32_t* __restrict__ d0, int32_t* __restrict__ d1,
                        int32_t* __restrict__ e, int32_t* __restrict__ rt, GcState* st) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float p0 = logits[i * ld], p1 = logits[i * ld + 1];
        int32_t a = 0, b = 0;
        if (!isfinite(p0) || !isfinite(p1)) {
            atomicOr(&st->err, GC_NONFINITE);
        } else {
            const float c0 = rintf(__fmul_rn(p1, uw)), c1 = rintf(__fmul_rn(p0, uw));   // the reference swaps the columns
            if (!(fabsf(c0) < 1073741824.f) || !(fabsf(c1) < 1073741824.f)) atomicOr(&st->err, GC_COST_RANGE);
            else { a = (int32_t)c0; b = (int32_t)c1; }
        }
        d0[i] = a;
        d1[i] = b;
        e[i] = b > a ? b - a : 0;    // s -> i, saturated from the start: the initial excess
        rt[i] = a > b ? a - b : 0;   // i -> t
    }
}

// the weight of row r: PER_ROW ? rw[r] : w (the scalar form never reads rw)
template <bool PER_ROW>
__device__ __forceinline__ int32_t row_weight(const int32_t* __restrict__ rw, int32_t w, int64_t r) {
    if constexpr (PER_ROW) return rw[r];
    else return w;
}

template <bool PER_ROW>
__global__ void k_count(const int32_t* __restrict__ edges, int64_t rows, int64_t n, const int32_t* __restrict__ rw, int32_t* __restrict__ deg,
                        GcState* st) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t i = edges[2 * r], j = edges[2 * r + 1];
        if (PER_ROW && rw[r] < 0) atomicOr(&st->err, GC_NEG_WEIGHT);   // of any row, a self-loop's included
        if (i < 0 || i >= n || j < 0 || j >= n) { atomicOr(&st->err, GC_BAD_EDGE); continue; }
        if (i == j) continue;   // a self-loop never separates its cell from itself
        atomicAdd(deg + i, 1);
        atomicAdd(deg + j, 1);
    }
}

// arc 2r = edges[r,0] -> edges[r,1], arc 2r+1 the other way; slots claimed in any order here, sorted by arc id in k_sort_segments
__global__ void k_fill(const int32_t* __restrict__ edges, int64_t rows, int64_t n, int32_t* __restrict__ cursor, int32_t* __restrict__ nbr,
                       int32_t* __restrict__ aid) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t i = edges[2 * r], j = edges[2 * r + 1];
        if (i < 0 || i >= n || j < 0 || j >= n || i == j) continue;
        const int32_t si = atomicAdd(cursor + i, 1), sj = atomicAdd(cursor + j, 1);
        nbr[si] = j;
        aid[si] = (int32_t)(2 * r);
        nbr[sj] = i;
        aid[sj] = (int32_t)(2 * r + 1);
    }
}

// each node's arcs in ascending arc id (a Delaunay cell has <= 4: sorted in registers; longer segments by insertion sort in
// place -- correct for any degree, quadratic in it); pos_of_arc[arc id] = slot
__global__ void k_sort_segments(const int32_t* __restrict__ rowptr, int64_t n, int32_t* __restrict__ nbr, int32_t* __restrict__ aid,
                                int32_t* __restrict__ pos_of_arc) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t b = rowptr[i], len = rowptr[i + 1] - b;
        if (len <= GC_SORT_INLINE) {
            int32_t k[GC_SORT_INLINE], v[GC_SORT_INLINE];
#pragma unroll
            for (int t = 0; t < GC_SORT_INLINE; ++t)
                if (t < len) { k[t] = aid[b + t]; v[t] = nbr[b + t]; }
#pragma unroll
            for (int t = 1; t < GC_SORT_INLINE; ++t)
#pragma unroll
                for (int u = t; u > 0; --u)
                    if (u < len && k[u - 1] > k[u]) {
                        const int32_t tk = k[u], tv = v[u];
                        k[u] = k[u - 1]; v[u] = v[u - 1];
                        k[u - 1] = tk; v[u - 1] = tv;
                    }
#pragma unroll
            for (int t = 0; t < GC_SORT_INLINE; ++t)
                if (t < len) { aid[b + t] = k[t]; nbr[b + t] = v[t]; pos_of_arc[k[t]] = b + t; }
        } else {
            for (int32_t t = 1; t < len; ++t) {
                const int32_t tk = aid[b + t], tv = nbr[b + t];
                int32_t u = t;
                for (; u > 0 && aid[b + u - 1] > tk; --u) { aid[b + u] = aid[b + u - 1]; nbr[b + u] = nbr[b + u - 1]; }
                aid[b + u] = tk;
                nbr[b + u] = tv;
            }
            for (int32_t t = 0; t < len; ++t) pos_of_arc[aid[b + t]] = b + t;
        }
    }
}

// the slots in use are [0, rowptr[n]) (self-loop rows and rows with a bad id have none); arc id >> 1 = its row
template <bool PER_ROW>
__global__ void k_rev(const int32_t* __restrict__ rowptr, int64_t n, const int32_t* __restrict__ aid, const int32_t* __restrict__ pos_of_arc,
                      const int32_t* __restrict__ rw, int32_t w, int32_t* __restrict__ rev, int32_t* __restrict__ res, int32_t* __restrict__ push) {
    const int64_t n_arcs = rowptr[n];
    for (int64_t a = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; a < n_arcs; a += (int64_t)gridDim.x * blockDim.x) {
        rev[a] = pos_of_arc[aid[a] ^ 1];
        res[a] = row_weight<PER_ROW>(rw, w, aid[a] >> 1);
        push[a] = 0;
    }
}

// terminal capacity + max(sum of the incident weights, 2 * the largest of them) must fit int32: bounds the excess (<= cs + what can flow
// in) and an arc's residual (<= twice its row's weight).  With one weight w that is max(degree, 2) * w.
template <bool PER_ROW>
__global__ void k_check_caps(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ aid, const int32_t* __restrict__ e,
                             const int32_t* __restrict__ rt, int64_t n, const int32_t* __restrict__ rw, int32_t w, GcState* st) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t b = rowptr[i], end = rowptr[i + 1];
        if (end == b) continue;
        int64_t sum, top;
        if constexpr (PER_ROW) {
            sum = 0;
            top = 0;
            for (int32_t a = b; a < end; ++a) {
                const int64_t wa = rw[aid[a] >> 1];
                sum += wa;
                top = wa > top ? wa : top;
            }
        } else {
            sum = (int64_t)(end - b) * w;
            top = w;
        }
        const int64_t cap = (int64_t)e[i] + rt[i] + (sum > 2 * top ? sum : 2 * top);
        if (cap > INT32_MAX) atomicOr(&st->err, GC_CAP_OVERFLOW);
    }
}

// ---- phase 1: one synchronous push-relabel step = k_push + k_gather ------------------------------------------------------------
// k_push reads h (neighbours' heights: a snapshot, nothing writes h in this launch) and its own node's state; writes the amounts into
// the node's own slots push[a], its own residuals / excess, its new height into hnew and `touched` of itself and of every neighbour
// it pushed to (the same value 1 from every writer).
__global__ void k_push(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ nbr, const int32_t* __restrict__ h, int64_t n,
                       int32_t* __restrict__ e, int32_t* __restrict__ rt, int32_t* __restrict__ res, int32_t* __restrict__ push,
                       int32_t* __restrict__ hnew, int32_t* __restrict__ touched) {
    const int32_t hn = (int32_t)n + 1;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int32_t ex = e[i];
        if (ex <= 0) continue;
        const int32_t hi = h[i];
        if (hi >= hn) continue;
        const int32_t t_res = rt[i];
        if (t_res > 0) {                       // t is below every node
            const int32_t d = ex < t_res ? ex : t_res;
            rt[i] = t_res - d;
            ex -= d;
        }
        const int32_t b = rowptr[i], end = rowptr[i + 1];
        int32_t hmin = INT32_MAX;
        for (int32_t a = b; a < end && ex > 0; ++a) {
            int32_t r = res[a];
            if (r <= 0) continue;
            const int32_t j = nbr[a], hj = h[j];
            if (hj < hi || (hj == hi && j < i)) {
                const int32_t d = ex < r ? ex : r;
                push[a] = d;
                res[a] = r - d;
                ex -= d;
                r -= d;
                touched[j] = 1;
            }
            if (r > 0 && hj < hmin) hmin = hj;
        }
        e[i] = ex;
        if (ex > 0) {   // the loop saw every arc and saturated each lower one: relabel to the lowest residual neighbour + 1 (> hi)
            hnew[i] = hmin >= hn - 1 ? hn : hmin + 1;
            touched[i] = 1;
        }
    }
}

// k_gather: a touched node takes in what its neighbours pushed (through the reverse slots, which it clears) and its new height
__global__ void k_gather(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ rev, int64_t n, int32_t* __restrict__ e,
                         int32_t* __restrict__ res, int32_t* __restrict__ push, int32_t* __restrict__ h, const int32_t* __restrict__ hnew,
                         int32_t* __restrict__ touched) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (!touched[i]) continue;
        touched[i] = 0;
        h[i] = hnew[i];
        int32_t in = 0;
        for (int32_t a = rowptr[i], end = rowptr[i + 1]; a < end; ++a) {
            const int32_t ra = rev[a], d = push[ra];
            if (d) {
                push[ra] = 0;
                res[a] += d;
                in += d;
            }
        }
        e[i] += in;
    }
}

// ---- global relabel: BFS from t over residual arcs (level L's frontier holds the nodes at distance L + 1) -------------------------
__global__ void k_bfs_init(const int32_t* __restrict__ e, const int32_t* __restrict__ rt, int64_t n, int32_t* __restrict__ h,
                           int32_t* __restrict__ hnew, int32_t* __restrict__ frontier, GcState* st) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int32_t d = (int32_t)n + 1;   // unreached (a reached node is at most n hops from t)
        if (rt[i] > 0) {
            d = 1;
            frontier[atomicAdd(&st->cnt[0], 1)] = (int32_t)i;
            if (e[i] > 0) st->excess_hit = 1;
        }
        h[i] = d;
        hnew[i] = d;
    }
}

__global__ void k_bfs_level(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ nbr, const int32_t* __restrict__ rev,
                            const int32_t* __restrict__ res, const int32_t* __restrict__ e, int64_t n, int level,
                            const int32_t* __restrict__ cur, int32_t* __restrict__ next, int32_t* __restrict__ h, int32_t* __restrict__ hnew,
                            GcState* st) {
    const int32_t count = st->cnt[level % 3];
    if (blockIdx.x == 0 && threadIdx.x == 0) st->cnt[(level + 2) % 3] = 0;   // read by the previous level, written by the next
    const int32_t hn = (int32_t)n + 1, dist = level + 2;
    for (int32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        const int32_t u = cur[k];
        for (int32_t a = rowptr[u], end = rowptr[u + 1]; a < end; ++a) {
            if (res[rev[a]] <= 0) continue;    // arc j -> u has no residual capacity
            const int32_t j = nbr[a];
            if (h[j] != hn) continue;
            if (atomicCAS(h + j, hn, dist) == hn) {
                hnew[j] = dist;
                next[atomicAdd(&st->cnt[(level + 1) % 3], 1)] = j;
                if (e[j] > 0) st->excess_hit = 1;
            }
        }
    }
}

// ---- result ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MESH_THREADS) k_labels_energy(const int32_t* __restrict__ h, const int32_t* __restrict__ d0,
                                                              const int32_t* __restrict__ d1, const int32_t* __restrict__ rt, int64_t n,
                                                              int32_t* __restrict__ labels, GcState* st) {
    long long ed = 0, fl = 0, mn = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t l = h[i] <= (int32_t)n, a = d0[i], b = d1[i];
        labels[i] = l;
        ed += l ? b : a;
        fl += (a > b ? a - b : 0) - rt[i];
        mn += a < b ? a : b;
    }
    block_add_atomic(&st->sums[0], ed);
    block_add_atomic(&st->sums[2], fl);
    block_add_atomic(&st->sums[3], mn);
}

template <bool PER_ROW>
__global__ void __launch_bounds__(MESH_THREADS) k_pair_energy(const int32_t* __restrict__ edges, int64_t rows, const int32_t* __restrict__ labels,
                                                            const int32_t* __restrict__ rw, int32_t w, GcState* st) {
    long long cut = 0;
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
        const bool differ = labels[edges[2 * r]] != labels[edges[2 * r + 1]];
        if constexpr (PER_ROW) cut += differ ? (long long)rw[r] : 0;
        else cut += differ;
    }
    block_add_atomic(&st->sums[1], PER_ROW ? cut : cut * (long long)w);
}

__global__ void k_outputs(const GcState* st, int64_t* energy_out, int64_t* flow_out, int32_t* stats_out, int32_t steps, int32_t relabels) {
    if (threadIdx.x == 0) {
        if (energy_out) *energy_out = (int64_t)(st->sums[0] + st->sums[1]);
        if (flow_out) *flow_out = (int64_t)st->sums[2];
        if (stats_out) { stats_out[0] = steps; stats_out[1] = relabels; }
    }
}

struct GcLayout {
    GcState* st;
    int32_t *d0, *d1, *e, *rt, *h, *hnew, *touched, *rowptr, *cursor, *fr0, *fr1, *sums;
    int32_t *nbr, *aid, *pos, *rev, *res, *push;
    int64_t bytes;
};

GcLayout gc_layout(void* base, int64_t n, int64_t rows) {
    GcLayout L{};
    char* p = (char*)base;
    int64_t off = 0;
    auto take = [&](int64_t elems) {
        int32_t* q = (int32_t*)(p ? p + off : nullptr);
        off += (((elems > 0 ? elems : 1) * 4 + 255) / 256) * 256;
        return q;
    };
    L.st = (GcState*)(p ? p : nullptr);
    off = 256;
    L.d0 = take(n); L.d1 = take(n); L.e = take(n); L.rt = take(n); L.h = take(n); L.hnew = take(n); L.touched = take(n);
    L.rowptr = take(n + 1); L.cursor = take(n + 1); L.fr0 = take(n); L.fr1 = take(n); L.sums = take(dgnn_cdiv(n + 1, 2048) + 2);
    const int64_t arcs = 2 * rows;
    L.nbr = take(arcs); L.aid = take(arcs); L.pos = take(arcs); L.rev = take(arcs); L.res = take(arcs); L.push = take(arcs);
    L.bytes = off;
    return L;
}

// The solver behind both entry points.  PER_ROW: row r weighs row_weights[r]; else every row weighs w.
template <bool PER_ROW>
int gc_solve(const char* what, const float* logits, int64_t ld, int64_t n, const int32_t* edges, int64_t n_rows, float unary_weight,
             const int32_t* row_weights, int32_t w, int32_t* labels_out, int64_t* energy_out, int64_t* flow_out, int32_t* stats_out, void* scratch,
             hipStream_t stream) {
    char where[96];
    auto at = [&](const char* phase) { snprintf(where, sizeof(where), "%s (%s)", what, phase); return where; };
    DGNN_REQUIRE(n >= 0 && n_rows >= 0 && ld >= 2 && scratch && (n == 0 || (logits && labels_out)) && (n_rows == 0 || edges) &&
                     (!PER_ROW || n_rows == 0 || row_weights),
                 DGNN_E_INVALID, "%s: bad args", what);
    DGNN_REQUIRE(w >= 0, DGNN_E_INVALID, "%s: binary_weight %d < 0 is not a cut problem", what, w);
    DGNN_REQUIRE(n < INT32_MAX / 2 && n_rows < INT32_MAX / 2, DGNN_E_UNSUPPORTED, "%s: %lld cells / %lld rows exceed the int32 indexing", what,
                 (long long)n, (long long)n_rows);
    const GcLayout L = gc_layout(scratch, n, n_rows);
    const int64_t arcs = 2 * n_rows;
    const dim3 block(MESH_THREADS);
    GcState hs{};

    // costs; graph: degrees counted into `cursor`, scanned into rowptr, cursor = rowptr again as the fill's claim pointers
    (void)hipMemsetAsync(L.st, 0, sizeof(GcState), stream);
    (void)hipMemsetAsync(L.cursor, 0, sizeof(int32_t) * (n + 1), stream);
    (void)hipMemsetAsync(L.touched, 0, sizeof(int32_t) * (n > 0 ? n : 1), stream);
    hipLaunchKernelGGL(k_costs, mesh_launch_grid(n), block, 0, stream, logits, ld, n, unary_weight, L.d0, L.d1, L.e, L.rt, L.st);
    hipLaunchKernelGGL(k_count<PER_ROW>, mesh_launch_grid(n_rows), block, 0, stream, edges, n_rows, n, row_weights, L.cursor, L.st);
    int rc = dgnn_exclusive_scan_i32(L.cursor, n, L.rowptr, L.sums, stream);
    if (rc) return rc;
    (void)hipMemcpyAsync(L.cursor, L.rowptr, sizeof(int32_t) * (n + 1), hipMemcpyDeviceToDevice, stream);
    hipLaunchKernelGGL(k_fill, mesh_launch_grid(n_rows), block, 0, stream, edges, n_rows, n, L.cursor, L.nbr, L.aid);
    hipLaunchKernelGGL(k_sort_segments, mesh_launch_grid(n), block, 0, stream, L.rowptr, n, L.nbr, L.aid, L.pos);
    hipLaunchKernelGGL(k_rev<PER_ROW>, mesh_launch_grid(arcs), block, 0, stream, L.rowptr, n, L.aid, L.pos, row_weights, w, L.rev, L.res, L.push);
    hipLaunchKernelGGL(k_check_caps<PER_ROW>, mesh_launch_grid(n), block, 0, stream, L.rowptr, L.aid, L.e, L.rt, n, row_weights, w, L.st);
    if ((rc = dgnn_check_launch(at("build")))) return rc;
    if ((rc = mm_read(&hs, L.st, sizeof(GcState), stream, what))) return rc;
    if (hs.err) {
        dgnn_set_error("%s: %s%s%s%s%s", what, hs.err & GC_BAD_EDGE ? "edge id outside [0, n); " : "",
                       hs.err & GC_NONFINITE ? "non-finite logits; " : "", hs.err & GC_COST_RANGE ? "|unary cost| >= 2^30; " : "",
                       hs.err & GC_NEG_WEIGHT ? "a row weight < 0; " : "", hs.err & GC_CAP_OVERFLOW ? "a node's capacities overflow int32; " : "");
        return DGNN_E_INVALID;
    }

    // phase 1: global relabel, stop test, K synchronous steps; repeat
    int64_t steps = 0;
    int relabels = 0;
    for (;;) {
        if (relabels >= GC_MAX_RELABELS) {
            dgnn_set_error("%s: no maximum preflow after %d global relabels / %lld steps (cap)", what, relabels, (long long)steps);
            return DGNN_E_UNSUPPORTED;
        }
        (void)hipMemsetAsync(&L.st->excess_hit, 0, sizeof(int32_t) * 4, stream);   // excess_hit, cnt[0..2]
        hipLaunchKernelGGL(k_bfs_init, mesh_launch_grid(n), block, 0, stream, L.e, L.rt, n, L.h, L.hnew, L.fr0, L.st);
        int level = 0;
        for (;;) {   // at most n + 1 non-empty levels
            for (int b = 0; b < GC_BFS_BATCH; ++b, ++level)
                hipLaunchKernelGGL(k_bfs_level, dim3(GC_BFS_GRID), block, 0, stream, L.rowptr, L.nbr, L.rev, L.res, L.e, n, level,
                                   level & 1 ? L.fr1 : L.fr0, level & 1 ? L.fr0 : L.fr1, L.h, L.hnew, L.st);
            if ((rc = dgnn_check_launch(at("bfs")))) return rc;
            if ((rc = mm_read(&hs, L.st, sizeof(GcState), stream, what))) return rc;   // synchronises the stream
            if (hs.cnt[level % 3] == 0) break;
        }
        ++relabels;
        if (!hs.excess_hit) break;   // no excess can reach t: the preflow is maximum, the BFS marks the sink side
        const int64_t k = level > 16 ? level : 16;   // excess moves one hop per step: about one BFS depth of steps between relabels
        if (steps + k > GC_MAX_STEPS) {
            dgnn_set_error("%s: no maximum preflow after %lld steps / %d global relabels (cap)", what, (long long)steps, relabels);
            return DGNN_E_UNSUPPORTED;
        }
        for (int64_t s = 0; s < k; ++s) {
            hipLaunchKernelGGL(k_push, mesh_launch_grid(n), block, 0, stream, L.rowptr, L.nbr, L.h, n, L.e, L.rt, L.res, L.push, L.hnew, L.touched);
            hipLaunchKernelGGL(k_gather, mesh_launch_grid(n), block, 0, stream, L.rowptr, L.rev, n, L.e, L.res, L.push, L.h, L.hnew, L.touched);
        }
        steps += k;
        if ((rc = dgnn_check_launch(at("push-relabel")))) return rc;
    }

    // labels = reached by the last BFS; energy, flow and the identity between them
    hipLaunchKernelGGL(k_labels_energy, mesh_launch_grid(n), block, 0, stream, L.h, L.d0, L.d1, L.rt, n, labels_out, L.st);
    hipLaunchKernelGGL(k_pair_energy<PER_ROW>, mesh_launch_grid(n_rows), block, 0, stream, edges, n_rows, labels_out, row_weights, w, L.st);
    hipLaunchKernelGGL(k_outputs, dim3(1), dim3(64), 0, stream, L.st, energy_out, flow_out, stats_out, (int32_t)steps, relabels);
    if ((rc = dgnn_check_launch(at("energy")))) return rc;
    if ((rc = mm_read(&hs, L.st, sizeof(GcState), stream, what))) return rc;
    const int64_t energy = (int64_t)(hs.sums[0] + hs.sums[1]), flow = (int64_t)hs.sums[2], base = (int64_t)hs.sums[3];
    DGNN_REQUIRE(energy == flow + base, DGNN_E_UNSUPPORTED, "%s: energy %lld != flow %lld + sum min D %lld (not a minimum cut)", what,
                 (long long)energy, (long long)flow, (long long)base);
    return DGNN_OK;
}

}  // namespace

extern "C" int64_t dgnn_graph_cut_scratch_bytes(int64_t n, int64_t n_rows) {
    if (n < 0 || n_rows < 0) return 0;
    return gc_layout(nullptr, n, n_rows).bytes;
}

extern "C" int dgnn_graph_cut_binary(const float* logits, int64_t ld, int64_t n, const int32_t* edges, int64_t n_rows, float unary_weight,
                                     int32_t binary_weight, int32_t* labels_out, int64_t* energy_out, int64_t* flow_out, int32_t* stats_out,
                                     void* scratch, void* stream_) {
    return gc_solve<false>("graph_cut_binary", logits, ld, n, edges, n_rows, unary_weight, nullptr, binary_weight, labels_out, energy_out, flow_out,
                           stats_out, scratch, (hipStream_t)stream_);
}

extern "C" int64_t dgnn_graph_cut_weighted_scratch_bytes(int64_t n, int64_t n_rows) { return dgnn_graph_cut_scratch_bytes(n, n_rows); }

extern "C" int dgnn_graph_cut_weighted(const float* logits, int64_t ld, int64_t n, const int32_t* edges, int64_t n_rows, float unary_weight,
                                       const int32_t* row_weights, int32_t* labels_out, int64_t* energy_out, int64_t* flow_out, int32_t* stats_out,
                                       void* scratch, void* stream_) {
    return gc_solve<true>("graph_cut_weighted", logits, ld, n, edges, n_rows, unary_weight, row_weights, 0, labels_out, energy_out, flow_out,
                          stats_out, scratch, (hipStream_t)stream_);
}
