// 3D Delaunay triangulation on the device with exact predicates (the contract is in include/dgnn_hip.h).
//
// Round-based parallel Bowyer-Watson with a ghost vertex (id n): an infinite cell is an ordinary cell with the ghost in one slot, oriented
// so that putting a point p in the ghost's slot gives a positive cell exactly when p lies strictly beyond the hull facet.  The points arrive
// in PRIORITY ORDER (point id = priority), so "lowest priority" is "lowest id" and an integer atomicMin decides every contest.
//
//   conflict   finite cell: p strictly inside its sphere (insphere_pos).  Infinite cell: p strictly beyond the hull facet, or in its plane and in
//              conflict with the finite cell behind it.  Strict conflicts need no perturbation: cavities are star-shaped from p, no flat cell
//              is ever made (DESIGN §28 has the argument).
//   a round    1 pick: every uninserted point holds a cell that conflicts with it; a cell's lowest such point is its candidate (cand[]).
//              2 grow: one thread per candidate walks its cavity breadth-first into a per-lane list.  It gives up -- and claims nothing -- as
//                soon as a cavity or ring cell has a lower candidate, a rule that depends on cand[] alone, not on the schedule.  A survivor
//                claims its cavity and ring with atomicMin(owner) and its cavity with atomicMin(cavq).  A cavity that outgrows the list
//                takes the slow path: the lowest such candidate alone grows its cavity by sweeps over all cells through mark[], then claims.
//              3 verify: a survivor that owns all of its claims wins.  The lowest candidate of all always does: every round inserts a point.
//              4 carve, data-parallel over cells: count the boundary facets per cavity cell, prefix sums give every new cell a rank, ranks
//                below the number of dead cells reuse the dead cells' ids in ascending order, the rest extend the array: ids are free of
//                the schedule.  New cells are staged (the old ones are still read), linked by rotating about each boundary edge inside
//                the cavity, then committed.
//              5 relocate: a point whose cell died walks (exact visibility walk) from the lowest new cell of the cavity that killed it.
//   safety     every device loop is capped by the cell count and raises DL_LOOP; the host runs at most n rounds; no kernel waits on another
//              workgroup; all communication between workgroups is through kernel boundaries.
// The caller turns the raw cells (priority-space ids, ghost = n, dead cells marked -1) into the canonical output (ops.delaunay).
#include "exact_insphere.h"
#include "mesh_common.h"

int dgnn_exclusive_scan_i32(const int32_t* in, int64_t n, int32_t* out, int32_t* sums_scratch, hipStream_t stream);   // plan.hip

namespace {

using dgnn_exact::V3;
using dgnn_exact::load_v3;

constexpr int DL_LIST = 128;           // the fast path's per-lane cavity list
constexpr int32_t DL_INF = 0x7fffffff;
enum { DL_LOOP = 1, DL_DUP = 2, DL_RANGE = 4, DL_NONFINITE = 8, DL_INTERNAL = 16 };
enum { ST_FREE = 0, ST_IN = 1, ST_SURVIVOR = 2, ST_WON = 3 };

struct DlHead {
    int32_t err, bigmin, nwin, maxcav, changed, bigfail, biglose, bigcav, i2, i3;
    unsigned long long dup;   // (q << 32) | v of the lowest duplicate q and the vertex it equals; all ones = none
    unsigned long long ex_insphere, ex_orient;
};

struct Ctr { int in, orient; };

__device__ __forceinline__ void flush(DlHead* h, const Ctr& c) {
    if (c.in) atomicAdd(&h->ex_insphere, (unsigned long long)c.in);
    if (c.orient) atomicAdd(&h->ex_orient, (unsigned long long)c.orient);
}
__device__ __forceinline__ int slot_of(const int32_t* v, int32_t x) { return v[0] == x ? 0 : (v[1] == x ? 1 : (v[2] == x ? 2 : (v[3] == x ? 3 : -1))); }

// orientation of cell v with the point q in slot k (the ghost never reaches a predicate: k is its slot when there is one)
__device__ __forceinline__ int orient_with(const double* __restrict__ P, const int32_t* v, int k, const V3& q, Ctr& ctr) {
    V3 w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = j == k ? q : load_v3(P, v[j]);
    int ex = 0;
    const int s = dgnn_exact::orient_sign(w[0], w[1], w[2], w[3], &ex);
    ctr.orient += ex;
    return s;
}

__device__ __forceinline__ bool in_sphere(const double* __restrict__ P, const int32_t* v, const V3& q, Ctr& ctr) {
    int ex = 0;
    const int s = dgnn_exact::insphere_pos(load_v3(P, v[0]), load_v3(P, v[1]), load_v3(P, v[2]), load_v3(P, v[3]), q, &ex);
    ctr.in += ex;
    return s > 0;
}

__device__ bool conflict(const double* __restrict__ P, const int32_t* tv, const int32_t* tn, int32_t G, int c, const V3& q, Ctr& ctr) {
    int32_t v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = tv[4 * (int64_t)c + j];
    const int g = slot_of(v, G);
    if (g < 0) return in_sphere(P, v, q, ctr);
    const int s = orient_with(P, v, g, q, ctr);
    if (s != 0) return s > 0;
    const int f = tn[4 * (int64_t)c + g];   // the finite cell behind the hull facet
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = tv[4 * (int64_t)f + j];
    return in_sphere(P, v, q, ctr);
}

// ---- start -----------------------------------------------------------------------------------------------------------------------
__global__ void k_check_points(const double* __restrict__ P, int64_t n3, DlHead* h) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n3; i += (int64_t)gridDim.x * blockDim.x) {
        const double x = P[i];
        if (!dgnn_exact::coord_finite(x)) atomicOr(&h->err, DL_NONFINITE);
        else if (!dgnn_exact::insphere_coord_ok(x)) atomicOr(&h->err, DL_RANGE);          // (its range is narrower than coord_class's)
    }
}

// exact 2D orientation of the projections of a, b, c on one coordinate plane, as a 3D orientation with a unit normal
__device__ __forceinline__ int orient2(double ax, double ay, double bx, double by, double cx, double cy, Ctr& ctr) {
    int ex = 0;
    const int s = dgnn_exact::orient_sign(V3{ax, ay, 0.0}, V3{bx, by, 0.0}, V3{cx, cy, 0.0}, V3{ax, ay, 1.0}, &ex);
    ctr.orient += ex;
    return s;
}

__global__ void k_find_i2(const double* __restrict__ P, int n, DlHead* h) {   // the lowest point not collinear with points 0 and 1
    Ctr ctr{0, 0};
    const V3 a = load_v3(P, 0), b = load_v3(P, 1);
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.x == b.x && a.y == b.y && a.z == b.z) {
        atomicOr(&h->err, DL_DUP);
        atomicMin(&h->dup, 1ull << 32);
    }
    for (int i = 2 + blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (i >= h->i2) continue;   // (a stale read only costs the test)
        const V3 c = load_v3(P, i);
        if (orient2(a.x, a.y, b.x, b.y, c.x, c.y, ctr) || orient2(a.y, a.z, b.y, b.z, c.y, c.z, ctr) || orient2(a.z, a.x, b.z, b.x, c.z, c.x, ctr))
            atomicMin(&h->i2, i);
    }
    flush(h, ctr);
}

__global__ void k_find_i3(const double* __restrict__ P, int n, DlHead* h) {   // the lowest point not coplanar with points 0, 1 and i2
    Ctr ctr{0, 0};
    const int i2 = h->i2;
    const V3 a = load_v3(P, 0), b = load_v3(P, 1), c = load_v3(P, i2);
    for (int i = 2 + blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (i == i2) continue;
        int ex = 0;
        if (dgnn_exact::orient_sign(a, b, c, load_v3(P, i), &ex)) atomicMin(&h->i3, i);
        ctr.orient += ex;
    }
    flush(h, ctr);
}

__global__ void k_init(const double* __restrict__ P, int32_t G, int32_t* tv, int32_t* tn, int32_t* state, DlHead* h) {
    if (blockIdx.x || threadIdx.x) return;
    int32_t v[4] = {0, 1, h->i2, h->i3};
    if (dgnn_exact::orient_sign(load_v3(P, v[0]), load_v3(P, v[1]), load_v3(P, v[2]), load_v3(P, v[3])) < 0) {
        const int32_t t = v[2];
        v[2] = v[3];
        v[3] = t;
    }
    for (int k = 0; k < 4; ++k) {
        tv[k] = v[k];
        state[v[k]] = ST_IN;
        int32_t w[4] = {v[0], v[1], v[2], v[3]};
        w[k] = G;
        const int x = k == 0 ? 1 : 0, y = k <= 1 ? 2 : 1;   // the two lowest slots other than k change places: the ghost lies BEYOND facet k
        const int32_t t = w[x];
        w[x] = w[y];
        w[y] = t;
        for (int j = 0; j < 4; ++j) tv[4 * (1 + k) + j] = w[j];
    }
    for (int k = 0; k < 4; ++k) {
        tn[k] = 1 + k;
        for (int j = 0; j < 4; ++j) {
            const int32_t w = tv[4 * (1 + k) + j];
            tn[4 * (1 + k) + j] = w == G ? 0 : 1 + slot_of(v, w);   // across the facet opposite vertex v[m]: the infinite cell of facet m
        }
    }
}

// ---- a round ---------------------------------------------------------------------------------------------------------------------
__global__ void k_reset(int32_t ncell, int32_t* cand, int32_t* owner, int32_t* cavq, int32_t* cav, int32_t* mark, DlHead* h) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        h->bigmin = DL_INF;
        h->changed = h->bigfail = h->biglose = h->bigcav = h->nwin = 0;
    }
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < ncell; c += gridDim.x * blockDim.x) {
        cand[c] = owner[c] = cavq[c] = DL_INF;
        cav[c] = -1;
        mark[c] = 0;
    }
}

__global__ void k_pick(int n, const int32_t* __restrict__ state, const int32_t* __restrict__ pcell, int32_t* cand) {
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x)
        if (state[q] == ST_FREE) atomicMin(&cand[pcell[q]], q);
}

__device__ __forceinline__ bool listed(const int32_t* list, int n, int32_t c) {
    for (int i = 0; i < n; ++i)
        if (list[i] == c) return true;
    return false;
}

__global__ void __launch_bounds__(MESH_THREADS)
k_grow(const double* __restrict__ P, int n, const int32_t* tv, const int32_t* tn, int32_t* state, const int32_t* __restrict__ pcell,
       const int32_t* __restrict__ cand, int32_t* owner, int32_t* cavq, DlHead* h) {
    Ctr ctr{0, 0};
    const int32_t G = n;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x) {
        if (state[q] != ST_FREE) continue;
        const int32_t c0 = pcell[q];
        if (cand[c0] != q) continue;
        const V3 pq = load_v3(P, q);
        if (!conflict(P, tv, tn, G, c0, pq, ctr)) {   // an empty cavity: q is a vertex of the cell that holds it
            int32_t dv = -1;
            for (int j = 0; j < 4; ++j) {
                const int32_t v = tv[4 * (int64_t)c0 + j];
                if (v == G) continue;
                const V3 pv = load_v3(P, v);
                if (pv.x == pq.x && pv.y == pq.y && pv.z == pq.z) dv = v;
            }
            atomicOr(&h->err, dv >= 0 ? DL_DUP : DL_INTERNAL);
            if (dv >= 0) atomicMin(&h->dup, ((unsigned long long)q << 32) | (unsigned long long)dv);
            continue;
        }
        int32_t list[DL_LIST];
        int m = 1, head = 0;
        bool lose = false, big = false;
        list[0] = c0;
        while (head < m && !lose && !big) {
            const int32_t c = list[head++];
            for (int k = 0; k < 4; ++k) {
                const int32_t nb = tn[4 * (int64_t)c + k];
                if (listed(list, m, nb)) continue;
                if (cand[nb] < q) { lose = true; break; }
                if (!conflict(P, tv, tn, G, nb, pq, ctr)) continue;
                if (m == DL_LIST) { big = true; break; }
                list[m++] = nb;
            }
        }
        if (lose) continue;
        if (big) { atomicMin(&h->bigmin, q); continue; }
        for (int i = 0; i < m; ++i) {
            const int32_t c = list[i];
            atomicMin(&owner[c], q);
            atomicMin(&cavq[c], q);
            for (int k = 0; k < 4; ++k) atomicMin(&owner[tn[4 * (int64_t)c + k]], q);
        }
        state[q] = ST_SURVIVOR;
    }
    flush(h, ctr);
}

// the slow path: the cavity of the one candidate q = bigmin through mark[] (1 = cavity, 2 = ring), one sweep per launch
__global__ void k_big_seed(const int32_t* __restrict__ pcell, int32_t* mark, DlHead* h) {
    if (blockIdx.x == 0 && threadIdx.x == 0) mark[pcell[h->bigmin]] = 1;
}

__global__ void __launch_bounds__(MESH_THREADS)
k_big_sweep(const double* __restrict__ P, int n, int32_t ncell, const int32_t* tv, const int32_t* tn, const int32_t* __restrict__ cand, int32_t* mark,
            DlHead* h) {
    Ctr ctr{0, 0};
    const int32_t q = h->bigmin, G = n;
    const V3 pq = load_v3(P, q);
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < ncell; c += gridDim.x * blockDim.x) {
        if (mark[c] != 1) continue;
        for (int k = 0; k < 4; ++k) {
            const int32_t nb = tn[4 * (int64_t)c + k];
            if (mark[nb] != 0) continue;
            if (cand[nb] < q) h->biglose = 1;
            if (conflict(P, tv, tn, G, nb, pq, ctr)) {
                mark[nb] = 1;
                h->changed = 1;
            } else {
                mark[nb] = 2;
            }
        }
    }
    flush(h, ctr);
}

__global__ void k_big_claim(int32_t ncell, const int32_t* __restrict__ mark, int32_t* owner, int32_t* cavq, const DlHead* h) {
    if (h->biglose) return;
    const int32_t q = h->bigmin;
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < ncell; c += gridDim.x * blockDim.x) {
        if (mark[c] == 0) continue;
        atomicMin(&owner[c], q);
        if (mark[c] == 1) atomicMin(&cavq[c], q);
    }
}

__global__ void k_big_verify(int32_t ncell, const int32_t* __restrict__ mark, const int32_t* __restrict__ owner, DlHead* h) {
    const int32_t q = h->bigmin;
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < ncell; c += gridDim.x * blockDim.x)
        if (mark[c] != 0 && owner[c] != q) h->bigfail = 1;
}

__global__ void k_big_commit(int32_t ncell, const int32_t* __restrict__ mark, int32_t* cav, int32_t* state, DlHead* h) {
    if (h->biglose || h->bigfail) return;
    const int32_t q = h->bigmin;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        state[q] = ST_WON;
        atomicAdd(&h->nwin, 1);
    }
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < ncell; c += gridDim.x * blockDim.x)
        if (mark[c] == 1) {
            cav[c] = q;
            atomicAdd(&h->bigcav, 1);
        }
}

__global__ void __launch_bounds__(MESH_THREADS)
k_verify(int n, const int32_t* tn, int32_t* state, const int32_t* __restrict__ pcell, const int32_t* __restrict__ owner,
         const int32_t* __restrict__ cavq, int32_t* cav, DlHead* h) {
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x) {
        if (state[q] != ST_SURVIVOR) continue;
        int32_t list[DL_LIST];
        int m = 1, head = 0;
        list[0] = pcell[q];
        bool ok = owner[list[0]] == q;
        while (head < m && ok) {
            const int32_t c = list[head++];
            for (int k = 0; k < 4 && ok; ++k) {
                const int32_t nb = tn[4 * (int64_t)c + k];
                if (owner[nb] != q) ok = false;
                else if (cavq[nb] == q && !listed(list, m, nb)) {
                    if (m == DL_LIST) { ok = false; atomicOr(&h->err, DL_INTERNAL); }   // cannot happen: the same cavity fitted in k_grow
                    else list[m++] = nb;
                }
            }
        }
        if (!ok) { state[q] = ST_FREE; continue; }
        state[q] = ST_WON;
        for (int i = 0; i < m; ++i) cav[list[i]] = q;
        atomicAdd(&h->nwin, 1);
        atomicMax(&h->maxcav, m);
    }
}

// ---- carve -----------------------------------------------------------------------------------------------------------------------
__global__ void k_count(int32_t ncell, const int32_t* __restrict__ tv, const int32_t* __restrict__ tn, const int32_t* __restrict__ cav, int32_t* cnt,
                        int32_t* dead) {
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < ncell; c += gridDim.x * blockDim.x) {
        int k4 = 0, d = 0;
        const int32_t q = cav[c];
        if (q >= 0 && tv[4 * (int64_t)c] >= 0) {
            d = 1;
            for (int k = 0; k < 4; ++k) k4 += cav[tn[4 * (int64_t)c + k]] != q;
        }
        cnt[c] = k4;
        dead[c] = d;
    }
}

__global__ void k_deadlist(int32_t ncell, const int32_t* __restrict__ dead, const int32_t* __restrict__ doff, int32_t* deadlist) {
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < ncell; c += gridDim.x * blockDim.x)
        if (dead[c]) deadlist[doff[c]] = c;
}

__device__ __forceinline__ int32_t id_of(int32_t r, int32_t D, int32_t ncell, const int32_t* __restrict__ deadlist) {
    return r < D ? deadlist[r] : ncell + (r - D);
}

__global__ void k_create(int32_t ncell, int32_t D, const int32_t* __restrict__ tv, int32_t* tn, const int32_t* __restrict__ cav,
                         const int32_t* __restrict__ dead, const int32_t* __restrict__ off, const int32_t* __restrict__ deadlist, int32_t* newid,
                         int32_t* stv, int32_t* stn, int32_t* firstnew, DlHead* h) {
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < ncell; c += gridDim.x * blockDim.x) {
        if (!dead[c]) continue;
        const int32_t q = cav[c];
        int32_t r = off[c];
        int32_t v[4];
        for (int j = 0; j < 4; ++j) v[j] = tv[4 * (int64_t)c + j];
        for (int k = 0; k < 4; ++k) {
            const int32_t nb = tn[4 * (int64_t)c + k];
            if (cav[nb] == q) continue;
            const int32_t id = id_of(r, D, ncell, deadlist);
            newid[4 * (int64_t)c + k] = id;
            for (int j = 0; j < 4; ++j) stv[4 * (int64_t)r + j] = j == k ? q : v[j];
            stn[4 * (int64_t)r + k] = nb;
            int back = -1;   // the slot of nb whose vertex is not on the shared facet (nb is a ring cell: nobody else writes this slot)
            for (int j = 0; j < 4; ++j) {
                const int32_t w = tv[4 * (int64_t)nb + j];
                bool on = false;
                for (int i = 0; i < 4; ++i) on |= i != k && v[i] == w;
                if (!on) back = j;
            }
            if (back < 0) atomicOr(&h->err, DL_INTERNAL);
            else tn[4 * (int64_t)nb + back] = id;
            atomicMin(&firstnew[q], id);
            ++r;
        }
    }
}

__global__ void k_link(int32_t ncell, const int32_t* __restrict__ tv, const int32_t* __restrict__ tn, const int32_t* __restrict__ cav,
                       const int32_t* __restrict__ dead, const int32_t* __restrict__ off, const int32_t* __restrict__ newid, int32_t* stn, DlHead* h) {
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < ncell; c += gridDim.x * blockDim.x) {
        if (!dead[c]) continue;
        const int32_t q = cav[c];
        int32_t r = off[c];
        for (int k = 0; k < 4; ++k) {
            if (cav[tn[4 * (int64_t)c + k]] == q) continue;
            for (int j = 0; j < 4; ++j) {
                if (j == k) continue;
                // rotate about the edge of facet k that misses vertex j, away from the facet, until the cavity ends
                int32_t e1 = -1, e2 = -1;
                for (int i = 0; i < 4; ++i)
                    if (i != k && i != j) (e1 < 0 ? e1 : e2) = tv[4 * (int64_t)c + i];
                int32_t cur = c, drop = tv[4 * (int64_t)c + j], found = -1;
                for (int32_t step = 0; step <= ncell; ++step) {
                    int32_t w[4];
                    for (int i = 0; i < 4; ++i) w[i] = tv[4 * (int64_t)cur + i];
                    const int s = slot_of(w, drop);
                    if (s < 0) break;
                    const int32_t nxt = tn[4 * (int64_t)cur + s];
                    if (cav[nxt] != q) { found = newid[4 * (int64_t)cur + s]; break; }
                    int32_t t = -1;
                    for (int i = 0; i < 4; ++i)
                        if (w[i] != e1 && w[i] != e2 && w[i] != drop) t = w[i];
                    cur = nxt;
                    drop = t;
                }
                if (found < 0) {   // reported at the host's next read; the link stays a valid index until then
                    atomicOr(&h->err, DL_LOOP);
                    found = 0;
                }
                stn[4 * (int64_t)r + j] = found;
            }
            ++r;
        }
    }
}

__global__ void k_commit(int32_t ncell, int32_t N, int32_t D, const int32_t* __restrict__ deadlist, const int32_t* __restrict__ stv,
                         const int32_t* __restrict__ stn, int32_t* tv, int32_t* tn) {
    const int32_t top = N > D ? N : D;
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < top; r += gridDim.x * blockDim.x) {
        if (r < N) {
            const int32_t id = id_of(r, D, ncell, deadlist);
            for (int j = 0; j < 4; ++j) {
                tv[4 * (int64_t)id + j] = stv[4 * (int64_t)r + j];
                tn[4 * (int64_t)id + j] = stn[4 * (int64_t)r + j];
            }
        } else {   // a dead cell no new cell reuses
            const int32_t id = deadlist[r];
            for (int j = 0; j < 4; ++j) {   // (links of a dead cell stay valid indices: nothing follows them, and nothing could leave the arrays)
                tv[4 * (int64_t)id + j] = -1;
                tn[4 * (int64_t)id + j] = 0;
            }
        }
    }
}

// exact visibility walk to a cell that conflicts with q: the finite cell that holds it (closed), or the infinite cell it lies strictly beyond
__global__ void __launch_bounds__(MESH_THREADS)
k_relocate(const double* __restrict__ P, int n, int32_t ncell, int first_round, const int32_t* __restrict__ tv, const int32_t* __restrict__ tn,
           int32_t* state, int32_t* pcell, const int32_t* __restrict__ cav, const int32_t* __restrict__ firstnew, DlHead* h) {
    Ctr ctr{0, 0};
    const int32_t G = n;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x) {
        if (state[q] == ST_WON) { state[q] = ST_IN; continue; }
        if (state[q] != ST_FREE) continue;
        int32_t cur = 0;
        if (!first_round) {
            const int32_t w = cav[pcell[q]];
            if (w < 0) continue;
            cur = firstnew[w];
        }
        const V3 pq = load_v3(P, q);
        bool done = false;
        for (int64_t step = 0; step <= 4 * (int64_t)ncell + 16 && !done; ++step) {
            int32_t v[4];
            for (int j = 0; j < 4; ++j) v[j] = tv[4 * (int64_t)cur + j];
            const int g = slot_of(v, G);
            if (g >= 0) {
                if (orient_with(P, v, g, pq, ctr) > 0) done = true;
                else cur = tn[4 * (int64_t)cur + g];
                continue;
            }
            int k = 0;
            for (; k < 4; ++k)
                if (orient_with(P, v, k, pq, ctr) < 0) break;
            if (k == 4) { done = true; continue; }
            cur = tn[4 * (int64_t)cur + k];
            if (slot_of(tv + 4 * (int64_t)cur, G) >= 0) done = true;   // entered through its hull facet, strictly beyond it
        }
        if (!done) atomicOr(&h->err, DL_LOOP);
        pcell[q] = cur;
    }
    flush(h, ctr);
}

__global__ void k_fill(int32_t* p, int64_t n, int32_t v) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = v;
}

// ---- the predicate as an operation, and the certificate ------------------------------------------------------------------------------
__global__ void k_insphere(const double* __restrict__ pts, int64_t n, int8_t* __restrict__ out, unsigned long long* counts, int32_t* err) {
    Ctr ctr{0, 0};
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double* p = pts + 15 * i;
        bool ok = true;
        for (int j = 0; j < 15; ++j) ok &= dgnn_exact::insphere_coord_ok(p[j]);   // (NaN and infinities fail it too)
        if (!ok) { atomicOr(err, DL_RANGE); out[i] = 0; continue; }
        int ei = 0, eo = 0;
        out[i] = (int8_t)dgnn_exact::insphere_sign(V3{p[0], p[1], p[2]}, V3{p[3], p[4], p[5]}, V3{p[6], p[7], p[8]}, V3{p[9], p[10], p[11]},
                                                   V3{p[12], p[13], p[14]}, &ei, &eo);
        ctr.in += ei;
        ctr.orient += eo;
    }
    if (ctr.in) atomicAdd(&counts[0], (unsigned long long)ctr.in);
    if (ctr.orient) atomicAdd(&counts[1], (unsigned long long)ctr.orient);
}

enum { VI_FLAT = 0, VI_NEGATIVE, VI_NONLOCAL, VI_CONCAVE, VI_BAD_LINK, VI_N };

// one thread per (cell, slot) of any cell list with its neighbour table (-1 = no cell across)
__global__ void __launch_bounds__(MESH_THREADS)
k_violations(const double* __restrict__ P, int64_t nv, const int32_t* __restrict__ tets, const int32_t* __restrict__ nbr, int64_t nt,
             unsigned long long* counts, int32_t* err) {
    unsigned long long loc[VI_N] = {0, 0, 0, 0, 0};
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < 4 * nt; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = i >> 2;
        const int k = (int)(i & 3);
        int32_t v[4];
        bool ok = true;
        for (int j = 0; j < 4; ++j) {
            v[j] = tets[4 * c + j];
            ok &= v[j] >= 0 && v[j] < nv;
        }
        const int32_t nb = nbr[i];
        ok &= nb >= -1 && nb < nt;
        if (!ok) { atomicOr(err, DL_INTERNAL); continue; }
        const V3 a = load_v3(P, v[0]), b = load_v3(P, v[1]), cc = load_v3(P, v[2]), d = load_v3(P, v[3]);
        const int o = dgnn_exact::orient_sign(a, b, cc, d);
        if (k == 0) {
            loc[VI_FLAT] += o == 0;
            loc[VI_NEGATIVE] += o < 0;
        }
        if (nb >= 0) {
            if (c > nb) continue;   // an interior facet is tested once, from its lower cell
            int32_t opp = -1;
            for (int j = 0; j < 4; ++j) {
                const int32_t w = tets[4 * (int64_t)nb + j];
                bool on = false;
                for (int m = 0; m < 4; ++m) on |= m != k && v[m] == w;
                if (!on) opp = opp < 0 ? w : -2;
            }
            if (opp < 0 || opp >= nv) { ++loc[VI_BAD_LINK]; continue; }
            if (dgnn_exact::insphere_sign(a, b, cc, d, load_v3(P, opp)) > 0) ++loc[VI_NONLOCAL];
            continue;
        }
        if (o == 0) continue;
        for (int j = 0; j < 4; ++j) {   // the hull edge of facet k that misses vertex j: find the hull facet on its other side
            if (j == k) continue;
            int32_t e1 = -1, e2 = -1;
            for (int m = 0; m < 4; ++m)
                if (m != k && m != j) (e1 < 0 ? e1 : e2) = v[m];
            int64_t cur = c;
            int32_t drop = v[j], apex = -1;
            for (int64_t step = 0; step <= nt; ++step) {
                int32_t w[4];
                for (int m = 0; m < 4; ++m) w[m] = tets[4 * cur + m];
                const int s = slot_of(w, drop);
                if (s < 0) break;
                int32_t t = -1;
                for (int m = 0; m < 4; ++m)
                    if (w[m] != e1 && w[m] != e2 && w[m] != drop) t = w[m];
                const int32_t nxt = nbr[4 * cur + s];
                if (nxt < 0) { apex = t; break; }
                if (nxt >= nt || t < 0) break;
                cur = nxt;
                drop = t;
            }
            if (apex < 0 || apex >= nv) { ++loc[VI_BAD_LINK]; continue; }
            V3 w4[4] = {a, b, cc, d};
            w4[k] = load_v3(P, apex);
            if (dgnn_exact::orient_sign(w4[0], w4[1], w4[2], w4[3]) * o < 0) ++loc[VI_CONCAVE];   // the other facet's apex lies strictly beyond this facet
        }
    }
    for (int j = 0; j < VI_N; ++j)
        if (loc[j]) atomicAdd(&counts[j], loc[j]);
}

struct DlLayout {
    DlHead* head;
    int32_t *cand, *owner, *cavq, *cav, *mark, *cnt, *off, *dead, *doff, *deadlist, *newid, *stv, *stn, *sums, *pcell, *state, *firstnew;
    int64_t bytes;
};

DlLayout dl_layout(char* base, int64_t n, int64_t cap) {
    Take t{base, 0};
    DlLayout L;
    L.head = t.take<DlHead>(1);
    L.cand = t.take<int32_t>(cap);
    L.owner = t.take<int32_t>(cap);
    L.cavq = t.take<int32_t>(cap);
    L.cav = t.take<int32_t>(cap);
    L.mark = t.take<int32_t>(cap);
    L.cnt = t.take<int32_t>(cap + 1);
    L.off = t.take<int32_t>(cap + 2);
    L.dead = t.take<int32_t>(cap + 1);
    L.doff = t.take<int32_t>(cap + 2);
    L.deadlist = t.take<int32_t>(cap);
    L.newid = t.take<int32_t>(4 * cap);
    L.stv = t.take<int32_t>(4 * cap);
    L.stn = t.take<int32_t>(4 * cap);
    L.sums = t.take<int32_t>(dgnn_cdiv(cap + 1, 2048) + 4);
    L.pcell = t.take<int32_t>(n);
    L.state = t.take<int32_t>(n);
    L.firstnew = t.take<int32_t>(n);
    L.bytes = t.off;
    return L;
}

bool dl_sizes_ok(int64_t n, int64_t cap) { return n >= 4 && n < INT32_MAX / 8 && cap >= 5 && cap < INT32_MAX / 4; }

}  // namespace

// ================================================================================================================================
extern "C" int64_t dgnn_delaunay_default_capacity(int64_t n) { return 8 * n + 64; }

extern "C" int64_t dgnn_delaunay_scratch_bytes(int64_t n, int64_t cell_capacity) {
    return dl_sizes_ok(n, cell_capacity) ? dl_layout(nullptr, n, cell_capacity).bytes : 0;
}

#define DL_LAUNCH(kernel, count, ...) hipLaunchKernelGGL(kernel, mesh_launch_grid(count), dim3(MESH_THREADS), 0, stream, __VA_ARGS__)

extern "C" int dgnn_delaunay(const double* points, int64_t n, int64_t cell_capacity, int32_t* cells_out, int32_t* neighbors_out, int64_t* stats_out,
                             void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(n >= 4, DGNN_E_INVALID, "delaunay: %lld points, at least 4 are needed", (long long)n);
    DGNN_REQUIRE(dl_sizes_ok(n, cell_capacity), DGNN_E_UNSUPPORTED, "delaunay: sizes exceed the int32 indexing (or a capacity below 5)");
    DGNN_REQUIRE(points && cells_out && neighbors_out && stats_out && scratch, DGNN_E_INVALID, "delaunay: bad args");
    const DlLayout L = dl_layout((char*)scratch, n, cell_capacity);
    int32_t *tv = cells_out, *tn = neighbors_out;
    const int32_t ni = (int32_t)n, cap = (int32_t)cell_capacity;
    for (int i = 0; i < DGNN_DELAUNAY_N_STATS; ++i) stats_out[i] = 0;
    int rc;
    DlHead hh;

    auto read_head = [&](const char* what) -> int {
        if ((rc = mm_read(&hh, L.head, sizeof(DlHead), stream, what))) return rc;
        stats_out[DGNN_DELAUNAY_EXACT_INSPHERE] = (int64_t)hh.ex_insphere;
        stats_out[DGNN_DELAUNAY_EXACT_ORIENT] = (int64_t)hh.ex_orient;
        if (hh.err & DL_NONFINITE) { dgnn_set_error("delaunay: a coordinate is not finite"); return DGNN_E_INVALID; }
        if (hh.err & DL_RANGE) {
            dgnn_set_error("delaunay: a coordinate outside the exact predicates' range (0 or a magnitude in [2^-150, 2^150])");
            return DGNN_E_UNSUPPORTED;
        }
        if (hh.err & DL_DUP) {
            stats_out[DGNN_DELAUNAY_DUP_A] = (int64_t)(hh.dup >> 32);
            stats_out[DGNN_DELAUNAY_DUP_B] = (int64_t)(hh.dup & 0xffffffffull);
            dgnn_set_error("delaunay: a duplicate point (priority ranks %lld and %lld)", (long long)stats_out[DGNN_DELAUNAY_DUP_B],
                           (long long)stats_out[DGNN_DELAUNAY_DUP_A]);
            return DGNN_E_DUPLICATE;
        }
        if (hh.err & DL_LOOP) { dgnn_set_error("delaunay: a device loop reached its cap (%s)", what); return DGNN_E_UNSUPPORTED; }
        if (hh.err) { dgnn_set_error("delaunay: inconsistent cells (%s)", what); return DGNN_E_UNSUPPORTED; }
        return DGNN_OK;
    };

    (void)hipMemsetAsync(L.head, 0, sizeof(DlHead), stream);
    (void)hipMemsetAsync(L.state, 0, sizeof(int32_t) * n, stream);
    (void)hipMemsetAsync(L.pcell, 0, sizeof(int32_t) * n, stream);
    DL_LAUNCH(k_fill, n, L.firstnew, n, DL_INF);
    DL_LAUNCH(k_fill, 1, &L.head->i2, (int64_t)2, DL_INF);   // i2 and i3 lie side by side
    DL_LAUNCH(k_fill, 1, (int32_t*)&L.head->dup, (int64_t)2, -1);
    DL_LAUNCH(k_check_points, 3 * n, points, 3 * n, L.head);
    if ((rc = read_head("the input check"))) return rc;
    DL_LAUNCH(k_find_i2, n, points, ni, L.head);
    if ((rc = read_head("the start search"))) return rc;
    if (hh.i2 != DL_INF) {
        DL_LAUNCH(k_find_i3, n, points, ni, L.head);
        if ((rc = read_head("the start search"))) return rc;
    }
    if (hh.i2 == DL_INF || hh.i3 == DL_INF) {
        dgnn_set_error("delaunay: all %lld points are %s", (long long)n, hh.i2 == DL_INF ? "collinear" : "coplanar");
        return DGNN_E_DEGENERATE;
    }
    hipLaunchKernelGGL(k_init, dim3(1), dim3(64), 0, stream, points, ni, tv, tn, L.state, L.head);
    int32_t ncell = 5;
    DL_LAUNCH(k_relocate, n, points, ni, ncell, 1, tv, tn, L.state, L.pcell, L.cav, L.firstnew, L.head);
    if ((rc = read_head("the first location"))) return rc;

    int64_t inserted = 4, rounds = 0, win_min = INT64_MAX, win_max = 0, maxcav = 0, big_runs = 0;
    while (inserted < n) {
        if (rounds >= n) { dgnn_set_error("delaunay: %lld rounds without finishing", (long long)rounds); return DGNN_E_UNSUPPORTED; }
        ++rounds;
        DL_LAUNCH(k_reset, ncell, ncell, L.cand, L.owner, L.cavq, L.cav, L.mark, L.head);
        DL_LAUNCH(k_pick, n, ni, L.state, L.pcell, L.cand);
        DL_LAUNCH(k_grow, n, points, ni, tv, tn, L.state, L.pcell, L.cand, L.owner, L.cavq, L.head);
        if ((rc = read_head("cavity growth"))) return rc;
        if (hh.bigmin != DL_INF) {
            ++big_runs;
            hipLaunchKernelGGL(k_big_seed, dim3(1), dim3(64), 0, stream, L.pcell, L.mark, L.head);
            for (int64_t sweep = 0;; ++sweep) {
                if (sweep > ncell) { dgnn_set_error("delaunay: the slow path's sweeps reached their cap"); return DGNN_E_UNSUPPORTED; }
                DL_LAUNCH(k_fill, 1, &L.head->changed, (int64_t)1, 0);
                DL_LAUNCH(k_big_sweep, ncell, points, ni, ncell, tv, tn, L.cand, L.mark, L.head);
                if ((rc = read_head("the slow path"))) return rc;
                if (!hh.changed || hh.biglose) break;
            }
            DL_LAUNCH(k_big_claim, ncell, ncell, L.mark, L.owner, L.cavq, L.head);
            DL_LAUNCH(k_big_verify, ncell, ncell, L.mark, L.owner, L.head);
            DL_LAUNCH(k_big_commit, ncell, ncell, L.mark, L.cav, L.state, L.head);
        }
        DL_LAUNCH(k_verify, n, ni, tn, L.state, L.pcell, L.owner, L.cavq, L.cav, L.head);
        DL_LAUNCH(k_count, ncell, ncell, tv, tn, L.cav, L.cnt, L.dead);
        if ((rc = dgnn_exclusive_scan_i32(L.cnt, ncell, L.off, L.sums, stream))) return rc;
        if ((rc = dgnn_exclusive_scan_i32(L.dead, ncell, L.doff, L.sums, stream))) return rc;
        DL_LAUNCH(k_deadlist, ncell, ncell, L.dead, L.doff, L.deadlist);
        int32_t tot[2];
        (void)hipMemcpyAsync(&tot[0], L.off + ncell, sizeof(int32_t), hipMemcpyDeviceToHost, stream);
        (void)hipMemcpyAsync(&tot[1], L.doff + ncell, sizeof(int32_t), hipMemcpyDeviceToHost, stream);
        if ((rc = read_head("the verification"))) return rc;
        const int32_t N = tot[0], D = tot[1];
        if (hh.nwin <= 0 || N <= 0) { dgnn_set_error("delaunay: a round inserted no point"); return DGNN_E_UNSUPPORTED; }
        const int64_t next = (int64_t)ncell + (N > D ? N - D : 0);
        if (next > cap) {
            stats_out[DGNN_DELAUNAY_NEED] = next;
            dgnn_set_error("delaunay: %lld cells needed, the capacity is %d", (long long)next, cap);
            return DGNN_E_CAPACITY;
        }
        DL_LAUNCH(k_create, ncell, ncell, D, tv, tn, L.cav, L.dead, L.off, L.deadlist, L.newid, L.stv, L.stn, L.firstnew, L.head);
        DL_LAUNCH(k_link, ncell, ncell, tv, tn, L.cav, L.dead, L.off, L.newid, L.stn, L.head);
        DL_LAUNCH(k_commit, N > D ? N : D, ncell, N, D, L.deadlist, L.stv, L.stn, tv, tn);
        ncell = (int32_t)next;
        DL_LAUNCH(k_relocate, n, points, ni, ncell, 0, tv, tn, L.state, L.pcell, L.cav, L.firstnew, L.head);
        inserted += hh.nwin;
        win_min = hh.nwin < win_min ? hh.nwin : win_min;
        win_max = hh.nwin > win_max ? hh.nwin : win_max;
        const int64_t cavmax = hh.maxcav > hh.bigcav ? hh.maxcav : hh.bigcav;
        maxcav = cavmax > maxcav ? cavmax : maxcav;
    }
    if ((rc = read_head("the last round"))) return rc;
    stats_out[DGNN_DELAUNAY_ROUNDS] = rounds;
    stats_out[DGNN_DELAUNAY_WIN_MIN] = rounds ? win_min : 0;
    stats_out[DGNN_DELAUNAY_WIN_MAX] = win_max;
    stats_out[DGNN_DELAUNAY_MAX_CAVITY] = maxcav;
    stats_out[DGNN_DELAUNAY_CELLS] = ncell;
    stats_out[DGNN_DELAUNAY_SLOW_PATHS] = big_runs;
    return DGNN_OK;
}

extern "C" int dgnn_insphere_sign(const double* points5, int64_t n, int8_t* sign_out, int64_t* exact_out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(n >= 0 && n < INT32_MAX && exact_out && (n == 0 || (points5 && sign_out)), DGNN_E_INVALID, "insphere_sign: bad args");
    // exact_out: int64 [3] on the device: exact-stage calls of the in-sphere determinant, of the orientation, and the error word
    (void)hipMemsetAsync(exact_out, 0, 3 * sizeof(int64_t), stream);
    if (n > 0) DL_LAUNCH(k_insphere, n, points5, n, sign_out, (unsigned long long*)exact_out, (int32_t*)(exact_out + 2));
    int64_t h[3];
    int rc;
    if ((rc = mm_read(h, exact_out, sizeof(h), stream, "insphere_sign"))) return rc;
    DGNN_REQUIRE(h[2] == 0, DGNN_E_UNSUPPORTED, "insphere_sign: a coordinate outside the exact range (0 or a magnitude in [2^-150, 2^150])");
    return DGNN_OK;
}

extern "C" int dgnn_delaunay_violations(const double* vertices, int64_t n_vertices, const int32_t* tetrahedra, const int32_t* neighbors, int64_t n_tets,
                                        int64_t* counts_out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(n_tets >= 0 && n_tets < INT32_MAX / 4 && n_vertices >= 0 && n_vertices < INT32_MAX, DGNN_E_UNSUPPORTED,
                 "delaunay_violations: sizes exceed the int32 indexing");
    DGNN_REQUIRE(counts_out && (n_tets == 0 || (vertices && tetrahedra && neighbors)), DGNN_E_INVALID, "delaunay_violations: bad args");
    // counts_out: int64 [DGNN_VIOLATION_N + 1] on the device, the last word is the error word
    (void)hipMemsetAsync(counts_out, 0, (VI_N + 1) * sizeof(int64_t), stream);
    if (n_tets > 0)
        DL_LAUNCH(k_violations, 4 * n_tets, vertices, n_vertices, tetrahedra, neighbors, n_tets, (unsigned long long*)counts_out,
                  (int32_t*)(counts_out + VI_N));
    int64_t h[VI_N + 1];
    int rc;
    if ((rc = mm_read(h, counts_out, sizeof(h), stream, "delaunay_violations"))) return rc;
    DGNN_REQUIRE(h[VI_N] == 0, DGNN_E_INVALID, "delaunay_violations: a vertex or cell id out of range");
    return DGNN_OK;
}
