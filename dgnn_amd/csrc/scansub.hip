// Subsampling a scan before it is triangulated (ops.voxel_subsample, ops.min_distance_thin): one point per occupied voxel, and the exact
// minimum-distance (Poisson-disk) thinning.  DESIGN §35; the contract is in include/dgnn_hip.h.  Everything is fp64 and every product, sum,
// difference and division rounds on its own (-ffp-contract=off).  Both results are functions of the input alone: no float is added by an
// atomic, and what the atomics do order (the records inside a cell, the compacted lists) no result depends on.
//
// voxel grid
//   key        c_a = floor(fl(fl(x_a - o_a) / h)), refused unless |c_a| < 2^20; the 63-bit key is the three c_a + 2^20 side by side.
//   voxels     a stable LSD radix sort of (key, index) pairs (reorder.hip's): a voxel is a run of equal keys, its members in ascending
//              index, the run's head its lowest member.  is_first[i] = 1 at those members; an exclusive scan of it over the POINT indices
//              numbers the voxels by first member.
//   centroid   one wavefront per voxel.  The 64 lanes load 64 members; every lane then adds them in member order (a shuffle per member), so
//              the sum is the serial one; after every 256 members the chunk's sum is added to the total (fixed_sum.h's order).
//   nearest    the lanes take the members 64 at a time, each keeps its smallest (d2, index), a butterfly takes the wave's.
//
// thinning
//   rule       r2 = fl(r r); i and j conflict iff d2(i, j) < r2, d2 = (dx dx + dy dy) + dz dz (point_grid.h's; dx = x_i - x_j and its negation
//              square alike: symmetric in its bits).  The order is (key_i, i); the kept set is the lexicographically first maximal independent
//              set of the conflict graph.
//   rank       the same stable sort on (key_i, i) gives every point its rank in the order, an int32 that rides in the record's free word:
//              "j is earlier than i" is one integer compare.
//   rounds     state per point: undecided / kept / removed.  A round takes every undecided i (a compacted list, one wavefront each), reads its
//              earlier conflicting j, and: any kept -> i is removed (a ballot ends the point there); none undecided -> i is kept; else i goes
//              on the next list.  States move only from undecided to final, and a final state is the sequential greedy's (induction along
//              the order), so stale or in-round reads (relaxed atomic loads) only delay a decision.  The earliest undecided point has no
//              undecided earlier conflict: every round decides it, and the loop ends.  The host launches THIN_ROUNDS_PER_READ rounds, then
//              reads the list's length back; three length counters rotate (read / appended to / zeroed for the round after).
//   grid       point_grid.h's records.  Point i reads the cells grid_cell(x_a - r') .. grid_cell(x_a + r') on each axis, r' = fl(r THIN_WIDEN).
//              Why that holds every conflict: a conflict has fl(dx dx) <= d2 < fl(r r) (sums of non-negative terms and rounding are monotone),
//              so dx^2 < r^2 by the monotonicity of rounding again: |fl(x_i - x_j)| < r with NO margin.  The true difference is within
//              (1 + 2 u) of the rounded one (u = 2^-53; a difference below 2^-1021 is exact), so x_j < x_i + r (1 + 2 u) <= x_i + r' in the
//              reals once r' >= r (1 + 2 u), and then fl(x_i + r') >= fl(x_j) = x_j, and grid_cell, a chain of monotone steps, maps x_j to a
//              cell no higher than that of fl(x_i + r') (the same below).  The need is 2 u plus one rounding of r THIN_WIDEN, 3 u;
//              THIN_WIDEN = 1 + 2^-46 = 1 + 128 u.  A radius below 2^-1021, whose product may round back to r, meets only exact differences.
//              Nothing here uses the size of a cell: the answer is the all-pairs answer at every resolution.
//   all pairs  grid_resolution = 0: the points in tiles of 256 through LDS with their ranks, four undecided points (waves) per block.
#include <math.h>

#include "fixed_sum.h"
#include "mesh_faces.h"
#include "mix64.h"
#include "point_grid.h"

namespace {

__device__ __forceinline__ bool sub_less(double a, int32_t ia, double b, int32_t ib) { return a < b || (a == b && ia < ib); }

__global__ void k_sub_iota(int32_t* __restrict__ x, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) x[i] = (int32_t)i;
}

// ---- voxel grid -----------------------------------------------------------------------------------------------------------------------------
constexpr int32_t VOX_NONFINITE = 1, VOX_RANGE = 2;
constexpr double VOX_LIMIT = 0x1p20;          // |c_a| below it: three 21-bit fields
constexpr int VOX_WAVES = MESH_THREADS / DGNN_WAVE;

struct Origin { double o[3]; };

__global__ void k_vox_keys(const double* __restrict__ p, int64_t n, double h, Origin org, uint64_t* __restrict__ keys, int32_t* __restrict__ vals,
                           int32_t* err) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        uint64_t key = 0;
        int32_t e = 0;
        for (int a = 0; a < 3; ++a) {
            const double x = p[3 * i + a];
            if (!isfinite(x)) { e |= VOX_NONFINITE; continue; }
            const double c = floor((x - org.o[a]) / h);
            if (!(fabs(c) < VOX_LIMIT)) { e |= VOX_RANGE; continue; }
            key = (key << 21) | (uint64_t)((int64_t)c + (int64_t)VOX_LIMIT);
        }
        if (e) atomicOr(err, e);
        keys[i] = key;
        vals[i] = (int32_t)i;
    }
}

// the sorted pairs: head[i] = position i opens a run of equal keys; is_first (zeroed) = 1 at the run's lowest member
__global__ void k_vox_heads(const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals, int64_t n, int32_t* __restrict__ head,
                            int32_t* __restrict__ is_first) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t h = (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
        head[i] = h;
        if (h) is_first[vals[i]] = 1;
    }
}

// run_start[r] = the position that opens run r (hscan: the exclusive scan of head)
__global__ void k_vox_starts(const int32_t* __restrict__ head, const int32_t* __restrict__ hscan, int64_t n, int32_t* __restrict__ run_start) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        if (head[i]) run_start[hscan[i]] = (int32_t)i;
}

// vrank: the exclusive scan of is_first over the point indices = the voxel's row.  Every run index is below the number of runs <= n, every
// row below it too.
__global__ void k_vox_rows(const int32_t* __restrict__ vals, const int32_t* __restrict__ head, const int32_t* __restrict__ hscan,
                           const int32_t* __restrict__ vrank, const int32_t* __restrict__ run_start, int64_t n, int32_t* __restrict__ voxel,
                           int32_t* __restrict__ first, int32_t* __restrict__ count, int32_t* __restrict__ vstart) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t s = run_start[hscan[i] + head[i] - 1];
        const int32_t v = vrank[vals[s]];
        voxel[vals[i]] = v;
        if (head[i]) {
            first[v] = vals[i];
            vstart[v] = (int32_t)i;
        }
        if (i == n - 1 || head[i + 1]) count[v] = (int32_t)(i - s) + 1;
    }
}

// one wavefront per voxel: its members are vals[vstart[v] .. + count[v]), ascending
__global__ void __launch_bounds__(MESH_THREADS) k_vox_centroid(const double* __restrict__ p, const int32_t* __restrict__ vals,
                                                             const int32_t* __restrict__ vstart, const int32_t* __restrict__ count,
                                                             const int32_t* __restrict__ m_dev, double* __restrict__ centroid,
                                                             int32_t* __restrict__ nearest, int64_t* __restrict__ m_out) {
    const int64_t m = *m_dev;
    if (blockIdx.x == 0 && threadIdx.x == 0) *m_out = m;
    const int lane = lane_id();
    for (int64_t v = (int64_t)blockIdx.x * VOX_WAVES + wave_id_uniform(); v < m; v += (int64_t)gridDim.x * VOX_WAVES) {
        const int32_t s0 = vstart[v], cnt = count[v];
        double acc[3] = {0.0, 0.0, 0.0}, s[3] = {0.0, 0.0, 0.0};
        for (int32_t b = 0; b < cnt; b += DGNN_WAVE) {
            const bool in = b + lane < cnt;
            const int64_t id = in ? vals[s0 + b + lane] : 0;
            const double x = in ? p[3 * id] : 0.0, y = in ? p[3 * id + 1] : 0.0, z = in ? p[3 * id + 2] : 0.0;
            const int lim = cnt - b < DGNN_WAVE ? cnt - b : DGNN_WAVE;
            for (int l = 0; l < lim; ++l) {
                s[0] += __shfl(x, l);
                s[1] += __shfl(y, l);
                s[2] += __shfl(z, l);
            }
            if ((b + DGNN_WAVE) % FIXED_SUM_CHUNK == 0 || b + DGNN_WAVE >= cnt)          // the chunk of 256 members ends here
                for (int a = 0; a < 3; ++a) { acc[a] += s[a]; s[a] = 0.0; }
        }
        const double c[3] = {acc[0] / (double)cnt, acc[1] / (double)cnt, acc[2] / (double)cnt};
        double bd = INFINITY;
        int32_t bi = INT32_MAX;
        for (int32_t b = 0; b < cnt; b += DGNN_WAVE) {
            if (b + lane < cnt) {
                const int32_t id = vals[s0 + b + lane];
                const double d2 = knn_d2(c, p[3 * (int64_t)id], p[3 * (int64_t)id + 1], p[3 * (int64_t)id + 2]);
                if (sub_less(d2, id, bd, bi)) { bd = d2; bi = id; }
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double od = __shfl_xor(bd, o);
            const int32_t oi = __shfl_xor(bi, o);
            if (sub_less(od, oi, bd, bi)) { bd = od; bi = oi; }
        }
        if (lane == 0) {
            centroid[3 * v] = c[0];
            centroid[3 * v + 1] = c[1];
            centroid[3 * v + 2] = c[2];
            nearest[v] = bi == INT32_MAX ? vals[s0] : bi;          // every d2 a NaN (the sums overflowed both ways): the first member
        }
    }
}

struct VoxLayout { int32_t *err, *head, *hscan, *is_first, *vrank, *run_start, *vstart, *sums; SortBufs sort; int64_t bytes; };
VoxLayout vox_layout(void* base, int64_t n) {
    Take t{(char*)base, 256};
    VoxLayout L{};
    L.err = (int32_t*)base;
    take_sort(t, n, L.sort);
    L.head = t.take<int32_t>(n + 1);
    L.hscan = t.take<int32_t>(n + 1);
    L.is_first = t.take<int32_t>(n + 1);
    L.vrank = t.take<int32_t>(n + 1);
    L.run_start = t.take<int32_t>(n);
    L.vstart = t.take<int32_t>(n);
    L.sums = t.take<int32_t>(dgnn_cdiv(n + 1, 2048) + 2);
    L.bytes = t.off;
    return L;
}

// ---- thinning -------------------------------------------------------------------------------------------------------------------------------
constexpr double THIN_WIDEN = 1.0 + 0x1p-46;          // of r: 128 u against a need of 3 u (the derivation is above)
constexpr int32_t THIN_UNDECIDED = 0, THIN_KEPT = 1, THIN_REMOVED = 2;
constexpr int THIN_ROUNDS_PER_READ = 4;
constexpr int THIN_WAVES = MESH_THREADS / DGNN_WAVE, THIN_TILE = 256;
constexpr uint64_t THIN_GOLDEN = 0x9E3779B97F4A7C15ull;
enum { THIN_N_KEPT = 0, THIN_ROUNDS, THIN_CANDIDATES, THIN_N_OUT };

struct ThinState {
    PointBox box;
    uint32_t cnt[3], pad;          // the lengths of the lists: round t reads cnt[t % 3], appends under cnt[(t + 1) % 3], zeroes cnt[(t + 2) % 3]
    unsigned long long out[THIN_N_OUT];
};
static_assert(sizeof(ThinState) <= 256, "ThinState must fit the first scratch slot");

// the order's keys as unsigned: a priority with its sign bit turned, or the hash of (seed, i)
__global__ void k_thin_keys(int64_t n, const int64_t* __restrict__ priority, uint64_t seed, uint64_t* __restrict__ keys, int32_t* __restrict__ vals) {
    const uint64_t base = mix64(seed + THIN_GOLDEN);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        keys[i] = priority ? ((uint64_t)priority[i] ^ 0x8000000000000000ull) : mix64(base + (uint64_t)i);
        vals[i] = (int32_t)i;
    }
}

__global__ void k_thin_rank(const int32_t* __restrict__ vals, int64_t n, int32_t* __restrict__ rank) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) rank[vals[i]] = (int32_t)i;
}

__device__ __forceinline__ int32_t thin_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void thin_store(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the round's bookkeeping, by one thread: the counter of the round after next, the rounds that had work
__device__ __forceinline__ uint32_t thin_begin(ThinState* st, int t) {
    const uint32_t count = st->cnt[t % 3];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->cnt[(t + 2) % 3] = 0;
        if (count) st->out[THIN_ROUNDS] += 1;
    }
    return count;
}

// what the wave found about its point `id` (list entry `entry`)
__device__ __forceinline__ void thin_decide(bool removed, bool pending, int32_t id, int32_t entry, int32_t* state, int32_t* __restrict__ list_dst,
                                            ThinState* st, int t) {
    if (lane_id() != 0) return;
    if (removed) thin_store(state + id, THIN_REMOVED);
    else if (!pending) thin_store(state + id, THIN_KEPT);
    else list_dst[atomicAdd(&st->cnt[(t + 1) % 3], 1u)] = entry;          // at most the source list's length: below n
}

// the lanes' candidates (valid: the lane has one, an earlier conflicting point j) -> true: a kept one, the point is removed
__device__ __forceinline__ bool thin_look(bool valid, int32_t j, const int32_t* state, bool& pending) {
    const int32_t s = valid ? thin_load(state + j) : THIN_REMOVED;
    if (__ballot(valid && s == THIN_KEPT)) return true;
    pending = pending || __ballot(valid && s == THIN_UNDECIDED) != 0;
    return false;
}

// list entries: record slots
__global__ void __launch_bounds__(MESH_THREADS) k_thin_round_grid(const KnnPoint* __restrict__ rec, const int32_t* __restrict__ rowptr, CellGrid G,
                                                                double r2, double rw, int32_t* state, const int32_t* __restrict__ list_src,
                                                                int32_t* __restrict__ list_dst, ThinState* st, int t) {
    const uint32_t count = thin_begin(st, t);
    const int lane = lane_id();
    unsigned long long cands = 0;
    for (int64_t w = (int64_t)blockIdx.x * THIN_WAVES + wave_id_uniform(); w < count; w += (int64_t)gridDim.x * THIN_WAVES) {
        const int32_t slot = list_src[w];
        const KnnPoint me = rec[slot];
        const double q[3] = {me.x, me.y, me.z};
        int32_t c0[3], c1[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            c0[a] = grid_cell(G, a, q[a] - rw);
            c1[a] = grid_cell(G, a, q[a] + rw);
        }
        bool removed = false, pending = false;
        for (int32_t x = c0[0]; x <= c1[0] && !removed; ++x)
            for (int32_t y = c0[1]; y <= c1[1] && !removed; ++y) {
                const int64_t col = ((int64_t)x * G.n[1] + y) * G.n[2];          // the column's cells c0[2] .. c1[2] are one run of records
                const int32_t beg = rowptr[col + c0[2]], end = rowptr[col + c1[2] + 1];
                for (int32_t b = beg; b < end && !removed; b += DGNN_WAVE) {
                    const bool in = b + lane < end;
                    KnnPoint p{0.0, 0.0, 0.0, 0, 0};
                    if (in) p = rec[b + lane];
                    cands += (unsigned long long)(end - b < DGNN_WAVE ? end - b : DGNN_WAVE);
                    removed = thin_look(in && p.pad < me.pad && knn_d2(q, p.x, p.y, p.z) < r2, p.id, state, pending);
                }
            }
        thin_decide(removed, pending, me.id, slot, state, list_dst, st, t);
    }
    if (lane == 0 && cands) atomicAdd(&st->out[THIN_CANDIDATES], cands);
}

// list entries: point indices
__global__ void __launch_bounds__(MESH_THREADS) k_thin_round_all_pairs(const double* __restrict__ points, const int32_t* __restrict__ rank, int64_t n,
                                                                     double r2, int32_t* state, const int32_t* __restrict__ list_src,
                                                                     int32_t* __restrict__ list_dst, ThinState* st, int t) {
    __shared__ double tile[3 * THIN_TILE];
    __shared__ int32_t tile_rank[THIN_TILE];
    const uint32_t count = thin_begin(st, t);
    const int lane = lane_id(), wave = wave_id_uniform();
    unsigned long long cands = 0;
    for (int64_t base = (int64_t)blockIdx.x * THIN_WAVES; base < count; base += (int64_t)gridDim.x * THIN_WAVES) {
        const int64_t w = base + wave;
        const bool active = w < count;
        const int32_t id = active ? list_src[w] : 0;
        const double q[3] = {points[3 * (int64_t)id], points[3 * (int64_t)id + 1], points[3 * (int64_t)id + 2]};
        const int32_t my_rank = rank[id];
        bool removed = false, pending = false;
        for (int64_t t0 = 0; t0 < n; t0 += THIN_TILE) {
            const int cnt = (int)(n - t0 < THIN_TILE ? n - t0 : THIN_TILE);
            __syncthreads();
            for (int i = threadIdx.x; i < 3 * cnt; i += MESH_THREADS) tile[i] = points[3 * t0 + i];
            for (int i = threadIdx.x; i < cnt; i += MESH_THREADS) tile_rank[i] = rank[t0 + i];
            __syncthreads();
            if (active && !removed)
                for (int c = 0; c < cnt && !removed; c += DGNN_WAVE) {
                    const int i = c + lane;
                    const bool in = i < cnt;
                    const bool conflict = in && tile_rank[i] < my_rank && knn_d2(q, tile[3 * i], tile[3 * i + 1], tile[3 * i + 2]) < r2;
                    cands += (unsigned long long)(cnt - c < DGNN_WAVE ? cnt - c : DGNN_WAVE);
                    removed = thin_look(conflict, (int32_t)(t0 + i), state, pending);
                }
        }
        if (active) thin_decide(removed, pending, id, id, state, list_dst, st, t);
    }
    if (lane == 0 && cands) atomicAdd(&st->out[THIN_CANDIDATES], cands);
}

__global__ void __launch_bounds__(MESH_THREADS) k_thin_finish(const int32_t* __restrict__ state, int64_t n, uint8_t* __restrict__ keep, ThinState* st) {
    unsigned long long kept = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const bool k = state[i] == THIN_KEPT;
        keep[i] = k ? 1 : 0;
        kept += k ? 1 : 0;
    }
    wave_add_atomic(kept, &st->out[THIN_N_KEPT]);
}

struct ThinLayout { ThinState* st; SortBufs sort; int32_t *rank, *state, *list[2]; PointBins bins; int64_t bytes; };
ThinLayout thin_layout(void* base, int64_t n, int64_t R) {
    Take t{(char*)base, 256};
    ThinLayout L{};
    L.st = (ThinState*)base;
    take_sort(t, n, L.sort);
    L.rank = t.take<int32_t>(n);
    L.state = t.take<int32_t>(n);
    L.list[0] = t.take<int32_t>(n);
    L.list[1] = t.take<int32_t>(n);
    if (R > 0) L.bins = take_point_bins(t, n, R);
    L.bytes = t.off;
    return L;
}

}  // namespace

// ================================================================================================================================
extern "C" int64_t dgnn_voxel_subsample_scratch_bytes(int64_t n) { return n < 0 ? 256 : vox_layout(nullptr, n).bytes; }

extern "C" int dgnn_voxel_subsample(const double* points, int64_t n, double h, const double* origin, int32_t* voxel_out, int32_t* count_out,
                                    int32_t* first_out, double* centroid_out, int32_t* nearest_out, int64_t* m_out, void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(scratch && origin && m_out && n >= 0 && (n == 0 || (points && voxel_out && count_out && first_out && centroid_out && nearest_out)),
                 DGNN_E_INVALID, "voxel_subsample: bad args");
    DGNN_REQUIRE(isfinite(h) && h > 0.0, DGNN_E_INVALID, "voxel_subsample: the voxel size %g is not a finite positive number", h);
    DGNN_REQUIRE(isfinite(origin[0]) && isfinite(origin[1]) && isfinite(origin[2]), DGNN_E_INVALID, "voxel_subsample: a non-finite origin");
    DGNN_REQUIRE(n < INT32_MAX, DGNN_E_UNSUPPORTED, "voxel_subsample: sizes exceed the int32 indexing");
    if (n == 0) {
        (void)hipMemsetAsync(m_out, 0, sizeof(int64_t), stream);
        return dgnn_check_launch("voxel_subsample");
    }
    const VoxLayout L = vox_layout(scratch, n);
    const dim3 block(MESH_THREADS), grid = mesh_launch_grid(n);
    (void)hipMemsetAsync(L.err, 0, 256, stream);
    hipLaunchKernelGGL(k_vox_keys, grid, block, 0, stream, points, n, h, Origin{{origin[0], origin[1], origin[2]}}, L.sort.keys[0], L.sort.vals[0], L.err);
    int32_t herr = 0;
    int rc = dgnn_check_launch("voxel_subsample");
    if (rc || (rc = mm_read(&herr, L.err, sizeof(int32_t), stream, "voxel_subsample"))) return rc;
    DGNN_REQUIRE(!(herr & VOX_NONFINITE), DGNN_E_INVALID, "voxel_subsample: a non-finite coordinate");
    DGNN_REQUIRE(!herr, DGNN_E_INVALID, "voxel_subsample: a voxel coordinate floor((x - origin) / voxel_size) outside (-2^20, 2^20), the limit of the 63-bit key");
    int cur = 0;
    if ((rc = sort_pairs(L.sort, n, 63, stream, &cur))) return rc;
    const uint64_t* keys = L.sort.keys[cur];
    const int32_t* vals = L.sort.vals[cur];
    (void)hipMemsetAsync(L.is_first, 0, sizeof(int32_t) * n, stream);
    hipLaunchKernelGGL(k_vox_heads, grid, block, 0, stream, keys, vals, n, L.head, L.is_first);
    if ((rc = dgnn_exclusive_scan_i32(L.head, n, L.hscan, L.sums, stream))) return rc;
    if ((rc = dgnn_exclusive_scan_i32(L.is_first, n, L.vrank, L.sums, stream))) return rc;
    hipLaunchKernelGGL(k_vox_starts, grid, block, 0, stream, L.head, L.hscan, n, L.run_start);
    hipLaunchKernelGGL(k_vox_rows, grid, block, 0, stream, vals, L.head, L.hscan, L.vrank, L.run_start, n, voxel_out, first_out, count_out, L.vstart);
    hipLaunchKernelGGL(k_vox_centroid, dim3(dgnn_grid_cap(dgnn_cdiv(n, VOX_WAVES))), block, 0, stream, points, vals, L.vstart, count_out, L.hscan + n,
                       centroid_out, nearest_out, m_out);
    return dgnn_check_launch("voxel_subsample");
}

extern "C" int64_t dgnn_min_distance_thin_scratch_bytes(int64_t n, int32_t grid_resolution) {
    if (n < 0 || !knn_resolution_ok(grid_resolution)) return 256;
    return thin_layout(nullptr, n, grid_resolution).bytes;
}

extern "C" int dgnn_min_distance_thin(const double* points, int64_t n, double radius, const int64_t* priority, uint64_t seed, int32_t grid_resolution,
                                      uint8_t* keep_out, int64_t* stats_out, void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int32_t R = grid_resolution;
    DGNN_REQUIRE(scratch && stats_out && n >= 0 && (n == 0 || (points && keep_out)), DGNN_E_INVALID, "min_distance_thin: bad args");
    DGNN_REQUIRE(isfinite(radius) && radius >= 0.0, DGNN_E_INVALID, "min_distance_thin: the radius %g is not a finite number >= 0", radius);
    DGNN_REQUIRE(knn_resolution_ok(R), DGNN_E_UNSUPPORTED, "min_distance_thin: grid_resolution %d outside [0, %d]", R, KNN_MAX_R);
    DGNN_REQUIRE(n < INT32_MAX, DGNN_E_UNSUPPORTED, "min_distance_thin: sizes exceed the int32 indexing");
    const ThinLayout L = thin_layout(scratch, n, R);
    const dim3 block(MESH_THREADS), grid = mesh_launch_grid(n);
    ThinState hs{};
    hs.box.lo[0] = hs.box.lo[1] = hs.box.lo[2] = ~0ull;
    hs.cnt[0] = (uint32_t)n;
    (void)hipMemcpyAsync(L.st, &hs, sizeof(ThinState), hipMemcpyHostToDevice, stream);
    if (n > 0) hipLaunchKernelGGL(k_knn_bbox, grid, block, 0, stream, points, n, &L.st->box);
    int rc = dgnn_check_launch("min_distance_thin");
    if (rc || (rc = mm_read(&hs, L.st, sizeof(ThinState), stream, "min_distance_thin"))) return rc;
    DGNN_REQUIRE(!hs.box.err, DGNN_E_INVALID, "min_distance_thin: a non-finite coordinate");
    if (n > 0) {
        const double r2 = radius * radius, rw = radius * THIN_WIDEN;
        hipLaunchKernelGGL(k_thin_keys, grid, block, 0, stream, n, priority, seed, L.sort.keys[0], L.sort.vals[0]);
        int cur = 0;
        if ((rc = sort_pairs(L.sort, n, 64, stream, &cur))) return rc;
        hipLaunchKernelGGL(k_thin_rank, grid, block, 0, stream, L.sort.vals[cur], n, L.rank);
        CellGrid g{};
        if (R > 0 && (rc = bin_points(points, n, hs.box, R, L.bins, L.rank, &g, stream))) return rc;
        (void)hipMemsetAsync(L.state, 0, sizeof(int32_t) * n, stream);          // THIN_UNDECIDED
        hipLaunchKernelGGL(k_sub_iota, grid, block, 0, stream, L.list[0], n);
        int64_t left = n;
        for (int64_t t = 0; left > 0;) {
            DGNN_REQUIRE(t <= n, DGNN_E_LAUNCH, "min_distance_thin: %lld points undecided after %lld rounds", (long long)left, (long long)t);
            const dim3 rgrid(dgnn_grid_cap(dgnn_cdiv(left, THIN_WAVES)));
            for (int k = 0; k < THIN_ROUNDS_PER_READ; ++k, ++t) {
                if (R > 0)
                    hipLaunchKernelGGL(k_thin_round_grid, rgrid, block, 0, stream, L.bins.rec, L.bins.rowptr, g, r2, rw, L.state, L.list[t & 1],
                                       L.list[(t & 1) ^ 1], L.st, (int)(t % 3));
                else
                    hipLaunchKernelGGL(k_thin_round_all_pairs, rgrid, block, 0, stream, points, L.rank, n, r2, L.state, L.list[t & 1],
                                       L.list[(t & 1) ^ 1], L.st, (int)(t % 3));
            }
            rc = dgnn_check_launch("min_distance_thin");
            if (rc || (rc = mm_read(&hs, L.st, sizeof(ThinState), stream, "min_distance_thin"))) return rc;
            left = hs.cnt[t % 3];
        }
        hipLaunchKernelGGL(k_thin_finish, grid, block, 0, stream, L.state, n, keep_out, L.st);
    }
    (void)hipMemcpyAsync(stats_out, L.st->out, sizeof(int64_t) * THIN_N_OUT, hipMemcpyDeviceToDevice, stream);
    return dgnn_check_launch("min_distance_thin");
}
