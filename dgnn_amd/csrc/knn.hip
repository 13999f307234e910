// The k nearest neighbours of every query among a set of points, exactly, and the scan operations that rest on the lists: the mean
// neighbour distance, the statistical outlier mask and PCA normals (ops.knn, ops.knn_mean_distance, ops.outlier_mask, ops.estimate_normals).
// DESIGN §34; the contract is in include/dgnn_hip.h.  Everything is fp64 and every product, sum, difference and division rounds on its own
// (-ffp-contract=off).
//
//   rule       d2 = (dx dx + dy dy) + dz dz with dx = q.x - p.x and so on; a query's answer is the k smallest of ALL (d2, j) in lexicographic
//              order.  A total order: whatever order the candidates are met in, the list ends the same.
//   list       one wavefront per query, one entry of the sorted list per lane (so k <= 64, and no scratch).  The 64 lanes take one candidate
//              each; a ballot against the k-th entry drops nearly all of them once the list is warm; a survivor's place is the number of
//              entries below it (the popcount of a ballot), the lanes above that place take their lower neighbour's entry, the lane at it
//              takes the candidate.  All 64 lanes keep a sorted list; the answer is its first k.
//   grid       mesh_grid.h's frame over the box of the points and its monotone cell map.  The points are binned (point_grid.h) by count / scan / fill as
//              (x, y, z, index) records, cell after cell, z fastest: the cells of one (x, y) column that a shell touches are one run of
//              records, read 64 at a time.  The order inside a cell is whatever the atomics give; the total order does not see it.
//   search     Chebyshev shells of cells about the query's (clamped) cell.  After shell s the block B = [c - s, c + s]^3 (cut to the grid) has
//              been read.  A point j outside B has, on some axis a, its cell beyond a side of B that is not at the grid's edge, say below
//              B's low side k: fl(fl(x - lo) inv) < k, so x < X + 4 u M for the side's plane X = lo + k h (u = 2^-53, M the largest
//              coordinate magnitude of the box; §30's count).  The plane as computed, fl(lo + fl(k h)), and the difference fl(q_a - plane)
//              add less than 4 u (M + |q_a|).  A point has no extent, so nothing else enters: 12 u max(M, |q|_inf) in all, against
//              KNN_MARGIN = 2^-46 = 128 u.  With b = max(fl(|q_a - plane|) - KNN_MARGIN max(M, |q|_inf), 0) such a point has
//              |q_a - x| >= b.  On the two other axes the point lies in the box, so |q_k - x_k| >= o_k = max(lo_k - q_k, q_k - hi_k) - the
//              margin, or 0: the terms that let a query far outside the box stop after a few shells.  Its computed d2, a sum of three rounded
//              squares of rounded differences, is at least (b^2 + o_k^2 + o_l^2) (1 - 5 u), and B2 = the minimum over the open sides of
//              fl(b b + (o_k^2 + o_l^2)) is within (1 + 3 u) of that sum: the search stops when the list is full and its k-th d2 is
//              STRICTLY below B2 (1 - 2^-50), so that a tie in d2 with a lower index further out is still found.  "Every side at the grid's
//              edge" is a flag of its own (for coordinates whose squares overflow B2 is inf and the search reads on to the last shell); a
//              list that is not full always reads on.
//   order      with the points as their own queries the waves take them in the grid's cell order (the binned records), so neighbouring
//              waves read the same cells; the rows are written by original index.  Query i leaves out point i by INDEX.
//   all pairs  grid_resolution = 0: tiles of 256 points through LDS, four queries (waves) per block.  The cross-check and the path for tiny sets.
//   stats      shells read, candidates evaluated (every record of the cells read, the query's own included; all pairs: Q n), survivors placed.
#include <math.h>

#include "fixed_sum.h"
#include "point_grid.h"

namespace {

constexpr int KNN_MAX_K = 64;
constexpr double KNN_MARGIN = 0x1p-46;          // of max(M, |q|_inf): 128 u, u = 2^-53, against a need of 12 u (the derivation is above)
constexpr double KNN_SHRINK = 1.0 - 0x1p-50;
constexpr int32_t KNN_NONE = INT32_MAX;          // the index of an empty entry: above every point's
constexpr int KNN_TILE = 256, KNN_WAVES = MESH_THREADS / DGNN_WAVE;
enum { KNN_SHELLS = 0, KNN_CANDIDATES, KNN_PLACED, KNN_N_STATS };

struct KnnState {
    PointBox box;          // err, the bbox of the points
    unsigned long long stats[KNN_N_STATS];
};
static_assert(sizeof(KnnState) <= 256, "KnnState must fit the first scratch slot");

// ---- validation (the box and the bins are point_grid.h's) ---------------------------------------------------------------------------------
__global__ void k_knn_check_finite(const double* __restrict__ p, int64_t n3, KnnState* st) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n3; i += (int64_t)gridDim.x * blockDim.x)
        if (!isfinite(p[i])) atomicOr(&st->box.err, KNN_NONFINITE);
}

// ---- the list: lane r holds the r-th smallest (d2, id) met so far ------------------------------------------------------------------------
struct KnnList {
    double d2, kd2;          // this lane's entry; the k-th entry (uniform)
    int32_t id, kid;
    unsigned long long placed;
};

__device__ __forceinline__ bool knn_less(double a, int32_t ia, double b, int32_t ib) { return a < b || (a == b && ia < ib); }

__device__ __forceinline__ KnnList knn_empty() { return KnnList{INFINITY, INFINITY, KNN_NONE, KNN_NONE, 0}; }

// every lane arrives with its candidate (valid: it has one)
__device__ __forceinline__ void knn_offer(KnnList& L, int k, bool valid, double cd2, int32_t cid) {
    unsigned long long m = __ballot(valid && knn_less(cd2, cid, L.kd2, L.kid));
    const int lane = lane_id();
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const double d = __shfl(cd2, src);
        const int32_t j = __shfl(cid, src);
        if (!knn_less(d, j, L.kd2, L.kid)) continue;          // the k-th entry fell since the ballot
        const int pos = __popcll(__ballot(knn_less(L.d2, L.id, d, j)));
        const double ud = __shfl_up(L.d2, 1);
        const int32_t ui = __shfl_up(L.id, 1);
        if (lane > pos) {
            L.d2 = ud;
            L.id = ui;
        } else if (lane == pos) {
            L.d2 = d;
            L.id = j;
        }
        L.kd2 = __shfl(L.d2, k - 1);
        L.kid = __shfl(L.id, k - 1);
        ++L.placed;
    }
}

__device__ __forceinline__ void knn_store(const KnnList& L, int k, int64_t row, int32_t* __restrict__ idx_out, double* __restrict__ d2_out) {
    const int lane = lane_id();
    if (lane < k) {
        const bool none = L.id == KNN_NONE;
        idx_out[row * k + lane] = none ? -1 : L.id;
        d2_out[row * k + lane] = none ? INFINITY : L.d2;
    }
}

__device__ __forceinline__ void knn_add_stats(KnnState* st, unsigned long long shells, unsigned long long cands, unsigned long long placed) {
    if (lane_id() == 0) {          // the three counts are the same in every lane of the wave
        if (shells) atomicAdd(&st->stats[KNN_SHELLS], shells);
        if (cands) atomicAdd(&st->stats[KNN_CANDIDATES], cands);
        if (placed) atomicAdd(&st->stats[KNN_PLACED], placed);
    }
}

// ---- all pairs ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MESH_THREADS) k_knn_all_pairs(const double* __restrict__ points, int64_t n, const double* __restrict__ queries, int64_t nq,
                                                              int k, int32_t* __restrict__ idx_out, double* __restrict__ d2_out, KnnState* st) {
    __shared__ double tile[3 * KNN_TILE];
    const int lane = lane_id(), wave = wave_id_uniform();
    unsigned long long cands = 0, placed = 0;
    for (int64_t base = (int64_t)blockIdx.x * KNN_WAVES; base < nq; base += (int64_t)gridDim.x * KNN_WAVES) {
        const int64_t w = base + wave;
        const bool active = w < nq;
        const double* src = queries ? queries : points;
        const double q[3] = {active ? src[3 * w] : 0.0, active ? src[3 * w + 1] : 0.0, active ? src[3 * w + 2] : 0.0};
        const int32_t self = queries ? -1 : (int32_t)w;
        KnnList L = knn_empty();
        for (int64_t t0 = 0; t0 < n; t0 += KNN_TILE) {
            const int cnt = (int)(n - t0 < KNN_TILE ? n - t0 : KNN_TILE);
            __syncthreads();
            for (int i = threadIdx.x; i < 3 * cnt; i += MESH_THREADS) tile[i] = points[3 * t0 + i];
            __syncthreads();
            if (active)
                for (int c = 0; c < cnt; c += DGNN_WAVE) {
                    const int i = c + lane;
                    const bool in = i < cnt;
                    const double d2 = in ? knn_d2(q, tile[3 * i], tile[3 * i + 1], tile[3 * i + 2]) : 0.0;
                    const int32_t id = (int32_t)(t0 + i);
                    knn_offer(L, k, in && id != self, d2, id);
                }
        }
        if (active) {
            knn_store(L, k, w, idx_out, d2_out);
            cands += (unsigned long long)n;
            placed += L.placed;
        }
    }
    knn_add_stats(st, 0, cands, placed);
}

// ---- the search ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int32_t knn_max(int32_t a, int32_t b) { return a > b ? a : b; }
__device__ __forceinline__ int32_t knn_min(int32_t a, int32_t b) { return a < b ? a : b; }

// the records [beg, end), 64 at a time
__device__ __forceinline__ void knn_run(KnnList& L, int k, const KnnPoint* __restrict__ rec, int32_t beg, int32_t end, const double (&q)[3], int32_t self) {
    for (int32_t b = beg; b < end; b += DGNN_WAVE) {
        const int32_t i = b + lane_id();
        const bool in = i < end;
        KnnPoint p{0.0, 0.0, 0.0, -1, 0};
        if (in) p = rec[i];
        knn_offer(L, k, in && p.id != self, knn_d2(q, p.x, p.y, p.z), p.id);
    }
}

// queries == NULL: the points themselves, in the order of their records
__global__ void __launch_bounds__(MESH_THREADS) k_knn_search(const KnnPoint* __restrict__ rec, const int32_t* __restrict__ rowptr, CellGrid G,
                                                           const double* __restrict__ queries, int64_t nq, int k, int32_t* __restrict__ idx_out,
                                                           double* __restrict__ d2_out, KnnState* st) {
    unsigned long long shells = 0, cands = 0, placed = 0;
    const int32_t s_end = knn_max(G.n[0], knn_max(G.n[1], G.n[2]));          // shells <= the resolution
    const int64_t n_waves = (int64_t)gridDim.x * KNN_WAVES;
    for (int64_t w = (int64_t)blockIdx.x * KNN_WAVES + wave_id_uniform(); w < nq; w += n_waves) {
        double q[3];
        int32_t self = -1;
        int64_t row = w;
        if (queries) {
            q[0] = queries[3 * w];
            q[1] = queries[3 * w + 1];
            q[2] = queries[3 * w + 2];
        } else {
            const KnnPoint me = rec[w];
            q[0] = me.x;
            q[1] = me.y;
            q[2] = me.z;
            self = me.id;
            row = me.id;
        }
        int32_t c[3];
        double mag = G.mag;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            c[a] = grid_cell(G, a, q[a]);
            mag = fmax(mag, fabs(q[a]));
        }
        const double eps = KNN_MARGIN * mag;
        double out2[3];          // per axis, the squared distance from the query to the box's span (0 inside it), shrunk by the margin
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double o = fmax(fmax(G.lo[a] - q[a], q[a] - G.hi[a]) - eps, 0.0);
            out2[a] = o * o;
        }
        KnnList L = knn_empty();
        int32_t s = 0;
        for (; s < s_end; ++s) {
            const int32_t x0 = knn_max(c[0] - s, 0), x1 = knn_min(c[0] + s, G.n[0] - 1);
            const int32_t y0 = knn_max(c[1] - s, 0), y1 = knn_min(c[1] + s, G.n[1] - 1);
            const int32_t z0 = knn_max(c[2] - s, 0), z1 = knn_min(c[2] + s, G.n[2] - 1);
            for (int32_t x = x0; x <= x1; ++x)
                for (int32_t y = y0; y <= y1; ++y) {
                    // the cells of the column at Chebyshev distance s: all of it when x or y is on the shell (one run of records), else its two ends
                    const int64_t col = ((int64_t)x * G.n[1] + y) * G.n[2];
                    if (x == c[0] - s || x == c[0] + s || y == c[1] - s || y == c[1] + s) {
                        const int32_t beg = rowptr[col + z0], end = rowptr[col + z1 + 1];
                        knn_run(L, k, rec, beg, end, q, self);
                        cands += (unsigned long long)(end - beg);
                    } else {
                        for (int32_t z = c[2] - s; z <= c[2] + s; z += 2 * s) {
                            if (z < z0 || z > z1) continue;
                            const int32_t beg = rowptr[col + z], end = rowptr[col + z + 1];
                            knn_run(L, k, rec, beg, end, q, self);
                            cands += (unsigned long long)(end - beg);
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
                    const double b = fmax((q[a] - (G.lo[a] + (double)blo[a] * G.h[a])) - eps, 0.0);
                    b2 = fmin(b2, b * b + rest);
                }
                if (bhi[a] < G.n[a] - 1) {
                    open_side = true;
                    const double b = fmax(((G.lo[a] + (double)(bhi[a] + 1) * G.h[a]) - q[a]) - eps, 0.0);
                    b2 = fmin(b2, b * b + rest);
                }
            }
            if (!open_side) { ++s; break; }          // every side at the grid's edge: the whole grid was read
            if (L.kid != KNN_NONE && L.kd2 < b2 * KNN_SHRINK) { ++s; break; }
        }
        shells += (unsigned long long)s;
        placed += L.placed;
        knn_store(L, k, row, idx_out, d2_out);
    }
    knn_add_stats(st, shells, cands, placed);
}

// ---- on the lists: mean distance, the outlier mask, normals ------------------------------------------------------------------------------
// m[i] = (the sum of sqrt(d2[i, r]) over the valid entries, in rank order) / their number (none: 0 / 0)
__global__ void k_knn_mean_distance(const double* __restrict__ d2, const int32_t* __restrict__ idx, int64_t n, int k, double* __restrict__ m) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        double s = 0.0, cnt = 0.0;
        for (int r = 0; r < k; ++r)
            if (idx[i * k + r] >= 0) {
                s += sqrt(d2[i * k + r]);
                cnt += 1.0;
            }
        m[i] = s / cnt;
    }
}

// dev[i] = (m[i] - mu)^2 with mu = *sum / n
__global__ void k_knn_sq_dev(const double* __restrict__ m, int64_t n, const double* __restrict__ sum, double* __restrict__ dev) {
    const double mu = *sum / (double)n;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double d = m[i] - mu;
        dev[i] = d * d;
    }
}

// values[0..3] = mu, sigma, threshold; keep[i] = m[i] <= threshold; the removed are counted (an integer sum: order-free)
__global__ void __launch_bounds__(MESH_THREADS) k_knn_keep(const double* __restrict__ m, int64_t n, const double* __restrict__ sums, double std_ratio,
                                                         uint8_t* __restrict__ keep, double* __restrict__ values, unsigned long long* n_removed) {
    const double mu = sums[0] / (double)n, sigma = sqrt(sums[1] / (double)n);
    const double threshold = mu + std_ratio * sigma;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        values[0] = mu;
        values[1] = sigma;
        values[2] = threshold;
    }
    unsigned long long removed = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const bool kept = m[i] <= threshold;
        keep[i] = kept ? 1 : 0;
        removed += kept ? 0 : 1;
    }
    wave_add_atomic(removed, n_removed);
}

__global__ void k_knn_check_rows(const int32_t* __restrict__ idx, int64_t total, int64_t n, int32_t* err) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
        if (idx[i] < -1 || idx[i] >= n) atomicOr(err, KNN_BAD_ID);
}

// one Jacobi rotation in the (p, q) plane of the symmetric A; r is the third index: (a_pp, a_qq, a_pq, a_rp, a_rq) and the columns p, q of V
__device__ __forceinline__ void knn_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double (&v)[3][3], int p, int q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp;
    arq = rq;
    apq = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double vp = v[i][p], vq = v[i][q];
        v[i][p] = c * vp - s * vq;
        v[i][q] = s * vp + c * vq;
    }
}

constexpr int KNN_JACOBI_SWEEPS = 6;

// one lane per point: the point, then its neighbours in rank order
__global__ void __launch_bounds__(MESH_THREADS) k_knn_normals(const double* __restrict__ pts, int64_t n, const int32_t* __restrict__ idx, int k,
                                                            const double* __restrict__ sensors, double* __restrict__ normals, double* __restrict__ eig) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
        double sx = px, sy = py, sz = pz, m = 1.0;
        for (int r = 0; r < k; ++r) {
            const int64_t j = idx[i * k + r];
            if (j < 0) continue;
            sx += pts[3 * j];
            sy += pts[3 * j + 1];
            sz += pts[3 * j + 2];
            m += 1.0;
        }
        const double cx = sx / m, cy = sy / m, cz = sz / m;
        double dx = px - cx, dy = py - cy, dz = pz - cz;
        double a00 = dx * dx, a11 = dy * dy, a22 = dz * dz, a01 = dx * dy, a02 = dx * dz, a12 = dy * dz;
        for (int r = 0; r < k; ++r) {
            const int64_t j = idx[i * k + r];
            if (j < 0) continue;
            dx = pts[3 * j] - cx;
            dy = pts[3 * j + 1] - cy;
            dz = pts[3 * j + 2] - cz;
            a00 += dx * dx;
            a11 += dy * dy;
            a22 += dz * dz;
            a01 += dx * dy;
            a02 += dx * dz;
            a12 += dy * dz;
        }
        double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
        for (int sweep = 0; sweep < KNN_JACOBI_SWEEPS; ++sweep) {
            knn_rotate(a00, a11, a01, a02, a12, v, 0, 1);
            knn_rotate(a00, a22, a02, a01, a12, v, 0, 2);
            knn_rotate(a11, a22, a12, a01, a02, v, 1, 2);
        }
        const double d[3] = {a00, a11, a22};
        int col = 0;
        if (d[1] < d[col]) col = 1;
        if (d[2] < d[col]) col = 2;
        double e0 = d[0], e1 = d[1], e2 = d[2], t;          // ascending, ties by column: three strict exchanges
        if (e1 < e0) { t = e0; e0 = e1; e1 = t; }
        if (e2 < e1) { t = e1; e1 = e2; e2 = t; }
        if (e1 < e0) { t = e0; e0 = e1; e1 = t; }
        double nx = col == 0 ? v[0][0] : (col == 1 ? v[0][1] : v[0][2]);
        double ny = col == 0 ? v[1][0] : (col == 1 ? v[1][1] : v[1][2]);
        double nz = col == 0 ? v[2][0] : (col == 1 ? v[2][1] : v[2][2]);
        const double len = sqrt((nx * nx + ny * ny) + nz * nz);
        nx = nx / len;
        ny = ny / len;
        nz = nz / len;
        double big = nx, ab = fabs(nx);          // the component of largest magnitude, ties to the lowest axis
        if (fabs(ny) > ab) { big = ny; ab = fabs(ny); }
        if (fabs(nz) > ab) { big = nz; ab = fabs(nz); }
        bool flip = big < 0.0;
        if (flip) { nx = -nx; ny = -ny; nz = -nz; }
        if (sensors) {
            const double tx = sensors[3 * i] - px, ty = sensors[3 * i + 1] - py, tz = sensors[3 * i + 2] - pz;
            if ((nx * tx + ny * ty) + nz * tz < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
        }
        normals[3 * i] = nx;
        normals[3 * i + 1] = ny;
        normals[3 * i + 2] = nz;
        eig[3 * i] = e0;
        eig[3 * i + 1] = e1;
        eig[3 * i + 2] = e2;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
struct KnnLayout { KnnState* st; PointBins bins; int64_t bytes; };
KnnLayout knn_layout(void* base, int64_t n, int64_t R) {
    Take t{(char*)base, 256};
    KnnLayout L{};
    L.st = (KnnState*)base;
    if (R > 0) L.bins = take_point_bins(t, n, R);
    L.bytes = t.off;
    return L;
}

}  // namespace

// ================================================================================================================================
extern "C" int64_t dgnn_knn_scratch_bytes(int64_t n_points, int32_t grid_resolution) {
    if (n_points < 0 || !knn_resolution_ok(grid_resolution)) return 256;
    return knn_layout(nullptr, n_points, grid_resolution).bytes;
}

extern "C" int dgnn_knn(const double* points, int64_t n_points, const double* queries, int64_t n_queries, int32_t k, int32_t grid_resolution,
                        int32_t* idx_out, double* d2_out, int64_t* stats_out, void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t n = n_points, nq = queries ? n_queries : n_points;
    const int32_t R = grid_resolution;
    DGNN_REQUIRE(scratch && stats_out && n >= 0 && nq >= 0 && (n == 0 || points) && (nq == 0 || (idx_out && d2_out)), DGNN_E_INVALID, "knn: bad args");
    DGNN_REQUIRE(k >= 1 && k <= KNN_MAX_K, DGNN_E_INVALID, "knn: k = %d outside [1, %d]", k, KNN_MAX_K);
    DGNN_REQUIRE(knn_resolution_ok(R), DGNN_E_UNSUPPORTED, "knn: grid_resolution %d outside [0, %d]", R, KNN_MAX_R);
    DGNN_REQUIRE(n < INT32_MAX && nq < INT32_MAX, DGNN_E_UNSUPPORTED, "knn: sizes exceed the int32 indexing");
    const KnnLayout L = knn_layout(scratch, n, R);
    const dim3 block(MESH_THREADS);
    KnnState hs{};
    hs.box.lo[0] = hs.box.lo[1] = hs.box.lo[2] = ~0ull;
    (void)hipMemcpyAsync(L.st, &hs, sizeof(KnnState), hipMemcpyHostToDevice, stream);
    if (n > 0) hipLaunchKernelGGL(k_knn_bbox, mesh_launch_grid(n), block, 0, stream, points, n, &L.st->box);
    if (queries && nq > 0) hipLaunchKernelGGL(k_knn_check_finite, mesh_launch_grid(3 * nq), block, 0, stream, queries, 3 * nq, L.st);
    int rc = dgnn_check_launch("knn");
    if (rc || (rc = mm_read(&hs, L.st, sizeof(KnnState), stream, "knn"))) return rc;
    DGNN_REQUIRE(!hs.box.err, DGNN_E_INVALID, "knn: a non-finite coordinate of a point or of a query");
    if (nq > 0) {
        const dim3 grid(dgnn_grid_cap(dgnn_cdiv(nq, KNN_WAVES)));
        if (R == 0 || n == 0) {
            hipLaunchKernelGGL(k_knn_all_pairs, grid, block, 0, stream, points, n, queries, nq, k, idx_out, d2_out, L.st);
        } else {
            CellGrid g;
            if ((rc = bin_points(points, n, hs.box, R, L.bins, nullptr, &g, stream))) return rc;
            hipLaunchKernelGGL(k_knn_search, grid, block, 0, stream, L.bins.rec, L.bins.rowptr, g, queries, nq, k, idx_out, d2_out, L.st);
        }
    }
    (void)hipMemcpyAsync(stats_out, L.st->stats, sizeof(int64_t) * KNN_N_STATS, hipMemcpyDeviceToDevice, stream);
    return dgnn_check_launch("knn");
}

extern "C" int dgnn_knn_mean_distance(const double* d2, const int32_t* idx, int64_t n, int32_t k, double* mean_out, void* stream_) {
    DGNN_REQUIRE(n >= 0 && k >= 1 && (n == 0 || (d2 && idx && mean_out)), DGNN_E_INVALID, "knn_mean_distance: bad args");
    if (n == 0) return DGNN_OK;
    hipLaunchKernelGGL(k_knn_mean_distance, mesh_launch_grid(n), dim3(MESH_THREADS), 0, (hipStream_t)stream_, d2, idx, n, k, mean_out);
    return dgnn_check_launch("knn_mean_distance");
}

extern "C" int64_t dgnn_outlier_mask_scratch_bytes(int64_t n) {
    if (n < 0) return 256;
    return 256 + (((n + dgnn_cdiv(n, FIXED_SUM_CHUNK) + 1) * (int64_t)sizeof(double) + 255) / 256) * 256;
}

extern "C" int dgnn_outlier_mask(const double* mean_distance, int64_t n, double std_ratio, uint8_t* keep_out, double* values_out, int64_t* n_removed_out,
                                 void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(scratch && mean_distance && keep_out && values_out && n_removed_out, DGNN_E_INVALID, "outlier_mask: bad args");
    DGNN_REQUIRE(n >= 2, DGNN_E_INVALID, "outlier_mask: %lld points, at least 2 are needed", (long long)n);
    double* sums = (double*)scratch;                                    // [0] the sum of m, [1] the sum of the squared deviations
    double* dev = (double*)((char*)scratch + 256);
    double* part = dev + n;
    (void)hipMemsetAsync(n_removed_out, 0, sizeof(int64_t), stream);
    fixed_sum(const_cast<double*>(mean_distance), n, 0, part, sums, stream);
    hipLaunchKernelGGL(k_knn_sq_dev, mesh_launch_grid(n), dim3(MESH_THREADS), 0, stream, mean_distance, n, sums, dev);
    fixed_sum(dev, n, 0, part, sums + 1, stream);
    hipLaunchKernelGGL(k_knn_keep, mesh_launch_grid(n), dim3(MESH_THREADS), 0, stream, mean_distance, n, sums, std_ratio, keep_out, values_out,
                       (unsigned long long*)n_removed_out);
    return dgnn_check_launch("outlier_mask");
}

extern "C" int dgnn_knn_normals(const double* points, int64_t n, const int32_t* idx, int32_t k, const double* sensors, double* normals_out,
                                double* eigenvalues_out, void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(scratch && n >= 0 && k >= 1 && (n == 0 || (points && idx && normals_out && eigenvalues_out)), DGNN_E_INVALID, "knn_normals: bad args");
    DGNN_REQUIRE(n < INT32_MAX, DGNN_E_UNSUPPORTED, "knn_normals: sizes exceed the int32 indexing");
    if (n == 0) return DGNN_OK;
    int32_t* err = (int32_t*)scratch;
    int32_t herr = 0;
    (void)hipMemsetAsync(err, 0, sizeof(int32_t), stream);
    hipLaunchKernelGGL(k_knn_check_rows, mesh_launch_grid(n * k), dim3(MESH_THREADS), 0, stream, idx, n * k, n, err);
    int rc = dgnn_check_launch("knn_normals");
    if (rc || (rc = mm_read(&herr, err, sizeof(int32_t), stream, "knn_normals"))) return rc;   // ids are read below: checked first
    DGNN_REQUIRE(!herr, DGNN_E_INVALID, "knn_normals: a neighbour index outside [-1, n)");
    hipLaunchKernelGGL(k_knn_normals, mesh_launch_grid(n), dim3(MESH_THREADS), 0, stream, points, n, idx, k, sensors, normals_out, eigenvalues_out);
    return dgnn_check_launch("knn_normals");
}
