// Mesh metrics of the reconstructed interface surface (reference processing/generate_mesh.py:126-163, processing/evaluate_mesh.py).
//
//   locate     point location in the labelled tetrahedralization: a query is inside the reconstructed surface iff the finite cell
//              that contains it is labelled inside.  Neighbour table from the facet list (one write per slot), start
//              cell = the lowest cell id among the cells whose centroid bins with the query (uniform grid, atomicMin: order-free;
//              empty bins filled by axis sweeps, k_start_axis),
//              then a visibility walk with fp64 orientations taken on the facet's SORTED vertex ids, so the two cells of a facet see
//              the same number with opposite signs (no rounding gap between them).  A cell is accepted when its four signs are >= 0;
//              otherwise the walk steps across the lowest-k face whose sign is < 0; stepping across a hull face = outside.
//   iou counts |A n B|, |A u B| against the ground-truth occupancies, int64 sums.
//   sampler    fp64 areas, a fixed-order fp64 inclusive scan, face = first j with cum[j] >= u0 * total (np.searchsorted 'left'),
//              barycentric (u, v) reflected when u + v > 1; randomness from mm_hash(seed, 3 i + k + 1) (header).
//   nearest    exact nearest neighbour over a uniform grid of the reference set (count / scan / fill), shells searched outward until
//              the best squared distance is below the bound for every unvisited bin (with slack for the fp32 bin arithmetic).
//              The answer is the lexicographic minimum of ((dx*dx + dy*dy) + dz*dz, index), so it does not depend on the order inside
//              a bin: the bins are not sorted.  Sum of the distances in a fixed order (fp64).
#include <math.h>
#include <string.h>

#include "common.h"
#include "mesh_common.h"
#include "vec3.h"
#include "tet_common.h"
#include "fixed_sum.h"

int dgnn_exclusive_scan_i32(const int32_t* in, int64_t n, int32_t* out, int32_t* sums_scratch, hipStream_t stream);  // plan.hip

namespace {

using dgnn_exact::V3;
using dgnn_exact::load_v3;

constexpr int32_t MM_MAX_STEPS = 1 << 16;            // walk steps per query
constexpr int32_t MM_NBR_UNSET = (int32_t)0x80808080;
constexpr int MM_MAX_DIM = 1024;                      // grid bins per axis
// status bits
constexpr int32_t MM_BAD_ID = 1, MM_NONFINITE = 2, MM_MALFORMED = 4, MM_CAP = 8;

struct MmState {
    int32_t err, max_steps, pad[2];
    unsigned int lo_bits[3], hi_bits[3];   // bbox of fp32 data as order-preserving uint keys
    unsigned long long lo64[3], hi64[3];   // bbox of fp64 data
    unsigned long long counts[2];          // iou: |A n B|, |A u B|
};

__device__ __forceinline__ unsigned int f32_key(float x) {
    const unsigned int u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
inline float f32_unkey(unsigned int k) {
    const unsigned int u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// ---- uniform grid geometry (host picks it, kernels read it by value) ----------------------------------------------------------
struct Grid {
    double lo[3];
    double h;            // bin edge
    int32_t d[3];        // bins per axis
};

// the largest bin edge with prod ceil(ext / h) <= target (bisection; every axis at least 1, at most MM_MAX_DIM bins)
Grid grid_for(const double lo[3], const double hi[3], int64_t target) {
    Grid g{};
    double ext[3], emax = 0;
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = lo[a];
        ext[a] = hi[a] - lo[a];
        if (ext[a] > emax) emax = ext[a];
    }
    auto dims = [&](double h, int32_t* d) {
        double p = 1;
        for (int a = 0; a < 3; ++a) {
            double n = ceil(ext[a] / h);
            n = n < 1 ? 1 : (n > MM_MAX_DIM ? MM_MAX_DIM : n);
            if (d) d[a] = (int32_t)n;
            p *= n;
        }
        return p;
    };
    if (!(emax > 0)) {
        g.h = 1.0;
        g.d[0] = g.d[1] = g.d[2] = 1;
        return g;
    }
    double hi_h = emax, lo_h = emax / MM_MAX_DIM / 2;   // dims(hi_h) = 1 bin per axis
    if (target < 1) target = 1;
    for (int it = 0; it < 60; ++it) {
        const double mid = 0.5 * (lo_h + hi_h);
        if (dims(mid, nullptr) <= (double)target) hi_h = mid;
        else lo_h = mid;
    }
    g.h = hi_h;
    dims(hi_h, g.d);
    return g;
}

__device__ __forceinline__ int32_t bin_axis(double t, int32_t d) {
    const double f = floor(t);
    return f < 0 ? 0 : (f >= d - 1 ? d - 1 : (int32_t)f);
}

// ---- fp64 orientation --------------------------------------------------------------------------------------------------------
// det[b - a, c - a, p - a], evaluated left to right (the numpy model, tests/mesh_metrics_model.py, repeats it operation for operation)
__device__ __forceinline__ double orient(const V3& a, const V3& b, const V3& c, const V3& p) {
    const double ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z;
    const double vx = c.x - a.x, vy = c.y - a.y, vz = c.z - a.z;
    const double wx = p.x - a.x, wy = p.y - a.y, wz = p.z - a.z;
    return ux * (vy * wz - vz * wy) - uy * (vx * wz - vz * wx) + uz * (vx * wy - vy * wx);
}

__device__ __forceinline__ void sort3(int32_t& a, int32_t& b, int32_t& c) {
    int32_t t;
    if (a > b) { t = a; a = b; b = t; }
    if (b > c) { t = b; b = c; c = t; }
    if (a > b) { t = a; a = b; b = t; }
}

__global__ void k_fill_i32(int32_t* __restrict__ x, int64_t n, int32_t v) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) x[i] = v;
}

// ---- neighbour table ---------------------------------------------------------------------------------------------------------
__global__ void k_check_vertices(const double* __restrict__ v, int64_t nv, MmState* st) {
    unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0, 0, 0};
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
        for (int a = 0; a < 3; ++a) {
            const double x = v[3 * i + a];
            if (!isfinite(x)) { atomicOr(&st->err, MM_NONFINITE); continue; }
            const unsigned long long k = f64_key(x);
            lo[a] = k < lo[a] ? k : lo[a];
            hi[a] = k > hi[a] ? k : hi[a];
        }
    }
    for (int a = 0; a < 3; ++a) wave_minmax_atomic(lo[a], hi[a], &st->lo64[a], &st->hi64[a]);
}

// facet f = vertices (x, y, z) between cells nfacets[f] = (a, b), -1 = the infinite cell: nbr[4 c + k] = the other cell, k = the vertex
// of c that is not on the facet.  Every slot is written by exactly the facet of that face of a well-formed triangulation.
__global__ void k_nbr_fill(const int32_t* __restrict__ tets, int64_t nc, const int32_t* __restrict__ facets, const int32_t* __restrict__ nfacets,
                           int64_t nf, int64_t nv, int32_t* __restrict__ nbr, MmState* st) {
    for (int64_t f = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; f < nf; f += (int64_t)gridDim.x * blockDim.x) {
        const int32_t x = facets[3 * f], y = facets[3 * f + 1], z = facets[3 * f + 2];
        const int32_t c2[2] = {nfacets[2 * f], nfacets[2 * f + 1]};
        if (x < 0 || x >= nv || y < 0 || y >= nv || z < 0 || z >= nv || c2[0] < -1 || c2[0] >= nc || c2[1] < -1 || c2[1] >= nc) {
            atomicOr(&st->err, MM_BAD_ID);
            continue;
        }
        if (x == y || y == z || x == z || c2[0] == c2[1]) { atomicOr(&st->err, MM_MALFORMED); continue; }
        for (int s = 0; s < 2; ++s) {
            const int32_t c = c2[s];
            if (c < 0) continue;
            const int miss = facet_opposite_slot(tets + 4 * (int64_t)c, x, y, z);
            if (miss < 0) { atomicOr(&st->err, MM_MALFORMED); continue; }
            nbr[4 * (int64_t)c + miss] = c2[1 - s];
        }
    }
}

// every face of every cell has its facet, and a finite neighbour points back
__global__ void k_nbr_check(const int32_t* __restrict__ nbr, int64_t nc, MmState* st) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < 4 * nc; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t d = nbr[i];
        if (d == MM_NBR_UNSET) { atomicOr(&st->err, MM_MALFORMED); continue; }
        if (d < 0) continue;
        const int32_t c = (int32_t)(i >> 2);
        if (nbr[4 * (int64_t)d] != c && nbr[4 * (int64_t)d + 1] != c && nbr[4 * (int64_t)d + 2] != c && nbr[4 * (int64_t)d + 3] != c)
            atomicOr(&st->err, MM_MALFORMED);
    }
}

// start cells: start[bin] = the lowest id among the cells whose centroid falls in the bin (atomicMin: order-free)
__global__ void k_start_min(const double* __restrict__ v, const int32_t* __restrict__ tets, int64_t nc, Grid g, int32_t* __restrict__ start) {
    for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < nc; c += (int64_t)gridDim.x * blockDim.x) {
        double m[3] = {0, 0, 0};
        for (int k = 0; k < 4; ++k) {
            const V3 p = load_v3(v, tets[4 * c + k]);
            m[0] += p.x; m[1] += p.y; m[2] += p.z;
        }
        int32_t b[3];
        for (int a = 0; a < 3; ++a) b[a] = bin_axis((0.25 * m[a] - g.lo[a]) / g.h, g.d[a]);
        atomicMin(start + ((int64_t)b[2] * g.d[1] + b[1]) * g.d[0] + b[0], (int32_t)c);
    }
}

// an empty bin takes the start of the nearest non-empty bin on its line along `axis` (ties to the lower index); launched for x, y, z
// in turn, so a bin empty after the x pass looks along y among the x-filled bins, and so on.  One thread per line, two sweeps: O(bins)
// in all, whatever the shape of the empty region.  The backward sweep parks the position of the nearest non-empty bin to the right in
// out[] as -(pos + 2) (cell ids are >= 0).
__global__ void k_start_axis(const int32_t* __restrict__ in, Grid g, int axis, int32_t* __restrict__ out) {
    const int64_t sy = g.d[0], sz = (int64_t)g.d[0] * g.d[1];
    const int64_t stride = axis == 0 ? 1 : (axis == 1 ? sy : sz);
    const int32_t len = g.d[axis], d_u = axis == 0 ? g.d[1] : g.d[0];   // the other two axes: u (the lower), w
    const int64_t s_u = axis == 0 ? sy : 1, s_w = axis == 2 ? sy : sz;
    const int64_t lines = sz * g.d[2] / len;
    for (int64_t l = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; l < lines; l += (int64_t)gridDim.x * blockDim.x) {
        const int64_t base = (l % d_u) * s_u + (l / d_u) * s_w;
        int32_t r = -1;
        for (int32_t i = len - 1; i >= 0; --i) {
            const int32_t v = in[base + i * stride];
            if (v != INT32_MAX) r = i;
            out[base + i * stride] = v != INT32_MAX ? v : (r >= 0 ? -(r + 2) : INT32_MAX);
        }
        int32_t left = -1;
        for (int32_t i = 0; i < len; ++i) {
            const int32_t v = in[base + i * stride];
            if (v != INT32_MAX) { left = i; continue; }
            const int32_t o = out[base + i * stride], right = o == INT32_MAX ? -1 : -o - 2;
            const int32_t pick = left >= 0 && (right < 0 || i - left <= right - i) ? left : right;
            out[base + i * stride] = pick >= 0 ? in[base + pick * stride] : INT32_MAX;
        }
    }
}

// ---- the walk ----------------------------------------------------------------------------------------------------------------
__global__ void k_locate(const double* __restrict__ v, const int32_t* __restrict__ tets, const int32_t* __restrict__ nbr,
                         const int32_t* __restrict__ start, Grid g, const float* __restrict__ pts, int64_t np, int32_t* __restrict__ cell_out,
                         MmState* st) {
    int32_t my_max = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < np; i += (int64_t)gridDim.x * blockDim.x) {
        const V3 q{(double)pts[3 * i], (double)pts[3 * i + 1], (double)pts[3 * i + 2]};
        if (!isfinite(q.x) || !isfinite(q.y) || !isfinite(q.z)) {
            atomicOr(&st->err, MM_NONFINITE);
            cell_out[i] = -1;
            continue;
        }
        const int32_t bx = bin_axis((q.x - g.lo[0]) / g.h, g.d[0]), by = bin_axis((q.y - g.lo[1]) / g.h, g.d[1]),
                      bz = bin_axis((q.z - g.lo[2]) / g.h, g.d[2]);
        int32_t c = start[((int64_t)bz * g.d[1] + by) * g.d[0] + bx], steps = 0;
        for (; c >= 0; ++steps) {
            if (steps >= MM_MAX_STEPS) {
                atomicOr(&st->err, MM_CAP);
                c = -1;
                break;
            }
            int32_t id[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) id[k] = tets[4 * (int64_t)c + k];
            int32_t next = -2;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int32_t a = id[(k + 1) & 3], b = id[(k + 2) & 3], e = id[(k + 3) & 3];
                sort3(a, b, e);
                const V3 pa = load_v3(v, a), pb = load_v3(v, b), pe = load_v3(v, e);
                const double o = orient(pa, pb, pe, q), s = orient(pa, pb, pe, load_v3(v, id[k]));
                // q on the side of vertex k (or on the face): >= 0; a flat cell (s == 0) holds only points on its plane
                const bool neg = s > 0 ? o < 0 : (s < 0 ? o > 0 : o != 0);
                if (neg) { next = k; break; }
            }
            if (next == -2) break;                   // all four signs >= 0: c contains q
            c = nbr[4 * (int64_t)c + next];          // -1: across a hull face, q is outside the convex hull
        }
        cell_out[i] = c;
        my_max = steps > my_max ? steps : my_max;
    }
    for (int o = 32; o > 0; o >>= 1) my_max = max(my_max, __shfl_xor(my_max, o));
    if (lane_id() == 0 && my_max) atomicMax(&st->max_steps, my_max);
}

__global__ void __launch_bounds__(MESH_THREADS) k_iou_counts(const int32_t* __restrict__ cells, int64_t np, const int32_t* __restrict__ labels,
                                                           int64_t nc, const uint8_t* __restrict__ occ_gt, int32_t* __restrict__ occ_out,
                                                           MmState* st) {
    long long inter = 0, uni = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < np; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t c = cells[i];
        const int32_t a = c >= 0 && c < nc && labels[c] == 0, b = occ_gt[i] != 0;
        if (occ_out) occ_out[i] = a;
        inter += a & b;
        uni += a | b;
    }
    block_add_atomic(&st->counts[0], inter);
    block_add_atomic(&st->counts[1], uni);
}

__global__ void k_counts_out(const MmState* st, int64_t* counts_out) {
    if (threadIdx.x == 0) { counts_out[0] = (int64_t)st->counts[0]; counts_out[1] = (int64_t)st->counts[1]; }
}

// ---- fixed-order fp64 sums / inclusive scan: fixed_sum (fixed_sum.h); the scan's second pass -------------------------------------
__global__ void k_chunk_add(double* __restrict__ x, int64_t n, const double* __restrict__ part) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        x[i] += part[i / FIXED_SUM_CHUNK];
}

// ---- sampler -----------------------------------------------------------------------------------------------------------------
__global__ void k_face_area(const double* __restrict__ v, int64_t nv, const int32_t* __restrict__ facets, int64_t n_facets,
                            const int32_t* __restrict__ face_ids, int64_t nfc, double* __restrict__ area, MmState* st) {
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < nfc; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = face_ids ? face_ids[j] : j;
        double ar = 0;
        if (f < 0 || f >= n_facets) {
            atomicOr(&st->err, MM_BAD_ID);
        } else {
            const int32_t ia = facets[3 * f], ib = facets[3 * f + 1], ic = facets[3 * f + 2];
            if (ia < 0 || ia >= nv || ib < 0 || ib >= nv || ic < 0 || ic >= nv) {
                atomicOr(&st->err, MM_BAD_ID);
            } else {
                const V3 a = load_v3(v, ia), b = load_v3(v, ib), c = load_v3(v, ic);
                const double ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z, wx = c.x - a.x, wy = c.y - a.y, wz = c.z - a.z;
                const double cx = uy * wz - uz * wy, cy = uz * wx - ux * wz, cz = ux * wy - uy * wx;
                ar = 0.5 * sqrt(cx * cx + cy * cy + cz * cz);
                if (!isfinite(ar)) { atomicOr(&st->err, MM_NONFINITE); ar = 0; }
            }
        }
        area[j] = ar;
    }
}

__global__ void k_sample(const double* __restrict__ v, const int32_t* __restrict__ facets, const int32_t* __restrict__ face_ids, int64_t nfc,
                         const double* __restrict__ cum, int64_t ns, uint64_t seed, float* __restrict__ pts, int32_t* __restrict__ face_out) {
    const double total = cum[nfc - 1];
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < ns; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t c = 3 * (uint64_t)i + 1;
        const double r0 = (double)((mm_hash(seed, c) >> 11) + 1) * 0x1p-53;   // (0, 1]
        double u = (double)(mm_hash(seed, c + 1) >> 11) * 0x1p-53, w = (double)(mm_hash(seed, c + 2) >> 11) * 0x1p-53;   // [0, 1)
        const double x = r0 * total;
        int64_t lo = 0, hi = nfc - 1;   // first j with cum[j] >= x (cum[nfc - 1] = total >= x)
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (cum[mid] >= x) hi = mid;
            else lo = mid + 1;
        }
        if (u + w > 1.0) { u = 1.0 - u; w = 1.0 - w; }
        const int64_t f = face_ids ? face_ids[lo] : lo;
        const V3 a = load_v3(v, facets[3 * f]), b = load_v3(v, facets[3 * f + 1]), e = load_v3(v, facets[3 * f + 2]);
        pts[3 * i] = (float)((u * (b.x - a.x) + w * (e.x - a.x)) + a.x);
        pts[3 * i + 1] = (float)((u * (b.y - a.y) + w * (e.y - a.y)) + a.y);
        pts[3 * i + 2] = (float)((u * (b.z - a.z) + w * (e.z - a.z)) + a.z);
        if (face_out) face_out[i] = (int32_t)lo;
    }
}

// ---- nearest neighbour -------------------------------------------------------------------------------------------------------
struct GridF {
    float lo[3], h, ext;   // ext: the largest extent (slack scale)
    int32_t d[3];
};

__global__ void k_bbox_f32(const float* __restrict__ p, int64_t n, MmState* st) {
    unsigned int lo[3] = {~0u, ~0u, ~0u}, hi[3] = {0, 0, 0};
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        for (int a = 0; a < 3; ++a) {
            const float x = p[3 * i + a];
            if (!isfinite(x)) { atomicOr(&st->err, MM_NONFINITE); continue; }
            const unsigned int k = f32_key(x);
            lo[a] = k < lo[a] ? k : lo[a];
            hi[a] = k > hi[a] ? k : hi[a];
        }
    for (int a = 0; a < 3; ++a) wave_minmax_atomic(lo[a], hi[a], &st->lo_bits[a], &st->hi_bits[a]);
}

__device__ __forceinline__ float tbin(float x, float lo, float h) { return (x - lo) / h; }
__device__ __forceinline__ int32_t bin_f(float t, int32_t d) {
    const float f = floorf(t);
    return f < 0.f ? 0 : (f >= (float)(d - 1) ? d - 1 : (int32_t)f);
}
__device__ __forceinline__ int64_t bin_of(const float* p, const GridF& g) {
    const int32_t bx = bin_f(tbin(p[0], g.lo[0], g.h), g.d[0]), by = bin_f(tbin(p[1], g.lo[1], g.h), g.d[1]),
                  bz = bin_f(tbin(p[2], g.lo[2], g.h), g.d[2]);
    return ((int64_t)bz * g.d[1] + by) * g.d[0] + bx;
}

__global__ void k_nn_count(const float* __restrict__ p, int64_t n, GridF g, int32_t* __restrict__ cnt) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        atomicAdd(cnt + bin_of(p + 3 * i, g), 1);
}

__global__ void k_nn_fill(const float* __restrict__ p, int64_t n, GridF g, int32_t* __restrict__ cursor, float4* __restrict__ cells) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t s = atomicAdd(cursor + bin_of(p + 3 * i, g), 1);
        cells[s] = make_float4(p[3 * i], p[3 * i + 1], p[3 * i + 2], __int_as_float((int32_t)i));
    }
}

__device__ __forceinline__ void nn_scan_bin(const int32_t* __restrict__ rowptr, const float4* __restrict__ cells, int64_t bin, float qx, float qy,
                                            float qz, float& best, int32_t& bi) {
    for (int32_t s = rowptr[bin], e = rowptr[bin + 1]; s < e; ++s) {
        const float4 c = cells[s];
        const float dx = qx - c.x, dy = qy - c.y, dz = qz - c.z;
        const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
        const int32_t j = __float_as_int(c.w);
        if (d2 < best || (d2 == best && j < bi)) { best = d2; bi = j; }
    }
}

__global__ void k_nn_query(const int32_t* __restrict__ rowptr, const float4* __restrict__ cells, GridF g, const float* __restrict__ q, int64_t nq,
                           float* __restrict__ dist, int32_t* __restrict__ idx, MmState* st) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nq; i += (int64_t)gridDim.x * blockDim.x) {
        const float qx = q[3 * i], qy = q[3 * i + 1], qz = q[3 * i + 2];
        if (!isfinite(qx) || !isfinite(qy) || !isfinite(qz)) {
            atomicOr(&st->err, MM_NONFINITE);
            dist[i] = INFINITY;
            idx[i] = -1;
            continue;
        }
        const float t[3] = {tbin(qx, g.lo[0], g.h), tbin(qy, g.lo[1], g.h), tbin(qz, g.lo[2], g.h)};
        const int32_t b[3] = {bin_f(t[0], g.d[0]), bin_f(t[1], g.d[1]), bin_f(t[2], g.d[2])};
        const int32_t rmax = max(max(max(b[0], g.d[0] - 1 - b[0]), max(b[1], g.d[1] - 1 - b[1])), max(b[2], g.d[2] - 1 - b[2]));
        // slack for the fp32 bin arithmetic of the points and of q (relative 2^-23 of |x - lo| / h, in bins), generously
        const float tq = fmaxf(fmaxf(fabsf(t[0]), fabsf(t[1])), fabsf(t[2]));
        const float slack = 1e-5f * (g.ext + g.h * (1.f + tq));
        float best = INFINITY;
        int32_t bi = INT32_MAX;
        for (int32_t r = 0; r <= rmax; ++r) {
            for (int32_t z = max(b[2] - r, 0); z <= min(b[2] + r, g.d[2] - 1); ++z)
                for (int32_t y = max(b[1] - r, 0); y <= min(b[1] + r, g.d[1] - 1); ++y) {
                    const int64_t row = ((int64_t)z * g.d[1] + y) * g.d[0];
                    if (abs(z - b[2]) == r || abs(y - b[1]) == r) {
                        for (int32_t x = max(b[0] - r, 0); x <= min(b[0] + r, g.d[0] - 1); ++x) nn_scan_bin(rowptr, cells, row + x, qx, qy, qz, best, bi);
                    } else {
                        if (b[0] - r >= 0) nn_scan_bin(rowptr, cells, row + b[0] - r, qx, qy, qz, best, bi);
                        if (r > 0 && b[0] + r < g.d[0]) nn_scan_bin(rowptr, cells, row + b[0] + r, qx, qy, qz, best, bi);
                    }
                }
            // every unvisited bin lies beyond one face of the visited box on some axis: distance >= the nearest such face
            float bound = INFINITY;
            for (int a = 0; a < 3; ++a) {
                if (b[a] - r > 0) bound = fminf(bound, (t[a] - (float)(b[a] - r)) * g.h);
                if (b[a] + r < g.d[a] - 1) bound = fminf(bound, ((float)(b[a] + r + 1) - t[a]) * g.h);
            }
            const float lb = bound * (1.f - 1e-6f) - slack;
            if (lb > 0.f && best < lb * lb) break;
        }
        dist[i] = sqrtf(best);
        idx[i] = bi;
    }
}

// ---- scratch layouts -----------------------------------------------------------------------------------------------------------
int64_t start_bins(int64_t nc) { return nc / 2 > 1 ? nc / 2 : 1; }
int64_t nn_bins(int64_t nr) { return nr > 1 ? nr : 1; }

struct LocLayout { MmState* st; int32_t *nbr, *start, *start2; int64_t bytes; };
LocLayout loc_layout(void* base, int64_t nc) {
    Take t{(char*)base, 256};
    LocLayout L{};
    L.st = (MmState*)base;
    L.nbr = t.take<int32_t>(4 * nc);
    L.start = t.take<int32_t>(start_bins(nc));
    L.start2 = t.take<int32_t>(start_bins(nc));
    L.bytes = t.off;
    return L;
}

struct SampLayout { MmState* st; double *area, *part, *total; int64_t bytes; };
SampLayout samp_layout(void* base, int64_t nfc) {
    Take t{(char*)base, 256};
    SampLayout L{};
    L.st = (MmState*)base;
    L.area = t.take<double>(nfc);
    L.part = t.take<double>(dgnn_cdiv(nfc, FIXED_SUM_CHUNK) + 1);
    L.total = t.take<double>(1);
    L.bytes = t.off;
    return L;
}

struct NnLayout { MmState* st; int32_t *cnt, *rowptr, *sums; float4* cells; double* part; int64_t bytes; };
NnLayout nn_layout(void* base, int64_t nr, int64_t nq) {
    Take t{(char*)base, 256};
    NnLayout L{};
    L.st = (MmState*)base;
    const int64_t nb = nn_bins(nr);
    L.cnt = t.take<int32_t>(nb + 1);
    L.rowptr = t.take<int32_t>(nb + 1);
    L.sums = t.take<int32_t>(dgnn_cdiv(nb + 1, 2048) + 2);
    L.cells = t.take<float4>(nr);
    L.part = t.take<double>(dgnn_cdiv(nq, FIXED_SUM_CHUNK) + 1);
    L.bytes = t.off;
    return L;
}

int mm_status(const MmState& hs, const char* what) {
    if (!hs.err) return DGNN_OK;
    dgnn_set_error("%s: %s%s%s%s", what, hs.err & MM_BAD_ID ? "an id out of range; " : "", hs.err & MM_NONFINITE ? "non-finite coordinates; " : "",
                   hs.err & MM_MALFORMED ? "facets / nfacets do not describe the tetrahedra's faces; " : "",
                   hs.err & MM_CAP ? "a point did not resolve within the walk's step cap; " : "");
    return hs.err == MM_CAP ? DGNN_E_UNSUPPORTED : DGNN_E_INVALID;
}

}  // namespace

// ================================================================================================================================
extern "C" int64_t dgnn_locate_scratch_bytes(int64_t n_cells) {
    if (n_cells < 0) return 0;
    return loc_layout(nullptr, n_cells).bytes;
}

extern "C" int dgnn_locate_points(const double* vertices, int64_t n_vertices, const int32_t* tets, int64_t n_cells, const int32_t* facets,
                                  const int32_t* nfacets, int64_t n_facets, const float* points, int64_t n_points, int32_t* cell_out,
                                  int32_t* steps_out, void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(n_vertices >= 0 && n_cells >= 0 && n_facets >= 0 && n_points >= 0 && scratch && (n_points == 0 || (points && cell_out)) &&
                     (n_vertices == 0 || vertices) && (n_cells == 0 || tets) && (n_facets == 0 || (facets && nfacets)),
                 DGNN_E_INVALID, "locate_points: bad args");
    DGNN_REQUIRE(n_cells < INT32_MAX / 4 && n_vertices < INT32_MAX && n_points < INT32_MAX, DGNN_E_UNSUPPORTED,
                 "locate_points: sizes exceed the int32 indexing");
    const LocLayout L = loc_layout(scratch, n_cells);
    const dim3 block(MESH_THREADS);
    MmState hs{};
    hs.lo64[0] = hs.lo64[1] = hs.lo64[2] = ~0ull;
    (void)hipMemcpyAsync(L.st, &hs, sizeof(MmState), hipMemcpyHostToDevice, stream);
    (void)hipMemsetAsync(L.nbr, 0x80, sizeof(int32_t) * 4 * (n_cells > 0 ? n_cells : 1), stream);
    hipLaunchKernelGGL(k_check_vertices, mesh_launch_grid(n_vertices), block, 0, stream, vertices, n_vertices, L.st);
    hipLaunchKernelGGL(k_check_ids, mesh_launch_grid(4 * n_cells), block, 0, stream, tets, 4 * n_cells, n_vertices, &L.st->err, MM_BAD_ID);
    int rc = dgnn_check_launch("locate_points (check)");
    if (rc || (rc = mm_read(&hs, L.st, sizeof(MmState), stream, "locate_points"))) return rc;   // tets are read by id below: checked first
    if ((rc = mm_status(hs, "locate_points"))) return rc;
    hipLaunchKernelGGL(k_nbr_fill, mesh_launch_grid(n_facets), block, 0, stream, tets, n_cells, facets, nfacets, n_facets, n_vertices, L.nbr, L.st);
    hipLaunchKernelGGL(k_nbr_check, mesh_launch_grid(4 * n_cells), block, 0, stream, L.nbr, n_cells, L.st);
    if ((rc = dgnn_check_launch("locate_points (neighbours)")) || (rc = mm_read(&hs, L.st, sizeof(MmState), stream, "locate_points"))) return rc;
    if ((rc = mm_status(hs, "locate_points"))) return rc;
    if (n_points == 0) {
        if (steps_out) (void)hipMemsetAsync(steps_out, 0, sizeof(int32_t), stream);
        return dgnn_check_launch("locate_points");
    }
    if (n_cells == 0) {   // no finite cell: everything is outside
        (void)hipMemsetAsync(cell_out, 0xFF, sizeof(int32_t) * n_points, stream);
        if (steps_out) (void)hipMemsetAsync(steps_out, 0, sizeof(int32_t), stream);
        return dgnn_check_launch("locate_points");
    }
    double lo[3], hi[3];
    bbox_unkey(hs.lo64, hs.hi64, lo, hi);
    const Grid g = grid_for(lo, hi, start_bins(n_cells));
    const int64_t nb = (int64_t)g.d[0] * g.d[1] * g.d[2];
    hipLaunchKernelGGL(k_fill_i32, mesh_launch_grid(nb), block, 0, stream, L.start, nb, (int32_t)INT32_MAX);
    hipLaunchKernelGGL(k_start_min, mesh_launch_grid(n_cells), block, 0, stream, vertices, tets, n_cells, g, L.start);
    hipLaunchKernelGGL(k_start_axis, mesh_launch_grid(nb / g.d[0]), block, 0, stream, L.start, g, 0, L.start2);
    hipLaunchKernelGGL(k_start_axis, mesh_launch_grid(nb / g.d[1]), block, 0, stream, L.start2, g, 1, L.start);
    hipLaunchKernelGGL(k_start_axis, mesh_launch_grid(nb / g.d[2]), block, 0, stream, L.start, g, 2, L.start2);
    hipLaunchKernelGGL(k_locate, mesh_launch_grid(n_points), block, 0, stream, vertices, tets, L.nbr, L.start2, g, points, n_points, cell_out, L.st);
    if ((rc = dgnn_check_launch("locate_points (walk)")) || (rc = mm_read(&hs, L.st, sizeof(MmState), stream, "locate_points"))) return rc;
    if (steps_out) (void)hipMemcpyAsync(steps_out, &L.st->max_steps, sizeof(int32_t), hipMemcpyDeviceToDevice, stream);
    if ((rc = mm_status(hs, "locate_points"))) return rc;
    return dgnn_check_launch("locate_points");
}

extern "C" int dgnn_mesh_iou_counts(const int32_t* cells, int64_t n_points, const int32_t* labels, int64_t n_cells, const uint8_t* occ_gt,
                                    int32_t* occ_out, int64_t* counts_out, void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(n_points >= 0 && n_cells >= 0 && counts_out && scratch && (n_points == 0 || (cells && occ_gt)) && (n_cells == 0 || labels),
                 DGNN_E_INVALID, "mesh_iou_counts: bad args");
    MmState* st = (MmState*)scratch;
    (void)hipMemsetAsync(st, 0, sizeof(MmState), stream);
    if (n_points > 0)
        hipLaunchKernelGGL(k_iou_counts, mesh_launch_grid(n_points), dim3(MESH_THREADS), 0, stream, cells, n_points, labels, n_cells, occ_gt, occ_out, st);
    hipLaunchKernelGGL(k_counts_out, dim3(1), dim3(64), 0, stream, st, counts_out);
    return dgnn_check_launch("mesh_iou_counts");
}

extern "C" int64_t dgnn_sample_faces_scratch_bytes(int64_t n_faces) {
    if (n_faces < 0) return 0;
    return samp_layout(nullptr, n_faces).bytes;
}

extern "C" int dgnn_sample_faces(const double* vertices, int64_t n_vertices, const int32_t* facets, int64_t n_facets, const int32_t* face_ids,
                                 int64_t n_faces, int64_t n_samples, uint64_t seed, float* points_out, int32_t* face_out, double* cumarea_out,
                                 void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(n_vertices >= 0 && n_facets >= 0 && n_faces >= 0 && n_samples >= 0 && scratch && (n_samples == 0 || points_out) &&
                     (n_faces == 0 || (vertices && facets)),
                 DGNN_E_INVALID, "sample_faces: bad args");
    DGNN_REQUIRE(n_faces < INT32_MAX && n_facets < INT32_MAX && n_vertices < INT32_MAX, DGNN_E_UNSUPPORTED, "sample_faces: sizes exceed the int32 indexing");
    const SampLayout L = samp_layout(scratch, n_faces);
    double* cum = cumarea_out ? cumarea_out : L.area;
    const dim3 block(MESH_THREADS);
    MmState hs{};
    (void)hipMemsetAsync(L.st, 0, sizeof(MmState), stream);
    (void)hipMemsetAsync(L.total, 0, sizeof(double), stream);
    if (n_faces > 0) {
        hipLaunchKernelGGL(k_face_area, mesh_launch_grid(n_faces), block, 0, stream, vertices, n_vertices, facets, n_facets, face_ids, n_faces, cum, L.st);
        fixed_sum(cum, n_faces, 1, L.part, L.total, stream);
        hipLaunchKernelGGL(k_chunk_add, mesh_launch_grid(n_faces), block, 0, stream, cum, n_faces, L.part);
    }
    double total = 0;
    int rc = dgnn_check_launch("sample_faces (areas)");
    if (rc || (rc = mm_read(&hs, L.st, sizeof(MmState), stream, "sample_faces")) || (rc = mm_read(&total, L.total, sizeof(double), stream, "sample_faces")))
        return rc;
    if ((rc = mm_status(hs, "sample_faces"))) return rc;
    if (n_samples == 0) return DGNN_OK;
    DGNN_REQUIRE(total > 0 && isfinite(total), DGNN_E_INVALID, "sample_faces: %lld samples asked of faces with total area %g", (long long)n_samples, total);
    hipLaunchKernelGGL(k_sample, mesh_launch_grid(n_samples), block, 0, stream, vertices, facets, face_ids, n_faces, cum, n_samples, seed, points_out, face_out);
    return dgnn_check_launch("sample_faces");
}

extern "C" int64_t dgnn_nearest_scratch_bytes(int64_t n_ref, int64_t n_query) {
    if (n_ref < 0 || n_query < 0) return 0;
    return nn_layout(nullptr, n_ref, n_query).bytes;
}

extern "C" int dgnn_nearest_neighbor(const float* ref, int64_t n_ref, const float* query, int64_t n_query, float* dist_out, int32_t* idx_out,
                                     double* sum_out, void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(n_ref > 0 && n_query >= 0 && ref && scratch && (n_query == 0 || (query && dist_out && idx_out)), DGNN_E_INVALID,
                 "nearest_neighbor: bad args (%lld reference points)", (long long)n_ref);
    DGNN_REQUIRE(n_ref < INT32_MAX / 2 && n_query < INT32_MAX, DGNN_E_UNSUPPORTED, "nearest_neighbor: sizes exceed the int32 indexing");
    const NnLayout L = nn_layout(scratch, n_ref, n_query);
    const dim3 block(MESH_THREADS);
    MmState hs{};
    hs.lo_bits[0] = hs.lo_bits[1] = hs.lo_bits[2] = ~0u;
    (void)hipMemcpyAsync(L.st, &hs, sizeof(MmState), hipMemcpyHostToDevice, stream);
    hipLaunchKernelGGL(k_bbox_f32, mesh_launch_grid(n_ref), block, 0, stream, ref, n_ref, L.st);
    int rc = dgnn_check_launch("nearest_neighbor (bbox)");
    if (rc || (rc = mm_read(&hs, L.st, sizeof(MmState), stream, "nearest_neighbor"))) return rc;
    if ((rc = mm_status(hs, "nearest_neighbor"))) return rc;
    double lo[3], hi[3];
    for (int a = 0; a < 3; ++a) { lo[a] = f32_unkey(hs.lo_bits[a]); hi[a] = f32_unkey(hs.hi_bits[a]); }
    const Grid g64 = grid_for(lo, hi, nn_bins(n_ref));
    GridF g{};
    for (int a = 0; a < 3; ++a) { g.lo[a] = (float)lo[a]; g.d[a] = g64.d[a]; g.ext = fmaxf(g.ext, (float)(hi[a] - lo[a])); }
    g.h = (float)g64.h;
    const int64_t nb = (int64_t)g.d[0] * g.d[1] * g.d[2];
    (void)hipMemsetAsync(L.cnt, 0, sizeof(int32_t) * (nb + 1), stream);
    hipLaunchKernelGGL(k_nn_count, mesh_launch_grid(n_ref), block, 0, stream, ref, n_ref, g, L.cnt);
    if ((rc = dgnn_exclusive_scan_i32(L.cnt, nb, L.rowptr, L.sums, stream))) return rc;
    (void)hipMemcpyAsync(L.cnt, L.rowptr, sizeof(int32_t) * (nb + 1), hipMemcpyDeviceToDevice, stream);
    hipLaunchKernelGGL(k_nn_fill, mesh_launch_grid(n_ref), block, 0, stream, ref, n_ref, g, L.cnt, L.cells);
    if (n_query > 0) hipLaunchKernelGGL(k_nn_query, mesh_launch_grid(n_query), block, 0, stream, L.rowptr, L.cells, g, query, n_query, dist_out, idx_out, L.st);
    if (sum_out) {
        (void)hipMemsetAsync(sum_out, 0, sizeof(double), stream);
        if (n_query > 0) fixed_sum(dist_out, n_query, 0, L.part, sum_out, stream);
    }
    if ((rc = dgnn_check_launch("nearest_neighbor (query)")) || (rc = mm_read(&hs, L.st, sizeof(MmState), stream, "nearest_neighbor"))) return rc;
    return mm_status(hs, "nearest_neighbor");
}
