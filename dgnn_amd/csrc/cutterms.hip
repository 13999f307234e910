// Per-facet capacities of the graph cut from the geometry of `<scene>_3dt.npz` (include/dgnn_hip.h: dgnn_facet_cut_terms): the
// reference leaves them at one (processing/generate_mesh.py:34-40, its TODO), the paper's regulariser charges a facet by its area or by the
// beta-skeleton term 1 - min(cos phi, cos psi) of Labatut et al. 2009.
//
//   k_facet_terms   one thread per facet: the nfacets row decides whether the facet is a graph row (both cells finite); a row gathers its
//                   three vertices (area) or its three vertices and the four vertices of each of its two cells (beta: the circumsphere is
//                   recomputed per side, no per-cell pass; the arithmetic is facet_geom.h's, which facetgeom.hip runs in two passes: DESIGN
//                   §23 compares them).  beta quantises at once; area stores A_f (0 for the other facets).
//   fixed_sum       the sum of the A_f in a fixed order (fixed_sum.h)
//   k_area_quantise q_f = A_f / mean, w_f = rint(binary_weight q_f)
// All fp64, the operation order of the header, no contraction (the build's -ffp-contract=off); the counters are integer atomics: reruns are
// bit-identical.
#include <math.h>

#include "common.h"
#include "mesh_common.h"
#include "facet_geom.h"
#include "tet_common.h"
#include "fixed_sum.h"

namespace {

using dgnn_exact::FacetPlane;
using dgnn_exact::V3;
using dgnn_exact::load_v3;

constexpr int32_t CT_BAD_ID = 1, CT_MALFORMED = 2, CT_BAD_MEAN = 4, CT_W_RANGE = 8;

struct CtState {
    int32_t err, max_w, pad[2];
    unsigned long long rows, neutral, zeros;
};

// per-thread counters of a kernel, added up per wave (every lane arrives: the callers' loops are block-uniform) and sent with one atomic each
struct CtCounts { int32_t rows, neutral, zeros, max_w; };
__device__ __forceinline__ void ct_flush(CtCounts c, CtState* st) {
    c.rows = wave_sum(c.rows);
    c.neutral = wave_sum(c.neutral);
    c.zeros = wave_sum(c.zeros);
    for (int o = 32; o > 0; o >>= 1) {
        const int32_t m = __shfl_xor(c.max_w, o);
        c.max_w = m > c.max_w ? m : c.max_w;
    }
    if (lane_id() != 0) return;
    if (c.rows) atomicAdd(&st->rows, (unsigned long long)c.rows);
    if (c.neutral) atomicAdd(&st->neutral, (unsigned long long)c.neutral);
    if (c.zeros) atomicAdd(&st->zeros, (unsigned long long)c.zeros);
    if (c.max_w) atomicMax(&st->max_w, c.max_w);
}

// w = (int32) rint(bw q): fp64 product, half to even; anything not below 2^30 (a NaN too) is an error
__device__ __forceinline__ int32_t quantise(double bw, double q, CtCounts& c, CtState* st) {
    const double x = rint(bw * q);
    if (!(x < 1073741824.0) || !(x >= 0.0)) { atomicOr(&st->err, CT_W_RANGE); return 0; }
    const int32_t w = (int32_t)x;
    c.zeros += w == 0;
    c.max_w = w > c.max_w ? w : c.max_w;
    return w;
}

// cos phi of the facet `p` = (ia, ib, ic) seen from the cell `cell`, its circumsphere recomputed here (facet_geom.h: sphere_cosine; 0 and
// *neutral += 1 for a degenerate side).  false: the facet is not a face of the cell / an id out of range.
__device__ __forceinline__ bool side_cosine(const double* __restrict__ v, int64_t nv, const int32_t* __restrict__ tets, int32_t cell, int32_t ia,
                                            int32_t ib, int32_t ic, const FacetPlane& p, double* cosine, int* neutral, CtState* st) {
    int32_t t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        t[k] = tets[4 * (int64_t)cell + k];
        if (t[k] < 0 || t[k] >= nv) { atomicOr(&st->err, CT_BAD_ID); return false; }
    }
    const int slot = facet_opposite_slot(t, ia, ib, ic);
    if (slot < 0) { atomicOr(&st->err, CT_MALFORMED); return false; }
    const dgnn_exact::Sphere s = dgnn_exact::cell_sphere(load_v3(v, t[0]), load_v3(v, t[1]), load_v3(v, t[2]), load_v3(v, t[3]));
    *cosine = dgnn_exact::sphere_cosine(s.o, s.R, p, load_v3(v, row_at(t, slot)), neutral);
    return true;
}

// KIND 1: val[f] = A_f (quantised later); KIND 2: q, w at once.  Every facet that is not a graph row gets 0 everywhere.  (waves_per_eu, a
// minimum, is on both instantiations: the beta form stays at 4 waves per SIMD, 128 VGPRs without scratch -- left alone the scheduler takes 130
// and loses a wave; the area form has 34 VGPRs and 8 waves with or without it.)
template <int KIND>
__global__ void __launch_bounds__(MESH_THREADS) __attribute__((amdgpu_waves_per_eu(4))) k_facet_terms(const double* __restrict__ v, int64_t nv, const int32_t* __restrict__ tets, int64_t nc,
                                                            const int32_t* __restrict__ facets, const int32_t* __restrict__ nfacets, int64_t nf,
                                                            double bw, double* __restrict__ val, double* __restrict__ q_out,
                                                            int32_t* __restrict__ w_out, CtState* st) {
    CtCounts cnt{0, 0, 0, 0};
    for (int64_t f0 = blockIdx.x * (int64_t)blockDim.x; f0 < nf; f0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = f0 + threadIdx.x;
        if (f >= nf) continue;
        const int32_t c0 = nfacets[2 * f], c1 = nfacets[2 * f + 1];
        const int32_t ia = facets[3 * f], ib = facets[3 * f + 1], ic = facets[3 * f + 2];
        double q = 0;
        int32_t w = 0;
        bool ok = true;
        if (c0 >= nc || c1 >= nc || ia < 0 || ia >= nv || ib < 0 || ib >= nv || ic < 0 || ic >= nv) {
            atomicOr(&st->err, CT_BAD_ID);
            ok = false;
        }
        if (ok && c0 >= 0 && c1 >= 0) {
            ++cnt.rows;
            const FacetPlane p = dgnn_exact::facet_plane(load_v3(v, ia), load_v3(v, ib), load_v3(v, ic));
            if (KIND == 1) {
                q = 0.5 * p.nn;
            } else {
                double cos0 = 0, cos1 = 0;
                int neutral = 0;
                if (side_cosine(v, nv, tets, c0, ia, ib, ic, p, &cos0, &neutral, st) && side_cosine(v, nv, tets, c1, ia, ib, ic, p, &cos1, &neutral, st)) {
                    cnt.neutral += neutral;
                    q = 1.0 - (cos0 < cos1 ? cos0 : cos1);
                    w = quantise(bw, q, cnt, st);
                }
            }
        }
        if (KIND == 1) {
            val[f] = q;
        } else {
            if (q_out) q_out[f] = q;
            w_out[f] = w;
        }
    }
    ct_flush(cnt, st);
}

// mean = total / rows (one division, the same in every thread); a mean that is 0 or not finite is an error and leaves zeros
__global__ void __launch_bounds__(MESH_THREADS) k_area_quantise(const double* __restrict__ area, const int32_t* __restrict__ nfacets, int64_t nf,
                                                              const double* __restrict__ total, double bw, double* __restrict__ q_out,
                                                              int32_t* __restrict__ w_out, CtState* st) {
    CtCounts cnt{0, 0, 0, 0};
    const double mean = *total / (double)st->rows;   // rows: written by the launch before this one
    const bool bad = st->rows != 0 && !(mean > 0 && isfinite(mean));
    if (bad && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&st->err, CT_BAD_MEAN);
    for (int64_t f0 = blockIdx.x * (int64_t)blockDim.x; f0 < nf; f0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = f0 + threadIdx.x;
        if (f >= nf) continue;
        double q = 0;
        int32_t w = 0;
        if (!bad && nfacets[2 * f] >= 0 && nfacets[2 * f + 1] >= 0) {
            q = area[f] / mean;
            w = quantise(bw, q, cnt, st);
        }
        if (q_out) q_out[f] = q;
        w_out[f] = w;
    }
    cnt.rows = 0;
    ct_flush(cnt, st);
}

__global__ void k_terms_stats(const CtState* st, int64_t* stats_out) {
    if (threadIdx.x == 0) {
        stats_out[0] = (int64_t)st->rows;
        stats_out[1] = (int64_t)st->neutral;
        stats_out[2] = (int64_t)st->zeros;
        stats_out[3] = st->max_w;
    }
}

struct CtLayout { CtState* st; double *area, *part, *total; int64_t bytes; };
CtLayout ct_layout(void* base, int64_t nf) {
    Take t{(char*)base, 256};
    CtLayout L{};
    L.st = (CtState*)base;
    L.area = t.take<double>(nf);
    L.part = t.take<double>(dgnn_cdiv(nf, FIXED_SUM_CHUNK) + 1);
    L.total = t.take<double>(1);
    L.bytes = t.off;
    return L;
}

}  // namespace

extern "C" int64_t dgnn_facet_cut_terms_scratch_bytes(int64_t n_facets) {
    if (n_facets < 0) return 0;
    return ct_layout(nullptr, n_facets).bytes;
}

extern "C" int dgnn_facet_cut_terms(const double* vertices, int64_t n_vertices, const int32_t* tets, int64_t n_cells, const int32_t* facets,
                                    const int32_t* nfacets, int64_t n_facets, int kind, double binary_weight, double* q_out, int32_t* w_out,
                                    int64_t* stats_out, void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(n_vertices >= 0 && n_cells >= 0 && n_facets >= 0 && scratch && (n_facets == 0 || (facets && nfacets && w_out)) &&
                     (n_vertices == 0 || vertices) && (n_cells == 0 || tets),
                 DGNN_E_INVALID, "facet_cut_terms: bad args");
    DGNN_REQUIRE(kind == 1 || kind == 2, DGNN_E_INVALID, "facet_cut_terms: kind %d (1 = area, 2 = beta)", kind);
    DGNN_REQUIRE(isfinite(binary_weight) && binary_weight >= 0, DGNN_E_INVALID, "facet_cut_terms: binary_weight %g must be finite and >= 0",
                 binary_weight);
    DGNN_REQUIRE(n_cells < INT32_MAX / 4 && n_vertices < INT32_MAX && n_facets < INT32_MAX, DGNN_E_UNSUPPORTED,
                 "facet_cut_terms: sizes exceed the int32 indexing");
    const CtLayout L = ct_layout(scratch, n_facets);
    const dim3 block(MESH_THREADS), grid = mesh_launch_grid(n_facets);
    (void)hipMemsetAsync(L.st, 0, sizeof(CtState), stream);
    if (n_facets > 0) {
        if (kind == 1) {
            (void)hipMemsetAsync(L.total, 0, sizeof(double), stream);
            hipLaunchKernelGGL(k_facet_terms<1>, grid, block, 0, stream, vertices, n_vertices, tets, n_cells, facets, nfacets, n_facets, binary_weight,
                               L.area, q_out, w_out, L.st);
            fixed_sum(L.area, n_facets, 0, L.part, L.total, stream);
            hipLaunchKernelGGL(k_area_quantise, grid, block, 0, stream, L.area, nfacets, n_facets, L.total, binary_weight, q_out, w_out, L.st);
        } else {
            hipLaunchKernelGGL(k_facet_terms<2>, grid, block, 0, stream, vertices, n_vertices, tets, n_cells, facets, nfacets, n_facets, binary_weight,
                               L.area, q_out, w_out, L.st);
        }
    }
    if (stats_out) hipLaunchKernelGGL(k_terms_stats, dim3(1), dim3(64), 0, stream, L.st, stats_out);
    CtState hs{};
    int rc = dgnn_check_launch("facet_cut_terms");
    if (rc || (rc = mm_read(&hs, L.st, sizeof(CtState), stream, "facet_cut_terms"))) return rc;
    if (hs.err) {
        dgnn_set_error("facet_cut_terms: %s%s%s%s", hs.err & CT_BAD_ID ? "an id out of range; " : "",
                       hs.err & CT_MALFORMED ? "a facet is not a face of the cell its nfacets row names; " : "",
                       hs.err & CT_BAD_MEAN ? "the mean facet area is 0 or not finite; " : "",
                       hs.err & CT_W_RANGE ? "a weight is not below 2^30; " : "");
        return DGNN_E_INVALID;
    }
    return DGNN_OK;
}
