// Connected components of a triangle mesh on the device (the `components` metric and the small-component filter of `generate`; the
// reference gets them from trimesh's split / body_count).  DESIGN §22.
//
//   components  faces that share an undirected edge are connected, however many faces meet on it; a shared vertex alone does not connect.
//               The sorted edge keys of mesh_faces.h carry the face as value; every element whose key equals its predecessor's joins the two
//               faces in a union-find over the faces (the larger root hooked under the smaller by compare-and-swap: parents only decrease,
//               so every retry loop ends and no thread waits for another).  A second launch points every face at its root = the smallest
//               face id of its component; the roots are flagged, scanned and gathered: component c is the one with the c-th smallest root.
//   measures    the faces sorted stably by component (ascending face id inside one); per face one fp64 area and one fp64 volume term; per
//               component a two-level serial sum in a fixed order.  Bit-identical from run to run.
//   keep        `largest` (ties to the smaller id) or `at least n faces`: integer logic.
#include "mesh_faces.h"

namespace {

constexpr int MC_CHUNK = 256;   // sorted positions per serial partial sum
constexpr int MC_RULE_LARGEST = 0, MC_RULE_MIN_FACES = 1;

__global__ void k_iota(int32_t* __restrict__ x, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) x[i] = (int32_t)i;
}

// after every union has finished: root[f] = the smallest face id of f's component, is_root[f] = (f is that face)
__global__ void k_face_roots(int32_t* parent, int64_t n, int32_t* __restrict__ root, int32_t* __restrict__ is_root) {
    for (int64_t f = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; f < n; f += (int64_t)gridDim.x * blockDim.x) {
        const int32_t r = uf_find(parent, (int32_t)f);
        root[f] = r;
        is_root[f] = r == (int32_t)f;
    }
}

// rank[f] = number of roots below f: the component number of root f
__global__ void k_number(const int32_t* __restrict__ root, const int32_t* __restrict__ rank, int64_t n, int32_t* __restrict__ comp) {
    for (int64_t f = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; f < n; f += (int64_t)gridDim.x * blockDim.x) comp[f] = rank[root[f]];
}

// ---- measures ----------------------------------------------------------------------------------------------------------------
__global__ void k_check_measures(const int32_t* __restrict__ faces, const int32_t* __restrict__ comp, int64_t n, int64_t nv, int64_t k, MtState* st) {
    for (int64_t f = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; f < n; f += (int64_t)gridDim.x * blockDim.x) {
        const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2], q = comp[f];
        if (a < 0 || a >= nv || b < 0 || b >= nv || c < 0 || c >= nv || q < 0 || q >= k) atomicOr(&st->err, MT_BAD_ID);
    }
}

__global__ void k_comp_keys(const int32_t* __restrict__ comp, int64_t n, uint64_t* __restrict__ keys, int32_t* __restrict__ vals) {
    for (int64_t f = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; f < n; f += (int64_t)gridDim.x * blockDim.x) {
        keys[f] = (uint64_t)(uint32_t)comp[f];
        vals[f] = (int32_t)f;
    }
}

// sorted position i holds face order[i] of component keys[i]: the first and one past the last position of every component, and the two
// terms of the face (the expressions of include/dgnn_hip.h; every product, sum and the square root round on their own)
__global__ void k_terms(const double* __restrict__ v, const int32_t* __restrict__ faces, const uint64_t* __restrict__ keys,
                        const int32_t* __restrict__ order, int64_t n, int32_t* __restrict__ seg_begin, int32_t* __restrict__ seg_end,
                        double* __restrict__ t_area, double* __restrict__ t_vol) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t c = keys[i];
        if (i == 0 || keys[i - 1] != c) seg_begin[c] = (int32_t)i;
        if (i == n - 1 || keys[i + 1] != c) seg_end[c] = (int32_t)(i + 1);
        const int64_t f = order[i];
        const double* p0 = v + 3 * (int64_t)faces[3 * f];
        const double* p1 = v + 3 * (int64_t)faces[3 * f + 1];
        const double* p2 = v + 3 * (int64_t)faces[3 * f + 2];
        const double ax = p0[0], ay = p0[1], az = p0[2], bx = p1[0], by = p1[1], bz = p1[2], cx = p2[0], cy = p2[1], cz = p2[2];
        const double ux = bx - ax, uy = by - ay, uz = bz - az, wx = cx - ax, wy = cy - ay, wz = cz - az;
        const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
        t_area[i] = 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
        t_vol[i] = ((ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz)) + az * (bx * cy - by * cx)) / 6.0;
    }
}

// one thread per chunk of MC_CHUNK sorted positions: every run of one component inside the chunk is summed serially from 0.0 in ascending
// position, and the sum is left at the run's first position (in place: a thread touches its own chunk only)
__global__ void k_run_partials(const uint64_t* __restrict__ keys, int64_t n, double* __restrict__ t_area, double* __restrict__ t_vol) {
    const int64_t nch = (n + MC_CHUNK - 1) / MC_CHUNK;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < nch; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = t * MC_CHUNK, e = b + MC_CHUNK < n ? b + MC_CHUNK : n;
        int64_t first = b;
        uint64_t c = keys[b];
        double sa = 0.0, sv = 0.0;
        for (int64_t i = b; i < e; ++i) {
            const uint64_t ci = keys[i];
            if (ci != c) {
                t_area[first] = sa;
                t_vol[first] = sv;
                first = i;
                c = ci;
                sa = 0.0;
                sv = 0.0;
            }
            sa += t_area[i];
            sv += t_vol[i];
        }
        t_area[first] = sa;
        t_vol[first] = sv;
    }
}

// one thread per component: its run partials (at its first position and at every multiple of MC_CHUNK inside it) added serially from 0.0
// in ascending position.  Eight partials are requested at a time; the additions keep their order.
__global__ void k_comp_sums(const int32_t* __restrict__ seg_begin, const int32_t* __restrict__ seg_end, int64_t k, const double* __restrict__ t_area,
                            const double* __restrict__ t_vol, int64_t* __restrict__ count, double* __restrict__ area, double* __restrict__ vol) {
    for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < k; c += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = seg_begin[c], e = seg_end[c];
        double sa = 0.0, sv = 0.0;
        if (e > s) {
            const int64_t c0 = s / MC_CHUNK, pieces = (e - 1) / MC_CHUNK - c0 + 1;
            for (int64_t j = 0; j < pieces; j += 8) {
                double a[8], w[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int64_t pos = j + u == 0 ? s : (c0 + j + u) * MC_CHUNK;
                    const bool live = j + u < pieces;
                    a[u] = live ? t_area[pos] : 0.0;
                    w[u] = live ? t_vol[pos] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (j + u < pieces) { sa += a[u]; sv += w[u]; }
            }
        }
        count[c] = e > s ? e - s : 0;
        area[c] = sa;
        vol[c] = sv;
    }
}

// ---- keep --------------------------------------------------------------------------------------------------------------------
// one block: the component with the most faces, ties to the smaller id -> *best (-1 without components)
__global__ void __launch_bounds__(MESH_THREADS) k_largest(const int64_t* __restrict__ count, int64_t k, int32_t* __restrict__ best) {
    __shared__ long long s_cnt[MESH_THREADS];
    __shared__ int32_t s_id[MESH_THREADS];
    long long bc = -1;
    int32_t bi = -1;
    for (int64_t c = threadIdx.x; c < k; c += MESH_THREADS)   // ascending ids per thread: `>` keeps the smaller id on a tie
        if (count[c] > bc) { bc = count[c]; bi = (int32_t)c; }
    s_cnt[threadIdx.x] = bc;
    s_id[threadIdx.x] = bi;
    __syncthreads();
    for (int o = MESH_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const long long oc = s_cnt[threadIdx.x + o];
            const int32_t oi = s_id[threadIdx.x + o];
            if (oi >= 0 && (oc > s_cnt[threadIdx.x] || (oc == s_cnt[threadIdx.x] && oi < s_id[threadIdx.x]))) {
                s_cnt[threadIdx.x] = oc;
                s_id[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *best = s_id[0];
}

__global__ void k_keep(const int32_t* __restrict__ comp, int64_t n, const int64_t* __restrict__ count, int64_t k, int rule, int64_t min_faces,
                       const int32_t* __restrict__ best, int32_t* __restrict__ keep, unsigned long long* n_kept, MtState* st) {
    unsigned long long kept = 0;
    for (int64_t f = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; f < n; f += (int64_t)gridDim.x * blockDim.x) {
        const int32_t c = comp[f];
        int32_t kp = 0;
        if (c < 0 || c >= k) atomicOr(&st->err, MT_BAD_ID);
        else kp = rule == MC_RULE_LARGEST ? c == *best : count[c] >= min_faces;
        keep[f] = kp;
        kept += kp;
    }
    wave_add_atomic(kept, n_kept);   // every lane is here: the loop has ended for all of them
}

// ---- scratch layouts ---------------------------------------------------------------------------------------------------------
struct CompLayout { MtState* st; SortBufs S; int32_t *parent, *root, *is_root, *rank, *scan_sums; int64_t bytes; };
CompLayout comp_layout(void* base, int64_t nf) {
    Take t{(char*)base, 256};
    CompLayout L{};
    L.st = (MtState*)base;
    take_sort(t, 3 * nf, L.S);
    L.parent = t.take<int32_t>(nf);
    L.root = t.take<int32_t>(nf);
    L.is_root = t.take<int32_t>(nf);
    L.rank = t.take<int32_t>(nf + 1);
    L.scan_sums = t.take<int32_t>(dgnn_cdiv(nf, 2048) + 4);
    L.bytes = t.off;
    return L;
}

struct MeasLayout { MtState* st; SortBufs S; int32_t *seg_begin, *seg_end; double *t_area, *t_vol; int64_t bytes; };
MeasLayout meas_layout(void* base, int64_t nf, int64_t k) {
    Take t{(char*)base, 256};
    MeasLayout L{};
    L.st = (MtState*)base;
    take_sort(t, nf, L.S);
    L.seg_begin = t.take<int32_t>(k);
    L.seg_end = t.take<int32_t>(k);
    L.t_area = t.take<double>(nf);
    L.t_vol = t.take<double>(nf);
    L.bytes = t.off;
    return L;
}

}  // namespace

// ================================================================================================================================
extern "C" int64_t dgnn_mesh_components_scratch_bytes(int64_t n_faces) {
    if (n_faces < 0 || 3 * n_faces >= (int64_t)INT32_MAX) return 0;
    return comp_layout(nullptr, n_faces).bytes;
}

extern "C" int dgnn_mesh_components(const int32_t* faces, int64_t n_faces, int64_t n_vertices, int32_t* comp_out, int32_t* n_components_out,
                                    void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(n_faces < INT32_MAX / 3 + 1 && 3 * n_faces < (int64_t)INT32_MAX && n_vertices < INT32_MAX, DGNN_E_UNSUPPORTED,
                 "mesh_components: sizes exceed the int32 indexing");   // (before the pointers: no scratch size exists for such a mesh)
    DGNN_REQUIRE(n_faces >= 0 && n_vertices >= 0 && scratch && n_components_out && (n_faces == 0 || (faces && comp_out)), DGNN_E_INVALID,
                 "mesh_components: bad args");
    const CompLayout L = comp_layout(scratch, n_faces);
    const dim3 block(MESH_THREADS);
    (void)hipMemsetAsync(L.st, 0, sizeof(MtState), stream);
    (void)hipMemsetAsync(n_components_out, 0, sizeof(int32_t), stream);
    if (n_faces > 0) hipLaunchKernelGGL(k_check_faces, mesh_launch_grid(n_faces), block, 0, stream, faces, n_faces, n_vertices, L.st);
    MtState hs{};
    int rc = mt_read_status(&hs, L.st, stream, "mesh_components");
    if (rc || n_faces == 0) return rc;
    const int vb = key_bits(n_vertices);
    const int64_t n3 = 3 * n_faces;
    int cur = 0;
    hipLaunchKernelGGL(k_edge_keys, mesh_launch_grid(n3), block, 0, stream, faces, n3, vb, 1, L.S.keys[0], L.S.vals[0]);
    hipLaunchKernelGGL(k_iota, mesh_launch_grid(n_faces), block, 0, stream, L.parent, n_faces);
    if ((rc = sort_pairs(L.S, n3, 2 * vb, stream, &cur))) return rc;
    hipLaunchKernelGGL(k_link_union, mesh_launch_grid(n3), block, 0, stream, L.S.keys[cur], L.S.vals[cur], n3, L.parent);
    hipLaunchKernelGGL(k_face_roots, mesh_launch_grid(n_faces), block, 0, stream, L.parent, n_faces, L.root, L.is_root);
    if ((rc = dgnn_exclusive_scan_i32(L.is_root, n_faces, L.rank, L.scan_sums, stream))) return rc;
    hipLaunchKernelGGL(k_number, mesh_launch_grid(n_faces), block, 0, stream, L.root, L.rank, n_faces, comp_out);
    (void)hipMemcpyAsync(n_components_out, L.rank + n_faces, sizeof(int32_t), hipMemcpyDeviceToDevice, stream);
    return dgnn_check_launch("mesh_components");
}

extern "C" int64_t dgnn_mesh_component_measures_scratch_bytes(int64_t n_faces, int64_t n_components) {
    if (n_faces < 0 || n_components < 0 || 3 * n_faces >= (int64_t)INT32_MAX) return 0;
    return meas_layout(nullptr, n_faces, n_components).bytes;
}

extern "C" int dgnn_mesh_component_measures(const double* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const int32_t* comp,
                                            int64_t n_components, int64_t* n_faces_out, double* area_out, double* volume_out, void* scratch,
                                            void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t k = n_components;
    DGNN_REQUIRE(n_faces < INT32_MAX / 3 + 1 && 3 * n_faces < (int64_t)INT32_MAX && n_vertices < INT32_MAX, DGNN_E_UNSUPPORTED,
                 "mesh_component_measures: sizes exceed the int32 indexing");
    DGNN_REQUIRE(n_faces >= 0 && n_vertices >= 0 && k >= 0 && scratch && (n_faces == 0 || (vertices && faces && comp)) &&
                     (k == 0 || (n_faces_out && area_out && volume_out)),
                 DGNN_E_INVALID, "mesh_component_measures: bad args");
    DGNN_REQUIRE(k <= n_faces, DGNN_E_INVALID, "mesh_component_measures: %lld components for %lld faces", (long long)k, (long long)n_faces);
    DGNN_REQUIRE(k > 0 || n_faces == 0, DGNN_E_INVALID, "mesh_component_measures: a component id out of range (%lld faces, no components)",
                 (long long)n_faces);
    if (k == 0) return DGNN_OK;
    const MeasLayout L = meas_layout(scratch, n_faces, k);
    const dim3 block(MESH_THREADS);
    (void)hipMemsetAsync(L.st, 0, sizeof(MtState), stream);
    hipLaunchKernelGGL(k_check_measures, mesh_launch_grid(n_faces), block, 0, stream, faces, comp, n_faces, n_vertices, k, L.st);
    MtState hs{};
    int rc = mt_read_status(&hs, L.st, stream, "mesh_component_measures");
    if (rc) return rc;
    int cur = 0;
    hipLaunchKernelGGL(k_comp_keys, mesh_launch_grid(n_faces), block, 0, stream, comp, n_faces, L.S.keys[0], L.S.vals[0]);
    if ((rc = sort_pairs(L.S, n_faces, key_bits(k), stream, &cur))) return rc;
    (void)hipMemsetAsync(L.seg_begin, 0, sizeof(int32_t) * k, stream);   // a component id without faces: an empty segment
    (void)hipMemsetAsync(L.seg_end, 0, sizeof(int32_t) * k, stream);
    hipLaunchKernelGGL(k_terms, mesh_launch_grid(n_faces), block, 0, stream, vertices, faces, L.S.keys[cur], L.S.vals[cur], n_faces, L.seg_begin, L.seg_end,
                       L.t_area, L.t_vol);
    hipLaunchKernelGGL(k_run_partials, mesh_launch_grid(dgnn_cdiv(n_faces, MC_CHUNK)), block, 0, stream, L.S.keys[cur], n_faces, L.t_area, L.t_vol);
    hipLaunchKernelGGL(k_comp_sums, mesh_launch_grid(k), block, 0, stream, L.seg_begin, L.seg_end, k, L.t_area, L.t_vol, n_faces_out, area_out, volume_out);
    return dgnn_check_launch("mesh_component_measures");
}

extern "C" int64_t dgnn_mesh_component_keep_scratch_bytes(void) { return 512; }

extern "C" int dgnn_mesh_component_keep(const int32_t* comp, int64_t n_faces, const int64_t* component_faces, int64_t n_components, int rule,
                                        int64_t min_faces, int32_t* keep_out, int64_t* n_kept_out, void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(n_faces >= 0 && n_components >= 0 && scratch && n_kept_out && (n_faces == 0 || (comp && keep_out)) &&
                     (n_components == 0 || component_faces),
                 DGNN_E_INVALID, "mesh_component_keep: bad args");
    DGNN_REQUIRE(rule == MC_RULE_LARGEST || (rule == MC_RULE_MIN_FACES && min_faces >= 1), DGNN_E_INVALID,
                 "mesh_component_keep: rule %d, min_faces %lld (0 = largest; 1 = at least min_faces >= 1 faces)", rule, (long long)min_faces);
    DGNN_REQUIRE(n_faces < INT32_MAX && n_components < INT32_MAX, DGNN_E_UNSUPPORTED, "mesh_component_keep: sizes exceed the int32 indexing");
    MtState* st = (MtState*)scratch;
    int32_t* best = (int32_t*)((char*)scratch + 256);
    (void)hipMemsetAsync(st, 0, sizeof(MtState), stream);
    (void)hipMemsetAsync(n_kept_out, 0, sizeof(int64_t), stream);
    if (n_faces > 0) {
        if (rule == MC_RULE_LARGEST) hipLaunchKernelGGL(k_largest, dim3(1), dim3(MESH_THREADS), 0, stream, component_faces, n_components, best);
        hipLaunchKernelGGL(k_keep, mesh_launch_grid(n_faces), dim3(MESH_THREADS), 0, stream, comp, n_faces, component_faces, n_components, rule, min_faces, best,
                           keep_out, (unsigned long long*)n_kept_out, st);
    }
    MtState hs{};
    return mt_read_status(&hs, st, stream, "mesh_component_keep");
}
