// Training-mode conv layer as ONE call each way (SurfaceNet.forward :214-219 + autograd at runModel.py:279).
//
// The training step runs on 4-hop blocks of ~10^5 cells: every kernel is short (10-100 us) and the step was bound by the ~250
// launches issued one by one from Python, not by a kernel.  These two entry points issue a layer's whole launch chain from
// C++ -- the same kernels as the separate entry points, in the same order, so results are bit-identical to calling them one by
// one (tests/test_gpu_train.py) -- into caller-provided buffers; nothing allocates or synchronises.
//
//   forward : a = mean_j x_j * (We.A + be)          dgnn_sage_aggregate_fwd   (rowptr == NULL: a = x, a plain Linear + BN block)
//             z = a.Wj^T + x_dst.Wi^T + bj           dgnn_linear_fwd / _x3
//             mean, var (+ running statistics),      dgnn_bn_batch_stats_fold (= dgnn_bn_batch_stats + dgnn_bn_fold, the fold computed
//             scale, shift                             by the finalising kernel on the values it has just stored)
//             y = relu(z * scale + shift)            dgnn_scale_shift_act
//   backward: dz, dgamma, dbeta                      dgnn_bn_relu_bwd
//             dWj = dz^T a, dWi = dz^T x_dst, dbj    dgnn_linear_wgrad / _x3, dgnn_colsum
//             da = dz.Wj                              dgnn_linear_fwd on Wj^T (transposed here)
//             dx_src, dWe, dbe                        dgnn_sage_aggregate_bwd   (dx_src == NULL: first layer, x is data)
//             dx_src[:n_dst] += dz.Wi                 dgnn_linear_fwd with DGNN_LINEAR_ACCUMULATE
#include <cstdlib>

#include "common.h"
#include "reduce_common.h"

namespace {

__global__ void k_transpose(const float* __restrict__ in, int rows, int cols, float* __restrict__ out) {
    const int n = rows * cols;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int r = i / cols, c = i - r * cols;
        out[c * rows + r] = in[i];
    }
}
// two matrices of one shape in one launch (lin_j and lin_i of a layer)
__global__ void k_transpose2(const float* __restrict__ in0, const float* __restrict__ in1, int rows, int cols, float* __restrict__ out0,
                             float* __restrict__ out1) {
    const int n = rows * cols;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 2 * n; i += gridDim.x * blockDim.x) {
        const int j = i < n ? i : i - n;
        const int r = j / cols, c = j - r * cols;
        (i < n ? out0 : out1)[c * rows + r] = (i < n ? in0 : in1)[j];
    }
}

inline int64_t align4(int64_t v) { return (v + 3) & ~(int64_t)3; }

// every layer's lin_j / lin_i transposed by ONE launch at the start of a backward pass (was one or two launches per layer)
struct TrJobs {
    const float* in[16];
    float* out[16];
    int rows[16], cols[16], end[16];   // end[j] = elements of jobs 0 .. j
    int n;
};
__global__ void k_transpose_many(TrJobs jobs) {
    const int total = jobs.end[jobs.n - 1];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        int j = 0;
        while (i >= jobs.end[j]) ++j;
        const int e = i - (j ? jobs.end[j - 1] : 0);
        const int r = e / jobs.cols[j], c = e - r * jobs.cols[j];
        jobs.out[j][c * jobs.rows[j] + r] = jobs.in[j][e];
    }
}

// both reductions of a conv layer's backward in one launch of 1024-thread blocks: blocks [0, ns) sum the aggregate backward's slabs
// (dWe, dbe), every later block runs four 256-thread blocks of the weight-gradient reduction (dWj, dWi, dbj)
__global__ void __launch_bounds__(1024) k_reduce_layer(SlabReduceDesc sd, WgradReduceDesc wd, int ns) {
    __shared__ float red[RS_SLICES][17];
    __shared__ float redf[4][16][17];
    __shared__ double redd[4][16][17];
    if ((int)blockIdx.x < ns) {
        reduce_slabs_block(sd, blockIdx.x, red);
        return;
    }
    const int sub = threadIdx.x >> 8, t = threadIdx.x & 255;
    const int blk = ((int)blockIdx.x - ns) * 4 + sub;
    const bool on = blk < wgrad_reduce_blocks(wd);
    if (on) wgrad_reduce_cat_phase(wd, blk, t, redf[sub], redd[sub], 0);
    __syncthreads();
    if (on) wgrad_reduce_cat_phase(wd, blk, t, redf[sub], redd[sub], 1);
}

// DGNN_TRAIN_FUSED=0: the launch chain of the separate entry points (one launch per weight gradient, bias sum, transpose and
// input-gradient GEMM).  Default: dWj / dWi / dbj from one launch pair (dgnn_linear_wgrad_x3_cat), da and dz.Wi from one GEMM against
// the stacked [Wj^T ; Wi^T], the latter added where the aggregate backward stores dx (dgnn_sage_aggregate_bwd_add), all transposes of a
// backward pass in one launch.  Same arithmetic per element; only dbj is summed in another (fp64) order.
int g_fused_on = -1;   // bit 0: the backward chain, bit 1: batch statistics from the forward GEMM's epilogue
int fused_mask() {
    int v = __atomic_load_n(&g_fused_on, __ATOMIC_ACQUIRE);
    if (v < 0) {
        const char* e = getenv("DGNN_TRAIN_FUSED");
        v = e ? atoi(e) & 3 : 3;
        __atomic_store_n(&g_fused_on, v, __ATOMIC_RELEASE);
    }
    return v;
}
bool fused_enabled() { return (fused_mask() & 1) != 0; }
bool fused_stats_enabled() { return (fused_mask() & 2) != 0; }


void tr_add(TrJobs& jobs, const float* in, float* out, int rows, int cols) {
    const int j = jobs.n++;
    jobs.in[j] = in, jobs.out[j] = out, jobs.rows[j] = rows, jobs.cols[j] = cols;
    jobs.end[j] = (j ? jobs.end[j - 1] : 0) + rows * cols;
}
void transpose_many(const TrJobs& jobs, hipStream_t stream) {
    if (jobs.n) hipLaunchKernelGGL(k_transpose_many, dim3(dgnn_grid_cap(dgnn_cdiv(jobs.end[jobs.n - 1], 256))), dim3(256), 0, stream, jobs);
}
inline void transpose_to(const float* W, int rows, int cols, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(k_transpose, dim3(dgnn_grid_cap(dgnn_cdiv((int64_t)rows * cols, 256))), dim3(256), 0, stream, W, rows, cols, out);
}

template <typename T>
__global__ void k_add_inplace(T* __restrict__ a, const T* __restrict__ b, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dgnn_st(a + i, dgnn_ld(a + i) + dgnn_ld(b + i));
}

}  // namespace

#define TRY(call)                 \
    do {                          \
        const int rc_ = (call);   \
        if (rc_ != DGNN_OK) return rc_; \
    } while (0)

// library-internal (csrc/norm.hip): dgnn_bn_relu_bwd with the ReLU mask from x and the forward's (scale, shift)
int dgnn_bn_relu_bwd_zmask(const float* x, int64_t ldx, const float* y, int64_t ldy, const float* dy, int64_t lddy, const float* gamma, const float* mean,
                           const float* var, float eps, int train, int relu, int64_t M, int c, float* dx, int64_t lddx, float* dgamma, float* dbeta,
                           float* scratch, const float* zscale, const float* zshift, void* stream);
// library-internal (csrc/norm.hip): dgnn_bn_stats_finalize_fold that also counts the batch in *nbt
int dgnn_bn_stats_finalize_fold_nbt(const double* colstats, int64_t nblk, int64_t M, int c, float* mean, float* var, float* running_mean, float* running_var,
                                    float momentum, const float* gamma, const float* beta, float eps, float* scale, float* shift, int64_t* nbt, void* stream);
// csrc/aggregate.hip
extern "C" int dgnn_sage_aggregate_bwd_phi_add_masked(const int32_t* t_rowptr, const int32_t* t_dst, const int32_t* t_eid, int64_t n_src, const int32_t* rowptr_dst,
                                           const void* x_src, int64_t ldx, int c_in, const void* phi, int64_t ldphi, const void* da, int64_t ldda,
                                           void* dx_src, int64_t lddx, const void* add, int64_t ldadd, int64_t n_add, void* dphi_out, int64_t lddphi,
                                           const void* dphi_ext, int bf16, int mask_dx, void* stream);

namespace {

// =====================================================================================================================
// One training layer, described once (the idiom of fused_common.h): the extern "C" entry points fill a Layer, everything below them passes it.
// Rows of the storage type (fp32, or bf16 bit patterns) go through void*; the chains are written over the storage policies F32 / BF16.
// Static: lin_e (We, be) on edge_attr inside the aggregate, lin_j (Wj, bj), lin_i (Wi), BatchNorm.  Updated: lin_e on ea into phi, the model's
// lin_l / lin_r under the names Wj, bj / Wi, no BatchNorm.  A field a variant does not have stays zero.
// =====================================================================================================================
struct Plan {                                  // a block's graph; rowptr / t_rowptr NULL: a plain Linear block (no aggregate)
    const int32_t *rowptr, *src, *eid;         // destination-sorted: the forward
    const int32_t *t_rowptr, *t_dst, *t_eid;   // source-sorted: the backward, with the forward's rowptr as rowptr_dst
    const int32_t* rowptr_dst;
    int64_t n_src, n_dst, E;
};
struct Params {
    int c_in, c_out, f_e;                      // f_e: columns of the edge input that lin_e reads (0: no lin_e)
    const float *We, *be, *Wj, *bj, *Wi;
    const float *gamma, *beta;
    float *running_mean, *running_var;
    float momentum, eps;
    int relu;
    bool has_bn;                               // false in the backward: a plain Linear (the decoder's output layer), dz is dy itself
    int64_t* nbt;                              // the BatchNorm's num_batches_tracked, or NULL
};
struct Saved {                                 // the layer's input and what the forward leaves for the backward (which only reads them)
    const void* x;
    int64_t ldx;
    const void* edge;                          // Static: edge_attr (fp32 in both storage types); Updated: ea
    int64_t lde;
    void *a, *z, *y, *phi;
    float *mean, *var, *scale, *shift;         // the four rows of `stats`; scale NULL in the backward: the ReLU mask comes from y
};
struct Grads {
    const void *dy, *dphi_ext;
    void *dx, *d_ea;
    float *dWe, *dbe, *dWj, *dbj, *dWi, *dgamma, *dbeta;
    bool dy_is_dz;                             // Updated: dy already carries this layer's ReLU mask (the layer above stored its dx masked)
    bool want_mask;                            // Updated: store dx with the mask of the layer BELOW (dx * [x > 0]) -- done in the fused chain only ...
    bool* masked;                              // ... which says here whether it has
};
struct Work {
    float* fwd_scratch;                        // forward: column-statistics partials
    void *dz, *da, *dphi;                      // storage type; da holds [n_dst, 2 c_in] in the fused chains
    float *WjT, *WiT, *WeT;                    // transposes; fused chains: WiT == WjT + c_in * c_out (the stacked [Wj^T ; Wi^T])
    float *tmp, *tmp_w;                        // partial sums: the dx chain's | the weight gradients' (both alive until k_reduce_layer)
    bool pre_t;                                // the caller has transposed Wj / Wi already (one launch for the whole pass)
    bool* counted;                             // forward: whether this call has counted the batch in *nbt (the finalising launch of the statistics
                                               // does when they come out of the GEMM's epilogue; otherwise the caller still has to)
};
struct Layer {
    Plan g;
    Params p;
    Saved s;
    Grads d;
    Work w;
    int mode;                                  // DGNN_GEMM_*
    void* stream;
};
// a backward entry point's saved rows into Saved
inline void* unconst(const void* p) { return const_cast<void*>(p); }
inline float* unconst(const float* p) { return const_cast<float*>(p); }

// the two storage types behind one set of names
struct F32 {
    typedef float T;
    static constexpr int kBf16 = 0;
    static bool can_fuse(int mode) { return mode != DGNN_GEMM_F32; }
    static int linear(const T* A1, int64_t lda1, int k1, const float* W1, int64_t ldw1, const T* A2, int64_t lda2, int k2, const float* W2, int64_t ldw2,
                      const float* bias, int flags, int64_t M, int n, T* out, int64_t ldo, int mode, void* st) {
        return mode == DGNN_GEMM_F32 ? dgnn_linear_fwd(A1, lda1, k1, W1, ldw1, A2, lda2, k2, W2, ldw2, bias, nullptr, nullptr, flags, M, n, out, ldo, st)
                                     : dgnn_linear_fwd_x3(A1, lda1, k1, W1, ldw1, A2, lda2, k2, W2, ldw2, bias, nullptr, nullptr, flags, M, n, out, ldo, st);
    }
    static int wgrad(const T* A, int64_t lda, int na, const T* B, int64_t ldb, int nb, int64_t M, float* dW, float* tmp, int mode, void* st) {
        return mode == DGNN_GEMM_F32 ? dgnn_linear_wgrad(A, lda, na, B, ldb, nb, M, dW, nb, 0, tmp, st)
                                     : dgnn_linear_wgrad_x3(A, lda, na, B, ldb, nb, M, dW, nb, 0, tmp, st);
    }
    static int colsum(const T* x, int64_t ld, int64_t M, int c, float* out, float* tmp, void* st) { return dgnn_colsum(x, ld, M, c, out, 0, tmp, st); }
    static int wgrad_cat(const T* A, int64_t lda, int na, const T* B1, int64_t ldb1, int nb1, const T* B2, int64_t ldb2, int nb2, int64_t M, float* dW1,
                         float* dW2, float* dbias, float* tmp, void* st) {
        return dgnn_linear_wgrad_x3_cat(A, lda, na, B1, ldb1, nb1, B2, ldb2, nb2, M, dW1, dW2, dbias, tmp, st);
    }
    static int relu_bwd(const T* y, const T* g, int64_t n, T* out, void* st) { return dgnn_relu_bwd(y, g, n, out, st); }
    // the filter either from lin_e on edge_attr (Static) or stored in phi (Updated)
    static int agg_fwd(const Plan& g, const T* x, int64_t ldx, int c, const float* edge_attr, int64_t lde, int f_e, const float* We, const float* be, const T* phi,
                       T* a, void* st) {
        return dgnn_sage_aggregate_fwd(g.rowptr, g.src, g.eid, g.n_dst, x, ldx, c, edge_attr, lde, f_e, We, be, phi, phi ? c : 0, nullptr, 0, a, c, st);
    }
    static int agg_bwd(const Plan& g, const T* x, int64_t ldx, int c, const float* edge_attr, int64_t lde, int f_e, const float* We, const float* be, const T* phi,
                       const T* da, T* dx, float* dWe, float* dbe, T* dphi, float* tmp, void* st) {
        return dgnn_sage_aggregate_bwd(g.t_rowptr, g.t_dst, g.t_eid, g.n_src, g.rowptr_dst, x, ldx, c, edge_attr, lde, f_e, We, be, phi, phi ? c : 0, da, c, dx, c, dWe,
                                       dbe, dphi, dphi ? c : 0, tmp, st);
    }
    static int bn_relu_bwd(const T* z, const T* y, const T* dy, const float* gamma, const float* mean, const float* var, float eps, int relu, int64_t M, int c, T* dz,
                           float* dgamma, float* dbeta, float* tmp, void* st) {
        return dgnn_bn_relu_bwd(z, c, y, c, dy, c, gamma, mean, var, eps, 1, relu, M, c, dz, c, dgamma, dbeta, tmp, st);
    }
    // batch statistics (+ running statistics) and the folded (scale, shift): one call, the fold computed by the finalising kernel
    static int batch_stats_fold(const T* z, int64_t M, int c, const Params& p, const Saved& s, float* scratch, void* st) {
        return dgnn_bn_batch_stats_fold(z, c, M, c, s.mean, s.var, p.running_mean, p.running_var, p.momentum, p.gamma, p.beta, p.eps, s.scale, s.shift, scratch, st);
    }
    static int scale_shift_act(const T* z, const float* scale, const float* shift, int relu, int64_t M, int c, T* y, void* st) {
        return dgnn_scale_shift_act(z, c, scale, shift, relu, M, c, y, c, st);
    }
};
struct BF16 {
    typedef uint16_t T;
    static constexpr int kBf16 = 1;
    static bool can_fuse(int) { return true; }
    static int linear(const T* A1, int64_t lda1, int k1, const float* W1, int64_t ldw1, const T* A2, int64_t lda2, int k2, const float* W2, int64_t ldw2,
                      const float* bias, int flags, int64_t M, int n, T* out, int64_t ldo, int, void* st) {
        return dgnn_linear_fwd_bf16(A1, lda1, k1, W1, ldw1, A2, lda2, k2, W2, ldw2, bias, nullptr, nullptr, flags, M, n, out, ldo, 0, st);
    }
    static int wgrad(const T* A, int64_t lda, int na, const T* B, int64_t ldb, int nb, int64_t M, float* dW, float* tmp, int, void* st) {
        return dgnn_linear_wgrad_bf16(A, 0, lda, na, B, 0, ldb, nb, M, dW, nb, 0, tmp, st);
    }
    static int colsum(const T* x, int64_t ld, int64_t M, int c, float* out, float* tmp, void* st) { return dgnn_colsum_bf16(x, ld, M, c, out, 0, tmp, st); }
    static int wgrad_cat(const T* A, int64_t lda, int na, const T* B1, int64_t ldb1, int nb1, const T* B2, int64_t ldb2, int nb2, int64_t M, float* dW1,
                         float* dW2, float* dbias, float* tmp, void* st) {
        return dgnn_linear_wgrad_bf16_cat(A, 0, lda, na, B1, ldb1, nb1, B2, ldb2, nb2, 0, M, dW1, dW2, dbias, tmp, st);
    }
    static int relu_bwd(const T* y, const T* g, int64_t n, T* out, void* st) { return dgnn_relu_bwd_bf16(y, g, n, out, st); }
    static int agg_fwd(const Plan& g, const T* x, int64_t ldx, int c, const float* edge_attr, int64_t lde, int f_e, const float* We, const float* be, const T* phi,
                       T* a, void* st) {
        return dgnn_sage_aggregate_fwd_bf16(g.rowptr, g.src, g.eid, g.n_dst, x, ldx, c, edge_attr, lde, f_e, We, be, phi, phi ? c : 0, nullptr, 0, a, c, st);
    }
    static int agg_bwd(const Plan& g, const T* x, int64_t ldx, int c, const float* edge_attr, int64_t lde, int f_e, const float* We, const float* be, const T* phi,
                       const T* da, T* dx, float* dWe, float* dbe, T* dphi, float* tmp, void* st) {
        return dgnn_sage_aggregate_bwd_bf16(g.t_rowptr, g.t_dst, g.t_eid, g.n_src, g.rowptr_dst, x, ldx, c, edge_attr, lde, f_e, We, be, phi, phi ? c : 0, da, c, dx, c,
                                            dWe, dbe, dphi, dphi ? c : 0, tmp, st);
    }
    static int bn_relu_bwd(const T* z, const T* y, const T* dy, const float* gamma, const float* mean, const float* var, float eps, int relu, int64_t M, int c, T* dz,
                           float* dgamma, float* dbeta, float* tmp, void* st) {
        return dgnn_bn_relu_bwd_bf16(z, c, y, c, dy, c, gamma, mean, var, eps, 1, relu, M, c, dz, c, dgamma, dbeta, tmp, st);
    }
    // two launches where fp32 has one: the bf16 statistics kernel does not fold
    static int batch_stats_fold(const T* z, int64_t M, int c, const Params& p, const Saved& s, float* scratch, void* st) {
        TRY(dgnn_bn_batch_stats_bf16(z, c, M, c, s.mean, s.var, p.running_mean, p.running_var, p.momentum, scratch, st));
        return dgnn_bn_fold(p.gamma, p.beta, s.mean, s.var, p.eps, c, s.scale, s.shift, st);
    }
    static int scale_shift_act(const T* z, const float* scale, const float* shift, int relu, int64_t M, int c, T* y, void* st) {
        return dgnn_scale_shift_act_bf16(z, c, scale, shift, relu, M, c, y, c, st);
    }
};

// ---- Static layer ------------------------------------------------------------------------------------------------------
// scratch of dgnn_sage_layer_train_bwd: dz [n_dst, c_out] | da [n_dst, 2 c_in] | [Wj^T ; Wi^T] | partials of the dx chain (column reductions, aggregate
// backward slabs) | partials of the weight gradients (the fused chain keeps both alive until k_reduce_layer)
struct LayerScratch {
    int64_t dz = 0, da = 0, wt = 0, tmp = 0, tmp_w = 0, total = 0;
};
LayerScratch layer_scratch(int64_t n_src, int64_t n_dst, int c_in, int c_out, int f_e) {
    const int64_t stats = dgnn_colstats_scratch_elems(n_dst, c_out > c_in ? c_out : c_in);
    const int64_t wg = dgnn_linear_wgrad_scratch_elems(n_dst, c_out, c_in), wc = dgnn_linear_wgrad_cat_scratch_elems(n_dst, c_out, c_in, c_in);
    const int64_t ab = dgnn_sage_aggregate_bwd_scratch_elems(n_src, c_in, f_e > 0 ? f_e : 1);
    int64_t big = stats > wg ? stats : wg;
    if (ab > big) big = ab;
    LayerScratch r;
    r.da = align4(n_dst * c_out);
    r.wt = r.da + 2 * align4(n_dst * c_in);
    r.tmp = r.wt + 2 * align4((int64_t)c_in * c_out);
    r.tmp_w = r.tmp + align4(big);
    r.total = r.tmp_w + align4(big > wc ? big : wc) + 64;
    return r;
}

//   a = mean_j x_j * (We.A + be)   ->   z = a.Wj^T + x_dst.Wi^T + bj   ->   mean, var, scale, shift   ->   y = relu(z * scale + shift)
template <typename K>
int static_fwd(const Layer& L) {
    typedef typename K::T T;
    const auto& [g, p, s, d, w, mode, st] = L;
    if (w.counted) *w.counted = false;
    DGNN_REQUIRE(g.n_dst > 0 && p.c_in > 0 && p.c_out > 0, DGNN_E_INVALID, "sage_layer_train_fwd: bad sizes (BatchNorm needs at least one row)");
    DGNN_REQUIRE(s.x && p.Wj && s.z && s.mean && s.var && s.scale && s.shift && s.y && w.fwd_scratch, DGNN_E_INVALID, "sage_layer_train_fwd: null pointer");
    const T* x = (const T*)s.x;
    T *a = (T*)s.a, *z = (T*)s.z, *y = (T*)s.y;
    const T* A1 = x;
    int64_t lda1 = s.ldx;
    if (g.rowptr) {
        DGNN_REQUIRE(a && g.src, DGNN_E_INVALID, "sage_layer_train_fwd: the aggregate needs src and a");
        TRY(K::agg_fwd(g, x, s.ldx, p.c_in, (const float*)s.edge, s.lde, p.f_e, p.We, p.be, nullptr, a, st));
        A1 = a;
        lda1 = p.c_in;
    }
    const T* A2 = (g.rowptr && p.Wi) ? x : nullptr;   // x_dst = x[:n_dst] (reference :217)
    const int k2 = A2 ? p.c_in : 0;
    const float* W2 = A2 ? p.Wi : nullptr;
    if (!K::kBf16 && mode != DGNN_GEMM_F32 && fused_stats_enabled()) {
        // fp32 storage only: the GEMM's epilogue leaves the column sums of z per block of 32 rows -- no launch that reads z back for the batch statistics
        double* cs = reinterpret_cast<double*>(((uintptr_t)w.fwd_scratch + 7) & ~(uintptr_t)7);
        const int rc = dgnn_linear_fwd_x3_stats((const float*)A1, lda1, p.c_in, p.Wj, p.c_in, (const float*)A2, s.ldx, k2, W2, p.c_in, p.bj, g.n_dst, p.c_out, (float*)z,
                                                p.c_out, cs, st);
        if (rc == DGNN_OK) {
            TRY(dgnn_bn_stats_finalize_fold_nbt(cs, (g.n_dst + 31) / 32, g.n_dst, p.c_out, s.mean, s.var, p.running_mean, p.running_var, p.momentum, p.gamma, p.beta,
                                                p.eps, s.scale, s.shift, p.nbt, st));
            if (w.counted) *w.counted = p.nbt != nullptr;
            return K::scale_shift_act(z, s.scale, s.shift, p.relu, g.n_dst, p.c_out, y, st);
        }
        if (rc != DGNN_E_UNSUPPORTED) return rc;
    }
    TRY(K::linear(A1, lda1, p.c_in, p.Wj, p.c_in, A2, s.ldx, k2, W2, p.c_in, p.bj, 0, g.n_dst, p.c_out, z, p.c_out, mode, st));
    TRY(K::batch_stats_fold(z, g.n_dst, p.c_out, p, s, w.fwd_scratch, st));
    return K::scale_shift_act(z, s.scale, s.shift, p.relu, g.n_dst, p.c_out, y, st);
}

// DGNN_BN_ZMASK=0: the ReLU mask of the BatchNorm backward from y even where the forward's (scale, shift) are at hand
bool zmask_enabled() {
    static const bool on = !(getenv("DGNN_BN_ZMASK") && getenv("DGNN_BN_ZMASK")[0] == '0');
    return on;
}

//   dz, dgamma, dbeta -> dWj, dbj, dWi -> transposes -> da = dz.Wj -> (dx, dWe, dbe) = aggregate backward -> dx[:n_dst] += dz.Wi
// in the order of the separate entry points.  fp32 storage with x3 products and fused_enabled(): the fused chain (see g_fused_on).
template <typename K>
int static_bwd(const Layer& L) {
    typedef typename K::T T;
    const auto& [g, p, s, d, w, mode, st] = L;
    hipStream_t stream = (hipStream_t)st;
    const int c_in = p.c_in, c_out = p.c_out;
    const int64_t n_dst = g.n_dst;
    const T *x = (const T*)s.x, *a = (const T*)s.a, *z = (const T*)s.z, *y = (const T*)s.y, *dy = (const T*)d.dy;
    T *dx = (T*)d.dx, *da = (T*)w.da;
    const bool agg = g.t_rowptr != nullptr;
    const bool fused = !K::kBf16 && mode != DGNN_GEMM_F32 && fused_enabled();
    // BatchNorm (batch statistics) + ReLU backward.  fp32 storage, the forward's (scale, shift) handed on: the ReLU mask from z, y is not read
    if (p.has_bn) {
        if (!K::kBf16 && zmask_enabled() && s.scale && p.relu)
            TRY(dgnn_bn_relu_bwd_zmask((const float*)z, c_out, (const float*)y, c_out, (const float*)dy, c_out, p.gamma, s.mean, s.var, p.eps, 1, p.relu, n_dst, c_out,
                                       (float*)w.dz, c_out, d.dgamma, d.dbeta, w.tmp, s.scale, s.shift, st));
        else
            TRY(K::bn_relu_bwd(z, y, dy, p.gamma, s.mean, s.var, p.eps, p.relu, n_dst, c_out, (T*)w.dz, d.dgamma, d.dbeta, w.tmp, st));
    }
    const T* const dz = p.has_bn ? (const T*)w.dz : dy;
    const T* A1 = agg ? a : x;
    const int64_t lda1 = agg ? c_in : s.ldx;
    const bool need_dx = dx != nullptr;
    const bool need_da = agg ? (need_dx || p.We != nullptr) : need_dx;
    const bool both = need_da && agg && need_dx && p.Wi;
    const bool one_gemm = fused && both && p.We && p.f_e == 20;   // [da | dz.Wi] from one GEMM, the layer's two reductions from one launch
    WgradReduceDesc wdesc;
    if (fused) {
        const float* B2 = (agg && p.Wi && d.dWi) ? (const float*)x : nullptr;
        TRY(dgnn_linear_wgrad_x3_cat_deferred((const float*)dz, c_out, c_out, (const float*)A1, lda1, c_in, B2, s.ldx, B2 ? c_in : 0, n_dst, d.dWj, d.dWi, d.dbj, w.tmp_w,
                                              st, one_gemm ? &wdesc : nullptr));
    } else {
        TRY(K::wgrad(dz, c_out, c_out, A1, lda1, c_in, n_dst, d.dWj, w.tmp_w, mode, st));
        if (d.dbj) TRY(K::colsum(dz, c_out, n_dst, c_out, d.dbj, w.tmp_w, st));
        if (agg && p.Wi && d.dWi) TRY(K::wgrad(dz, c_out, c_out, x, s.ldx, c_in, n_dst, d.dWi, w.tmp_w, mode, st));
    }
    if (both && !w.pre_t)
        hipLaunchKernelGGL(k_transpose2, dim3(dgnn_grid_cap(dgnn_cdiv((int64_t)2 * c_in * c_out, 256))), dim3(256), 0, stream, p.Wj, p.Wi, c_out, c_in, w.WjT, w.WiT);
    if (one_gemm) {
        // [da | dz.Wi] = dz . [Wj^T ; Wi^T]^T in one GEMM (every output column is the separate GEMMs' own dot product), the second half added to
        // the aggregate's sums where dx is stored
        DGNN_REQUIRE(d.dWe && d.dbe, DGNN_E_INVALID, "sage_layer_train_bwd: dWe / dbe missing");
        TRY(K::linear(dz, c_out, c_out, w.WjT, c_out, nullptr, 0, 0, nullptr, 0, nullptr, 0, n_dst, 2 * c_in, da, 2 * c_in, mode, st));
        SlabReduceDesc sdesc;
        TRY(dgnn_sage_aggregate_bwd_add_deferred(g.t_rowptr, g.t_dst, g.t_eid, g.n_src, g.rowptr_dst, (const float*)x, s.ldx, c_in, (const float*)s.edge, s.lde, p.f_e,
                                                 p.We, p.be, (const float*)da, 2 * c_in, (float*)dx, c_in, (const float*)da + c_in, 2 * c_in, n_dst, d.dWe, d.dbe, w.tmp,
                                                 st, &sdesc));
        const int ns = slab_reduce_blocks(sdesc), nw = (wgrad_reduce_blocks(wdesc) + 3) / 4;
        hipLaunchKernelGGL(k_reduce_layer, dim3((unsigned)(ns + nw)), dim3(1024), 0, stream, sdesc, wdesc, ns);
        return dgnn_check_launch("sage_layer_train_bwd");
    }
    if (need_da) {
        DGNN_REQUIRE(!agg || da, DGNN_E_INVALID, "sage_layer_train_bwd: da buffer missing");
        if (!both && !w.pre_t) transpose_to(p.Wj, c_out, c_in, w.WjT, stream);
        // plain Linear block: the gradient of the input is da itself
        TRY(K::linear(dz, c_out, c_out, w.WjT, c_out, nullptr, 0, 0, nullptr, 0, nullptr, 0, n_dst, c_in, agg ? da : dx, c_in, mode, st));
    }
    if (agg) {
        if (p.We) DGNN_REQUIRE(d.dWe && d.dbe, DGNN_E_INVALID, "sage_layer_train_bwd: dWe / dbe missing");
        if (need_da)   // dWe / dbe are written (not accumulated) by the slab reduction: no fill
            TRY(K::agg_bwd(g, x, s.ldx, c_in, (const float*)s.edge, s.lde, p.f_e, p.We, p.be, nullptr, da, dx, d.dWe, d.dbe, nullptr, w.tmp, st));
        if (need_dx && p.Wi) {
            if (!both && !w.pre_t) transpose_to(p.Wi, c_out, c_in, w.WiT, stream);
            TRY(K::linear(dz, c_out, c_out, w.WiT, c_out, nullptr, 0, 0, nullptr, 0, nullptr, DGNN_LINEAR_ACCUMULATE, n_dst, c_in, dx, c_in, mode, st));
        }
    }
    return dgnn_check_launch("sage_layer_train_bwd");
}

}  // namespace

extern "C" int64_t dgnn_sage_layer_train_scratch_elems(int64_t n_src, int64_t n_dst, int c_in, int c_out, int f_e) {
    if (n_src < 0 || n_dst < 0 || c_in <= 0 || c_out <= 0) return 16;
    return layer_scratch(n_src, n_dst, c_in, c_out, f_e).total;
}

extern "C" int dgnn_sage_layer_train_fwd(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int64_t n_dst, const float* x,
                                         int64_t ldx, int c_in, const float* edge_attr, int64_t lde, int f_e, const float* We,
                                         const float* be, const float* Wj, const float* bj, const float* Wi, int c_out, const float* gamma,
                                         const float* beta, float* running_mean, float* running_var, float momentum, float eps, int relu,
                                         float* a, float* z, float* mean, float* var, float* scale, float* shift, float* y, float* scratch,
                                         int gemm_mode, void* stream) {
    Layer L = {};
    L.mode = gemm_mode, L.stream = stream;
    L.g.rowptr = rowptr, L.g.src = src, L.g.eid = eid, L.g.n_dst = n_dst;
    L.s.x = x, L.s.ldx = ldx, L.s.edge = edge_attr, L.s.lde = lde;
    L.p.c_in = c_in, L.p.c_out = c_out, L.p.f_e = f_e, L.p.We = We, L.p.be = be, L.p.Wj = Wj, L.p.bj = bj, L.p.Wi = Wi, L.p.relu = relu;
    L.p.has_bn = true, L.p.gamma = gamma, L.p.beta = beta, L.p.running_mean = running_mean, L.p.running_var = running_var, L.p.momentum = momentum, L.p.eps = eps;
    L.s.a = unconst(a), L.s.z = unconst(z), L.s.y = unconst(y);
    L.s.mean = unconst(mean), L.s.var = unconst(var), L.s.scale = unconst(scale), L.s.shift = unconst(shift);
    L.w.fwd_scratch = scratch;
    return static_fwd<F32>(L);
}

extern "C" int dgnn_sage_layer_train_bwd(const int32_t* t_rowptr, const int32_t* t_dst, const int32_t* t_eid, const int32_t* rowptr_dst,
                                         int64_t n_src, int64_t n_dst, const float* x, int64_t ldx, int c_in, const float* edge_attr,
                                         int64_t lde, int f_e, const float* We, const float* be, const float* Wj, const float* Wi, int c_out,
                                         const float* gamma, const float* mean, const float* var, float eps, int relu, const float* a,
                                         const float* z, const float* y, const float* dy, float* dx, float* dWe, float* dbe, float* dWj,
                                         float* dbj, float* dWi, float* dgamma, float* dbeta, float* scratch, int gemm_mode, void* stream) {
    DGNN_REQUIRE(n_dst > 0 && n_src >= n_dst && c_in > 0 && c_out > 0, DGNN_E_INVALID, "sage_layer_train_bwd: bad sizes");
    DGNN_REQUIRE(x && Wj && z && y && dy && mean && var && dWj && dgamma && dbeta && scratch, DGNN_E_INVALID, "sage_layer_train_bwd: null pointer");
    Layer L = {};
    L.mode = gemm_mode, L.stream = stream;
    L.g.t_rowptr = t_rowptr, L.g.t_dst = t_dst, L.g.t_eid = t_eid, L.g.rowptr_dst = rowptr_dst, L.g.n_src = n_src, L.g.n_dst = n_dst;
    L.s.x = x, L.s.ldx = ldx, L.s.edge = edge_attr, L.s.lde = lde;
    L.p.c_in = c_in, L.p.c_out = c_out, L.p.f_e = f_e, L.p.We = We, L.p.be = be, L.p.Wj = Wj, L.p.Wi = Wi, L.p.relu = relu;
    L.p.has_bn = true, L.p.gamma = gamma, L.p.eps = eps;
    L.s.a = unconst(a), L.s.z = unconst(z), L.s.y = unconst(y);
    L.s.mean = unconst(mean), L.s.var = unconst(var);
    L.d.dy = dy, L.d.dx = dx, L.d.dWe = dWe, L.d.dbe = dbe, L.d.dWj = dWj, L.d.dbj = dbj, L.d.dWi = dWi, L.d.dgamma = dgamma, L.d.dbeta = dbeta;
    const LayerScratch lay = layer_scratch(n_src, n_dst, c_in, c_out, f_e);
    L.w.dz = scratch + lay.dz, L.w.da = scratch + lay.da;
    L.w.WjT = scratch + lay.wt, L.w.WiT = L.w.WjT + (int64_t)c_in * c_out;   // stacked: [Wj^T ; Wi^T] is one [2 c_in, c_out] matrix
    L.w.tmp = scratch + lay.tmp, L.w.tmp_w = scratch + lay.tmp_w;
    return static_bwd<F32>(L);
}

// Static conv layer in training mode with bf16 STORAGE (activations bf16, parameters / statistics / gradients of parameters fp32): the same chains over
// the *_bf16 entry points.  Scratch sizes as for the fp32 functions.
extern "C" int dgnn_sage_layer_train_fwd_bf16(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int64_t n_dst, const uint16_t* x,
                                              int64_t ldx, int c_in, const float* edge_attr, int64_t lde, int f_e, const float* We,
                                              const float* be, const float* Wj, const float* bj, const float* Wi, int c_out,
                                              const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum,
                                              float eps, int relu, uint16_t* a, uint16_t* z, float* mean, float* var, float* scale, float* shift,
                                              uint16_t* y, float* scratch, void* stream) {
    Layer L = {};
    L.stream = stream;   // (mode stays 0: the arithmetic switch does not reach the bf16 kernels)
    L.g.rowptr = rowptr, L.g.src = src, L.g.eid = eid, L.g.n_dst = n_dst;
    L.s.x = x, L.s.ldx = ldx, L.s.edge = edge_attr, L.s.lde = lde;
    L.p.c_in = c_in, L.p.c_out = c_out, L.p.f_e = f_e, L.p.We = We, L.p.be = be, L.p.Wj = Wj, L.p.bj = bj, L.p.Wi = Wi, L.p.relu = relu;
    L.p.has_bn = true, L.p.gamma = gamma, L.p.beta = beta, L.p.running_mean = running_mean, L.p.running_var = running_var, L.p.momentum = momentum, L.p.eps = eps;
    L.s.a = unconst(a), L.s.z = unconst(z), L.s.y = unconst(y);
    L.s.mean = unconst(mean), L.s.var = unconst(var), L.s.scale = unconst(scale), L.s.shift = unconst(shift);
    L.w.fwd_scratch = scratch;
    return static_fwd<BF16>(L);
}

// dz / da: work buffers [n_dst, c_out] / [n_dst, c_in] of bf16; scratch (floats): dgnn_sage_layer_train_scratch_elems, of which this chain uses
// Wj^T | Wi^T | one region of partials (no fused chain in bf16 storage: nothing keeps two sets of partials alive)
extern "C" int dgnn_sage_layer_train_bwd_bf16(const int32_t* t_rowptr, const int32_t* t_dst, const int32_t* t_eid, const int32_t* rowptr_dst,
                                              int64_t n_src, int64_t n_dst, const uint16_t* x, int64_t ldx, int c_in, const float* edge_attr,
                                              int64_t lde, int f_e, const float* We, const float* be, const float* Wj, const float* Wi, int c_out,
                                              const float* gamma, const float* mean, const float* var, float eps, int relu, const uint16_t* a,
                                              const uint16_t* z, const uint16_t* y, const uint16_t* dy, uint16_t* dx, float* dWe, float* dbe,
                                              float* dWj, float* dbj, float* dWi, float* dgamma, float* dbeta, uint16_t* dz, uint16_t* da,
                                              float* scratch, void* stream) {
    DGNN_REQUIRE(n_dst > 0 && n_src >= n_dst && c_in > 0 && c_out > 0, DGNN_E_INVALID, "sage_layer_train_bwd_bf16: bad sizes");
    DGNN_REQUIRE(x && Wj && z && y && dy && mean && var && dWj && dgamma && dbeta && dz && scratch, DGNN_E_INVALID, "sage_layer_train_bwd_bf16: null pointer");
    Layer L = {};
    L.stream = stream;
    L.g.t_rowptr = t_rowptr, L.g.t_dst = t_dst, L.g.t_eid = t_eid, L.g.rowptr_dst = rowptr_dst, L.g.n_src = n_src, L.g.n_dst = n_dst;
    L.s.x = x, L.s.ldx = ldx, L.s.edge = edge_attr, L.s.lde = lde;
    L.p.c_in = c_in, L.p.c_out = c_out, L.p.f_e = f_e, L.p.We = We, L.p.be = be, L.p.Wj = Wj, L.p.Wi = Wi, L.p.relu = relu;
    L.p.has_bn = true, L.p.gamma = gamma, L.p.eps = eps;
    L.s.a = unconst(a), L.s.z = unconst(z), L.s.y = unconst(y);
    L.s.mean = unconst(mean), L.s.var = unconst(var);
    L.d.dy = dy, L.d.dx = dx, L.d.dWe = dWe, L.d.dbe = dbe, L.d.dWj = dWj, L.d.dbj = dbj, L.d.dWi = dWi, L.d.dgamma = dgamma, L.d.dbeta = dbeta;
    L.w.dz = dz, L.w.da = da;
    L.w.WjT = scratch, L.w.WiT = L.w.WjT + align4((int64_t)c_in * c_out);
    L.w.tmp = L.w.tmp_w = L.w.WiT + align4((int64_t)c_in * c_out);
    return static_bwd<BF16>(L);
}

// =====================================================================================================================
// Updated variant (surfaceNetUpdatedEdgeFilters.py:147-170 and its autograd): one conv layer per call each way, fp32 or bf16
// storage (activations / phi bf16, parameters and their gradients fp32).
//   forward : phi = ea.We^T + be  [E, c_in]   ->   a = mean_j x_j * phi   ->   y = relu?(a.Wl^T + x[:n_dst].Wr^T + bl)
//   backward: dz = dy * [y > 0]; dWl, dbl, dWr; da = dz.Wl; (dx, dphi) = aggregate backward; dx[:n_dst] += dz.Wr;
//             dphi += dphi_ext (the next layer's use of phi as its edge input); dWe = dphi^T ea, dbe, d_ea = dphi.We
// The same kernels in the same order as the separate entry points (bit-identical results).
// =====================================================================================================================
namespace {

// scratch of dgnn_sage_updated_train_bwd: Wl^T | Wr^T | We^T | partial sums (weight gradients and bias sums are the only kernels here that use them)
struct UpdatedScratch {
    int64_t WlT = 0, WrT = 0, WeT = 0, tmp = 0, total = 0;
};
UpdatedScratch updated_scratch(int64_t n_dst, int64_t E, int c_in, int c_out, int k_e) {
    int64_t big = dgnn_colstats_scratch_elems(n_dst > E ? n_dst : E, c_in > c_out ? c_in : c_out);
    const int64_t w1 = dgnn_linear_wgrad_cat_scratch_elems(n_dst, c_out, c_in, c_in), w2 = dgnn_linear_wgrad_cat_scratch_elems(E, c_in, k_e, 0);
    if (w1 > big) big = w1;
    if (w2 > big) big = w2;
    UpdatedScratch r;
    r.WrT = align4((int64_t)c_in * c_out);
    r.WeT = r.WrT + align4((int64_t)c_in * c_out);
    r.tmp = r.WeT + align4((int64_t)c_in * k_e);
    r.total = r.tmp + align4(big) + 64;
    return r;
}

template <typename K>
int updated_fwd(const Layer& L) {
    typedef typename K::T T;
    const auto& [g, p, s, d, w, mode, st] = L;
    const T *x = (const T*)s.x, *ea = (const T*)s.edge;
    T *phi = (T*)s.phi, *a = (T*)s.a, *y = (T*)s.y;
    if (g.E > 0) TRY(K::linear(ea, s.lde, p.f_e, p.We, p.f_e, nullptr, 0, 0, nullptr, 0, p.be, 0, g.E, p.c_in, phi, p.c_in, mode, st));   // :156
    TRY(K::agg_fwd(g, x, s.ldx, p.c_in, nullptr, 0, 0, nullptr, nullptr, phi, a, st));                                                      // :158
    return K::linear(a, p.c_in, p.c_in, p.Wj, p.c_in, p.Wi ? x : nullptr, s.ldx, p.Wi ? p.c_in : 0, p.Wi, p.c_in, p.bj, p.relu ? 1 : 0, g.n_dst, p.c_out, y, p.c_out,
                     mode, st);                                                                                                           // :159-165
}

template <typename K>
int updated_bwd(const Layer& L) {
    typedef typename K::T T;
    const auto& [g, p, s, d, w, mode, st] = L;
    hipStream_t stream = (hipStream_t)st;
    const int c_in = p.c_in, c_out = p.c_out, k_e = p.f_e;
    const int64_t n_dst = g.n_dst, E = g.E;
    if (d.masked) *d.masked = false;
    const T *x = (const T*)s.x, *ea = (const T*)s.edge, *phi = (const T*)s.phi, *a = (const T*)s.a, *y = (const T*)s.y, *dy = (const T*)d.dy,
            *dphi_ext = (const T*)d.dphi_ext;
    T *dx = (T*)d.dx, *d_ea = (T*)d.d_ea, *dz = (T*)w.dz, *da = (T*)w.da, *dphi = (T*)w.dphi;
    const T* gr = dy;
    if (p.relu && !d.dy_is_dz) {
        TRY(K::relu_bwd(y, dy, n_dst * c_out, dz, st));
        gr = dz;
    }
    const bool fused = fused_enabled() && K::can_fuse(mode);
    const int mask_dx = (fused && d.want_mask && dx) ? 1 : 0;
    if (d.masked) *d.masked = mask_dx != 0;
    const bool both = dx && p.Wi;
    const T* B2 = (p.Wi && d.dWi) ? x : nullptr;
    if (fused) {
        // The launch chain of the Static layer's fused backward for this variant: dWl / dWr / dbl from one launch pair, the three transposes from one
        // launch, [da | dz.Wr] from one GEMM against the stacked [Wl^T ; Wr^T] with the second half added where the aggregate backward stores dx,
        // dWe / dbe from one launch pair.  `da` holds [n_dst, 2 c_in]; Wr^T sits right under Wl^T (its own region begins at or after that).
        TrJobs jobs;
        jobs.n = 0;
        tr_add(jobs, p.Wj, w.WjT, c_out, c_in);
        if (both) tr_add(jobs, p.Wi, w.WjT + (int64_t)c_in * c_out, c_out, c_in);
        if (E > 0 && d_ea) tr_add(jobs, p.We, w.WeT, c_in, k_e);
        transpose_many(jobs, stream);
        TRY(K::wgrad_cat(gr, c_out, c_out, a, c_in, c_in, B2, s.ldx, B2 ? c_in : 0, n_dst, d.dWj, d.dWi, d.dbj, w.tmp, st));
        const int ldda = both ? 2 * c_in : c_in;
        TRY(K::linear(gr, c_out, c_out, w.WjT, c_out, nullptr, 0, 0, nullptr, 0, nullptr, 0, n_dst, ldda, da, ldda, mode, st));
        TRY(dgnn_sage_aggregate_bwd_phi_add_masked(g.t_rowptr, g.t_dst, g.t_eid, g.n_src, g.rowptr_dst, x, s.ldx, c_in, phi, c_in, da, ldda, dx, c_in,
                                                   both ? da + c_in : nullptr, both ? ldda : 0, both ? n_dst : 0, dphi, c_in, nullptr, K::kBf16, mask_dx, st));
    } else {
        TRY(K::wgrad(gr, c_out, c_out, a, c_in, c_in, n_dst, d.dWj, w.tmp, mode, st));
        if (d.dbj) TRY(K::colsum(gr, c_out, n_dst, c_out, d.dbj, w.tmp, st));
        if (B2) TRY(K::wgrad(gr, c_out, c_out, x, s.ldx, c_in, n_dst, d.dWi, w.tmp, mode, st));
        transpose_to(p.Wj, c_out, c_in, w.WjT, stream);
        TRY(K::linear(gr, c_out, c_out, w.WjT, c_out, nullptr, 0, 0, nullptr, 0, nullptr, 0, n_dst, c_in, da, c_in, mode, st));
        TRY(K::agg_bwd(g, x, s.ldx, c_in, nullptr, 0, 0, nullptr, nullptr, phi, da, dx, nullptr, nullptr, dphi, nullptr, st));
        if (both) {
            transpose_to(p.Wi, c_out, c_in, w.WiT, stream);
            TRY(K::linear(gr, c_out, c_out, w.WiT, c_out, nullptr, 0, 0, nullptr, 0, nullptr, DGNN_LINEAR_ACCUMULATE, n_dst, c_in, dx, c_in, mode, st));
        }
    }
    if (E == 0) {
        (void)hipMemsetAsync(d.dWe, 0, sizeof(float) * (size_t)c_in * k_e, stream);
        (void)hipMemsetAsync(d.dbe, 0, sizeof(float) * (size_t)c_in, stream);
        return dgnn_check_launch("sage_updated_train_bwd");
    }
    // (dphi += dphi_ext stays a launch of its own: folded into the aggregate backward's dphi store -- dgnn_sage_aggregate_bwd_phi_add can do
    // it -- the fourth row load per edge cost the kernel 60 % (72 -> 115 us on the outermost block) against the 7-9 us of k_add_inplace)
    if (dphi_ext) hipLaunchKernelGGL((k_add_inplace<T>), dim3(dgnn_grid_cap(dgnn_cdiv(E * c_in, 256))), dim3(256), 0, stream, dphi, dphi_ext, E * c_in);
    if (fused) {
        TRY(K::wgrad_cat(dphi, c_in, c_in, ea, s.lde, k_e, nullptr, 0, 0, E, d.dWe, nullptr, d.dbe, w.tmp, st));
    } else {
        TRY(K::wgrad(dphi, c_in, c_in, ea, s.lde, k_e, E, d.dWe, w.tmp, mode, st));
        TRY(K::colsum(dphi, c_in, E, c_in, d.dbe, w.tmp, st));
        if (d_ea) transpose_to(p.We, c_in, k_e, w.WeT, stream);
    }
    if (d_ea) TRY(K::linear(dphi, c_in, c_in, w.WeT, c_in, nullptr, 0, 0, nullptr, 0, nullptr, 0, E, k_e, d_ea, k_e, mode, st));
    return dgnn_check_launch("sage_updated_train_bwd");
}

void set_updated_work(Layer& L, void* dz, void* da, void* dphi, float* scratch) {
    const UpdatedScratch lay = updated_scratch(L.g.n_dst, L.g.E, L.p.c_in, L.p.c_out, L.p.f_e);
    L.w.dz = dz, L.w.da = da, L.w.dphi = dphi;
    L.w.WjT = scratch + lay.WlT, L.w.WiT = scratch + lay.WrT, L.w.WeT = scratch + lay.WeT, L.w.tmp = scratch + lay.tmp;
}

}  // namespace

extern "C" int64_t dgnn_sage_updated_train_scratch_elems(int64_t n_dst, int64_t E, int c_in, int c_out, int k_e) {
    if (n_dst < 0 || E < 0 || c_in <= 0 || c_out <= 0 || k_e <= 0) return 16;
    return updated_scratch(n_dst, E, c_in, c_out, k_e).total;
}

extern "C" int dgnn_sage_updated_train_fwd(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int64_t n_dst, const void* x, int64_t ldx,
                                           int c_in, const void* ea, int64_t lde, int k_e, int64_t E, const float* We, const float* be,
                                           const float* Wl, const float* bl, const float* Wr, int c_out, int relu, void* phi, void* a, void* y,
                                           int bf16, int gemm_mode, void* stream) {
    DGNN_REQUIRE(n_dst > 0 && E >= 0 && c_in > 0 && c_out > 0 && k_e > 0, DGNN_E_INVALID, "sage_updated_train_fwd: bad sizes");
    DGNN_REQUIRE(rowptr && src && x && We && be && Wl && phi && a && y && (E == 0 || ea), DGNN_E_INVALID, "sage_updated_train_fwd: null pointer");
    Layer L = {};
    L.mode = gemm_mode, L.stream = stream;
    L.g.rowptr = rowptr, L.g.src = src, L.g.eid = eid, L.g.n_dst = n_dst, L.g.E = E;
    L.s.x = x, L.s.ldx = ldx, L.s.edge = ea, L.s.lde = lde;
    L.p.c_in = c_in, L.p.c_out = c_out, L.p.f_e = k_e, L.p.We = We, L.p.be = be, L.p.Wj = Wl, L.p.bj = bl, L.p.Wi = Wr, L.p.relu = relu;
    L.s.a = unconst(a), L.s.y = unconst(y), L.s.phi = unconst(phi);
    return bf16 ? updated_fwd<BF16>(L) : updated_fwd<F32>(L);
}

extern "C" int dgnn_sage_updated_train_bwd(const int32_t* t_rowptr, const int32_t* t_dst, const int32_t* t_eid, const int32_t* rowptr_dst,
                                           int64_t n_src, int64_t n_dst, int64_t E, const void* x, int64_t ldx, int c_in, const void* ea, int64_t lde,
                                           int k_e, const float* We, const float* Wl, const float* Wr, int c_out, int relu, const void* phi,
                                           const void* a, const void* y, const void* dy, const void* dphi_ext, void* dx, void* d_ea, float* dWe,
                                           float* dbe, float* dWl, float* dbl, float* dWr, void* dz, void* da, void* dphi, float* scratch, int bf16,
                                           int gemm_mode, void* stream) {
    DGNN_REQUIRE(n_dst > 0 && n_src >= n_dst && E >= 0 && c_in > 0 && c_out > 0 && k_e > 0, DGNN_E_INVALID, "sage_updated_train_bwd: bad sizes");
    DGNN_REQUIRE(t_rowptr && t_dst && t_eid && rowptr_dst && x && We && Wl && phi && a && dy && dWe && dbe && dWl && da && dphi && scratch &&
                     (!relu || (y && dz)) && (E == 0 || ea),
                 DGNN_E_INVALID, "sage_updated_train_bwd: null pointer");
    Layer L = {};
    L.mode = gemm_mode, L.stream = stream;
    L.g.t_rowptr = t_rowptr, L.g.t_dst = t_dst, L.g.t_eid = t_eid, L.g.rowptr_dst = rowptr_dst, L.g.n_src = n_src, L.g.n_dst = n_dst, L.g.E = E;
    L.s.x = x, L.s.ldx = ldx, L.s.edge = ea, L.s.lde = lde;
    L.p.c_in = c_in, L.p.c_out = c_out, L.p.f_e = k_e, L.p.We = We, L.p.Wj = Wl, L.p.Wi = Wr, L.p.relu = relu;
    L.s.a = unconst(a), L.s.y = unconst(y), L.s.phi = unconst(phi);
    L.d.dy = dy, L.d.dphi_ext = dphi_ext, L.d.dx = dx, L.d.d_ea = d_ea, L.d.dWe = dWe, L.d.dbe = dbe, L.d.dWj = dWl, L.d.dbj = dbl, L.d.dWi = dWr;
    set_updated_work(L, dz, da, dphi, scratch);
    return bf16 ? updated_bwd<BF16>(L) : updated_bwd<F32>(L);
}

// =====================================================================================================================
// Static model, training mode, ALL layers per call: the chain of dgnn_sage_layer_train_fwd / _bwd calls (conv layers, then the
// decoder's Linear + BatchNorm + ReLU block as a layer with rowptr[l] == NULL) issued from one entry point each way.  Layer l
// reads the previous layer's y (layer 0: x0); the blocks nest (the destinations of layer l are the sources of layer l+1), so
// layer l's output gradient IS layer l+1's dx.  Per-layer arrays are HOST arrays of device pointers / sizes.
// =====================================================================================================================
namespace {
struct Ptr8 {
    int64_t* p[8];
};
__global__ void k_inc_i64(Ptr8 ps, int n) {
    if (threadIdx.x < n && ps.p[threadIdx.x]) *ps.p[threadIdx.x] += 1;
}
}  // namespace

extern "C" int dgnn_static_train_fwd(int n_layers, const int32_t* const* rowptr, const int32_t* const* src, const int32_t* const* eid,
                                     const int64_t* n_dst, const float* x0, int64_t ldx0, const int32_t* widths, const float* const* edge_attr,
                                     const int64_t* lde, int f_e, const float* const* We, const float* const* be, const float* const* Wj,
                                     const float* const* bj, const float* const* Wi, const float* const* gamma, const float* const* beta,
                                     float* const* running_mean, float* const* running_var, int64_t* const* num_batches_tracked,
                                     const float* momentum, const float* eps, float* const* a, float* const* z, float* const* stats,
                                     float* const* y, float* scratch, int gemm_mode, void* stream) {
    DGNN_REQUIRE(n_layers >= 1 && n_layers <= 8 && rowptr && src && eid && n_dst && x0 && widths && edge_attr && lde && We && be && Wj && bj && Wi && gamma &&
                     beta && running_mean && running_var && momentum && eps && a && z && stats && y && scratch,
                 DGNN_E_INVALID, "static_train_fwd: bad args (at most 8 layers)");
    const float* x = x0;
    int64_t ldx = ldx0;
    unsigned counted_mask = 0;
    for (int l = 0; l < n_layers; ++l) {
        const int c_in = widths[l], c_out = widths[l + 1];
        float* st = stats[l];
        if (!st) {   // a plain Linear (the decoder's output layer, :187): y = x . Wj^T + bj, no BatchNorm, no ReLU
            DGNN_REQUIRE(!rowptr[l] && Wj[l] && y[l], DGNN_E_INVALID, "static_train_fwd: a layer without statistics is a plain Linear");
            TRY(F32::linear(x, ldx, c_in, Wj[l], c_in, nullptr, 0, 0, nullptr, 0, bj[l], 0, n_dst[l], c_out, y[l], c_out, gemm_mode, stream));
        } else {
            bool counted = false;
            Layer L = {};
            L.mode = gemm_mode, L.stream = stream;
            L.g.rowptr = rowptr[l], L.g.src = src[l], L.g.eid = eid[l], L.g.n_dst = n_dst[l];
            L.s.x = x, L.s.ldx = ldx, L.s.edge = edge_attr[l], L.s.lde = lde[l];
            L.p.c_in = c_in, L.p.c_out = c_out, L.p.f_e = We[l] ? f_e : 0, L.p.We = We[l], L.p.be = be[l], L.p.Wj = Wj[l], L.p.bj = bj[l], L.p.Wi = Wi[l], L.p.relu = 1;
            L.p.has_bn = true, L.p.gamma = gamma[l], L.p.beta = beta[l], L.p.running_mean = running_mean[l], L.p.running_var = running_var[l], L.p.momentum = momentum[l], L.p.eps = eps[l];
            L.s.a = unconst(a[l]), L.s.z = unconst(z[l]), L.s.y = unconst(y[l]);
            L.s.mean = unconst(st), L.s.var = unconst(st + c_out), L.s.scale = unconst(st + 2 * c_out), L.s.shift = unconst(st + 3 * c_out);
            L.p.nbt = num_batches_tracked ? num_batches_tracked[l] : nullptr;
            L.w.fwd_scratch = scratch, L.w.counted = &counted;
            TRY(static_fwd<F32>(L));
            if (counted) counted_mask |= 1u << l;
        }
        x = y[l];
        ldx = c_out;
    }
    if (num_batches_tracked) {
        // the counters the statistics' finalising launches have not already stepped (in the default arithmetic every BatchNorm's has been)
        Ptr8 ps;
        int left = 0;
        for (int l = 0; l < 8; ++l) {
            ps.p[l] = (l < n_layers && !((counted_mask >> l) & 1u)) ? num_batches_tracked[l] : nullptr;
            left += ps.p[l] != nullptr;
        }
        if (left) hipLaunchKernelGGL(k_inc_i64, dim3(1), dim3(64), 0, (hipStream_t)stream, ps, n_layers);
    }
    return dgnn_check_launch("static_train_fwd");
}

namespace {
// scratch of dgnn_static_train_bwd: dz ping-pong | da ([n_dst, 2 c_in]: da next to dz.Wi) | every layer's [Wj^T ; Wi^T] | partials of the dx chain |
// partials of the weight gradients
struct StaticScratch {
    int64_t dz = 0, da = 0, wt_total = 0, tmp = 0, tw = 0, wt_off[8] = {};
};
StaticScratch static_scratch(int n_layers, const int64_t* n_src, const int64_t* n_dst, const int32_t* widths, int f_e) {
    StaticScratch r;
    for (int l = 0; l < n_layers; ++l) {
        const int ci = widths[l], co = widths[l + 1];
        const int64_t a1 = align4(n_dst[l] * co), a2 = 2 * align4(n_dst[l] * ci), a3 = 2 * align4((int64_t)ci * co);
        const int64_t stats = dgnn_colstats_scratch_elems(n_dst[l], co > ci ? co : ci), wg = dgnn_linear_wgrad_scratch_elems(n_dst[l], co, ci),
                      wc = dgnn_linear_wgrad_cat_scratch_elems(n_dst[l], co, ci, ci), ab = dgnn_sage_aggregate_bwd_scratch_elems(n_src[l], ci, f_e > 0 ? f_e : 1);
        if (a1 > r.dz) r.dz = a1;
        if (a2 > r.da) r.da = a2;
        r.wt_off[l] = r.wt_total;
        r.wt_total += a3;
        const int64_t t1 = align4(stats > ab ? stats : ab);
        int64_t t2 = stats > wg ? stats : wg;
        if (wc > t2) t2 = wc;
        t2 = align4(t2);
        if (t1 > r.tmp) r.tmp = t1;
        if (t2 > r.tw) r.tw = t2;
    }
    return r;
}
}  // namespace

extern "C" int64_t dgnn_static_train_scratch_elems(int n_layers, const int64_t* n_src, const int64_t* n_dst, const int32_t* widths, int f_e) {
    if (n_layers < 1 || n_layers > 8 || !n_src || !n_dst || !widths) return 16;
    const StaticScratch r = static_scratch(n_layers, n_src, n_dst, widths, f_e);
    return 2 * r.dz + r.da + r.wt_total + r.tmp + r.tw + 64;
}

// dy: gradient of the last layer's y.  dx_buf[0], dx_buf[1]: two work buffers of max_l n_src[l] * widths[l] floats (layer l writes
// its dx into dx_buf[l & 1], layer l-1 reads it as dy); layer 0's input is data (no dx).  Parameter gradients per layer.  scratch:
// dgnn_static_train_scratch_elems floats.  Everything runs on `stream`.
extern "C" int dgnn_static_train_bwd(int n_layers, const int32_t* const* t_rowptr, const int32_t* const* t_dst, const int32_t* const* t_eid,
                                     const int32_t* const* rowptr_dst, const int64_t* n_src, const int64_t* n_dst, const float* x0, int64_t ldx0,
                                     const int32_t* widths, const float* const* edge_attr, const int64_t* lde, int f_e, const float* const* We,
                                     const float* const* be, const float* const* Wj, const float* const* Wi, const float* const* gamma,
                                     const float* const* stats, const float* eps, const float* const* a, const float* const* z,
                                     const float* const* y, const float* dy, float* const* dWe, float* const* dbe, float* const* dWj,
                                     float* const* dbj, float* const* dWi, float* const* dgamma, float* const* dbeta, float* const* dx_buf,
                                     float* scratch, int gemm_mode, void* stream) {
    DGNN_REQUIRE(n_layers >= 1 && n_layers <= 8 && t_rowptr && t_dst && t_eid && rowptr_dst && n_src && n_dst && x0 && widths && edge_attr && lde && We && be &&
                     Wj && Wi && gamma && stats && eps && a && z && y && dy && dWe && dbe && dWj && dbj && dWi && dgamma && dbeta && dx_buf && scratch,
                 DGNN_E_INVALID, "static_train_bwd: bad args");
    const StaticScratch lay = static_scratch(n_layers, n_src, n_dst, widths, f_e);
    float* dzb[2] = {scratch, scratch + lay.dz};
    float* da = scratch + 2 * lay.dz;
    float* wt = da + lay.da;
    float* tmp = wt + lay.wt_total;
    float* tmp_w = tmp + lay.tmp;
    // all transposes of the pass in one launch (fused chain), into per-layer regions; otherwise every layer transposes into the first region
    const bool pre_t = gemm_mode != DGNN_GEMM_F32 && fused_enabled();
    if (pre_t) {
        TrJobs jobs;
        jobs.n = 0;
        for (int l = 0; l < n_layers; ++l) {
            const int ci = widths[l], co = widths[l + 1];
            const bool agg = t_rowptr[l] != nullptr, need_dx = l > 0;
            const bool need_da = agg ? (need_dx || We[l] != nullptr) : need_dx;
            if (!need_da) continue;
            tr_add(jobs, Wj[l], wt + lay.wt_off[l], co, ci);
            if (agg && need_dx && Wi[l]) tr_add(jobs, Wi[l], wt + lay.wt_off[l] + (int64_t)ci * co, co, ci);
        }
        transpose_many(jobs, (hipStream_t)stream);
    }
    const float* g = dy;
    for (int l = n_layers - 1; l >= 0; --l) {
        const int c_in = widths[l], c_out = widths[l + 1];
        const float* st = stats[l];   // (mean, var, scale, shift); NULL: a plain Linear
        float* dx = l == 0 ? nullptr : dx_buf[l & 1];
        Layer L = {};
        L.mode = gemm_mode, L.stream = stream;
        L.g.t_rowptr = t_rowptr[l], L.g.t_dst = t_dst[l], L.g.t_eid = t_eid[l], L.g.rowptr_dst = rowptr_dst[l], L.g.n_src = n_src[l], L.g.n_dst = n_dst[l];
        L.s.x = l == 0 ? x0 : y[l - 1], L.s.ldx = l == 0 ? ldx0 : c_in, L.s.edge = edge_attr[l], L.s.lde = lde[l];
        L.p.c_in = c_in, L.p.c_out = c_out, L.p.f_e = We[l] ? f_e : 0, L.p.We = We[l], L.p.be = be[l], L.p.Wj = Wj[l], L.p.Wi = Wi[l], L.p.relu = 1;
        if (st) {
            L.p.has_bn = true, L.p.gamma = gamma[l], L.p.eps = eps[l];
            L.s.mean = unconst(st), L.s.var = unconst(st + c_out), L.s.scale = unconst(st + 2 * c_out), L.s.shift = unconst(st + 3 * c_out);
        }
        L.s.a = unconst(a[l]), L.s.z = unconst(z[l]), L.s.y = unconst(y[l]);
        L.d.dy = g, L.d.dx = dx, L.d.dWe = dWe[l], L.d.dbe = dbe[l], L.d.dWj = dWj[l], L.d.dbj = dbj[l], L.d.dWi = dWi[l], L.d.dgamma = dgamma[l], L.d.dbeta = dbeta[l];
        L.w.dz = dzb[l & 1], L.w.da = da;
        L.w.WjT = wt + (pre_t ? lay.wt_off[l] : 0), L.w.WiT = L.w.WjT + (int64_t)c_in * c_out;
        L.w.tmp = tmp, L.w.tmp_w = tmp_w, L.w.pre_t = pre_t;
        TRY(static_bwd<F32>(L));
        g = dx;
    }
    return DGNN_OK;
}

// =====================================================================================================================
// All conv layers of the Updated variant per call (surfaceNetUpdatedEdgeFilters.py:229-243 and its autograd): the per-layer composite calls
// above and the edge chaining between them (chain.hip) issued back to back from C++ -- one autograd node for the stack instead of three per
// layer (edge rows, cast, conv): the step was bound by the ~16 Python-level nodes each way.  The same kernels in the same order as the
// per-layer path (bit-identical results).
//   ea_0 = edge_attr_all[rows0, :edge_in_0]                        (:237; bf16 storage: cast once)
//   ea_l = relu(zeros[E_all, C]; [e_id_{l-1}] = phi_{l-1})[e_id_l, :edge_in_l]      (:233-241, only the rows that are read)
//   (y_l, phi_l) = conv_l(x_l, ea_l), x_{l+1} = relu?(y_l)
// Backward: layer l's d_ea goes through the chaining's backward into dphi_ext of layer l-1.
// =====================================================================================================================
extern "C" int dgnn_updated_stack_fwd(int n_layers, const int32_t* const* rowptr, const int32_t* const* src, const int32_t* const* eid,
                                      const int64_t* const* e_id, const int32_t* rows0, const int64_t* n_dst, const int64_t* E, const void* x0,
                                      int64_t ldx0, const int32_t* widths, const int32_t* edge_in, const float* edge_attr_all, int64_t lde_all,
                                      int64_t E_all, int32_t* pos, const float* const* We, const float* const* be, const float* const* Wl,
                                      const float* const* bl, const float* const* Wr, const int32_t* relu, void* const* ea, const int64_t* ld_ea,
                                      float* ea0_f32, void* const* phi, void* const* a, void* const* y, int32_t* const* inv, int bf16, int gemm_mode,
                                      void* stream) {
    DGNN_REQUIRE(n_layers >= 1 && n_layers <= 8 && rowptr && src && eid && e_id && rows0 && n_dst && E && x0 && widths && edge_in && edge_attr_all && pos &&
                     We && be && Wl && bl && Wr && relu && ea && ld_ea && phi && a && y && inv && (!bf16 || ea0_f32),
                 DGNN_E_INVALID, "updated_stack_fwd: bad args (at most 8 layers)");
    const void* x = x0;
    int64_t ldx = ldx0;
    for (int l = 0; l < n_layers; ++l) {
        const int c_in = widths[l], c_out = widths[l + 1], k = edge_in[l];
        if (l == 0) {
            if (E[0] > 0) {
                if (bf16) {
                    TRY(dgnn_gather_rows_f32(edge_attr_all, lde_all, rows0, E[0], k, ea0_f32, k, stream));
                    TRY(dgnn_cast_f32_to_bf16(ea0_f32, k, E[0], k, (int)ld_ea[0], (uint16_t*)ea[0], ld_ea[0], stream));
                } else {
                    TRY(dgnn_gather_rows_f32(edge_attr_all, lde_all, rows0, E[0], k, (float*)ea[0], ld_ea[0], stream));
                }
            }
        } else if (E[l] > 0 || E[l - 1] > 0) {
            DGNN_REQUIRE(inv[l], DGNN_E_INVALID, "updated_stack_fwd: inv[%d] missing", l);
            if (bf16)
                TRY(dgnn_edge_chain_fwd_bf16((const uint16_t*)phi[l - 1], widths[l - 1], k, e_id[l - 1], E[l - 1], e_id[l], E[l], E_all, pos, 1, (uint16_t*)ea[l],
                                             ld_ea[l], inv[l], stream));
            else
                TRY(dgnn_edge_chain_fwd((const float*)phi[l - 1], widths[l - 1], k, e_id[l - 1], E[l - 1], e_id[l], E[l], E_all, pos, 1, (float*)ea[l], ld_ea[l],
                                        inv[l], stream));
        }
        TRY(dgnn_sage_updated_train_fwd(rowptr[l], src[l], eid[l], n_dst[l], x, ldx, c_in, ea[l], ld_ea[l], k, E[l], We[l], be[l], Wl[l], bl[l], Wr[l], c_out,
                                        relu[l], phi[l], a[l], y[l], bf16, gemm_mode, stream));
        x = y[l];
        ldx = c_out;
    }
    return dgnn_check_launch("updated_stack_fwd");
}

// scratch: max over the layers of dgnn_sage_updated_train_scratch_elems.  Work buffers (storage type): dx_buf[0], dx_buf[1] (max n_src * c_in
// over the layers l >= 1), d_ea (max E_l * edge_in_l, l >= 1), dphi_ext (max E_l * c_in_l, l < n_layers - 1), dz (max n_dst * c_out), da
// (max 2 * n_dst * c_in), dphi (max E_l * c_in_l).
extern "C" int dgnn_updated_stack_bwd(int n_layers, const int32_t* const* t_rowptr, const int32_t* const* t_dst, const int32_t* const* t_eid,
                                      const int32_t* const* rowptr_dst, const int64_t* n_src, const int64_t* n_dst, const int64_t* E, const void* x0,
                                      int64_t ldx0, const int32_t* widths, const int32_t* edge_in, const float* const* We, const float* const* Wl,
                                      const float* const* Wr, const int32_t* relu, const void* const* ea, const int64_t* ld_ea, const void* const* phi,
                                      const void* const* a, const void* const* y, const int32_t* const* inv, const void* dy, float* const* dWe,
                                      float* const* dbe, float* const* dWl, float* const* dbl, float* const* dWr, void* const* dx_buf, void* d_ea,
                                      void* dphi_ext, void* dz, void* da, void* dphi, float* scratch, int bf16, int gemm_mode, void* stream) {
    DGNN_REQUIRE(n_layers >= 1 && n_layers <= 8 && t_rowptr && t_dst && t_eid && rowptr_dst && n_src && n_dst && E && x0 && widths && edge_in && We && Wl && Wr &&
                     relu && ea && ld_ea && phi && a && y && inv && dy && dWe && dbe && dWl && dbl && dWr && dx_buf && dz && da && dphi && scratch &&
                     (n_layers == 1 || (d_ea && dphi_ext && dx_buf[0] && dx_buf[1])),
                 DGNN_E_INVALID, "updated_stack_bwd: bad args");
    int (*const layer_bwd)(const Layer&) = bf16 ? updated_bwd<BF16> : updated_bwd<F32>;
    const void* g = dy;
    bool have_ext = false;
    // a layer stores its dx already masked by the ReLU of the layer below (its own input x is that layer's post-ReLU output), so the layer below
    // takes it as dz: one k_relu_bwd launch per inner layer less.  DGNN_UPDATED_MASK_DX=0: every layer masks its own dy.
    static const bool mask_on = !(getenv("DGNN_UPDATED_MASK_DX") && getenv("DGNN_UPDATED_MASK_DX")[0] == '0');
    bool g_masked = false;
    for (int l = n_layers - 1; l >= 0; --l) {
        const int c_in = widths[l], c_out = widths[l + 1], k = edge_in[l];
        void* dx = l == 0 ? nullptr : dx_buf[l & 1];
        DGNN_REQUIRE(n_dst[l] > 0 && n_src[l] >= n_dst[l] && E[l] >= 0 && c_in > 0 && c_out > 0 && k > 0, DGNN_E_INVALID, "updated_stack_bwd: bad sizes");
        bool masked = false;
        Layer L = {};
        L.mode = gemm_mode, L.stream = stream;
        L.g.t_rowptr = t_rowptr[l], L.g.t_dst = t_dst[l], L.g.t_eid = t_eid[l], L.g.rowptr_dst = rowptr_dst[l], L.g.n_src = n_src[l], L.g.n_dst = n_dst[l], L.g.E = E[l];
        L.s.x = l == 0 ? x0 : y[l - 1], L.s.ldx = l == 0 ? ldx0 : c_in, L.s.edge = ea[l], L.s.lde = ld_ea[l];
        L.p.c_in = c_in, L.p.c_out = c_out, L.p.f_e = k, L.p.We = We[l], L.p.Wj = Wl[l], L.p.Wi = Wr[l], L.p.relu = relu[l];
        L.s.a = unconst(a[l]), L.s.y = unconst(y[l]), L.s.phi = unconst(phi[l]);
        L.d.dy = g, L.d.dphi_ext = have_ext ? dphi_ext : nullptr, L.d.dx = dx, L.d.d_ea = l > 0 ? d_ea : nullptr, L.d.dWe = dWe[l], L.d.dbe = dbe[l], L.d.dWj = dWl[l], L.d.dbj = dbl[l], L.d.dWi = dWr[l];
        set_updated_work(L, dz, da, dphi, scratch);
        L.d.dy_is_dz = g_masked, L.d.want_mask = mask_on && l > 0 && relu[l - 1] != 0, L.d.masked = &masked;
        TRY(layer_bwd(L));
        g_masked = masked;
        have_ext = false;
        if (l > 0 && E[l - 1] > 0) {   // layer l's edge rows came out of phi_{l-1}: their gradient is what layer l-1 adds to its dphi
            if (bf16)
                TRY(dgnn_edge_chain_bwd_bf16((const uint16_t*)d_ea, k, (const uint16_t*)phi[l - 1], widths[l - 1], inv[l], E[l - 1], k, widths[l - 1], 1,
                                             (uint16_t*)dphi_ext, widths[l - 1], stream));
            else
                TRY(dgnn_edge_chain_bwd((const float*)d_ea, k, (const float*)phi[l - 1], widths[l - 1], inv[l], E[l - 1], k, widths[l - 1], 1, (float*)dphi_ext,
                                        widths[l - 1], stream));
            have_ext = true;
        }
        g = dx;
    }
    return dgnn_check_launch("updated_stack_bwd");
}

// The Updated model's output network behind the conv stack ("sage+": out_net = ReLU, Linear(C, H), ReLU, Linear(H, n_out), reference
// surfaceNetUpdatedEdgeFilters.py:210, 245-247; the first ReLU is the one after the last conv) as one call each way, for the same autograd node:
//   h = relu(x . W1^T + b1)   (storage type)        logits = h . W3^T + b3   (fp32)
// backward: dW3 / db3 and dW1 / db1 from one launch pair each, dh = g . W3, dz1 = dh * [h > 0], dx = dz1 . W1; one transpose launch.
// dh: [n, H] work buffer (storage type).
extern "C" int dgnn_updated_tail_fwd(int64_t n, const void* x, int64_t ldx, int c, const float* W1, const float* b1, int hdim, const float* W3, const float* b3,
                                     int n_out, void* h, float* logits, int bf16, int gemm_mode, void* stream) {
    DGNN_REQUIRE(n > 0 && c > 0 && hdim > 0 && n_out > 0 && x && W1 && W3 && h && logits, DGNN_E_INVALID, "updated_tail_fwd: bad arguments");
    if (bf16) {
        TRY(BF16::linear((const uint16_t*)x, ldx, c, W1, c, nullptr, 0, 0, nullptr, 0, b1, 1, n, hdim, (uint16_t*)h, hdim, gemm_mode, stream));
        // (fp32 logits from bf16 rows: the one GEMM here that is not in the storage type)
        return dgnn_linear_fwd_bf16((const uint16_t*)h, hdim, hdim, W3, hdim, nullptr, 0, 0, nullptr, 0, b3, nullptr, nullptr, 0, n, n_out, logits, n_out, 1, stream);
    }
    TRY(F32::linear((const float*)x, ldx, c, W1, c, nullptr, 0, 0, nullptr, 0, b1, 1, n, hdim, (float*)h, hdim, gemm_mode, stream));
    return F32::linear((const float*)h, hdim, hdim, W3, hdim, nullptr, 0, 0, nullptr, 0, b3, 0, n, n_out, logits, n_out, gemm_mode, stream);
}

namespace {
// scratch of dgnn_updated_tail_bwd: W3^T [hdim, n_out] | W1^T [c, hdim] | partial sums | bf16 copy of the logits' gradient (bf16 storage) | slack (the
// size has always counted the transposes twice; callers allocate by it)
struct TailScratch {
    int64_t W3T = 0, W1T = 0, tmp = 0, gb = 0, total = 0;
};
TailScratch tail_scratch(int64_t n, int c, int hdim, int n_out) {
    const int64_t w1 = dgnn_linear_wgrad_cat_scratch_elems(n, hdim, c, 0), w3 = dgnn_linear_wgrad_cat_scratch_elems(n, n_out, hdim, 0);
    const int64_t cs = dgnn_colstats_scratch_elems(n, hdim > n_out ? hdim : n_out), wg = dgnn_linear_wgrad_scratch_elems(n, hdim, c);
    int64_t big = w1 > w3 ? w1 : w3;
    if (cs > big) big = cs;
    if (wg > big) big = wg;
    TailScratch r;
    r.W1T = align4((int64_t)hdim * n_out);
    r.tmp = r.W1T + align4((int64_t)c * hdim);
    r.gb = r.tmp + align4(big);
    r.total = r.gb + align4(n * n_out) + r.tmp + 64;
    return r;
}
}  // namespace

extern "C" int64_t dgnn_updated_tail_scratch_elems(int64_t n, int c, int hdim, int n_out) {
    if (n < 0 || c <= 0 || hdim <= 0 || n_out <= 0) return 64;
    return tail_scratch(n, c, hdim, n_out).total;
}

extern "C" int dgnn_updated_tail_bwd(int64_t n, const void* x, int64_t ldx, int c, const float* W1, int hdim, const float* W3, int n_out, const void* h,
                                     const float* g, float* dW1, float* db1, float* dW3, float* db3, void* dx, void* dh, float* scratch, int bf16,
                                     int gemm_mode, void* stream_) {
    DGNN_REQUIRE(n > 0 && c > 0 && hdim > 0 && n_out > 0 && x && W1 && W3 && h && g && dW1 && dW3 && dx && dh && scratch, DGNN_E_INVALID,
                 "updated_tail_bwd: bad arguments");
    const TailScratch lay = tail_scratch(n, c, hdim, n_out);
    float *W3T = scratch + lay.W3T, *W1T = scratch + lay.W1T, *tmp = scratch + lay.tmp;
    TrJobs jobs;
    jobs.n = 0;
    tr_add(jobs, W3, W3T, n_out, hdim);
    tr_add(jobs, W1, W1T, hdim, c);
    transpose_many(jobs, (hipStream_t)stream_);
    const bool fused = fused_enabled();
    if (bf16) {
        uint16_t* gb = reinterpret_cast<uint16_t*>(scratch + lay.gb);
        const uint16_t* hb = (const uint16_t*)h;
        uint16_t* dhb = (uint16_t*)dh;
        const int gp = (n_out + 1) / 2 * 2;
        TRY(dgnn_cast_f32_to_bf16(g, n_out, n, n_out, gp, gb, gp, stream_));
        if (fused) {   // (g stays fp32 in the weight gradient: the `1` behind it)
            TRY(dgnn_linear_wgrad_bf16_cat(g, 1, n_out, n_out, h, hdim, hdim, nullptr, 0, 0, 0, n, dW3, nullptr, db3, tmp, stream_));
        } else {
            TRY(dgnn_linear_wgrad_bf16(g, 1, n_out, n_out, h, 0, hdim, hdim, n, dW3, hdim, 0, tmp, stream_));
            if (db3) TRY(dgnn_colsum(g, n_out, n, n_out, db3, 0, tmp, stream_));
        }
        TRY(BF16::linear(gb, gp, n_out, W3T, n_out, nullptr, 0, 0, nullptr, 0, nullptr, 0, n, hdim, dhb, hdim, gemm_mode, stream_));
        TRY(BF16::relu_bwd(hb, dhb, n * hdim, dhb, stream_));
        if (fused) {
            TRY(BF16::wgrad_cat(dhb, hdim, hdim, (const uint16_t*)x, ldx, c, nullptr, 0, 0, n, dW1, nullptr, db1, tmp, stream_));
        } else {
            TRY(BF16::wgrad(dhb, hdim, hdim, (const uint16_t*)x, ldx, c, n, dW1, tmp, gemm_mode, stream_));
            if (db1) TRY(BF16::colsum(dhb, hdim, n, hdim, db1, tmp, stream_));
        }
        TRY(BF16::linear(dhb, hdim, hdim, W1T, hdim, nullptr, 0, 0, nullptr, 0, nullptr, 0, n, c, (uint16_t*)dx, c, gemm_mode, stream_));
        return dgnn_check_launch("updated_tail_bwd");
    }
    const float* hf = (const float*)h;
    float* dhf = (float*)dh;
    auto wgrad = [&](const float* A, int64_t lda, int na, const float* B, int64_t ldb, int nb, float* dW, float* dbias) {
        if (fused && F32::can_fuse(gemm_mode)) return F32::wgrad_cat(A, lda, na, B, ldb, nb, nullptr, 0, 0, n, dW, nullptr, dbias, tmp, stream_);
        int rc = F32::wgrad(A, lda, na, B, ldb, nb, n, dW, tmp, gemm_mode, stream_);
        if (rc == DGNN_OK && dbias) rc = F32::colsum(A, lda, n, na, dbias, tmp, stream_);
        return rc;
    };
    TRY(wgrad(g, n_out, n_out, hf, hdim, hdim, dW3, db3));
    TRY(F32::linear(g, n_out, n_out, W3T, n_out, nullptr, 0, 0, nullptr, 0, nullptr, 0, n, hdim, dhf, hdim, gemm_mode, stream_));
    TRY(F32::relu_bwd(hf, dhf, n * hdim, dhf, stream_));
    TRY(wgrad(dhf, hdim, hdim, (const float*)x, ldx, c, dW1, db1));
    TRY(F32::linear(dhf, hdim, hdim, W1T, hdim, nullptr, 0, 0, nullptr, 0, nullptr, 0, n, c, (float*)dx, c, gemm_mode, stream_));
    return dgnn_check_launch("updated_tail_bwd");
}

// Which of the training step's fused launch chains run (bit 0: backward chain, bit 1: batch statistics from the forward GEMM's epilogue;
// default 3, DGNN_TRAIN_FUSED in the environment).  Returns the previous mask.
extern "C" int dgnn_train_set_fused(int mask) {
    const int was = fused_mask();
    __atomic_store_n(&g_fused_on, mask & 3, __ATOMIC_RELEASE);
    return was;
}
