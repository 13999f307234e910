/*
 * dgnn_hip.h -- C ABI of libdgnn_hip.so: the MI355X (gfx950) kernels behind the hot path of
 * raphaelsulzer/dgnn (edge-filtered GraphSAGE over the tetrahedron-adjacency graph).
 *
 * The reference has no FFI / operator registry: its seam is the Python module API
 * (learning/surfaceNetStaticEdgeFilters.py, learning/surfaceNetUpdatedEdgeFilters.py).  The Python
 * mirror in dgnn_amd/ keeps that API and binds these entry points with ctypes;
 * each entry point below cites the reference lines (relative to the reference root) it replaces.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer (e.g. torch.Tensor.data_ptr()); sizes are element counts;
 *    `ld*` are row strides in elements; all float data is fp32 row-major, all indices int32 unless
 *    stated (the reference's edge_index is int64 [2,E] and is consumed as such by the plan builder);
 *  - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *  - nothing here allocates, frees or synchronises: the caller owns every buffer, including the
 *    plan arrays and scratch; calls are asynchronous on `stream`;
 *  - return value: 0 = ok, negative = DGNN_E_*; dgnn_last_error_string() describes the last
 *    failure on the calling thread.  Functions never throw.
 *  - thread safety: no global mutable state except the thread-local error string; calls on
 *    distinct streams may run concurrently.
 */
#ifndef DGNN_HIP_H
#define DGNN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DGNN_VERSION 100 /* major*10000 + minor*100 + patch */

#define DGNN_OK 0
#define DGNN_E_INVALID -1     /* bad argument (null pointer, negative size, unsupported width) */
#define DGNN_E_UNSUPPORTED -2 /* shape outside what the kernel family handles */
#define DGNN_E_LAUNCH -3      /* hipGetLastError() after launch */
#define DGNN_E_INDEX -4       /* a kernel met an index outside its range (reported asynchronously, see dgnn_poll_async_error) */

int dgnn_version(void);
const char* dgnn_last_error_string(void);
/* Data-dependent errors a launch-time check cannot see (an edge_index entry outside [0, n): torch's scatter raises an index
 * error there, surfaceNetStaticEdgeFilters.py:80) are reported asynchronously, like HIP's own: the kernel stays memory-safe
 * (skips the edge), sets a bit in a pinned host word, and this call -- after any later stream synchronisation, or simply at
 * the next entry point -- returns DGNN_E_INDEX once and clears it (0 = nothing pending). */
int dgnn_poll_async_error(void);

/* ------------------------------------------------------------------------------------------------
 * Graph plan: destination-sorted CSR of an edge list, STABLE in edge position.
 *
 * Replaces the implicit per-call work of PyG `MessagePassing.propagate` + torch_scatter
 * `scatter(reduce='mean')` (call site surfaceNetStaticEdgeFilters.py:80): there the aggregation
 * index is edge_index[1] and CPU accumulation runs in ascending edge position per destination.  The
 * plan makes that order explicit: for destination i, sorted edges rowptr[i]..rowptr[i+1]-1 are its
 * in-edges in ascending original position; src[k] = edge_index[0][eid[k]].
 *
 * `by` selects the sort key row of edge_index: 1 = by destination (forward), 0 = by source
 * (the transposed plan used by the backward pass; then `src` receives the OTHER endpoint,
 * i.e. the destination, and n_key = number of sources).
 *
 *   edge_index : int64 [2,E] view, row0=src row1=dst: element (r,k) at edge_index[r*stride_row + k*stride_col].
 *                The reference passes torch.transpose(adjacencies,1,0) (processing/data.py:434-438), i.e.
 *                strides (1,2) over the [E,2] array; a contiguous [2,E] tensor has (E,1).  Read in place.
 *   n_other    : number of nodes on the OTHER side (sources for by=1), for range checking; 0 = unknown, unchecked.
 *                Endpoints outside [0,n_key) / [0,n_other) never index memory: such edges are left out of the plan (key)
 *                or point at node 0 (other) and DGNN_E_INDEX is reported through dgnn_poll_async_error().
 *   rowptr     : int32 [n_key+1]   out
 *   other      : int32 [E]         out  (src for by=1, dst for by=0)
 *   eid        : int32 [E]         out  original edge position of the k-th sorted edge
 *   scratch    : int32 [dgnn_plan_scratch_elems(E,n_key)]
 * Two verified single-pass builders run before the generic count/scan/fill/sort kernels:
 *   GROUPED   - the edge list is already ascending in the key row (k-hop sampled blocks, a partition's local
 *               list, the by-source plan of the reference layout): the sort is the identity;
 *   REFERENCE - by destination, E == 4*n_key, row 4t+r = r-th neighbour of cell t, symmetric relation (what
 *               processing/data.py hands the model): in-edges are the reversed out-edges, no atomics/scan/sort.
 * `hint` only selects which of them is attempted (AUTO: both).  Each checks its precondition on the device;
 * when it does not hold, the generic builder queued behind it -- ONE persistent launch that returns at once when a fast path
 * produced the plan -- rebuilds it.  Same result in every case.  (REFERENCE with the (src, dst) pairs interleaved in memory,
 * stride_row 1 / stride_col 2 and a 16-byte aligned base: four lanes per cell, 16-byte loads.)
 * ---------------------------------------------------------------------------------------------- */
#define DGNN_PLAN_HINT_AUTO 0
#define DGNN_PLAN_HINT_GROUPED 1
#define DGNN_PLAN_HINT_REFERENCE 2
#define DGNN_PLAN_HINT_GENERIC 3 /* attempt neither: straight to the generic kernels */
#define DGNN_PLAN_HINT_GROUPED_TRUSTED 4 /* GROUPED without the device-side check and without the generic builder standing by: ONE launch.  For lists
                                           * the caller laid out itself (a ring part); a list that is not ascending in range gives a wrong plan (never an
                                           * out-of-bounds write) */
int64_t dgnn_plan_scratch_elems(int64_t E, int64_t n_key);
int dgnn_plan_build(const int64_t* edge_index, int64_t stride_row, int64_t stride_col, int64_t E, int64_t n_key,
                    int64_t n_other, int by, int hint, int32_t* rowptr, int32_t* other, int32_t* eid, int32_t* scratch,
                    void* stream);

/* out[k, 0:cols] = in[idx[k], 0:cols]  -- stages edge_attr rows into plan order once per scene
 * (the reference gathers them implicitly: `xe[e_id]` at surfaceNetStaticEdgeFilters.py:262,304). */
int dgnn_gather_rows_f32(const float* in, int64_t ld_in, const int32_t* idx, int64_t n, int cols, float* out,
                         int64_t ld_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Edge-filtered mean aggregation (forward).  Replaces surfaceNetStaticEdgeFilters.py:75-80 + :89-96
 * (lin_e -> index_select -> x_j * phi -> scatter mean) and surfaceNetUpdatedEdgeFilters.py:156-158.
 *
 *   a[i,:] = ( sum_{k in rowptr[i]..rowptr[i+1]} x_src[src[k],:] * phi_k ) / max(deg_i,1)
 *   phi_k  = We . edge_attr[e,:] + be          (mode "fused": We != NULL, F_e <= 32)
 *          = phi[e,:]                           (mode "given": We == NULL, phi != NULL)
 *          = 1                                  (both NULL: plain mean, lin_e is None at :77-78)
 *   e      = eid ? eid[k] : k                   (eid == NULL: edge rows already in plan order)
 *
 * The sum runs in plan order with separately rounded multiply and add, i.e. the CPU order of
 * torch_scatter.  phi_out (optional, fused mode) receives phi rows at index e: the Updated variant
 * returns them (surfaceNetUpdatedEdgeFilters.py:170).
 * ---------------------------------------------------------------------------------------------- */
int dgnn_sage_aggregate_fwd(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int64_t n_dst,
                            const float* x_src, int64_t ldx, int c_in, const float* edge_attr, int64_t lde, int f_e,
                            const float* We, const float* be, const float* phi, int64_t ldphi, float* phi_out,
                            int64_t ldphi_out, float* a, int64_t lda, void* stream);

/* ------------------------------------------------------------------------------------------------
 * out = act( (A1 . W1^T + A2 . W2^T + bias) * scale + shift )      [M, n_out]
 *
 * Replaces lin_j(out) + lin_i(x_r) (surfaceNetStaticEdgeFilters.py:81-86; lin_l/lin_r at
 * surfaceNetUpdatedEdgeFilters.py:159-165), eval-mode BatchNorm folded to scale/shift (:218) and
 * ReLU (:219); also the decoder Linears (:180-187) and lin_e of the Updated variant when its input
 * is wide.  W1 [n_out,K1], W2 [n_out,K2] are torch.nn.Linear weights (row-major).  A2/W2, bias,
 * scale/shift may be NULL.  `relu`: bit 0 applies max(0,.); bit 1 (DGNN_LINEAR_ACCUMULATE) adds the result to what `out`
 * holds (dx_dst += G . Wi in the backward pass).  fp32 MFMA (v_mfma_f32_32x32x2_f32).
 * ---------------------------------------------------------------------------------------------- */
#define DGNN_LINEAR_ACCUMULATE 2
int dgnn_linear_fwd(const float* A1, int64_t lda1, int k1, const float* W1, int64_t ldw1, const float* A2,
                    int64_t lda2, int k2, const float* W2, int64_t ldw2, const float* bias, const float* scale,
                    const float* shift, int relu, int64_t M, int n_out, float* out, int64_t ldo, void* stream);

/* dgnn_linear_fwd / dgnn_linear_wgrad with the fused layers' arithmetic (DGNN_GEMM_BF16X3): both fp32 operands are split exactly
 * into 3 bf16 parts while staged, 6 partial products on v_mfma_f32_32x32x16_bf16, fp32 accumulate -- fp32-class accuracy
 * (dropped terms <= 2^-25 relative) at 6/16 of the fp32-MFMA time.  Same arguments and scratch sizes. */
int dgnn_linear_fwd_x3(const float* A1, int64_t lda1, int k1, const float* W1, int64_t ldw1, const float* A2, int64_t lda2, int k2,
                       const float* W2, int64_t ldw2, const float* bias, const float* scale, const float* shift, int relu, int64_t M,
                       int n_out, float* out, int64_t ldo, void* stream);
/* The same product in the fp16 form of DGNN_GEMM_F16X2 (below): every row of [A1 | A2] and of [W1 | W2] scaled by its own power of two,
 * split into 2 fp16 parts, 3 products per fp32 product on v_mfma_f32_32x32x16_f16, fp32 accumulate (dropped terms <= 2^-22 relative).
 * Covers M >= 8192 with n_out > 128 (the wide conv layers); other shapes return DGNN_E_UNSUPPORTED -- use dgnn_linear_fwd_x3.
 * scratch: dgnn_linear_fwd_x2h_scratch_elems(M, n_out) floats (the row scales, written by a first pass over the operands). */
int64_t dgnn_linear_fwd_x2h_scratch_elems(int64_t M, int n_out);
int dgnn_linear_fwd_x2h(const float* A1, int64_t lda1, int k1, const float* W1, int64_t ldw1, const float* A2, int64_t lda2, int k2,
                        const float* W2, int64_t ldw2, const float* bias, const float* scale, const float* shift, int relu,
                        int64_t M, int n_out, float* out, int64_t ldo, float* scratch, void* stream);
/* dgnn_linear_fwd_x2h with both operands split ONCE by a pass of their own (row scale, (hi, lo) fp16 in the GEMM's staging format) and staged
 * global -> LDS by DMA: same arguments, results bit-identical to dgnn_linear_fwd_x2h, no split arithmetic between the matrix instructions.
 * scratch: dgnn_linear_fwd_x2hp_scratch_elems(M, n_out, k1, k2) floats, 16-byte aligned (row scales + the pre-split operands, 4 bytes per
 * element of [A1 | A2] and [W1 | W2] with k1, k2 rounded up to multiples of 32). */
int64_t dgnn_linear_fwd_x2hp_scratch_elems(int64_t M, int n_out, int k1, int k2);
int dgnn_linear_fwd_x2hp(const float* A1, int64_t lda1, int k1, const float* W1, int64_t ldw1, const float* A2, int64_t lda2, int k2,
                         const float* W2, int64_t ldw2, const float* bias, const float* scale, const float* shift, int relu,
                         int64_t M, int n_out, float* out, int64_t ldo, float* scratch, void* stream);

int dgnn_linear_wgrad_x3(const float* A, int64_t lda, int n_a, const float* B, int64_t ldb, int n_b, int64_t M, float* dW, int64_t lddw,
                         int accumulate, float* partials, void* stream);

/* Training forward of `lin_j(a) + lin_i(x_dst)` with the BatchNorm that follows (:217-218): dgnn_linear_fwd_x3 (no scale / shift / relu) whose
 * epilogue also leaves the fp64 column sums and sums of squares of `out` per block of 32 rows in colstats[ceil(M / 32)][2][n_out]
 * (8-byte aligned; dgnn_colstats_scratch_elems floats hold it); dgnn_bn_stats_finalize_fold turns them into mean / var / running
 * statistics / folded scale and shift like dgnn_bn_batch_stats_fold does from its own partial sums.  DGNN_E_UNSUPPORTED (nothing
 * launched) where the GEMM takes its 256 x 256 tile (n_out > 128 and at least 192 such tiles). */
int dgnn_linear_fwd_x3_stats(const float* A1, int64_t lda1, int k1, const float* W1, int64_t ldw1, const float* A2, int64_t lda2, int k2,
                             const float* W2, int64_t ldw2, const float* bias, int64_t M, int n_out, float* out, int64_t ldo,
                             double* colstats, void* stream);
int dgnn_bn_stats_finalize_fold(const double* colstats, int64_t nblk, int64_t M, int c, float* mean, float* var, float* running_mean,
                                float* running_var, float momentum, const float* gamma, const float* beta, float eps, float* scale,
                                float* shift, void* stream);

/* Both weight gradients of a conv layer and its bias gradient in one launch pair (autograd of :81-86 for lin_j, lin_i and lin_j.bias):
 * dW1[n_a, n_b1] = A^T . B1, dW2[n_a, n_b2] = A^T . B2 (B2 NULL / n_b2 0: none), dbias[n_a] = column sums of A (NULL: none), all
 * WRITTEN, contiguous.  dW1 / dW2 are bit-identical to two dgnn_linear_wgrad_x3 calls (same row splits, same products); dbias is summed
 * in fp64 like dgnn_colsum, in another order.  scratch: dgnn_linear_wgrad_cat_scratch_elems floats. */
int64_t dgnn_linear_wgrad_cat_scratch_elems(int64_t M, int n_a, int n_b1, int n_b2);
int dgnn_linear_wgrad_x3_cat(const float* A, int64_t lda, int n_a, const float* B1, int64_t ldb1, int n_b1, const float* B2, int64_t ldb2,
                             int n_b2, int64_t M, float* dW1, float* dW2, float* dbias, float* scratch, void* stream);

/* dW[n_a, n_b] (+)= A^T . B over M rows (weight gradients of the Linears above: autograd of :81-86).
 * Deterministic two-stage reduction; `partials` holds dgnn_linear_wgrad_scratch_elems floats. */
int64_t dgnn_linear_wgrad_scratch_elems(int64_t M, int n_a, int n_b);
int dgnn_linear_wgrad(const float* A, int64_t lda, int n_a, const float* B, int64_t ldb, int n_b, int64_t M,
                      float* dW, int64_t lddw, int accumulate, float* partials, void* stream);

/* ------------------------------------------------------------------------------------------------
 * BatchNorm1d pieces (torch_geometric BatchNorm -> torch.nn.BatchNorm1d, eps 1e-5, momentum 0.1;
 * used at surfaceNetStaticEdgeFilters.py:165,173,185; applied :218,263,305,345).
 * ---------------------------------------------------------------------------------------------- */
/* eval fold: scale = gamma/sqrt(var+eps), shift = beta - mean*scale */
int dgnn_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float eps, int c,
                 float* scale, float* shift, void* stream);
/* column sums and sums of squares (fp64 accumulation inside) -> mean[c], biased var[c]; when
 * running_* != NULL updates them with momentum and the UNBIASED variance, as BatchNorm1d.train(). */
int64_t dgnn_colstats_scratch_elems(int64_t M, int c);
int dgnn_bn_batch_stats(const float* x, int64_t ldx, int64_t M, int c, float* mean, float* var, float* running_mean,
                        float* running_var, float momentum, float* scratch, void* stream);
/* dgnn_bn_batch_stats followed by dgnn_bn_fold on its result, in the same two launches as dgnn_bn_batch_stats alone */
int dgnn_bn_batch_stats_fold(const float* x, int64_t ldx, int64_t M, int c, float* mean, float* var, float* running_mean,
                             float* running_var, float momentum, const float* gamma, const float* beta, float eps, float* scale,
                             float* shift, float* scratch, void* stream);
/* y = act(x*scale + shift) elementwise over [M,c] (train-mode BN apply + ReLU; in place allowed) */
int dgnn_scale_shift_act(const float* x, int64_t ldx, const float* scale, const float* shift, int relu, int64_t M,
                         int c, float* y, int64_t ldy, void* stream);
/* backward of y = relu(bn(x)):  given y, dy (and x_hat recomputed from x, mean, invstd) produce
 * dx, dgamma, dbeta.  train != 0 uses the batch-statistics formula, else dx = dy*mask*scale. */
int dgnn_bn_relu_bwd(const float* x, int64_t ldx, const float* y, int64_t ldy, const float* dy, int64_t lddy,
                     const float* gamma, const float* mean, const float* var, float eps, int train, int relu,
                     int64_t M, int c, float* dx, int64_t lddx, float* dgamma, float* dbeta, float* scratch,
                     void* stream);
/* ------------------------------------------------------------------------------------------------
 * Graph LayerNorm (torch_geometric.nn.norm.LayerNorm, PyG 2.0.2, batch=None; surfaceNetStaticEdgeFilters.py:116-123 with
 * normalization 'l'): ONE mean and ONE biased std over all M*c elements, out = (x - m) / (std + eps) * weight + bias.
 * No running statistics (train = eval).  Deterministic fp64 reductions; the statistics stay on the device.
 * ---------------------------------------------------------------------------------------------- */
/* partial rows dgnn_graph_ln_stats writes (its `partials` hold 2 * that many doubles) */
int64_t dgnn_graph_ln_stats_blocks(int64_t M, int c);
/* floats of scratch for dgnn_graph_ln_relu_bwd and for the first stage of dgnn_graph_ln_finalize_fold */
int64_t dgnn_graph_ln_scratch_elems(int64_t M, int c);
/* standalone statistics pass over x [M, c]: partials[nblk][2] = (sum x, sum x^2) per block of rows, fp64 */
int dgnn_graph_ln_stats(const float* x, int64_t ldx, int64_t M, int c, double* partials, void* stream);
/* partials [nblk][2][pc] (pc = 1: dgnn_graph_ln_stats; pc = c: the colstats of dgnn_linear_fwd_x3_stats, nblk = ceil(M / 32)) ->
 * stats[4] = (m, sigma, r = 1 / (sigma + eps), M c) and scale[c] = w r, shift[c] = b - m w r (weight / bias NULL: 1 / 0).
 * scratch (8-byte aligned, >= 512 doubles) is used when there are many partial rows. */
int dgnn_graph_ln_finalize_fold(const double* partials, int64_t nblk, int pc, int64_t M, int c, const float* weight, const float* bias,
                                float eps, float* stats, float* scale, float* shift, double* scratch, void* stream);
/* y = act((x - m) * scale + bias): the apply centres first, as PyG does (in place allowed) */
int dgnn_graph_ln_apply(const float* x, int64_t ldx, int64_t M, int c, const float* stats, const float* scale, const float* bias, int relu,
                        float* y, int64_t ldy, void* stream);
/* backward of y = act(LayerNorm(x)) from the forward's stats / scale (the ReLU mask is recomputed from x, y is not read): dx (WRITTEN),
 * dweight = sum g xhat, dbias = sum g (NULL: not stored).  scratch: dgnn_graph_ln_scratch_elems(M, c) floats. */
int dgnn_graph_ln_relu_bwd(const float* x, int64_t ldx, const float* dy, int64_t lddy, const float* stats, const float* weight, const float* scale,
                           const float* bias, int relu, int64_t M, int c, float* dx, int64_t lddx, float* dweight, float* dbias, float* scratch,
                           void* stream);
/* out[c] (+)= sum over rows (bias gradients) */
/* dgnn_bn_relu_bwd in two halves, for batch statistics that span several ranks (a scene cut across GPUs; SURVEY 8e: the [2 C] all-reduce per layer):
 * _sums: sums[0..c) = sum g, sums[c..2c) = sum g * x_hat over the M local rows (g = dy behind the ReLU mask; also this rank's dbeta / dgamma terms);
 * _apply: dx from sums taken over `count` rows (all ranks').  fp32 rows; scratch as dgnn_bn_relu_bwd. */
int dgnn_bn_relu_bwd_sums(const float* x, int64_t ldx, const float* y, int64_t ldy, const float* dy, int64_t lddy, const float* mean,
                          const float* var, float eps, int relu, int64_t M, int c, float* sums, float* scratch, void* stream);
int dgnn_bn_relu_bwd_apply(const float* x, int64_t ldx, const float* y, int64_t ldy, const float* dy, int64_t lddy, const float* gamma,
                           const float* mean, const float* var, float eps, int relu, int64_t M, int c, const float* sums, double count,
                           float* dx, int64_t lddx, void* stream);
int dgnn_colsum(const float* x, int64_t ldx, int64_t M, int c, float* out, int accumulate, float* scratch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Aggregation backward (autograd of :75-80,:89-96, invoked at learning/runModel.py:279).
 * Runs over the TRANSPOSED plan (edges grouped by source) so dx_src needs no atomics:
 *   dm_e   = da[dst_e,:] / max(deg_dst,1)
 *   dphi_e = dm_e * x_src[s,:]          dx_src[s,:] = sum_e dm_e * phi_e
 *   fused mode (We != NULL): phi recomputed; dWe = sum_e dphi_e (x) edge_attr[e]; dbe = sum_e dphi_e
 *   given mode (phi != NULL): dphi written to dphi_out[e,:]
 *   t_rowptr/t_dst/t_eid : transposed plan (dgnn_plan_build with by=0); deg_dst from rowptr_dst.
 * dWe [c_in,f_e], dbe [c_in] are WRITTEN (no zero fill needed), summed deterministically via `partials`.
 * ---------------------------------------------------------------------------------------------- */
int64_t dgnn_sage_aggregate_bwd_scratch_elems(int64_t n_src, int c_in, int f_e);
int dgnn_sage_aggregate_bwd(const int32_t* t_rowptr, const int32_t* t_dst, const int32_t* t_eid, int64_t n_src,
                            const int32_t* rowptr_dst, const float* x_src, int64_t ldx, int c_in,
                            const float* edge_attr, int64_t lde, int f_e, const float* We, const float* be,
                            const float* phi, int64_t ldphi, const float* da, int64_t ldda, float* dx_src,
                            int64_t lddx, float* dWe, float* dbe, float* dphi_out, int64_t lddphi, float* partials,
                            void* stream);

/* bf16-storage form of dgnn_linear_wgrad_x3_cat (A, B1, B2 bf16, or fp32 rounded to bf16 when staged: a_f32 / b_f32 = 1): one bf16 product per
 * element, dW1 / dW2 bit-identical to dgnn_linear_wgrad_bf16; same scratch size function. */
int dgnn_linear_wgrad_bf16_cat(const void* A, int a_f32, int64_t lda, int n_a, const void* B1, int64_t ldb1, int n_b1, const void* B2, int64_t ldb2,
                               int n_b2, int b_f32, int64_t M, float* dW1, float* dW2, float* dbias, float* scratch, void* stream);

/* Given-phi form of the aggregate backward (the Updated variant, surfaceNetUpdatedEdgeFilters.py:147-170) with the two additions of its conv
 * layer's backward folded into the stores: dx_src[row] += add[row] for row < n_add (add NULL: none) and dphi_out[e] = dphi_e + dphi_ext[e]
 * (dphi_ext NULL: none; :233-241: the next layer takes this layer's phi as its edge input and sends a gradient back to it).  bf16 = 1: bf16
 * storage of x, phi, da, dx, add, dphi. */
int dgnn_sage_aggregate_bwd_phi_add(const int32_t* t_rowptr, const int32_t* t_dst, const int32_t* t_eid, int64_t n_src, const int32_t* rowptr_dst,
                                    const void* x_src, int64_t ldx, int c_in, const void* phi, int64_t ldphi, const void* da, int64_t ldda,
                                    void* dx_src, int64_t lddx, const void* add, int64_t ldadd, int64_t n_add, void* dphi_out, int64_t lddphi,
                                    const void* dphi_ext, int bf16, void* stream);
/* The same with the ReLU mask of the layer below folded into the dx store (mask_dx != 0): dx_src[row] = x_src[row] > 0 ? dx_src[row] : +0,
 * after the addend (x_src is relu(y_below); needs dx_src).  mask_dx = 0: dgnn_sage_aggregate_bwd_phi_add. */
int dgnn_sage_aggregate_bwd_phi_add_masked(const int32_t* t_rowptr, const int32_t* t_dst, const int32_t* t_eid, int64_t n_src,
                                           const int32_t* rowptr_dst, const void* x_src, int64_t ldx, int c_in, const void* phi, int64_t ldphi,
                                           const void* da, int64_t ldda, void* dx_src, int64_t lddx, const void* add, int64_t ldadd, int64_t n_add,
                                           void* dphi_out, int64_t lddphi, const void* dphi_ext, int bf16, int mask_dx, void* stream);

/* dgnn_sage_aggregate_bwd in fused mode (f_e = 20, fp32) with `dx_src[row] += add[row]` for row < n_add folded into the store of dx_src:
 * the x_dst = x[:n_dst] branch of a conv layer (:217, lin_i) sends its gradient dz . Wi to the first n_dst rows of dx; the addend is
 * added to the finished sum in one fp32 addition, like an accumulating GEMM epilogue after the aggregate would. */
int dgnn_sage_aggregate_bwd_add(const int32_t* t_rowptr, const int32_t* t_dst, const int32_t* t_eid, int64_t n_src,
                                const int32_t* rowptr_dst, const float* x_src, int64_t ldx, int c_in, const float* edge_attr,
                                int64_t lde, int f_e, const float* We, const float* be, const float* da, int64_t ldda, float* dx_src,
                                int64_t lddx, const float* add, int64_t ldadd, int64_t n_add, float* dWe, float* dbe, float* partials,
                                void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused inference layer (the timed path, surfaceNetStaticEdgeFilters.py:343-346, one call per
 * layer): aggregate + lin_j + lin_i + BN(eval) + ReLU in one persistent launch; the aggregate
 * never leaves the CU.  Requires c_in <= 128, c_out in {64,128}, f_e == 20 with packed rows.
 * Edge row of plan position k = edge_attr[eid ? eid[k] : k]: pass the plan's eid to read the
 * caller's edge_attr in place (each 80-byte row is DMA-gathered into LDS; no staging copy), or
 * eid == NULL with rows already in plan order (dgnn_gather_rows_f32).  Returns DGNN_E_UNSUPPORTED
 * for other shapes (callers fall back to the aggregate + linear pair above).
 * x_dst: own rows of the n_dst destinations (row stride ldx), the second element of the reference's
 * (x_src, x_dst) pair (:66-72); NULL = x_src (x_dst is x_src[:n_dst] at every reference call site).
 * A sub-range [b, b+n) of the destinations is one call with rowptr+b, x_dst = x_src + b*ldx, out + b*ldo
 * (the partitioned forward runs interior and boundary cells as two such launches).  gemm_mode selects how the dense part runs on the matrix cores.
 * ---------------------------------------------------------------------------------------------- */
#define DGNN_GEMM_F32 0    /* v_mfma_f32_32x32x2_f32: bit-faithful fp32 fmaf chains */
#define DGNN_GEMM_BF16X3 1 /* operands split exactly into 3 bf16 parts, 6 partial products on v_mfma_f32_32x32x16_bf16,
                              fp32 accumulate: fp32-class accuracy (dropped terms <= 2^-25 relative) at 6/16 of the time */
#define DGNN_GEMM_BF16X3_FILTER 2 /* as BF16X3, and the 20-tap filter MLP runs on v_mfma_f32_16x16x32_bf16 too (same exact
                                     3-part split, 6 products, fp32 accumulate); falls back to BF16X3 for shapes it
                                     does not cover (c_in not a multiple of c_in_pad/16, unaligned wide rows) */
#define DGNN_GEMM_F16X2_DENSE 3 /* dense product in the fp16 two-part form: every [mean | own] row of a tet and the [Wj | Wi] pair are multiplied
                                  by a power of two (exact) that puts their largest magnitude into [2^14, 2^15), split into (hi, lo) fp16
                                  parts (22 significand bits), 3 products hi.hi + hi.lo + lo.hi on v_mfma_f32_32x32x16_f16 with fp32
                                  accumulation (lo.lo dropped: <= 2^-22 relative -- the "3xTF32" scheme, TF32 and fp16 both carry 11
                                  significant bits), inverse scales applied to the accumulator; filter MLP as BF16X3_FILTER */
#define DGNN_GEMM_F16X2 4       /* (library default of the Python host) as F16X2_DENSE, and the filter MLP on v_mfma_f32_16x16x32_f16 in the
                                  same form: one scale per EDGE (its 20 attributes and the constant 1 of the bias column) and one for
                                  [We | be].  Half the matrix instructions and a third of the split instructions of BF16X3_FILTER; measured
                                  error against fp64 at the level of the other modes, also with rows / edges / weights spread over 60
                                  binades (tests/test_gpu_parity.py).  Falls back like BF16X3_FILTER.  The training entry points and
                                  dgnn_linear_*_x3 treat both F16X2 values as BF16X3; dgnn_linear_fwd_x2h is the GEMM in this form */
int dgnn_sage_layer_fused_fwd(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int64_t n_dst, const float* x_src,
                              const float* x_dst, int64_t ldx, int c_in, const float* edge_attr, int64_t lde, int f_e,
                              const float* We, const float* be, const float* Wj, const float* bj, const float* Wi,
                              const float* scale, const float* shift, int relu, int c_out, float* out, int64_t ldo,
                              int gemm_mode, void* stream);
/* 1: the 128 -> 128 layers in DGNN_GEMM_F16X2 (plain and decoder-carrying) run as the WAVE-SPECIALISED kernel (csrc/fused_ws.hip: workgroups of 8
 * producer wavefronts -- gather, filter MLP, mean, row split -- and 8 consumer wavefronts -- the dense product against register-resident weights, the
 * epilogue, the decoder -- around a ring of 32-tet tiles in LDS; same arithmetic form and error level as the two-phase kernel, not the same bits);
 * 0: the two-phase kernel of rounds 2-4 (environment DGNN_WS=0, read once per process).  What a benchmark line names its dominant kernel by.
 * The same kernel takes the 64 -> 128 layer (DGNN_WS_64=0: not) and, in the bf16-storage chain, the plain 64 -> 128 and 128 -> 128 layers on UNSIGNED
 * 16-bit rows (dgnn_sage_layer_fused_fwd_bf16 with DGNN_BF16_COMPENSATED | _ROWS_IN_UNSIGNED | _ROWS_OUT_UNSIGNED; DGNN_WS_16=0: not): rows decoded
 * exactly, the fp16 two-part arithmetic of the fp32-I/O kernel in between (tighter than the compensated bf16 products), rows encoded in the epilogue. */
int dgnn_wave_specialised_enabled(void);

/* The LAST conv layer + BatchNorm(eval) + ReLU of SurfaceNet.inference_layer (learning/surfaceNetStaticEdgeFilters.py:343-347) together with the
 * decoder Linear(c_out -> c_hidden) - BatchNorm(eval, folded into scale1 / shift1, NULL = none) - ReLU - Linear(c_hidden -> n_logits)
 * (:180-187, applied :350-351) in ONE launch: a finished tile of 32 tets stays in the compute unit, goes through the decoder there and
 * only logits [n_dst, n_logits] (row stride n_logits) are written -- 8 bytes per tet instead of 512 out and 512 back in.
 * Layer arguments as dgnn_sage_layer_fused_fwd.  Covers the shipped shape: 64 < c_in <= 128 (c_in % 8 == 0), c_out = 128, f_e = 20 (packed rows),
 * c_hidden = 64, n_logits = 2, rows 16-byte aligned; arithmetic = DGNN_GEMM_F16X2 throughout (the decoder's first product: one power-of-two
 * scale per tet row and 16-column slab, applied to the fp32 sum).  Any other shape: DGNN_E_UNSUPPORTED, nothing launched -- the caller then
 * runs dgnn_sage_layer_fused_fwd and dgnn_decoder_fused_fwd.  A tet's logits depend on its own inputs only (destination sub-ranges of a
 * partitioned scene give bit-identical results). */
int dgnn_sage_layer_fused_decoder_fwd(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int64_t n_dst, const float* x_src,
                                      const float* x_dst, int64_t ldx, int c_in, const float* edge_attr, int64_t lde, int f_e,
                                      const float* We, const float* be, const float* Wj, const float* bj, const float* Wi,
                                      const float* scale, const float* shift, int relu, int c_out, const float* W0, const float* b0,
                                      const float* scale1, const float* shift1, int c_hidden, const float* W3, const float* b3, int n_logits,
                                      float* logits, void* stream);

/* Prepared parameters of the fused layers (fp16 two-part arithmetic, DGNN_GEMM_F16X2).  What a fused launch derives from the layer's parameters
 * before its first tile -- two power-of-two scales, the split filter operand [We | be], every wavefront's resident fragments of [Wj | Wi], the
 * decoder's W0 fragments and folded constants -- costs each of the 256 workgroups a column-wise read of the weights and their split: 15-20 us per
 * launch.  dgnn_sage_layer_prepare runs that prologue once and parks the result in `prepared` (dgnn_sage_layer_prepared_bytes(c_in, c_out,
 * with_decoder) bytes, 16-byte aligned; 0 = shape not covered); dgnn_sage_layer_fused_fwd_p / dgnn_sage_layer_fused_decoder_fwd_p are the two
 * entry points above reading it back (coalesced 16-byte loads).  The values are the same: results are bit-identical to the unprepared calls.
 * The buffer belongs to the parameter VALUES it was made from (W0 .. b3: the decoder's, NULL for a plain layer); prepare again when they change.
 * BatchNorm(eval) scale / shift and bj are still passed per call.  Shapes outside the all-matrix-core kernel: DGNN_E_UNSUPPORTED. */
int64_t dgnn_sage_layer_prepared_bytes(int c_in, int c_out, int with_decoder);
int dgnn_sage_layer_prepare(int c_in, int c_out, const float* We, const float* be, const float* Wj, const float* Wi, const float* W0,
                            const float* b0, const float* scale1, const float* shift1, const float* W3, const float* b3, void* prepared,
                            void* stream);
int dgnn_sage_layer_fused_fwd_p(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int64_t n_dst, const float* x_src,
                                const float* x_dst, int64_t ldx, int c_in, const float* edge_attr, int64_t lde, int f_e, const float* We,
                                const float* be, const float* Wj, const float* bj, const float* Wi, const float* scale, const float* shift,
                                int relu, int c_out, float* out, int64_t ldo, const void* prepared, void* stream);
int dgnn_sage_layer_fused_decoder_fwd_p(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int64_t n_dst, const float* x_src,
                                        const float* x_dst, int64_t ldx, int c_in, const float* edge_attr, int64_t lde, int f_e,
                                        const float* We, const float* be, const float* Wj, const float* bj, const float* Wi,
                                        const float* scale, const float* shift, int relu, int c_out, const float* W0, const float* b0,
                                        const float* scale1, const float* shift1, int c_hidden, const float* W3, const float* b3, int n_logits,
                                        float* logits, const void* prepared, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Whole-scene inference, ONE call (SurfaceNet.inference_layer, learning/surfaceNetStaticEdgeFilters.py:323-355: every conv -> norm -> relu
 * over the whole graph, then the decoder :350-351).
 *   plan     edge_index != NULL: the destination-sorted plan of the scene is built first (dgnn_plan_build with `plan_hint`) INTO the caller's
 *            rowptr [n+1] / src [E] / eid [E] / plan_scratch [dgnn_plan_scratch_elems(E, n)] -- they stay valid for later calls on the same
 *            graph; edge_index == NULL: rowptr / src / eid ARE the plan (eid NULL = edge_attr already in plan order).  edge_attr rows follow
 *            edge_index and are gathered through eid inside the layer launches.
 *   layers   n_layers fused conv layers (dgnn_sage_layer_fused_fwd[_p]; BatchNorm(eval) folded into scale[l] / shift[l], NULL = none; ReLU)
 *   decoder  Linear(widths[L] -> c_hidden) - BatchNorm(eval, scale1 / shift1) - ReLU - Linear(-> n_logits): fuse_decoder != 0 -- inside the last
 *            layer's launch where its shape allows (dgnn_sage_layer_fused_decoder_fwd[_p]; prepared[L-1], if given, must then have been made
 *            WITH the decoder); otherwise dgnn_decoder_fused_fwd behind a plain last layer (prepared[L-1] a plain layer's).  W0 == NULL: no
 *            decoder, `logits` receives the last layer's rows [n, widths[L]]
 * Per-layer arguments are HOST arrays [n_layers] of device pointers (widths [n_layers + 1]); prepared (may be NULL, entries may be NULL):
 * dgnn_sage_layer_prepare buffers, the last one made WITH the decoder.  Issues exactly the launches of the per-layer entry points, in their
 * order: bit-identical results; nothing allocates or synchronises.  Shapes outside the fused kernels (see dgnn_sage_layer_fused_fwd):
 * DGNN_E_UNSUPPORTED before anything is launched.  workspace: dgnn_static_infer_workspace_bytes(n, n_layers, widths) bytes, 16-byte aligned.
 * ---------------------------------------------------------------------------------------------- */
int64_t dgnn_static_infer_workspace_bytes(int64_t n, int n_layers, const int32_t* widths);
int dgnn_static_infer_fwd(const int64_t* edge_index, int64_t stride_row, int64_t stride_col, int64_t E, int plan_hint, int32_t* rowptr,
                          int32_t* src, int32_t* eid, int32_t* plan_scratch, int64_t n, const float* x, int64_t ldx, const float* edge_attr,
                          int64_t lde, int f_e, int n_layers, const int32_t* widths, const float* const* We, const float* const* be,
                          const float* const* Wj, const float* const* bj, const float* const* Wi, const float* const* scale,
                          const float* const* shift, const void* const* prepared, const float* W0, const float* b0, const float* scale1,
                          const float* shift1, int c_hidden, const float* W3, const float* b3, int n_logits, int fuse_decoder, int gemm_mode,
                          void* workspace, float* logits, void* stream);

/* ------------------------------------------------------------------------------------------------
 * One rank's part of a scene cut across GPUs, ONE call per step and NO data-path exchange.  Behind its owned cells the part holds the
 * rings of cells 1 .. L hops away (L = n_layers; their input rows are static and resident), and layer l is computed for the owned cells and the
 * rings up to L-1-l hops out -- the reference's own k-hop recomputation (learning/surfaceNetStaticEdgeFilters.py:232-275, one sampled batch at a
 * time) applied to a whole part.  Local cell order: owned cells, ring 1, ring 2, ...; the local edge list holds the in-edges of every cell that some
 * layer computes (owned + rings 1 .. L-1), sources < n_loc.
 *   n_dst [n_layers]  destinations of layer l = the first n_dst[l] local cells (non-increasing; n_dst[L-1] = the owned cells = rows of `logits`);
 *                     the plan (built when edge_index != NULL) covers n_dst[0] destinations, n_loc = all local cells incl. the outermost ring
 *   attr_in_plan_order != 0: edge_attr rows are grouped by destination already (a part's local list is): read in place, not through eid
 * Everything else as dgnn_static_infer_fwd (which is this call with every n_dst[l] = n).  On a reference-layout scene (4 in-edges per cell) a cell's
 * result does not depend on which other cells share its launch: the union of the ranks' logits is bit-identical to the whole scene's (a ragged graph:
 * equal to fp32 rounding).  workspace: dgnn_static_infer_workspace_bytes(n_dst[0], ...).
 * ---------------------------------------------------------------------------------------------- */
int dgnn_static_infer_rings_fwd(const int64_t* edge_index, int64_t stride_row, int64_t stride_col, int64_t E, int plan_hint, int32_t* rowptr,
                                int32_t* src, int32_t* eid, int32_t* plan_scratch, int attr_in_plan_order, int64_t n_loc, const int64_t* n_dst,
                                const float* x, int64_t ldx, const float* edge_attr, int64_t lde, int f_e, int n_layers, const int32_t* widths,
                                const float* const* We, const float* const* be, const float* const* Wj, const float* const* bj,
                                const float* const* Wi, const float* const* scale, const float* const* shift, const void* const* prepared,
                                const float* W0, const float* b0, const float* scale1, const float* shift1, int c_hidden, const float* W3,
                                const float* b3, int n_logits, int fuse_decoder, int gemm_mode, void* workspace, float* logits, void* stream);

/* The same in bf16 STORAGE (BASELINE config 3; whole scene: every n_dst[l] = n_loc): layer 0 reads the caller's fp32 rows in place (widths[0] <= 32) and
 * starts the 16-bit rows -- unsigned when `mode` carries DGNN_BF16_ROWS_OUT_UNSIGNED --, the middle layers keep the format, the last layer's launch
 * carries the decoder (dgnn_sage_layer_fused_decoder_fwd_bf16) and writes fp32 logits.  mode = DGNN_BF16_COMPENSATED [| DGNN_BF16_ROWS_OUT_UNSIGNED];
 * the decoder is required (128 -> 64 -> 2 behind a 128-wide last layer).  Anything else: DGNN_E_UNSUPPORTED, nothing launched.  Bit-identical to the
 * per-layer bf16 entry points.  workspace as dgnn_static_infer_rings_fwd. */
int dgnn_static_infer_rings_fwd_bf16(const int64_t* edge_index, int64_t stride_row, int64_t stride_col, int64_t E, int plan_hint, int32_t* rowptr,
                                     int32_t* src, int32_t* eid, int32_t* plan_scratch, int attr_in_plan_order, int64_t n_loc, const int64_t* n_dst,
                                     const float* x, int64_t ldx, const float* edge_attr, int64_t lde, int f_e, int n_layers, const int32_t* widths,
                                     const float* const* We, const float* const* be, const float* const* Wj, const float* const* bj,
                                     const float* const* Wi, const float* const* scale, const float* const* shift, const float* W0, const float* b0,
                                     const float* scale1, const float* shift1, int c_hidden, const float* W3, const float* b3, int n_logits, int mode,
                                     void* workspace, float* logits, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training-mode conv layer, one call each way (SurfaceNet.forward :214-219 and its autograd, learning/runModel.py:279):
 *   forward : a = aggregate(x)  ->  z = a.Wj^T + x[:n_dst].Wi^T + bj  ->  BatchNorm1d with batch statistics (running buffers
 *             updated when given)  ->  y = relu(.)       rowptr == NULL: a plain Linear + BatchNorm (+ReLU) block, z = x.Wj^T + bj
 *   backward: dy -> dx (NULL: x is data), dWe, dbe, dWj, dbj (NULL: no bias), dWi, dgamma, dbeta
 * Both issue the launch chain of the separate entry points above, in the same order, on `stream` (results are bit-identical
 * to calling them one by one); nothing allocates or synchronises.  Buffers: a [n_dst,c_in], z / y [n_dst,c_out], mean / var /
 * scale / shift [c_out]; forward scratch = dgnn_colstats_scratch_elems(n_dst, c_out) floats, backward scratch =
 * dgnn_sage_layer_train_scratch_elems floats.  Transposed plan (t_*) and rowptr_dst as dgnn_sage_aggregate_bwd.
 * ---------------------------------------------------------------------------------------------- */
int64_t dgnn_sage_layer_train_scratch_elems(int64_t n_src, int64_t n_dst, int c_in, int c_out, int f_e);
int dgnn_sage_layer_train_fwd(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int64_t n_dst, const float* x, int64_t ldx,
                              int c_in, const float* edge_attr, int64_t lde, int f_e, const float* We, const float* be, const float* Wj,
                              const float* bj, const float* Wi, int c_out, const float* gamma, const float* beta, float* running_mean,
                              float* running_var, float momentum, float eps, int relu, float* a, float* z, float* mean, float* var,
                              float* scale, float* shift, float* y, float* scratch, int gemm_mode, void* stream);
int dgnn_sage_layer_train_bwd(const int32_t* t_rowptr, const int32_t* t_dst, const int32_t* t_eid, const int32_t* rowptr_dst,
                              int64_t n_src, int64_t n_dst, const float* x, int64_t ldx, int c_in, const float* edge_attr, int64_t lde,
                              int f_e, const float* We, const float* be, const float* Wj, const float* Wi, int c_out, const float* gamma,
                              const float* mean, const float* var, float eps, int relu, const float* a, const float* z, const float* y,
                              const float* dy, float* dx, float* dWe, float* dbe, float* dWj, float* dbj, float* dWi, float* dgamma,
                              float* dbeta, float* scratch, int gemm_mode, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Edge-embedding chaining of the Updated variant (surfaceNetUpdatedEdgeFilters.py:233-241): the next layer's edge rows
 *   out[k, :c] = relu?( phi[r, :c] )  where e_id_cur[r] == e_id_next[k],   0 when this layer did not produce that edge
 * i.e. relu(zeros[E_all, C]; [e_id_cur] = phi)[e_id_next, :c] without materialising the [E_all, C] tensor.  `pos` is an
 * [n_edges] int32 table that must hold -1 everywhere on entry and does again on exit (only e_id_cur entries are touched);
 * `inv` [n_cur] receives the inverse map (row of `out` that read phi row r, or -1) for the backward pass:
 *   dphi[r, j] = (inv[r] >= 0 && j < c) ? g[inv[r], j] * [phi[r, j] > 0] : 0        (dphi [n_cur, c_tot], fully written)
 * Edge ids are unique within a block (k-hop blocks: every graph edge appears once).  Ids outside [0, n_edges) are skipped
 * and reported through dgnn_poll_async_error.
 * ---------------------------------------------------------------------------------------------- */
int dgnn_edge_chain_fwd(const float* phi, int64_t ldphi, int c, const int64_t* e_id_cur, int64_t n_cur, const int64_t* e_id_next,
                        int64_t n_next, int64_t n_edges, int32_t* pos, int relu, float* out, int64_t ldo, int32_t* inv, void* stream);
int dgnn_edge_chain_fwd_bf16(const uint16_t* phi, int64_t ldphi, int c, const int64_t* e_id_cur, int64_t n_cur, const int64_t* e_id_next,
                             int64_t n_next, int64_t n_edges, int32_t* pos, int relu, uint16_t* out, int64_t ldo, int32_t* inv, void* stream);
int dgnn_edge_chain_bwd(const float* g, int64_t ldg, const float* phi, int64_t ldphi, const int32_t* inv, int64_t n_cur, int c, int c_tot,
                        int relu, float* dphi, int64_t lddphi, void* stream);
int dgnn_edge_chain_bwd_bf16(const uint16_t* g, int64_t ldg, const uint16_t* phi, int64_t ldphi, const int32_t* inv, int64_t n_cur, int c,
                             int c_tot, int relu, uint16_t* dphi, int64_t lddphi, void* stream);

/* dgnn_sage_layer_train_fwd / _bwd with bf16 STORAGE: x / a / z / y / dy / dx (and the work buffers dz [n_dst,c_out], da [n_dst,c_in]) are bf16
 * bit patterns, parameters, statistics and parameter gradients fp32; the chain of the *_bf16 entry points.  Scratch (floats) as for the
 * fp32 functions. */
int dgnn_sage_layer_train_fwd_bf16(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int64_t n_dst, const uint16_t* x, int64_t ldx,
                                   int c_in, const float* edge_attr, int64_t lde, int f_e, const float* We, const float* be, const float* Wj,
                                   const float* bj, const float* Wi, int c_out, const float* gamma, const float* beta, float* running_mean,
                                   float* running_var, float momentum, float eps, int relu, uint16_t* a, uint16_t* z, float* mean, float* var,
                                   float* scale, float* shift, uint16_t* y, float* scratch, void* stream);
int dgnn_sage_layer_train_bwd_bf16(const int32_t* t_rowptr, const int32_t* t_dst, const int32_t* t_eid, const int32_t* rowptr_dst, int64_t n_src,
                                   int64_t n_dst, const uint16_t* x, int64_t ldx, int c_in, const float* edge_attr, int64_t lde, int f_e,
                                   const float* We, const float* be, const float* Wj, const float* Wi, int c_out, const float* gamma,
                                   const float* mean, const float* var, float eps, int relu, const uint16_t* a, const uint16_t* z,
                                   const uint16_t* y, const uint16_t* dy, uint16_t* dx, float* dWe, float* dbe, float* dWj, float* dbj,
                                   float* dWi, float* dgamma, float* dbeta, uint16_t* dz, uint16_t* da, float* scratch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Static model in training mode, ALL layers per call (SurfaceNet.forward :196-227 up to the decoder's last Linear, and its
 * autograd): the chain of dgnn_sage_layer_train_fwd / _bwd calls issued from one entry point each way.  Per-layer arguments are
 * HOST arrays [n_layers] of device pointers / sizes (widths [n_layers+1]); rowptr[l] == NULL marks a plain Linear + BatchNorm +
 * ReLU block (the decoder's).  Layer l reads y[l-1] (layer 0: x0); stats[l] = [4, widths[l+1]] (mean, var, scale, shift).
 * Forward scratch: max_l dgnn_colstats_scratch_elems(n_dst[l], widths[l+1]); backward scratch: dgnn_static_train_scratch_elems
 * (host arrays); dx_buf[0..1]: max_l n_src[l] * widths[l] floats each.  Everything runs on `stream`.
 * num_batches_tracked (may be NULL): device int64 counters of the BatchNorm modules, incremented once.
 * ---------------------------------------------------------------------------------------------- */
int dgnn_static_train_fwd(int n_layers, const int32_t* const* rowptr, const int32_t* const* src, const int32_t* const* eid, const int64_t* n_dst,
                          const float* x0, int64_t ldx0, const int32_t* widths, const float* const* edge_attr, const int64_t* lde, int f_e,
                          const float* const* We, const float* const* be, const float* const* Wj, const float* const* bj, const float* const* Wi,
                          const float* const* gamma, const float* const* beta, float* const* running_mean, float* const* running_var,
                          int64_t* const* num_batches_tracked, const float* momentum, const float* eps, float* const* a, float* const* z,
                          float* const* stats, float* const* y, float* scratch, int gemm_mode, void* stream);
/* The training step's fused launch chains: bit 0 = backward (dgnn_linear_wgrad_x3_cat, the stacked input-gradient GEMM with
 * dgnn_sage_aggregate_bwd_add, one transpose launch per pass), bit 1 = BatchNorm statistics from the forward GEMM's epilogue
 * (dgnn_linear_fwd_x3_stats).  Default 3 (environment: DGNN_TRAIN_FUSED=<mask>); 0 = the launch chain of the separate entry points.
 * Returns the previous mask. */
int dgnn_train_set_fused(int mask);

/* One Adam step over n_tensors fp32 parameter tensors in one launch (reference learning/runModel.py:290 torch.optim.Adam(model.parameters(), lr),
 * stepped at :282; no amsgrad / weight decay): p, g, m (exp_avg), v (exp_avg_sq) are host arrays of device pointers, numel the element counts,
 * step the 1-based step count (bias corrections are computed on the host in double precision). */
int dgnn_adam_step(int n_tensors, float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* numel, float lr,
                   float beta1, float beta2, float eps, int64_t step, void* stream);

/* All conv layers of the Updated variant (learning/surfaceNetUpdatedEdgeFilters.py:229-243) and the edge chaining between them per call: the
 * per-layer composite calls (dgnn_sage_updated_train_fwd / _bwd) and dgnn_edge_chain_fwd / _bwd issued back to back, results bit-identical to
 * calling them one by one.  Per layer l: plan (rowptr, src, eid), e_id[l] = the block edges' rows in the scene's edge tensor (int64; rows0 = e_id[0]
 * as int32), n_dst, E; widths[0 .. n_layers], edge_in[l] = columns of the layer's edge input (layer 0: of edge_attr_all, layer l: of phi_{l-1});
 * pos: the int32 [E_all] table of dgnn_edge_chain_fwd (all -1 between calls); relu[l]: the ReLU that follows conv l.  Saved for the backward:
 * ea[l] [E_l, ld_ea[l]], phi[l] [E_l, widths[l]], a[l] [n_dst_l, widths[l]], y[l] [n_dst_l, widths[l+1]], inv[l] [E_{l-1}] (l >= 1).
 * bf16 = 1: bf16 storage of x0 and of every saved tensor (ea0_f32: an [E_0, edge_in_0] fp32 work buffer for the cast).  Work buffers of the backward
 * (storage type): dx_buf[0 / 1] [max_l>=1 n_src_l * widths[l]], d_ea [max_l>=1 E_l * edge_in_l], dphi_ext and dphi [max_l E_l * widths[l]],
 * dz [max n_dst_l * widths[l+1]], da [max 2 * n_dst_l * widths[l]]; scratch: the largest dgnn_sage_updated_train_scratch_elems of the layers. */
int dgnn_updated_stack_fwd(int n_layers, const int32_t* const* rowptr, const int32_t* const* src, const int32_t* const* eid, const int64_t* const* e_id,
                           const int32_t* rows0, const int64_t* n_dst, const int64_t* E, const void* x0, int64_t ldx0, const int32_t* widths,
                           const int32_t* edge_in, const float* edge_attr_all, int64_t lde_all, int64_t E_all, int32_t* pos, const float* const* We,
                           const float* const* be, const float* const* Wl, const float* const* bl, const float* const* Wr, const int32_t* relu,
                           void* const* ea, const int64_t* ld_ea, float* ea0_f32, void* const* phi, void* const* a, void* const* y, int32_t* const* inv,
                           int bf16, int gemm_mode, void* stream);
int dgnn_updated_stack_bwd(int n_layers, const int32_t* const* t_rowptr, const int32_t* const* t_dst, const int32_t* const* t_eid,
                           const int32_t* const* rowptr_dst, const int64_t* n_src, const int64_t* n_dst, const int64_t* E, const void* x0, int64_t ldx0,
                           const int32_t* widths, const int32_t* edge_in, const float* const* We, const float* const* Wl, const float* const* Wr,
                           const int32_t* relu, const void* const* ea, const int64_t* ld_ea, const void* const* phi, const void* const* a,
                           const void* const* y, const int32_t* const* inv, const void* dy, float* const* dWe, float* const* dbe, float* const* dWl,
                           float* const* dbl, float* const* dWr, void* const* dx_buf, void* d_ea, void* dphi_ext, void* dz, void* da, void* dphi,
                           float* scratch, int bf16, int gemm_mode, void* stream);
/* The Updated model's output network behind the conv stack ("sage+": out_net, surfaceNetUpdatedEdgeFilters.py:210, 245-247), one call each way:
 * h = relu(x . W1^T + b1) in the storage type, logits = h . W3^T + b3 in fp32.  Backward from g = d logits: dW3 / db3 and dW1 / db1 (one launch
 * pair each), dx [n, c] in the storage type.  dh: an [n, hdim] work buffer (storage type); scratch: dgnn_updated_tail_scratch_elems floats. */
int dgnn_updated_tail_fwd(int64_t n, const void* x, int64_t ldx, int c, const float* W1, const float* b1, int hdim, const float* W3, const float* b3,
                          int n_out, void* h, float* logits, int bf16, int gemm_mode, void* stream);
int64_t dgnn_updated_tail_scratch_elems(int64_t n, int c, int hdim, int n_out);
int dgnn_updated_tail_bwd(int64_t n, const void* x, int64_t ldx, int c, const float* W1, int hdim, const float* W3, int n_out, const void* h,
                          const float* g, float* dW1, float* db1, float* dW3, float* db3, void* dx, void* dh, float* scratch, int bf16,
                          int gemm_mode, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Updated variant, whole-scene inference (csrc/updated_infer.hip).  On a whole graph every layer's e_id is the identity and the reference's edge
 * chaining is ea_{l+1} = relu(phi_l)[:, :edge_in_{l+1}].
 *
 * dgnn_edge_chain_aggregate_fwd: lin_e, the mean aggregate and the next layer's edge rows of ONE conv layer in one launch, fp32 rows:
 *   phi = ea[eid[k], :k_e] . We^T + be per plan position k (never stored), a [n_dst, c_in] = mean over each destination's segment of x[src[k]] * phi
 *   (plan order, from 0, / max(deg, 1); any in-degree, 0 included), ea_next[eid[k]] = relu(phi) (row stride ldn >= c_in; write_next = 0: nothing is
 *   stored per edge and ea_next may be NULL).  eid NULL: the identity.  The filter product follows gemm_mode as the GEMM entry points do: DGNN_GEMM_F32 =
 *   per (edge, channel) the fmaf chain over ascending k that starts at the bias; any other mode = the bits of dgnn_linear_fwd_x3.
 *   c_in in {64, 128}, k_e <= 128 (dgnn_edge_chain_aggregate_supported), x / a / ea_next rows 16-byte aligned with strides % 4 == 0; anything else:
 *   DGNN_E_UNSUPPORTED, nothing launched.  A workgroup walks 16 destinations' plan positions in tiles of 64.
 *
 * dgnn_updated_infer_fwd: every conv layer of a scene on ONE plan (n sources = n destinations) and the "sage+" output network, one call.  Layer l maps
 *   widths[l] -> widths[l + 1] channels and reads edge_in[l] edge columns: of edge_attr (fp32 [E, >= edge_in[0]], scene edge order) for l = 0, of
 *   relu(phi_{l-1}) behind it.  A layer the launch above takes runs through it and dgnn_linear_fwd / _x3; any other (layer 0, widths >= 256, bf16 = 1:
 *   x and every intermediate in bf16) through dgnn_sage_updated_train_fwd with the ReLU applied in place.  ea_buf0 / ea_buf1: two [E, max_l widths[l]]
 *   edge buffers of the storage type, 16-byte aligned; workspace: dgnn_updated_infer_workspace_bytes bytes, 16-byte aligned.  relu[l]: the ReLU behind
 *   conv l.  W1 NULL: no output network and `out` receives the last layer's rows [n, widths[n_layers]] in the storage type; else (W1 [hdim, widths[L]],
 *   W3 [n_out, hdim]) fp32 logits [n, n_out] as dgnn_updated_tail_fwd writes them.  fused_layers (host memory, may be NULL): bit l is set when
 *   layer l ran through dgnn_edge_chain_aggregate_fwd.  Nothing allocates or synchronises.
 * ---------------------------------------------------------------------------------------------- */
int dgnn_edge_chain_aggregate_supported(int c_in, int k_e, int bf16, int gemm_mode);
int dgnn_edge_chain_aggregate_fwd(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int64_t n_dst, const float* x, int64_t ldx, int c_in,
                                  const float* ea, int64_t lde, int k_e, const float* We, const float* be, float* a, int64_t lda, float* ea_next,
                                  int64_t ldn, int write_next, int gemm_mode, void* stream);
int64_t dgnn_updated_infer_workspace_bytes(int64_t n, int64_t E, int n_layers, const int32_t* widths, const int32_t* edge_in, int hdim, int bf16);
int dgnn_updated_infer_fwd(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int64_t n, int64_t E, const void* x, int64_t ldx,
                           const float* edge_attr, int64_t lde, int n_layers, const int32_t* widths, const int32_t* edge_in, const float* const* We,
                           const float* const* be, const float* const* Wl, const float* const* bl, const float* const* Wr, const int32_t* relu,
                           const float* W1, const float* b1, int hdim, const float* W3, const float* b3, int n_out, void* ea_buf0, void* ea_buf1,
                           void* workspace, void* out, int32_t* fused_layers, int bf16, int gemm_mode, void* stream);

int64_t dgnn_static_train_scratch_elems(int n_layers, const int64_t* n_src, const int64_t* n_dst, const int32_t* widths, int f_e);
int dgnn_static_train_bwd(int n_layers, const int32_t* const* t_rowptr, const int32_t* const* t_dst, const int32_t* const* t_eid,
                          const int32_t* const* rowptr_dst, const int64_t* n_src, const int64_t* n_dst, const float* x0, int64_t ldx0,
                          const int32_t* widths, const float* const* edge_attr, const int64_t* lde, int f_e, const float* const* We,
                          const float* const* be, const float* const* Wj, const float* const* Wi, const float* const* gamma,
                          const float* const* stats, const float* eps, const float* const* a, const float* const* z, const float* const* y,
                          const float* dy, float* const* dWe, float* const* dbe, float* const* dWj, float* const* dbj, float* const* dWi,
                          float* const* dgamma, float* const* dbeta, float* const* dx_buf, float* scratch, int gemm_mode, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Updated variant, one conv layer per call each way (surfaceNetUpdatedEdgeFilters.py:147-170 and its autograd); `bf16` != 0:
 * x / ea / phi / a / y / dy and the gradients of activations are bf16 (uint16_t), parameters and their gradients fp32.
 *   forward : phi [E,c_in] = ea.We^T + be;  a [n_dst,c_in] = mean_j x_j * phi;  y [n_dst,c_out] = relu?(a.Wl^T + x[:n_dst].Wr^T + bl)
 *   backward: dy (+ dphi_ext [E,c_in], the gradient reaching phi through the next layer's edge input, or NULL) ->
 *             dx [n_src,c_in] (NULL: not needed), d_ea [E,k_e] (NULL: not needed), dWe, dbe, dWl, dbl (NULL: no bias), dWr;
 *             dz [n_dst,c_out] (relu only), da [n_dst,c_in], dphi [E,c_in] are work buffers of the activations' type,
 *             scratch = dgnn_sage_updated_train_scratch_elems floats.  Plans as dgnn_sage_aggregate_fwd / _bwd.
 * The launch chain of the separate entry points in the same order; nothing allocates or synchronises.
 * ---------------------------------------------------------------------------------------------- */
int64_t dgnn_sage_updated_train_scratch_elems(int64_t n_dst, int64_t E, int c_in, int c_out, int k_e);
int dgnn_sage_updated_train_fwd(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int64_t n_dst, const void* x, int64_t ldx, int c_in,
                                const void* ea, int64_t lde, int k_e, int64_t E, const float* We, const float* be, const float* Wl,
                                const float* bl, const float* Wr, int c_out, int relu, void* phi, void* a, void* y, int bf16, int gemm_mode,
                                void* stream);
int dgnn_sage_updated_train_bwd(const int32_t* t_rowptr, const int32_t* t_dst, const int32_t* t_eid, const int32_t* rowptr_dst, int64_t n_src,
                                int64_t n_dst, int64_t E, const void* x, int64_t ldx, int c_in, const void* ea, int64_t lde, int k_e,
                                const float* We, const float* Wl, const float* Wr, int c_out, int relu, const void* phi, const void* a,
                                const void* y, const void* dy, const void* dphi_ext, void* dx, void* d_ea, float* dWe, float* dbe, float* dWl,
                                float* dbl, float* dWr, void* dz, void* da, void* dphi, float* scratch, int bf16, int gemm_mode, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Volume-weighted KL cell loss of the training step (learning/runModel.py:171-209), one launch each way:
 *   cell_k = sum_c kl_div(log_softmax(logits_k)_c, gt_kc);  w_k = vol_k | log(1+vol_k) | sqrt(vol_k)  (norm 0 | 1 | 2)
 *   loss = sum cell_k w_k / sum w_k;   sums[3] (fp64) = sum cell_k w_k, sum w_k, #{k: [gt_k0 > gt_k1] == argmax log_softmax(logits_k), fp32, first index on a tie}
 *   backward: dlogits_kc = grad_loss * w_k / sums[1] * (softmax_kc (gt_k0 + gt_k1) - gt_kc)
 * logits / gt: two leading columns of rows with strides ldl / ldg; vol: element stride ldv.  scratch:
 * dgnn_kl_cell_loss_scratch_doubles(n) doubles.  grad_loss: device pointer to the upstream scalar.
 * ---------------------------------------------------------------------------------------------- */
int64_t dgnn_kl_cell_loss_scratch_doubles(int64_t n);
int dgnn_kl_cell_loss_fwd(const float* logits, int64_t ldl, const float* gt, int64_t ldg, const float* vol, int64_t ldv, int norm, int64_t n,
                          double* sums, float* loss, double* scratch, void* stream);
int dgnn_kl_cell_loss_bwd(const float* logits, int64_t ldl, const float* gt, int64_t ldg, const float* vol, int64_t ldv, int norm, int64_t n,
                          const double* sums, const float* grad_loss, float* dlogits, int64_t ldd, void* stream);
/* forward + (running += sums) + backward of one batch as ONE launch (round 6; the step around learning/runModel.py:171-209 and its gradient, with the
 * metric sums of :48-80 accumulated on the device): the same bits as dgnn_kl_cell_loss_fwd followed by dgnn_kl_cell_loss_bwd.  grad_loss NULL = 1;
 * running (fp64 [3]) and dlogits may be NULL.  DGNN_E_UNSUPPORTED (nothing launched) for n > 65536: use the two entry points above. */
int dgnn_kl_cell_loss_step(const float* logits, int64_t ldl, const float* gt, int64_t ldg, const float* vol, int64_t ldv, int norm, int64_t n,
                           const float* grad_loss, double* sums, float* loss, double* running, float* dlogits, int64_t ldd, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Edge total-variation regulariser of the training objective (learning/runModel.py:109-160, :250-256), csrc/edge_tv.hip:
 *   p(v) = softmax(logits_v)_0;  tv_e = |p(src_e) - p(dst_e)|;  reg = weight * sum_e tv_e / E;  sums[2] (fp64) = weight * sum_e tv_e, E
 *   backward: dlogits_v = grad * (weight / E) * c(v) * p(v) (1 - p(v)) * (+1, -1),  c(v) = sum_{src_e = v} sgn_e - sum_{dst_e = v} sgn_e,
 *   sgn_e = sign(p(src_e) - p(dst_e)) with sign(0) = 0.  c(v) is accumulated in `net` (int32 [n]) with integer atomics and the sum of tv in fp64
 *   in a fixed order: results do not depend on the order of the edges' arrival, reruns are bit-identical.
 * logits: n rows of two leading columns, row stride ldl.  src / dst: E indices in [0, n) each, element stride estride, int64 (idx64 != 0) or int32,
 * any alignment of their type (16-byte aligned rows of stride 1, and the (src, dst) pairs of a transposed [E, 2] array, are read 16 bytes a load);
 * any other layout -- a contiguous [2, E] tensor whose second row is not 16-byte aligned, i.e. E odd (int64) or E % 4 != 0 (int32), included -- is
 * read one index a load, four loads of each row in flight); an index outside [0, n) is skipped and reported by dgnn_poll_async_error.  scratch:
 * dgnn_edge_tv_scratch_doubles() doubles.  max_blocks: 0, or a cap on the edge pass's workgroups (each call of a fwd / step pair the same).
 *   _fwd:  edge pass + finish (two launches).  net NULL: no gradient wanted; else it is zeroed here and filled with c(v) for _bwd.
 *   _bwd:  one launch; dlogits rows are written, or added to (accumulate != 0).  grad: device pointer to the upstream scalar, NULL = 1.
 *   _step: _fwd + _bwd as two launches: the finish pass also writes dlogits, *total = *add_loss + reg (total / add_loss may be NULL) and
 *          running[2] += sums (may be NULL), and leaves net ZEROED.  net_is_zero != 0: the caller hands in a zeroed net (one that an earlier
 *          _step left); otherwise it is zeroed here first.  Same bits as _fwd followed by _bwd.
 * ---------------------------------------------------------------------------------------------- */
int64_t dgnn_edge_tv_scratch_doubles(void);
int dgnn_edge_tv_fwd(const float* logits, int64_t ldl, int64_t n, const void* src, const void* dst, int64_t estride, int idx64, int64_t E, float weight, int32_t* net,
                     double* sums, float* reg, double* scratch, int max_blocks, void* stream);
int dgnn_edge_tv_bwd(const float* logits, int64_t ldl, int64_t n, const int32_t* net, float weight, int64_t E, const float* grad, float* dlogits,
                     int64_t ldd, int accumulate, void* stream);
int dgnn_edge_tv_step(const float* logits, int64_t ldl, int64_t n, const void* src, const void* dst, int64_t estride, int idx64, int64_t E, float weight,
                      const float* grad, int32_t* net, int net_is_zero, double* sums, float* reg, const float* add_loss, float* total,
                      double* running, float* dlogits, int64_t ldd, int accumulate, double* scratch, int max_blocks, void* stream);

/* Fused decoder, eval mode (reference :180-187 applied at :350-351):
 *   logits = W3 . relu((W0 . y + b0) * scale + shift) + b3,   y [M,k] -> out [M,n_out]
 * Supports k == 128, hidden == 64, n_out in {1,2}; DGNN_E_UNSUPPORTED otherwise (use dgnn_linear_fwd twice). */
int dgnn_decoder_fused_fwd(const float* y, int64_t ldy, int64_t M, int k, const float* W0, const float* b0,
                           const float* scale, const float* shift, int hidden, const float* W3, const float* b3, int n_out,
                           float* out, int64_t ldo, void* stream);

/* ------------------------------------------------------------------------------------------------
 * bf16 STORAGE path (BASELINE config 3): activations (and, for the Updated variant, the edge
 * embeddings phi) live in HBM as bf16 (uint16_t bit patterns here, torch.bfloat16 on the Python side), every matrix
 * product runs once on the bf16 matrix cores with fp32 accumulation, parameters stay fp32 (master weights, rounded to
 * bf16 when staged).  Stated tolerance: |dlogit| <= 5e-2 * max(1, |logit|/8), arg-max agreement >= 99.9 % vs fp32.
 * Same argument meaning as the fp32 entry points of the same name; rows must be aligned as each comment says.
 * ---------------------------------------------------------------------------------------------- */
#define DGNN_BF16_SINGLE 0      /* every operand rounded to bf16 once, one MFMA per product */
#define DGNN_BF16_COMPENSATED 1 /* only what is STORED is bf16: the fp32 mean, attributes and parameters enter the matrix cores as
                                   (hi, lo) bf16 pairs (16 bits; filter 3 products, a.Wj 3, x_i.Wi 2) -- the default */
/* Row-format flags OR-ed into `mode` of dgnn_sage_layer_fused_fwd_bf16 / dgnn_sage_layer_fused_decoder_fwd_bf16 (round 4, compensated arithmetic only):
 * UNSIGNED rows.  A row written behind a ReLU has no negative entries, so its 16 bits can hold the fp32 bits [30:15] -- bf16's 8 exponent bits and
 * EIGHT explicit mantissa bits (9 significant bits; value = bits << 15) -- instead of sign + 7: same bytes, half the storage rounding (2^-10 of a
 * value).  _OUT: this launch writes such rows (needs relu != 0); _IN: x_src / x_dst are such rows.  A layer on 16-bit rows keeps the format (IN and OUT
 * together); the first layer, reading fp32 rows, may start it (OUT only); the decoder-carrying launch takes IN.  With the three stored layers of the
 * shipped model unsigned: max |dlogit| on the 1M-tet graph 5.9e-2 -> 2.1e-2.  dgnn_rows_unsigned_to_bf16 converts to plain bf16. */
#define DGNN_BF16_ROWS_IN_UNSIGNED 16
#define DGNN_BF16_ROWS_OUT_UNSIGNED 32
int dgnn_rows_unsigned_to_bf16(const uint16_t* in, int64_t ld_in, int64_t n, int cols, uint16_t* out, int64_t ld_out, void* stream);
/* out[r, 0:cols] = bf16(in[r, 0:cols]), out[r, cols:cols_pad] = 0   (cols_pad even, ld_out >= cols_pad, ld_out even) */
int dgnn_cast_f32_to_bf16(const float* in, int64_t ld_in, int64_t n, int cols, int cols_pad, uint16_t* out, int64_t ld_out, void* stream);
int dgnn_cast_bf16_to_f32(const uint16_t* in, int64_t ld_in, int64_t n, int cols, float* out, int64_t ld_out, void* stream);
/* dgnn_sage_layer_fused_fwd with bf16 x_src / x_dst / out (edge_attr and all parameters fp32).  c_in <= 128, c_out in {64,128};
 * with nb = 2/4/8 for c_in <= 32/64/128: c_in % nb == 0, ldx % nb == 0, rows 2*nb-byte aligned; ldo even, out 4-byte aligned.
 * x_f32 != 0 (c_in <= 32, the first layer): x_src / x_dst are the caller's fp32 rows (any 4-byte aligned stride), read in
 * place -- the input features are never rounded to bf16; the output is bf16 as always. */
int dgnn_sage_layer_fused_fwd_bf16(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int64_t n_dst, const void* x_src, int x_f32,
                                   const void* x_dst, int64_t ldx, int c_in, const float* edge_attr, int64_t lde, int f_e,
                                   const float* We, const float* be, const float* Wj, const float* bj, const float* Wi,
                                   const float* scale, const float* shift, int relu, int c_out, uint16_t* out, int64_t ldo, int mode,
                                   void* stream);
/* dgnn_decoder_fused_fwd on bf16 rows (16-byte aligned, ldy % 8 == 0); logits stay fp32 */
/* The LAST conv layer in bf16 storage with the decoder inside its launch (round 4; SurfaceNet.inference_layer :343-351 in the bf16 storage path):
 * dgnn_sage_layer_fused_fwd_bf16 followed by dgnn_decoder_fused_fwd_bf16 without the bf16 round trip of the layer's output -- the finished tile
 * reaches the decoder's matrix products as (hi, lo) bf16 pairs (16 significant bits; it is NEVER rounded to bf16: the storage rounding next to
 * the logits is gone) and only fp32 logits [n_dst, 2] are written.  Arguments as the two entry points.  Covers the shipped shape in the
 * compensated arithmetic: 64 < c_in <= 128 (c_in % 8 == 0), c_out = 128, f_e = 20 packed rows, decoder 128 -> 64 -> 2, bf16 rows 16-byte aligned
 * (ldx % 8 == 0), mode = DGNN_BF16_COMPENSATED; anything else: DGNN_E_UNSUPPORTED, nothing launched.  A tet's logits depend on its own inputs only
 * (destination sub-ranges give bit-identical results). */
int dgnn_sage_layer_fused_decoder_fwd_bf16(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int64_t n_dst, const uint16_t* x_src,
                                           const uint16_t* x_dst, int64_t ldx, int c_in, const float* edge_attr, int64_t lde, int f_e,
                                           const float* We, const float* be, const float* Wj, const float* bj, const float* Wi,
                                           const float* scale, const float* shift, int relu, int c_out, const float* W0, const float* b0,
                                           const float* scale1, const float* shift1, int c_hidden, const float* W3, const float* b3, int n_logits,
                                           float* logits, int mode, void* stream);
int dgnn_decoder_fused_fwd_bf16(const uint16_t* y, int64_t ldy, int64_t M, int k, const float* W0, const float* b0, const float* scale,
                                const float* shift, int hidden, const float* W3, const float* b3, int n_out, float* out, int64_t ldo,
                                int mode, void* stream);

/* bf16-storage twins of the generic (training / any-width) entry points above: x / phi / a / gradients of activations are
 * bf16, parameters and their gradients fp32, all arithmetic fp32 between a widening load and a rounding store; the GEMMs run
 * on v_mfma_f32_32x32x16_bf16.  dgnn_linear_fwd_bf16: out is bf16 (out_f32 == 0) or fp32 (logits).  dgnn_linear_wgrad_bf16:
 * A / B are bf16 (x_f32 == 0) or fp32 (rounded to bf16 when staged); scratch sizes as for the fp32 functions. */
int dgnn_sage_aggregate_fwd_bf16(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int64_t n_dst, const uint16_t* x_src,
                                 int64_t ldx, int c_in, const float* edge_attr, int64_t lde, int f_e, const float* We, const float* be,
                                 const uint16_t* phi, int64_t ldphi, uint16_t* phi_out, int64_t ldphi_out, uint16_t* a, int64_t lda,
                                 void* stream);
int dgnn_sage_aggregate_bwd_bf16(const int32_t* t_rowptr, const int32_t* t_dst, const int32_t* t_eid, int64_t n_src,
                                 const int32_t* rowptr_dst, const uint16_t* x_src, int64_t ldx, int c_in, const float* edge_attr,
                                 int64_t lde, int f_e, const float* We, const float* be, const uint16_t* phi, int64_t ldphi,
                                 const uint16_t* da, int64_t ldda, uint16_t* dx_src, int64_t lddx, float* dWe, float* dbe,
                                 uint16_t* dphi_out, int64_t lddphi, float* partials, void* stream);
int dgnn_linear_fwd_bf16(const uint16_t* A1, int64_t lda1, int k1, const float* W1, int64_t ldw1, const uint16_t* A2, int64_t lda2, int k2,
                         const float* W2, int64_t ldw2, const float* bias, const float* scale, const float* shift, int relu, int64_t M,
                         int n_out, void* out, int64_t ldo, int out_f32, void* stream);
int dgnn_linear_wgrad_bf16(const void* A, int a_f32, int64_t lda, int n_a, const void* B, int b_f32, int64_t ldb, int n_b, int64_t M,
                           float* dW, int64_t lddw, int accumulate, float* partials, void* stream);
int dgnn_bn_batch_stats_bf16(const uint16_t* x, int64_t ldx, int64_t M, int c, float* mean, float* var, float* running_mean,
                             float* running_var, float momentum, float* scratch, void* stream);
int dgnn_scale_shift_act_bf16(const uint16_t* x, int64_t ldx, const float* scale, const float* shift, int relu, int64_t M, int c,
                              uint16_t* y, int64_t ldy, void* stream);
int dgnn_bn_relu_bwd_bf16(const uint16_t* x, int64_t ldx, const uint16_t* y, int64_t ldy, const uint16_t* dy, int64_t lddy,
                          const float* gamma, const float* mean, const float* var, float eps, int train, int relu, int64_t M, int c,
                          uint16_t* dx, int64_t lddx, float* dgamma, float* dbeta, float* scratch, void* stream);
int dgnn_colsum_bf16(const uint16_t* x, int64_t ldx, int64_t M, int c, float* out, int accumulate, float* scratch, void* stream);
int dgnn_relu_bf16(const uint16_t* x, int64_t n, uint16_t* y, void* stream);
int dgnn_relu_bwd_bf16(const uint16_t* y, const uint16_t* g, int64_t n, uint16_t* out, void* stream);

/* Debug only: register a device buffer of n int64 slots; workgroup 0 of the fused kernel then stamps
 * wall_clock64() at phase boundaries (slot = (tile_iter*12 + wave)*8 + phase).  NULL disables. */
int dgnn_debug_trace_buffer(int64_t* dev_buf, int64_t n);

/* Debug only: the kernel the calling thread's last dense forward call chose (dgnn_linear_fwd, _x3, _x3_stats, _bf16, _x2h, _x2hp, and
 * the composite entry points that go through them); NONE before the first call and after a call that launched nothing (M = 0, an
 * argument error, DGNN_E_UNSUPPORTED).  A host-side record of the dispatch: the kernels do not know about it. */
enum dgnn_linear_variant {
    DGNN_LINEAR_VARIANT_NONE = 0,
    DGNN_LINEAR_VARIANT_F32 = 1,             /* k_linear_fwd */
    DGNN_LINEAR_VARIANT_X3 = 2,              /* k_linear_fwd_x3, 128 x 128 tiles */
    DGNN_LINEAR_VARIANT_X3_N64 = 3,          /* k_linear_fwd_x3_n64 */
    DGNN_LINEAR_VARIANT_X3_BIG = 4,          /* k_linear_fwd_x3_big, 256 x 256 tiles */
    DGNN_LINEAR_VARIANT_X3_MID1 = 5,         /* k_linear_fwd_x3_mid<1> */
    DGNN_LINEAR_VARIANT_X3_MID4 = 6,         /* k_linear_fwd_x3_mid<4> */
    DGNN_LINEAR_VARIANT_X3_SMALL = 7,        /* k_linear_fwd_x3_small<false> */
    DGNN_LINEAR_VARIANT_X3_SMALL_SPLITK = 8, /* k_linear_fwd_x3_small<true> */
    DGNN_LINEAR_VARIANT_B = 9,               /* k_linear_fwd_b */
    DGNN_LINEAR_VARIANT_B_MID1 = 10,         /* k_linear_fwd_b_mid<., 1> */
    DGNN_LINEAR_VARIANT_B_MID4 = 11,         /* k_linear_fwd_b_mid<., 4> */
    DGNN_LINEAR_VARIANT_B_SMALL = 12,        /* k_linear_fwd_b_small<., false> */
    DGNN_LINEAR_VARIANT_B_SMALL_SPLITK = 13, /* k_linear_fwd_b_small<., true> */
    DGNN_LINEAR_VARIANT_X2H = 14,            /* k_x2h_row_scales + k_linear_fwd_x2h_big */
    DGNN_LINEAR_VARIANT_X2HP = 15            /* k_x2hp_presplit + k_linear_fwd_x2hp_big */
};
int dgnn_debug_last_linear_variant(void);

/* ------------------------------------------------------------------------------------------------
 * k-hop block builder (full neighbourhoods here, sampled ones below): GPU replacement of the CPU
 * torch_geometric NeighborSampler(edge_index, sizes) the reference builds at run.py:72-74,221-223.
 * One hop: dgnn_khop_count -> host reads off[n_t] (edge total) -> dgnn_khop_expand -> host reads *n_new ->
 * dgnn_khop_commit; dgnn_khop_reset after the last hop of a batch.  `pos` int32 [n_nodes] all -1 and `first`
 * int32 [n_nodes] all INT32_MAX between batches (dgnn_fill_i32).  rowptr/src/eid: the by-destination plan.
 * Output of a hop: local edge list e_src/e_dst int64 [n_edges] (targets keep ids 0..n_t-1, new sources appended in
 * first-appearance order), e_id int64 [n_edges] rows of edge_attr, n_id_out int64 [n_t + n_new].
 * ---------------------------------------------------------------------------------------------- */
int dgnn_fill_i32(int32_t* p, int64_t n, int32_t value, void* stream);
int64_t dgnn_khop_scratch_elems(int64_t n_t, int64_t max_edges);
int dgnn_khop_count(const int32_t* rowptr, const int64_t* n_id, int64_t n_t, int first_hop, int32_t* pos, int32_t* off,
                    int32_t* scratch, void* stream);
int dgnn_khop_expand(const int32_t* rowptr, const int32_t* src, const int32_t* eid, const int64_t* n_id, int64_t n_t,
                     const int32_t* off, int64_t n_edges, int32_t* pos, int32_t* first, int64_t* e_src, int64_t* e_dst,
                     int64_t* e_id, int64_t* n_id_out, int32_t* n_new_out, int32_t* scratch, void* stream);
int dgnn_khop_commit(const int64_t* n_id_out, int64_t n_t, int64_t n_all, int32_t* pos, int32_t* first, void* stream);
int dgnn_khop_reset(const int64_t* n_id, int64_t n, int32_t* pos, void* stream);
/* All hops of one batch in one call for graphs with exactly `deg` in-edges per node (Delaunay scenes: 4): edge counts are known
 * without a read-back, the one 4-byte read per hop (new-node count) is waited for inside the call.  Hop h writes into
 * caller-allocated buffers of capacity cap_t[h] targets / cap_e[h] edges: ei[h] int64 [2, cap_e[h]], e_id[h] int64 [cap_e[h]],
 * src32[h] / e_id32[h] int32 [cap_e[h]] (int32 copies of ei[h] row 0 and of e_id[h]), off[h] int32 [cap_t[h]+1], n_id_out[h] int64 [cap_t[h]+cap_e[h]]; scratch =
 * max_h dgnn_khop_scratch_elems(cap_t[h], cap_e[h]) int32; n_new_dev one device int32; counts_out HOST int64 [hops+1] = targets
 * of every hop, then the node count of the outermost block.  t_rowptr != NULL also builds every hop's transposed plan (by source:
 * t_rowptr[h] int32 [cap_all[h]+1], t_dst[h] / t_eid[h] int32 [cap_e[h]]) and t_rows[h] = e_id32[h][t_eid[h]], with plan_scratch =
 * max_h dgnn_plan_scratch_elems(cap_e[h], cap_all[h]) int32.  DGNN_E_INVALID if a capacity is too small (pos is left all -1).
 * The per-hop count travels through pinned host memory the GPU writes to, not through a stream synchronize, so a host thread
 * running this call does not contend with another one that is launching kernels. */
int dgnn_khop_blocks_regular(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int deg, const int64_t* batch, int64_t n_batch,
                             int hops, int32_t* pos, int32_t* first, int64_t* const* ei, int64_t* const* e_id, int32_t* const* src32,
                             int32_t* const* e_id32, int32_t* const* off, int64_t* const* n_id_out, const int64_t* cap_t, const int64_t* cap_e, int32_t* scratch,
                             int32_t* n_new_dev, int32_t* const* t_rowptr, int32_t* const* t_dst, int32_t* const* t_eid, int32_t* const* t_rows,
                             const int64_t* cap_all, int32_t* plan_scratch, int64_t* counts_out, void* stream);
/* The same call on a library-owned host thread: start() returns a job handle at once (NULL + error text on bad arguments), a
 * std::thread issues the launches on `stream` and waits for the per-hop counts, wait() joins it, fills counts_out [hops+1] and
 * frees the job.  Between the two the caller may enqueue on OTHER streams only and must leave pos / first / the buffers alone. */
void* dgnn_khop_blocks_regular_start(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int deg, const int64_t* batch,
                                     int64_t n_batch, int hops, int32_t* pos, int32_t* first, int64_t* const* ei, int64_t* const* e_id,
                                     int32_t* const* src32, int32_t* const* e_id32, int32_t* const* off, int64_t* const* n_id_out,
                                     const int64_t* cap_t, const int64_t* cap_e, int32_t* scratch, int32_t* n_new_dev, int32_t* const* t_rowptr,
                                     int32_t* const* t_dst, int32_t* const* t_eid, int32_t* const* t_rows, const int64_t* cap_all,
                                     int32_t* plan_scratch, void* stream);
/* ... and up to 4 row gathers behind the block, on the builder's stream (the head-of-step x_all[n_id, 1:] / x_all[ids] / y_all[ids] of the reference's
 * training loop, learning/surfaceNetStaticEdgeFilters.py:206 and learning/runModel.py:273-274): r_out[i][k, 0:r_cols[i]] = r_src[i][id_k * r_ld[i] + 0:r_cols[i]]
 * for id_k = the nodes of the outermost block (r_which[i] = 0; n_id_out[hops-1][:counts[hops]]) or the batch's targets (r_which[i] = 1).  r_src[i] is
 * fp32 and already points at the first wanted column; r_out[i] holds capacity x r_cols[i] packed rows.  Valid after dgnn_khop_blocks_regular_wait. */
void* dgnn_khop_blocks_regular_start_rows(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int deg, const int64_t* batch,
                                          int64_t n_batch, int hops, int32_t* pos, int32_t* first, int64_t* const* ei, int64_t* const* e_id,
                                          int32_t* const* src32, int32_t* const* e_id32, int32_t* const* off, int64_t* const* n_id_out,
                                          const int64_t* cap_t, const int64_t* cap_e, int32_t* scratch, int32_t* n_new_dev,
                                          int32_t* const* t_rowptr, int32_t* const* t_dst, int32_t* const* t_eid, int32_t* const* t_rows,
                                          const int64_t* cap_all, int32_t* plan_scratch, int n_rows, const float* const* r_src, const int64_t* r_ld,
                                          const int32_t* r_cols, const int32_t* r_which, float* const* r_out, void* stream);
int dgnn_khop_blocks_regular_wait(void* job, int hops, int64_t* counts_out);
/* Sampled neighbourhoods (NeighborSampler sizes[h] > 0).  A target with global id g and d > size in-edges keeps the `size` of them with the
 * smallest 64-bit keys, ties to the smaller j, and the kept ones stay in plan order:
 *     mix = the splitmix64 finaliser;   key(j) = mix(mix(mix(seed + 0x9E3779B97F4A7C15 * (draw + 1)) ^ g) + ((hop << 32) | j))
 * with j = 0..d-1 the rank of the in-edge in plan order -- a counter-based hash, no RNG state and no atomics: the block is a pure function of
 * (graph, batch, size, seed, draw, hop).  Targets with d <= size, and size = -1, keep everything.  dgnn_khop_count_sampled /
 * dgnn_khop_expand_sampled replace dgnn_khop_count / dgnn_khop_expand in the per-hop protocol above (off = scan of min(d, size); the same
 * buffers; hop = 0 for the batch's own neighbourhood); size is -1 or > 0, draw >= 0, 0 <= hop < 65536. */
int dgnn_khop_count_sampled(const int32_t* rowptr, const int64_t* n_id, int64_t n_t, int first_hop, int size, uint64_t seed, int64_t draw, int hop,
                            int32_t* pos, int32_t* off, int32_t* scratch, void* stream);
int dgnn_khop_expand_sampled(const int32_t* rowptr, const int32_t* src, const int32_t* eid, const int64_t* n_id, int64_t n_t, const int32_t* off,
                             int64_t n_edges, int size, uint64_t seed, int64_t draw, int hop, int32_t* pos, int32_t* first, int64_t* e_src,
                             int64_t* e_dst, int64_t* e_id, int64_t* n_id_out, int32_t* n_new_out, int32_t* scratch, void* stream);
/* dgnn_khop_blocks_regular with sampled hops: sizes HOST int32 [hops] (-1 or > 0); hop h emits e_h = min(sizes[h], deg) edges per target (deg
 * for -1), so its edge count counts[h] * e_h needs no read-back and off[h][i] = e_h * i.  Capacities: cap_t[h] >= targets of hop h (at most
 * n_batch * prod_{g<h} (1 + e_g)), cap_e[h] >= e_h * cap_t[h]; row 1 of ei[h] starts at ei[h] + cap_e[h].  Everything else -- buffers,
 * transposed plans, counts_out, DGNN_E_INVALID on a small capacity with pos / first left clean, the _start / _start_rows forms on the
 * library's host thread, joined by dgnn_khop_blocks_regular_wait -- is as described there. */
int dgnn_khop_blocks_sampled(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int deg, const int64_t* batch, int64_t n_batch,
                             int hops, const int32_t* sizes, uint64_t seed, int64_t draw, int32_t* pos, int32_t* first, int64_t* const* ei,
                             int64_t* const* e_id, int32_t* const* src32, int32_t* const* e_id32, int32_t* const* off, int64_t* const* n_id_out,
                             const int64_t* cap_t, const int64_t* cap_e, int32_t* scratch, int32_t* n_new_dev, int32_t* const* t_rowptr,
                             int32_t* const* t_dst, int32_t* const* t_eid, int32_t* const* t_rows, const int64_t* cap_all, int32_t* plan_scratch,
                             int64_t* counts_out, void* stream);
void* dgnn_khop_blocks_sampled_start(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int deg, const int64_t* batch, int64_t n_batch,
                                     int hops, const int32_t* sizes, uint64_t seed, int64_t draw, int32_t* pos, int32_t* first, int64_t* const* ei,
                                     int64_t* const* e_id, int32_t* const* src32, int32_t* const* e_id32, int32_t* const* off,
                                     int64_t* const* n_id_out, const int64_t* cap_t, const int64_t* cap_e, int32_t* scratch, int32_t* n_new_dev,
                                     int32_t* const* t_rowptr, int32_t* const* t_dst, int32_t* const* t_eid, int32_t* const* t_rows,
                                     const int64_t* cap_all, int32_t* plan_scratch, void* stream);
void* dgnn_khop_blocks_sampled_start_rows(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int deg, const int64_t* batch,
                                          int64_t n_batch, int hops, const int32_t* sizes, uint64_t seed, int64_t draw, int32_t* pos, int32_t* first,
                                          int64_t* const* ei, int64_t* const* e_id, int32_t* const* src32, int32_t* const* e_id32,
                                          int32_t* const* off, int64_t* const* n_id_out, const int64_t* cap_t, const int64_t* cap_e, int32_t* scratch,
                                          int32_t* n_new_dev, int32_t* const* t_rowptr, int32_t* const* t_dst, int32_t* const* t_eid,
                                          int32_t* const* t_rows, const int64_t* cap_all, int32_t* plan_scratch, int n_rows, const float* const* r_src,
                                          const int64_t* r_ld, const int32_t* r_cols, const int32_t* r_which, float* const* r_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Logits -> labels -> interface facets (reference processing/generate_mesh.py:75 and :93-105).
 *   dgnn_argmax_rows     labels[i] = argmax_c logits[i,c]             (log_softmax(...).argmax(1), ties -> 0)
 *   dgnn_compact_i32     order-preserving stream compaction (finite-cell labels; interface facet ids)
 *   dgnn_interface_flags flags[f] = label(nfacets[f,0]) != label(nfacets[f,1]), cell -1 = outside
 *   dgnn_graph_cut_binary the optional graph cut between the two (:84-91), exact, on the device
 *   dgnn_graph_cut_weighted the same cut with one capacity per facet; dgnn_facet_cut_terms makes the capacities from the geometry
 * ---------------------------------------------------------------------------------------------- */
int dgnn_argmax_rows(const float* logits, int64_t ld, int64_t n, int c, int32_t* labels, void* stream);
int64_t dgnn_compact_scratch_elems(int64_t n);
int dgnn_compact_i32(const int32_t* values, const int32_t* keep, int invert, int64_t n, int32_t* out, int32_t* count_out,
                     int32_t* scratch, void* stream);
int dgnn_interface_flags(const int32_t* nfacets, const int32_t* labels_finite, int64_t n_facets, int32_t* flags, void* stream);

/* Exact binary graph cut of the finite cells' labels (reference processing/generate_mesh.py:15-58: gco alpha-expansion, two labels,
 * Potts term; with two labels a converged expansion is a global minimum, so one s-t minimum cut reaches the same energy).
 *   logits      fp32 [n, 2] (row stride ld >= 2), the finite cells in file order
 *   edges       int32 [n_rows, 2], the facets with two finite cells; duplicate rows add up, self-loops contribute nothing
 *   costs       D_i(0) = rint(fl(logits[i,1] * unary_weight)), D_i(1) = rint(fl(logits[i,0] * unary_weight)): the fp32 product and
 *               half-to-even rounding of `(prediction[:, [1, 0]] * uw).round()`; label 0 = inside, 1 = outside
 *   energy      E(l) = sum_i D_i(l_i) + binary_weight * #{rows (i, j): l_i != l_j}
 *   labels_out  int32 [n]: the minimiser with the FEWEST outside cells (unique; ties in the unary cost resolve to inside): the nodes that
 *               reach t in the residual graph of a maximum preflow (s -> i: max(D_i(1) - D_i(0), 0), i -> t: max(D_i(0) - D_i(1), 0),
 *               i <-> j: binary_weight per row)
 *   energy_out  int64 [1] E(labels_out); flow_out int64 [1] the maximum flow (E = flow + sum_i min D_i(.), checked before returning);
 *   stats_out   int32 [2] push-relabel steps, global relabels.  All three are DEVICE pointers (NULL: not written).
 *   scratch     dgnn_graph_cut_scratch_bytes(n, n_rows) bytes, 256-byte aligned.
 * DGNN_E_INVALID: binary_weight < 0, an edge id outside [0, n), non-finite logits, |D_i| >= 2^30, or a node whose capacities could overflow
 * int32 (terminal capacity + max(degree, 2) * binary_weight).  DGNN_E_UNSUPPORTED: the step / relabel cap was reached (never spins).
 * Unlike the rest of this header the call SYNCHRONISES `stream`: after the graph is built (error check), after every few BFS levels of each
 * global relabel (the frontier size and the stop flag are read on the host) and at the end (energy identity).  Synchronous push-relabel
 * without atomics on the flow: labels, energy and step counts are bit-identical from run to run. */
int64_t dgnn_graph_cut_scratch_bytes(int64_t n, int64_t n_rows);
int dgnn_graph_cut_binary(const float* logits, int64_t ld, int64_t n, const int32_t* edges, int64_t n_rows, float unary_weight,
                          int32_t binary_weight, int32_t* labels_out, int64_t* energy_out, int64_t* flow_out, int32_t* stats_out,
                          void* scratch, void* stream);

/* The same cut with one capacity per row: E(l) = sum_i D_i(l_i) + sum_r row_weights[r] [l_i != l_j].  Everything else is
 * dgnn_graph_cut_binary's (the same solver body): costs, labels_out = the minimiser with the fewest outside cells, energy / flow / stats,
 * scratch (dgnn_graph_cut_weighted_scratch_bytes = dgnn_graph_cut_scratch_bytes), the synchronisation points.
 *   row_weights int32 [n_rows], each >= 0.  A row of weight 0 stays in the graph with no capacity; duplicate rows add up; a self-loop never
 *               counts, whatever its weight.  With every weight = w the labels, energy, flow, steps and relabels are those of
 *               dgnn_graph_cut_binary(w): the same arithmetic in the same order.
 * DGNN_E_INVALID as above, and: a weight < 0 (of any row); a node with terminal capacity + max(sum of its incident weights, 2 * the
 * largest of them) > INT32_MAX (the excess is bounded by the terminal capacity plus what can flow in, an arc's residual by twice its row's
 * weight). */
int64_t dgnn_graph_cut_weighted_scratch_bytes(int64_t n, int64_t n_rows);
int dgnn_graph_cut_weighted(const float* logits, int64_t ld, int64_t n, const int32_t* edges, int64_t n_rows, float unary_weight,
                            const int32_t* row_weights, int32_t* labels_out, int64_t* energy_out, int64_t* flow_out, int32_t* stats_out,
                            void* scratch, void* stream);

/* Per-facet weights for dgnn_graph_cut_weighted from the geometry of `<scene>_3dt.npz` (the layout of
 * dgnn_locate_points: vertices fp64 [n_vertices, 3], tets int32 [n_cells, 4], facets int32 [n_facets, 3], nfacets int32 [n_facets, 2]).
 *   kind 1 (area)  q_f = A_f / mean(A),  A_f = |(b - a) x (c - a)| / 2
 *   kind 2 (beta)  q_f = 1 - min(cos phi_T1, cos phi_T2) in [0, 2]  (Labatut et al. 2009: phi = the angle between the facet and the
 *                  circumsphere of the cell on that side; cos > 0 when the circumcentre lies on the cell's own side of the facet)
 *   w_f = (int32) rint(binary_weight * q_f)   (fp64 product, half to even)
 * A facet is a graph row iff both entries of its nfacets row are >= 0; every other facet gets q = 0, w = 0 (and is in none of the sums).
 * q_out DEVICE fp64 [n_facets] (NULL: not written), w_out DEVICE int32 [n_facets], stats_out DEVICE int64 [4] (NULL: not written): graph
 * rows, neutralised sides, graph rows with w_f == 0, max w_f.  scratch: dgnn_facet_cut_terms_scratch_bytes(n_facets) bytes.
 *
 * OPERATION ORDER (fp64, no contraction; tests/graph_cut_weights_model.py restates it).  For 3-vectors
 *   x - y = componentwise;  x X y = (x.y y.z - x.z y.y,  x.z y.x - x.x y.z,  x.x y.y - x.y y.x);  x . y = (x.x y.x + x.y y.y) + x.z y.z.
 * With (a, b, c) the facet's vertices as stored:
 *   n = (b - a) X (c - a);  nn = sqrt(n . n);  A_f = 0.5 * nn.
 *   mean(A) = S / rows: S = the sum over ALL facets f = 0 .. n_facets-1 of A_f (0 for a facet that is no graph row) taken serially in chunks
 *   of 256 consecutive facets, the chunk sums then added serially in chunk order, each from 0.0; rows as a double.  q_f = A_f / mean(A).
 * beta, for the side of cell T = nfacets[f, k] with vertices p0..p3 as stored and d = the one vertex id of T not in the facet:
 *   u = p1 - p0, v = p2 - p0, w = p3 - p0;  vw = v X w, wu = w X u, uv = u X v;  det = u . vw;  d2 = 2.0 * det;
 *   c.x = ((|u|^2 vw.x + |v|^2 wu.x) + |w|^2 uv.x) / d2  (y, z alike; |x|^2 = x . x): the circumcentre relative to p0;  R = sqrt(c . c);
 *   sd = n . (d - a);  g = (p0 + c) - a;  hn = n . g;  h = (sd > 0 ? hn : -hn) / nn;  r = h / R;  cos phi_T = min(max(r, -1), 1).
 *   The side is NEUTRAL (cos phi_T = 0, counted in stats_out[1]) when det == 0, nn == 0, sd == 0 or one of R, h, r is not finite.
 *   q_f = 1.0 - (cos phi_T1 < cos phi_T2 ? cos phi_T1 : cos phi_T2), T1 = nfacets[f, 0], T2 = nfacets[f, 1].
 * DGNN_E_INVALID: kind not 1 / 2; binary_weight < 0 or not finite; a vertex id of any facet, or of a cell named by a graph row, outside
 * [0, n_vertices), or a cell id >= n_cells; a graph row whose facet is not a face of a cell its nfacets row names (beta); mean(A) that is
 * 0 or not finite when there are graph rows (area); a w_f that is not below 2^30.  The call SYNCHRONISES `stream` once, at its end.  All
 * counters are integer atomics and the sum has a fixed order: reruns are bit-identical. */
int64_t dgnn_facet_cut_terms_scratch_bytes(int64_t n_facets);
int dgnn_facet_cut_terms(const double* vertices, int64_t n_vertices, const int32_t* tets, int64_t n_cells, const int32_t* facets,
                         const int32_t* nfacets, int64_t n_facets, int kind, double binary_weight, double* q_out, int32_t* w_out,
                         int64_t* stats_out, void* scratch, void* stream);

/* The facet geometry columns of `<scene>_fgeom.npz` (a definition of this package's own: the reference's file is
 * missing and its column names are unknown).  Inputs in the layout above; the arithmetic, operation for operation, is the one stated for
 * dgnn_facet_cut_terms (csrc/facet_geom.h holds it once for both), in two passes: every cell's circumsphere once, then every facet.
 *
 * dgnn_cell_circumspheres: centre_radius_out DEVICE fp64 [n_cells, 4], 32-byte aligned: (o.x, o.y, o.z, R) per cell with c as above,
 *   o = p0 + c per component and R = sqrt(c . c).  A flat cell (det == 0) divides by zero: its R is inf or NaN, its o not finite; no flag
 *   is kept, the conditions of a NEUTRAL side catch it.  stats_out DEVICE int64 [4] (NULL: not written): [3] = the cells with det == 0,
 *   [0..2] = 0.  scratch: dgnn_cell_circumspheres_scratch_bytes() bytes.
 *
 * dgnn_facet_geometry: out DEVICE fp64 [4, 4 n_cells], zero-filled by the call, the four columns area, cos_own, cos_neighbor, beta of the
 *   rows 4 t + k = the facet of cell t opposite its vertex k (the row order of `_adjacencies.npz`).  Per facet f = (a, b, c) as stored:
 *     n = (b - a) X (c - a);  nn = sqrt(n . n);  area = 0.5 * nn;
 *     per side s with T = nfacets[f, s]:  T >= 0: cos_s = cos phi_T from T's stored (o, R): sd = n . (d - a); hn = n . (o - a);
 *       h = (sd > 0 ? hn : -hn) / nn; r = h / R; cos_s = min(max(r, -1), 1); NEUTRAL (cos_s = 0, counted) when nn == 0, sd == 0 or one of R, h,
 *       r is not finite -- dgnn_facet_cut_terms' rule: det == 0 makes R not finite;  T < 0 (the infinite cell): cos_s = 1.0, not counted:
 *       the circumsphere of an infinite cell is the half-space beyond the hull facet, its centre infinitely far on its own side, h / R -> 1;
 *     beta = 1.0 - (cos_0 < cos_1 ? cos_0 : cos_1);
 *     every side with a cell T writes the row 4 T + k, k = the slot of T's one vertex that is not on the facet:
 *       (area, cos_own = cos_s, cos_neighbor = cos_(1-s), beta).  A facet with both nfacets entries < 0 writes nothing.
 *   area and beta are bit-equal on the two directed rows of a facet, cos_own and cos_neighbor swap; all four are finite on every input,
 *   the cosines in [-1, 1], beta in [0, 2]; at a facet between two finite cells beta is dgnn_facet_cut_terms' q (kind 2) bit for bit.
 *   spheres   DEVICE fp64 [n_cells, 4] as dgnn_cell_circumspheres wrote it (32-byte aligned), or NULL: computed into the scratch here.
 *   stats_out DEVICE int64 [4] (NULL: not written): rows written, rows whose neighbour is the infinite cell, neutral sides, flat cells
 *             (0 when `spheres` was given).  A `_3dt` that lists every facet of every finite cell once gives rows == 4 n_cells.
 *   scratch   dgnn_facet_geometry_scratch_bytes(n_cells) bytes.
 * DGNN_E_INVALID: a vertex id of a facet or of a cell outside [0, n_vertices), a cell id >= n_cells, a facet that is not a face of a cell
 * its nfacets row names.  DGNN_E_UNSUPPORTED: 4 n_cells, n_vertices or 3 n_facets beyond int32.  Both calls SYNCHRONISE `stream` once, at
 * their end.  Every row has one writer, the counters are integer atomics: reruns are bit-identical. */
int64_t dgnn_cell_circumspheres_scratch_bytes(void);
int dgnn_cell_circumspheres(const double* vertices, int64_t n_vertices, const int32_t* tets, int64_t n_cells, double* centre_radius_out,
                            int64_t* stats_out, void* scratch, void* stream);
int64_t dgnn_facet_geometry_scratch_bytes(int64_t n_cells);
int dgnn_facet_geometry(const double* vertices, int64_t n_vertices, const int32_t* tets, int64_t n_cells, const int32_t* facets,
                        const int32_t* nfacets, int64_t n_facets, const double* spheres, double* out, int64_t* stats_out, void* scratch,
                        void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mesh metrics of the interface surface (reference processing/generate_mesh.py:126-163, processing/evaluate_mesh.py compute_iou /
 * compute_chamfer).  DESIGN.md section 14.
 *
 * dgnn_locate_points: the finite cell that contains each query point, by a walk in the tetrahedralization of `<scene>_3dt.npz`.
 *   vertices  fp64 [n_vertices, 3]; tets int32 [n_cells, 4] (the finite cells); facets int32 [n_facets, 3] vertex ids; nfacets int32
 *             [n_facets, 2] the two cells of each facet, -1 = the infinite cell.  Every face of every cell must have its facet.
 *   points    fp32 [n_points, 3]; cell_out int32 [n_points]: a cell whose four orientation signs are >= 0 (see below), -1 = outside the
 *             convex hull.  steps_out: DEVICE int32 [1], the longest walk (NULL: not written).
 *   rule      orientations are det[b - a, c - a, p - a] in fp64 with (a, b, c) the facet's vertices in ascending id order, so the two
 *             cells of a facet see one number with opposite signs.  The walk starts at the lowest-id cell whose centroid bins with the
 *             point (uniform grid of about n_cells / 2 bins over the vertices' box; an empty bin takes the start of the nearest non-empty
 *             bin along x, ties to the lower index, then of the nearest filled one along y, then along z), accepts the first cell on its path whose four signs are >= 0, and otherwise steps across the
 *             lowest-k face (opposite tets[c][k]) whose sign is < 0.  A point on a shared face or vertex is given the first cell on that
 *             path that has it on its boundary.  Deterministic.
 *   scratch   dgnn_locate_scratch_bytes(n_cells) bytes, 256-byte aligned.
 * DGNN_E_INVALID: a vertex / cell id out of range, non-finite vertices or points, or facets / nfacets that do not describe the tets' faces
 * (a facet whose vertices are not three of a listed cell's, a face without a facet, a neighbour that does not point back).
 * DGNN_E_UNSUPPORTED: a walk reached 65536 steps (it never spins).  SYNCHRONISES `stream` three times (input check, table check, end).
 *
 * dgnn_mesh_iou_counts: occ_out[i] = (cells[i] in [0, n_cells) and labels[cells[i]] == 0) (0 = inside; NULL: not written);
 *   counts_out DEVICE int64 [2] = (|A n B|, |A u B|) with A = occ_out, B = occ_gt[i] != 0 (uint8).  scratch: 256 bytes.  Asynchronous.
 *
 * dgnn_sample_faces: n_samples points on the faces face_ids[0 .. n_faces) of `facets` (face_ids NULL: facets 0 .. n_faces), chosen by area:
 *   area_j = 0.5 |(b - a) x (c - a)| (fp64), cum = their inclusive sum in a fixed order (cumarea_out: DEVICE fp64 [n_faces], NULL = kept in
 *   scratch).  Sample i draws r_k = mm_hash(seed, 3 i + k + 1), k = 0, 1, 2, with
 *       mm_hash(s, c): z = s + c * 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *                      return z ^ (z >> 31)                                          (uint64 arithmetic, wrapping)
 *   x = ((r_0 >> 11) + 1) 2^-53 * cum[n_faces - 1]; face j = the first with cum[j] >= x (zero-area faces get no samples);
 *   u = (r_1 >> 11) 2^-53, v = (r_2 >> 11) 2^-53, both replaced by 1 - u, 1 - v when u + v > 1;
 *   point = float((u (b - a) + v (c - a)) + a) per coordinate in fp64.  face_out int32 [n_samples] = j (NULL: not written).
 *   scratch: dgnn_sample_faces_scratch_bytes(n_faces) bytes.  DGNN_E_INVALID: ids out of range, non-finite areas, or samples asked of a
 *   total area of 0.  SYNCHRONISES `stream` once (after the areas).
 *
 * dgnn_nearest_neighbor: for every query point the nearest reference point (both fp32 [n, 3]): idx_out int32 = the smallest index among
 *   the minimisers of d2 = (dx*dx + dy*dy) + dz*dz (fp32, no contraction), dist_out fp32 = sqrtf(d2).  sum_out: DEVICE fp64 [1], the sum of
 *   dist_out in a fixed order (NULL: not computed).  n_ref >= 1.  scratch: dgnn_nearest_scratch_bytes(n_ref, n_query) bytes.
 *   DGNN_E_INVALID: non-finite coordinates.  SYNCHRONISES `stream` twice (the reference set's box, the end).
 * All four are bit-identical from run to run.
 * ---------------------------------------------------------------------------------------------- */
int64_t dgnn_locate_scratch_bytes(int64_t n_cells);
int dgnn_locate_points(const double* vertices, int64_t n_vertices, const int32_t* tets, int64_t n_cells, const int32_t* facets,
                       const int32_t* nfacets, int64_t n_facets, const float* points, int64_t n_points, int32_t* cell_out, int32_t* steps_out,
                       void* scratch, void* stream);
int dgnn_mesh_iou_counts(const int32_t* cells, int64_t n_points, const int32_t* labels, int64_t n_cells, const uint8_t* occ_gt, int32_t* occ_out,
                         int64_t* counts_out, void* scratch, void* stream);
int64_t dgnn_sample_faces_scratch_bytes(int64_t n_faces);
int dgnn_sample_faces(const double* vertices, int64_t n_vertices, const int32_t* facets, int64_t n_facets, const int32_t* face_ids,
                      int64_t n_faces, int64_t n_samples, uint64_t seed, float* points_out, int32_t* face_out, double* cumarea_out,
                      void* scratch, void* stream);
int64_t dgnn_nearest_scratch_bytes(int64_t n_ref, int64_t n_query);
int dgnn_nearest_neighbor(const float* ref, int64_t n_ref, const float* query, int64_t n_query, float* dist_out, int32_t* idx_out,
                          double* sum_out, void* scratch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The mesh `generate` returns (reference processing/generate_mesh.py:107-124: trimesh.Trimesh(process=True), fix_normals, Open3D's
 * is_watertight).  DESIGN.md section 15.
 *
 * dgnn_orient_interface: faces_out int32 [n_faces, 3] = the facets face_ids[0 .. n_faces) (ids into facets / nfacets, the scene layout of
 *   dgnn_locate_points), wound by the rule below when `orient` != 0, else as stored.  labels int32 [n_cells]: 0 = inside; cell -1 (the
 *   infinite cell) is outside.
 *   rule      for facet (a, b, c) let o(p) = det[b - a, c - a, p - a], evaluated EXACTLY on the fp64 coordinates, and d_in the vertex of
 *             the inside cell that is not on the facet.  o(d_in) != 0: emit (a, b, c) when o(d_in) < 0, else (a, c, b) (the normal points
 *             away from the inside cell).  o(d_in) == 0 and a finite outside cell: the same with its opposite vertex d_out, (a, b, c) when
 *             o(d_out) > 0, else (a, c, b).  Otherwise the stored winding, counted in n_undetermined_out (DEVICE int64 [1], NULL: not
 *             written).  exact_used_out: DEVICE int32 [1], 1 when the fp64 filter left some sign to the exact stage (NULL: not written).
 *   scratch   dgnn_orient_interface_scratch_bytes() bytes.
 * DGNN_E_INVALID: an id out of range; a facet whose three vertices are not a face of a finite cell nfacets names; a facet that does not
 * separate an inside cell from an outside one; a non-finite coordinate (orient != 0).  DGNN_E_UNSUPPORTED: a coordinate that is not 0 and
 * has a magnitude outside [2^-300, 2^300] (where the exact stage is not exact).  SYNCHRONISES `stream` once (status).
 *
 * dgnn_compact_vertices: kept_out int32 [n_vertices] = the vertex ids `faces` references, ascending (dgnn_compact_i32), n_kept_out DEVICE
 *   int32 [1] = their number, faces_out int32 [n_faces, 3] = faces renumbered onto them.  scratch: dgnn_compact_vertices_scratch_bytes
 *   (n_vertices) bytes.  DGNN_E_INVALID: an id out of range.  SYNCHRONISES `stream` once (status).
 *
 * dgnn_mesh_topology: counts_out DEVICE int64 [5] of the triangle mesh faces int32 [n_faces, 3]:
 *   [0] n_edges                 undirected edges
 *   [1] boundary_edges          edges in exactly 1 face
 *   [2] nonmanifold_edges       edges in 3 or more faces
 *   [3] nonmanifold_vertices    referenced vertices whose incident faces are not ONE set connected through shared edges that contain the
 *                               vertex (Open3D's IsVertexManifold)
 *   [4] winding_mismatch_edges  undirected edges {u, v} with #(u -> v) != #(v -> u) over the faces' directed edges (a, b), (b, c), (c, a)
 *   watertight = [1] == 0 && [2] == 0 && [3] == 0 (Open3D's IsEdgeManifold(false) && IsVertexManifold(); self-intersection is not tested).
 *   Integer counts: independent of the schedule.  scratch: dgnn_mesh_topology_scratch_bytes(n_faces, n_vertices) bytes.
 *   DGNN_E_INVALID: an id out of range or a face with a repeated vertex.  SYNCHRONISES `stream` once (input check).
 * ---------------------------------------------------------------------------------------------- */
int64_t dgnn_orient_interface_scratch_bytes(void);
int dgnn_orient_interface(const double* vertices, int64_t n_vertices, const int32_t* tets, int64_t n_cells, const int32_t* facets,
                          const int32_t* nfacets, int64_t n_facets, const int32_t* labels, const int32_t* face_ids, int64_t n_faces, int orient,
                          int32_t* faces_out, int64_t* n_undetermined_out, int32_t* exact_used_out, void* scratch, void* stream);
int64_t dgnn_compact_vertices_scratch_bytes(int64_t n_vertices);
int dgnn_compact_vertices(const int32_t* faces, int64_t n_faces, int64_t n_vertices, int32_t* faces_out, int32_t* kept_out, int32_t* n_kept_out,
                          void* scratch, void* stream);
int64_t dgnn_mesh_topology_scratch_bytes(int64_t n_faces, int64_t n_vertices);
int dgnn_mesh_topology(const int32_t* faces, int64_t n_faces, int64_t n_vertices, int64_t* counts_out, void* scratch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Connected components of a triangle mesh, their measures and the small-component filter (the reference: trimesh split / body_count).
 * DESIGN.md section 22.
 *
 * dgnn_mesh_components: comp_out int32 [n_faces] = the component of every face of faces int32 [n_faces, 3], n_components_out DEVICE
 *   int32 [1] = their number K.
 *   rule      two faces are connected when they share an undirected edge {u, v}, however many faces share it: a non-manifold edge joins
 *             all of its faces (Open3D's cluster_connected_triangles).  Contact at a vertex alone does not connect.
 *   numbering components are numbered 0 .. K-1 in ascending order of their smallest face id: comp_out is a function of the mesh alone, the
 *             same for every schedule and every rerun.
 *   scratch   dgnn_mesh_components_scratch_bytes(n_faces) bytes.
 *   n_faces == 0 is valid: K = 0.  DGNN_E_INVALID: an id out of range or a face with a repeated vertex (as dgnn_mesh_topology);
 *   DGNN_E_UNSUPPORTED: 3 n_faces >= 2^31 - 1.  SYNCHRONISES `stream` once (input check).
 *
 * dgnn_mesh_component_measures: per component c of comp int32 [n_faces] (values in [0, n_components)), for vertices fp64 [n_vertices, 3]:
 *   n_faces_out int64 [K], area_out fp64 [K], volume_out fp64 [K] (a component id without faces gets 0, 0.0, 0.0).
 *   terms     of face (v0, v1, v2), every operation an fp64 operation rounded on its own (no fused multiply-add), with u = v1 - v0,
 *             w = v2 - v0, n = (uy wz - uz wy, uz wx - ux wz, ux wy - uy wx):
 *               area   = 0.5 * sqrt((nx nx + ny ny) + nz nz)
 *               volume = ((v0x (v1y v2z - v1z v2y) + v0y (v1z v2x - v1x v2z)) + v0z (v1x v2y - v1y v2x)) / 6
 *             volume_out = the signed volume of the component in its stored winding (positive when a closed component is wound outward).
 *   order     the faces are sorted stably by component: component c holds positions [s, e) of that order, in ascending face id.  [s, e)
 *             is cut at the multiples of 256; every piece is summed from 0.0 in ascending position, and the piece sums are added from 0.0
 *             in ascending position.  Bit-identical from run to run.
 *   scratch   dgnn_mesh_component_measures_scratch_bytes(n_faces, n_components) bytes.
 *   DGNN_E_INVALID: a vertex or component id out of range (faces with n_components == 0 included), n_components > n_faces;
 *   DGNN_E_UNSUPPORTED as above.  Non-finite coordinates give non-finite sums.  SYNCHRONISES `stream` once (input check).
 *
 * dgnn_mesh_component_keep: keep_out int32 [n_faces] = 1 for the faces of the components the rule keeps, n_kept_out DEVICE int64 [1] =
 *   their number; component_faces int64 [n_components] = the n_faces_out above.  Integer logic only.
 *   rule 0    `largest`: the one component with the most faces; a tie goes to the smaller component id (min_faces is ignored)
 *   rule 1    `min_faces`: every component with at least min_faces (>= 1) faces
 *   The kept faces are compacted with dgnn_compact_i32 (face order preserved) and their vertices with dgnn_compact_vertices.
 *   scratch   dgnn_mesh_component_keep_scratch_bytes() bytes.  DGNN_E_INVALID: a component id out of range, an unknown rule, min_faces < 1.
 *   SYNCHRONISES `stream` once (status).
 * ---------------------------------------------------------------------------------------------- */
int64_t dgnn_mesh_components_scratch_bytes(int64_t n_faces);
int dgnn_mesh_components(const int32_t* faces, int64_t n_faces, int64_t n_vertices, int32_t* comp_out, int32_t* n_components_out, void* scratch,
                         void* stream);
int64_t dgnn_mesh_component_measures_scratch_bytes(int64_t n_faces, int64_t n_components);
int dgnn_mesh_component_measures(const double* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const int32_t* comp,
                                 int64_t n_components, int64_t* n_faces_out, double* area_out, double* volume_out, void* scratch, void* stream);
int64_t dgnn_mesh_component_keep_scratch_bytes(void);
int dgnn_mesh_component_keep(const int32_t* comp, int64_t n_faces, const int64_t* component_faces, int64_t n_components, int rule,
                             int64_t min_faces, int32_t* keep_out, int64_t* n_kept_out, void* scratch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The scene front end: cell adjacency, cell geometry (`_cgeom`) and the vertex-ray visibility aggregates (`_cbvf`, `_fbvf`) of a
 * triangulation in `_3dt.npz` layout (vertices fp64 [n_vertices, 3], tetrahedra int32 [n_tets, 4] = the finite cells, facets int32
 * [n_facets, 3], nfacets int32 [n_facets, 2], -1 = the infinite cell).  DESIGN.md section 25.  Everything is fp64, every operation
 * rounded on its own (no fused multiply-add); (a, b, c) . (d, e, f) below means (a d + b e) + c f.  Every entry point SYNCHRONISES `stream`
 * (status read).  DGNN_E_INVALID: an id out of range; DGNN_E_UNSUPPORTED: 4 n_tets, n_vertices or n_rays beyond int32.
 *
 * dgnn_tet_neighbors: neighbors_out int32 [n_tets, 4]: slot k = the cell across the facet opposite vertex k of the tet (the facet made of
 *   its three other vertices), -1 = the infinite cell (also where no facet names the slot).  n_bad_out DEVICE int64 [1] = the (facet,
 *   cell) pairs whose facet is not made of three vertices of the cell nfacets names; such a pair writes nothing.  scratch: 256 bytes.
 *
 * dgnn_cell_geometry: per tet (p0, p1, p2, p3), with u = p1 - p0, v = p2 - p0, w = p3 - p0, a x b the usual cross product (each component
 *   one product minus one product):
 *     det      = u . (v x w)
 *     vol      = |det| / 6
 *     radius   = sqrt(r . r) / (2 |det|) with r = ((u . u) (v x w) + (v . v) (w x u)) + (w . w) (u x v) per component; +inf when det == 0
 *                (n_flat_out DEVICE int64 [1] counts those tets)
 *     longest, shortest = max, min of sqrt(d . d), d = pj - pi over the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
 *   edge_sums_out DEVICE fp64 [2] = the sums of longest_out and of shortest_out in a fixed order: chunks of 256 tets summed serially from
 *   0.0, then the chunk sums serially from 0.0 (the loader's mean_edge = (the two sums) / (2 * number of cells)).
 *   scratch   dgnn_cell_geometry_scratch_bytes(n_tets) bytes.
 *
 * dgnn_vertex_incidence: rowptr_out int32 [n_vertices + 1], entries_out int32 [4 n_tets]: row v holds the entries 4 t + k with
 *   tetrahedra[t][k] == v.  The order inside a row is not specified (and may differ between runs); nothing computed from it depends on it.
 *   scratch   dgnn_vertex_incidence_scratch_bytes(n_vertices) bytes.
 *
 * dgnn_vertex_rays: ray r runs from p = vertices[ray_vertex[r]] towards s = sensors[r] (fp64 [n_rays, 3]); rowptr / entries as above.
 *   used      a ray with s == p is skipped (stats 2); with unique != 0 only the lowest-index ray of every vertex is used, the others are
 *             skipped (stats 1).
 *   cell      side 0 (`outside`, towards the sensor), side 1 (`inside`, away from it).  For an incident tet with p at slot k and the other
 *             vertices q0, q1, q2 in slot order, D = sign det[q0 - p, q1 - p, q2 - p] and S_i = sign det[qa - p, qb - p, s - p] over
 *             (a, b) = (0,1), (1,2), (2,0), all EXACT on the input coordinates (csrc/exact_orient.h: an fp64 filter, then an exact
 *             expansion).  The tet qualifies for side 0 when D != 0 and every S_i D >= 0 (the sensor on the tet's side of each of its three
 *             facets through p, or on the plane), for side 1 when D != 0 and every S_i D <= 0.  Per side the LOWEST qualifying tet index
 *             is taken; none: the side records nothing (stats 3, 4).
 *   dist      t = n . (q0 - p) / (n . d), n = (q1 - q0) x (q2 - q0), d = e / sqrt(e . e) (each component divided) with e = s - p, negated
 *             for side 1.
 *   per ray   ray_tet_out, ray_slot_out int32 [n_rays, 2] (-1 = none), ray_dist_out fp64 [n_rays, 2] (0 where none).
 *   per tet   tet_count_out int32 [2, n_tets], tet_stat_out fp64 [2, 3, n_tets] = min, max, sum of dist over the rays that chose the tet
 *             on that side; slot_count_out int32 [2, n_tets, 4], slot_stat_out fp64 [2, 3, n_tets, 4] the same per (tet, slot k).  min and
 *             max are 0 where the count is 0.  The sums add from 0.0 in ascending ray index: bit-identical from run to run.
 *   stats_out DEVICE int64 [6]: rays used, duplicates skipped, s == p skipped, used rays without an outside cell, without an inside cell,
 *             orientation signs the exact stage decided.
 *   scratch   dgnn_vertex_rays_scratch_bytes(n_rays, n_tets, n_vertices) bytes.
 *   DGNN_E_INVALID also: an entry that is not a corner of the ray's vertex, non-finite coordinates; DGNN_E_UNSUPPORTED also: a non-zero
 *   coordinate magnitude outside [2^-300, 2^300] (the exact predicate's range).
 * ---------------------------------------------------------------------------------------------- */
int64_t dgnn_tet_neighbors_scratch_bytes(void);
int dgnn_tet_neighbors(const int32_t* tetrahedra, int64_t n_tets, const int32_t* facets, const int32_t* nfacets, int64_t n_facets,
                       int32_t* neighbors_out, int64_t* n_bad_out, void* scratch, void* stream);
int64_t dgnn_cell_geometry_scratch_bytes(int64_t n_tets);
int dgnn_cell_geometry(const double* vertices, int64_t n_vertices, const int32_t* tetrahedra, int64_t n_tets, double* radius_out, double* vol_out,
                       double* longest_out, double* shortest_out, double* edge_sums_out, int64_t* n_flat_out, void* scratch, void* stream);
int64_t dgnn_vertex_incidence_scratch_bytes(int64_t n_vertices);
int dgnn_vertex_incidence(const int32_t* tetrahedra, int64_t n_tets, int64_t n_vertices, int32_t* rowptr_out, int32_t* entries_out, void* scratch,
                          void* stream);
int64_t dgnn_vertex_rays_scratch_bytes(int64_t n_rays, int64_t n_tets, int64_t n_vertices);
int dgnn_vertex_rays(const double* vertices, int64_t n_vertices, const int32_t* tetrahedra, int64_t n_tets, const int32_t* rowptr,
                     const int32_t* entries, const int32_t* ray_vertex, const double* sensors, int64_t n_rays, int unique, int32_t* ray_tet_out,
                     int32_t* ray_slot_out, double* ray_dist_out, int32_t* tet_count_out, double* tet_stat_out, int32_t* slot_count_out,
                     double* slot_stat_out, int64_t* stats_out, void* scratch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The facet-ray walk (`_cbff`, `_fbff`): every ray of dgnn_vertex_rays followed through ALL the cells it crosses.  DESIGN.md section 29.
 * The rule is this package's own definition (the reference binary's walk is not known).  vertices, tetrahedra, rowptr / entries, ray_vertex,
 * sensors and unique as for dgnn_vertex_rays; neighbors int32 [n_tets, 4] as dgnn_tet_neighbors writes it (-1 = the infinite cell).  fp64,
 * every operation rounded on its own; orient(a, b, c, x) = sign det[b - a, c - a, x - a], EXACT (csrc/exact_orient.h).  SYNCHRONISES `stream`.
 *
 *   ray       from p = vertices[ray_vertex[r]] to s = sensors[r].  Skipped: s == p, and with unique != 0 every ray but the lowest-index one
 *             of its vertex.  Lane (r, side): side 0 (`outside`) walks from p towards s, side 1 (`inside`) from p away from s.
 *   sigma     the side of the ray's line against an edge (u, v): sigma(u, v) = sign det[s' - p, u - p, v - p] with the symbolically perturbed
 *             sensor s' = s + (eps, eps^2, eps^3), i.e. the first non-zero of
 *               orient(p, s, u, v), orient(p, px, u, v), orient(p, py, u, v), orient(p, pz, u, v)
 *             where pa is p with its coordinate a replaced by up(a) = 0 for a < 0, 1 for a == 0, 2 a for a > 0 (a representable point
 *             straight above p on that axis, so the sign is that of det[e_a, u - p, v - p]).  Later terms are evaluated only when the earlier
 *             ones are 0.  sigma is 0 only when p, u, v are collinear, it is antisymmetric, and it depends on coordinates alone.
 *   crossed   a facet (a, b, c) is crossed with sign +1 when sigma(a,b), sigma(b,c), sigma(c,a) are all >= 0 and not all 0, with sign -1
 *             when all <= 0 and not all 0.
 *   start     over the tets incident to p (p at slot k, the others q0, q1, q2 in slot order): D = orient(p, q0, q1, q2), then sigma(q0,q1),
 *             sigma(q1,q2), sigma(q2,q0).  A tet with D != 0 whose facet is crossed with sign D starts side 0, with sign -D side 1; per
 *             side the lowest such tet index.  None: status `none`.  The exit facet is f = (q0, q1, q2) with its three signs, exit slot k.
 *   loop      in cell c with exit slot k, exit facet f = (f0, f1, f2) and sg = (sigma(f0,f1), sigma(f1,f2), sigma(f2,f0)):
 *             1. side 0 only: when orient(f0, f1, f2, s) differs from the crossing sign of sg, s is not strictly beyond the facet: the walk
 *                ends (`sensor`); a cell other than the start cell is recorded with slot -1 and second = sqrt(e . e), e = s - p.
 *             2. dist = n . (q0 - p) / (n . d), n = (q1 - q0) x (q2 - q0) with q0, q1, q2 the vertices of c other than slot k in slot order,
 *                d = e / sqrt(e . e) per component, negated for side 1 (dgnn_vertex_rays' dist).  n . d == 0 or a non-finite dist: dist =
 *                the previous crossing's dist (0 before the first), counted in stats.
 *             3. a cell other than the start cell is recorded with slot k and second = dist; when the side's depth is non-zero and that many
 *                cells are recorded, the walk ends (`depth`).
 *             4. m = neighbors[c][k]; m == -1 ends the walk (`hull`); more than n_tets steps end it (`capped`).
 *             5. in m, w = its one vertex not in f (none or several: DGNN_E_INVALID).  a_i = sigma(w, f_i), i = 0, 1, 2.  The facet opposite
 *                f_i is (w, f_i+1, f_i+2) with the signs (a_i+1, sg_i+1, -a_i+2) (indices mod 3).  Not exactly one of the three crossed: the
 *                walk ends (`stuck`, m is not recorded).  Otherwise c = m, first = dist, k = the slot of f_i in m, f and sg = that facet and
 *                its signs; back to 1.
 *   records   one per recorded cell, in ascending (ray, side, step): cell, slot (-1 in the sensor's cell), first (the distance from p to the
 *             entry crossing = the dist of the cell before), second.  record_ids_out int32 [5, records_capacity] = ray, side, step, cell,
 *             slot and record_dist_out fp64 [2, records_capacity] = first, second (records_capacity == 0: not written; else it must hold
 *             every record).
 *   per cell  cell_count_out int32 [2, n_tets]; cell_stat_out fp64 [2, 6, n_tets] = min, max, sum of first, then of second, over the records
 *             of the cell on that side; slot_count_out int32 [2, n_tets, 4], slot_stat_out fp64 [2, 3, n_tets, 4] = the same of second over
 *             the records with that cell and slot >= 0 (edge row 4 c + k of the cell the ray LEAVES, as in `_fbvf`).  min and max are 0 where
 *             the count is 0; the sums add from 0.0 in ascending (ray, step).  No floating-point atomics: bit-identical from run to run and
 *             for every max_records.
 *   per lane  ray_status_out int32 [n_rays, 2]: 0 none, 1 sensor, 2 hull, 3 depth, 4 stuck, 5 capped; ray_cells_out int32 [n_rays, 2] = the
 *             recorded cells.
 *   stats_out DEVICE int64 [13]: rays used, skipped, perturbed (used rays with an axis term evaluated anywhere), orientation signs the exact
 *             stage decided, degenerate distances, the lanes per status (6, `none` includes the skipped rays' lanes), records, the longest
 *             lane's records.
 *   workspace the records are staged in ascending chunks of lanes that hold at most max_records records; DGNN_E_UNSUPPORTED when one lane has
 *             more (a lane never has more than n_tets + 1).  scratch: dgnn_ray_walk_scratch_bytes(n_rays, n_tets, n_vertices, max_records).
 *   DGNN_E_INVALID: an id out of range, an entry that is not a corner of the ray's vertex, non-finite coordinates, tetrahedra / neighbors not
 *   16-byte aligned; DGNN_E_UNSUPPORTED: n_rays >= 2^30, 8 n_tets or 2 max_records beyond int32, a non-zero coordinate magnitude of ANY
 *   vertex or sensor outside [2^-300, 2^300].
 * ---------------------------------------------------------------------------------------------- */
/* Stage times for benchmarks: stage_ms_out (HOST fp64 [4], may be NULL) receives the milliseconds spent since the last call of this function
 * in 0 the checks, the start cells and the counting walk, 1 the filling walk, 2 the sort, 3 the fold; then the sums are cleared and timing
 * is switched on or off (off at load).  While on, dgnn_ray_walk synchronises the stream at every stage boundary.  Not thread-safe. */
int dgnn_ray_walk_timing(int on, double* stage_ms_out);
int64_t dgnn_ray_walk_scratch_bytes(int64_t n_rays, int64_t n_tets, int64_t n_vertices, int64_t max_records);
int dgnn_ray_walk(const double* vertices, int64_t n_vertices, const int32_t* tetrahedra, int64_t n_tets, const int32_t* neighbors,
                  const int32_t* rowptr, const int32_t* entries, const int32_t* ray_vertex, const double* sensors, int64_t n_rays, int unique,
                  int64_t outside_depth, int64_t inside_depth, int64_t max_records, int32_t* ray_status_out, int32_t* ray_cells_out,
                  int32_t* cell_count_out, double* cell_stat_out, int32_t* slot_count_out, double* slot_stat_out, int64_t* stats_out,
                  int64_t records_capacity, int32_t* record_ids_out, double* record_dist_out, void* scratch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Occupancy of points in an arbitrary triangle mesh (reference utils/libmesh check_mesh_contains) and the generators of the
 * evaluation-sample builder (reference processing/<dataset>/sample_mesh.py).  DESIGN.md section 21.
 *
 * dgnn_mesh_contains: contains_out uint8 [n_points] = (above odd) & (below odd), n_disagree_out DEVICE int64 [1] = the points whose two
 *   parities differ (NULL: not written), for vertices fp64 [n_vertices, 3], faces int32 [n_faces, 3], points fp64 [n_points, 3].
 *   frame     per axis, over the vertices the faces reference: scale = (R - 1) / (max - min), translate = 0.5 - scale * min, R =
 *             hash_resolution in [2, 4096]; vertices and points are rescaled as scale * a + translate (a product, then a sum).
 *   rule      a rescaled point outside 0 <= p <= R on an axis (NaN included) is not contained.  Otherwise, over the triangles
 *             (t1, t2, t3) whose xy projection passes det = a00 a11 - a01 a10 != 0 with a00 = t1x - t3x, a01 = t2x - t3x, a10 = t1y - t3y,
 *             a11 = t2y - t3y, y = p - t3, u = (a11 y0 - a01 y1) sign(det), v = (-a10 y0 + a00 y1) sign(det), 0 < u, v, u + v < |det|:
 *             n = (t3 - t1) x (t2 - t1), depth = t1z |n2| + (n0 (t1x - px) + n1 (t1y - py)) sign(n2) (none when n2 == 0); the triangle
 *             is above when depth >= pz |n2|, below when depth < pz |n2|.
 *   grid      candidates come from an xy grid on int(coord) >> shift (cells clamped to [0, R - 1]); shift = the smallest for which the
 *             (triangle, cell) entries number at most max_entries.  The answer does not depend on it.  `entries` int32
 *             [entry_capacity] holds them: dgnn_mesh_contains_plan returns the number (n_entries_out, shift_out: HOST values).
 *   scratch   dgnn_mesh_contains_scratch_bytes(n_vertices, n_faces, hash_resolution) bytes for either call.
 * DGNN_E_INVALID: no faces, a face id out of range, a non-finite referenced vertex, no extent on an axis, entry_capacity too small;
 * DGNN_E_UNSUPPORTED: hash_resolution above 4096, max_entries below n_faces.  Ids are validated before any kernel indexes with them.
 * Both calls SYNCHRONISE `stream` three times (ids, box, entry totals).  Integer counts: bit-identical from run to run.
 *
 * dgnn_box_points:    points_out fp64 [n, 3], element j = boxsize * (u - 0.5), u = (mm_hash(seed, j + 1) >> 11) 2^-53.
 * dgnn_jitter_points: points_out[j] = points[j] + sigma * sqrt(-2 log u1) cos(2 pi u2) per element j (fp64), u1 = ((mm_hash(seed, 2 j + 1)
 *                     >> 11) + 1) 2^-53, u2 = (mm_hash(seed, 2 j + 2) >> 11) 2^-53.  In place allowed.
 * dgnn_face_normals:  normals_out fp64 [n_faces, 3] = (v1 - v0) x (v2 - v0) / its length; zeros for a face without area.  scratch: 256
 *                     bytes.  DGNN_E_INVALID: a face id out of range.  SYNCHRONISES `stream` once.
 * ---------------------------------------------------------------------------------------------- */
int64_t dgnn_mesh_contains_scratch_bytes(int64_t n_vertices, int64_t n_faces, int32_t hash_resolution);
int dgnn_mesh_contains_plan(const double* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int32_t hash_resolution,
                            int64_t max_entries, int32_t* shift_out, int64_t* n_entries_out, void* scratch, void* stream);
int dgnn_mesh_contains(const double* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int32_t hash_resolution,
                       int64_t max_entries, const double* points, int64_t n_points, uint8_t* contains_out, int64_t* n_disagree_out,
                       int32_t* entries, int64_t entry_capacity, void* scratch, void* stream);
int dgnn_box_points(int64_t n_points, double boxsize, uint64_t seed, double* points_out, void* stream);
int dgnn_jitter_points(const double* points, int64_t n_points, double sigma, uint64_t seed, double* points_out, void* stream);
int dgnn_face_normals(const double* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, double* normals_out, void* scratch,
                      void* stream);

/* ------------------------------------------------------------------------------------------------
 * Ground-truth cell labels: the share of each tetrahedron that lies inside a closed triangle mesh, by sampling (what the reference gets
 * from its external binary as <scene>_labels.npz inside_perc / outside_perc).  DESIGN.md section 26.  Every *, + and - below is one fp64
 * rounding, in the order written (no contraction).
 *
 * sample j (0 <= j < k = n_samples) of tet t: the 64-bit counter c = 3 ((tet_offset + t) k + j) + 1, wrapping mod 2^64, and
 *   s = u01(mm_hash(seed, c)), t = u01(mm_hash(seed, c + 1)), u = u01(mm_hash(seed, c + 2)), u01(h) = (h >> 11) 2^-53 (dgnn_box_points' draw);
 *   the unit cube folded onto the unit tet:
 *     if s + t > 1: s = 1 - s, t = 1 - t
 *     st = s + t
 *     if t + u > 1:        (s, t, u) <- (s, 1 - u, (1 - s) - t)
 *     else if st + u > 1:  (s, t, u) <- ((1 - t) - u, t, (st + u) - 1)
 *   the point, per coordinate, with e_i = p_i - p_0 over the vertices p_0..p_3 of the tet's `tetrahedra` row:
 *     x = ((s e_1 + t e_2) + u e_3) + p_0
 * A sample is inside exactly when dgnn_mesh_contains says so for x (the same frame, candidate grid, 2D test, depth and (above odd) &
 * (below odd)); a sample whose two parities differ counts as outside and is tallied in n_disagree.
 *
 * dgnn_tet_sample_points: points_out fp64 [n_tets n_samples, 3], row t k + j = sample j of tet t, for vertices fp64 [n_vertices, 3] and
 *   tetrahedra int32 [n_tets, 4].  scratch: dgnn_tet_sample_points_scratch_bytes() bytes.  SYNCHRONISES `stream` once (ids).
 * dgnn_cell_labels: count_out int32 [n_tets] = the inside samples of each tet (inside_perc = (double)count / (double)k, outside_perc =
 *   (double)(k - count) / (double)k), n_disagree_out DEVICE int64 [1] (NULL: not written).  The mesh arguments (mesh_vertices, faces,
 *   hash_resolution, max_entries, entries, entry_capacity) are dgnn_mesh_contains' and are planned the same way; scratch:
 *   dgnn_cell_labels_scratch_bytes(n_mesh_vertices, n_faces, hash_resolution) bytes.  No sample is written to memory and T k carries no int32
 *   limit (n_samples itself is at most 2^31 - 1); integer counts without atomics: bit-identical from run to run.  SYNCHRONISES `stream`
 *   four times (the plan's three, the tets' ids).
 * DGNN_E_INVALID: n_samples < 1, a tetrahedron's vertex id out of range (validated before any kernel indexes with it), and for
 * dgnn_cell_labels what dgnn_mesh_contains refuses.  n_tets == 0: nothing is written but n_disagree_out = 0.
 * ---------------------------------------------------------------------------------------------- */
int64_t dgnn_tet_sample_points_scratch_bytes(void);
int dgnn_tet_sample_points(const double* vertices, int64_t n_vertices, const int32_t* tetrahedra, int64_t n_tets, int64_t n_samples, uint64_t seed,
                           uint64_t tet_offset, double* points_out, void* scratch, void* stream);
int64_t dgnn_cell_labels_scratch_bytes(int64_t n_mesh_vertices, int64_t n_faces, int32_t hash_resolution);
int dgnn_cell_labels(const double* mesh_vertices, int64_t n_mesh_vertices, const int32_t* faces, int64_t n_faces, int32_t hash_resolution,
                     int64_t max_entries, int32_t* entries, int64_t entry_capacity, const double* vertices, int64_t n_vertices,
                     const int32_t* tetrahedra, int64_t n_tets, int64_t n_samples, uint64_t seed, uint64_t tet_offset, int32_t* count_out,
                     int64_t* n_disagree_out, void* scratch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * First hit of rays on a triangle mesh: the primitive of the virtual scanner (dgnn_amd/processing/scan_mesh.py; what the reference gets
 * from its external `scan` binary, processing/modelnet/scan.py, processing/shapenet/scan.py).  DESIGN.md section 27.  The binary's rule is
 * not known: this is this library's definition, not a reproduction.  Every *, +, - and / below is one fp64 rounding, in the order written (no
 * contraction); (a, b, c) . (d, e, f) means (a d + b e) + c f and a x b has one product minus one product per component.
 *
 * dgnn_ray_first_hit: for vertices fp64 [n_vertices, 3], faces int32 [n_faces, 3], origins and aims fp64 [n_rays, 3], t_min >= 0: ray r is
 *   o + t d with o = origins[r], g = aims[r], d = g - o.  It is unbounded: the aim is at t = 1.
 *   crossing  for face (a, b, c): s1 = sign det[g - o, a - o, b - o], s2 = sign det[g - o, b - o, c - o], s3 = sign det[g - o, c - o, a - o],
 *             each EXACT on the input coordinates (csrc/exact_orient.h orient_sign(o, g, x, y): an fp64 filter, then an exact expansion).
 *             The line crosses the face when the three are all >= 0 or all <= 0 and not all 0: a line in the face's plane crosses nothing, a
 *             line through a shared edge or vertex crosses every incident face, and no rounding opens a gap between two faces that share
 *             an edge.  A face without area or with a repeated id is never crossed.
 *   t         n = (b - a) x (c - a), t = (n . (a - o)) / (n . d).  A crossed face with n . d == 0 or a non-finite t is dropped and counted
 *             (stats 2); one with t <= t_min is dropped silently.
 *   result    the smallest t over the faces left, ties in t to the lowest face id: hit_face_out int32 [n_rays] (-1 = none), hit_t_out fp64
 *             [n_rays] (0 where none), hit_point_out fp64 [n_rays, 3] = o + t d per coordinate, one product and one sum (zeros where none;
 *             NULL: not written).  A ray with o == g is skipped: face -1, counted (stats 1).
 *   stats_out DEVICE int64 [4]: rays with a hit; rays skipped; crossings dropped as degenerate, every (ray, face) pair once, over all
 *             faces; the signs of the HIT faces (three per hit) that the exact stage decided.
 *   grid      candidates come from a uniform grid over the box of the referenced vertices: grid_resolution R in [1, 1024] cells along the
 *             longest axis, ceil(extent / (longest / R)) on the others (1 without extent); a face is entered in every cell its bounding box
 *             touches.  The whole line is walked through the box, every bound widened by 2^-46 of the largest coordinate magnitude of the box
 *             and the ray, and no hit is final before the walk ends: the set of tested faces contains every crossed face, and the
 *             result, a minimum under a total order, depends neither on R nor on the order of the entries.  `entries` int32
 *             [entry_capacity] holds the (face, cell) entries: dgnn_ray_first_hit_plan returns their number (n_entries_out, and the cells
 *             per axis in cells_out [3] when not NULL: HOST values).
 *   scratch   dgnn_ray_first_hit_scratch_bytes(n_faces, grid_resolution) bytes for either call.
 * DGNN_E_INVALID: no faces, a face id out of range, a non-finite coordinate of a referenced vertex, an origin or an aim (an unreferenced
 * vertex is not read), t_min < 0, entry_capacity too small; DGNN_E_UNSUPPORTED: a non-zero coordinate magnitude outside [2^-300, 2^300]
 * (the exact predicate's range), R outside [1, 1024], 2^31 or more entries.  Ids and coordinates are validated before any kernel uses
 * them.  Both calls SYNCHRONISE `stream` three times (ids, box and coordinates, entry total).  No floating-point atomics: bit-identical
 * from run to run.  One lane per ray; n_rays has no int32 limit.
 * ---------------------------------------------------------------------------------------------- */
int64_t dgnn_ray_first_hit_scratch_bytes(int64_t n_faces, int32_t grid_resolution);
int dgnn_ray_first_hit_plan(const double* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int32_t grid_resolution,
                            int64_t* n_entries_out, int32_t* cells_out, void* scratch, void* stream);
int dgnn_ray_first_hit(const double* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int32_t grid_resolution,
                       const double* origins, const double* aims, int64_t n_rays, double t_min, int32_t* hit_face_out, double* hit_t_out,
                       double* hit_point_out, int64_t* stats_out, int32_t* entries, int64_t entry_capacity, void* scratch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Distance from points to a triangle mesh, with the closest face: the primitive of the surface metrics (ops.surface_metrics: accuracy,
 * completeness, Hausdorff distance, F-score, normal consistency).  DESIGN.md section 30.  Every *, +, - and / below is one fp64 rounding, in
 * the order written (no contraction); x . y means (x0 y0 + x1 y1) + x2 y2 and x X y has one product minus one product per component.
 *
 * dgnn_point_mesh_distance: for vertices fp64 [n_vertices, 3], faces int32 [n_faces, 3], points fp64 [n_points, 3]: for every point p the
 *   lexicographic minimum over ALL faces f of (d2_f, f), with the closest point and the region of that face:
 *   segment   (u, v), taken with u the endpoint of the LOWER VERTEX ID (so two faces that share an edge or a vertex compute the same bits
 *             for it, and the tie goes to the lower face, not to the winding that happened to round lower): e = v - u, w = p - u,
 *             ee = e . e, we = w . e; we <= 0 or ee == 0: c = u; else we >= ee: c = v; else t = we / ee, c = u + t e per coordinate (one
 *             product, one sum).  d2 = (p - c) . (p - c).
 *   face      (v0, v1, v2): the segments (v0, v1), (v1, v2), (v2, v0) in this order, a later one replacing an earlier one only when its
 *             d2 is smaller.  Then the plane candidate: n = (v1 - v0) X (v2 - v0), nn = n . n; when nn > 0 and ((vj - vi) X (p - vi)) . n > 0
 *             for (i, j) = (0, 1), (1, 2), (2, 0): s = ((p - v0) . n) / nn, q = p - s n per coordinate (one product, one difference), c[k] =
 *             min(max(q[k], min_i vi[k]), max_i vi[k]) on the three axes k (the foot of the perpendicular, clamped to the face's bounding
 *             box: exactly onto the plane of an axis-aligned face), d2 = (p - c) . (p - c), and it replaces the segments' result when
 *             smaller (on equality the segment stays).  d2 is thus always the squared distance, as rounded, to the closest point that is
 *             reported, and that point lies in the face's bounding box (up to the rounding of u + t e) even where a sliver's computed
 *             normal is far from the true one: what the search's stopping bound rests on.  A face without area (collinear or repeated vertices) is its segments, a face of one repeated vertex that
 *             point; short of overflow nothing non-finite comes from finite input.
 *   region    of the winning candidate: 0 the face's interior (the plane candidate), 1..3 on the edge (v0 v1), (v1 v2), (v2 v0), 4..6 at
 *             vertex 0, 1, 2 (a segment clamped to an endpoint reports that endpoint's position in the face).
 *   outputs   d2_out fp64 [n], dist_out fp64 [n] = sqrt(d2), correctly rounded (NULL: not written), face_out int32 [n], closest_out fp64
 *             [n, 3], region_out uint8 [n].
 *   grid      grid_resolution R = 0: no grid, every lane tests every face.  R in [1, 1024]: a uniform grid over the box of the referenced
 *             vertices, R cells along the longest axis, ceil(extent / (longest / R)) on the others (1 without extent); a face is entered
 *             in every cell its bounding box touches.  One lane per point reads the cells in Chebyshev shells about the point's (clamped)
 *             cell and stops when its best d2 is below the squared distance, shrunk by 2^-46 of the largest coordinate magnitude of the box
 *             and the point, to every cell not yet read (csrc/meshdist.hip has the derivation): the result does not depend on R.
 *             `entries` int32 [entry_capacity] holds the (face, cell) entries: dgnn_point_mesh_distance_plan returns their number (0 for
 *             R = 0, where entries may be NULL).
 *   stats_out DEVICE int64 [4]: the grid's entries; the most shells one point read; the shells read in total; the (point, face)
 *             evaluations (R = 0: n_points * n_faces).  A point deep inside an empty region, at about the same distance from much of the
 *             mesh, reads nearly the whole grid (O(R^3) cells): for such queries R = 0 is the faster call.
 *   scratch   dgnn_point_mesh_distance_scratch_bytes(n_faces, grid_resolution) bytes for either call.
 * DGNN_E_INVALID: no faces, a face id out of range, a non-finite coordinate of a referenced vertex or of a point (an unreferenced vertex
 * is not read), entry_capacity too small; DGNN_E_UNSUPPORTED: R outside [0, 1024], 2^31 or more entries.  No exact predicate is involved:
 * there is no coordinate-range refusal.  Ids and coordinates are validated before any kernel uses them.  Both calls SYNCHRONISE `stream`
 * twice (ids, box and coordinates), three times with a grid (the entry total).  No floating-point atomics: bit-identical from run to run.
 * n_points == 0 is fine (the mesh is still validated).
 *
 * dgnn_distance_fold: for dist fp64 [n], cosine fp64 [n] or NULL, thresholds fp64 [n_thresholds] (all DEVICE): sums_out DEVICE fp64 [3] =
 *   the sum of dist, the sum of |cosine| (0 for NULL), the maximum of dist (0 for n == 0), the sums in fixed_sum.h's order (serial sums over
 *   chunks of 256 elements, then the chunk totals serially); counts_out DEVICE int64 [n_thresholds] = #{i: dist[i] <= thresholds[t]}
 *   (integer sums: order-free).  scratch: dgnn_distance_fold_scratch_bytes(n) bytes.  Bit-identical from run to run.
 *
 * dgnn_row_dot3: out[i] = a[ia[i]] . b[ib[i]] for a fp64 [n_a, 3], b fp64 [n_b, 3], ia, ib int32 [n] (the cosine between a sample's face
 *   normal and its closest face's normal).  DGNN_E_INVALID for an index out of range (validated first: SYNCHRONISES once).  scratch: 256 bytes.
 * ---------------------------------------------------------------------------------------------- */
int64_t dgnn_point_mesh_distance_scratch_bytes(int64_t n_faces, int32_t grid_resolution);
int dgnn_point_mesh_distance_plan(const double* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int32_t grid_resolution,
                                  int64_t* n_entries_out, void* scratch, void* stream);
int dgnn_point_mesh_distance(const double* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int32_t grid_resolution,
                             const double* points, int64_t n_points, double* d2_out, double* dist_out, int32_t* face_out, double* closest_out,
                             uint8_t* region_out, int64_t* stats_out, int32_t* entries, int64_t entry_capacity, void* scratch, void* stream);
int64_t dgnn_distance_fold_scratch_bytes(int64_t n);
int dgnn_distance_fold(const double* dist, const double* cosine, int64_t n, const double* thresholds, int32_t n_thresholds, double* sums_out,
                       int64_t* counts_out, void* scratch, void* stream);
int dgnn_row_dot3(const double* a, int64_t n_a, const int32_t* ia, const double* b, int64_t n_b, const int32_t* ib, int64_t n, double* out,
                  void* scratch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The k nearest neighbours of every query among a set of points, exactly, and the scan operations on the lists: the mean neighbour
 * distance, the statistical outlier mask, PCA normals (ops.knn, ops.knn_mean_distance, ops.outlier_mask, ops.estimate_normals).  DESIGN.md
 * section 34.  Every *, +, -, / and sqrt below is one fp64 rounding, in the order written (no contraction).
 *
 * dgnn_knn: points fp64 [n_points, 3], queries fp64 [n_queries, 3] or NULL, 1 <= k <= 64.  For a query q and a point j:
 *   dx = q.x - p_j.x, dy = q.y - p_j.y, dz = q.z - p_j.z, d2 = (dx dx + dy dy) + dz dz.
 *   answer    row i of idx_out int32 [Q, k] and d2_out fp64 [Q, k] = the k smallest of ALL (d2_j, j) in lexicographic order, ascending.
 *             queries == NULL: the queries are the points themselves (Q = n_points, n_queries is not read) and query i leaves out point i BY
 *             INDEX, not by distance: a duplicate of a point is its neighbour at d2 = 0.  With queries nothing is left out.  Where fewer
 *             than k points qualify the row ends in idx = -1, d2 = +inf.  Row offsets are int64: Q k has no int32 limit.
 *   grid      grid_resolution R = 0: no grid; tiles of 256 points pass through LDS and every query meets every point.  R in [1, 1024]: a
 *             uniform grid over the box of the points, R cells along the longest axis, ceil(extent / (longest / R)) on the others (1
 *             without extent), the cell of a coordinate x on axis a being trunc((x - lo_a) inv_a) clamped to the grid; the points are
 *             binned as (x, y, z, index) records.  One wavefront per query keeps the sorted list one entry per lane, reads the cells in
 *             Chebyshev shells about the query's (clamped) cell and stops when the list is full and its k-th d2 is strictly below the
 *             squared distance, shrunk by 2^-46 of the largest coordinate magnitude of the box and the query, to every cell not yet read
 *             (csrc/knn.hip has the derivation); a list that is not full reads on to the last shell.  The result does not depend on R.
 *   stats_out DEVICE int64 [3], summed over the call: shells read (R = 0: 0); candidates evaluated = the records of the cells read, the
 *             query's own included (R = 0: Q n_points); survivors placed in a list.
 *   scratch   dgnn_knn_scratch_bytes(n_points, grid_resolution) bytes.
 * DGNN_E_INVALID: k outside [1, 64], a non-finite coordinate of a point or of a query (validated before any kernel uses them: the call
 * SYNCHRONISES `stream` once); DGNN_E_UNSUPPORTED: R outside [0, 1024], n_points or Q >= 2^31 - 1.  No floating-point atomics and a total
 * order: bit-identical from run to run, whatever order the bins were filled in.
 *
 * dgnn_knn_mean_distance: d2 fp64 [n, k], idx int32 [n, k] (dgnn_knn's) -> mean_out fp64 [n]: s = 0, then s = s + sqrt(d2[i, r]) over the
 *   entries with idx[i, r] >= 0 in rank order r, divided by their number (as a double; none: 0 / 0).
 *
 * dgnn_outlier_mask: mean_distance fp64 [n], n >= 2 (DEVICE) -> mu = S(m) / n, sigma = sqrt(S((m_i - mu) (m_i - mu)) / n), threshold = mu +
 *   std_ratio sigma (one product, one sum), keep_out uint8 [n] = m_i <= threshold; values_out DEVICE fp64 [3] = mu, sigma, threshold;
 *   n_removed_out DEVICE int64 [1].  S is fixed_sum.h's sum: serial sums over chunks of 256 elements, then the chunk totals serially.
 *   PCL / Open3D's statistical outlier removal with the population deviation.  scratch: dgnn_outlier_mask_scratch_bytes(n) bytes.
 *
 * dgnn_knn_normals: points fp64 [n, 3], idx int32 [n, k] with entries in [-1, n) (validated first: SYNCHRONISES once), sensors fp64 [n, 3] or
 *   NULL -> normals_out fp64 [n, 3], eigenvalues_out fp64 [n, 3].  One lane per point.  The neighbourhood of point i is the point itself, then
 *   the points idx[i, r] >= 0 in rank order; m is their number, as a double.  Every sum below runs over the neighbourhood in that order, serially.
 *   centroid  c = (sum p) / m per coordinate.
 *   sums      with d = p - c: a00 = sum dx dx, a11 = sum dy dy, a22 = sum dz dz, a01 = sum dx dy, a02 = sum dx dz, a12 = sum dy dz (not
 *             divided by m), the symmetric matrix A; V = the identity.
 *   Jacobi    SIX cyclic sweeps over (p, q) = (0, 1), (0, 2), (1, 2), r the third index.  A rotation with a_pq == 0.0 is skipped.  Else
 *             theta = (a_qq - a_pp) / (2 a_pq); t = sign / (|theta| + sqrt(theta theta + 1)) with sign = 1 for theta >= 0, else -1 (theta
 *             theta overflowing to inf gives t = 0); c = 1 / sqrt(t t + 1); s = t c; then, all from the old values,
 *               a_pp = a_pp - t a_pq;  a_qq = a_qq + t a_pq;  a_rp = c a_rp - s a_rq;  a_rq = s a_rp + c a_rq;  a_pq = 0;
 *               v_ip = c v_ip - s v_iq;  v_iq = s v_ip + c v_iq   for the rows i = 0, 1, 2 of V.
 *             Six is a count, not a tolerance: fixed-sweep Jacobi reaches its floor at four (DESIGN section 34 has the measurement).
 *   normal    the column of V at the smallest diagonal entry of A (ties: the lower column), each component divided by the column's length
 *             sqrt((x x + y y) + z z); negated when its component of largest magnitude (ties: the lowest axis) is negative; then, with
 *             sensors, negated when (n.x t.x + n.y t.y) + n.z t.z < 0 for t = sensor_i - p_i: the rule of scan_mesh's own normals.
 *   eigenvalues  the three diagonal entries ascending, ties by column.
 *   Only + - * / sqrt are used, each correctly rounded on the device and in numpy: tests/knn_model.py agrees bit for bit.  scratch: 256 bytes.
 * ---------------------------------------------------------------------------------------------- */
int64_t dgnn_knn_scratch_bytes(int64_t n_points, int32_t grid_resolution);
int dgnn_knn(const double* points, int64_t n_points, const double* queries, int64_t n_queries, int32_t k, int32_t grid_resolution,
             int32_t* idx_out, double* d2_out, int64_t* stats_out, void* scratch, void* stream);
int dgnn_knn_mean_distance(const double* d2, const int32_t* idx, int64_t n, int32_t k, double* mean_out, void* stream);
int64_t dgnn_outlier_mask_scratch_bytes(int64_t n);
int dgnn_outlier_mask(const double* mean_distance, int64_t n, double std_ratio, uint8_t* keep_out, double* values_out, int64_t* n_removed_out,
                      void* scratch, void* stream);
int dgnn_knn_normals(const double* points, int64_t n, const int32_t* idx, int32_t k, const double* sensors, double* normals_out,
                     double* eigenvalues_out, void* scratch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Subsampling a scan before it is triangulated: one point per occupied voxel, and exact minimum-distance (Poisson-disk) thinning
 * (ops.voxel_subsample, ops.min_distance_thin).  DESIGN.md section 35.  Every *, +, -, / below is one fp64 rounding, in the order written (no
 * contraction); d2 is dgnn_knn's.  Both results depend on the input alone: bit-identical from run to run.
 *
 * dgnn_voxel_subsample: points fp64 [n, 3], the voxel's edge h, origin HOST fp64 [3].
 *   voxel     c_a = floor((x_a - o_a) / h) per axis a; a point's voxel is (c_x, c_y, c_z).  A point ON a voxel face belongs to the voxel above.
 *   numbering voxel v is the one whose lowest member index is the v-th smallest ("numbered by first member").
 *   outputs   for m occupied voxels (every array has room for n rows; rows >= m are not written): voxel_out int32 [n] the point's voxel row;
 *             count_out int32 [m]; first_out int32 [m] the lowest member; centroid_out fp64 [m, 3]; nearest_out int32 [m]; m_out DEVICE int64 [1].
 *   centroid  per axis S(x) / count (count as a double) over the members in ascending index; S is fixed_sum.h's sum: s = 0, s = s + x over a
 *             chunk of 256 members, total = 0, total = total + s over the chunks in order (at most 256 members: a plain left-to-right sum).
 *   nearest   the member with the smallest (d2, index), d2 = (dx dx + dy dy) + dz dz, dx = centroid.x - p.x and so on (where every d2 is a
 *             NaN, the sums having overflowed both ways: the first member).
 *   scratch   dgnn_voxel_subsample_scratch_bytes(n) bytes.  n = 0: m = 0.
 * DGNN_E_INVALID, nothing written: h not finite or <= 0, a non-finite origin, a non-finite coordinate, any |c_a| >= 2^20 (the triple is a
 * 63-bit key: three fields of 21 bits); the points are validated before anything is written: the call SYNCHRONISES `stream` once.
 * DGNN_E_UNSUPPORTED: n >= 2^31 - 1.  The voxels are found by a stable radix sort of (key, index); no result depends on an atomic's order.
 *
 * dgnn_min_distance_thin: points fp64 [n, 3], radius r finite and >= 0, priority int64 [n] or NULL, seed.
 *   conflict  r2 = r r; i and j conflict iff d2(i, j) < r2 (d2 == r2 is no conflict; r = 0 keeps everything, duplicates included).
 *   order     by (key_i, i), lexicographic.  With a priority key_i = priority[i], signed, lower first; without one
 *             key_i = mix(mix(seed + 0x9E3779B97F4A7C15) + i) modulo 2^64, compared unsigned, mix the splitmix64 finaliser
 *             z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31.
 *   answer    walk the points in that order and keep a point iff it conflicts with no point kept before it: the lexicographically first
 *             maximal independent set of the conflict graph.  keep_out uint8 [n].
 *   rounds    computed in parallel rounds over the undecided points (one wavefront each): an earlier conflicting point kept -> removed; none
 *             undecided -> kept; else the point waits.  The earliest undecided point is decided in every round.  With the hashed key the
 *             number of rounds is O(log n) with high probability; a priority can make a chain as long as n.
 *   grid      grid_resolution R = 0: all pairs, tiles of 256 points through LDS.  R in [1, 1024]: dgnn_knn's grid and records; a point reads
 *             the cells of x_a - r' .. x_a + r' on each axis, r' = r (1 + 2^-46) (csrc/scansub.hip has the count).  The answer does not depend
 *             on R, cells smaller than r included.
 *   stats_out DEVICE int64 [3]: the points kept; the rounds that had an undecided point; candidates evaluated = the records (R = 0: points)
 *             read, summed over the rounds.
 *   scratch   dgnn_min_distance_thin_scratch_bytes(n, grid_resolution) bytes.  n = 0: nothing kept, no round.
 * DGNN_E_INVALID, nothing written: r not finite or < 0, a non-finite coordinate.  DGNN_E_UNSUPPORTED: R outside [0, 1024], n >= 2^31 - 1.
 * The call SYNCHRONISES `stream` once for the validation and once per four rounds.
 * ---------------------------------------------------------------------------------------------- */
int64_t dgnn_voxel_subsample_scratch_bytes(int64_t n);
int dgnn_voxel_subsample(const double* points, int64_t n, double h, const double* origin, int32_t* voxel_out, int32_t* count_out, int32_t* first_out,
                         double* centroid_out, int32_t* nearest_out, int64_t* m_out, void* scratch, void* stream);
int64_t dgnn_min_distance_thin_scratch_bytes(int64_t n, int32_t grid_resolution);
int dgnn_min_distance_thin(const double* points, int64_t n, double radius, const int64_t* priority, uint64_t seed, int32_t grid_resolution,
                           uint8_t* keep_out, int64_t* stats_out, void* scratch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-scene standardisation (reference processing/data.py:444-506 sklearn StandardScaler + :512-519
 * float32 cast): out[i,c] = float((x[i,c] - mean_c) / std_c) for c >= c_first, plain cast for c < c_first;
 * fp64 statistics (population variance, zero scale -> 1).  scratch: dgnn_standardize_scratch_doubles(c) doubles.
 * ---------------------------------------------------------------------------------------------- */
int64_t dgnn_standardize_scratch_doubles(int c);
int dgnn_standardize_f64(const double* x, int64_t ld, int64_t n, int c, int c_first, float* out, int64_t ldo, double* scratch,
                         void* stream);

/* ------------------------------------------------------------------------------------------------
 * Feature scaling with the reference's pre-steps and all of its scalers (processing/data.py:444-506, then the float32 cast).
 * Every pass reads v = the pre-transformed value, in fp64, in this order (an empty column range c0 >= c1 switches a step off):
 *   sum     v = (x*1000)/colsum             columns [sum_c0, sum_c1)
 *   div     v = v/(x[row, div_col] + 1e-4)  columns [div_c0, div_c1); the divisor is taken after `sum`, before `div`
 *   scalar  v = v/div_scalar                columns [sc_c0, sc_c1)
 * kind (fitted on columns >= c_first; columns below are pre-transformed and cast): 0 none, 1 standard (StandardScaler),
 * 2 minmax (MinMaxScaler onto [range_lo, range_hi]), 3 robust (RobustScaler: exact median and quartiles by radix selection,
 * numpy's linear quantile rule).  A scale below 10 eps becomes 1.  stats (optional, device fp64 [2][c]): what was subtracted and
 * what was divided by (minmax: data_min and the zero-handled data_range; columns < c_first: 0 and 1).  Non-finite inputs are out
 * of scope.  n < 2^32.  Integer counts only: reruns are bit-identical.  scratch: dgnn_scale_features_scratch_bytes(c) bytes.
 * ---------------------------------------------------------------------------------------------- */
int64_t dgnn_scale_features_scratch_bytes(int c);
int dgnn_scale_features_f64(const double* x, int64_t ld, int64_t n, int c, int c_first, int kind, double range_lo, double range_hi,
                            int sum_c0, int sum_c1, int div_col, int div_c0, int div_c1, double div_scalar, int sc_c0, int sc_c1,
                            float* out, int64_t ldo, double* stats, void* scratch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Ingest-time cell locality order (sits where the reference builds edge_index, processing/data.py:434-438).
 * CGAL writes the cells in insertion order (the 4 neighbours of a cell are tens of thousands of rows apart); the loader relabels them once
 * per scene so that the conv layers' neighbour gathers hit L2, and keeps the permutation for the places where per-cell results leave
 * (dataLoader.exportScore, generate_mesh.generate :75-81).  All int32 index work, deterministic:
 *   dgnn_cell_centroids_3dt  centroids [n,3] from <scene>_3dt.npz: `vertices` fp32 [n_vertices,3], `tetrahedra` int32 [n_finite,4] = the
 *                            FINITE cells in file order (generate_mesh.py:78-81 relies on the same correspondence); `infinite` int32 [n]
 *                            (labels.npz, :202-208); an infinite cell takes its finite neighbour's centroid (edge_index rows 4i..4i+3).
 *                            scratch: dgnn_cell_centroids_scratch_elems(n) int32
 *   dgnn_cell_order_morton   order[i] = old id of new cell i (cells sorted, stable, by the 48-bit Morton code of their centroid: 16 bits per
 *                            axis over the bounding box), rank = its inverse.  scratch (8-byte aligned): dgnn_cell_order_morton_scratch_elems(n) int32
 *   dgnn_cell_order_bfs      the same from the adjacency alone (no coordinates): breadth-first order, every level in the order a serial
 *                            queue produces (first discoverer wins, neighbours in slot order), components started at their lowest cell id.
 *                            Reference layout required (row 4t+k leaves cell t).  SYNCHRONISES `stream` once per level (ingest-time call).
 *                            scratch: dgnn_cell_order_bfs_scratch_elems(n) int32
 *   dgnn_reorder_edges_ref   relabelled adjacency: pairs_out int64 [4n,2] = (new src, new dst) of new edge row e = old row 4*order[e/4] + e%4,
 *                            i.e. the reference layout again (its transposed [2,4n] view with strides (1,2) is what dgnn_plan_build's
 *                            REFERENCE fast path takes); edge_rows_out int32 [4n] = that old row (gathers edge_attr with dgnn_gather_rows_f32).
 *                            A source that is not the reference layout raises the asynchronous index error.
 * ---------------------------------------------------------------------------------------------- */
int64_t dgnn_cell_centroids_scratch_elems(int64_t n);
int dgnn_cell_centroids_3dt(const float* vertices, int64_t n_vertices, const int32_t* tetrahedra, int64_t n_finite, const int32_t* infinite,
                            const int64_t* edge_index, int64_t stride_row, int64_t stride_col, int64_t n, float* centroids, int32_t* scratch,
                            void* stream);
int64_t dgnn_cell_order_morton_scratch_elems(int64_t n);
int dgnn_cell_order_morton(const float* centroids, int64_t n, int32_t* order, int32_t* rank, int32_t* scratch, void* stream);
int64_t dgnn_cell_order_bfs_scratch_elems(int64_t n);
int dgnn_cell_order_bfs(const int64_t* edge_index, int64_t stride_row, int64_t stride_col, int64_t n, int32_t* order, int32_t* rank,
                        int32_t* scratch, void* stream);
int dgnn_reorder_edges_ref(const int64_t* edge_index, int64_t stride_row, int64_t stride_col, int64_t n, const int32_t* order,
                           const int32_t* rank, int64_t* pairs_out, int32_t* edge_rows_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Partitioned scene: per-layer halo exchange over RCCL (what replaces the reference's k-hop recomputation for scenes that do not
 * fit one pass, learning/surfaceNetStaticEdgeFilters.py:232-275 / run.py:221-223).  A rank's activation buffer is [n_own + n_halo, C]: owned
 * rows first, then the halo rows grouped by owner rank.  Before conv layer l >= 1:
 *   dgnn_halo_exchange_start  packs x[send_idx] on `stream`, then -- on the plan's own side stream, ordered behind the pack by an event -- ONE
 *                             group of ncclRecv (straight into the buffer's tail) and ncclSend (every GPU pair of an MI355X node has a direct xGMI
 *                             link: single-hop neighbour exchange, no ring)
 *   dgnn_halo_exchange_wait   makes `stream` wait for the received rows
 * Launches queued on `stream` between the two (the interior cells) overlap the transfer.  Rows are `elem_bytes` (2 or 4) x C bytes, whole 4-byte
 * words; send_buf: dgnn_halo_send_rows(plan) * C * elem_bytes bytes, caller-owned, reusable after the wait.  send_idx (device int32, caller-owned,
 * must outlive the plan): local ids of the owned rows to send, grouped by destination rank; send_counts / recv_counts: host arrays [world].
 * `comm`: an ncclComm_t -- the caller's, or one made by dgnn_comm_create from the 128-byte id of dgnn_comm_unique_id (rank 0 asks, the host
 * broadcasts it over its own channel, every rank creates on its current device).  RCCL is resolved at run time (DGNN_RCCL_LIB, an already
 * loaded librccl, the loader's path): dgnn_rccl_available() == 0 and DGNN_E_UNSUPPORTED from these entry points where there is none.
 * What goes over a link is ONE message of rows * C * elem_bytes per peer and direction, whatever either side's row stride: with ld == C it lands in
 * the tail directly and nothing allocates or synchronises the host; with ld != C it lands in a receive staging area owned by the plan (allocated on
 * first use, grown on demand, freed by dgnn_halo_plan_destroy) and is spread into the strided tail by a copy kernel on the side stream.
 * A rank may be its own peer (RCCL allows self send / recv inside a group).  dgnn_comm_count: ncclCommCount of `comm` (the number of ranks the
 * communicator spans: what a benchmark line reports as the RCCL world size), negative error code on failure.
 * ---------------------------------------------------------------------------------------------- */
typedef struct dgnn_halo_plan dgnn_halo_plan;
int dgnn_rccl_available(void);
int dgnn_comm_unique_id(void* id128);
int dgnn_comm_create(const void* id128, int rank, int world, void** comm_out);
int dgnn_comm_destroy(void* comm);
int dgnn_comm_count(void* comm);
int dgnn_halo_plan_create(int rank, int world, int64_t n_own, const int32_t* send_idx, const int64_t* send_counts, const int64_t* recv_counts,
                          dgnn_halo_plan** out);
int dgnn_halo_plan_destroy(dgnn_halo_plan* plan);
int64_t dgnn_halo_send_rows(const dgnn_halo_plan* plan);
int64_t dgnn_halo_recv_rows(const dgnn_halo_plan* plan);
int dgnn_halo_exchange_start(dgnn_halo_plan* plan, void* comm, void* x, int64_t ld, int C, int elem_bytes, void* send_buf, void* stream);
int dgnn_halo_exchange_wait(dgnn_halo_plan* plan, void* stream);

/* ------------------------------------------------------------------------------------------------
 * One rank's part of a scene cut across GPUs, ONE call per step (what replaces the reference's k-hop recomputation at
 * learning/surfaceNetStaticEdgeFilters.py:232-275 for a scene larger than -- or, strong scaling, spread over more than -- one GPU).
 * dgnn_static_infer_fwd for the LOCAL bipartite graph of a part: n_own owned cells (the first n_interior of them neither read a halo row nor are
 * sent to a peer) + n_halo halo rows behind them; x [n_own + n_halo, widths[0]] with the halo's input rows resident; the local edge list has
 * destinations < n_own and sources < n_own + n_halo.  Launch chain (dgnn_amd/partition.py run_partitioned_layers, now inside the library):
 *   plan of the local graph (edge_index != NULL; n_key = n_own, n_other = n_own + n_halo) -> layer 0 over the owned cells ->
 *   per layer l >= 1: interior cells [0, n_interior) | dgnn_halo_exchange_wait | boundary cells [n_interior, n_own)
 *   behind every layer but the last: dgnn_halo_exchange_start on its output rows [n_own + n_halo, widths[l+1]] (fp32, packed)
 *   last layer: both launches carry the decoder where dgnn_static_infer_fwd's would; logits [n_own, n_logits]
 * attr_in_plan_order != 0: edge_attr rows are already grouped by destination (a part's local list is): the layers read them in place, eid is
 * only written by the plan build.  halo == NULL (n_halo must be 0): a single-rank part, no exchange.  send_buf: dgnn_halo_send_rows(halo) *
 * max(widths[1..L-1]) * 4 bytes.  workspace: dgnn_static_infer_workspace_bytes(n_own + n_halo, n_layers, widths).  Same kernels, ranges and
 * order as the per-layer calls: the union of the ranks' logits is bit-identical to dgnn_static_infer_fwd on the whole scene.
 * Nothing allocates or synchronises; DGNN_E_UNSUPPORTED before anything is launched for shapes outside the fused kernels.
 * ---------------------------------------------------------------------------------------------- */
int dgnn_static_infer_partitioned_fwd(const int64_t* edge_index, int64_t stride_row, int64_t stride_col, int64_t E, int plan_hint, int32_t* rowptr,
                                      int32_t* src, int32_t* eid, int32_t* plan_scratch, int attr_in_plan_order, int64_t n_own, int64_t n_interior,
                                      int64_t n_halo, const float* x, int64_t ldx, const float* edge_attr, int64_t lde, int f_e, int n_layers,
                                      const int32_t* widths, const float* const* We, const float* const* be, const float* const* Wj,
                                      const float* const* bj, const float* const* Wi, const float* const* scale, const float* const* shift,
                                      const void* const* prepared, const float* W0, const float* b0, const float* scale1, const float* shift1,
                                      int c_hidden, const float* W3, const float* b3, int n_logits, int fuse_decoder, int gemm_mode,
                                      dgnn_halo_plan* halo, void* comm, void* send_buf, void* workspace, float* logits, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Wide conv layers on SPLIT ROWS (round 5; csrc/wide.hip).  SAGEConv.forward (learning/surfaceNetStaticEdgeFilters.py:66-96) at the widths the
 * reference's real configs use (configs/eth.yaml:56, aerial.yaml:57: [64,128,256,512]; configs/modelnet.yaml:56: [128,256,512,1024]): layers
 * with C_in in {128, 256, 512} and C_out a multiple of 256 -- outside dgnn_sage_layer_fused_fwd's shapes -- as
 *     dgnn_sage_aggregate_sr   a = mean_j x_j * lin_e(edge_attr_j)                       (:75-80, :89-96)
 *     dgnn_linear_sr           act(([a | x_i] . [Wj | Wi]^T + bj) * scale + shift)       (:81-86 + BatchNorm(eval) + ReLU; also the decoder's first Linear)
 * with every wide activation stored in HBM as SPLIT ROWS: a row of C channels (C % 32 == 0) is C / 32 chunks of 128 bytes; chunk q holds, for its 32
 * positions p, hi[p] (fp16, bytes 2p) and lo[p] (fp16, bytes 64 + 2p) of x * s for channel 32 q + PI(p), PI(p) = (p & 3) | (p >> 4) << 2 |
 * ((p >> 2) & 3) << 3, hi = RN16(x s), lo = RN16(x s - hi) (22 significand bits in 4 bytes); s is a power of two per row and GROUP of 256 channels
 * (`scales` [rows][ceil(C / 256)] fp32) that puts the group's largest magnitude into [2^14, 2^15); a group below 2^-112 is stored as zeros with
 * s = 2^127.  dgnn_sr_row_bytes(C) = C / 32 * 128.  The format is what the fp16 two-part matrix products consume (3 products per fp32 product,
 * fp32 accumulation: fp32-class results, tests/test_gpu_wide.py), written by the kernel that PRODUCES the activation: no row-scale pass, no
 * split instructions and no fp32 staging in the consumer.  dgnn_sr_pack / dgnn_sr_unpack convert from / to fp32 rows (weights at prepare time,
 * boundaries, tests).  All pointers 16-byte aligned; nothing allocates or synchronises.
 * ---------------------------------------------------------------------------------------------- */
int64_t dgnn_sr_row_bytes(int C);
/* fp32 rows [rows][k1 (+ k2)] (k1, k2 multiples of 32) -> split rows dst [rows][dst_row_bytes] + scales [rows][ng]; gch = chunks per scale group:
 * 8 for activations (ng = ceil(chunks / 8)), 0 = ONE group per row (ng = 1): the weights of dgnn_linear_sr are [Wj | Wi] packed with gch = 0 */
int dgnn_sr_pack(const float* A1, int64_t ld1, int k1, const float* A2, int64_t ld2, int k2, int64_t rows, int gch, void* dst,
                 int64_t dst_row_bytes, float* scales, int ng, void* stream);
int dgnn_sr_unpack(const void* src, int64_t row_bytes, const float* scales, int ng, int gch, int C, int64_t rows, float* out, int64_t ldo,
                   void* stream);
/* the filter operand [We^T ; be] of dgnn_sage_aggregate_sr, prepared once per set of weights (C in {128, 256, 512}; 0 bytes = unsupported width) */
int64_t dgnn_sr_filter_prepared_bytes(int C);
int dgnn_sr_prepare_filter(const float* We, const float* be, int C, void* buf, void* stream);
/* a_out / a_scales: split rows of a [n_dst][C].  x: the source rows, split rows (x_is_sr != 0, xs their scales) or fp32 rows (row stride ldx floats);
 * with fp32 rows and x_out != NULL the destinations' own rows x[:n_dst] are also written as split rows (x_out, x_scales).  edge_attr: fp32 packed
 * [E][20] rows, gathered by eid (NULL: plan order).  Any in-degree (4-regular groups take the matrix-core path).  DGNN_E_UNSUPPORTED before anything
 * is launched for other widths / layouts. */
int dgnn_sage_aggregate_sr(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int64_t n_dst, const void* x, int x_is_sr, int64_t ldx,
                           const float* xs, int C, const float* edge_attr, int64_t lde, const float* We, const float* be, const void* prep, void* a_out,
                           float* a_scales, void* x_out, float* x_scales, void* stream);
/* A1 (C1 channels) and A2 (C2 channels; NULL / 0: one operand) split rows with their scales; Wp / sw = dgnn_sr_pack([W1 | W2] fp32 [n_out][C1 + C2],
 * gch = 0); n_out a multiple of 256.  Exactly ONE output: split rows (out_sr, out_row_bytes, out_scales [M][n_out / 256]); fp32 rows out_f32
 * [M][n_out] with row stride ldo; or logits [M][n_proj] = act(...) . W3^T + b3 (W3 fp32 [n_proj][n_out], n_proj 1 or 2: the decoder's output
 * Linear applied to the finished hidden rows inside the launch, reference :180-187; n_out > 256: logits must be ZERO on entry, the column tiles
 * add into them -- two addends per logit at n_out = 512, an order-independent sum; n_out > 512 is declined).  DGNN_E_UNSUPPORTED for other shapes. */
int dgnn_linear_sr(const void* A1, int64_t row_bytes1, const float* scales1, int C1, const void* A2, int64_t row_bytes2, const float* scales2, int C2,
                   const void* Wp, const float* sw, const float* bias, const float* scale, const float* shift, int relu, int64_t M, int n_out, void* out_sr,
                   int64_t out_row_bytes, float* out_scales, float* out_f32, int64_t ldo, const float* W3, const float* b3, int n_proj, float* logits,
                   void* stream);

/* elementwise helpers used by the Updated variant (F.relu at surfaceNetUpdatedEdgeFilters.py:239-241
 * and the scatter of phi rows into the zero [E_all,C] buffer at :236-237) */
int dgnn_relu(const float* x, int64_t n, float* y, void* stream);
int dgnn_relu_bwd(const float* y, const float* g, int64_t n, float* out, void* stream); /* out = g * [y > 0] */
int dgnn_scatter_rows_f32(const float* in, int64_t ld_in, const int64_t* idx, int64_t n, int cols, float* out,
                          int64_t ld_out, void* stream);

/* ---- exact in-sphere predicate, 3D Delaunay triangulation and its certificate (csrc/exact_insphere.h, csrc/delaunay.hip) ----
 *
 * dgnn_insphere_sign: points5 fp64 [n, 5, 3] (a, b, c, d, e per case) -> sign_out int8 [n]: +1 when e lies strictly inside the sphere through
 *   a, b, c, d, 0 on it, -1 outside, for any non-flat a..d; 0 for flat (coplanar) a..d.  With L the determinant of the rows
 *   [x y z x^2+y^2+z^2 1] of a..e the result is -sign(L) * sign(det[b - a, c - a, d - a]), both signs exact.
 *   filter  every +, - and * below is one fp64 operation (no contraction).  p' = p - e for p = a..d (12 differences);
 *           ab = a'x b'y - b'x a'y, and bc, cd, da, ac, bd likewise; abc = a'z bc - b'z ac + c'z ab, bcd = b'z cd - c'z bd + d'z bc,
 *           cda = c'z da + d'z ac + a'z cd, dab = d'z ab + a'z bd + b'z da; lift(p) = p'x p'x + p'y p'y + p'z p'z;
 *           L~ = (lift(d) abc - lift(c) dab) + (lift(b) cda - lift(a) bcd).  The permanent is the same expression with every product taken by
 *           magnitude and every difference replaced by a sum.  sign(L~) is returned when |L~| > (16 + 224 eps) eps permanent + 2^-600,
 *           eps = 2^-53; the derivation of both terms is in csrc/exact_insphere.h.
 *   exact   otherwise L is summed exactly on the raw coordinates: 360 products of five coordinates in a fixed-point accumulator of 58 64-bit
 *           limbs.  The orientation has its own filter and exact stage (csrc/exact_orient.h).
 *   range   every coordinate 0 or of a magnitude in [2^-150, 2^150]; anything else (NaN, infinities, subnormals) returns DGNN_E_UNSUPPORTED
 *           and is never answered approximately.
 *   exact_out int64 [3] on the device: exact-stage calls of L, exact-stage calls of the orientation, an error word.  Synchronises the stream.
 *
 * dgnn_delaunay: points fp64 [n, 3], distinct, GIVEN IN PRIORITY ORDER (row r is the point of priority rank r; the lowest rank is inserted
 *   first among points that contend).  Builds the Delaunay triangulation with a ghost vertex (id n): cells_out / neighbors_out int32
 *   [cell_capacity, 4] hold stats_out[DGNN_DELAUNAY_CELLS] rows on return; a row whose first vertex is -1 is a dead cell; a row with the
 *   ghost is an infinite cell (its other three vertices are a hull facet; with p in the ghost's slot the row is positively oriented exactly
 *   for p strictly beyond that facet); every other row is a finite cell with det[v1 - v0, v2 - v0, v3 - v0] > 0 exactly.  neighbors_out[c][k]
 *   is the cell across the facet opposite vertex k.  The set of finite cells is a function of the points and their order alone (in general
 *   position of the points alone); row numbers are a function of those too -- nothing depends on the schedule, reruns are bit-identical.
 *   A cell conflicts with p when p is strictly inside its sphere (finite), or strictly beyond its facet, or in the facet's plane and in
 *   conflict with the finite cell behind it (infinite).  No input point is strictly inside any finite cell's sphere on return.
 *   stats_out: int64 [DGNN_DELAUNAY_N_STATS] on the HOST.  scratch: dgnn_delaunay_scratch_bytes(n, cell_capacity) bytes; nothing is
 *   allocated inside.  Returns DGNN_E_INVALID for n < 4 or a non-finite coordinate, DGNN_E_UNSUPPORTED for a coordinate outside the
 *   predicate's range or a device loop that reached its cap (cell count), DGNN_E_DUPLICATE for two equal points (their ranks in
 *   stats_out[DGNN_DELAUNAY_DUP_A / _B]), DGNN_E_DEGENERATE when all points are coplanar, DGNN_E_CAPACITY when cell_capacity is too small
 *   (stats_out[DGNN_DELAUNAY_NEED] cells were needed at that moment; call again with more).  At most n rounds; synchronises the stream
 *   several times per round.
 *
 * dgnn_delaunay_violations: any cell list (vertices fp64 [n_vertices, 3], tetrahedra int32 [n_tets, 4]) with its neighbour table (int32
 *   [n_tets, 4], -1 = no cell across) -> counts_out int64 [DGNN_VIOLATION_N + 1] on the device (the last word is an error word): flat cells,
 *   negatively oriented cells, interior facets whose opposite vertex lies strictly inside the cell's sphere (counted once per facet),
 *   (hull facet, edge) pairs at which the hull is locally concave, and links that do not share a facet.  All exact.  Synchronises. */
#define DGNN_E_CAPACITY -5   /* caller-provided storage too small; the need is reported */
#define DGNN_E_DUPLICATE -6  /* two equal input points */
#define DGNN_E_DEGENERATE -7 /* all input points coplanar */
enum { DGNN_DELAUNAY_ROUNDS = 0, DGNN_DELAUNAY_WIN_MIN, DGNN_DELAUNAY_WIN_MAX, DGNN_DELAUNAY_MAX_CAVITY, DGNN_DELAUNAY_EXACT_INSPHERE,
       DGNN_DELAUNAY_EXACT_ORIENT, DGNN_DELAUNAY_CELLS, DGNN_DELAUNAY_NEED, DGNN_DELAUNAY_DUP_A, DGNN_DELAUNAY_DUP_B, DGNN_DELAUNAY_SLOW_PATHS,
       DGNN_DELAUNAY_N_STATS = 16 };
enum { DGNN_VIOLATION_FLAT = 0, DGNN_VIOLATION_NEGATIVE, DGNN_VIOLATION_NONLOCAL, DGNN_VIOLATION_CONCAVE, DGNN_VIOLATION_BAD_LINK, DGNN_VIOLATION_N };
int dgnn_insphere_sign(const double* points5, int64_t n, int8_t* sign_out, int64_t* exact_out, void* stream);
int64_t dgnn_delaunay_default_capacity(int64_t n);
int64_t dgnn_delaunay_scratch_bytes(int64_t n, int64_t cell_capacity);
int dgnn_delaunay(const double* points, int64_t n, int64_t cell_capacity, int32_t* cells_out, int32_t* neighbors_out, int64_t* stats_out,
                  void* scratch, void* stream);
int dgnn_delaunay_violations(const double* vertices, int64_t n_vertices, const int32_t* tetrahedra, const int32_t* neighbors, int64_t n_tets,
                             int64_t* counts_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Singular vertices of a labelled tetrahedralization and their repair by relabelling cells.  DESIGN.md section 31.  Integers only; nothing
 * depends on the schedule: reruns are bit-identical.  tetrahedra int32 [n_tets, 4] (the finite cells), neighbors int32 [n_tets, 4] as
 * dgnn_tet_neighbors writes it (slot k = the cell across the facet opposite vertex k, -1 = the infinite cell), labels int32 [n_tets]
 * (0 inside, 1 outside; the infinite cell is outside).  tetrahedra and neighbors are read a row (16 bytes) at a time and must be 16-byte
 * aligned.  Both entry points SYNCHRONISE `stream` (status reads).
 *
 *   star graph of vertex v
 *     nodes   every cell c with tetrahedra[c][k] == v for some k (its corner 4 c + k), and one node INF when for some such corner a slot
 *             j != k has neighbors[c][j] == -1 (a hull facet through v).
 *     edges   corner (c, k) -- the corner of n = neighbors[c][j] that holds v, for every j != k with n >= 0 and labels[n] == labels[c];
 *             corner (c, k) -- INF for every j != k with neighbors[c][j] == -1 when labels[c] == 1.
 *     a(v)    the connected components whose cells are labelled 0; b(v) those labelled 1, the component of INF among them (it counts also
 *             when no cell was joined to it).  v is SINGULAR when a(v) > 1 or b(v) > 1.
 *
 * dgnn_vertex_components: n_inside_out, n_outside_out int32 [n_vertices] = a(v), b(v) (0, 0 for a vertex of no cell); *n_singular_out (HOST
 *   int64) = the number of singular vertices.
 *
 * dgnn_manifold_repair: labels is read and rewritten in place.  cost int32 [n_tets], each >= 0 (NULL: every cell costs 1).  flipped[c] = 0.
 *   A round, on the labels and marks as the round finds them:
 *     1  the components of every vertex as above.
 *     2  a component of a singular vertex v is a CANDIDATE when its side has at least two components at v, it does not hold INF and none of
 *        its cells has flipped[c] == 1.  Its key is (the sum of cost over its cells, int64; its smallest cell id).  The MOVE of v is the
 *        candidate with the lexicographically smallest key; a singular vertex without a candidate has no move.
 *     3  claim[c] = the smallest v, among the vertices with a move, that has c in its star.  A vertex with a move WINS when claim[c] == v for
 *        every cell c of its star.
 *     4  every cell c of the move of every winner: labels[c] = 1 - labels[c], flipped[c] = 1.
 *   Rounds repeat until a round has no move (at most n_tets rounds apply one, a cell flipping at most once), or max_rounds rounds have been
 *   applied (max_rounds < 0: no limit): the labels after r rounds are those of r rounds of the unlimited call.  One host read per round.
 *   stats_out: int64 [DGNN_MANIFOLD_N_STATS] on the HOST: rounds that applied a move, moves applied, cells flipped, of those 1 -> 0 and
 *   0 -> 1, the sum of cost over the flipped cells, singular vertices before the first round and on the returned labels (the STUCK vertices
 *   when no limit ended the call).  flipped_out int32 [n_tets] or NULL: the marks.
 *
 *   scratch   dgnn_vertex_components_scratch_bytes / dgnn_manifold_repair_scratch_bytes (n_tets, n_vertices) bytes (0: sizes beyond int32).
 *   DGNN_E_INVALID: a vertex or neighbour id out of range, a cell with a repeated vertex, a neighbour that does not hold the three shared
 *   vertices or does not name the cell back in the slot of its fourth, a label outside {0, 1}, a negative cost.  DGNN_E_UNSUPPORTED:
 *   4 n_tets + n_vertices beyond int32.
 * ---------------------------------------------------------------------------------------------- */
enum { DGNN_MANIFOLD_ROUNDS = 0, DGNN_MANIFOLD_MOVES, DGNN_MANIFOLD_FLIPPED_CELLS, DGNN_MANIFOLD_TO_INSIDE, DGNN_MANIFOLD_TO_OUTSIDE,
       DGNN_MANIFOLD_FLIPPED_COST, DGNN_MANIFOLD_SINGULAR_BEFORE, DGNN_MANIFOLD_SINGULAR_AFTER, DGNN_MANIFOLD_N_STATS };
int64_t dgnn_vertex_components_scratch_bytes(int64_t n_tets, int64_t n_vertices);
int dgnn_vertex_components(const int32_t* tetrahedra, const int32_t* neighbors, const int32_t* labels, int64_t n_tets, int64_t n_vertices,
                           int32_t* n_inside_out, int32_t* n_outside_out, int64_t* n_singular_out, void* scratch, void* stream);
int64_t dgnn_manifold_repair_scratch_bytes(int64_t n_tets, int64_t n_vertices);
int dgnn_manifold_repair(const int32_t* tetrahedra, const int32_t* neighbors, int32_t* labels, const int32_t* cost, int64_t n_tets,
                         int64_t n_vertices, int64_t max_rounds, int32_t* flipped_out, int64_t* stats_out, void* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DGNN_HIP_H */
