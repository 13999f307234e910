// Graph LayerNorm (torch_geometric.nn.norm.LayerNorm, PyG 2.0.2, the batch=None branch the reference takes at
// surfaceNetStaticEdgeFilters.py:165,173,185 and inside the two-layer edge filter :134):
//   x = x - x.mean()                              ONE scalar mean over all M*C elements
//   out = x / (x.std(unbiased=False) + eps)       eps on the std, not under the square root
//   out = out * weight + bias                     per channel
// Train and eval modes are the same: the statistics always come from the tensor itself, so the layer is a whole-tensor
// reduction between the GEMM and the ReLU (and one in the backward).  No host synchronisation: the statistics stay on the
// device.  Every reduction is deterministic (fixed-order fp64 partial sums, as norm.hip).
//
// Forward:  partial sums [nblk][2][pc] -- the GEMM epilogue's colstats (pc = C, dgnn_linear_fwd_x3_stats) or this file's own
//           pass (pc = 1, dgnn_graph_ln_stats) -- -> dgnn_graph_ln_finalize_fold -> stats (m, sigma, r = 1 / (sigma + eps)) and
//           per-channel scale = w r, shift = b - m w r -> dgnn_graph_ln_apply: y = act((x - m) * scale + b).
//           The apply centres first, as PyG does: x - m is exact where x is near m, so a tensor far off zero keeps its digits.
// Backward of y = relu(w xhat + b), xhat = (x - m) r, g = dy [z > 0] (z recomputed from x: y is not read):
//           db_c = sum_n g, dw_c = sum_n g xhat (one column pass), S1 = sum_c w_c db_c, S2 = sum_c w_c dw_c,
//           dx = r (g w - S1 / N) - xhat S2 / (N sigma),  N = M C   (sigma = 0: xhat = 0 and the second term is 0).
#include "common.h"

namespace {

constexpr int LN_THREADS = 256;
constexpr int LN_BLOCKS = 1024;     // partial rows of the standalone statistics pass and of the backward's column pass
constexpr int LN_PAIR_BLOCKS = 256; // first stage of the finaliser on many partial rows (the GEMM epilogue leaves one per 32 rows)

// fixed-order block sum of a pair (tree over LN_THREADS lanes); every thread gets the result
__device__ __forceinline__ void block_sum2(double& a, double& b) {
    __shared__ double red[2][LN_THREADS];
    const int t = threadIdx.x;
    red[0][t] = a;
    red[1][t] = b;
    __syncthreads();
    for (int o = LN_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) {
            red[0][t] += red[0][t + o];
            red[1][t] += red[1][t + o];
        }
        __syncthreads();
    }
    a = red[0][0];
    b = red[1][0];
    __syncthreads();
}

template <int V>
struct Piece {
    float v[V];
    __device__ __forceinline__ void load(const float* p) {
        if constexpr (V == 4) {
            const float4 q = *reinterpret_cast<const float4*>(p);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            v[0] = *p;
        }
    }
    __device__ __forceinline__ void store(float* p) const {
        if constexpr (V == 4) {
            *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            *p = v[0];
        }
    }
};

// element piece i of the rows [r0, r0 + ...) of a [M, c] tensor with leading dimension ld, in pieces of V columns (cv = c / V per row)
__device__ __forceinline__ int64_t piece_off(uint32_t i, int64_t r0, int64_t ld, uint32_t cv, int V, bool dense) {
    if (dense) return r0 * ld + (int64_t)i * V;
    const uint32_t r = i / cv;
    return (r0 + r) * ld + (int64_t)(i - r * cv) * V;
}

// Standalone statistics: block b sums x and x^2 over rows [b rpb, (b + 1) rpb) into partials[b][2] (fp64)
template <int V>
__global__ void __launch_bounds__(LN_THREADS) k_ln_stats(const float* __restrict__ x, int64_t ldx, int64_t M, int c, int64_t rpb,
                                                         double* __restrict__ partials) {
    const int64_t r0 = (int64_t)blockIdx.x * rpb;
    const int64_t r1 = min(M, r0 + rpb);
    const uint32_t cv = (uint32_t)(c / V);
    const uint32_t n = r1 > r0 ? (uint32_t)((r1 - r0) * cv) : 0u;
    const bool dense = ldx == c;
    double s = 0.0, q = 0.0;
    uint32_t i = threadIdx.x;
    for (; i + 3 * LN_THREADS < n; i += 4 * LN_THREADS) {      // four pieces in flight per lane, added in ascending order
        Piece<V> p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) p[u].load(x + piece_off(i + u * LN_THREADS, r0, ldx, cv, V, dense));
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const double v = p[u].v[j];
                s += v;
                q = fma(v, v, q);
            }
    }
    for (; i < n; i += LN_THREADS) {
        Piece<V> p;
        p.load(x + piece_off(i, r0, ldx, cv, V, dense));
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const double v = p.v[j];
            s += v;
            q = fma(v, v, q);
        }
    }
    block_sum2(s, q);
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x + 0] = s;
        partials[2 * blockIdx.x + 1] = q;
    }
}

// sum of every entry of partial rows [b0, b1) of P[nrows][2][pc] -> (s, q), fixed order
__device__ __forceinline__ void sum_partial_rows(const double* __restrict__ P, int64_t b0, int64_t b1, int pc, double& s, double& q) {
    s = 0.0;
    q = 0.0;
    const int64_t n = (b1 - b0) * pc;
    for (int64_t i = threadIdx.x; i < n; i += LN_THREADS) {
        const int64_t b = b0 + i / pc, j = i % pc;
        s += P[(2 * b + 0) * pc + j];
        q += P[(2 * b + 1) * pc + j];
    }
    block_sum2(s, q);
}

__global__ void __launch_bounds__(LN_THREADS) k_ln_pairs(const double* __restrict__ P, int64_t nrows, int pc, int64_t rpb, double* __restrict__ out) {
    const int64_t b0 = (int64_t)blockIdx.x * rpb;
    const int64_t b1 = min(nrows, b0 + rpb);
    double s, q;
    sum_partial_rows(P, b0, b1 > b0 ? b1 : b0, pc, s, q);
    if (threadIdx.x == 0) {
        out[2 * blockIdx.x + 0] = s;
        out[2 * blockIdx.x + 1] = q;
    }
}

// one block: the global (m, sigma, r) and the per-channel fold
__global__ void __launch_bounds__(LN_THREADS) k_ln_finalize(const double* __restrict__ P, int64_t nrows, int pc, int64_t M, int c,
                                                            const float* __restrict__ weight, const float* __restrict__ bias, float eps,
                                                            float* __restrict__ stats, float* __restrict__ scale, float* __restrict__ shift) {
    double s, q;
    sum_partial_rows(P, 0, nrows, pc, s, q);
    const double N = (double)M * (double)c;
    const double m = s / N;
    double var = q / N - m * m;
    if (var < 0.0) var = 0.0;
    const double sd = sqrt(var);
    const double r = 1.0 / (sd + (double)eps);
    if (threadIdx.x == 0) {
        stats[0] = (float)m;
        stats[1] = (float)sd;
        stats[2] = (float)r;
        stats[3] = (float)N;
    }
    for (int k = threadIdx.x; k < c; k += LN_THREADS) {
        const double wr = (weight ? (double)weight[k] : 1.0) * r;
        scale[k] = (float)wr;
        shift[k] = (float)((bias ? (double)bias[k] : 0.0) - m * wr);
    }
}

// y = act((x - m) * scale + b) over rows [b rpb, (b + 1) rpb)
template <int V>
__global__ void __launch_bounds__(LN_THREADS) k_ln_apply(const float* __restrict__ x, int64_t ldx, int64_t M, int c, int64_t rpb,
                                                         const float* __restrict__ stats, const float* __restrict__ scale,
                                                         const float* __restrict__ bias, int relu, float* __restrict__ y, int64_t ldy) {
    const int64_t r0 = (int64_t)blockIdx.x * rpb;
    const int64_t r1 = min(M, r0 + rpb);
    const uint32_t cv = (uint32_t)(c / V);
    const uint32_t n = r1 > r0 ? (uint32_t)((r1 - r0) * cv) : 0u;
    const bool dx_ = ldx == c, dy_ = ldy == c;
    const float m = stats[0];
    for (uint32_t i = threadIdx.x; i < n; i += LN_THREADS) {
        const uint32_t r = i / cv, k = (i - r * cv) * V;
        Piece<V> p;
        p.load(x + (dx_ ? r0 * ldx + (int64_t)i * V : (r0 + r) * ldx + k));
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float v = __fmaf_rn(p.v[j] - m, scale[k + j], bias ? bias[k + j] : 0.f);
            p.v[j] = relu ? fmaxf(v, 0.f) : v;
        }
        p.store(y + (dy_ ? r0 * ldy + (int64_t)i * V : (r0 + r) * ldy + k));
    }
}

// backward column pass: partials[b][0][c] = sum g, [b][1][c] = sum g xhat over rows [b rpb, (b + 1) rpb).  Lanes = cw column pieces x nrl
// row lanes; rows wider than 256 pieces take several windows.
template <int V>
__global__ void __launch_bounds__(LN_THREADS) k_ln_bwd_cols(const float* __restrict__ x, int64_t ldx, const float* __restrict__ dy, int64_t lddy,
                                                            const float* __restrict__ stats, const float* __restrict__ scale,
                                                            const float* __restrict__ bias, int relu, int64_t M, int c, int64_t rpb,
                                                            double* __restrict__ partials) {
    __shared__ double red[2][LN_THREADS * V];
    const int cv = c / V;
    const int cw = cv < LN_THREADS ? cv : LN_THREADS;
    const int nrl = LN_THREADS / cw;
    const int tg = threadIdx.x % cw, ty = threadIdx.x / cw;
    const int64_t r0 = (int64_t)blockIdx.x * rpb;
    const int64_t r1 = min(M, r0 + rpb);
    const float m = stats[0], r = stats[2];
    for (int w0 = 0; w0 < cv; w0 += cw) {
        const int piece = w0 + tg;
        const bool live = ty < nrl && piece < cv;
        const int col = piece * V;
        double s0[V], s1[V];
        float sc[V], bb[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            s0[j] = s1[j] = 0.0;
            sc[j] = live ? scale[col + j] : 0.f;
            bb[j] = (live && bias) ? bias[col + j] : 0.f;
        }
        if (live) {
            for (int64_t row = r0 + ty; row < r1; row += nrl) {
                Piece<V> xv, gv;
                xv.load(x + row * ldx + col);
                gv.load(dy + row * lddy + col);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const float xm = xv.v[j] - m;
                    float g = gv.v[j];
                    if (relu && !(__fmaf_rn(xm, sc[j], bb[j]) > 0.f)) g = 0.f;
                    s0[j] += g;
                    s1[j] += (double)g * (double)(xm * r);
                }
            }
        }
        if (ty < nrl) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                red[0][ty * cw * V + tg * V + j] = s0[j];
                red[1][ty * cw * V + tg * V + j] = s1[j];
            }
        }
        __syncthreads();
        const int wcols = (min(cv, w0 + cw) - w0) * V;
        for (int o = threadIdx.x; o < 2 * wcols; o += LN_THREADS) {
            const int qd = o / wcols, cc = o - qd * wcols;
            double t = 0.0;
            for (int k = 0; k < nrl; ++k) t += red[qd][k * cw * V + cc];
            partials[((int64_t)blockIdx.x * 2 + qd) * c + w0 * V + cc] = t;
        }
        __syncthreads();
    }
}

// per-column sums of the backward partials: 16 columns x 64 slices per block (slice s adds rows s, s + 64, ... in order, then the slices in order)
constexpr int CF_COLS = 16, CF_SLICES = 64;
__global__ void __launch_bounds__(CF_COLS * CF_SLICES) k_ln_bwd_colsum(const double* __restrict__ P, int nblk, int c, double* __restrict__ sums64,
                                                                       float* __restrict__ dweight, float* __restrict__ dbias) {
    __shared__ double red[2][CF_SLICES][CF_COLS + 1];
    const int o = threadIdx.x % CF_COLS, sl = threadIdx.x / CF_COLS, col = blockIdx.x * CF_COLS + o;
    double ps = 0.0, pq = 0.0;
    if (col < c)
        for (int b = sl; b < nblk; b += CF_SLICES) {
            ps += P[((int64_t)b * 2 + 0) * c + col];
            pq += P[((int64_t)b * 2 + 1) * c + col];
        }
    red[0][sl][o] = ps;
    red[1][sl][o] = pq;
    __syncthreads();
    if (sl != 0 || col >= c) return;
    double s = 0.0, q = 0.0;
    for (int k = 0; k < CF_SLICES; ++k) {
        s += red[0][k][o];
        q += red[1][k][o];
    }
    sums64[col] = s;
    sums64[c + col] = q;
    if (dbias) dbias[col] = (float)s;
    if (dweight) dweight[col] = (float)q;
}

// one block: coef[0] = S1 / N, coef[1] = S2 / (N sigma) (0 where sigma = 0)
__global__ void __launch_bounds__(LN_THREADS) k_ln_bwd_scalars(const double* __restrict__ sums64, int c, const float* __restrict__ weight,
                                                               const float* __restrict__ stats, float* __restrict__ coef) {
    double s1 = 0.0, s2 = 0.0;
    for (int k = threadIdx.x; k < c; k += LN_THREADS) {
        const double w = weight ? (double)weight[k] : 1.0;
        s1 += w * sums64[k];
        s2 += w * sums64[c + k];
    }
    block_sum2(s1, s2);
    if (threadIdx.x == 0) {
        const double N = (double)stats[3], sd = (double)stats[1];
        coef[0] = (float)(s1 / N);
        coef[1] = sd > 0.0 ? (float)(s2 / (N * sd)) : 0.f;
    }
}

template <int V>
__global__ void __launch_bounds__(LN_THREADS) k_ln_bwd_apply(const float* __restrict__ x, int64_t ldx, const float* __restrict__ dy, int64_t lddy,
                                                             const float* __restrict__ stats, const float* __restrict__ weight,
                                                             const float* __restrict__ scale, const float* __restrict__ bias, int relu,
                                                             const float* __restrict__ coef, int64_t M, int c, int64_t rpb, float* __restrict__ dx,
                                                             int64_t lddx) {
    const int64_t r0 = (int64_t)blockIdx.x * rpb;
    const int64_t r1 = min(M, r0 + rpb);
    const uint32_t cv = (uint32_t)(c / V);
    const uint32_t n = r1 > r0 ? (uint32_t)((r1 - r0) * cv) : 0u;
    const float m = stats[0], r = stats[2], c1 = coef[0], c2 = coef[1];
    for (uint32_t i = threadIdx.x; i < n; i += LN_THREADS) {
        const uint32_t rr = i / cv, k = (i - rr * cv) * V;
        const int64_t row = r0 + rr;
        Piece<V> xv, gv;
        xv.load(x + row * ldx + k);
        gv.load(dy + row * lddy + k);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float xm = xv.v[j] - m;
            float g = gv.v[j];
            if (relu && !(__fmaf_rn(xm, scale[k + j], bias ? bias[k + j] : 0.f) > 0.f)) g = 0.f;
            const float gh = g * (weight ? weight[k + j] : 1.f);
            gv.v[j] = r * (gh - c1) - (xm * r) * c2;
        }
        gv.store(dx + row * lddx + k);
    }
}

inline bool vec4(const float* p, int64_t ld, int c) { return p == nullptr || ((((uintptr_t)p) & 15) == 0 && ld % 4 == 0 && c % 4 == 0); }

int ln_red_blocks(int64_t M) {
    int64_t b = dgnn_cdiv(M, 64);
    if (b > LN_BLOCKS) b = LN_BLOCKS;
    return (int)(b < 1 ? 1 : b);
}

// rows per block of the elementwise passes: ~8 pieces of 4 per lane, and the in-block piece index stays below 2^31
int64_t ln_apply_rpb(int64_t M, int c) {
    const int64_t per = (int64_t)LN_THREADS * 32;
    int64_t rpb = dgnn_cdiv(per, c);
    if (rpb < 1) rpb = 1;
    if (rpb > M) rpb = M;
    return rpb;
}

double* as_f64(float* scratch) { return reinterpret_cast<double*>(((uintptr_t)scratch + 7) & ~(uintptr_t)7); }

}  // namespace

extern "C" int64_t dgnn_graph_ln_stats_blocks(int64_t M, int c) { return M > 0 && c > 0 ? ln_red_blocks(M) : 0; }

// floats: the backward's column partials [LN_BLOCKS][2][c] doubles + their fp64 sums [2][c] + the finaliser's first stage + coefficients
extern "C" int64_t dgnn_graph_ln_scratch_elems(int64_t M, int c) {
    if (c <= 0) c = 1;
    const int64_t blk = M > 0 ? ln_red_blocks(M) : 1;
    return 2 * (blk * 2 * c + 2 * c + 2 * LN_PAIR_BLOCKS + 2 * LN_BLOCKS + 8) + 8;
}

extern "C" int dgnn_graph_ln_stats(const float* x, int64_t ldx, int64_t M, int c, double* partials, void* stream) {
    DGNN_REQUIRE(M >= 0 && c > 0 && ldx >= c, DGNN_E_INVALID, "graph_ln_stats: bad sizes M=%lld c=%d ldx=%lld", (long long)M, c, (long long)ldx);
    if (M == 0) return DGNN_OK;
    DGNN_REQUIRE(x && partials && ((uintptr_t)partials & 7) == 0, DGNN_E_INVALID, "graph_ln_stats: null or unaligned pointer");
    const int nblk = ln_red_blocks(M);
    const int64_t rpb = dgnn_cdiv(M, nblk);
    DGNN_REQUIRE(rpb * c < (int64_t)1 << 31, DGNN_E_UNSUPPORTED, "graph_ln_stats: %lld rows x %d channels per block", (long long)rpb, c);
    if (vec4(x, ldx, c))
        hipLaunchKernelGGL(k_ln_stats<4>, dim3(nblk), dim3(LN_THREADS), 0, (hipStream_t)stream, x, ldx, M, c, rpb, partials);
    else
        hipLaunchKernelGGL(k_ln_stats<1>, dim3(nblk), dim3(LN_THREADS), 0, (hipStream_t)stream, x, ldx, M, c, rpb, partials);
    return dgnn_check_launch("graph_ln_stats");
}

extern "C" int dgnn_graph_ln_finalize_fold(const double* partials, int64_t nblk, int pc, int64_t M, int c, const float* weight, const float* bias,
                                           float eps, float* stats, float* scale, float* shift, double* scratch, void* stream) {
    DGNN_REQUIRE(M >= 0 && c > 0 && nblk >= 0 && pc > 0, DGNN_E_INVALID, "graph_ln_finalize_fold: bad sizes");
    if (M == 0) return DGNN_OK;
    DGNN_REQUIRE(partials && nblk > 0 && stats && scale && shift, DGNN_E_INVALID, "graph_ln_finalize_fold: null pointer");
    if (nblk * pc > 8 * LN_THREADS) {      // many partial rows: a first stage spreads them over LN_PAIR_BLOCKS workgroups
        DGNN_REQUIRE(scratch && ((uintptr_t)scratch & 7) == 0, DGNN_E_INVALID, "graph_ln_finalize_fold: scratch missing or unaligned");
        const int64_t rpb = dgnn_cdiv(nblk, LN_PAIR_BLOCKS);
        const int g = (int)dgnn_cdiv(nblk, rpb);
        hipLaunchKernelGGL(k_ln_pairs, dim3(g), dim3(LN_THREADS), 0, (hipStream_t)stream, partials, nblk, pc, rpb, scratch);
        hipLaunchKernelGGL(k_ln_finalize, dim3(1), dim3(LN_THREADS), 0, (hipStream_t)stream, (const double*)scratch, (int64_t)g, 1, M, c, weight, bias, eps,
                           stats, scale, shift);
    } else {
        hipLaunchKernelGGL(k_ln_finalize, dim3(1), dim3(LN_THREADS), 0, (hipStream_t)stream, partials, nblk, pc, M, c, weight, bias, eps, stats, scale,
                           shift);
    }
    return dgnn_check_launch("graph_ln_finalize_fold");
}

extern "C" int dgnn_graph_ln_apply(const float* x, int64_t ldx, int64_t M, int c, const float* stats, const float* scale, const float* bias, int relu,
                                   float* y, int64_t ldy, void* stream) {
    DGNN_REQUIRE(M >= 0 && c > 0 && ldx >= c && ldy >= c, DGNN_E_INVALID, "graph_ln_apply: bad sizes");
    if (M == 0) return DGNN_OK;
    DGNN_REQUIRE(x && stats && scale && y, DGNN_E_INVALID, "graph_ln_apply: null pointer");
    const int64_t rpb = ln_apply_rpb(M, c);
    const int64_t nb = dgnn_cdiv(M, rpb);
    DGNN_REQUIRE(nb < (int64_t)1 << 31, DGNN_E_UNSUPPORTED, "graph_ln_apply: too many rows");
    if (vec4(x, ldx, c) && vec4(y, ldy, c))
        hipLaunchKernelGGL(k_ln_apply<4>, dim3((unsigned)nb), dim3(LN_THREADS), 0, (hipStream_t)stream, x, ldx, M, c, rpb, stats, scale, bias, relu, y, ldy);
    else
        hipLaunchKernelGGL(k_ln_apply<1>, dim3((unsigned)nb), dim3(LN_THREADS), 0, (hipStream_t)stream, x, ldx, M, c, rpb, stats, scale, bias, relu, y, ldy);
    return dgnn_check_launch("graph_ln_apply");
}

extern "C" int dgnn_graph_ln_relu_bwd(const float* x, int64_t ldx, const float* dy, int64_t lddy, const float* stats, const float* weight,
                                      const float* scale, const float* bias, int relu, int64_t M, int c, float* dx, int64_t lddx, float* dweight,
                                      float* dbias, float* scratch, void* stream) {
    DGNN_REQUIRE(M >= 0 && c > 0 && ldx >= c && lddy >= c && lddx >= c, DGNN_E_INVALID, "graph_ln_relu_bwd: bad sizes");
    if (M == 0) return DGNN_OK;
    DGNN_REQUIRE(x && dy && stats && scale && dx && scratch, DGNN_E_INVALID, "graph_ln_relu_bwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int nblk = ln_red_blocks(M);
    const int64_t rpb = dgnn_cdiv(M, nblk);
    double* P = as_f64(scratch);
    double* sums64 = P + (int64_t)nblk * 2 * c;
    float* coef = reinterpret_cast<float*>(sums64 + 2 * c);
    const bool v = vec4(x, ldx, c) && vec4(dy, lddy, c) && vec4(dx, lddx, c);
    if (v)
        hipLaunchKernelGGL(k_ln_bwd_cols<4>, dim3(nblk), dim3(LN_THREADS), 0, st, x, ldx, dy, lddy, stats, scale, bias, relu, M, c, rpb, P);
    else
        hipLaunchKernelGGL(k_ln_bwd_cols<1>, dim3(nblk), dim3(LN_THREADS), 0, st, x, ldx, dy, lddy, stats, scale, bias, relu, M, c, rpb, P);
    hipLaunchKernelGGL(k_ln_bwd_colsum, dim3((c + CF_COLS - 1) / CF_COLS), dim3(CF_COLS * CF_SLICES), 0, st, P, nblk, c, sums64, dweight, dbias);
    hipLaunchKernelGGL(k_ln_bwd_scalars, dim3(1), dim3(LN_THREADS), 0, st, sums64, c, weight, stats, coef);
    const int64_t arpb = ln_apply_rpb(M, c);
    const int64_t nb = dgnn_cdiv(M, arpb);
    if (v)
        hipLaunchKernelGGL(k_ln_bwd_apply<4>, dim3((unsigned)nb), dim3(LN_THREADS), 0, st, x, ldx, dy, lddy, stats, weight, scale, bias, relu, coef, M, c,
                           arpb, dx, lddx);
    else
        hipLaunchKernelGGL(k_ln_bwd_apply<1>, dim3((unsigned)nb), dim3(LN_THREADS), 0, st, x, ldx, dy, lddy, stats, weight, scale, bias, relu, coef, M, c,
                           arpb, dx, lddx);
    return dgnn_check_launch("graph_ln_relu_bwd");
}
