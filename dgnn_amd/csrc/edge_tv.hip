// Edge total-variation regulariser of the training objective (reference learning/runModel.py:109-160, added at :250-256) and its gradient:
//
//     p(v)  = softmax(logits_v)_0                                      (the inside-probability of cell v)
//     tv_e  = |p(s_e) - p(d_e)|
//     reg   = w * sum_e tv_e / E                                       sums[2] (fp64) = w * sum_e tv_e, E   (the running metric sums of :48-80)
//     c(v)  = sum_{e: s_e = v} sgn_e - sum_{e: d_e = v} sgn_e          sgn_e = sign(p(s_e) - p(d_e)), sign(0) = 0 (torch's abs rule)
//     dlogits_v = g * (w / E) * c(v) * p(v) (1 - p(v)) * (+1, -1)
//
// Two launches.  The EDGE pass streams src / dst once (the logits table, 8 B a row, stays in L2), sums tv in fp64 per workgroup and adds sgn_e into
// the int32 table `net` with integer atomics: c(v) is an integer, so the gradient does not depend on the order in which the edges arrive.  The
// FINISH pass adds the workgroup sums in a fixed order (reg, sums, optionally `total = loss + reg` and the running metric sums) and, when a gradient
// is wanted, writes or adds dlogits from net -- and can hand net back zeroed, so that a caller who keeps the table never pays a memset launch.
// Row terms are fp32 like the reference's, the sum is fp64 in a fixed order: reruns are bit-identical.
#include "common.h"

namespace {

constexpr int TV_THREADS = 256;
constexpr int TV_UNROLL = 4;      // 16-byte index loads in flight per lane and index row (the pass is bound by the index stream; DESIGN 12 on
                                  // the LayerNorm elementwise passes: one load -> use chain per lane leaves the memory pipe idle)

template <typename T, int V>
struct alignas(sizeof(T) * V) IdxVec {
    T v[V];
};

// e = exp(-|l1 - l0|) <= 1 never overflows; a saturated row gives e = 0: p in {0, 1}, p (1 - p) = 0
struct Prob {
    float p, pq;      // p(v), p(v) (1 - p(v))
};
__device__ __forceinline__ Prob inside_prob(const float* __restrict__ logits, int64_t ldl, bool pair, int64_t v) {
    float l0, l1;
    if (pair) {
        const float2 l = *reinterpret_cast<const float2*>(logits + 2 * v);
        l0 = l.x, l1 = l.y;
    } else {
        l0 = logits[v * ldl], l1 = logits[v * ldl + 1];
    }
    const float d = l1 - l0;
    const float e = expf(-fabsf(d));
    const float r = 1.f / (1.f + e);
    return {d >= 0.f ? e * r : r, e * r * r};
}

// fp64 sum of one value per thread, in a fixed order: the 64 lanes of a wave by shuffles, the waves in wave order.  Valid in thread 0.
__device__ __forceinline__ double block_sum(double x, double* red /*[TV_THREADS / 64]*/) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    double s = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < TV_THREADS / 64; ++w) s += red[w];
    return s;
}

// partials[b] = sum of tv_e * w over block b's edges; net[s_e] += sgn_e, net[d_e] -= sgn_e (GRAD).  Edge e is (src[e * es], dst[e * es]).  V indices
// per load: the vector forms need 16-byte aligned rows -- two rows of stride 1 (a contiguous [2, E] edge_index), or INTER: one row of (src, dst) pairs
// (es == 2, dst == src + 1: the transposed view of an [E, 2] array, what the scene loader hands out) --, V = 1 takes any alignment and stride (a column
// slice of a [2, E] edge_index).  An index outside [0, n) is skipped and reported through the asynchronous error word.
template <typename T, int V, bool INTER, bool GRAD>
__global__ void __launch_bounds__(TV_THREADS) k_edge_tv(const float* __restrict__ logits, int64_t ldl, int pair, int64_t n, const T* __restrict__ src,
                                                        const T* __restrict__ dst, int64_t es, int64_t E, float weight, int32_t* __restrict__ net,
                                                        double* __restrict__ partials, int32_t* aflag) {
    __shared__ double red[TV_THREADS / 64];
    typedef IdxVec<T, V> Vec;
    constexpr int EPV = INTER ? V / 2 : V;      // edges per load
    const int64_t nvec = E / EPV;
    double acc = 0;
    auto edge = [&](int64_t s, int64_t d) {
        if ((uint64_t)s >= (uint64_t)n || (uint64_t)d >= (uint64_t)n) {
            dgnn_raise_async(aflag, DGNN_ASYNC_KEY_RANGE);
            return;
        }
        const float diff = inside_prob(logits, ldl, pair, s).p - inside_prob(logits, ldl, pair, d).p;
        acc += (double)(fabsf(diff) * weight);
        if (GRAD && diff != 0.f) {
            const int sg = diff > 0.f ? 1 : -1;
            atomicAdd(&net[s], sg);
            atomicAdd(&net[d], -sg);
        }
    };
    const int64_t stride = (int64_t)gridDim.x * TV_THREADS * TV_UNROLL;
    for (int64_t base = (int64_t)blockIdx.x * TV_THREADS * TV_UNROLL + threadIdx.x; base < nvec; base += stride) {
        Vec s[TV_UNROLL], d[TV_UNROLL];
#pragma unroll
        for (int u = 0; u < TV_UNROLL; ++u) {
            const int64_t j = base + u * TV_THREADS;
            if (j < nvec) {
                s[u] = reinterpret_cast<const Vec*>(src)[j];
                if (!INTER) d[u] = reinterpret_cast<const Vec*>(dst)[j];
            }
        }
#pragma unroll
        for (int u = 0; u < TV_UNROLL; ++u) {
            if (base + u * TV_THREADS < nvec) {
#pragma unroll
                for (int q = 0; q < EPV; ++q) INTER ? edge((int64_t)s[u].v[2 * q], (int64_t)s[u].v[2 * q + 1]) : edge((int64_t)s[u].v[q], (int64_t)d[u].v[q]);
            }
        }
    }
    if (blockIdx.x == 0 && (int64_t)threadIdx.x < E - nvec * EPV) edge((int64_t)src[(nvec * EPV + threadIdx.x) * es], (int64_t)dst[(nvec * EPV + threadIdx.x) * es]);
    const double tot = block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = tot;
}

// Block 0 (partials != NULL): sums = {sum of the nb partials in a fixed order, E}, reg = sums[0] / E, total = *add_loss + reg, running += sums.
// Every block (dlogits != NULL): rows v < n of dlogits from net, written or added; clear: net[v] = 0 behind the read.
__global__ void __launch_bounds__(TV_THREADS) k_edge_tv_finish(const double* __restrict__ partials, int nb, int64_t E, double* __restrict__ sums,
                                                               float* __restrict__ reg, const float* __restrict__ add_loss, float* __restrict__ total,
                                                               double* __restrict__ running, const float* __restrict__ logits, int64_t ldl, int pair,
                                                               int64_t n, int32_t* __restrict__ net, int clear, float weight, const float* __restrict__ g,
                                                               float* __restrict__ dlogits, int64_t ldd, int accumulate) {
    __shared__ double red[TV_THREADS / 64];
    if (blockIdx.x == 0 && partials) {
        double x = 0;
        for (int b = threadIdx.x; b < nb; b += TV_THREADS) x += partials[b];
        const double tot = block_sum(x, red);
        if (threadIdx.x == 0) {
            const float r = (float)(tot / (double)E);
            sums[0] = tot, sums[1] = (double)E;
            *reg = r;
            if (total) *total = (add_loss ? *add_loss : 0.f) + r;
            if (running) running[0] += tot, running[1] += (double)E;
        }
    }
    if (!dlogits) return;
    const float coef = (g ? *g : 1.f) * weight / (float)E;
    for (int64_t v = (int64_t)blockIdx.x * TV_THREADS + threadIdx.x; v < n; v += (int64_t)gridDim.x * TV_THREADS) {
        const int32_t c = net[v];
        if (clear) net[v] = 0;
        const float dl = coef * (float)c * inside_prob(logits, ldl, pair, v).pq;
        if (accumulate) {
            dlogits[v * ldd] = dlogits[v * ldd] + dl;
            dlogits[v * ldd + 1] = dlogits[v * ldd + 1] - dl;
        } else {
            dlogits[v * ldd] = dl;
            dlogits[v * ldd + 1] = -dl;
        }
    }
}

// a [n][2] table with 8-byte aligned rows is read one float2 a row
inline int rows_are_pairs(const float* logits, int64_t ldl) { return ldl == 2 && ((uintptr_t)logits & 7) == 0; }

// how the edge pass reads the indices: 0 = one index a load (any stride and alignment), 1 = two rows of stride 1, 2 = one row of (src, dst) pairs
inline int index_form(const void* src, const void* dst, int64_t es, int isz) {
    if (es == 1 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0) return 1;
    if (es == 2 && (const char*)dst == (const char*)src + isz && ((uintptr_t)src & 15) == 0) return 2;
    return 0;
}

template <typename T, bool GRAD>
void launch_edge(int form, const float* logits, int64_t ldl, int64_t n, const void* src, const void* dst, int64_t es, int64_t E, float weight, int32_t* net,
                 double* partials, int64_t nb, hipStream_t stream) {
    constexpr int V = 16 / sizeof(T);
    int32_t* const aflag = dgnn_async_flag_dev();
    const int pair = rows_are_pairs(logits, ldl);
    const T *s = (const T*)src, *d = (const T*)dst;
    const dim3 grid((unsigned)nb), block(TV_THREADS);
    if (form == 1)
        hipLaunchKernelGGL((k_edge_tv<T, V, false, GRAD>), grid, block, 0, stream, logits, ldl, pair, n, s, d, es, E, weight, net, partials, aflag);
    else if (form == 2)
        hipLaunchKernelGGL((k_edge_tv<T, V, true, GRAD>), grid, block, 0, stream, logits, ldl, pair, n, s, d, es, E, weight, net, partials, aflag);
    else
        hipLaunchKernelGGL((k_edge_tv<T, 1, false, GRAD>), grid, block, 0, stream, logits, ldl, pair, n, s, d, es, E, weight, net, partials, aflag);
}

// number of workgroups (= partial sums) of the edge pass: a function of E, the index width, the layout of src / dst and max_blocks alone
int64_t edge_pass(const float* logits, int64_t ldl, int64_t n, const void* src, const void* dst, int64_t es, int idx64, int64_t E, float weight, int32_t* net,
                  double* partials, int max_blocks, hipStream_t stream) {
    const int isz = idx64 ? 8 : 4, form = index_form(src, dst, es, isz);
    const int64_t loads = E / (form == 0 ? 1 : 16 / isz / form);      // edges per 16-byte load: 16 / isz of a row, half as many of a row of pairs
    int64_t nb = dgnn_grid_cap(dgnn_cdiv(loads > 0 ? loads : 1, (int64_t)TV_THREADS * TV_UNROLL));
    if (max_blocks > 0 && max_blocks < nb) nb = max_blocks;
    if (idx64)
        net ? launch_edge<int64_t, true>(form, logits, ldl, n, src, dst, es, E, weight, net, partials, nb, stream)
            : launch_edge<int64_t, false>(form, logits, ldl, n, src, dst, es, E, weight, net, partials, nb, stream);
    else
        net ? launch_edge<int32_t, true>(form, logits, ldl, n, src, dst, es, E, weight, net, partials, nb, stream)
            : launch_edge<int32_t, false>(form, logits, ldl, n, src, dst, es, E, weight, net, partials, nb, stream);
    return nb;
}

}  // namespace

extern "C" int64_t dgnn_edge_tv_scratch_doubles(void) { return (int64_t)DGNN_NUM_CU * 8; }

extern "C" int dgnn_edge_tv_fwd(const float* logits, int64_t ldl, int64_t n, const void* src, const void* dst, int64_t estride, int idx64, int64_t E, float weight, int32_t* net,
                                double* sums, float* reg, double* scratch, int max_blocks, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(logits && src && dst && sums && reg && scratch && n > 0 && E > 0 && estride >= 1 && ldl >= 2, DGNN_E_INVALID,
                 "edge_tv_fwd: bad args (two-class logits, at least one row and one edge)");
    if (net && hipMemsetAsync(net, 0, (size_t)n * sizeof(int32_t), stream) != hipSuccess) return dgnn_check_launch("edge_tv_fwd");
    const int64_t nb = edge_pass(logits, ldl, n, src, dst, estride, idx64, E, weight, net, scratch, max_blocks, stream);
    hipLaunchKernelGGL(k_edge_tv_finish, dim3(1), dim3(TV_THREADS), 0, stream, scratch, (int)nb, E, sums, reg, (const float*)nullptr, (float*)nullptr,
                       (double*)nullptr, logits, ldl, 0, (int64_t)0, (int32_t*)nullptr, 0, weight, (const float*)nullptr, (float*)nullptr, (int64_t)2, 0);
    return dgnn_check_launch("edge_tv_fwd");
}

extern "C" int dgnn_edge_tv_bwd(const float* logits, int64_t ldl, int64_t n, const int32_t* net, float weight, int64_t E, const float* grad, float* dlogits,
                                int64_t ldd, int accumulate, void* stream_) {
    DGNN_REQUIRE(logits && net && dlogits && n > 0 && E > 0 && ldl >= 2 && ldd >= 2, DGNN_E_INVALID, "edge_tv_bwd: bad args");
    hipLaunchKernelGGL(k_edge_tv_finish, dim3(dgnn_grid_cap(dgnn_cdiv(n, TV_THREADS))), dim3(TV_THREADS), 0, (hipStream_t)stream_, (const double*)nullptr, 0, E,
                       (double*)nullptr, (float*)nullptr, (const float*)nullptr, (float*)nullptr, (double*)nullptr, logits, ldl, rows_are_pairs(logits, ldl), n,
                       const_cast<int32_t*>(net), 0, weight, grad, dlogits, ldd, accumulate);
    return dgnn_check_launch("edge_tv_bwd");
}

extern "C" int dgnn_edge_tv_step(const float* logits, int64_t ldl, int64_t n, const void* src, const void* dst, int64_t estride, int idx64, int64_t E, float weight,
                                 const float* grad, int32_t* net, int net_is_zero, double* sums, float* reg, const float* add_loss, float* total,
                                 double* running, float* dlogits, int64_t ldd, int accumulate, double* scratch, int max_blocks, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(logits && src && dst && net && sums && reg && scratch && dlogits && n > 0 && E > 0 && estride >= 1 && ldl >= 2 && ldd >= 2, DGNN_E_INVALID,
                 "edge_tv_step: bad args (two-class logits, at least one row and one edge)");
    if (!net_is_zero && hipMemsetAsync(net, 0, (size_t)n * sizeof(int32_t), stream) != hipSuccess) return dgnn_check_launch("edge_tv_step");
    const int64_t nb = edge_pass(logits, ldl, n, src, dst, estride, idx64, E, weight, net, scratch, max_blocks, stream);
    hipLaunchKernelGGL(k_edge_tv_finish, dim3(dgnn_grid_cap(dgnn_cdiv(n, TV_THREADS))), dim3(TV_THREADS), 0, stream, scratch, (int)nb, E, sums, reg, add_loss, total,
                       running, logits, ldl, rows_are_pairs(logits, ldl), n, net, 1, weight, grad, dlogits, ldd, accumulate);
    return dgnn_check_launch("edge_tv_step");
}
