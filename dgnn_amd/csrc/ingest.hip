// Per-scene feature standardisation on the device: what processing/data.py:444-506 does with
// sklearn.preprocessing.StandardScaler on pandas float64 frames, then toTorch() casts to float32 (:512-519).
//   mean_c, var_c (population) over the scene's rows, columns [c_first, C); scale_c = sqrt(var_c), 0 -> 1;
//   out[i,c] = float((x[i,c] - mean_c) / scale_c);  columns < c_first (the un-scaled loss-weight copy, :485-488) are cast.
// Two passes in fp64 (mean, then centred sum of squares), per-block partials summed in a fixed order.
//
// dgnn_scale_features_f64 (below the standardisation) is the rest of standardizeFeatures: the 'sum' / normalisation-feature / 'edge'
// pre-steps applied on the fly in every pass, then StandardScaler, MinMaxScaler or RobustScaler.  RobustScaler's median and quartiles
// are exact order statistics of the column (most-significant-digit radix selection on order-preserving 64-bit keys, integer counts only:
// reruns are bit-identical and nothing synchronises with the host).  Non-finite inputs are out of scope there as they are here: a NaN
// or an infinity in a scaled column gives the statistics no defined order.
#include "common.h"

namespace {

constexpr int ING_BLOCKS = 512;

// MODE 0: sum x.  MODE 1: sum (x - mean)^2
template <int MODE>
__global__ void __launch_bounds__(256) k_ing_colreduce(const double* __restrict__ x, int64_t ld, int64_t n, int c, int64_t rpb,
                                                       const double* __restrict__ mean, double* __restrict__ partials) {
    __shared__ double red[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * rpb, r1 = min(n, r0 + rpb);
    for (int cb = 0; cb < c; cb += 64) {
        const int col = cb + tx;
        double s = 0.0;
        if (col < c) {
            const double mu = MODE ? mean[col] : 0.0;
            for (int64_t r = r0 + ty; r < r1; r += 4) {
                const double v = x[r * ld + col] - mu;
                s += MODE ? v * v : v;
            }
        }
        red[ty][tx] = s;
        __syncthreads();
        if (ty == 0 && col < c) partials[(int64_t)blockIdx.x * c + col] = ((red[0][tx] + red[1][tx]) + red[2][tx]) + red[3][tx];
        __syncthreads();
    }
}

__global__ void k_ing_finalize(const double* __restrict__ partials, int nblk, int64_t n, int c, int sqrt_it, double* __restrict__ out) {
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= c) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += partials[(int64_t)b * c + col];
    s /= (double)n;
    if (sqrt_it) {
        s = sqrt(s);
        if (s < 10.0 * 2.220446049250313e-16) s = 1.0;  // sklearn _handle_zeros_in_scale
    }
    out[col] = s;
}

__global__ void k_ing_apply(const double* __restrict__ x, int64_t ld, int64_t n, int c, int c_first, const double* __restrict__ mean,
                            const double* __restrict__ scale, float* __restrict__ out, int64_t ldo) {
    const int64_t total = n * c;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = t / c;
        const int col = (int)(t - r * c);
        const double v = x[r * ld + col];
        out[r * ldo + col] = col < c_first ? (float)v : (float)((v - mean[col]) / scale[col]);
    }
}


// ==================================================================================================================================
// Feature scaling with pre-steps (reference processing/data.py:444-506), every pass over v(r,col) = the pre-transformed value, in the
// reference's order and with pandas' operations (no contraction: the file is built with -ffp-contract=off):
//   sum     v = (x*1000)/colsum[col]                col in [sum_c0, sum_c1)     colsum over the raw column
//   div     v = v/(w + 1e-4), w = x[r,div_col] after `sum`, before `div`        col in [div_c0, div_c1)
//   scalar  v = v/scalar                                                        col in [sc_c0, sc_c1)
// Scalers over columns >= c_first (sklearn semantics; a scale below 10 eps becomes 1):
//   standard  two-pass fp64 mean and population variance, as above; also scale 1 for a column that is constant up to rounding (k_sc_stdfin)
//   minmax    rg = max - min; scale = (hi-lo)/rg; out = v*scale + (lo - min*scale)
//   robust    centre = median (mean of the two middle values for an even count), scale = q75 - q25 with numpy's linear rule
//             h = (n-1)p, t = h - floor(h), d = s[hi]-s[lo]:  s[lo] + d*t for t < 0.5, else s[hi] - d*(1-t);  out = (v-centre)/scale
// Selection: v -> key (sign-flipped bits; -0.0 and +0.0 share one key, so the same value comes back whichever the column held).  Eight
// passes of 8 bits from the top: per (column, rank in {q25, median, q75}) a 256-bin histogram of the keys that match the rank's prefix
// so far, counted in an LDS tile of 16 columns (3 x 256 x 16 x 4 B = 48 KB, three blocks to a CU) and merged with integer atomics; one
// wave per (column, rank) then picks the bin that holds the rank.  s[lo+1] comes from one more pass: count(<= s[lo]) and min(> s[lo]).
// Rows are row-major: a wave reads 4 rows x 16 neighbouring columns, a block walks its own row range.
// ==================================================================================================================================
enum { SC_NONE = 0, SC_STANDARD = 1, SC_MINMAX = 2, SC_ROBUST = 3 };
constexpr int SC_CT = 16;          // columns per tile of the selection / extrema kernels
constexpr int SC_RP = 16;          // row phases of a block (256 threads / SC_CT)
constexpr double SC_EPS10 = 10.0 * 2.220446049250313e-16;
typedef unsigned long long u64;

struct ScPre {
    int sum_c0, sum_c1, div_c0, div_c1, div_col, sc_c0, sc_c1;
    double scalar;
    const double* colsum;
};

struct ScCol {                     // what the pre-steps do to one column
    double cs, dcs, scalar;
    int div_col;
    bool sum, div, dsum, sc;
};

__device__ __forceinline__ ScCol sc_col(int col, const ScPre& p) {
    ScCol t;
    t.sum = col >= p.sum_c0 && col < p.sum_c1;
    t.div = col >= p.div_c0 && col < p.div_c1;
    t.dsum = t.div && p.div_col >= p.sum_c0 && p.div_col < p.sum_c1;
    t.sc = col >= p.sc_c0 && col < p.sc_c1;
    t.cs = t.sum ? p.colsum[col] : 1.0;
    t.dcs = t.dsum ? p.colsum[p.div_col] : 1.0;
    t.scalar = p.scalar;
    t.div_col = p.div_col;
    return t;
}

__device__ __forceinline__ double sc_val(const double* __restrict__ row, int col, const ScCol& t) {
    double v = row[col];
    if (t.sum) v = (v * 1000.0) / t.cs;
    if (t.div) {
        double w = row[t.div_col];
        if (t.dsum) w = (w * 1000.0) / t.dcs;
        v = v / (w + 0.0001);
    }
    if (t.sc) v = v / t.scalar;
    return v;
}

__device__ __forceinline__ u64 sc_key(double v) {
    if (v == 0.0) v = 0.0;                                  // -0.0 -> +0.0
    const u64 b = (u64)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double sc_unkey(u64 k) {
    return __longlong_as_double((long long)((k >> 63) ? (k ^ 0x8000000000000000ull) : ~k));
}

__global__ void k_sc_sumfin(const double* __restrict__ partials, int nblk, int c, double* __restrict__ out) {
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= c) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += partials[(int64_t)b * c + col];
    out[col] = s;
}

// sklearn's StandardScaler also takes a column for constant when its variance is within the rounding of its mean (_is_constant_feature:
// var <= n eps var + (n mean eps)^2).  A pre-step turns a constant column into a constant that is no fp64 number times n, whose mean is
// a few ulps off and whose deviations are all that rounding error: without this rule it would come out as +-1 instead of ~0.
__global__ void k_sc_stdfin(const double* __restrict__ partials, int nblk, int64_t n, int c, const double* __restrict__ mean, double* __restrict__ scale) {
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= c) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += partials[(int64_t)b * c + col];
    const double eps = 2.220446049250313e-16, var = s / (double)n, me = (double)n * mean[col] * eps;
    double sd = sqrt(var);
    if (var <= (double)n * eps * var + me * me || sd < SC_EPS10) sd = 1.0;
    scale[col] = sd;
}

// k_ing_colreduce over the pre-transformed values (same rows per thread, same order of the sums)
template <int MODE>
__global__ void __launch_bounds__(256) k_sc_colreduce(const double* __restrict__ x, int64_t ld, int64_t n, int c, int64_t rpb, ScPre pre,
                                                      const double* __restrict__ mean, double* __restrict__ partials) {
    __shared__ double red[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * rpb, r1 = min(n, r0 + rpb);
    for (int cb = 0; cb < c; cb += 64) {
        const int col = cb + tx;
        double s = 0.0;
        if (col < c) {
            const ScCol t = sc_col(col, pre);
            const double mu = MODE ? mean[col] : 0.0;
            for (int64_t r = r0 + ty; r < r1; r += 4) {
                const double v = sc_val(x + r * ld, col, t) - mu;
                s += MODE ? v * v : v;
            }
        }
        red[ty][tx] = s;
        __syncthreads();
        if (ty == 0 && col < c) partials[(int64_t)blockIdx.x * c + col] = ((red[0][tx] + red[1][tx]) + red[2][tx]) + red[3][tx];
        __syncthreads();
    }
}

// selection state per (column, rank): prefix (the key's digits chosen so far), krem (the rank among the keys that share the prefix),
// cnt_le / min_gt (the last pass); extrema per column: kmin / kmax
struct ScSel {
    u64 *prefix, *krem, *cnt_le, *min_gt, *kmin, *kmax;
    uint32_t* hist;                // [c][3][256]
};

__global__ void k_sc_init(ScSel s, int64_t n, int c, int with_hist) {          // with_hist: the selection's histograms (robust); minmax reads none
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (with_hist && i < 3 * c * 256) s.hist[i] = 0u;
    if (i < 3 * c) {
        const int r = i % 3;
        const double h = (double)(n - 1) * (r == 0 ? 0.25 : r == 1 ? 0.5 : 0.75);
        s.prefix[i] = 0ull;
        s.krem[i] = (u64)floor(h);
        s.cnt_le[i] = 0ull;
        s.min_gt[i] = ~0ull;
    }
    if (i < c) {
        s.kmin[i] = ~0ull;
        s.kmax[i] = 0ull;
    }
}

__global__ void __launch_bounds__(256) k_sc_extrema(const double* __restrict__ x, int64_t ld, int64_t n, int c, int c_first, int64_t rpb, ScPre pre,
                                                    ScSel s) {
    __shared__ u64 red[2][SC_RP][SC_CT];
    const int tc = threadIdx.x % SC_CT, tr = threadIdx.x / SC_CT, col = blockIdx.y * SC_CT + tc;
    const int64_t r0 = (int64_t)blockIdx.x * rpb, r1 = min(n, r0 + rpb);
    u64 lo = ~0ull, hi = 0ull;
    if (col < c && col >= c_first) {
        const ScCol t = sc_col(col, pre);
        for (int64_t r = r0 + tr; r < r1; r += SC_RP) {
            const u64 k = sc_key(sc_val(x + r * ld, col, t));
            lo = k < lo ? k : lo;
            hi = k > hi ? k : hi;
        }
    }
    red[0][tr][tc] = lo;
    red[1][tr][tc] = hi;
    __syncthreads();
    if (tr == 0 && col < c && col >= c_first) {
        for (int i = 1; i < SC_RP; ++i) {
            lo = red[0][i][tc] < lo ? red[0][i][tc] : lo;
            hi = red[1][i][tc] > hi ? red[1][i][tc] : hi;
        }
        atomicMin(&s.kmin[col], lo);
        atomicMax(&s.kmax[col], hi);
    }
}

__global__ void __launch_bounds__(256) k_sc_hist(const double* __restrict__ x, int64_t ld, int64_t n, int c, int c_first, int64_t rpb, ScPre pre,
                                                 int shift, ScSel s) {
    __shared__ uint32_t lh[3 * 256 * SC_CT];               // [rank][digit][column of the tile]
    for (int i = threadIdx.x; i < 3 * 256 * SC_CT; i += 256) lh[i] = 0u;
    __syncthreads();
    const int tc = threadIdx.x % SC_CT, tr = threadIdx.x / SC_CT, col0 = blockIdx.y * SC_CT, col = col0 + tc;
    const int64_t r0 = (int64_t)blockIdx.x * rpb, r1 = min(n, r0 + rpb);
    if (col < c && col >= c_first) {
        const ScCol t = sc_col(col, pre);
        const u64 p0 = s.prefix[col * 3], p1 = s.prefix[col * 3 + 1], p2 = s.prefix[col * 3 + 2];
        const u64 above = shift >= 56 ? 0ull : ~0ull << (shift + 8);          // the digits already chosen
        for (int64_t r = r0 + tr; r < r1; r += SC_RP) {
            const u64 k = sc_key(sc_val(x + r * ld, col, t));
            const int d = (int)((k >> shift) & 255);
            if (((k ^ p0) & above) == 0) atomicAdd(&lh[(0 * 256 + d) * SC_CT + tc], 1u);
            if (((k ^ p1) & above) == 0) atomicAdd(&lh[(1 * 256 + d) * SC_CT + tc], 1u);
            if (((k ^ p2) & above) == 0) atomicAdd(&lh[(2 * 256 + d) * SC_CT + tc], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * 256 * SC_CT; i += 256) {
        const uint32_t v = lh[i];
        const int cc = col0 + i % SC_CT, d = (i / SC_CT) & 255, r = i / (SC_CT * 256);
        if (v && cc < c) atomicAdd(&s.hist[((int64_t)cc * 3 + r) * 256 + d], v);
    }
}

// one wave per (column, rank): the bin that holds the rank; the histogram is left zeroed for the next pass
__global__ void __launch_bounds__(256) k_sc_pick(ScSel s, int c, int c_first, int shift) {
    const int lane = threadIdx.x & 63, pair = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= 3 * c || pair / 3 < c_first) return;
    uint32_t* h = s.hist + (int64_t)pair * 256 + lane * 4;
    const uint4 v = *reinterpret_cast<const uint4*>(h);
    *reinterpret_cast<uint4*>(h) = make_uint4(0u, 0u, 0u, 0u);
    const u64 mine = (u64)v.x + v.y + v.z + v.w;
    u64 incl = mine;
    for (int off = 1; off < 64; off <<= 1) {
        const u64 up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
    }
    const u64 k = s.krem[pair];
    u64 cum = incl - mine;
    if (cum <= k && k < incl) {                               // exactly one lane: the counts of a pass sum to more than its rank
        int d = 0;
        if (cum + v.x <= k) {
            cum += v.x, d = 1;
            if (cum + v.y <= k) {
                cum += v.y, d = 2;
                if (cum + v.z <= k) cum += v.z, d = 3;
            }
        }
        s.prefix[pair] |= (u64)(lane * 4 + d) << shift;
        s.krem[pair] = k - cum;
    }
}

__global__ void __launch_bounds__(256) k_sc_next(const double* __restrict__ x, int64_t ld, int64_t n, int c, int c_first, int64_t rpb, ScPre pre,
                                                 ScSel s) {
    __shared__ u64 red[6][SC_RP][SC_CT];
    const int tc = threadIdx.x % SC_CT, tr = threadIdx.x / SC_CT, col = blockIdx.y * SC_CT + tc;
    const int64_t r0 = (int64_t)blockIdx.x * rpb, r1 = min(n, r0 + rpb);
    u64 cnt[3] = {0ull, 0ull, 0ull}, mn[3] = {~0ull, ~0ull, ~0ull};
    const bool on = col < c && col >= c_first;
    if (on) {
        const ScCol t = sc_col(col, pre);
        const u64 v[3] = {s.prefix[col * 3], s.prefix[col * 3 + 1], s.prefix[col * 3 + 2]};
        for (int64_t r = r0 + tr; r < r1; r += SC_RP) {
            const u64 k = sc_key(sc_val(x + r * ld, col, t));
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                cnt[q] += k <= v[q];
                if (k > v[q] && k < mn[q]) mn[q] = k;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        red[q][tr][tc] = cnt[q];
        red[3 + q][tr][tc] = mn[q];
    }
    __syncthreads();
    if (tr == 0 && on) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            for (int i = 1; i < SC_RP; ++i) {
                cnt[q] += red[q][i][tc];
                mn[q] = red[3 + q][i][tc] < mn[q] ? red[3 + q][i][tc] : mn[q];
            }
            atomicAdd(&s.cnt_le[col * 3 + q], cnt[q]);
            atomicMin(&s.min_gt[col * 3 + q], mn[q]);
        }
    }
}

// per column: a (subtracted), b (divided by), and for minmax the scale and offset of the transform; stats [2][c] when asked for
__global__ void k_sc_params(int kind, int64_t n, int c, int c_first, double range_lo, double range_hi, ScSel s, double* __restrict__ a,
                            double* __restrict__ b, double* __restrict__ mul, double* __restrict__ add, double* __restrict__ stats) {
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= c) return;
    double sub = 0.0, div = 1.0;
    if (col >= c_first) {
        if (kind == SC_STANDARD) {
            sub = a[col];
            div = b[col];
        } else if (kind == SC_MINMAX) {
            sub = sc_unkey(s.kmin[col]);
            div = sc_unkey(s.kmax[col]) - sub;
            if (div < SC_EPS10) div = 1.0;
            const double sc = (range_hi - range_lo) / div;
            mul[col] = sc;
            add[col] = range_lo - sub * sc;
        } else if (kind == SC_ROBUST) {
            double q[3];
            for (int r = 0; r < 3; ++r) {
                const double h = (double)(n - 1) * (r == 0 ? 0.25 : r == 1 ? 0.5 : 0.75);
                const double fl = floor(h), t = h - fl;
                const u64 lo = (u64)fl;
                const double slo = sc_unkey(s.prefix[col * 3 + r]);
                double shi = slo;                                               // s[lo+1]: still s[lo] while lo+1 < count(<= s[lo])
                if (lo + 1 < (u64)n && s.cnt_le[col * 3 + r] < lo + 2) shi = sc_unkey(s.min_gt[col * 3 + r]);
                const double d = shi - slo;
                if (r == 1) q[r] = (n & 1) ? slo : (slo + shi) / 2.0;
                else q[r] = t < 0.5 ? slo + d * t : shi - d * (1.0 - t);
            }
            sub = q[1];
            div = q[2] - q[0];
            if (div < SC_EPS10) div = 1.0;
        }
    }
    a[col] = sub;
    b[col] = div;
    if (stats) {
        stats[col] = sub;
        stats[c + col] = div;
    }
}

__global__ void k_sc_apply(const double* __restrict__ x, int64_t ld, int64_t n, int c, int c_first, int kind, ScPre pre, const double* __restrict__ a,
                           const double* __restrict__ b, const double* __restrict__ mul, const double* __restrict__ add,
                           float* __restrict__ out, int64_t ldo) {
    const int64_t total = n * c;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = t / c;
        const int col = (int)(t - r * c);
        double v = sc_val(x + r * ld, col, sc_col(col, pre));
        if (col >= c_first) {
            if (kind == SC_MINMAX) v = v * mul[col] + add[col];
            else if (kind != SC_NONE) v = (v - a[col]) / b[col];
        }
        out[r * ldo + col] = (float)v;
    }
}

}  // namespace

// scratch: doubles: partials [ING_BLOCKS][c] + mean [c] + scale [c]
extern "C" int64_t dgnn_standardize_scratch_doubles(int c) { return (int64_t)ING_BLOCKS * c + 2 * c; }

extern "C" int dgnn_standardize_f64(const double* x, int64_t ld, int64_t n, int c, int c_first, float* out, int64_t ldo,
                                    double* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(n > 0 && c > 0 && c_first >= 0 && c_first <= c && x && out && scratch, DGNN_E_INVALID, "standardize_f64: bad args");
    double* partials = scratch;
    double* mean = scratch + (int64_t)ING_BLOCKS * c;
    double* scale = mean + c;
    int nblk = (int)(dgnn_cdiv(n, 64) < ING_BLOCKS ? dgnn_cdiv(n, 64) : ING_BLOCKS);
    const int64_t rpb = dgnn_cdiv(n, nblk);
    nblk = (int)dgnn_cdiv(n, rpb);
    hipLaunchKernelGGL((k_ing_colreduce<0>), dim3(nblk), dim3(256), 0, stream, x, ld, n, c, rpb, nullptr, partials);
    hipLaunchKernelGGL(k_ing_finalize, dim3((c + 255) / 256), dim3(256), 0, stream, partials, nblk, n, c, 0, mean);
    hipLaunchKernelGGL((k_ing_colreduce<1>), dim3(nblk), dim3(256), 0, stream, x, ld, n, c, rpb, mean, partials);
    hipLaunchKernelGGL(k_ing_finalize, dim3((c + 255) / 256), dim3(256), 0, stream, partials, nblk, n, c, 1, scale);
    hipLaunchKernelGGL(k_ing_apply, dim3(dgnn_grid_cap(dgnn_cdiv(n * c, 256))), dim3(256), 0, stream, x, ld, n, c, c_first, mean, scale,
                       out, ldo);
    return dgnn_check_launch("standardize_f64");
}

// scratch (bytes): the 32-bit histograms [3c][256] (16-byte aligned rows); doubles partials [ING_BLOCKS][c], colsum / a / b / mul / add [c]
// each; then the selection state: 64-bit prefix, krem, cnt_le, min_gt [3c] each and kmin, kmax [c] each
extern "C" int64_t dgnn_scale_features_scratch_bytes(int c) {
    return ((int64_t)ING_BLOCKS * c + 5 * c) * 8 + (int64_t)(12 * c + 2 * c) * 8 + (int64_t)3 * c * 256 * 4;
}

extern "C" int dgnn_scale_features_f64(const double* x, int64_t ld, int64_t n, int c, int c_first, int kind, double range_lo, double range_hi,
                                       int sum_c0, int sum_c1, int div_col, int div_c0, int div_c1, double div_scalar, int sc_c0, int sc_c1,
                                       float* out, int64_t ldo, double* stats, void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DGNN_REQUIRE(n > 0 && n < ((int64_t)1 << 32) && c > 0 && c_first >= 0 && c_first <= c && ld >= c && ldo >= c && x && out && scratch,
                 DGNN_E_INVALID, "scale_features_f64: bad args");
    DGNN_REQUIRE(kind >= SC_NONE && kind <= SC_ROBUST, DGNN_E_INVALID, "scale_features_f64: kind %d (0 none, 1 standard, 2 minmax, 3 robust)", kind);
    const bool has_sum = sum_c0 < sum_c1, has_div = div_c0 < div_c1, has_sc = sc_c0 < sc_c1;
    DGNN_REQUIRE((!has_sum || (sum_c0 >= 0 && sum_c1 <= c)) && (!has_div || (div_c0 >= 0 && div_c1 <= c && div_col >= 0 && div_col < c)) &&
                     (!has_sc || (sc_c0 >= 0 && sc_c1 <= c)),
                 DGNN_E_INVALID, "scale_features_f64: a pre-step's columns lie outside [0, %d)", c);
    double* partials = (double*)((char*)scratch + (int64_t)3 * c * 256 * 4);
    double* colsum = partials + (int64_t)ING_BLOCKS * c;
    double *a = colsum + c, *b = a + c, *mul = b + c, *add = mul + c;
    ScSel s;
    s.prefix = (u64*)(add + c);
    s.krem = s.prefix + 3 * c;
    s.cnt_le = s.krem + 3 * c;
    s.min_gt = s.cnt_le + 3 * c;
    s.kmin = s.min_gt + 3 * c;
    s.kmax = s.kmin + c;
    s.hist = (uint32_t*)scratch;
    ScPre pre;
    pre.sum_c0 = has_sum ? sum_c0 : 0;  pre.sum_c1 = has_sum ? sum_c1 : 0;
    pre.div_c0 = has_div ? div_c0 : 0;  pre.div_c1 = has_div ? div_c1 : 0;  pre.div_col = has_div ? div_col : 0;
    pre.sc_c0 = has_sc ? sc_c0 : 0;     pre.sc_c1 = has_sc ? sc_c1 : 0;     pre.scalar = div_scalar;
    pre.colsum = colsum;
    int nblk = (int)(dgnn_cdiv(n, 64) < ING_BLOCKS ? dgnn_cdiv(n, 64) : ING_BLOCKS);
    const int64_t rpb = dgnn_cdiv(n, nblk);
    nblk = (int)dgnn_cdiv(n, rpb);
    const dim3 cgrid((c + 255) / 256), tiles(nblk, (c + SC_CT - 1) / SC_CT);
    if (has_sum) {
        hipLaunchKernelGGL((k_ing_colreduce<0>), dim3(nblk), dim3(256), 0, stream, x, ld, n, c, rpb, nullptr, partials);
        hipLaunchKernelGGL(k_sc_sumfin, cgrid, dim3(256), 0, stream, partials, nblk, c, colsum);
    }
    if (kind == SC_STANDARD) {
        hipLaunchKernelGGL((k_sc_colreduce<0>), dim3(nblk), dim3(256), 0, stream, x, ld, n, c, rpb, pre, nullptr, partials);
        hipLaunchKernelGGL(k_ing_finalize, cgrid, dim3(256), 0, stream, partials, nblk, n, c, 0, a);
        hipLaunchKernelGGL((k_sc_colreduce<1>), dim3(nblk), dim3(256), 0, stream, x, ld, n, c, rpb, pre, a, partials);
        hipLaunchKernelGGL(k_sc_stdfin, cgrid, dim3(256), 0, stream, partials, nblk, n, c, a, b);
    } else if (kind == SC_MINMAX || kind == SC_ROBUST) {
        const int with_hist = kind == SC_ROBUST;
        hipLaunchKernelGGL(k_sc_init, dim3(with_hist ? 3 * c : (3 * c + 255) / 256), dim3(256), 0, stream, s, n, c, with_hist);
        if (kind == SC_MINMAX) {
            hipLaunchKernelGGL(k_sc_extrema, tiles, dim3(256), 0, stream, x, ld, n, c, c_first, rpb, pre, s);
        } else {
            for (int shift = 56; shift >= 0; shift -= 8) {
                hipLaunchKernelGGL(k_sc_hist, tiles, dim3(256), 0, stream, x, ld, n, c, c_first, rpb, pre, shift, s);
                hipLaunchKernelGGL(k_sc_pick, dim3((3 * c + 3) / 4), dim3(256), 0, stream, s, c, c_first, shift);
            }
            hipLaunchKernelGGL(k_sc_next, tiles, dim3(256), 0, stream, x, ld, n, c, c_first, rpb, pre, s);
        }
    }
    hipLaunchKernelGGL(k_sc_params, cgrid, dim3(256), 0, stream, kind, n, c, c_first, range_lo, range_hi, s, a, b, mul, add, stats);
    hipLaunchKernelGGL(k_sc_apply, dim3(dgnn_grid_cap(dgnn_cdiv(n * c, 256))), dim3(256), 0, stream, x, ld, n, c, c_first, kind, pre, a, b, mul,
                       add, out, ldo);
    return dgnn_check_launch("scale_features_f64");
}
