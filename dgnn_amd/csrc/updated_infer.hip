// Whole-scene inference of the Updated SurfaceNet (learning/surfaceNetUpdatedEdgeFilters.py forward, :216-251, on adjs = [(edge_index, arange(E), (N, N))] * L).
// On a whole graph every layer's e_id is the identity, so the reference's edge chaining (zeros[E_all, C]; [e_prev] = phi; relu; [e_id, :k]) is
// ea_{k+1} = relu(phi_k)[:, :k]: a per-edge MLP chain beside the node rows.  One launch per conv layer (k_edge_chain_agg) covers lin_e, the mean aggregate
// and the next layer's edge rows -- the pre-ReLU phi never exists in memory -- and dgnn_updated_infer_fwd issues a scene's layers and the "sage+" output
// network back to back.  Layer shapes outside the launch take the per-layer calls (dgnn_sage_updated_train_fwd) with the ReLU applied in place.
//
// k_edge_chain_agg: a workgroup owns TD = 16 consecutive destinations at a time and walks their plan positions [rowptr[d0], rowptr[d0 + 16]) in tiles of
// TE = 64; a destination's sum is carried in its owner's registers from tile to tile, so a segment may straddle any number of tile boundaries and is still
// added up in plan order from 0 (the order and operations of aggregate.hip: acc = acc + x * phi, then / max(deg, 1)).  A reference-layout scene has 4 in-edges
// per cell: one tile per group.  Per tile:
//   0. what does not depend on phi is requested first and lands under the products: the next tile's edge ids, the ids of the rows to store, the first 4
//      neighbour rows x[src[k]] of every destination's piece of the tile;
//   1. the tile's edge rows ea[eid[k], :k_e] (requested one tile ahead, into registers) are written into LDS as the A operand, K zero-padded to KP there;
//   2. phi = ea . We^T + be on the matrix cores, We resident in LDS for the whole launch, in the arithmetic gemm.hip prescribes for the GEMM mode:
//      x3 (gemm_x3.h: both operands split in 3 bf16 parts, six products per k-step in THE order, bias added behind) -- the bits of dgnn_linear_fwd_x3 --
//      or, exact fp32, v_mfma_f32_16x16x4_f32 with the bias as the C input: per (edge, channel) the fmaf chain over ascending k that starts at the bias;
//   3. phi goes through an LDS tile (it takes the place of the A operand) to the two consumers: relu(phi) rows to ea_next[eid[k]] (whole 256 / 512-byte rows
//      per 16 / 32 lanes), and the owners' sums, C / 4 lanes per destination gathering x[src[k]] 16 bytes per lane.
// LDS at c_in = k_e = 128 in x3: 98 KiB of We parts + 49 KiB of tile = 147 of the 160 KiB, one workgroup of 8 wavefronts per CU; the smaller shapes fit 2 - 5.
#include "gemm_x3.h"

namespace {

constexpr int TE = 64;   // plan positions per tile
constexpr int TD = 16;   // destinations a workgroup owns at a time

typedef float f32x4v __attribute__((ext_vector_type(4)));

template <int C, int KP, bool EXACT>
struct Geo {
    static constexpr int T = 4 * C;                          // threads: C / 4 lanes per row x 16 rows
    static constexpr int NP = TE * KP / 4 / T;               // 16-byte pieces of the tile's edge rows per thread
    static constexpr int ROWB = EXACT ? (KP + 2) * 4 : 6 * KP + 16;   // operand row in LDS: fp32 + 2 pad floats (conflict-free 4-byte fragment reads), or
                                                                      // [hi | mid | lo] x KP bf16 + 16 B (an odd number of 16-byte slots, as gemm.hip's)
    static constexpr int LDP = C + 4;                        // phi tile row, floats
    static constexpr int W_BYTES = C * ROWB;
    static constexpr int A_BYTES = TE * ROWB, P_BYTES = TE * LDP * 4;
    static constexpr int LDS = W_BYTES + (A_BYTES > P_BYTES ? A_BYTES : P_BYTES);
};

// one 16-byte piece (4 consecutive k) of an operand row into its LDS image
template <int KP, bool EXACT>
__device__ __forceinline__ void put_piece(char* row, int c4, f32x4v v) {
    if constexpr (EXACT) {
        float* d = reinterpret_cast<float*>(row) + c4;
        *reinterpret_cast<float2*>(d) = make_float2(v[0], v[1]);
        *reinterpret_cast<float2*>(d + 2) = make_float2(v[2], v[3]);
    } else {
        uint32_t h0, m0, l0, h1, m1, l1;
        x3_split(v[0], v[1], h0, m0, l0);
        x3_split(v[2], v[3], h1, m1, l1);
        char* d = row + c4 * 2;
        *reinterpret_cast<uint2*>(d) = make_uint2(h0, h1);
        *reinterpret_cast<uint2*>(d + KP * 2) = make_uint2(m0, m1);
        *reinterpret_cast<uint2*>(d + KP * 4) = make_uint2(l0, l1);
    }
}

// 4 consecutive k of a global row, zeros from k_e on; vec: the row is 16-byte aligned and k_e % 4 == 0 (a piece is all in or all out)
__device__ __forceinline__ f32x4v get_piece(const float* __restrict__ row, int c4, int k_e, bool vec) {
    f32x4v v = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
        if (c4 < k_e) v = *reinterpret_cast<const f32x4v*>(row + c4);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c4 + j < k_e) v[j] = row[c4 + j];
    }
    return v;
}

template <int C, int KP, bool EXACT>
__global__ void __launch_bounds__(4 * C) k_edge_chain_agg(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ src, const int32_t* __restrict__ eid,
                                                          int64_t n_dst, const float* __restrict__ x, int64_t ldx, const float* __restrict__ ea, int64_t lde,
                                                          int k_e, int vec, const float* __restrict__ We, const float* __restrict__ be,
                                                          float* __restrict__ a, int64_t lda, float* __restrict__ ea_next, int64_t ldn, int write_next) {
    typedef Geo<C, KP, EXACT> G;
    constexpr int T = G::T, NP = G::NP, ROWB = G::ROWB, LDP = G::LDP, QL = C / 4, PR = KP / 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const Ws = smem;
    char* const As = smem + G::W_BYTES;
    float* const phi_t = reinterpret_cast<float*>(As);       // the tile's phi takes the A operand's place once the products have read it
    const int tid = threadIdx.x, lane = lane_id(), w = wave_id_uniform();
    const int64_t ngroups = (n_dst + TD - 1) / TD;
    if ((int64_t)blockIdx.x >= ngroups) return;

    // We [C, k_e] -> the resident B operand
    for (int i = tid; i < C * PR; i += T) {
        const int n = i / PR, c4 = (i % PR) * 4;
        put_piece<KP, EXACT>(Ws + n * ROWB, c4, get_piece(We + (int64_t)n * k_e, c4, k_e, false));
    }

    f32x4v ra[NP];
    auto load_tile = [&](int c0, int nv) {       // edge rows of the plan positions [c0, c0 + nv), zeros behind them
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int i = tid + p * T, r = i / PR, c4 = (i % PR) * 4;
            f32x4v v = {0.f, 0.f, 0.f, 0.f};
            if (r < nv) {
                const int64_t e_ = eid ? eid[c0 + r] : c0 + r;
                v = get_piece(ea + e_ * lde, c4, k_e, vec != 0);
            }
            ra[p] = v;
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int i = tid + p * T, r = i / PR, c4 = (i % PR) * 4;
            put_piece<KP, EXACT>(As + r * ROWB, c4, ra[p]);
        }
    };

    const int j = tid / QL, q4 = (tid % QL) * 4;        // this thread's destination of the group and its 4 channels
    int pf_c0 = -1;                                      // the tile `ra` holds
    for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const int64_t d0 = g * TD;
        const int nd = (int)(n_dst - d0 < TD ? n_dst - d0 : TD);
        const int e_lo = rowptr[d0], e_hi = rowptr[d0 + nd];
        const bool dv = j < nd;
        const int sb = dv ? rowptr[d0 + j] : 0, se = dv ? rowptr[d0 + j + 1] : 0;
        f32x4v acc = {0.f, 0.f, 0.f, 0.f};
        for (int c0 = e_lo; c0 < e_hi; c0 += TE) {
            const int nv = e_hi - c0 < TE ? e_hi - c0 : TE;
            // Everything that does not depend on phi is requested FIRST and lands under the products: the next tile's position (and its edge ids), the ids
            // of the rows this thread stores, and the first 4 neighbour rows of its destination's piece of the tile (a Delaunay cell has 4).
            int nc0 = c0 + TE, nhi = e_hi;
            if (nc0 >= e_hi) {
                const int64_t g2 = g + gridDim.x;
                nc0 = nhi = 0;
                if (g2 < ngroups) {
                    const int64_t d2 = g2 * TD;
                    nc0 = rowptr[d2];
                    nhi = rowptr[d2 + (n_dst - d2 < TD ? n_dst - d2 : TD)];
                }
            }
            const int nnv = nc0 < nhi ? (nhi - nc0 < TE ? nhi - nc0 : TE) : 0;
            const int lo = sb > c0 ? sb : c0, hi = se < c0 + nv ? se : c0 + nv;
            f32x4v xv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) xv[u] = f32x4v{0.f, 0.f, 0.f, 0.f};
            if (lo < hi) {
#pragma unroll
                for (int u = 0; u < 4; ++u) xv[u] = *reinterpret_cast<const f32x4v*>(x + (int64_t)src[lo + u < hi ? lo + u : hi - 1] * ldx + q4);
            }
            int er[TE / TD], pe[NP];
#pragma unroll
            for (int i = 0; i < TE / TD; ++i) {
                const int r = j + i * TD;
                er[i] = (write_next && r < nv) ? (eid ? eid[c0 + r] : c0 + r) : -1;
            }
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const int r = (tid + p * T) / PR;
                pe[p] = r < nnv ? (eid ? eid[nc0 + r] : nc0 + r) : -1;
            }
            if (pf_c0 != c0) load_tile(c0, nv);
            store_tile();
            __syncthreads();                             // (the first tile: We is in place too)
            if constexpr (EXACT) {
                // wavefront w: channels 16 w .. 16 w + 15 of the tile's 4 blocks of 16 edges; lane (n = lane & 15, kq = lane >> 4)
                const int fn = lane & 15, kq = lane >> 4;
                const float bias = be[16 * w + fn];
                f32x4v d[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) d[m] = f32x4v{bias, bias, bias, bias};
                const float* bp = reinterpret_cast<const float*>(Ws + (16 * w + fn) * ROWB) + kq;
                const float* ap = reinterpret_cast<const float*>(As + fn * ROWB) + kq;
#pragma unroll 4
                for (int ks = 0; ks < KP / 4; ++ks) {
                    const float bv = bp[4 * ks];
#pragma unroll
                    for (int m = 0; m < 4; ++m)
                        d[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[m * 16 * (ROWB / 4) + 4 * ks], bv, d[m], 0, 0, 0);
                }
                __syncthreads();                         // every wavefront has read the A operand
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int r = 0; r < 4; ++r) phi_t[(16 * m + 4 * kq + r) * LDP + 16 * w + fn] = d[m][r];
            } else {
                // wavefront w: the 32 x 32 block (edges 32 mb .., channels 32 nb ..); k-steps ascending, six products each (x3_mma6)
                constexpr int NBW = C / 32;
                const int mb = w / NBW, nb = w % NBW, h = lane >> 5, l31 = lane & 31;
                f32x16 pacc;
#pragma unroll
                for (int r = 0; r < 16; ++r) pacc[r] = 0.f;
                const char* ap = As + (32 * mb + l31) * ROWB + h * 16;
                const char* bp = Ws + (32 * nb + l31) * ROWB + h * 16;
#pragma unroll 2
                for (int S = 0; S < KP / 16; ++S) {
                    bf16x8_t af[3], bf[3];
#pragma unroll
                    for (int p = 0; p < 3; ++p) {
                        af[p] = *reinterpret_cast<const bf16x8_t*>(ap + p * KP * 2 + S * 32);
                        bf[p] = *reinterpret_cast<const bf16x8_t*>(bp + p * KP * 2 + S * 32);
                    }
                    x3_mma6(pacc, af, bf);
                }
                const float bias = be[32 * nb + l31];
                __syncthreads();                         // every wavefront has read the A operand
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    phi_t[(32 * mb + (r & 3) + 8 * (r >> 2) + 4 * h) * LDP + 32 * nb + l31] = pacc[r] + bias;
            }
            // the next tile's rows: in flight under this tile's stores and sums
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                f32x4v v = {0.f, 0.f, 0.f, 0.f};
                if (pe[p] >= 0) v = get_piece(ea + (int64_t)pe[p] * lde, ((tid + p * T) % PR) * 4, k_e, vec != 0);
                ra[p] = v;
            }
            pf_c0 = nnv > 0 ? nc0 : -1;
            __syncthreads();
#pragma unroll
            for (int i = 0; i < TE / TD; ++i)
                if (er[i] >= 0) {
                    const f32x4v v = *reinterpret_cast<const f32x4v*>(phi_t + (j + i * TD) * LDP + q4);
                    *reinterpret_cast<f32x4v*>(ea_next + (int64_t)er[i] * ldn + q4) =
                        f32x4v{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
                }
            for (int k = lo; k < hi; k += 4) {           // 4 rows in flight; added in plan order
                if (k > lo) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) xv[u] = *reinterpret_cast<const f32x4v*>(x + (int64_t)src[k + u < hi ? k + u : hi - 1] * ldx + q4);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (k + u < hi) {
                        const f32x4v pv = *reinterpret_cast<const f32x4v*>(phi_t + (k + u - c0) * LDP + q4);
#pragma unroll
                        for (int t = 0; t < 4; ++t) acc[t] = __fadd_rn(acc[t], __fmul_rn(xv[u][t], pv[t]));
                    }
            }
            __syncthreads();                             // the phi tile has been read: the next tile's operand may take its place
        }
        if (dv) {
            const float cnt = (float)(se - sb > 1 ? se - sb : 1);
            *reinterpret_cast<f32x4v*>(a + (d0 + j) * lda + q4) =
                f32x4v{__fdiv_rn(acc[0], cnt), __fdiv_rn(acc[1], cnt), __fdiv_rn(acc[2], cnt), __fdiv_rn(acc[3], cnt)};
        }
    }
}

inline int kpad(int k_e) { return k_e <= 32 ? 32 : (k_e <= 64 ? 64 : 128); }

struct ChainArgs {
    const int32_t *rowptr, *src, *eid;
    int64_t n_dst;
    const float* x;
    int64_t ldx;
    const float* ea;
    int64_t lde;
    int k_e;
    const float *We, *be;
    float* a;
    int64_t lda;
    float* ea_next;
    int64_t ldn;
    int write_next;
    hipStream_t stream;
};

template <int C, int KP, bool EXACT>
int launch_chain(const ChainArgs& c) {
    typedef Geo<C, KP, EXACT> G;
    static bool done[DGNN_MAX_DEVICES];
    const void* kern = reinterpret_cast<const void*>(&k_edge_chain_agg<C, KP, EXACT>);
    dgnn_allow_dynamic_lds(kern, G::LDS, done);
    int per_cu = (160 * 1024) / G::LDS;
    if (per_cu > 2048 / G::T) per_cu = 2048 / G::T;
    const int64_t ngroups = dgnn_cdiv(c.n_dst, TD);
    const int vec = (c.k_e % 4 == 0 && c.lde % 4 == 0 && ((uintptr_t)c.ea % 16) == 0) ? 1 : 0;
    hipLaunchKernelGGL((k_edge_chain_agg<C, KP, EXACT>), dim3(dgnn_grid_cap(ngroups, per_cu)), dim3(G::T), G::LDS, c.stream, c.rowptr, c.src, c.eid, c.n_dst,
                       c.x, c.ldx, c.ea, c.lde, c.k_e, vec, c.We, c.be, c.a, c.lda, c.ea_next, c.ldn, c.write_next);
    return dgnn_check_launch("edge_chain_aggregate_fwd");
}

template <bool EXACT>
int launch_chain_mode(const ChainArgs& c, int c_in) {
#define DGNN_CHAIN_CASE(CC, KK) \
    if (c_in == CC && kpad(c.k_e) == KK) return launch_chain<CC, KK, EXACT>(c);
    DGNN_CHAIN_CASE(64, 32)
    DGNN_CHAIN_CASE(64, 64)
    DGNN_CHAIN_CASE(64, 128)
    DGNN_CHAIN_CASE(128, 32)
    DGNN_CHAIN_CASE(128, 64)
    DGNN_CHAIN_CASE(128, 128)
#undef DGNN_CHAIN_CASE
    return DGNN_E_UNSUPPORTED;
}

inline int64_t align16(int64_t v) { return (v + 15) / 16 * 16; }

#define DGNN_TRY(call)                    \
    do {                                  \
        const int rc_ = (call);           \
        if (rc_ != DGNN_OK) return rc_;   \
    } while (0)

}  // namespace

// the layer shapes k_edge_chain_agg takes: fp32 rows of 64 or 128 channels, 1 .. 128 edge columns (row layout: see dgnn_edge_chain_aggregate_fwd)
extern "C" int dgnn_edge_chain_aggregate_supported(int c_in, int k_e, int bf16, int gemm_mode) {
    return (!bf16 && (c_in == 64 || c_in == 128) && k_e >= 1 && k_e <= 128 && gemm_mode >= DGNN_GEMM_F32 && gemm_mode <= DGNN_GEMM_F16X2) ? 1 : 0;
}

extern "C" int dgnn_edge_chain_aggregate_fwd(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int64_t n_dst, const float* x, int64_t ldx, int c_in,
                                             const float* ea, int64_t lde, int k_e, const float* We, const float* be, float* a, int64_t lda, float* ea_next,
                                             int64_t ldn, int write_next, int gemm_mode, void* stream) {
    DGNN_REQUIRE(n_dst >= 0 && c_in > 0 && k_e > 0 && lde >= k_e && ldx >= c_in && lda >= c_in, DGNN_E_INVALID, "edge_chain_aggregate_fwd: bad sizes");
    if (!dgnn_edge_chain_aggregate_supported(c_in, k_e, 0, gemm_mode) || ldx % 4 || lda % 4 || ((uintptr_t)x % 16) || ((uintptr_t)a % 16) ||
        (write_next && (ldn < c_in || ldn % 4 || ((uintptr_t)ea_next % 16)))) {
        dgnn_set_error("edge_chain_aggregate_fwd: c_in %d / k_e %d / row layout outside the launch", c_in, k_e);
        return DGNN_E_UNSUPPORTED;
    }
    if (n_dst == 0) return DGNN_OK;
    DGNN_REQUIRE(rowptr && src && x && ea && We && be && a && (!write_next || ea_next), DGNN_E_INVALID, "edge_chain_aggregate_fwd: null pointer");
    const ChainArgs c{rowptr, src, eid, n_dst, x, ldx, ea, lde, k_e, We, be, a, lda, ea_next, ldn, write_next ? 1 : 0, (hipStream_t)stream};
    return gemm_mode == DGNN_GEMM_F32 ? launch_chain_mode<true>(c, c_in) : launch_chain_mode<false>(c, c_in);
}

// workspace of dgnn_updated_infer_fwd: a [n, max c_in] | y0, y1 [n, max c_out] | h [n, hdim] | (bf16) the first layer's edge columns [E, edge_in_0 rounded up to even]
extern "C" int64_t dgnn_updated_infer_workspace_bytes(int64_t n, int64_t E, int n_layers, const int32_t* widths, const int32_t* edge_in, int hdim, int bf16) {
    if (n < 0 || E < 0 || n_layers < 1 || !widths || !edge_in) return 0;
    int ci = 0, co = 0;
    for (int l = 0; l < n_layers; ++l) {
        ci = widths[l] > ci ? widths[l] : ci;
        co = widths[l + 1] > co ? widths[l + 1] : co;
    }
    const int64_t esz = bf16 ? 2 : 4;
    return align16(n * ci * esz) + 2 * align16(n * co * esz) + align16(n * (int64_t)(hdim > 0 ? hdim : 0) * esz) +
           (bf16 ? align16(E * (int64_t)((edge_in[0] + 1) / 2 * 2) * 2) : 0) + 16;
}

// All conv layers of a scene and the "sage+" output network, one call.  One plan (rowptr, src, eid) for every layer, n sources = n destinations; x [n, widths[0]]
// in the storage type; edge_attr fp32 [E, >= edge_in[0]] in scene edge order.  ea_buf[0 / 1]: the caller's ping-pong edge buffers, [E, max_l<L-1 widths[l]]
// (L: the fall-back route also writes the last layer's phi) elements of the storage type each; layer l's relu(phi) rows (stride widths[l]) are layer l + 1's edge
// input.  W1 NULL: no output network, `out` receives the last layer's rows [n, widths[L]] in the storage type; else fp32 logits [n, n_out].
// fused_layers (host, may be NULL): bit l is set when layer l ran through k_edge_chain_agg.
extern "C" int dgnn_updated_infer_fwd(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int64_t n, int64_t E, const void* x, int64_t ldx,
                                      const float* edge_attr, int64_t lde, int n_layers, const int32_t* widths, const int32_t* edge_in, const float* const* We,
                                      const float* const* be, const float* const* Wl, const float* const* bl, const float* const* Wr, const int32_t* relu,
                                      const float* W1, const float* b1, int hdim, const float* W3, const float* b3, int n_out, void* ea_buf0, void* ea_buf1,
                                      void* workspace, void* out, int32_t* fused_layers, int bf16, int gemm_mode, void* stream) {
    const char* who = "updated_infer_fwd";
    DGNN_REQUIRE(n > 0 && E >= 0 && n_layers >= 1 && n_layers <= 16 && widths && edge_in && We && be && Wl && bl && Wr && relu, DGNN_E_INVALID,
                 "%s: bad sizes / null table", who);
    DGNN_REQUIRE(rowptr && src && x && (E == 0 || (edge_attr && ea_buf0 && ea_buf1)) && workspace && out && ((uintptr_t)workspace % 16) == 0 &&
                     ((uintptr_t)ea_buf0 % 16) == 0 && ((uintptr_t)ea_buf1 % 16) == 0,
                 DGNN_E_INVALID, "%s: null / unaligned pointer", who);
    DGNN_REQUIRE(!W1 || (W3 && hdim > 0 && n_out > 0), DGNN_E_INVALID, "%s: incomplete output network", who);
    for (int l = 0; l < n_layers; ++l)
        DGNN_REQUIRE(widths[l] > 0 && widths[l + 1] > 0 && edge_in[l] > 0 && We[l] && be[l] && Wl[l] && (l == 0 ? edge_in[0] <= lde : edge_in[l] <= widths[l - 1]),
                     DGNN_E_INVALID, "%s: layer %d: bad widths / edge columns / null parameter", who, l);
    const int64_t esz = bf16 ? 2 : 4;
    int ci = 0, co = 0;
    for (int l = 0; l < n_layers; ++l) {
        ci = widths[l] > ci ? widths[l] : ci;
        co = widths[l + 1] > co ? widths[l + 1] : co;
    }
    char* wsp = static_cast<char*>(workspace);
    void* a = wsp;
    wsp += align16(n * ci * esz);
    void* ybuf[2] = {wsp, wsp + align16(n * co * esz)};
    wsp += 2 * align16(n * co * esz);
    void* h = wsp;
    wsp += align16(n * (int64_t)(hdim > 0 ? hdim : 0) * esz);
    void* eab[2] = {ea_buf0, ea_buf1};
    const void* ea = edge_attr;
    int64_t ld_ea = lde;
    if (bf16 && E > 0) {       // forward()'s cast of the first layer's edge columns
        const int k0 = edge_in[0], kp = (k0 + 1) / 2 * 2;
        DGNN_TRY(dgnn_cast_f32_to_bf16(edge_attr, lde, E, k0, kp, (uint16_t*)wsp, kp, stream));
        ea = wsp;
        ld_ea = kp;
    }
    const void* xin = x;
    int64_t ldxin = ldx;
    int32_t fused = 0;
    for (int l = 0; l < n_layers; ++l) {
        const int c_in = widths[l], c_out = widths[l + 1], k = edge_in[l];
        const bool last = l == n_layers - 1;
        void* y = (last && !W1) ? out : ybuf[l & 1];
        void* nxt = eab[l & 1];
        int rc = DGNN_E_UNSUPPORTED;
        if (E > 0 && dgnn_edge_chain_aggregate_supported(c_in, k, bf16, gemm_mode)) {
            rc = dgnn_edge_chain_aggregate_fwd(rowptr, src, eid, n, (const float*)xin, ldxin, c_in, (const float*)ea, ld_ea, k, We[l], be[l], (float*)a, c_in,
                                               (float*)nxt, c_in, last ? 0 : 1, gemm_mode, stream);
            if (rc == DGNN_OK)      // :159-165 behind the launch: y = relu?(a . Wl^T + x . Wr^T + bl)
                rc = gemm_mode == DGNN_GEMM_F32
                         ? dgnn_linear_fwd((const float*)a, c_in, c_in, Wl[l], c_in, Wr[l] ? (const float*)xin : nullptr, ldxin, Wr[l] ? c_in : 0, Wr[l], c_in, bl[l],
                                           nullptr, nullptr, relu[l] ? 1 : 0, n, c_out, (float*)y, c_out, stream)
                         : dgnn_linear_fwd_x3((const float*)a, c_in, c_in, Wl[l], c_in, Wr[l] ? (const float*)xin : nullptr, ldxin, Wr[l] ? c_in : 0, Wr[l], c_in,
                                              bl[l], nullptr, nullptr, relu[l] ? 1 : 0, n, c_out, (float*)y, c_out, stream);
            if (rc == DGNN_OK) fused |= 1 << l;
        }
        if (rc == DGNN_E_UNSUPPORTED) {      // the per-layer calls: linear -> aggregate(phi) -> linear2, the whole-scene ReLU in place
            rc = dgnn_sage_updated_train_fwd(rowptr, src, eid, n, xin, ldxin, c_in, ea, ld_ea, k, E, We[l], be[l], Wl[l], bl[l], Wr[l], c_out, relu[l], nxt, a, y,
                                             bf16, gemm_mode, stream);
            if (rc == DGNN_OK && !last && E > 0)
                rc = bf16 ? dgnn_relu_bf16((const uint16_t*)nxt, E * c_in, (uint16_t*)nxt, stream) : dgnn_relu((const float*)nxt, E * c_in, (float*)nxt, stream);
        }
        if (rc != DGNN_OK) return rc;
        xin = y;
        ldxin = c_out;
        ea = nxt;
        ld_ea = c_in;
    }
    if (fused_layers) *fused_layers = fused;
    if (W1) DGNN_TRY(dgnn_updated_tail_fwd(n, xin, ldxin, widths[n_layers], W1, b1, hdim, W3, b3, n_out, h, (float*)out, bf16, gemm_mode, stream));
    return dgnn_check_launch(who);
}
