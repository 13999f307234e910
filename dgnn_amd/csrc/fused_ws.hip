// Wave-specialised fused conv layer, C_in in {64, 128} -> 128 (round 5; VERDICT r4 item 3, DESIGN 10 "next" of round 4).
//
// Reference: SAGEConv.forward + BatchNorm(eval) + ReLU, learning/surfaceNetStaticEdgeFilters.py:66-96, :345-346 -- the shipped model's layers 1, 2 and 3
// (the description below is for C_in = 128; 64: half the channels per producer lane, 512-byte ring rows, 4 k-steps).
// k_sage_fused_mfma<128,128> runs eight wavefronts that ALL walk the same two phases (filter / mean, barrier, dense product): 44-48 % of its wave cycles
// are parked, the matrix pipe is 26 % busy, and at 229-250 VGPRs two wavefronts per SIMD is all it admits (docs/history_r1-r4.md 5a, 5b).  A probe of
// round 5 says what the split buys: the producer side ALONE (gathers, filter product, mean, row split -- k_agg_sr<8, false> with its HBM
// stores off) runs 1M cells in 0.31-0.34 ms at 4 resp. 2 wavefronts per SIMD: it is bound by its reads, not by latency, once nothing else shares its
// wavefronts.  So here a 1024-thread workgroup (16 wavefronts, 4 per SIMD, <= 128 VGPRs each) is
//   8 PRODUCERS  one group of 4 cells each per 32-cell tile: index chain two tiles ahead, 4 neighbour rows + own row as 16-byte loads, filter product on
//                v_mfma_f32_16x16x32_f16 (per-edge power-of-two scales; the 62 real terms of the two-part form packed into TWO products, filter_pack.h --
//                as three products of 21 real K-slots in 32 a third of the producers' matrix instructions multiplied zeros: 128 -> 128 0.405 -> 0.390 ms,
//                profiles/filter_two_products.md), in-lane 4-term mean, the [a | x_i] row scaled by one power of two,
//                split (hi, lo) and parked in an LDS ring slot (1 KB per cell, XOR-swizzled 16-byte pieces, conflict-free for both sides);
//   8 CONSUMERS  16 output channels each, their [Wj | Wi] rows resident as fp16 (hi, lo) fragments (64 VGPRs): D[channel][cell] on v_mfma_f32_16x16x32_f16
//                with the weights as the A operand, 48 products per tile; epilogue per lane = one cell x 4 consecutive channels: inverse scales,
//                bias / BatchNorm / ReLU, one 16-byte non-temporal store;
//   The ring's swizzle and its addresses (profiles/r09_ws_loop.md): piece q of a row sits at piece q ^ (row & 15).  A consumer's 32 reads per tile come from
//   FOUR bases (the key meets only the bits of s & 3 and tq of a piece index 4 s + tq) plus immediate offsets.  Rows at a padded stride (8 CIN + 16 bytes,
//   natural piece order) were measured instead: a ds_read_b128 is served in four NON-contiguous groups of 16 lanes ({0-3, 12-15, 20-27}, ...), lanes of
//   two tq share a group, and SQ_LDS_BANK_CONFLICT went from 0 to 4 cycles on every read -- the swizzle stays.
//   The ring slots are handed over by LDS counters, no barrier in the loop: `ready[slot]` +1 per producer that has parked its rows of a tile, `done[slot]` +1
//   per consumer that has read them; every wavefront runs at its own pace, a producer only waits when the slot it is about to write (two tiles back) has
//   not been drained.  EVERY adder waits for the slot first, the producer groups past the end of the graph included -- a count that lands early can stand
//   in for a late wavefront's (that race, and the same one in the decoder's counters, are pinned by tests/test_gpu_infer.py::
//   test_ignatius_layers_repeat_bit_for_bit_with_cold_caches and tests/test_gpu_parity.py::test_last_layer_and_decoder_in_one_launch).  No K split, no
//   partial-sum exchange, no resident weights in the gathering wavefronts.
// Where the time goes (a build with s_memtime around the polls, profiles/r05_ws_phases.md): the producers bound the plain launch (they wait 8-12 % of their
// time, the consumers 35-45 %); a consumer's 48 products take ~2 us of a 3.3 us tile because the two consumers of a SIMD start together and share its
// matrix pipe with two producers.
// Arithmetic: the fp16 two-part form (fused_common.h): scaling groups per cell row [a | x_i], per edge, per [We | be], per consumer (its 16 weight rows).
// A cell's result depends on its own inputs only: destination sub-ranges, ring parts and differently tiled runs agree bit for bit.  Groups of any
// in-degree other than 4 take a per-lane fp32 path (never on Delaunay scenes).
#include <stdlib.h>

#include "common.h"
#include "filter_pack.h"
#include "fused_common.h"

namespace {
using namespace fused;

typedef float f32x4_t __attribute__((ext_vector_type(4)));
#define H8(v) __builtin_bit_cast(f16x8, v)

constexpr int WS_C = 128;                    // channels out (and in: CIN = 128, the shipped model's layers 2 and 3; CIN = 64: its layer 1)
constexpr int WS_TILE = 32;                  // cells per tile
constexpr int WS_NP = 8;                     // producer wavefronts (the other 8 of the 16 are consumers)
// per input width CIN: ring bytes per cell = [hi of a | hi of x | lo of a | lo of x], CIN fp16 each (1 KB / 512 B); a ring slot = 32 cells (32 / 16 KB);
// the filter operand [cb < CIN / 16][M2 | M1][64 lanes] x 16 B (filter_pack.h)
template <int CIN> struct WsC {
    static constexpr int NCH = CIN / 16;        // channels of a cell's rows per producer lane (8 / 4)
    static constexpr int NV = NCH / 4;          // ... as 16-byte loads
    static constexpr int KH = CIN / 32;         // k-steps of the dense product per half (a | x_i)
    static constexpr int PP = CIN / 8;          // 16-byte pieces per quarter of a ring row
    static constexpr int ROWB = 8 * CIN;
    static constexpr int SLOT = WS_TILE * ROWB;
    static constexpr int BP = NCH * 2 * 64 * 16;
};
// RING slots of the hand-off (counters, below): 2 for the 128-wide rows, 4 for the 64-wide 16-bit rows.
template <int CIN, int RING> struct WsL {
    static constexpr int OFF_BP = RING * WsC<CIN>::SLOT;
    static constexpr int OFF_ROWF = OFF_BP + WsC<CIN>::BP;          // [RING][32] inverse row scales
    static constexpr int OFF_CST = OFF_ROWF + RING * WS_TILE * 4;   // bias | scale | shift [128]
    static constexpr int OFF_SC = OFF_CST + 3 * WS_C * 4;           // max |We|, |be|; then ready[RING], done[RING], ycnt[2], yfree[2], lcnt[2], ccnt[2]
    static constexpr int OFF_DC = OFF_SC + 16 + 2 * RING * 4 + 16 + 16;   // decoder constants: A1 | B1 [64], W3 [2][64], b3 [2] (+2 pad)
    static constexpr int OFF_PLOG = OFF_DC + (64 + 64 + 128 + 4) * 4;     // partial logits [2 tiles][4 hidden blocks][32 cells][2]
    static constexpr int OFF_YS = OFF_PLOG + 2 * 4 * 32 * 8;              // inverse scales of the parked tiles [2 tiles][32 cells]
    static constexpr int OFF_CMAX = OFF_YS + 2 * 32 * 4;                  // largest exponent of a cell's 128 channels, tagged [4 tiles][32 cells]
    static constexpr int OFF_W0S = OFF_CMAX + 4 * 32 * 4;                 // W0's scaling groups: max |W0| [4 hidden blocks], inverse scale [4]
    static constexpr int OFF_W0 = (OFF_W0S + 32 + 255) & ~255;            // W0 as A-operand fragments [4 hidden blocks][4 k-steps][hi | lo][64 lanes] x 16 B
    static constexpr int OFF_YT = OFF_W0 + 4 * 4 * 2 * 64 * 16;           // the layer's finished tile as B-operand fragments [2 tiles][4 k-steps][2 blocks][hi | lo][64 lanes] x 16 B
    static constexpr int SMEM = OFF_SC + 16 + 2 * RING * 4 + 16 + 16;
    static constexpr int SMEM_DEC = OFF_YT + 2 * 4 * 2 * 2 * 64 * 16;
    static_assert(SMEM_DEC <= 160 * 1024, "the LDS of one CU");
};

// the decoder behind the last conv layer (reference learning/surfaceNetStaticEdgeFilters.py:180-187, applied at :350-351): Linear(128 -> 64) - BatchNorm(eval) -
// ReLU - Linear(64 -> 2).  In the DEC instantiation the consumers do not store the layer's rows.  Four stages, each one tile behind the one before it, so
// that no wavefront ever waits for data another one has only just produced (the first form of this kernel exchanged fp32 partial hidden rows of the SAME
// tile -- three lock-step meetings of the eight consumers per tile, 1.1 us of a tile's 4.4):
//   A1(t)   consumer s keeps its 16 finished channels of the 32 cells in registers (yv, 8 VGPRs, alive for one iteration) and folds the largest exponent of
//           each cell's 16 channels into cmax[t & 3][cell]: one LDS atomic unsigned max per lane and row block on the word (t / 4 + 1) << 8 | exponent.  The
//           maximum does not depend on the order the eight consumers arrive in, the tag in the upper bits makes a tile's word beat whatever the buffer's
//           previous tile left there (no clearing), and pow2_scales reads nothing but the exponent; then ccnt[t & 1] += 1;
//   A2(t-1) waits for ccnt at 8 per tile, takes ONE power-of-two scale per cell from the word's low byte (the cell's 128 channels: every consumer derives
//           the same scale), scales and splits (hi, lo) its yv and parks them as its share of the B operands of v_mfma_f32_16x16x32_f16: a k-step is 32
//           channels = the slices of consumers 2 ks and 2 ks + 1, a fragment lane (cell n, group g) holds channels 32 ks + 8 g .. + 7, so consumer s, lane
//           (n, tq) writes the 8 bytes [4 (tq & 1) .. + 3] of lane (n, g = 2 (s & 1) + (tq >> 1)) of k-step s >> 1, hi and lo fragments apart; consumer 0
//           writes the cell's inverse scale (ysc); then ycnt[t & 1] += 1;
//   B(t-2)  job (hb, b) of 8: hidden units 16 hb .. + 15 of cells 16 b .. + 15 = 4 k-steps x 3 products (lo.hi, hi.lo, hi.hi: small terms first, as in
//           the consumers' loop) against W0's fragments (LDS, laid out once per workgroup, one power-of-two scale per hidden block), all twelve in ONE
//           accumulator, scaled back once by the cell's and the hidden block's inverse scales; BatchNorm / ReLU / W3 over the lane's 4 units, the 4
//           lanes of a cell added in one order: partial logits per cell and hidden block.  A tile's 8 jobs go to the 8 wavefronts of ONE role (see
//           b_on_consumers): the producers, between issuing a tile's gathers and using them;
//   C(t-3)  consumer 0 adds the four partial logits of a cell in one order and stores 8 bytes per cell.
// Every sum has one order and touches one cell's values only (sub-ranges and ring parts give the same bits).
// Why cmax has FOUR buffers and needs no wait: a consumer writes cmax[t & 3] for tile t + 4 only after its own A2(t + 2), which waited for all eight A1(t + 2);
// a consumer that has run A1(t + 2) (iteration t + 3) has finished iteration t + 2 and with it A2(t), the last read of tile t's words.  With two buffers a
// consumer one iteration ahead of the slowest (the ring allows that) could overwrite a word the slowest has not read yet.  The same argument shows that
// every A1(t + 2) count lands in ccnt[t & 1] after that counter reached its target for tile t (the adder itself waited for it in A2(t)).
// LDS banks: stage B reads every fragment as 64 lanes x 16 contiguous bytes (ds_read_b128: four groups of 16 lanes, each group's 64 dwords on 64 different
// banks): conflict-free.  A2's 8-byte stores (16 lanes of one tq: the same half of 16 neighbouring 16-byte pieces) are 2-way, four stores per tile.
struct WsDec {
    const float* W0;      // [64, 128]
    const float* b0;      // [64]
    const float* scale1;  // [64] folded BatchNorm of the decoder, or NULL
    const float* shift1;
    const float* W3;      // [2, 64]
    const float* b3;      // [2]
    float* logits;        // [n_dst, 2]
};


__device__ __forceinline__ void st_nt16(float* p, f32x4_t v) { __builtin_nontemporal_store(v, reinterpret_cast<f32x4_t*>(p)); }
// IO16: the rows in HBM are the UNSIGNED 16-bit rows of the bf16-storage chain (fused_bf16.hip "UB": value = bits << 15 -- 8 exponent and 8 explicit
// mantissa bits of a value that is never negative, written behind a ReLU; round to nearest even on bit 15 of the fp32 pattern)
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float ub16_lo(uint32_t u) { return __builtin_fabsf(__builtin_bit_cast(float, u << 15)); }
__device__ __forceinline__ float ub16_hi(uint32_t u) { return __builtin_bit_cast(float, (u >> 16) << 15); }
__device__ __forceinline__ uint32_t ub16_enc(float v) {
    const uint32_t b = __builtin_bit_cast(uint32_t, v) & 0x7FFFFFFFu;
    return (b + 0x3FFFu + ((b >> 15) & 1u)) >> 15;
}
__device__ __forceinline__ uint32_t bits(float f) { return __builtin_bit_cast(uint32_t, f); }

// knobs (a launch argument, though every launch passes WS_KNOBS: with the value folded into the kernel the compiler schedules the loop differently and the
// layers ran 4-5 % slower): bit 0 = non-temporal row stores, bits 4-5 = who runs the decoder's stage B (see b_on_consumers)
constexpr int WS_KNOBS = 1 | (0 << 4);
template <int CIN, int RING, bool DEC, bool IO16 = false, bool LDC = false>
__global__ void __launch_bounds__(1024) k_sage_fused_ws(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ src, const int32_t* __restrict__ eid,
                                                        int64_t n_dst, const float* __restrict__ x, const float* __restrict__ xdst, int64_t ldx_arg,
                                                        const float* __restrict__ ea, int64_t lde, const float* __restrict__ We, const float* __restrict__ be,
                                                        const float* __restrict__ Wj, const float* __restrict__ bj, const float* __restrict__ Wi,
                                                        const float* __restrict__ scale, const float* __restrict__ shift, int relu, float* __restrict__ out,
                                                        int64_t ldo, int64_t ntiles, int knobs, WsDec dec) {
    static_assert(CIN == 128 || (CIN == 64 && !DEC), "input widths of the shipped model's 128-wide layers");
    static_assert(!IO16 || !DEC, "the decoder-carrying launch of the bf16-storage chain stays with fused_bf16.hip");
    // LDC: the input rows are dense (ldx == CIN, the previous fused layer's output: layers 1-3 of the shipped chain) -- a row's offset is a shift, not the
    // quarter-rate 64-bit multiply by a run-time stride (15 per tile and producer).  Any other stride runs the LDC = false instantiation.
    const int64_t ldx = LDC ? (int64_t)CIN : ldx_arg;
    // IO16: x / xdst / out are uint16_t rows (ldx / ldo in elements of that type)
    const uint16_t* const x16 = reinterpret_cast<const uint16_t*>(x);
    const uint16_t* const xdst16 = reinterpret_cast<const uint16_t*>(xdst);
    uint16_t* const out16 = reinterpret_cast<uint16_t*>(out);
    typedef WsC<CIN> G;
    constexpr int NCH = G::NCH, NV = G::NV, KH = G::KH, PP = G::PP;
    extern __shared__ __attribute__((aligned(16))) char ws_smem[];
    const bool nt_store = (knobs & 1) != 0;
    typedef WsL<CIN, RING> L;
    char* const ring = ws_smem;
    char* const bpbuf = ws_smem + L::OFF_BP;
    float* const rowf = reinterpret_cast<float*>(ws_smem + L::OFF_ROWF);
    float* const cst = reinterpret_cast<float*>(ws_smem + L::OFF_CST);
    uint32_t* const scbuf = reinterpret_cast<uint32_t*>(ws_smem + L::OFF_SC);
    volatile uint32_t* const ready = reinterpret_cast<volatile uint32_t*>(ws_smem + L::OFF_SC + 16);
    volatile uint32_t* const done = ready + RING;
    // DEC: one counter per buffer (tile parity), like ready / done per ring slot.  A single running counter is NOT enough: a fast consumer's count for the
    // next tile can stand in for a slow consumer's count of this one wherever nothing else holds the fast one back (the first tiles, the drain)
    volatile uint32_t* const ycnt = done + RING;          // [2] +1 per consumer whose 16 channels of a finished tile are parked (stage A2)
    volatile uint32_t* const yfree = ycnt + 2;            // [2] +1 per wavefront that has read a parked tile (stage B)
    volatile uint32_t* const lcnt = ycnt + 4;             // [2] +1 per wavefront whose partial logits of a tile are parked (stage B)
    volatile uint32_t* const ccnt = ycnt + 6;             // [2] +1 per consumer whose exponents of a finished tile are in cmax (stage A1)
    float* const dcst = reinterpret_cast<float*>(ws_smem + L::OFF_DC);
    float* const plog = reinterpret_cast<float*>(ws_smem + L::OFF_PLOG);
    float* const ysc = reinterpret_cast<float*>(ws_smem + L::OFF_YS);
    uint32_t* const cmax = reinterpret_cast<uint32_t*>(ws_smem + L::OFF_CMAX);
    uint32_t* const w0max = reinterpret_cast<uint32_t*>(ws_smem + L::OFF_W0S);
    float* const w0inv = reinterpret_cast<float*>(ws_smem + L::OFF_W0S + 16);
    char* const w0buf = ws_smem + L::OFF_W0;
    char* const ytile = ws_smem + L::OFF_YT;
    // wait until *ctr >= target (LDS word, wave-uniform): a short sleep between polls keeps the LDS and the issue slots for the working wavefronts
    // The compiler barriers matter: the poll is a volatile load, which orders nothing against the ORDINARY LDS loads behind it -- without the second one
    // the compiler hoisted the consumer's read of a tile's row scales above the poll (a stale scale for one producer's four cells, once in thousands of
    // tiles: caught by tests/test_gpu_parity.py::test_fused_layers_row_level_on_larger_graph) -- nor the ordinary stores in front of it.
    typedef __attribute__((address_space(3))) volatile uint32_t lds_vu32;
    auto wait_for = [&](volatile uint32_t* ctr, uint32_t target) {
        asm volatile("" ::: "memory");
        // (the poll through an LDS-space pointer = ds_read_b32: the generic pointer compiled to a flat load, whose s_waitcnt vmcnt(0) also drained the
        // wavefront's gathers in flight)
        lds_vu32* c3 = (lds_vu32*)ctr;
        while ((int32_t)(__builtin_amdgcn_readfirstlane((int)*c3) - (int)target) < 0) __builtin_amdgcn_s_sleep(1);
        asm volatile("" ::: "memory");
    };
    const int lane = lane_id(), w = wave_id_uniform();
    const int jcol = lane & 15, tq = lane >> 4;

    // tiles of this workgroup: XCD b % 8 walks one contiguous eighth of the cells (gathered neighbour rows stay in that XCD's L2)
    const int nwg = gridDim.x, xcd = blockIdx.x & 7, slot_ = blockIdx.x >> 3, wg_per_xcd = (nwg + 7 - xcd) >> 3;
    const int64_t per = (ntiles + 7) / 8, t_lo = xcd * per, t_hi = min(ntiles, t_lo + per);
    int64_t my_n = 0;
    if (t_lo + slot_ < t_hi) my_n = (t_hi - t_lo - slot_ + wg_per_xcd - 1) / wg_per_xcd;
    auto tile_of = [&](int64_t it) { return t_lo + slot_ + it * wg_per_xcd; };

    // ---- prologue: power-of-two scale of [We | be], the split filter operand in LDS, the epilogue's per-channel constants
    if (threadIdx.x == 0) scbuf[0] = 0u;
    if (threadIdx.x < 2 * RING + 8) ready[threadIdx.x] = 0u;
    if constexpr (DEC) {
        for (int n_ = threadIdx.x; n_ < 64; n_ += blockDim.x) {
            const float s1 = dec.scale1 ? dec.scale1[n_] : 1.f, h1 = dec.scale1 ? dec.shift1[n_] : 0.f;
            dcst[n_] = s1;                                   // h = relu(sum * A1 + B1)
            dcst[64 + n_] = __fmaf_rn(dec.b0[n_], s1, h1);
            dcst[128 + n_] = dec.W3[n_];
            dcst[192 + n_] = dec.W3[64 + n_];
        }
        if (threadIdx.x < 2) dcst[256 + threadIdx.x] = dec.b3[threadIdx.x];
        if (threadIdx.x < 4 * WS_TILE) cmax[threadIdx.x] = 0u;      // tag 0: below every tile's word
        if (threadIdx.x < 4) w0max[threadIdx.x] = 0u;
    }
    __syncthreads();
    if constexpr (DEC) {
        // W0's scaling groups: the 16 rows of a hidden block (what one accumulator of stage B covers)
#pragma unroll
        for (int hb = 0; hb < 4; ++hb) {
            uint32_t m0 = 0u;
            for (int e = threadIdx.x; e < 16 * WS_C; e += blockDim.x) m0 = umax(m0, absbits(dec.W0[hb * 16 * WS_C + e]));
            m0 = wave_umax(m0);
            if ((threadIdx.x & 63) == 0) atomicMax(&w0max[hb], m0);
        }
    }
    {
        uint32_t me = 0u;
        for (int e = threadIdx.x; e < CIN * FE; e += blockDim.x) me = umax(me, absbits(We[e]));
        for (int e = threadIdx.x; e < CIN; e += blockDim.x) me = umax(me, absbits(be[e]));
        me = wave_umax(me);
        if (lane == 0) atomicMax(&scbuf[0], me);
    }
    for (int c = threadIdx.x; c < WS_C; c += blockDim.x) {
        cst[c] = bj ? bj[c] : 0.f;
        cst[WS_C + c] = scale ? scale[c] : 1.f;
        cst[2 * WS_C + c] = scale ? shift[c] : 0.f;
    }
    __syncthreads();
    float sWe, inv_sWe;
    pow2_scales(scbuf[0], sWe, inv_sWe);
    // Which channels lane j of a cell's 16 lanes owns.  fp32 rows of 128 channels (two 16-byte loads per lane and row): channels 4 j .. 4 j + 3 and
    // 64 + 4 j .. + 3, so that ONE load instruction covers whole 128-byte lines (16 lanes x 16 bytes = lines 0-1, then lines 2-3).  With 8 contiguous channels
    // per lane (round 5) both instructions touched all four lines of a row, half of each: twice the tag look-ups in the vector L1, the second one a hit on
    // a line still in flight.  Same bits (a channel's arithmetic does not depend on which lane owns it); measured on one box (profiles/r06_l1_probe.md):
    // 128 -> 128 0.408 -> 0.406 ms, last layer + decoder 0.500 -> 0.490 ms.
    constexpr bool LINE_OWN = !IO16 && NV == 2;
    auto chan = [](int j, int cb) { return LINE_OWN ? ((cb >> 2) * 64 + 4 * j + (cb & 3)) : NCH * j + cb; };
    // The B fragments of the two filter products (filter_pack.h): entry (cb, j) lays out channel c = chan(j, cb) for both products and all four lane
    // groups -- the 11 words (k = 2 i, 2 i + 1; the bias at k = 20, then 0) of [We | be] . sWe split once, each slot's word picked by the map
    for (int e = threadIdx.x; e < NCH * 16; e += blockDim.x) {
        const int cb = e >> 4, j = e & 15;
        const int c = chan(j, cb);
        uint32_t wh[11], wl[11];
#pragma unroll
        for (int i = 0; i < 10; ++i) split2h(We[(int64_t)c * FE + 2 * i] * sWe, We[(int64_t)c * FE + 2 * i + 1] * sWe, wh[i], wl[i]);
        split2h(be[c] * sWe, 0.f, wh[10], wl[10]);
#pragma unroll
        for (int m = 0; m < 2; ++m) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                uint32_t wd[4];
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const filter_pack::Slot t = filter_pack::MAP[m][g][2 * d];
                    wd[d] = t.k < 0 ? 0u : (t.b == filter_pack::HI ? wh[t.k >> 1] : wl[t.k >> 1]);
                }
                *reinterpret_cast<uint4*>(bpbuf + (((cb * 2 + m) * 64 + g * 16 + j) << 4)) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
            }
        }
    }

    // DEC, stage B of tile t, job (hb, b) (either role runs it, see above): hidden units 16 hb .. + 15 of cells 16 b .. + 15 -- lane (cell n = jcol, tq) ends up with
    // units 16 hb + 4 tq .. + 3
    auto stage_b = [&](uint32_t t, int hb, int b) {
        wait_for(ycnt + (t & 1), 8u * (t / 2 + 1));
        int ln = lane;
        asm volatile("" : "+v"(ln));                            // (addresses recomputed per tile, see `key` below)
        const char* yt = ytile + ((t & 1) << 14) + ((b * 128 + ln) << 4);       // [k-step: 4 KB][row block: 2 KB][hi | lo: 1 KB]
        const char* wp = w0buf + ((hb * 512 + ln) << 4);                        // [hidden block: 8 KB][k-step: 2 KB][hi | lo: 1 KB]
        const float inv = ysc[(t & 1) * WS_TILE + 16 * b + (ln & 15)] * w0inv[hb];
        f32x4_t hs = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const f16x8 w0h = H8(*reinterpret_cast<const uint4*>(wp + (s << 11))), w0l = H8(*reinterpret_cast<const uint4*>(wp + (s << 11) + 1024));
            const f16x8 yh = H8(*reinterpret_cast<const uint4*>(yt + (s << 12))), yl = H8(*reinterpret_cast<const uint4*>(yt + (s << 12) + 1024));
            hs = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0l, yh, hs, 0, 0, 0);     // small terms first
            hs = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0h, yl, hs, 0, 0, 0);
            hs = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0h, yh, hs, 0, 0, 0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane == 0) atomicAdd(const_cast<uint32_t*>(yfree + (t & 1)), 1u);
#pragma unroll
        for (int i = 0; i < 4; ++i) hs[i] *= inv;                // one scale per cell and hidden block, powers of two: exact
        const int u0 = 16 * hb + 4 * (ln >> 4);
        float l0 = 0.f, l1 = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float hv = fmaxf(__fmaf_rn(hs[i], dcst[u0 + i], dcst[64 + u0 + i]), 0.f);
            l0 = __fmaf_rn(hv, dcst[128 + u0 + i], l0);
            l1 = __fmaf_rn(hv, dcst[192 + u0 + i], l1);
        }
        // the cell's 4 lanes (16 apart): (q0 + q1) + (q2 + q3) in every one of them, on the row-swap instructions (no LDS round trips)
        l0 = cross_row_sum(l0);
        l1 = cross_row_sum(l1);
        if (ln < 16) *reinterpret_cast<float2*>(plog + (((t & 1) * 4 + hb) * WS_TILE + 16 * b + ln) * 2) = make_float2(l0, l1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane == 0) atomicAdd(const_cast<uint32_t*>(lcnt + (t & 1)), 1u);
    };

    // who runs stage B of tile t: every wavefront of one role takes one of the tile's 8 jobs.  (knobs bits 4-5: 0 = producers always, 1 = consumers on even
    // tiles, 2 = consumers on three tiles of four, 3 = consumers always.  With the K = 16 products and a scale per slice, 2 was the best; with half the
    // products, one scale per cell and the consumers carrying A1 / A2, the job is cheapest between a producer's gathers and their use: 0 -- measured
    // 0.472 / 0.495 / 0.510 / 0.524 ms for 0 / 1 / 2 / 3, profiles/r08_dec_cellscale.md)
    const int bsel = (knobs >> 4) & 3;
    auto b_on_consumers = [&](uint32_t t) { return bsel == 0 ? false : bsel == 1 ? (t & 1) == 0 : bsel == 2 ? (t & 3) != 3 : true; };

    if (w >= WS_NP) {
        // =================================================================== CONSUMER: channels [16 cw, 16 cw + 16)
        const int cw = w - WS_NP;
        // resident weights: lane (m = jcol: channel 16 cw + m, g = tq) holds K index 32 s + 8 g + i of k-step s: s < KH -> Wj (the mean half), else Wi
        const int col = 16 * cw + jcol;
        uint32_t mw = 0u;
#pragma unroll
        for (int s = 0; s < 2 * KH; ++s) {
            const float* wr = (s < KH ? Wj : Wi) + (int64_t)col * CIN + 32 * (s % KH) + 8 * tq;
            const f32x4_t r0 = *reinterpret_cast<const f32x4_t*>(wr), r1 = *reinterpret_cast<const f32x4_t*>(wr + 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) mw = umax(mw, umax(absbits(r0[i]), absbits(r1[i])));
        }
        float sW, inv_sW;
        pow2_scales(wave_umax(mw), sW, inv_sW);     // one scale per consumer (its 16 weight rows)
        f16x8 wh[2 * KH], wl[2 * KH];
#pragma unroll
        for (int s = 0; s < 2 * KH; ++s) {
            const float* wr = (s < KH ? Wj : Wi) + (int64_t)col * CIN + 32 * (s % KH) + 8 * tq;
            const f32x4_t r0 = *reinterpret_cast<const f32x4_t*>(wr), r1 = *reinterpret_cast<const f32x4_t*>(wr + 4);
            uint32_t ph[4], pl[4];
            split2h(r0[0] * sW, r0[1] * sW, ph[0], pl[0]);
            split2h(r0[2] * sW, r0[3] * sW, ph[1], pl[1]);
            split2h(r1[0] * sW, r1[1] * sW, ph[2], pl[2]);
            split2h(r1[2] * sW, r1[3] * sW, ph[3], pl[3]);
            wh[s] = pack8h(ph);
            wl[s] = pack8h(pl);
        }
        // DEC: W0 as A-operand fragments of v_mfma_f32_16x16x32_f16, for everybody: lane (m = jcol, g = tq) of hidden block hb and k-step ks holds hidden
        // unit 16 hb + m, channels 32 ks + 8 g .. + 7, hi and lo fragments apart.  This consumer lays out k-step cw >> 1 of hidden blocks 2 (cw & 1), + 1.
        if constexpr (DEC) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int hb = 2 * (cw & 1) + u, ks = cw >> 1;
                float sW0, inv_sW0;
                pow2_scales(w0max[hb], sW0, inv_sW0);
                if (ks == 0 && lane == 0) w0inv[hb] = inv_sW0;
                const float* wr = dec.W0 + (int64_t)(16 * hb + jcol) * WS_C + 32 * ks + 8 * tq;
                const f32x4_t r0 = *reinterpret_cast<const f32x4_t*>(wr), r1 = *reinterpret_cast<const f32x4_t*>(wr + 4);
                uint32_t ph[4], pl[4];
                split2h(r0[0] * sW0, r0[1] * sW0, ph[0], pl[0]);
                split2h(r0[2] * sW0, r0[3] * sW0, ph[1], pl[1]);
                split2h(r1[0] * sW0, r1[1] * sW0, ph[2], pl[2]);
                split2h(r1[2] * sW0, r1[3] * sW0, ph[3], pl[3]);
                uint4* dst = reinterpret_cast<uint4*>(w0buf + (((hb * 4 + ks) * 128 + lane) << 4));
                dst[0] = make_uint4(ph[0], ph[1], ph[2], ph[3]);
                dst[64] = make_uint4(pl[0], pl[1], pl[2], pl[3]);
            }
        }
        __syncthreads();   // (the producers' prologue barrier)
        const int c0 = 16 * cw + 4 * tq;          // this lane's 4 consecutive output channels
        const int64_t n_it = my_n + (DEC ? 3 : 0);       // DEC: stage A2 runs one tile behind the product, stage B two, stage C three
        f32x4_t yp[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, yn[2] = {yp[0], yp[1]};     // DEC: the previous tile's finished channels, between A1 and A2
        for (int64_t it = 1; it <= n_it; ++it) {
            if constexpr (DEC) {
                // C(it - 4): consumer 0 adds the four partial logits of a cell in one order and stores them.  (First in the iteration: the others' B(it - 2)
                // -- next iteration -- reuses this buffer, and they get there only behind this wavefront's A2(it - 2) below.)
                if (cw == 0 && it >= 4) {
                    const uint32_t t = (uint32_t)(it - 4);
                    wait_for(lcnt + (t & 1), 8u * (t / 2 + 1));
                    if (lane < WS_TILE) {
                        float s0 = dcst[256], s1 = dcst[257];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const float* pq = plog + (((t & 1) * 4 + q) * WS_TILE + lane) * 2;
                            s0 += pq[0];
                            s1 += pq[1];
                        }
                        const int64_t cell = tile_of(t) * WS_TILE + lane;
                        if (cell < n_dst) *reinterpret_cast<float2*>(dec.logits + cell * 2) = make_float2(s0, s1);
                    }
                }
            }
            if (it >= 1 && it <= my_n) {
                const int sl = (int)((it - 1) % RING);
                wait_for(ready + sl, (uint32_t)(WS_NP * ((it - 1) / RING + 1)));
                f32x4_t acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
                // Ring-read addresses: FOUR bases per tile, everything else in the reads' immediate offsets.  The swizzle (piece ^ jcol for the rows jcol and
                // 16 + jcol this lane reads) touches the low four bits of a piece index only, and of 4 s + tq only s & 3 and tq live there: piece =
                // ((4 (s & 3) + tq) ^ jcol) + 16 (s >> 2) = (4 (s & 3) ^ key) + 16 (s >> 2) with key = jcol ^ tq; the lo quarters (+ 2 PP pieces) and the second
                // row block (+ 16 rows) are constants on top.  base[m] = row + (((4 m) ^ key) << 4) serves the eight reads of k-steps m, m + 4: nine integer
                // instructions per tile instead of two per read (41), the same addresses.
                // (the key passes through an empty asm every tile: left alone, the compiler keeps all 32 loop-invariant read addresses in registers -- 19
                // spilled in the decoder-carrying instantiation; the bases pass through one so that the reads stay base + immediate)
                int key = jcol ^ tq;
                asm volatile("" : "+v"(key));
                uint32_t rbase[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    rbase[m] = (uint32_t)(sl * G::SLOT + jcol * G::ROWB) + (uint32_t)(((4 * m) ^ key) << 4);
                    asm volatile("" : "+v"(rbase[m]));
                }
                // ring reads one whole k-step ahead of the products (two register sets).  The scheduling barrier pins that order: left alone, the compiler
                // sinks every read to just in front of its first use and waits for it on the spot -- sixteen exposed LDS round trips per tile.  (Two steps
                // ahead = three sets: over the 128-register budget, spills inside the loop, twice the time.)
                f16x8 xh[2][2], xl[2][2];
                auto ld_step = [&](int s, int set) {
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        const char* rp = ring + rbase[s & 3] + (16 * b * G::ROWB + ((s >> 2) << 8));
                        xh[set][b] = H8(*reinterpret_cast<const uint4*>(rp));
                        xl[set][b] = H8(*reinterpret_cast<const uint4*>(rp + 2 * PP * 16));
                    }
                };
                ld_step(0, 0);
#pragma unroll
                for (int s = 0; s < 2 * KH; ++s) {
                    const int set = s & 1;
                    if (s + 1 < 2 * KH) ld_step(s + 1, set ^ 1);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int b = 0; b < 2; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[s], xh[set][b], acc[b], 0, 0, 0);     // small terms first
#pragma unroll
                    for (int b = 0; b < 2; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[s], xl[set][b], acc[b], 0, 0, 0);
#pragma unroll
                    for (int b = 0; b < 2; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[s], xh[set][b], acc[b], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
                float invr[2];
#pragma unroll
                for (int b = 0; b < 2; ++b) invr[b] = rowf[sl * WS_TILE + 16 * b + jcol] * inv_sW;
                // every read of the slot has returned: hand it back
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (lane == 0) atomicAdd(const_cast<uint32_t*>(done + sl), 1u);
                // (the per-channel constants are re-read from LDS every tile: 12 registers the decoder stage needs)
                const f32x4_t bb = *reinterpret_cast<const f32x4_t*>(cst + c0), sc = *reinterpret_cast<const f32x4_t*>(cst + WS_C + c0),
                              sh = *reinterpret_cast<const f32x4_t*>(cst + 2 * WS_C + c0);
                f32x4_t yv[2];
#pragma unroll
                for (int b = 0; b < 2; ++b) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float t_ = __fmaf_rn(acc[b][i], invr[b], bb[i]);
                        t_ = __fmaf_rn(t_, sc[i], sh[i]);
                        yv[b][i] = relu ? fmaxf(t_, 0.f) : t_;
                    }
                }
                if constexpr (!DEC) {
                    const int64_t cell0 = tile_of(it - 1) * WS_TILE;
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        const int64_t cell = cell0 + 16 * b + jcol;
                        if (cell < n_dst) {
                            if constexpr (IO16) {
                                const u32x2_t pk = {ub16_enc(yv[b][0]) | (ub16_enc(yv[b][1]) << 16), ub16_enc(yv[b][2]) | (ub16_enc(yv[b][3]) << 16)};
                                if (nt_store) __builtin_nontemporal_store(pk, reinterpret_cast<u32x2_t*>(out16 + cell * ldo + c0));
                                else *reinterpret_cast<u32x2_t*>(out16 + cell * ldo + c0) = pk;
                            } else {
                                if (nt_store) st_nt16(out + cell * ldo + c0, yv[b]);
                                else *reinterpret_cast<f32x4_t*>(out + cell * ldo + c0) = yv[b];
                            }
                        }
                    }
                } else {
                    // A1(it - 1): the largest exponent of this lane's 4 channels of each cell into the cell's word (header comment: tag, four buffers)
                    const uint32_t t = (uint32_t)(it - 1);
                    uint32_t* cm = cmax + (t & 3) * WS_TILE + jcol;
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        const float my = fmaxf(fmaxf(fabsf(yv[b][0]), fabsf(yv[b][1])), fmaxf(fabsf(yv[b][2]), fabsf(yv[b][3])));
                        atomicMax(cm + 16 * b, ((t / 4 + 1) << 8) | (bits(my) >> 23));
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    if (lane == 0) atomicAdd(const_cast<uint32_t*>(ccnt + (t & 1)), 1u);
                    yn[0] = yv[0], yn[1] = yv[1];
                }
            }
            if constexpr (DEC) {
                if (it >= 2 && it <= my_n + 1) {
                    // A2(it - 2): all eight consumers' exponents of the tile are in; the buffer's previous tile (two back) has been read by everybody.
                    // One scale per cell (an all-zero cell: exponent 0 -> a finite scale, zeros parked, inverse scale 0)
                    const uint32_t t = (uint32_t)(it - 2);
                    wait_for(ccnt + (t & 1), 8u * (t / 2 + 1));
                    wait_for(yfree + (t & 1), 8u * (t / 2));
                    int ln = lane;
                    asm volatile("" : "+v"(ln));
                    const uint32_t* cm = cmax + (t & 3) * WS_TILE + (ln & 15);
                    char* yt = ytile + ((t & 1) << 14) + ((cw >> 1) << 12) + (((ln & 15) + 16 * (2 * (cw & 1) + (ln >> 5))) << 4) + (((ln >> 4) & 1) << 3);
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        float sY, inv_sY;
                        pow2_scales((cm[16 * b] & 255u) << 23, sY, inv_sY);
                        uint32_t ph[2], pl[2];
                        split2h(yp[b][0] * sY, yp[b][1] * sY, ph[0], pl[0]);
                        split2h(yp[b][2] * sY, yp[b][3] * sY, ph[1], pl[1]);
                        *reinterpret_cast<uint2*>(yt + (b << 11)) = make_uint2(ph[0], ph[1]);
                        *reinterpret_cast<uint2*>(yt + (b << 11) + 1024) = make_uint2(pl[0], pl[1]);
                        if (cw == 0 && ln < 16) ysc[(t & 1) * WS_TILE + 16 * b + ln] = inv_sY;
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    if (lane == 0) atomicAdd(const_cast<uint32_t*>(ycnt + (t & 1)), 1u);
                }
                yp[0] = yn[0], yp[1] = yn[1];
                if (it >= 3 && it <= my_n + 2 && b_on_consumers((uint32_t)(it - 3))) stage_b((uint32_t)(it - 3), cw & 3, cw >> 2);
            }
        }
        return;
    }

    // ======================================================================= PRODUCER: group p of 4 cells of every tile
    __syncthreads();   // filter operand and constants in place
    const int p = w;
    const int P0 = NCH * jcol;                     // the lane's NCH channels (contiguous ownership)
    const int Q0 = 4 * jcol;                       // LINE_OWN: its two quads start at Q0 and 64 + Q0
    // Loop bookkeeping in 32 bits (the scalar unit compares no 64-bit values for order: `it < my_n` and the clamp of n_dst - i0 went through the vector
    // unit, three times per tile): a workgroup's tile count is far below 2^31, and the only group that can be short (nv < 4) is this producer's in the
    // graph's LAST tile, which only this workgroup's last iteration can be.
    const int n_my = (int)my_n;
    const int it_short = (n_my > 0 && tile_of(n_my - 1) == ntiles - 1) ? n_my - 1 : -1;
    const int nv_short = (int)max((int64_t)0, min((int64_t)4, n_dst - ((ntiles - 1) * WS_TILE + 4 * p)));
    auto nv_of = [&](int it) { return it == it_short ? nv_short : 4; };
    auto load_rp = [&](int it, int& vb) {
        if (it < n_my) {
            const int64_t i0 = tile_of(it) * WS_TILE + 4 * p;
            const int nv = nv_of(it);
            vb = nv > 0 ? rowptr[i0 + (lane < nv ? lane : nv)] : 0;
        }
    };
    // A regular group's indices in the lane layout that uses them: the four source ids of the lane's own cell (one 16-byte load; a group's first edge need
    // not sit on a 16-byte boundary behind ragged cells, hence the 4-byte-aligned type) and the edge id of lane jcol -- no lane exchange at the head of
    // the gather chain (these were the src / eid of edge `lane`, handed round by nine ds_bpermute_b32 per tile)
    // (not in the decoder-carrying instantiation: the three more loop-carried registers spill there -- it keeps vs[0] / veid = src / eid of edge `lane`)
    typedef int32_t i32x4a_t __attribute__((ext_vector_type(4), aligned(4)));
    constexpr bool IDX_LANE = !DEC;
    auto load_idx = [&](int it, int vb, bool& reg, int (&vs)[4], int& veid) {
        reg = false;
        if (it < n_my) {
            const int nv = nv_of(it);
            if (nv > 0) {
                const int b0 = __builtin_amdgcn_readfirstlane(vb);
                reg = __all(vb == b0 + 4 * (lane < nv ? lane : nv)) != 0;
                if (reg) {
                    if constexpr (IDX_LANE) {
                        const i32x4a_t s4 = *reinterpret_cast<const i32x4a_t*>(src + b0 + 4 * (tq < nv ? tq : nv - 1));
                        vs[0] = s4[0], vs[1] = s4[1], vs[2] = s4[2], vs[3] = s4[3];
                        const int k_e = b0 + (jcol < 4 * nv ? jcol : 4 * nv - 1);
                        veid = eid ? eid[k_e] : k_e;
                    } else {
                        const int k_me = b0 + (lane < 4 * nv ? lane : 4 * nv - 1);
                        vs[0] = src[k_me];
                        veid = eid ? eid[k_me] : k_me;
                    }
                }
            }
        }
    };
    int vb1 = 0, vb2 = 0, vs1[4] = {0, 0, 0, 0}, veid1 = 0;
    bool reg1 = false;
    load_rp(0, vb1);
    load_rp(1, vb2);
    load_idx(0, vb1, reg1, vs1, veid1);

    // DEC: on the tiles the rule gives to the producers (b_on_consumers) this wavefront also runs stage B of tile it - 3 (hidden block p & 3 of row block
    // p >> 2) -- BETWEEN issuing its gathers for tile `it` and using them: the job fills the gather latency, and its data (the consumers' stage A2 of tile
    // it - 3, behind their product of tile it - 2) is complete about when the slot the producer is going to write is handed back anyway.  Three more
    // iterations drain the last three tiles.
    for (int it = 0; it < n_my + (DEC ? 3 : 0); ++it) {
        int nv = 0, sl = 0, tl = 0, vs[4] = {0, 0, 0, 0}, veid = 0;
        bool regular = false;
        f32x4_t xo[NV], q0, q1, rr[4][NV];              // the gathered rows (DEC: in flight across stage B); read only on the path that loaded them
        uint32_t xo16[NCH / 2], rr16[4][NCH / 2];       // IO16: the same rows as packed pairs of 16-bit values, decoded where they are used
        int64_t cell = 0;
        auto own_row = [&]() {
            if constexpr (IO16) {
                const uint16_t* rp0 = xdst16 + cell * ldx + P0;
                if constexpr (NCH == 8) {
                    const uint4 u = *reinterpret_cast<const uint4*>(rp0);
                    xo16[0] = u.x, xo16[1] = u.y, xo16[2] = u.z, xo16[3] = u.w;
                } else {
                    const uint2 u = *reinterpret_cast<const uint2*>(rp0);
                    xo16[0] = u.x, xo16[1] = u.y;
                }
            } else {
                const float* rp0 = xdst + cell * ldx + (LINE_OWN ? Q0 : P0);
#pragma unroll
                for (int v = 0; v < NV; ++v) xo[v] = *reinterpret_cast<const f32x4_t*>(rp0 + (LINE_OWN ? 64 : 4) * v);
            }
        };
        auto neighbour_rows = [&]() {
            auto src_of = [&](int r) {
                if constexpr (IDX_LANE) return vs[r];
                else return __shfl(vs[0], tl * 4 + r);
            };
            auto eid_of = [&]() {
                if constexpr (IDX_LANE) return veid;
                else return __shfl(veid, jcol);
            };
            // the edge's attributes this lane's slots of the two filter products are made of (filter_pack.h): from 0 / 8 / 16 / 4 on in k-groups 0 / 1 / 2 / 3,
            // eight of them (k-group 2: four).  k-group 3 reads lines the same instruction requests for k-groups 0 and 1: no more bytes from the fabric
            const float* er = ea + (int64_t)eid_of() * lde;
            q0 = *reinterpret_cast<const f32x4_t*>(er + (tq < 3 ? 8 * tq : 4));
            q1 = *reinterpret_cast<const f32x4_t*>(er + (tq < 2 ? 8 * tq + 4 : (tq == 2 ? 4 : 8)));
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if constexpr (IO16) {
                    const uint16_t* rp = x16 + (int64_t)src_of(r) * ldx + P0;
                    if constexpr (NCH == 8) {
                        const uint4 u = *reinterpret_cast<const uint4*>(rp);
                        rr16[r][0] = u.x, rr16[r][1] = u.y, rr16[r][2] = u.z, rr16[r][3] = u.w;
                    } else {
                        const uint2 u = *reinterpret_cast<const uint2*>(rp);
                        rr16[r][0] = u.x, rr16[r][1] = u.y;
                    }
                } else {
                    const float* rp = x + (int64_t)src_of(r) * ldx + (LINE_OWN ? Q0 : P0);
#pragma unroll
                    for (int v = 0; v < NV; ++v) rr[r][v] = *reinterpret_cast<const f32x4_t*>(rp + (LINE_OWN ? 64 : 4) * v);
                }
            }
        };
        if (it < n_my) {
            const int64_t i0 = tile_of(it) * WS_TILE + 4 * p;
            sl = it % RING;
            nv = nv_of(it);
            regular = reg1;
#pragma unroll
            for (int r = 0; r < 4; ++r) vs[r] = vs1[r];
            veid = veid1;
            vb1 = vb2;
            load_idx(it + 1, vb1, reg1, vs1, veid1);
            load_rp(it + 2, vb2);
            tl = tq < nv ? tq : nv - 1;      // a short group at the end of the graph: clamped (duplicated) cells
            cell = i0 + tl;
        }
        if constexpr (DEC) {
            // (the gathers leave ahead of stage B only in this instantiation: in the plain one the loads and their use stay in ONE basic block -- split, the
            // plain launch lost 9 %: 0.412 -> 0.450 ms)
            if (it < n_my && nv > 0) {
                own_row();
                if (regular) neighbour_rows();
            }
            if (it >= 3 && !b_on_consumers((uint32_t)(it - 3))) stage_b((uint32_t)(it - 3), p & 3, p >> 2);
        }
        if (it < n_my) {
            if (nv > 0) {
                if constexpr (!DEC) own_row();
                float aout[NCH], xv[NCH];
#pragma unroll
                for (int v = 0; v < NV; ++v) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if constexpr (IO16) xv[4 * v + i] = (i & 1) ? ub16_hi(xo16[2 * v + (i >> 1)]) : ub16_lo(xo16[2 * v + (i >> 1)]);
                        else xv[4 * v + i] = xo[v][i];
                    }
                }
                if (regular) {
                    if constexpr (!DEC) neighbour_rows();
                    // The A side of the two filter products (filter_pack.h).  The lane's eight values: attributes 0 .. 7 / 8 .. 15 / 4 .. 11 in k-groups 0 / 1 / 3,
                    // [a16 a17 a18 a19 | 1 0 | a16 a17] in k-group 2.  The hi words of their split are M1's operand in every group; M2's four words are picked
                    // from the lane's own hi and lo words (five selects, nothing crosses lanes).
                    using filter_pack::HI;
                    using filter_pack::LO;
                    static_assert(filter_pack::a_word(filter_pack::M2, 0, 0, LO, 0) && filter_pack::a_word(filter_pack::M2, 0, 1, LO, 2) &&
                                      filter_pack::a_word(filter_pack::M2, 0, 2, HI, 2) && filter_pack::a_word(filter_pack::M2, 0, 3, HI, 0) &&
                                      filter_pack::a_word(filter_pack::M2, 1, 0, HI, 12) && filter_pack::a_word(filter_pack::M2, 1, 1, HI, 14) &&
                                      filter_pack::a_word(filter_pack::M2, 1, 2, LO, 12) && filter_pack::a_word(filter_pack::M2, 1, 3, LO, 14) &&
                                      filter_pack::a_word(filter_pack::M2, 2, 0, LO, 16) && filter_pack::a_word(filter_pack::M2, 2, 1, LO, 18) &&
                                      filter_pack::a_word(filter_pack::M2, 2, 2, HI, 18) && filter_pack::a_word(filter_pack::M2, 2, 3, HI, 20) &&
                                      filter_pack::a_word(filter_pack::M2, 3, 0, LO, 4) && filter_pack::a_word(filter_pack::M2, 3, 3, LO, 10) &&
                                      filter_pack::LANE_K[2][4] == FE && filter_pack::LANE_K[2][6] == 16 && filter_pack::LANE_K[3][0] == 4,
                                  "the loads and selects here follow the map");
                    float av[8];
#pragma unroll
                    for (int i = 0; i < 4; ++i) av[i] = q0[i];
                    av[4] = tq == 2 ? 1.0f : q1[0];
                    av[5] = tq == 2 ? 0.f : q1[1];
                    av[6] = tq == 2 ? q0[0] : q1[2];
                    av[7] = tq == 2 ? q0[1] : q1[3];
                    // (k-group 3 holds values the edge's other lanes hold too: the maximum over the edge's 21 values as before)
                    float mf = 0.f;
#pragma unroll
                    for (int i = 0; i < 8; i += 2) mf = fmaxf(fmaxf(mf, fabsf(av[i])), fabsf(av[i + 1]));
                    float sA, inv_sA;
                    pow2_scales(cross_row_umax(bits(mf)), sA, inv_sA);      // one scale per EDGE (a row of the operand)
                    uint32_t ph[4], pl[4];
#pragma unroll
                    for (int d = 0; d < 4; ++d) split2h(av[2 * d] * sA, av[2 * d + 1] * sA, ph[d], pl[d]);
                    float inv_e[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) inv_e[r] = __shfl(inv_sA, 4 * tq + r);
                    const uint32_t p2[4] = {tq == 1 ? ph[2] : pl[0], tq == 1 ? ph[3] : pl[1], (tq & 1) ? pl[2] : ph[1], (tq & 1) ? pl[3] : (tq == 0 ? ph[0] : ph[2])};
                    const f16x8 a1 = pack8h(ph), a2 = pack8h(p2);
#pragma unroll
                    for (int c4 = 0; c4 < NCH; c4 += 2) {
                        f16x8 b2[2], b1[2];
                        f32x4_t d[2];
#pragma unroll
                        for (int u = 0; u < 2; ++u) {
                            const char* bp = bpbuf + ((((c4 + u) * 2) * 64 + lane) << 4);
                            b2[u] = H8(*reinterpret_cast<const uint4*>(bp));
                            b1[u] = H8(*reinterpret_cast<const uint4*>(bp + 1024));
                            d[u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
                        }
#pragma unroll
                        for (int u = 0; u < 2; ++u) d[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2, b2[u], d[u], 0, 0, 0);     // small terms first
#pragma unroll
                        for (int u = 0; u < 2; ++u) d[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, b1[u], d[u], 0, 0, 0);
#pragma unroll
                        for (int u = 0; u < 2; ++u) {
                            const int c8 = c4 + u;
#pragma unroll
                            for (int r = 0; r < 4; ++r) d[u][r] *= inv_e[r];     // exact: powers of two
                            auto nb_ = [&](int r) {
                                if constexpr (IO16) return (c8 & 1) ? ub16_hi(rr16[r][c8 >> 1]) : ub16_lo(rr16[r][c8 >> 1]);
                                else return rr[r][c8 >> 2][c8 & 3];
                            };
                            float a = __fmul_rn(nb_(0), d[u][0]);
#pragma unroll
                            for (int r = 1; r < 4; ++r) a = __fmaf_rn(nb_(r), d[u][r], a);
                            aout[c8] = a * (0.25f * inv_sWe);
                        }
                    }
                } else {
                    // generic path (a group with any in-degree other than 4): plain fp32 per lane, one edge at a time (never on Delaunay scenes)
#pragma unroll
                    for (int cb = 0; cb < NCH; ++cb) aout[cb] = 0.f;
                    if (tq < nv) {
                        const int b = rowptr[cell], e_end = rowptr[cell + 1];
                        for (int k = b; k < e_end; ++k) {
                            const int s_ = src[k];
                            const float* ar = ea + (int64_t)(eid ? eid[k] : k) * lde;
#pragma unroll 1
                            for (int cb = 0; cb < NCH; ++cb) {
                                const int c = chan(jcol, cb);
                                float pf = be[c];
                                for (int f = 0; f < FE; ++f) pf = __fmaf_rn(We[(int64_t)c * FE + f], ar[f], pf);
                                const float xs_ = IO16 ? __builtin_bit_cast(float, (uint32_t)x16[(int64_t)s_ * ldx + c] << 15) : x[(int64_t)s_ * ldx + c];
                                aout[cb] = __fadd_rn(aout[cb], __fmul_rn(xs_, pf));
                            }
                        }
                        const float cnt = (float)max(e_end - b, 1);
#pragma unroll
                        for (int cb = 0; cb < NCH; ++cb) aout[cb] = __fdiv_rn(aout[cb], cnt);
                    }
                }
                // the [mean | own] row: one power-of-two scale (its 16 lanes), split, parked in the ring slot of this tile
                float ma = 0.f;
#pragma unroll
                for (int i = 0; i < NCH; i += 2) {
                    ma = fmaxf(fmaxf(ma, fabsf(aout[i])), fabsf(aout[i + 1]));
                    ma = fmaxf(fmaxf(ma, fabsf(xv[i])), fabsf(xv[i + 1]));
                }
                float s_, inv_;
                pow2_scales(row16_umax(bits(ma)), s_, inv_);
                const int T = 4 * p + tq;
                wait_for(done + sl, (uint32_t)(8 * (it / RING)));      // the slot's previous tile has been read by all 8 consumers
                if (jcol == 0) rowf[sl * WS_TILE + T] = inv_;
                uint32_t ah_[NCH / 2], al_[NCH / 2], xh_[NCH / 2], xl_[NCH / 2];
#pragma unroll
                for (int d = 0; d < NCH / 2; ++d) {
                    split2h(aout[2 * d] * s_, aout[2 * d + 1] * s_, ah_[d], al_[d]);
                    split2h(xv[2 * d] * s_, xv[2 * d + 1] * s_, xh_[d], xl_[d]);
                }
                char* rowp = ring + sl * G::SLOT + T * G::ROWB;
                const int key = T & 15;
                if constexpr (LINE_OWN) {
                    // the lane's two quads of channels = half a piece each: quad q sits in piece 8 q + jcol / 2 of each quarter, half jcol & 1
                    const int half = (jcol & 1) << 3;
#pragma unroll
                    for (int qd = 0; qd < 2; ++qd) {
                        const int pc = 8 * qd + (jcol >> 1);
                        *reinterpret_cast<uint2*>(rowp + ((pc ^ key) << 4) + half) = make_uint2(ah_[2 * qd], ah_[2 * qd + 1]);
                        *reinterpret_cast<uint2*>(rowp + (((PP + pc) ^ key) << 4) + half) = make_uint2(xh_[2 * qd], xh_[2 * qd + 1]);
                        *reinterpret_cast<uint2*>(rowp + (((2 * PP + pc) ^ key) << 4) + half) = make_uint2(al_[2 * qd], al_[2 * qd + 1]);
                        *reinterpret_cast<uint2*>(rowp + (((3 * PP + pc) ^ key) << 4) + half) = make_uint2(xl_[2 * qd], xl_[2 * qd + 1]);
                    }
                } else if constexpr (NCH == 8) {
                    // the lane's 8 channels = one 16-byte piece of each quarter
                    *reinterpret_cast<uint4*>(rowp + ((jcol ^ key) << 4)) = make_uint4(ah_[0], ah_[1], ah_[2], ah_[3]);
                    *reinterpret_cast<uint4*>(rowp + (((PP + jcol) ^ key) << 4)) = make_uint4(xh_[0], xh_[1], xh_[2], xh_[3]);
                    *reinterpret_cast<uint4*>(rowp + (((2 * PP + jcol) ^ key) << 4)) = make_uint4(al_[0], al_[1], al_[2], al_[3]);
                    *reinterpret_cast<uint4*>(rowp + (((3 * PP + jcol) ^ key) << 4)) = make_uint4(xl_[0], xl_[1], xl_[2], xl_[3]);
                } else {
                    // the lane's 4 channels = half a piece: lanes 2 i, 2 i + 1 fill piece i of each quarter
                    const int pc = jcol >> 1, half = (jcol & 1) << 3;
                    *reinterpret_cast<uint2*>(rowp + ((pc ^ key) << 4) + half) = make_uint2(ah_[0], ah_[1]);
                    *reinterpret_cast<uint2*>(rowp + (((PP + pc) ^ key) << 4) + half) = make_uint2(xh_[0], xh_[1]);
                    *reinterpret_cast<uint2*>(rowp + (((2 * PP + pc) ^ key) << 4) + half) = make_uint2(al_[0], al_[1]);
                    *reinterpret_cast<uint2*>(rowp + (((3 * PP + pc) ^ key) << 4) + half) = make_uint2(xl_[0], xl_[1]);
                }
            } else {
                // a group past the end of the graph parks nothing, but its count must not land in `ready` while the slot's PREVIOUS tile is still being
                // produced: the consumers would take seven real producers plus this one for eight and read a late producer's rows before they are written
                // (seen on the workgroup that owns the last, partial tile of a scene: tools/det_ws_real.py)
                wait_for(done + sl, (uint32_t)(8 * (it / RING)));
            }
            // this producer's rows of the tile are parked (LDS operations of a wavefront complete in order)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (lane == 0) atomicAdd(const_cast<uint32_t*>(ready + sl), 1u);
        }
    }
}

}  // namespace

// 1 = the wave-specialised kernel takes the 64 -> 128 / 128 -> 128 layers in the default arithmetic (DGNN_WS=0: k_sage_fused_mfma<.., 128> as in rounds 2-4)
int dgnn_ws_enabled() {
    static const int v = getenv("DGNN_WS") ? atoi(getenv("DGNN_WS")) : 1;
    return v;
}

// C ABI (include/dgnn_hip.h): which kernel dgnn_sage_layer_fused_fwd / _decoder_fwd launch for a 64 -> 128 / 128 -> 128 layer in DGNN_GEMM_F16X2
extern "C" int dgnn_wave_specialised_enabled(void) { return dgnn_ws_enabled() != 0 ? 1 : 0; }

// contract: fused_common.h
int dgnn_sage_layer_fused_ws_try(const LayerCall& c, const DecoderTail& t) {
    const bool dec = t.W0 != nullptr;
    if ((c.c_in != WS_C && !(c.c_in == 64 && !dec)) || c.c_out != WS_C || c.lde != FE || c.ldx % 4 != 0 || (!dec && c.ldo % 4 != 0) ||
        ((((uintptr_t)c.x_src | (uintptr_t)c.x_dst | (uintptr_t)c.edge_attr | (uintptr_t)(dec ? nullptr : c.out) | (uintptr_t)c.Wj | (uintptr_t)c.Wi |
           (uintptr_t)t.W0) % 16) != 0) ||
        (dec && ((uintptr_t)t.logits % 8) != 0))
        return DGNN_E_UNSUPPORTED;
    static const int ws64 = getenv("DGNN_WS_64") ? atoi(getenv("DGNN_WS_64")) : 1;     // 0: the 64 -> 128 layer stays on the two-phase kernel
    if (c.c_in == 64 && !ws64) return DGNN_E_UNSUPPORTED;
    const int64_t ntiles = dgnn_cdiv(c.n_dst, WS_TILE);
    int grid = (int)(ntiles < DGNN_NUM_CU ? ntiles : DGNN_NUM_CU);
    if (grid < 1) grid = 1;
    const WsDec d{t.W0, t.b0, t.scale1, t.shift1, t.W3, t.b3, t.logits};
    // dense input rows (the previous fused layer's output) take the instantiation with the stride folded in; any other stride the run-time-stride one
    const bool ldc = c.ldx == c.c_in;
#define DGNN_WS_GO(C_, D_, L_)                                                                                                                              \
    do {                                                                                                                                                    \
        static bool attr_[DGNN_MAX_DEVICES] = {};                                                                                                           \
        const size_t sm_ = D_ ? WsL<C_, 2>::SMEM_DEC : WsL<C_, 2>::SMEM;                                                                                    \
        dgnn_allow_dynamic_lds(reinterpret_cast<const void*>(&k_sage_fused_ws<C_, 2, D_, false, L_>), sm_, attr_);                                          \
        hipLaunchKernelGGL((k_sage_fused_ws<C_, 2, D_, false, L_>), dim3(grid), dim3(1024), sm_, c.stream, c.rowptr, c.src, c.eid, c.n_dst, c.x_src,        \
                           c.x_dst, c.ldx, c.edge_attr, c.lde, c.We, c.be, c.Wj, c.bj, c.Wi, c.scale, c.shift, c.relu, c.out, c.ldo, ntiles, WS_KNOBS, d);  \
    } while (0)
#define DGNN_WS_GO2(C_, D_)                \
    do {                                   \
        if (ldc) DGNN_WS_GO(C_, D_, true); \
        else DGNN_WS_GO(C_, D_, false);    \
    } while (0)
    if (c.c_in == 64) DGNN_WS_GO2(64, false);
    else if (dec) DGNN_WS_GO2(128, true);
    else DGNN_WS_GO2(128, false);
#undef DGNN_WS_GO2
#undef DGNN_WS_GO
    return dgnn_check_launch(dec ? "sage_layer_fused_decoder_fwd(wave-specialised)" : "sage_layer_fused_fwd(wave-specialised)");
}

// The same kernel on the UNSIGNED 16-bit rows of the bf16-storage chain (DGNN_BF16_COMPENSATED | _ROWS_IN_UNSIGNED | _ROWS_OUT_UNSIGNED, fused_bf16.hip): rows
// decoded to fp32 where the producers use them (exact), the fp16 two-part arithmetic of the fp32-I/O kernel in between, rows encoded (round to nearest even
// on bit 15) in the consumers' epilogue.  c_in in {64, 128}, c_out == 128, relu (the format has no sign).  DGNN_E_UNSUPPORTED: the caller keeps its own kernel.
int dgnn_sage_layer_fused_ws16_try(const LayerCall16& c) {
    static const int on = getenv("DGNN_WS_16") ? atoi(getenv("DGNN_WS_16")) : 1;
    const int nch = c.c_in / 16;
    if (!on || !dgnn_ws_enabled() || (c.c_in != 128 && c.c_in != 64) || c.c_out != WS_C || !c.relu || c.lde != FE || c.ldx % nch != 0 || c.ldo % 4 != 0 ||
        ((((uintptr_t)c.x_src | (uintptr_t)c.x_dst) % (2 * nch)) != 0) || ((uintptr_t)c.out % 8) != 0 ||
        ((((uintptr_t)c.edge_attr | (uintptr_t)c.Wj | (uintptr_t)c.Wi) % 16) != 0))
        return DGNN_E_UNSUPPORTED;
    const int64_t ntiles = dgnn_cdiv(c.n_dst, WS_TILE);
    int grid = (int)(ntiles < DGNN_NUM_CU ? ntiles : DGNN_NUM_CU);
    if (grid < 1) grid = 1;
    const WsDec d{};
    const float* xs = static_cast<const float*>(c.x_src);
    const float* xd = static_cast<const float*>(c.x_dst);
    float* o = reinterpret_cast<float*>(c.out);
    const bool ldc = c.ldx == c.c_in;      // (as in dgnn_sage_layer_fused_ws_try)
#define DGNN_WS_GO16(C_, R_, L_)                                                                                                                            \
    do {                                                                                                                                                    \
        static bool attr_[DGNN_MAX_DEVICES] = {};                                                                                                           \
        const size_t sm_ = WsL<C_, R_>::SMEM;                                                                                                               \
        dgnn_allow_dynamic_lds(reinterpret_cast<const void*>(&k_sage_fused_ws<C_, R_, false, true, L_>), sm_, attr_);                                       \
        hipLaunchKernelGGL((k_sage_fused_ws<C_, R_, false, true, L_>), dim3(grid), dim3(1024), sm_, c.stream, c.rowptr, c.src, c.eid, c.n_dst, xs, xd,      \
                           c.ldx, c.edge_attr, c.lde, c.We, c.be, c.Wj, c.bj, c.Wi, c.scale, c.shift, c.relu, o, c.ldo, ntiles, WS_KNOBS, d);               \
    } while (0)
    if (c.c_in == 64) {
        if (ldc) DGNN_WS_GO16(64, 4, true);
        else DGNN_WS_GO16(64, 4, false);
    } else {
        if (ldc) DGNN_WS_GO16(128, 2, true);
        else DGNN_WS_GO16(128, 2, false);
    }
#undef DGNN_WS_GO16
    return dgnn_check_launch("sage_layer_fused_fwd_bf16(wave-specialised)");
}
