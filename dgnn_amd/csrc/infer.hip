// Whole-scene inference in ONE library call (reference SurfaceNet.inference_layer, learning/surfaceNetStaticEdgeFilters.py:323-355; VERDICT r3
// item 2b): destination-sorted plan of the scene's adjacency (dgnn_plan_build), every conv layer with BatchNorm(eval) + ReLU in its launch,
// the decoder inside the last layer's launch -- the launch chain the Python mirror issued call by call (45-65 us of interpreter time per
// layer: a reconbench-size scene of 66k cells was host-bound at 0.29 ms per pass with 0.2 ms of GPU time).  Same kernels, same order, same
// arguments: results are bit-identical to the per-layer entry points (tests/test_gpu_infer.py).  Nothing allocates or synchronises.
#include "fused_common.h"

namespace {

inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

struct Workspace {
    float* act[2];
    int64_t bytes;
};

// act0 | act1 : n x max hidden width floats each, 16-byte aligned
Workspace carve(void* base, int64_t n, int n_layers, const int32_t* widths) {
    Workspace w{};
    int maxw = 0;
    for (int l = 1; l <= n_layers; ++l) maxw = widths[l] > maxw ? widths[l] : maxw;   // outputs of layers 0 .. L-2 (and the last layer's, when the decoder runs apart)
    const int64_t each = align_up(4 * n * maxw, 16);
    char* b = static_cast<char*>(base);
    w.act[0] = reinterpret_cast<float*>(b);
    w.act[1] = reinterpret_cast<float*>(b + each);
    w.bytes = 2 * each;
    return w;
}

// ---- what every one-call entry point is given, filled once from its arguments ------------------------------------------------------------------------
struct Plan {       // the adjacency: an edge list the call sorts into (rowptr, src, eid) itself, or (edge_index NULL) those arrays of an earlier call
    const int64_t* edge_index;
    int64_t stride_row, stride_col, E;
    int hint;
    int32_t *rowptr, *src, *eid, *scratch;
    bool attr_in_plan_order;
};
struct Tables {     // per-layer parameter tables; layer l maps widths[l] -> widths[l + 1] channels
    int n_layers;
    const int32_t* widths;
    const float *const *We, *const *be, *const *Wj, *const *bj, *const *Wi, *const *scale, *const *shift;
};
struct Scene {
    const char* who;
    Plan p;
    int64_t n_loc;      // local rows of x: sources of layer 0
    const float* x;
    int64_t ldx;
    const float* edge_attr;
    int64_t lde;
    int f_e;
    Tables t;
    void* workspace;
    float* logits;
    void* stream;
};
struct Route {      // how the fp32-row chain issues its layers
    const void* const* prepared;
    fused::DecoderTail dec;
    int fuse_decoder, gemm_mode;
};

int check_tables(const Scene& s, int min_layers) {
    const Tables& t = s.t;
    DGNN_REQUIRE(s.n_loc >= 0 && s.p.E >= 0 && t.n_layers >= min_layers && t.n_layers <= 16 && t.widths && t.We && t.be && t.Wj && t.bj && t.Wi && t.scale && t.shift,
                 DGNN_E_INVALID, "%s: bad sizes / null table", s.who);
    return DGNN_OK;
}

// layer l runs over the destinations [0, n_dst[l]) of ONE plan: n_dst must not grow (sources of layer l lie in [0, n_dst[l-1]), in [0, n_loc) for layer 0)
int check_n_dst(const Scene& s, const int64_t* n_dst) {
    DGNN_REQUIRE(n_dst, DGNN_E_INVALID, "%s: bad sizes / null table", s.who);
    for (int l = 0; l < s.t.n_layers; ++l)
        DGNN_REQUIRE(n_dst[l] >= 0 && n_dst[l] <= (l ? n_dst[l - 1] : s.n_loc), DGNN_E_INVALID, "%s: destination counts must not grow from layer to layer", s.who);
    return DGNN_OK;
}

int check_pointers(const Scene& s) {
    DGNN_REQUIRE(s.x && s.edge_attr && s.workspace && s.logits && ((uintptr_t)s.workspace % 16) == 0, DGNN_E_INVALID, "%s: null / unaligned pointer", s.who);
    const Plan& p = s.p;
    DGNN_REQUIRE(p.rowptr && p.src && (!p.edge_index || (p.eid && p.scratch)) && (p.attr_in_plan_order || p.eid), DGNN_E_INVALID, "%s: plan arrays missing", s.who);
    return DGNN_OK;
}

// ---- what the chains below can run: checked before anything is launched ---------------------------------------------------------------------------------
bool rows_ok(const Scene& s) {       // edge rows the kernels read in place, 32-bit element offsets into the activations
    int maxw = 0;
    bool ok = s.f_e == 20 && s.lde == 20 && ((uintptr_t)s.edge_attr % 16) == 0;
    for (int l = 0; l < s.t.n_layers && ok; ++l) {
        const Tables& t = s.t;
        ok = t.We[l] && t.be[l] && t.Wj[l] && t.Wi[l] && ((t.scale[l] == nullptr) == (t.shift[l] == nullptr));
        maxw = t.widths[l + 1] > maxw ? t.widths[l + 1] : maxw;
    }
    return ok && s.n_loc * (int64_t)(s.ldx > maxw ? s.ldx : maxw) < ((int64_t)1 << 31);
}

int chain_supported(const Scene& s, const fused::DecoderTail& d) {
    const int32_t* w = s.t.widths;
    const bool dec2 = d.W0 != nullptr;                     // Linear - BN - ReLU - Linear decoder (:180-187); W0 NULL and W3 given: a single Linear is not covered here
    bool ok = dec2 || d.W3 == nullptr;
    for (int l = 0; l < s.t.n_layers && ok; ++l) ok = fused::takes_f32_rows(w[l], w[l + 1]) && (w[l] <= 64 || w[l] % 2 == 0);
    ok = ok && rows_ok(s);
    if (ok && w[0] > 64) ok = s.ldx % 2 == 0 && ((uintptr_t)s.x % 8) == 0;
    if (ok && dec2) ok = w[s.t.n_layers] == 128 && d.c_hidden == 64 && (d.n_logits == 1 || d.n_logits == 2);    // dgnn_decoder_fused_fwd's shapes
    DGNN_REQUIRE(ok, DGNN_E_UNSUPPORTED, "%s: a layer shape / operand layout outside the fused kernels", s.who);
    return DGNN_OK;
}

int chain_supported_bf16(const Scene& s, const fused::DecoderTail& d, int base) {
    const int32_t* w = s.t.widths;
    const int L = s.t.n_layers;
    bool ok = d.W0 && d.b0 && d.W3 && d.b3 && base == DGNN_BF16_COMPENSATED && w[0] <= 32 && w[0] % 2 == 0 && ((uintptr_t)s.x % 4) == 0 && w[L] == 128 &&
              w[L - 1] > 64 && d.c_hidden == 64 && d.n_logits == 2;
    for (int l = 0; l < L && ok; ++l) ok = fused::takes_bf16_rows(w[l], w[l + 1]);
    DGNN_REQUIRE(ok && rows_ok(s), DGNN_E_UNSUPPORTED, "%s: a layer shape / operand layout / arithmetic mode outside the fully fused bf16-storage chain", s.who);
    return DGNN_OK;
}

// destination-sorted plan of the first n_key local cells, unless the caller brought one
int build_plan(const Scene& s, int64_t n_key) {
    const Plan& p = s.p;
    if (!p.edge_index) return DGNN_OK;
    DGNN_REQUIRE(p.E < INT32_MAX && s.n_loc < INT32_MAX, DGNN_E_UNSUPPORTED, "%s: E and n must fit int32", s.who);
    return dgnn_plan_build(p.edge_index, p.stride_row, p.stride_col, p.E, n_key, s.n_loc, 1, p.hint, p.rowptr, p.src, p.eid, p.scratch, s.stream);
}

// ---- one layer of the fp32-row chain -----------------------------------------------------------------------------------------------------------------------
struct LayerRoute {
    const void* prep;   // prepared parameters of the launch that is tried first, or NULL
    bool with_dec;      // the last layer's launch carries the decoder (only logits are written)
};

LayerRoute route_of(const Scene& s, const Route& r, int l) {
    const bool tail = l == s.t.n_layers - 1 && r.dec.W0 != nullptr;
    LayerRoute k{(r.prepared && r.gemm_mode == DGNN_GEMM_F16X2) ? r.prepared[l] : nullptr,
                 tail && r.fuse_decoder && r.gemm_mode == DGNN_GEMM_F16X2 && r.dec.n_logits == 2};
    if (tail && r.fuse_decoder && !k.with_dec) k.prep = nullptr;      // (a decoder-carrying prepared block is not a plain layer's)
    return k;
}

// Layer l for the destinations [b, e) of the plan, rows h in, rows `out` (all destinations' buffer, stride widths[l + 1]) or logits out: the decoder-carrying launch
// when k.with_dec, else the prepared launch, else the plain one.  A decoder launch that refuses the shape / layout clears k.with_dec (and k.prep: that block is not
// a plain layer's) -- for this range and every later one of the layer, which then run layer and decoder apart.
int issue_layer(const Scene& s, const Route& r, int l, int64_t b, int64_t e, const float* h, int64_t ldh, float* out, LayerRoute& k) {
    const Tables& t = s.t;
    const fused::DecoderTail& d = r.dec;
    const int ci = t.widths[l], co = t.widths[l + 1];
    const int32_t* rowptr = s.p.rowptr + b;
    const int32_t* eid = s.p.attr_in_plan_order ? nullptr : s.p.eid;
    const float* xd = b ? h + b * ldh : nullptr;
    int rc = DGNN_E_UNSUPPORTED;
    if (k.with_dec) {
        float* lg = d.logits + b * d.n_logits;
        rc = k.prep ? dgnn_sage_layer_fused_decoder_fwd_p(rowptr, s.p.src, eid, e - b, h, xd, ldh, ci, s.edge_attr, s.lde, s.f_e, t.We[l], t.be[l], t.Wj[l], t.bj[l],
                                                          t.Wi[l], t.scale[l], t.shift[l], 1, co, d.W0, d.b0, d.scale1, d.shift1, d.c_hidden, d.W3, d.b3, d.n_logits,
                                                          lg, k.prep, s.stream)
                    : dgnn_sage_layer_fused_decoder_fwd(rowptr, s.p.src, eid, e - b, h, xd, ldh, ci, s.edge_attr, s.lde, s.f_e, t.We[l], t.be[l], t.Wj[l], t.bj[l],
                                                        t.Wi[l], t.scale[l], t.shift[l], 1, co, d.W0, d.b0, d.scale1, d.shift1, d.c_hidden, d.W3, d.b3, d.n_logits, lg,
                                                        s.stream);
        if (rc != DGNN_E_UNSUPPORTED) return rc;
        k = LayerRoute{nullptr, false};
    }
    float* o = out + b * co;
    if (k.prep)
        rc = dgnn_sage_layer_fused_fwd_p(rowptr, s.p.src, eid, e - b, h, xd, ldh, ci, s.edge_attr, s.lde, s.f_e, t.We[l], t.be[l], t.Wj[l], t.bj[l], t.Wi[l],
                                         t.scale[l], t.shift[l], 1, co, o, co, k.prep, s.stream);
    if (rc == DGNN_E_UNSUPPORTED)
        rc = dgnn_sage_layer_fused_fwd(rowptr, s.p.src, eid, e - b, h, xd, ldh, ci, s.edge_attr, s.lde, s.f_e, t.We[l], t.be[l], t.Wj[l], t.bj[l], t.Wi[l],
                                       t.scale[l], t.shift[l], 1, co, o, co, r.gemm_mode, s.stream);
    return rc;
}

int decoder_apart(const Scene& s, const fused::DecoderTail& d, const float* h, int64_t ldh, int64_t n) {
    return dgnn_decoder_fused_fwd(h, ldh, n, (int)ldh, d.W0, d.b0, d.scale1, d.shift1, d.c_hidden, d.W3, d.b3, d.n_logits, d.logits, d.n_logits, s.stream);
}

#define DGNN_TRY(call)                    \
    do {                                  \
        const int rc_ = (call);           \
        if (rc_ != DGNN_OK) return rc_;   \
    } while (0)

// The chain shared by the whole-scene call and the ring call: layer l runs over the destinations [0, n_dst[l]) of ONE plan; logits for the first n_dst[L-1] cells.
int infer_chain(const Scene& s, const Route& r, const int64_t* n_dst) {
    const int L = s.t.n_layers;
    DGNN_TRY(check_tables(s, 1));
    DGNN_TRY(check_n_dst(s, n_dst));
    if (n_dst[L - 1] == 0) return DGNN_OK;
    DGNN_TRY(check_pointers(s));
    const bool dec2 = r.dec.W0 != nullptr;
    DGNN_REQUIRE(!dec2 || (r.dec.b0 && r.dec.W3 && r.dec.b3), DGNN_E_INVALID, "%s: incomplete decoder", s.who);
    DGNN_TRY(chain_supported(s, r.dec));
    const Workspace ws = carve(s.workspace, n_dst[0], L, s.t.widths);
    DGNN_TRY(build_plan(s, n_dst[0]));
    const float* h = s.x;
    int64_t ldh = s.ldx;
    for (int l = 0; l < L; ++l) {
        LayerRoute k = route_of(s, r, l);
        float* out = (l == L - 1 && !dec2) ? s.logits : ws.act[l & 1];
        DGNN_TRY(issue_layer(s, r, l, 0, n_dst[l], h, ldh, out, k));
        if (k.with_dec) return DGNN_OK;
        h = out;
        ldh = s.t.widths[l + 1];
    }
    return dec2 ? decoder_apart(s, r.dec, h, ldh, n_dst[L - 1]) : DGNN_OK;
}

}  // namespace

extern "C" int64_t dgnn_static_infer_workspace_bytes(int64_t n, int n_layers, const int32_t* widths) {
    if (n < 0 || n_layers < 1 || !widths) return 0;
    return carve(nullptr, n, n_layers, widths).bytes + 16;
}

extern "C" int dgnn_static_infer_fwd(const int64_t* edge_index, int64_t stride_row, int64_t stride_col, int64_t E, int plan_hint, int32_t* rowptr,
                                     int32_t* src, int32_t* eid, int32_t* plan_scratch, int64_t n, const float* x, int64_t ldx, const float* edge_attr, int64_t lde,
                                     int f_e, int n_layers, const int32_t* widths, const float* const* We, const float* const* be,
                                     const float* const* Wj, const float* const* bj, const float* const* Wi, const float* const* scale,
                                     const float* const* shift, const void* const* prepared, const float* W0, const float* b0, const float* scale1,
                                     const float* shift1, int c_hidden, const float* W3, const float* b3, int n_logits, int fuse_decoder, int gemm_mode,
                                     void* workspace, float* logits, void* stream) {
    DGNN_REQUIRE(n >= 0 && n_layers >= 1 && n_layers <= 16, DGNN_E_INVALID, "static_infer_fwd: bad sizes");
    int64_t n_dst[16];
    for (int l = 0; l < n_layers; ++l) n_dst[l] = n;
    const Scene s{"static_infer_fwd", {edge_index, stride_row, stride_col, E, plan_hint, rowptr, src, eid, plan_scratch, /*attr_in_plan_order=*/eid == nullptr},
                  n, x, ldx, edge_attr, lde, f_e, {n_layers, widths, We, be, Wj, bj, Wi, scale, shift}, workspace, logits, stream};
    return infer_chain(s, {prepared, {W0, b0, scale1, shift1, c_hidden, W3, b3, n_logits, logits}, fuse_decoder, gemm_mode}, n_dst);
}

// ---- one rank's part of a scene cut across GPUs WITHOUT a data-path exchange --------------------------------------------------------------
// The part holds, behind its owned cells, the rings of cells 1 .. L hops away (input rows resident: they are static) and layer l is computed for the owned
// cells AND the rings up to L-1-l hops out -- what the reference does per sampled batch (k-hop recomputation, learning/surfaceNetStaticEdgeFilters.py:232-275)
// applied to a whole part.  A ring of a 1/8 part of the 1M-tet scene is 3.7 % of its cells: ~5 % redundant work buys a step with no collective, no
// interior / boundary split and no transfer latency between the layers (the exchange form below spends 0.35 ms per step where this one spends 0.22).
// Cells are independent of their tile's composition in every fused kernel: the union of the ranks' logits is bit-identical to the whole scene's.
extern "C" int dgnn_static_infer_rings_fwd(const int64_t* edge_index, int64_t stride_row, int64_t stride_col, int64_t E, int plan_hint, int32_t* rowptr, int32_t* src,
                                           int32_t* eid, int32_t* plan_scratch, int attr_in_plan_order, int64_t n_loc, const int64_t* n_dst, const float* x,
                                           int64_t ldx, const float* edge_attr, int64_t lde, int f_e, int n_layers, const int32_t* widths, const float* const* We,
                                           const float* const* be, const float* const* Wj, const float* const* bj, const float* const* Wi,
                                           const float* const* scale, const float* const* shift, const void* const* prepared, const float* W0, const float* b0,
                                           const float* scale1, const float* shift1, int c_hidden, const float* W3, const float* b3, int n_logits,
                                           int fuse_decoder, int gemm_mode, void* workspace, float* logits, void* stream) {
    DGNN_REQUIRE(attr_in_plan_order || eid, DGNN_E_INVALID, "static_infer_rings_fwd: eid missing");
    const Scene s{"static_infer_rings_fwd", {edge_index, stride_row, stride_col, E, plan_hint, rowptr, src, eid, plan_scratch, attr_in_plan_order != 0},
                  n_loc, x, ldx, edge_attr, lde, f_e, {n_layers, widths, We, be, Wj, bj, Wi, scale, shift}, workspace, logits, stream};
    return infer_chain(s, {prepared, {W0, b0, scale1, shift1, c_hidden, W3, b3, n_logits, logits}, fuse_decoder, gemm_mode}, n_dst);
}

// ---- bf16 STORAGE (BASELINE config 3), whole scene or ring part, one call ------------------------------------------------------------------------------
// The chain SurfaceNet.inference_layer runs in bf16 storage when every layer has the fused form: layer 0 reads the caller's fp32 rows in place and
// starts the 16-bit rows (UNSIGNED when `mode` carries DGNN_BF16_ROWS_OUT_UNSIGNED: 9 significant bits behind the ReLU), the middle layers keep the
// format, the last layer's launch carries the decoder and writes fp32 logits.  Configurations outside that form: DGNN_E_UNSUPPORTED, nothing launched
// (the Python mirror then issues its per-layer chain).
extern "C" int dgnn_static_infer_rings_fwd_bf16(const int64_t* edge_index, int64_t stride_row, int64_t stride_col, int64_t E, int plan_hint, int32_t* rowptr,
                                                int32_t* src, int32_t* eid, int32_t* plan_scratch, int attr_in_plan_order, int64_t n_loc, const int64_t* n_dst,
                                                const float* x, int64_t ldx, const float* edge_attr, int64_t lde, int f_e, int n_layers, const int32_t* widths,
                                                const float* const* We, const float* const* be, const float* const* Wj, const float* const* bj,
                                                const float* const* Wi, const float* const* scale, const float* const* shift, const float* W0, const float* b0,
                                                const float* scale1, const float* shift1, int c_hidden, const float* W3, const float* b3, int n_logits, int mode,
                                                void* workspace, float* logits, void* stream) {
    const Scene s{"static_infer_rings_fwd_bf16", {edge_index, stride_row, stride_col, E, plan_hint, rowptr, src, eid, plan_scratch, attr_in_plan_order != 0},
                  n_loc, x, ldx, edge_attr, lde, f_e, {n_layers, widths, We, be, Wj, bj, Wi, scale, shift}, workspace, logits, stream};
    DGNN_TRY(check_tables(s, 2));
    DGNN_TRY(check_n_dst(s, n_dst));
    if (n_dst[n_layers - 1] == 0) return DGNN_OK;
    DGNN_TRY(check_pointers(s));
    const bool uns = (mode & DGNN_BF16_ROWS_OUT_UNSIGNED) != 0;
    const int base = mode & ~(DGNN_BF16_ROWS_IN_UNSIGNED | DGNN_BF16_ROWS_OUT_UNSIGNED);
    DGNN_TRY(chain_supported_bf16(s, {W0, b0, scale1, shift1, c_hidden, W3, b3, n_logits, logits}, base));
    const Workspace ws = carve(workspace, n_dst[0], n_layers, widths);      // (sized for 4-byte rows: the 2-byte rows use half of each buffer)
    DGNN_TRY(build_plan(s, n_dst[0]));
    const int32_t* e_ = attr_in_plan_order ? nullptr : eid;
    const void* h = x;
    int64_t ldh = ldx;
    for (int l = 0; l < n_layers; ++l) {
        const int ci = widths[l], co = widths[l + 1];
        const int fmt = uns ? ((l ? DGNN_BF16_ROWS_IN_UNSIGNED : 0) | DGNN_BF16_ROWS_OUT_UNSIGNED) : 0;
        if (l == n_layers - 1)
            return dgnn_sage_layer_fused_decoder_fwd_bf16(rowptr, src, e_, n_dst[l], static_cast<const uint16_t*>(h), nullptr, ldh, ci, edge_attr, lde, f_e, We[l],
                                                          be[l], Wj[l], bj[l], Wi[l], scale[l], shift[l], 1, co, W0, b0, scale1, shift1, c_hidden, W3, b3, n_logits,
                                                          logits, base | (uns ? DGNN_BF16_ROWS_IN_UNSIGNED : 0), stream);
        uint16_t* out = reinterpret_cast<uint16_t*>(ws.act[l & 1]);
        DGNN_TRY(dgnn_sage_layer_fused_fwd_bf16(rowptr, src, e_, n_dst[l], h, l == 0, nullptr, ldh, ci, edge_attr, lde, f_e, We[l], be[l], Wj[l], bj[l], Wi[l],
                                                scale[l], shift[l], 1, co, out, co, base | fmt, stream));
        h = out;
        ldh = co;
    }
    return DGNN_OK;
}

// ---- one rank's part of a scene cut across GPUs, ONE call per step (dgnn_amd/partition.py run_partitioned_layers) -------------------------
// The launch chain PartitionedScene.inference_layer issued from Python -- plan of the local bipartite graph, layer 0 over the owned cells, then per
// later layer [interior cells | wait for the halo | boundary cells] with the exchange of the layer's output rows started right behind it -- was
// host-bound at a strong-scaling shard: a 1/8 part of the 1M-tet scene (126k owned cells) has 0.2 ms of GPU work behind 0.58 ms of interpreter time
// (tools/bench_partition_rank.py).  Same kernels, ranges and order: bit-identical to the per-layer calls and therefore to the whole scene.
extern "C" int dgnn_static_infer_partitioned_fwd(const int64_t* edge_index, int64_t stride_row, int64_t stride_col, int64_t E, int plan_hint, int32_t* rowptr,
                                                 int32_t* src, int32_t* eid, int32_t* plan_scratch, int attr_in_plan_order, int64_t n_own, int64_t n_interior,
                                                 int64_t n_halo, const float* x, int64_t ldx, const float* edge_attr, int64_t lde, int f_e, int n_layers,
                                                 const int32_t* widths, const float* const* We, const float* const* be, const float* const* Wj,
                                                 const float* const* bj, const float* const* Wi, const float* const* scale, const float* const* shift,
                                                 const void* const* prepared, const float* W0, const float* b0, const float* scale1, const float* shift1,
                                                 int c_hidden, const float* W3, const float* b3, int n_logits, int fuse_decoder, int gemm_mode,
                                                 dgnn_halo_plan* halo, void* comm, void* send_buf, void* workspace, float* logits, void* stream) {
    const char* who = "static_infer_partitioned_fwd";
    DGNN_REQUIRE(n_own >= 0 && n_halo >= 0 && n_interior >= 0 && n_interior <= n_own, DGNN_E_INVALID, "%s: bad sizes / null table", who);
    const int64_t n_loc = n_own + n_halo;
    const Scene s{who, {edge_index, stride_row, stride_col, E, plan_hint, rowptr, src, eid, plan_scratch, attr_in_plan_order != 0},
                  n_loc, x, ldx, edge_attr, lde, f_e, {n_layers, widths, We, be, Wj, bj, Wi, scale, shift}, workspace, logits, stream};
    const Route r{prepared, {W0, b0, scale1, shift1, c_hidden, W3, b3, n_logits, logits}, fuse_decoder, gemm_mode};
    DGNN_TRY(check_tables(s, 1));
    if (n_loc == 0) return DGNN_OK;
    DGNN_TRY(check_pointers(s));
    DGNN_REQUIRE(!halo || (dgnn_halo_recv_rows(halo) == n_halo && (dgnn_halo_send_rows(halo) == 0 || send_buf)), DGNN_E_INVALID,
                 "%s: the halo plan receives %lld rows, the part has %lld halo rows (or no send buffer)", who,
                 (long long)(halo ? dgnn_halo_recv_rows(halo) : 0), (long long)n_halo);
    DGNN_REQUIRE(halo || n_halo == 0, DGNN_E_INVALID, "%s: halo rows without a halo plan", who);
    const bool dec2 = W0 != nullptr;
    DGNN_REQUIRE(!dec2 || (b0 && W3 && b3), DGNN_E_INVALID, "%s: incomplete decoder", who);
    DGNN_TRY(chain_supported(s, r.dec));
    const Workspace ws = carve(workspace, n_loc, n_layers, widths);
    DGNN_TRY(build_plan(s, n_own));
    const float* h = x;
    int64_t ldh = ldx;
    bool decoder_done = false;
    for (int l = 0; l < n_layers; ++l) {
        const bool last = l == n_layers - 1;
        LayerRoute k = route_of(s, r, l);     // decided on the layer's first launch: a refused decoder launch sends BOTH ranges down the layer-then-decoder route
        float* out = (last && !dec2) ? logits : ws.act[l & 1];
        // layer 0 reads input rows only (the halo's are resident); later layers: interior cells, then -- the halo has landed -- boundary cells
        const int64_t cut[3] = {0, l == 0 ? n_own : n_interior, n_own};
        for (int part = 0; part < 2; ++part) {
            if (part == 1 && l > 0 && halo) DGNN_TRY(dgnn_halo_exchange_wait(halo, stream));
            if (cut[part + 1] <= cut[part]) continue;
            DGNN_TRY(issue_layer(s, r, l, cut[part], cut[part + 1], h, ldh, out, k));
            decoder_done = decoder_done || k.with_dec;
        }
        // the rows the peers' boundary cells read next, the peers' rows into this buffer's tail
        if (!last && halo) DGNN_TRY(dgnn_halo_exchange_start(halo, comm, out, widths[l + 1], widths[l + 1], 4, send_buf, stream));
        h = out;
        ldh = widths[l + 1];
    }
    return (dec2 && !decoder_done) ? decoder_apart(s, r.dec, h, ldh, n_own) : DGNN_OK;
}
