// k-hop full-neighbour block builder on the GPU: the replacement for
// torch_geometric NeighborSampler(edge_index, sizes=[-1]*k, ...) that the reference runs on the CPU
// (run.py:72-74, 221-223; consumed at surfaceNetStaticEdgeFilters.py:214-217, 258-264).
//
// One hop = dgnn_khop_count + (host reads the edge total to size the outputs) + dgnn_khop_expand.
// Semantics (PyG 2.0.2 sample_adj with size -1, see oracle/pyg_semantics.py): for the current target list
// n_id[0..n_t), emit all in-edges in (target order, plan order) -- plan order = ascending edge position, which
// for the reference's adjacency layout equals ascending source id, PyG's order -- relabelled to local ids where
// targets keep their positions and newly seen sources are appended in order of first appearance.
// `pos` (int32 [n_nodes], all -1 between batches) carries the global->local map across the hops of a batch.
//
// Sampled neighbourhoods (sizes[h] > 0; DESIGN "Sampled neighbourhoods"): the *_sampled entry points keep, of a target with more than
// `size` in-edges, the `size` of them with the smallest 64-bit keys key(seed, draw, hop, global id, j) -- j = rank of the in-edge in plan
// order, ties to the smaller j -- and leave them in plan order; everything downstream (local ids, first appearance, e_id) is the
// construction above applied to the kept edges.  The key is a counter-based hash (khop_select below): no device RNG, no atomics in the
// selection, so a block is a pure function of (graph, batch, sizes, seed, draw).  Every pass is ONE kernel template over the selection
// with two instantiations, KhopAll (every in-edge, no draw to carry) and KhopDraw; both families of entry points run the same host bodies.
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "common.h"
#include "mix64.h"

namespace {

// ---- the selection: which in-edges of a target a hop keeps --------------------------------------------------------------------------
struct KhopAll {};   // a full neighbourhood: every in-edge, rank = position, no draw to carry
struct KhopDraw {
    int size;        // in-edges kept per target at most; < 0: all of them
    uint64_t base;   // mix64(seed + 0x9E3779B97F4A7C15 * (draw + 1))
    uint64_t hop;    // builder hop << 32
};

inline KhopDraw khop_draw(int size, uint64_t seed, int64_t draw, int hop) {
    return KhopDraw{size, mix64(seed + 0x9E3779B97F4A7C15ull * ((uint64_t)draw + 1ull)), (uint64_t)(uint32_t)hop << 32};
}
constexpr KhopDraw KHOP_EVERYTHING{-1, 0, 0};   // what the host hands over for a full neighbourhood; the kernels then get a KhopAll

// how many of a target's d in-edges are kept: all the count pass needs of the selection
__device__ __forceinline__ int khop_kept(const KhopAll, int d) { return d; }
__device__ __forceinline__ int khop_kept(const KhopDraw s, int d) { return (s.size >= 0 && d > s.size) ? s.size : d; }

// THE selection, recomputed identically by the first, flags and emit passes: calls keep(j, r) for every kept in-edge j (rank in
// plan order) of the target with global id g and in-degree d, r = its rank among the kept ones, in ascending j; returns how many.
// key_j = mix64(mix64(base ^ g) + (hop << 32 | j)); kept = the `size` smallest (key, j) pairs.  d <= 8 (a Delaunay cell: 4): the keys sit
// in registers and every lane runs the same 8 x 8 compare network, predicated on j < d; longer segments recompute the keys in a loop
// that is quadratic in d (the convention of graphcut.hip's k_sort_segments).
template <typename F>
__device__ __forceinline__ int khop_select(const KhopAll, int64_t, int d, F keep) {
    for (int j = 0; j < d; ++j) keep(j, j);
    return d;
}

template <typename F>
__device__ __forceinline__ int khop_select(const KhopDraw s, int64_t g, int d, F keep) {
    if (s.size < 0 || d <= s.size) {   // (spelled out, not a call of the overload above: that moves instructions in all three kernels)
        for (int j = 0; j < d; ++j) keep(j, j);
        return d;
    }
    const uint64_t b = mix64(s.base ^ (uint64_t)g);
    int r = 0;
    if (d <= 8) {
        uint64_t key[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) key[j] = mix64(b + (s.hop | (uint64_t)j));
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            int smaller = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) smaller += (i < d && (key[i] < key[j] || (key[i] == key[j] && i < j))) ? 1 : 0;
            if (j < d && smaller < s.size) keep(j, r++);
        }
        return r;
    }
    for (int j = 0; j < d; ++j) {
        const uint64_t kj = mix64(b + (s.hop | (uint64_t)(uint32_t)j));
        int smaller = 0;
        for (int i = 0; i < d; ++i) {
            const uint64_t ki = mix64(b + (s.hop | (uint64_t)(uint32_t)i));
            smaller += (ki < kj || (ki == kj && i < j)) ? 1 : 0;
        }
        if (smaller < s.size) keep(j, r++);
    }
    return r;
}

// ---- the four passes of a hop, one thread per target; Sel = KhopAll | KhopDraw -------------------------------------------------------
template <typename Sel>
__global__ void k_khop_deg(const int32_t* __restrict__ rowptr, const int64_t* __restrict__ n_id, int64_t n_t, int first_hop, const Sel sel,
                           int32_t* __restrict__ deg, int32_t* __restrict__ pos) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_t; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t g = n_id[i];
        deg[i] = khop_kept(sel, rowptr[g + 1] - rowptr[g]);
        if (first_hop) pos[g] = (int32_t)i;  // later hops: already set when the node was discovered
    }
}

// first[g] = smallest slot at which an unseen source g appears
template <typename Sel>
__global__ void k_khop_first(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ src, const int64_t* __restrict__ n_id,
                             int64_t n_t, const int32_t* __restrict__ off, const int32_t* __restrict__ pos, const Sel sel,
                             int32_t* __restrict__ first) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_t; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t g = n_id[i];
        const int b = rowptr[g], e = rowptr[g + 1], o = off[i];
        khop_select(sel, g, e - b, [&](int j, int r) {
            const int s = src[b + j];
            if (pos[s] < 0) atomicMin(&first[s], o + r);
        });
    }
}

template <typename Sel>
__global__ void k_khop_flags(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ src, const int64_t* __restrict__ n_id,
                             int64_t n_t, const int32_t* __restrict__ off, const int32_t* __restrict__ pos,
                             const int32_t* __restrict__ first, const Sel sel, int32_t* __restrict__ flags) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_t; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t g = n_id[i];
        const int b = rowptr[g], e = rowptr[g + 1], o = off[i];
        khop_select(sel, g, e - b, [&](int j, int r) {
            const int s = src[b + j], q = o + r;
            flags[q] = (pos[s] < 0 && first[s] == q) ? 1 : 0;
        });
    }
}

template <typename Sel>
__global__ void k_khop_emit(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ src, const int32_t* __restrict__ eid,
                            const int64_t* __restrict__ n_id, int64_t n_t, const int32_t* __restrict__ off,
                            const int32_t* __restrict__ pos, const int32_t* __restrict__ first, const int32_t* __restrict__ rank,
                            const Sel sel, int64_t* __restrict__ e_src, int64_t* __restrict__ e_dst, int64_t* __restrict__ e_id,
                            int64_t* __restrict__ n_id_out) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_t; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t g = n_id[i];
        const int b = rowptr[g], e = rowptr[g + 1], o = off[i];
        n_id_out[i] = g;
        khop_select(sel, g, e - b, [&](int j, int r) {
            const int s = src[b + j], q = o + r;
            const int p = pos[s];
            int64_t local;
            if (p >= 0) {
                local = p;
            } else {
                const int fq = first[s];
                local = n_t + rank[fq];
                if (fq == q) n_id_out[local] = s;
            }
            e_src[q] = local;
            e_dst[q] = i;
            e_id[q] = eid[b + j];
        });
    }
}

// after emit: newly discovered nodes get their local id in `pos`, `first` goes back to INT_MAX
__global__ void k_khop_commit(const int64_t* __restrict__ n_id_out, int64_t n_t, int64_t n_all, int32_t* __restrict__ pos,
                              int32_t* __restrict__ first) {
    for (int64_t i = n_t + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_all; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t g = n_id_out[i];
        pos[g] = (int32_t)i;
        first[g] = INT32_MAX;
    }
}

__global__ void k_khop_reset(const int64_t* __restrict__ n_id, int64_t n, int32_t* __restrict__ pos) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) pos[n_id[i]] = -1;
}

__global__ void k_fill_i32(int32_t* p, int64_t n, int32_t v) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = v;
}

}  // namespace

int dgnn_exclusive_scan_i32(const int32_t* in, int64_t n, int32_t* out /*[n+1]*/, int32_t* sums_scratch, hipStream_t stream);  // plan.hip

extern "C" int dgnn_fill_i32(int32_t* p, int64_t n, int32_t value, void* stream) {
    DGNN_REQUIRE(n >= 0 && (n == 0 || p), DGNN_E_INVALID, "fill_i32: bad args");
    if (n == 0) return DGNN_OK;
    hipLaunchKernelGGL(k_fill_i32, dim3(dgnn_grid_cap(dgnn_cdiv(n, 256))), dim3(256), 0, (hipStream_t)stream, p, n, value);
    return dgnn_check_launch("fill_i32");
}

extern "C" int64_t dgnn_khop_scratch_elems(int64_t n_t, int64_t max_edges) {
    return (n_t + 1) + (max_edges + 1) + (max_edges + 1) + 2 * (dgnn_cdiv(n_t > max_edges ? n_t : max_edges, 2048) + 4);
}

// The two steps of a hop, written once for both families of entry points; `who` names the entry point in the error texts.  A selection that
// keeps every in-edge (size -1) runs the KhopAll instantiations, any other the KhopDraw ones.
template <typename F>
static int khop_with_selection(const KhopDraw& kd, F body) {
    return kd.size < 0 ? body(KhopAll{}) : body(kd);
}

// step 1: off[i] = exclusive scan of the kept in-degrees of the targets, off[n_t] = number of block edges (device)
static int khop_count(const char* who, const KhopDraw& kd, const int32_t* rowptr, const int64_t* n_id, int64_t n_t, int first_hop, int32_t* pos,
                      int32_t* off, int32_t* scratch, hipStream_t stream) {
    DGNN_REQUIRE(n_t >= 0 && rowptr && pos && off && scratch && (n_t == 0 || n_id), DGNN_E_INVALID, "%s: bad args", who);
    return khop_with_selection(kd, [&](auto sel) {
        int32_t* deg = scratch;
        if (n_t > 0)
            hipLaunchKernelGGL(k_khop_deg<decltype(sel)>, dim3(dgnn_grid_cap(dgnn_cdiv(n_t, 256))), dim3(256), 0, stream, rowptr, n_id, n_t, first_hop,
                               sel, deg, pos);
        const int rc = dgnn_exclusive_scan_i32(deg, n_t, off, scratch + n_t + 1, stream);
        return rc ? rc : dgnn_check_launch(who);
    });
}

// step 2: emit the block.  n_edges = off[n_t] as read by the host; `first` must be all INT32_MAX, `pos` as described above.
static int khop_expand(const char* who, const KhopDraw& kd, const int32_t* rowptr, const int32_t* src, const int32_t* eid, const int64_t* n_id,
                       int64_t n_t, const int32_t* off, int64_t n_edges, int32_t* pos, int32_t* first, int64_t* e_src, int64_t* e_dst, int64_t* e_id,
                       int64_t* n_id_out, int32_t* n_new_out, int32_t* scratch, hipStream_t stream) {
    DGNN_REQUIRE(n_t >= 0 && n_edges >= 0 && rowptr && src && eid && off && pos && first && n_id_out && n_new_out && scratch, DGNN_E_INVALID,
                 "%s: bad args", who);
    return khop_with_selection(kd, [&](auto sel) {
        using Sel = decltype(sel);
        int32_t* flags = scratch;                 // [n_edges]
        int32_t* rank = flags + n_edges + 1;      // [n_edges + 1]
        int32_t* sums = rank + n_edges + 1;
        const dim3 grid(dgnn_grid_cap(dgnn_cdiv(n_t > 0 ? n_t : 1, 256))), block(256);
        if (n_t > 0 && n_edges > 0) {
            hipLaunchKernelGGL(k_khop_first<Sel>, grid, block, 0, stream, rowptr, src, n_id, n_t, off, pos, sel, first);
            hipLaunchKernelGGL(k_khop_flags<Sel>, grid, block, 0, stream, rowptr, src, n_id, n_t, off, pos, first, sel, flags);
        }
        const int rc = dgnn_exclusive_scan_i32(flags, n_edges, rank, sums, stream);
        if (rc) return rc;
        (void)hipMemcpyAsync(n_new_out, rank + n_edges, sizeof(int32_t), hipMemcpyDeviceToDevice, stream);
        if (n_t > 0)
            hipLaunchKernelGGL(k_khop_emit<Sel>, grid, block, 0, stream, rowptr, src, eid, n_id, n_t, off, pos, first, rank, sel, e_src, e_dst, e_id,
                               n_id_out);
        return dgnn_check_launch(who);
    });
}

extern "C" int dgnn_khop_count(const int32_t* rowptr, const int64_t* n_id, int64_t n_t, int first_hop, int32_t* pos, int32_t* off,
                               int32_t* scratch, void* stream) {
    return khop_count("khop_count", KHOP_EVERYTHING, rowptr, n_id, n_t, first_hop, pos, off, scratch, (hipStream_t)stream);
}

extern "C" int dgnn_khop_expand(const int32_t* rowptr, const int32_t* src, const int32_t* eid, const int64_t* n_id, int64_t n_t,
                                const int32_t* off, int64_t n_edges, int32_t* pos, int32_t* first, int64_t* e_src, int64_t* e_dst,
                                int64_t* e_id, int64_t* n_id_out, int32_t* n_new_out, int32_t* scratch, void* stream) {
    return khop_expand("khop_expand", KHOP_EVERYTHING, rowptr, src, eid, n_id, n_t, off, n_edges, pos, first, e_src, e_dst, e_id, n_id_out, n_new_out,
                       scratch, (hipStream_t)stream);
}

// The sampled forms of dgnn_khop_count / dgnn_khop_expand (same buffers, same protocol): off[i] = exclusive scan of min(d_i, size) and the
// block of the kept in-edges only.  size = -1 keeps everything (the result of the plain entry points); seed / draw / hop feed the key -- the
// COUNT of kept edges depends on the size alone, its arguments mirror dgnn_khop_expand_sampled.
static bool khop_draw_ok(int size, int64_t draw, int hop) { return (size == -1 || size >= 1) && draw >= 0 && hop >= 0 && hop < 65536; }

extern "C" int dgnn_khop_count_sampled(const int32_t* rowptr, const int64_t* n_id, int64_t n_t, int first_hop, int size, uint64_t seed, int64_t draw,
                                       int hop, int32_t* pos, int32_t* off, int32_t* scratch, void* stream) {
    DGNN_REQUIRE(khop_draw_ok(size, draw, hop), DGNN_E_INVALID, "khop_count_sampled: bad args");
    return khop_count("khop_count_sampled", khop_draw(size, seed, draw, hop), rowptr, n_id, n_t, first_hop, pos, off, scratch, (hipStream_t)stream);
}

extern "C" int dgnn_khop_expand_sampled(const int32_t* rowptr, const int32_t* src, const int32_t* eid, const int64_t* n_id, int64_t n_t,
                                        const int32_t* off, int64_t n_edges, int size, uint64_t seed, int64_t draw, int hop, int32_t* pos,
                                        int32_t* first, int64_t* e_src, int64_t* e_dst, int64_t* e_id, int64_t* n_id_out, int32_t* n_new_out,
                                        int32_t* scratch, void* stream) {
    DGNN_REQUIRE(khop_draw_ok(size, draw, hop), DGNN_E_INVALID, "khop_expand_sampled: bad args");
    return khop_expand("khop_expand_sampled", khop_draw(size, seed, draw, hop), rowptr, src, eid, n_id, n_t, off, n_edges, pos, first, e_src, e_dst, e_id,
                       n_id_out, n_new_out, scratch, (hipStream_t)stream);
}

// step 3 (after the host read n_new): record the new nodes' local ids for the next hop
extern "C" int dgnn_khop_commit(const int64_t* n_id_out, int64_t n_t, int64_t n_all, int32_t* pos, int32_t* first, void* stream) {
    DGNN_REQUIRE(n_all >= n_t && n_t >= 0 && pos && first && (n_all == 0 || n_id_out), DGNN_E_INVALID, "khop_commit: bad args");
    if (n_all > n_t)
        hipLaunchKernelGGL(k_khop_commit, dim3(dgnn_grid_cap(dgnn_cdiv(n_all - n_t, 256))), dim3(256), 0, (hipStream_t)stream, n_id_out,
                           n_t, n_all, pos, first);
    return dgnn_check_launch("khop_commit");
}

// end of batch: pos[n_id[*]] = -1
extern "C" int dgnn_khop_reset(const int64_t* n_id, int64_t n, int32_t* pos, void* stream) {
    DGNN_REQUIRE(n >= 0 && pos && (n == 0 || n_id), DGNN_E_INVALID, "khop_reset: bad args");
    if (n > 0) hipLaunchKernelGGL(k_khop_reset, dim3(dgnn_grid_cap(dgnn_cdiv(n, 256))), dim3(256), 0, (hipStream_t)stream, n_id, n, pos);
    return dgnn_check_launch("khop_reset");
}

namespace {
__global__ void k_take_i32(const int32_t* __restrict__ in, const int32_t* __restrict__ idx, int64_t n, int32_t* __restrict__ out) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = in[idx[i]];
}

__global__ void k_i64_to_i32_x2(const int64_t* __restrict__ a, const int64_t* __restrict__ b, int64_t n, int32_t* __restrict__ a32,
                                int32_t* __restrict__ b32) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        a32[i] = (int32_t)a[i];
        b32[i] = (int32_t)b[i];
    }
}
}  // namespace

namespace {

// One device -> host word without a stream synchronize: a one-thread kernel stores {value, ticket} into pinned host memory that
// is mapped into the GPU, the host spins on the ticket.  hipStreamSynchronize / a pageable hipMemcpy would do, but both go
// through the runtime's queue locks, which a second host thread that is launching the training step at the same time also
// needs; the spin touches no HIP API.  Falls back to hipMemcpy + hipStreamSynchronize when pinned memory is unavailable.
struct Slot {
    volatile int32_t value;
    volatile uint32_t ticket;
    int32_t pad[14];
};
constexpr int N_SLOTS = 64;
Slot* g_slots_host = nullptr;
Slot* g_slots_dev = nullptr;
unsigned g_slot_busy[N_SLOTS];
unsigned g_ticket = 0;

bool slots_init() {
    static bool tried = false, ok = false;
    static std::mutex m;
    std::lock_guard<std::mutex> lock(m);
    if (!tried) {
        tried = true;
        const char* env = getenv("DGNN_KHOP_MAILBOX");   // "0": always hipMemcpy + hipStreamSynchronize (A/B measurements)
        if (env && env[0] == '0') return false;
        void* h = nullptr;
        if (hipHostMalloc(&h, sizeof(Slot) * N_SLOTS, hipHostMallocPortable | hipHostMallocMapped) == hipSuccess && h) {
            memset(h, 0, sizeof(Slot) * N_SLOTS);
            void* d = nullptr;
            if (hipHostGetDevicePointer(&d, h, 0) == hipSuccess && d) {
                g_slots_host = reinterpret_cast<Slot*>(h);
                g_slots_dev = reinterpret_cast<Slot*>(d);
                ok = true;
            } else {
                (void)hipHostFree(h);
            }
        }
        (void)hipGetLastError();
    }
    return ok;
}

inline void cpu_relax() {   // spin-wait hint of the host architecture (the library also builds on non-x86 hosts)
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield" ::: "memory");
#else
    std::this_thread::yield();
#endif
}

struct Mailbox {   // one slot for the duration of a call
    int idx = -1;
    Mailbox() {
        if (!slots_init()) return;
        for (int i = 0; i < N_SLOTS; ++i)
            if (__atomic_exchange_n(&g_slot_busy[i], 1u, __ATOMIC_ACQ_REL) == 0u) {
                idx = i;
                return;
            }
    }
    ~Mailbox() {
        if (idx >= 0) __atomic_store_n(&g_slot_busy[idx], 0u, __ATOMIC_RELEASE);
    }
};

__global__ void k_publish(const int32_t* __restrict__ value, Slot* slot, uint32_t ticket) {
    slot->value = *value;
    __threadfence_system();
    slot->ticket = ticket;
}

bool read_back(const int32_t* dev_value, int32_t* out, const Mailbox& mb, hipStream_t stream) {
    if (mb.idx >= 0) {
        uint32_t ticket = __atomic_add_fetch(&g_ticket, 1u, __ATOMIC_RELAXED);
        if (ticket == 0) ticket = __atomic_add_fetch(&g_ticket, 1u, __ATOMIC_RELAXED);
        hipLaunchKernelGGL(k_publish, dim3(1), dim3(1), 0, stream, dev_value, g_slots_dev + mb.idx, ticket);
        if (hipGetLastError() == hipSuccess) {
            Slot* s = g_slots_host + mb.idx;
            const auto t0 = std::chrono::steady_clock::now();
            for (uint64_t spins = 0;; ++spins) {
                if (__atomic_load_n(&s->ticket, __ATOMIC_ACQUIRE) == ticket) {
                    *out = s->value;
                    return true;
                }
                cpu_relax();
                if ((spins & 0xFFFF) == 0xFFFF && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(20)) break;   // a hung queue
            }
            // timed out: the queued k_publish still targets this slot.  It is only handed back (Mailbox destructor) after the stream has drained,
            // which the synchronising copy below does before this function returns.
        }
    }
    return hipMemcpyAsync(out, dev_value, sizeof(int32_t), hipMemcpyDeviceToHost, stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
}

}  // namespace

// All hops of one batch in ONE call, for graphs whose every node has exactly `deg` in-edges (a Delaunay scene: 4), so that a
// hop's edge count is known without reading it back and only the number of newly discovered nodes crosses to the host (one
// 4-byte read per hop, waited for INSIDE this call: a caller that runs it on a worker thread -- ctypes releases the GIL --
// overlaps those round trips with the training step it is enqueueing).  KhopBlocks is what the six dgnn_khop_blocks_* entry points
// share, in the order they take it: outputs go into caller-allocated buffers with per-hop capacities, and hop h (0 = the targets' own
// neighbourhood, i.e. the INNERMOST block) writes element h of every per-hop array.
struct KhopBlocks {
    const int32_t *rowptr, *src, *eid;   // the graph's destination-sorted plan; every node has exactly `deg` in-edges
    int deg;
    const int64_t* batch;                // the targets
    int64_t n_batch;
    int hops;
    int32_t *pos, *first;                // the builder's state: all -1 / all INT32_MAX between batches
    int64_t* const* ei;                  // ei[h] int64 [2, cap_e[h]]: rows 0 / 1 = local source / destination ids of its counts[h] * deg edges
    int64_t* const* e_id;                // e_id[h] int64 [cap_e[h]]: graph edge ids
    int32_t *const *src32, *const *e_id32;   // int32 [cap_e[h]] = row 0 of ei[h] (the plan's `src`) / e_id[h] (rows of the scene's edge_attr, read in place)
    int32_t* const* off;                 // off[h] int32 [cap_t[h] + 1]: row offsets (the plan's rowptr)
    int64_t* const* n_id_out;            // n_id_out[h] int64 [cap_t[h] + cap_e[h]]: node ids, its targets, then the new sources in order of first appearance
    const int64_t *cap_t, *cap_e;
    int32_t *scratch, *n_new_dev;
    // t_rowptr != NULL: every hop's transposed plan as well (dgnn_plan_build by source: t_rowptr[h] int32 [cap_all[h] + 1], t_dst[h] / t_eid[h]
    // int32 [cap_e[h]]) and t_rows[h] = e_id32[h][t_eid[h]]; plan_scratch = max_h dgnn_plan_scratch_elems(cap_e[h], cap_all[h])
    int32_t *const *t_rowptr, *const *t_dst, *const *t_eid, *const *t_rows;
    const int64_t* cap_all;
    int32_t* plan_scratch;
    void* stream;
    // `sizes` (NULL: full neighbourhoods, dgnn_khop_blocks_regular) makes it the sampled builder, dgnn_khop_blocks_sampled: hop h keeps
    // e_h = min(sizes[h], deg) in-edges per target (deg for sizes[h] = -1), drawn as khop_select says with (seed, draw, h), so its edge count
    // counts[h] * e_h is again known without a read-back; a hop with e_h = deg runs the KhopAll kernels.
    const int32_t* sizes = nullptr;
    uint64_t seed = 0;
    int64_t draw = 0;
};

// counts_out (HOST int64 [hops + 1]) receives the number of targets of every hop and, last, the node count of the outermost block.
// Returns DGNN_E_INVALID when a capacity is too small (nothing is left half-written in `pos` / `first`).
static int khop_blocks(const KhopBlocks& a, int64_t* counts_out) {
    hipStream_t stream = (hipStream_t)a.stream;
    DGNN_REQUIRE(a.hops >= 1 && a.hops <= 16 && a.deg >= 1 && a.n_batch >= 0 && a.rowptr && a.src && a.eid && a.pos && a.first && a.ei && a.e_id && a.src32 &&
                     a.e_id32 && a.off && a.n_id_out && a.cap_t && a.cap_e && a.scratch && a.n_new_dev && counts_out && (a.n_batch == 0 || a.batch),
                 DGNN_E_INVALID, "khop_blocks_regular: bad args");
    if (a.sizes) {
        DGNN_REQUIRE(a.draw >= 0, DGNN_E_INVALID, "khop_blocks_sampled: draw < 0");
        for (int q = 0; q < a.hops; ++q)
            DGNN_REQUIRE(a.sizes[q] == -1 || a.sizes[q] >= 1, DGNN_E_INVALID, "khop_blocks_sampled: sizes[%d] = %d (-1 or > 0)", q, a.sizes[q]);
    }
    const int hops = a.hops;
    const int64_t* n_id = a.batch;
    int64_t n_t = a.n_batch;
    int rc = DGNN_OK;
    int h = 0;
    Mailbox mailbox;
    for (; h < hops; ++h) {
        const int keep = (a.sizes && a.sizes[h] >= 0 && a.sizes[h] < a.deg) ? a.sizes[h] : a.deg;   // in-edges per target of this hop
        const KhopDraw kd = keep == a.deg ? KHOP_EVERYTHING : khop_draw(keep, a.seed, a.draw, h);
        const int64_t n_e = n_t * keep;
        counts_out[h] = n_t;
        if (n_t > a.cap_t[h] || n_e > a.cap_e[h]) {
            dgnn_set_error("khop_blocks_regular: hop %d needs %lld targets / %lld edges, capacity %lld / %lld", h, (long long)n_t, (long long)n_e,
                           (long long)a.cap_t[h], (long long)a.cap_e[h]);
            rc = DGNN_E_INVALID;
            break;
        }
        if ((rc = khop_count("khop_count", kd, a.rowptr, n_id, n_t, h == 0, a.pos, a.off[h], a.scratch, stream)) != DGNN_OK) break;
        if ((rc = khop_expand("khop_expand", kd, a.rowptr, a.src, a.eid, n_id, n_t, a.off[h], n_e, a.pos, a.first, a.ei[h], a.ei[h] + a.cap_e[h], a.e_id[h],
                              a.n_id_out[h], a.n_new_dev, a.scratch, stream)) != DGNN_OK)
            break;
        int32_t n_new = 0;
        if (!read_back(a.n_new_dev, &n_new, mailbox, stream)) {
            dgnn_set_error("khop_blocks_regular: reading the new-node count failed: %s", hipGetErrorString(hipGetLastError()));
            rc = DGNN_E_LAUNCH;
            break;
        }
        const int64_t n_all = n_t + n_new;
        if ((rc = dgnn_khop_commit(a.n_id_out[h], n_t, n_all, a.pos, a.first, a.stream)) != DGNN_OK) break;
        if (n_e > 0)
            hipLaunchKernelGGL(k_i64_to_i32_x2, dim3(dgnn_grid_cap(dgnn_cdiv(n_e, 256))), dim3(256), 0, stream, a.ei[h], a.e_id[h], n_e, a.src32[h],
                               a.e_id32[h]);
        if (a.t_rowptr) {   // the block's source-sorted plan (what the backward pass walks) and the edge rows in its order
            if (n_all > a.cap_all[h]) {
                dgnn_set_error("khop_blocks_regular: hop %d reaches %lld nodes, capacity %lld", h, (long long)n_all, (long long)a.cap_all[h]);
                rc = DGNN_E_INVALID;
                n_id = a.n_id_out[h], n_t = n_all;
                ++h;
                break;
            }
            if ((rc = dgnn_plan_build(a.ei[h], a.cap_e[h], 1, n_e, n_all, n_t, 0, DGNN_PLAN_HINT_GENERIC, a.t_rowptr[h], a.t_dst[h], a.t_eid[h], a.plan_scratch,
                                      a.stream)) != DGNN_OK) {
                n_id = a.n_id_out[h], n_t = n_all;
                ++h;
                break;
            }
            if (n_e > 0)
                hipLaunchKernelGGL(k_take_i32, dim3(dgnn_grid_cap(dgnn_cdiv(n_e, 256))), dim3(256), 0, stream, a.e_id32[h], a.t_eid[h], n_e, a.t_rows[h]);
        }
        n_id = a.n_id_out[h];
        n_t = n_all;
    }
    if (h < hops) {
        for (int q = h + 1; q <= hops; ++q) counts_out[q] = 0;
    }
    counts_out[h < hops ? h : hops] = n_t;
    // pos[...] = -1 for everything this batch touched (also on the error paths: n_id / n_t describe what has been committed)
    const int rc2 = dgnn_khop_reset(n_id, n_t, a.pos, a.stream);
    if (rc != DGNN_OK) return rc;
    if (rc2 != DGNN_OK) return rc2;
    return dgnn_check_launch("khop_blocks_regular");
}

extern "C" int dgnn_khop_blocks_regular(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int deg, const int64_t* batch,
                                        int64_t n_batch, int hops, int32_t* pos, int32_t* first, int64_t* const* ei, int64_t* const* e_id,
                                        int32_t* const* src32, int32_t* const* e_id32, int32_t* const* off, int64_t* const* n_id_out, const int64_t* cap_t,
                                        const int64_t* cap_e, int32_t* scratch, int32_t* n_new_dev, int32_t* const* t_rowptr, int32_t* const* t_dst,
                                        int32_t* const* t_eid, int32_t* const* t_rows, const int64_t* cap_all, int32_t* plan_scratch,
                                        int64_t* counts_out, void* stream) {
    return khop_blocks({rowptr, src, eid, deg, batch, n_batch, hops, pos, first, ei, e_id, src32, e_id32, off, n_id_out, cap_t, cap_e, scratch, n_new_dev,
                        t_rowptr, t_dst, t_eid, t_rows, cap_all, plan_scratch, stream},
                       counts_out);
}

// ... with sampled neighbourhoods: sizes int32 [hops] (HOST; -1 or > 0), the loader's seed and the block's draw number
extern "C" int dgnn_khop_blocks_sampled(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int deg, const int64_t* batch,
                                        int64_t n_batch, int hops, const int32_t* sizes, uint64_t seed, int64_t draw, int32_t* pos, int32_t* first,
                                        int64_t* const* ei, int64_t* const* e_id, int32_t* const* src32, int32_t* const* e_id32, int32_t* const* off,
                                        int64_t* const* n_id_out, const int64_t* cap_t, const int64_t* cap_e, int32_t* scratch, int32_t* n_new_dev,
                                        int32_t* const* t_rowptr, int32_t* const* t_dst, int32_t* const* t_eid, int32_t* const* t_rows,
                                        const int64_t* cap_all, int32_t* plan_scratch, int64_t* counts_out, void* stream) {
    DGNN_REQUIRE(sizes, DGNN_E_INVALID, "khop_blocks_sampled: sizes is NULL");
    return khop_blocks({rowptr, src, eid, deg, batch, n_batch, hops, pos, first, ei, e_id, src32, e_id32, off, n_id_out, cap_t, cap_e, scratch, n_new_dev,
                        t_rowptr, t_dst, t_eid, t_rows, cap_all, plan_scratch, stream, sizes, seed, draw},
                       counts_out);
}

// ---- the same call on a library-owned host thread ------------------------------------------------------------------------------
// start() returns at once; a std::thread (no interpreter lock involved) issues the launches on `stream` and waits for the per-hop
// counts; wait() joins it.  The caller keeps enqueueing the training step on its own stream meanwhile and must not touch
// `stream`, `pos`, `first` or the output buffers between start() and wait().
#include <string>
#include <thread>
#include <vector>

namespace {
struct KhopJob {
    std::thread th;
    int rc = DGNN_OK;
    std::string err;
    KhopBlocks a;   // the caller's arguments, their per-hop arrays (the caller's may go once start() has returned) redirected to the copies below
    std::vector<int64_t*> ei, e_id, n_id_out;
    std::vector<int32_t*> src32, e_id32, off, t_rowptr, t_dst, t_eid, t_rows;
    std::vector<int64_t> cap_t, cap_e, cap_all, counts;
    std::vector<int32_t> sizes;
};
template <typename T>
void own(const T*& field, std::vector<T>& copy, int n) {   // a NULL array stays NULL
    if (!field) return;
    copy.assign(field, field + n);
    field = copy.data();
}
// rows of a block gathered by the builder itself (round 4): out[i, 0:cols] = src[idx[i] * ld + 0:cols] for the block's node ids
// (which = 0: all nodes of the outermost block) or its targets (which = 1) -- the head-of-step x_all[n_id, 1:], x_all[ids], y_all[ids] of the
// training loop (learning/surfaceNetStaticEdgeFilters.py:206, learning/runModel.py:273-274), 30 us of torch indexing kernels on the step's own
// stream, now behind the block on the builder's stream a step ahead
struct KhopRows {
    int n = 0;
    const float* src[4];
    int64_t ld[4];
    int cols[4], which[4];
    float* out[4];
};
__global__ void k_gather_rows_i64(const float* __restrict__ src, int64_t ld, const int64_t* __restrict__ idx, int64_t n, int cols, float* __restrict__ out) {
    const int64_t total = n * cols;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = t / cols;
        const int c = (int)(t - r * cols);
        out[t] = src[idx[r] * ld + c];
    }
}
}  // namespace

static void* khop_start(const KhopBlocks& args, KhopRows rows) {
    const int hops = args.hops;
    if (hops < 1 || hops > 16 || !args.ei || !args.e_id || !args.src32 || !args.e_id32 || !args.off || !args.n_id_out || !args.cap_t || !args.cap_e) {
        dgnn_set_error("khop_blocks_regular_start: bad args");
        return nullptr;
    }
    int device = 0;
    (void)hipGetDevice(&device);
    KhopJob* j = new KhopJob();
    KhopBlocks& a = j->a = args;
    own(a.ei, j->ei, hops), own(a.e_id, j->e_id, hops), own(a.n_id_out, j->n_id_out, hops);
    own(a.src32, j->src32, hops), own(a.e_id32, j->e_id32, hops), own(a.off, j->off, hops);
    own(a.t_rowptr, j->t_rowptr, hops), own(a.t_dst, j->t_dst, hops), own(a.t_eid, j->t_eid, hops), own(a.t_rows, j->t_rows, hops);
    own(a.cap_t, j->cap_t, hops), own(a.cap_e, j->cap_e, hops), own(a.cap_all, j->cap_all, hops), own(a.sizes, j->sizes, hops);
    j->counts.assign(hops + 1, 0);
    j->th = std::thread([j, device, rows]() {
        const KhopBlocks& a = j->a;
        const int hops = a.hops;
        if (hipSetDevice(device) != hipSuccess) {
            j->rc = DGNN_E_LAUNCH;
            j->err = "khop_blocks_regular_start: hipSetDevice failed on the builder thread";
            return;
        }
        j->rc = khop_blocks(a, j->counts.data());
        if (j->rc != DGNN_OK) {
            j->err = dgnn_last_error_string();   // the error text is per thread: carry it over
            return;
        }
        for (int i = 0; i < rows.n; ++i) {       // the block's feature / label rows, behind the block on the builder's stream
            const int64_t n = rows.which[i] ? a.n_batch : j->counts[hops];
            const int64_t* idx = rows.which[i] ? a.batch : a.n_id_out[hops - 1];
            if (n <= 0) continue;
            hipLaunchKernelGGL(k_gather_rows_i64, dim3(dgnn_grid_cap(dgnn_cdiv(n * rows.cols[i], 256))), dim3(256), 0, (hipStream_t)a.stream, rows.src[i], rows.ld[i],
                               idx, n, rows.cols[i], rows.out[i]);
        }
        if (rows.n) {
            j->rc = dgnn_check_launch("khop_blocks_regular_start_rows");
            if (j->rc != DGNN_OK) j->err = dgnn_last_error_string();
        }
    });
    return j;
}

extern "C" void* dgnn_khop_blocks_regular_start(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int deg, const int64_t* batch,
                                                int64_t n_batch, int hops, int32_t* pos, int32_t* first, int64_t* const* ei, int64_t* const* e_id,
                                                int32_t* const* src32, int32_t* const* e_id32, int32_t* const* off, int64_t* const* n_id_out,
                                                const int64_t* cap_t, const int64_t* cap_e, int32_t* scratch, int32_t* n_new_dev,
                                                int32_t* const* t_rowptr, int32_t* const* t_dst, int32_t* const* t_eid, int32_t* const* t_rows,
                                                const int64_t* cap_all, int32_t* plan_scratch, void* stream) {
    return khop_start({rowptr, src, eid, deg, batch, n_batch, hops, pos, first, ei, e_id, src32, e_id32, off, n_id_out, cap_t, cap_e, scratch, n_new_dev,
                       t_rowptr, t_dst, t_eid, t_rows, cap_all, plan_scratch, stream},
                      KhopRows());
}

// ... and up to 4 row gathers behind the block: r_src[i] (fp32, already offset to its first column), row stride r_ld[i], r_cols[i] columns, r_which[i]
// 0 = all nodes of the outermost block (n_id_out[hops-1][:counts[hops]]) / 1 = the batch's targets, r_out[i] [capacity, r_cols[i]] packed rows
static bool khop_rows(KhopRows& rows, int n_rows, const float* const* r_src, const int64_t* r_ld, const int32_t* r_cols, const int32_t* r_which,
                      float* const* r_out) {
    if (n_rows < 0 || n_rows > 4 || (n_rows && !(r_src && r_ld && r_cols && r_which && r_out))) {
        dgnn_set_error("khop_blocks_regular_start_rows: at most 4 row gathers, all arrays given");
        return false;
    }
    rows.n = n_rows;
    for (int i = 0; i < n_rows; ++i) {
        if (!r_src[i] || !r_out[i] || r_cols[i] <= 0 || r_ld[i] < r_cols[i]) {
            dgnn_set_error("khop_blocks_regular_start_rows: bad row gather %d", i);
            return false;
        }
        rows.src[i] = r_src[i], rows.ld[i] = r_ld[i], rows.cols[i] = r_cols[i], rows.which[i] = r_which[i], rows.out[i] = r_out[i];
    }
    return true;
}

extern "C" void* dgnn_khop_blocks_regular_start_rows(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int deg, const int64_t* batch,
                                                     int64_t n_batch, int hops, int32_t* pos, int32_t* first, int64_t* const* ei, int64_t* const* e_id,
                                                     int32_t* const* src32, int32_t* const* e_id32, int32_t* const* off, int64_t* const* n_id_out,
                                                     const int64_t* cap_t, const int64_t* cap_e, int32_t* scratch, int32_t* n_new_dev,
                                                     int32_t* const* t_rowptr, int32_t* const* t_dst, int32_t* const* t_eid, int32_t* const* t_rows,
                                                     const int64_t* cap_all, int32_t* plan_scratch, int n_rows, const float* const* r_src, const int64_t* r_ld,
                                                     const int32_t* r_cols, const int32_t* r_which, float* const* r_out, void* stream) {
    KhopRows rows;
    if (!khop_rows(rows, n_rows, r_src, r_ld, r_cols, r_which, r_out)) return nullptr;
    return khop_start({rowptr, src, eid, deg, batch, n_batch, hops, pos, first, ei, e_id, src32, e_id32, off, n_id_out, cap_t, cap_e, scratch, n_new_dev,
                       t_rowptr, t_dst, t_eid, t_rows, cap_all, plan_scratch, stream},
                      rows);
}

// The sampled builder on the library-owned host thread, without and with the row gathers; dgnn_khop_blocks_regular_wait joins either.
extern "C" void* dgnn_khop_blocks_sampled_start(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int deg, const int64_t* batch,
                                                int64_t n_batch, int hops, const int32_t* sizes, uint64_t seed, int64_t draw, int32_t* pos, int32_t* first,
                                                int64_t* const* ei, int64_t* const* e_id, int32_t* const* src32, int32_t* const* e_id32, int32_t* const* off,
                                                int64_t* const* n_id_out, const int64_t* cap_t, const int64_t* cap_e, int32_t* scratch, int32_t* n_new_dev,
                                                int32_t* const* t_rowptr, int32_t* const* t_dst, int32_t* const* t_eid, int32_t* const* t_rows,
                                                const int64_t* cap_all, int32_t* plan_scratch, void* stream) {
    if (!sizes) {
        dgnn_set_error("khop_blocks_sampled_start: sizes is NULL");
        return nullptr;
    }
    return khop_start({rowptr, src, eid, deg, batch, n_batch, hops, pos, first, ei, e_id, src32, e_id32, off, n_id_out, cap_t, cap_e, scratch, n_new_dev,
                       t_rowptr, t_dst, t_eid, t_rows, cap_all, plan_scratch, stream, sizes, seed, draw},
                      KhopRows());
}

extern "C" void* dgnn_khop_blocks_sampled_start_rows(const int32_t* rowptr, const int32_t* src, const int32_t* eid, int deg, const int64_t* batch,
                                                     int64_t n_batch, int hops, const int32_t* sizes, uint64_t seed, int64_t draw, int32_t* pos,
                                                     int32_t* first, int64_t* const* ei, int64_t* const* e_id, int32_t* const* src32, int32_t* const* e_id32,
                                                     int32_t* const* off, int64_t* const* n_id_out, const int64_t* cap_t, const int64_t* cap_e,
                                                     int32_t* scratch, int32_t* n_new_dev, int32_t* const* t_rowptr, int32_t* const* t_dst,
                                                     int32_t* const* t_eid, int32_t* const* t_rows, const int64_t* cap_all, int32_t* plan_scratch, int n_rows,
                                                     const float* const* r_src, const int64_t* r_ld, const int32_t* r_cols, const int32_t* r_which,
                                                     float* const* r_out, void* stream) {
    KhopRows rows;
    if (!sizes) {
        dgnn_set_error("khop_blocks_sampled_start_rows: sizes is NULL");
        return nullptr;
    }
    if (!khop_rows(rows, n_rows, r_src, r_ld, r_cols, r_which, r_out)) return nullptr;
    return khop_start({rowptr, src, eid, deg, batch, n_batch, hops, pos, first, ei, e_id, src32, e_id32, off, n_id_out, cap_t, cap_e, scratch, n_new_dev,
                       t_rowptr, t_dst, t_eid, t_rows, cap_all, plan_scratch, stream, sizes, seed, draw},
                      rows);
}

extern "C" int dgnn_khop_blocks_regular_wait(void* job, int hops, int64_t* counts_out) {
    DGNN_REQUIRE(job && counts_out, DGNN_E_INVALID, "khop_blocks_regular_wait: bad args");
    KhopJob* j = reinterpret_cast<KhopJob*>(job);
    if (j->th.joinable()) j->th.join();
    const int rc = j->rc;
    for (int h = 0; h <= hops && h < (int)j->counts.size(); ++h) counts_out[h] = j->counts[h];
    if (rc != DGNN_OK) dgnn_set_error("%s", j->err.c_str());
    delete j;
    return rc;
}
