// The batch-graph builders ON THE DEVICE: what builder_both.hip (the merged training batch), builder_full.hip (the global
// model's full-graph batches), builder_grouped.hip (the grouped batches of batched inference) and builder_tail.hip
// (everything behind the edge list, and the kernels more than one front launches) share.  Every builder derives what the host
// builder (graph.py + host_builder.cpp) derives from a batch of indices, as kernels over data that is RESIDENT in HBM;
// nothing is synchronised in between: every stage launches over a capacity and guards on device-side counts.  Output = the
// arrays of graph.HostBatch, bit for bit.  Integer / index work: rocPRIM radix sorts and scans + small hand-written
// kernels; HBM-bound, no MFMA.
// Device helpers, the kernels' Store pack and the entries' small host helpers sit in the anonymous namespace of the
// including translation unit (every kernel lives in exactly one file).  The scratch structs and the host functions of
// builder_tail.hip cross translation units: library-internal (hidden visibility).  rocPRIM is instantiated in
// builder_tail.hip only; a front reaches its scans and sorts through scan_plus / scan_max / sort_pairs / sort_keys.
#pragma once
#include "common.h"

#define RENET_BB_HIDDEN __attribute__((visibility("hidden")))      // what crosses translation units is library-internal

struct RENET_BB_HIDDEN Carver {
    char* p; size_t left; size_t used = 0; bool ok = true;
    template <class T> T* take(size_t n) {
        const size_t bytes = (n * sizeof(T) + 255) & ~(size_t)255;
        used += bytes;
        if (bytes > left) { ok = false; left = 0; return nullptr; }
        T* r = reinterpret_cast<T*>(p);
        p += bytes; left -= bytes;
        return r;
    }
};

namespace {

constexpr int BB_MAXQ = 4096;          // sequences per batch (2 B)
constexpr int BB_MAXL = 32;            // history steps per sequence

// ---- block-wide exclusive scan (1024 threads) ----------------------------------------------------------------
__device__ __forceinline__ int block_excl_scan_1024(int v, int* total, int* wsum /* [16] LDS */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    __syncthreads();                                   // wsum may still be read by the previous call
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        const int s = wsum[w];
        if (w < wave) base += s;
        tot += s;
    }
    *total = tot;
    return base + inc - v;
}

struct Store {
    const int32_t *q_s, *q_r, *q_o;
    const int32_t* h_first[2];
    const int32_t* h_count[2];
    const int32_t* snap_t[2];
    const int32_t* snap_ptr[2];
    const int32_t* nbr_o[2];
    const int32_t* times;
    const int32_t* trip_ptr;
    const int32_t *trip_s, *trip_r, *trip_o;
    const int32_t* glob_times;
    int T, n_glob, num_ent, num_rels;
};

__device__ __forceinline__ int lower_bound_i32(const int32_t* a, int n, int v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

inline int bits_for(uint64_t v) { int b = 1; while (b < 63 && (1ull << b) <= v) ++b; return b; }

#define BB_HIP(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return (int)e__; } while (0)

// the fields of Store that both resident stores (RenetStoreDev, RenetGroupedStoreDev) name alike, and the quadruples; the
// five history-index arrays (h_first, h_count, snap_t, snap_ptr, nbr_o) are the entry's own
template <class SD>
Store fill_store(const SD* sd, const int32_t* q_s, const int32_t* q_r, const int32_t* q_o) {
    Store S;
    S.q_s = q_s; S.q_r = q_r; S.q_o = q_o;
    S.times = sd->times; S.trip_ptr = sd->trip_ptr; S.trip_s = sd->trip_s; S.trip_r = sd->trip_r; S.trip_o = sd->trip_o;
    S.glob_times = sd->glob_times; S.T = sd->T; S.n_glob = sd->n_glob; S.num_ent = sd->num_ent; S.num_rels = sd->num_rels;
    return S;
}

// what every build entry refuses as unsupported BEFORE its workspace check; gives T2 = 2 * num_rels and the (dst, type) key's bits
inline int check_common(int num_rels, int T, int heavy_thr, int group_budget, int chunk, int cap_nodes, int* T2, int* key_bits) {
    if (2 * num_rels > 1024 || T <= 0 || group_budget + heavy_thr + 1 > 64 || chunk <= 0) return RENET_ERR_UNSUPPORTED;
    *T2 = 2 * num_rels;
    *key_bits = bits_for((uint64_t)cap_nodes * *T2);
    return RENET_OK;
}

// bytes that BufsT::carve(cv, a...) takes: a dry run over a Carver that is never dereferenced
template <class BufsT, class... A>
size_t workspace_of(A... a) {
    Carver dry{reinterpret_cast<char*>(256), ~(size_t)0 >> 2};
    BufsT().carve(dry, a...);
    return dry.used + 256;
}

}  // namespace

// scratch of the shared tail (build_tail): everything from the edge list (src, dst, et, the sort keys, the in-degree and
// relation histograms) to the outputs.  `pruned` = the batch has a row prefix [0, nA) with layouts of its own.
struct RENET_BB_HIDDEN TailBufs {
    int32_t *src, *dst, *et;
    uint32_t *key_dt, *key_t, *key_t2, *key_sorted;
    int32_t *iota, *ord_dt, *ord_t, *ord_t2, *deg;
    int32_t *tc, *tc2;             // relation histograms [1024]; pruned: one block, tc2 = tc + 1024 the row prefix's, else nullptr
    int32_t *heavy_flag, *heavy_pos, *item_cnt, *item_start, *light_id, *prev_light;
    int32_t *first_flag, *first_pos, *first_out, *first_out_pos;
    uint32_t* pkey;
    int32_t *pflag, *ppos;
    void* tmp;                     // rocPRIM scratch of the scans and the 32-bit key sorts
    size_t tmp_bytes;
    bool carve_tail(Carver& cv, int cap_nodes, int cap_edges, int cap_steps, int cap_facts, bool pruned);
    size_t tc_bytes() const { return (tc2 ? 2048 : 1024) * sizeof(int32_t); }      // what an entry zeroes
};

// + the sequence / step scratch and the half edges of the fronts that start from sequences (merged, grouped)
struct RENET_BB_HIDDEN SeqBufs : TailBufs {
    int32_t *seq_first, *seq_len_s, *seq_start;
    int32_t *step_snap, *step_dense, *step_packed, *slot_used;
    int32_t *half_src, *half_dst, *half_et;
};

// ---- builder_tail.hip.  rocPRIM on the scratch of bf: exclusive scans of n ints (plus from 0; maximum from -1), the stable
// sort of n (key, bf.iota) pairs by the low `bits` key bits (keys -> bf.key_sorted); sort_keys: n 64-bit keys, rocPRIM's own
// protocol (tmp = nullptr: only sets tmp_bytes, else leaves it alone).  The status goes through BB_HIP.
RENET_BB_HIDDEN hipError_t scan_plus(const TailBufs& bf, int32_t* in, int32_t* out, size_t n, hipStream_t st);
RENET_BB_HIDDEN hipError_t scan_max(const TailBufs& bf, int32_t* in, int32_t* out, size_t n, hipStream_t st);
RENET_BB_HIDDEN hipError_t sort_pairs(const TailBufs& bf, uint32_t* keys, int32_t* vals_out, size_t n, int bits, hipStream_t st);
RENET_BB_HIDDEN hipError_t sort_keys(void* tmp, size_t& tmp_bytes, uint64_t* in, uint64_t* out, size_t n, int bits, hipStream_t st);
// stages A, B over Q sequences; S: the entry's Store (a type of the anonymous namespace cannot cross in a signature)
RENET_BB_HIDDEN int launch_seq_steps(const void* S, const int32_t* idx, int B, int Q, int seq_len, const RenetBatchOut* out,
                                     const SeqBufs& bf, int32_t* rel_label, int32_t* ent_label, hipStream_t st);
// pos = exclusive scan of flag[0 .. cap), then E2 = total of flag[0 .. *n_ptr) (bb_set_e2_kernel)
RENET_BB_HIDDEN int scan_set_e2(const TailBufs& bf, int32_t* flag, int32_t* pos, int32_t* counts, const int32_t* n_ptr, int cap,
                                int cap_edges, hipStream_t st);
// stages F, G, H behind the edge list; finish_batch: bb_expand_kernel first, all four plans, bb_finish_kernel last
RENET_BB_HIDDEN int build_tail(const TailBufs& bf, const RenetBatchOut* out, int cap_nodes, int cap_edges, int cap_steps,
                               int num_ent, int T2, int key_bits, int heavy_thr, int group_budget, int chunk, int n_plans,
                               int n_seq, bool pruned, hipStream_t st);
RENET_BB_HIDDEN int finish_batch(const SeqBufs& bf, const RenetBatchOut* out, int cap_nodes, int cap_edges, int cap_steps,
                                 int num_ent, int num_rels, int key_bits, int heavy_thr, int group_budget, int chunk, int n_seq,
                                 hipStream_t st);
