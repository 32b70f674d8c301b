// Batch-graph builder ON THE DEVICE for the GROUPED inference batches (graph.build_batch(..., group=...);
// RGCNAggregator.forward_grouped): the front of renet_build_batch_grouped.  One direction of B sequences, a member graph
// (slot) per (group, timestamp) pair.  Thousands of slots: no [slot][entity] table (slot * num_ent passes 2^31) -- slots and
// node sets are numbered by sorting 64-bit keys, membership is a binary search in the sorted keys, and the induced edges
// walk the store's per-timestamp subject index from every node (graph._induced_edges(sparse=True)).  Stages A / B are
// bb_seq_kernel (Q = B) and bb_steps_kernel; everything behind the half edges is bb_expand_kernel + build_tail, shared
// with renet_build_batch_both (builder_tail.hip).  tests/test_gpu_grouped_builder.py compares every array with the host
// builder's.
#include "builder_common.h"

namespace {

struct GroupedStore {
    const int32_t* group;
    const int32_t* snap_ptr;
    const int32_t* nbr_o;
    const int32_t* trip_ptr;
    const int32_t *trip_s, *trip_r, *trip_o;
    const int32_t *by_subj, *subj_sorted;
    int n_steps, n_nbr, n_facts;
};

constexpr uint64_t GB_NONE = ~0ull;                        // sentinel key: sorted behind every valid key

__device__ __forceinline__ int lower_bound_u64(const uint64_t* a, int n, uint64_t v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// S as the grouped stages see it: 0 after a bad timestamp (bb_steps_kernel then left step arrays unwritten)
__device__ __forceinline__ int gb_steps(const int32_t* counts) {
    return (counts[RENET_BB_ERR] & (RENET_BB_ERR_TIME | RENET_BB_ERR_GLOB)) ? 0 : counts[RENET_BB_S];
}

// row of node (slot, entity) in the batch, -1 if it is not a node: ukey = the N sorted unique keys, uid their rows
__device__ __forceinline__ int gb_row_of(const uint64_t* ukey, const int32_t* uid, int N, uint64_t key) {
    const int u = lower_bound_u64(ukey, N, key);
    return (u < N && ukey[u] == key) ? uid[u] : -1;
}

// ---- grouped stage C: slots.  Key of step k = (group << 32) | timestamp index; thread per (sorted sequence i, step j) ----
__global__ __launch_bounds__(256) void gb_slot_keys_kernel(GroupedStore gs, const int32_t* __restrict__ counts,
                                                           const int32_t* __restrict__ perm,
                                                           const int32_t* __restrict__ seq_len_s,
                                                           const int32_t* __restrict__ seq_start,
                                                           const int32_t* __restrict__ step_dense,
                                                           uint64_t* __restrict__ gkey) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = t / BB_MAXL, j = t - i * BB_MAXL;
    if (gb_steps(counts) == 0 || i >= counts[RENET_BB_NNZ] || j >= seq_len_s[i]) return;
    const int k = seq_start[i] + j;
    gkey[k] = ((uint64_t)(uint32_t)gs.group[perm[i]] << 32) | (uint32_t)step_dense[k];
}

// first-of-run flags of a sorted key array (sentinels are no keys); shift = 1 drops the neighbour bit of the node keys.
// fb (node keys only): the run has no subject key, i.e. its first key carries the neighbour bit.
__global__ __launch_bounds__(256) void gb_run_flags_kernel(const uint64_t* __restrict__ skey, int cap, int shift,
                                                           int32_t* __restrict__ fa, int32_t* __restrict__ fb) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap) return;
    const uint64_t k = skey[i];
    const bool first = k != GB_NONE && (i == 0 || (k >> shift) != (skey[i - 1] >> shift));
    const bool nbr = shift && (k & 1);
    fa[i] = first && !nbr;
    if (fb) fb[i] = first && nbr;
}

__global__ __launch_bounds__(256) void gb_slots_kernel(const uint64_t* __restrict__ skey, int cap,
                                                       const int32_t* __restrict__ flag, const int32_t* __restrict__ pos,
                                                       uint64_t* __restrict__ slot_key, int32_t* __restrict__ slot_ti,
                                                       int32_t* __restrict__ counts) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap) return;
    if (flag[i]) { slot_key[pos[i]] = skey[i]; slot_ti[pos[i]] = (int32_t)(uint32_t)skey[i]; }
    if (i == cap - 1) counts[RENET_BB_TB] = pos[i] + flag[i];
}

// ---- grouped stage D: node keys ((slot << 32 | entity) << 1) | neighbour bit.  One WAVE per step: lane 0 the subject (at
// the step's own position), the lanes the neighbours (behind the steps, at the neighbour's position): no scan, every key
// has a place of its own and the unused places keep the sentinel.
__global__ __launch_bounds__(256) void gb_node_keys_kernel(GroupedStore gs, const int32_t* __restrict__ counts,
                                                           const int32_t* __restrict__ step_snap,
                                                           const int32_t* __restrict__ step_packed,
                                                           const int32_t* __restrict__ row_ent,
                                                           const uint64_t* __restrict__ gkey,
                                                           const uint64_t* __restrict__ slot_key,
                                                           int32_t* __restrict__ slot_k, uint64_t* __restrict__ nkey) {
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= gb_steps(counts)) return;
    const int lane = threadIdx.x & 63;
    const int snap = step_snap[k] & 0x3FFFFFFF;
    if (snap >= gs.n_steps) return;
    const uint64_t slot = (uint64_t)lower_bound_u64(slot_key, counts[RENET_BB_TB], gkey[k]);
    if (lane == 0) {
        slot_k[k] = (int)slot;
        nkey[snap] = ((slot << 32) | (uint32_t)row_ent[step_packed[k]]) << 1;
    }
    const int b = gs.snap_ptr[snap], e = min(gs.snap_ptr[snap + 1], gs.n_nbr);
    for (int n = b + lane; n < e; n += 64) nkey[(size_t)gs.n_steps + n] = (((slot << 32) | (uint32_t)gs.nbr_o[n]) << 1) | 1;
}

// ---- grouped stage E: numbering: subject keys first (in key order), then the others (in key order) ------------------
__global__ void gb_node_count_kernel(const int32_t* __restrict__ fa, const int32_t* __restrict__ pa,
                                     const int32_t* __restrict__ fb, const int32_t* __restrict__ pb, int cap, int cap_nodes,
                                     int32_t* __restrict__ counts) {
    const int nA = pa[cap - 1] + fa[cap - 1], nB = pb[cap - 1] + fb[cap - 1];
    const bool over = (long long)nA + nB > cap_nodes;
    if (over) atomicOr(&counts[RENET_BB_ERR], RENET_BB_ERR_NODES);  // every later stage then sees an EMPTY graph (no OOB access)
    counts[RENET_BB_NA] = over ? 0 : nA;
    counts[RENET_BB_N] = over ? 0 : nA + nB;
}

__global__ __launch_bounds__(256) void gb_number_kernel(const uint64_t* __restrict__ skey, int cap,
                                                        const int32_t* __restrict__ fa, const int32_t* __restrict__ pa,
                                                        const int32_t* __restrict__ fb, const int32_t* __restrict__ pb,
                                                        const int32_t* __restrict__ counts, uint64_t* __restrict__ ukey,
                                                        int32_t* __restrict__ uid, int32_t* __restrict__ node_ent,
                                                        int32_t* __restrict__ node_slot) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap || !(fa[i] | fb[i])) return;
    const int N = counts[RENET_BB_N], nA = counts[RENET_BB_NA];
    const int u = pa[i] + pb[i], id = fa[i] ? pa[i] : nA + pb[i];
    if (u >= N || id >= N) return;                          // (N = 0 after an overflow)
    const uint64_t key = skey[i] >> 1;
    ukey[u] = key;
    uid[u] = id;
    node_ent[id] = (int32_t)(uint32_t)key;
    node_slot[id] = (int32_t)(key >> 32);
}

// subject row of every step, in packed order
__global__ __launch_bounds__(256) void gb_subj_row_kernel(const int32_t* __restrict__ counts,
                                                          const int32_t* __restrict__ step_packed,
                                                          const int32_t* __restrict__ row_ent,
                                                          const int32_t* __restrict__ slot_k,
                                                          const uint64_t* __restrict__ ukey, const int32_t* __restrict__ uid,
                                                          int32_t* __restrict__ subj_row) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = counts[RENET_BB_N];
    if (k >= gb_steps(counts) || N == 0) return;
    const int p = step_packed[k];
    subj_row[p] = max(gb_row_of(ukey, uid, N, ((uint64_t)slot_k[k] << 32) | (uint32_t)row_ent[p]), 0);
}

// ---- grouped stage F: induced edges, sparse.  Thread per node (slot, e): the facts of the slot's timestamp with subject e
// (a range of the subject index) whose object is a node of the slot.  emit = 0: counts them; emit = 1: writes their keys
// (slot << 32) | fact behind the node's scanned offset.  Sorting those keys restores the host's order: slot-major, and
// inside a slot the store's fact order.
__global__ __launch_bounds__(256) void gb_node_facts_kernel(GroupedStore gs, const int32_t* __restrict__ counts, int cap_nodes,
                                                            const uint64_t* __restrict__ ukey,
                                                            const int32_t* __restrict__ slot_ti, int emit,
                                                            int32_t* __restrict__ ecnt, const int32_t* __restrict__ epos,
                                                            uint64_t* __restrict__ fkey) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= cap_nodes) return;
    const int N = counts[RENET_BB_N];
    int c = 0;
    if (u < N && (!emit || counts[RENET_BB_E2] > 0)) {
        const uint64_t key = ukey[u], slot = key >> 32;
        const int ent = (int)(uint32_t)key, ti = slot_ti[slot];
        const int b = gs.trip_ptr[ti], e = min(gs.trip_ptr[ti + 1], gs.n_facts);
        const int lim = emit ? counts[RENET_BB_E2] : 0, at = emit ? epos[u] : 0;
        for (int q = b + lower_bound_i32(gs.subj_sorted + b, e - b, ent); q < e && gs.subj_sorted[q] == ent; ++q) {
            const int j = gs.by_subj[q];
            if ((unsigned)j >= (unsigned)gs.n_facts) continue;      // (the index is range-checked on the host; never index past it)
            const uint64_t ko = (slot << 32) | (uint32_t)gs.trip_o[j];
            const int v = lower_bound_u64(ukey, N, ko);
            if (v >= N || ukey[v] != ko) continue;
            if (emit && at + c < lim) fkey[at + c] = (slot << 32) | (uint32_t)j;
            ++c;
        }
    }
    if (!emit) ecnt[u] = c;
}

// the half edges of the sorted fact keys: local subject row -> local object row, type r (type_s: the direction is the
// kernels' type_shift)
__global__ __launch_bounds__(256) void gb_half_edges_kernel(GroupedStore gs, const int32_t* __restrict__ counts,
                                                            const uint64_t* __restrict__ fkey_sorted,
                                                            const uint64_t* __restrict__ ukey, const int32_t* __restrict__ uid,
                                                            int32_t* __restrict__ half_src, int32_t* __restrict__ half_dst,
                                                            int32_t* __restrict__ half_et) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= counts[RENET_BB_E2]) return;
    const int N = counts[RENET_BB_N];
    const uint64_t k = fkey_sorted[m], slot = k >> 32;
    const int j = (int)(uint32_t)k;
    half_src[m] = max(gb_row_of(ukey, uid, N, (slot << 32) | (uint32_t)gs.trip_s[j]), 0);
    half_dst[m] = max(gb_row_of(ukey, uid, N, (slot << 32) | (uint32_t)gs.trip_o[j]), 0);
    half_et[m] = gs.trip_r[j];
}

// scratch of the grouped front + the tail
struct GroupedBufs : SeqBufs {
    int32_t* rel_label;            // (bb_seq_kernel writes labels; a grouped batch has none)
    int32_t* ent_label;
    uint64_t* gkey;                // [cap_steps] slot key of every step
    uint64_t* slot_key;            // [cap_steps] the Tb unique slot keys, sorted
    int32_t* slot_ti;
    int32_t* slot_k;               // [cap_steps] slot of every step
    uint64_t* nkey;                // [cap_keys] node keys, a place per step and per neighbour
    uint64_t* skey;                // [max(cap_keys, cap_steps, cap_edges / 2)] sorted keys of the sort at hand
    uint64_t* ukey;                // [cap_keys] the N unique node keys, sorted
    int32_t* uid;                  // [cap_keys] their rows
    int32_t* fa;                   // [cap_scan] flags / counts and their scans
    int32_t* pa;
    int32_t* fb;
    int32_t* pb;
    uint64_t* fkey;                // [cap_edges / 2] keys of the kept facts
    void* tmp64;                   // rocPRIM scratch of the 64-bit key sorts
    size_t tmp64_bytes;
    static int cap_keys(const RenetGroupedStoreDev* sd) { return max(sd->n_steps, 0) + max(sd->n_nbr, 0) + 1; }
    bool carve(Carver& cv, const RenetGroupedStoreDev* sd, int B, int cap_nodes, int cap_edges) {
        const int cap_steps = B * BB_MAXL, ck = cap_keys(sd), ce2 = max(cap_edges / 2, 1);
        const int cap_sort = max(max(ck, cap_steps), ce2), cap_scan = max(max(ck, cap_steps), cap_nodes) + 2;
        seq_first = cv.take<int32_t>(BB_MAXQ); seq_len_s = cv.take<int32_t>(BB_MAXQ); seq_start = cv.take<int32_t>(BB_MAXQ);
        rel_label = cv.take<int32_t>(BB_MAXQ);
        ent_label = cv.take<int32_t>(BB_MAXQ);
        step_snap = cv.take<int32_t>(cap_steps); step_dense = cv.take<int32_t>(cap_steps);
        step_packed = cv.take<int32_t>(cap_steps); slot_used = cv.take<int32_t>(2 * sd->T + 2);
        gkey = cv.take<uint64_t>(cap_steps);
        slot_key = cv.take<uint64_t>(cap_steps);
        slot_ti = cv.take<int32_t>(cap_steps);
        slot_k = cv.take<int32_t>(cap_steps);
        nkey = cv.take<uint64_t>(ck);
        skey = cv.take<uint64_t>(cap_sort);
        ukey = cv.take<uint64_t>(ck);
        uid = cv.take<int32_t>(ck);
        fa = cv.take<int32_t>(cap_scan);
        pa = cv.take<int32_t>(cap_scan);
        fb = cv.take<int32_t>(cap_scan);
        pb = cv.take<int32_t>(cap_scan);
        fkey = cv.take<uint64_t>(ce2);
        half_src = cv.take<int32_t>(ce2); half_dst = cv.take<int32_t>(ce2); half_et = cv.take<int32_t>(ce2);
        (void)sort_keys(nullptr, tmp64_bytes, nullptr, nullptr, (size_t)cap_sort, 64, nullptr);       // (the size only)
        tmp64_bytes = (tmp64_bytes + 255) & ~(size_t)255;
        tmp64 = cv.take<char>(tmp64_bytes);
        return carve_tail(cv, cap_nodes, cap_edges, cap_steps, cap_scan, true) && tmp64 != nullptr;
    }
};

}  // namespace

extern "C" {

size_t renet_build_batch_grouped_workspace(const RenetGroupedStoreDev* sd, int B, int cap_nodes, int cap_edges) {
    if (!sd || B <= 0 || B > BB_MAXQ || cap_nodes <= 0 || cap_edges < 2 || sd->T <= 0 || sd->n_steps < 0 || sd->n_nbr < 0) return 0;
    return workspace_of<GroupedBufs>(sd, B, cap_nodes, cap_edges & ~1);
}

int renet_build_batch_grouped(const RenetGroupedStoreDev* sd, const int32_t* idx_dev, int B, int seq_len, int heavy_thr,
                              int group_budget, int chunk, const RenetBatchOut* out, void* workspace,
                              size_t workspace_bytes, void* stream) {
    if (!sd || !out || B <= 0 || B > BB_MAXQ || seq_len <= 0 || seq_len > BB_MAXL || sd->n_steps < 0 || sd->n_nbr < 0 ||
        sd->n_facts < 0 || out->cap_nodes <= 0 || out->cap_edges < 2)
        return RENET_ERR_BADARG;
    const int cap_nodes = out->cap_nodes, cap_edges = out->cap_edges & ~1, ce2 = cap_edges / 2;
    int T2, key_bits;
    if (sd->num_rels <= 0 || (long long)sd->n_steps + sd->n_nbr >= (1ll << 30) ||
        check_common(sd->num_rels, sd->T, heavy_thr, group_budget, chunk, cap_nodes, &T2, &key_bits))
        return RENET_ERR_UNSUPPORTED;
    if (workspace_bytes < renet_build_batch_grouped_workspace(sd, B, out->cap_nodes, out->cap_edges)) return RENET_ERR_WORKSPACE;
    if ((uint64_t)cap_nodes * T2 >= (1ull << 31)) return RENET_ERR_UNSUPPORTED;      // the (dst, type) sort keys are 32 bits
    hipStream_t st = (hipStream_t)stream;
    // the batch's own arrays as the one-role history index that bb_seq_kernel / bb_steps_kernel read
    Store S = fill_store(sd, sd->s, sd->r, sd->s);
    for (int r = 0; r < 2; ++r) {
        S.h_first[r] = sd->h_first; S.h_count[r] = sd->h_count; S.snap_t[r] = sd->step_t;
        S.snap_ptr[r] = sd->nbr_ptr; S.nbr_o[r] = sd->nbr_o;
    }
    GroupedStore GS;
    GS.group = sd->group; GS.snap_ptr = sd->nbr_ptr; GS.nbr_o = sd->nbr_o; GS.trip_ptr = sd->trip_ptr;
    GS.trip_s = sd->trip_s; GS.trip_r = sd->trip_r; GS.trip_o = sd->trip_o; GS.by_subj = sd->by_subj;
    GS.subj_sorted = sd->subj_sorted; GS.n_steps = sd->n_steps; GS.n_nbr = sd->n_nbr; GS.n_facts = sd->n_facts;
    const int cap_steps = B * BB_MAXL, ck = GroupedBufs::cap_keys(sd);
    // sorted bits of the node / fact keys: a slot is < cap_steps < 2^slot_bits - 1, so the sentinel's ones still sort last
    const int slot_bits = bits_for((uint64_t)cap_steps);

    Carver cv{reinterpret_cast<char*>(workspace), workspace_bytes};
    GroupedBufs bf;
    if (!bf.carve(cv, sd, B, cap_nodes, cap_edges)) return RENET_ERR_WORKSPACE;
    int32_t* counts = out->counts;

    BB_HIP(hipMemsetAsync(counts, 0, RENET_BB_NCOUNTS * sizeof(int32_t), st));
    BB_HIP(hipMemsetAsync(bf.gkey, 0xFF, (size_t)cap_steps * sizeof(uint64_t), st));           // GB_NONE
    BB_HIP(hipMemsetAsync(bf.nkey, 0xFF, (size_t)ck * sizeof(uint64_t), st));
    BB_HIP(hipMemsetAsync(bf.fkey, 0xFF, (size_t)ce2 * sizeof(uint64_t), st));
    BB_HIP(hipMemsetAsync(bf.deg, 0, (size_t)(cap_nodes + 2) * sizeof(int32_t), st));
    BB_HIP(hipMemsetAsync(bf.tc, 0, bf.tc_bytes(), st));

    // A, B: length sort and steps, subject side only (Q = B: every sequence has role 0)
    if (int rc = launch_seq_steps(&S, idx_dev, B, B, seq_len, out, bf, bf.rel_label, bf.ent_label, st)) return rc;
    // C: slots = sorted unique (group, timestamp index) keys
    RENET_LAUNCH(gb_slot_keys_kernel, dim3((cap_steps + 255) / 256), dim3(256), 0, st, GS, counts, out->perm, bf.seq_len_s,
                 bf.seq_start, bf.step_dense, bf.gkey);
    RENET_LAUNCH_CHECK();
    BB_HIP(sort_keys(bf.tmp64, bf.tmp64_bytes, bf.gkey, bf.skey, (size_t)cap_steps, 64, st));
    RENET_LAUNCH(gb_run_flags_kernel, dim3((cap_steps + 255) / 256), dim3(256), 0, st, bf.skey, cap_steps, 0, bf.fa, (int32_t*)nullptr);
    RENET_LAUNCH_CHECK();
    BB_HIP(scan_plus(bf, bf.fa, bf.pa, (size_t)cap_steps, st));
    RENET_LAUNCH(gb_slots_kernel, dim3((cap_steps + 255) / 256), dim3(256), 0, st, bf.skey, cap_steps, bf.fa, bf.pa, bf.slot_key,
                 bf.slot_ti, counts);
    RENET_LAUNCH_CHECK();
    // D, E: node sets = sorted unique (slot, entity) keys, subject rows numbered first
    RENET_LAUNCH(gb_node_keys_kernel, dim3((cap_steps + 3) / 4), dim3(256), 0, st, GS, counts, bf.step_snap, bf.step_packed,
                 out->row_ent, bf.gkey, bf.slot_key, bf.slot_k, bf.nkey);
    RENET_LAUNCH_CHECK();
    BB_HIP(sort_keys(bf.tmp64, bf.tmp64_bytes, bf.nkey, bf.skey, (size_t)ck, 33 + slot_bits, st));
    RENET_LAUNCH(gb_run_flags_kernel, dim3((ck + 255) / 256), dim3(256), 0, st, bf.skey, ck, 1, bf.fa, bf.fb);
    RENET_LAUNCH_CHECK();
    BB_HIP(scan_plus(bf, bf.fa, bf.pa, (size_t)ck, st));
    BB_HIP(scan_plus(bf, bf.fb, bf.pb, (size_t)ck, st));
    RENET_LAUNCH(gb_node_count_kernel, dim3(1), dim3(1), 0, st, bf.fa, bf.pa, bf.fb, bf.pb, ck, cap_nodes, counts);
    RENET_LAUNCH_CHECK();
    RENET_LAUNCH(gb_number_kernel, dim3((ck + 255) / 256), dim3(256), 0, st, bf.skey, ck, bf.fa, bf.pa, bf.fb, bf.pb, counts,
                 bf.ukey, bf.uid, out->node_ent, out->node_slot);
    RENET_LAUNCH_CHECK();
    RENET_LAUNCH(gb_subj_row_kernel, dim3((cap_steps + 255) / 256), dim3(256), 0, st, counts, bf.step_packed, out->row_ent,
                 bf.slot_k, bf.ukey, bf.uid, out->subj_row);
    RENET_LAUNCH_CHECK();
    // F: induced edges through the subject index: count per node, scan, emit fact keys, sort back to (slot, fact) order
    RENET_LAUNCH(gb_node_facts_kernel, dim3((cap_nodes + 255) / 256), dim3(256), 0, st, GS, counts, cap_nodes, bf.ukey, bf.slot_ti,
                 0, bf.fa, bf.pa, bf.fkey);
    RENET_LAUNCH_CHECK();
    if (int rc = scan_set_e2(bf, bf.fa, bf.pa, counts, counts + RENET_BB_N, cap_nodes, cap_edges, st)) return rc;
    RENET_LAUNCH(gb_node_facts_kernel, dim3((cap_nodes + 255) / 256), dim3(256), 0, st, GS, counts, cap_nodes, bf.ukey, bf.slot_ti,
                 1, bf.fa, bf.pa, bf.fkey);
    RENET_LAUNCH_CHECK();
    BB_HIP(sort_keys(bf.tmp64, bf.tmp64_bytes, bf.fkey, bf.skey, (size_t)ce2, 32 + slot_bits, st));
    RENET_LAUNCH(gb_half_edges_kernel, dim3((ce2 + 255) / 256), dim3(256), 0, st, GS, counts, bf.skey, bf.ukey, bf.uid,
                 bf.half_src, bf.half_dst, bf.half_et);
    RENET_LAUNCH_CHECK();
    return finish_batch(bf, out, cap_nodes, cap_edges, cap_steps, sd->num_ent, sd->num_rels, key_bits, heavy_thr, group_budget,
                        chunk, B, st);
}

}  // extern "C"
