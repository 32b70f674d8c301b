// The shared part of the device batch-graph builders (builder_common.h): the kernels that more than one front launches
// (length sort, steps, E2, edge expansion, the closing copy of the counts), and everything behind the edge list -- the CSR
// by destination with relation-sorted rows, the relation-bucketed edge list and its <= 64-edge chunks (full and restricted
// to the row prefix), hub rows, the gather item stream and its wave groups, and the segmented-add plans (build_tail).  The
// fronts reach these kernels only through the host functions at the end of this file, and every rocPRIM call of the
// builders is made here.
#include "builder_common.h"
#include <rocprim/rocprim.hpp>

namespace {

// ---- stage A: length sort + per-sequence arrays (ONE workgroup) --------------------------------------------------
// sequences q in [0, 2B): q < B = subject side of quadruple idx[q] (entity s, history role 0, relation row r),
// q >= B = object side (entity o, role 1, relation row R + r).  Stable sort by descending history length.
// Q = 2B for the merged batch; Q = B: the subject side only (the grouped front: one direction per batch).  idx = nullptr:
// the identity (sequence q is quadruple q of the store).
__global__ __launch_bounds__(1024) void bb_seq_kernel(Store st, const int32_t* __restrict__ idx, int B, int Q, int seq_len,
                                                      int32_t* __restrict__ perm, int32_t* __restrict__ seq_first,
                                                      int32_t* __restrict__ seq_len_s, int32_t* __restrict__ seq_start,
                                                      int32_t* __restrict__ s_sorted, int32_t* __restrict__ r_sorted,
                                                      int32_t* __restrict__ rel_label, int32_t* __restrict__ ent_label,
                                                      int32_t* __restrict__ step_off, int32_t* __restrict__ counts) {
    __shared__ int lens[BB_MAXQ];
    __shared__ int pos_of[BB_MAXQ];
    __shared__ int wsum[16];
    __shared__ int hist[BB_MAXL + 2];
    for (int q = threadIdx.x; q < BB_MAXQ; q += 1024) {
        int len = 0;
        if (q < Q) {
            const int role = q >= B, qi = idx ? idx[q - role * B] : q - role * B;
            len = min(st.h_count[role][qi], seq_len);          // (the index already holds <= history_len snapshots)
        }
        lens[q] = q < Q ? len : -1;
    }
    if (threadIdx.x < BB_MAXL + 2) hist[threadIdx.x] = 0;
    __syncthreads();
    // stable counting sort, longest first: value v from BB_MAXL down to 0, members in index order
    int base = 0;
    for (int v = BB_MAXL; v >= 0; --v) {
        int mine[4], cnt = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) { mine[u] = lens[4 * threadIdx.x + u] == v; cnt += mine[u]; }
        int tot;
        int off = block_excl_scan_1024(cnt, &tot, wsum);
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (mine[u]) pos_of[4 * threadIdx.x + u] = base + off++;
        if (threadIdx.x == 0) hist[v] = tot;
        base += tot;
    }
    __syncthreads();
    // per sorted position
    for (int q = threadIdx.x; q < Q; q += 1024) {
        const int p = pos_of[q];
        const int role = q >= B, qi = idx ? idx[q - role * B] : q - role * B;
        const int len = lens[q];
        perm[p] = q;
        seq_len_s[p] = len;
        // the newest `len` snapshots of the window (preprocess.HistoryIndex.take with max_len)
        seq_first[p] = st.h_first[role][qi] + (st.h_count[role][qi] - len);
        const int s = st.q_s[qi], r = st.q_r[qi], o = st.q_o[qi];
        s_sorted[p] = role ? o : s;
        r_sorted[p] = r + (role ? st.num_rels : 0);
        rel_label[p] = r;
        ent_label[p] = role ? s : o;
    }
    __syncthreads();
    // nnz, L, S, step offsets (batch size of step j = #sequences longer than j), sequence-major step starts
    if (threadIdx.x == 0) {
        int nnz = 0, S = 0, L = 0;
        for (int v = 1; v <= BB_MAXL; ++v) { nnz += hist[v]; S += v * hist[v]; if (hist[v]) L = v; }
        counts[RENET_BB_NNZ] = nnz; counts[RENET_BB_S] = S; counts[RENET_BB_L] = L;
        int longer = nnz, off = 0;                       // longer = #sequences with len > j
        for (int j = 0; j <= BB_MAXL; ++j) {
            step_off[j] = off;
            off += longer;
            longer -= hist[j + 1 <= BB_MAXL ? j + 1 : BB_MAXL + 1];
        }
    }
    __syncthreads();
    // seq_start = exclusive scan of the sorted lengths (sequence-major step index of every sequence's first step)
    {
        int v[4], cnt = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int p = 4 * threadIdx.x + u;
            // sorted length at position p: recover from the histogram (positions are grouped by length, descending)
            int acc = 0, len = 0;
            for (int vv = BB_MAXL; vv >= 1; --vv) { if (p < acc + hist[vv]) { len = vv; break; } acc += hist[vv]; }
            v[u] = p < Q ? len : 0;
            cnt += v[u];
        }
        int tot;
        int off = block_excl_scan_1024(cnt, &tot, wsum);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int p = 4 * threadIdx.x + u;
            if (p < Q) seq_start[p] = off;
            off += v[u];
        }
    }
}

// ---- stage B: steps -------------------------------------------------------------------------------------------
// thread per (sorted sequence i, step j): packed row p = step_off[j] + i, sequence-major k = seq_start[i] + j
__global__ __launch_bounds__(256) void bb_steps_kernel(Store st, int B, const int32_t* __restrict__ perm,
                                                       const int32_t* __restrict__ seq_first,
                                                       const int32_t* __restrict__ seq_len_s,
                                                       const int32_t* __restrict__ seq_start,
                                                       const int32_t* __restrict__ s_sorted,
                                                       const int32_t* __restrict__ r_sorted,
                                                       const int32_t* __restrict__ step_off,
                                                       const int32_t* __restrict__ counts,
                                                       int32_t* __restrict__ step_snap, int32_t* __restrict__ step_dense,
                                                       int32_t* __restrict__ step_packed, int32_t* __restrict__ slot_used,
                                                       int32_t* __restrict__ row_seq, int32_t* __restrict__ row_ent,
                                                       int32_t* __restrict__ row_rel, int32_t* __restrict__ glob_row,
                                                       int32_t* __restrict__ err) {
    const int nnz = counts[RENET_BB_NNZ];
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = t / BB_MAXL, j = t - i * BB_MAXL;
    if (i >= nnz || j >= seq_len_s[i]) return;
    const int role = perm[i] >= B;
    const int snap = seq_first[i] + j;
    const int k = seq_start[i] + j, p = step_off[j] + i;
    const int tt = st.snap_t[role][snap];
    const int tidx = lower_bound_i32(st.times, st.T, tt);
    if (tidx >= st.T || st.times[tidx] != tt) { atomicOr(err, RENET_BB_ERR_TIME); return; }
    const int dense = role * st.T + tidx;
    step_snap[k] = snap | (role << 30);
    step_dense[k] = dense;
    step_packed[k] = p;
    slot_used[dense] = 1;
    row_seq[p] = i;
    row_ent[p] = s_sorted[i];
    row_rel[p] = r_sorted[i];
    const int gi = lower_bound_i32(st.glob_times, st.n_glob, tt);
    if (gi >= st.n_glob || st.glob_times[gi] != tt) { atomicOr(err, RENET_BB_ERR_GLOB); return; }
    glob_row[p] = gi;
}

__global__ __launch_bounds__(256) void bb_expand_kernel(const int32_t* __restrict__ counts, int num_rels, int cap_edges,
                                                        int key_bits, const int32_t* __restrict__ half_src,
                                                        const int32_t* __restrict__ half_dst,
                                                        const int32_t* __restrict__ half_et,
                                                        int32_t* __restrict__ src, int32_t* __restrict__ dst,
                                                        int32_t* __restrict__ et, uint32_t* __restrict__ key_dt,
                                                        uint32_t* __restrict__ key_t, uint32_t* __restrict__ key_t2,
                                                        int32_t* __restrict__ iota, int32_t* __restrict__ deg,
                                                        int32_t* __restrict__ tc, int32_t* __restrict__ tc2) {
    // relation frequencies are Zipf-like (the hottest type owns a third of the edges): global atomics on the 2R-bin
    // histograms serialise (1.3 ms of a 2.2 ms build); workgroup-local LDS histograms, flushed once, instead
    __shared__ int h1[1024], h2[1024];
    const int T2 = 2 * num_rels;
    for (int i = threadIdx.x; i < T2; i += blockDim.x) { h1[i] = 0; h2[i] = 0; }
    __syncthreads();
    const int E2 = counts[RENET_BB_E2], E = 2 * E2, nA = counts[RENET_BB_NA];
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < cap_edges; e += gridDim.x * blockDim.x) {
        iota[e] = e;
        if (e >= E) {                                     // sentinels: sorted behind every valid key
            key_dt[e] = 1u << key_bits;
            key_t[e] = (uint32_t)T2;
            key_t2[e] = (uint32_t)T2;
            continue;
        }
        const int m = e < E2 ? e : e - E2;
        int s = half_src[m], d = half_dst[m], t = half_et[m];
        if (e >= E2) { const int tmp = s; s = d; d = tmp; t = t + num_rels >= T2 ? t + num_rels - T2 : t + num_rels; }
        src[e] = s; dst[e] = d; et[e] = t;
        key_dt[e] = (uint32_t)d * (uint32_t)T2 + (uint32_t)t;
        key_t[e] = (uint32_t)t;
        key_t2[e] = d < nA ? (uint32_t)t : (uint32_t)T2;
        atomicAdd(&deg[d], 1);
        atomicAdd(&h1[t], 1);
        if (d < nA) atomicAdd(&h2[t], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < T2; i += blockDim.x) {
        if (h1[i]) atomicAdd(&tc[i], h1[i]);
        if (h2[i]) atomicAdd(&tc2[i], h2[i]);
    }
}

// E2 = total of flag[0 .. *n_ptr) from its exclusive scan pos (flag = kept facts per entry: 0 / 1 per fact, or a count per node)
__global__ void bb_set_e2_kernel(const int32_t* __restrict__ flag, const int32_t* __restrict__ pos,
                                 int32_t* __restrict__ counts, const int32_t* __restrict__ n_ptr, int cap_facts,
                                 int cap_edges) {
    const int F = min(*n_ptr, cap_facts);
    int e2 = F > 0 ? pos[F - 1] + flag[F - 1] : 0;
    if (counts[RENET_BB_ERR] != 0) e2 = 0;                 // node overflow / bad timestamp: no edges (new_id is not valid)
    if (2 * e2 > cap_edges) { atomicOr(&counts[RENET_BB_ERR], RENET_BB_ERR_EDGES); e2 = 0; }
    counts[RENET_BB_E2] = e2;
    counts[RENET_BB_E] = 2 * e2;
}

// CSR columns / types from the (dst, type)-sorted order; relation-bucketed lists from the type-sorted orders
__global__ __launch_bounds__(256) void bb_apply_orders_kernel(const int32_t* __restrict__ counts, int cap_edges,
                                                              const int32_t* __restrict__ src,
                                                              const int32_t* __restrict__ dst,
                                                              const int32_t* __restrict__ et,
                                                              const int32_t* __restrict__ ord_dt,
                                                              const int32_t* __restrict__ ord_t,
                                                              const int32_t* __restrict__ ord_t2,
                                                              const int32_t* __restrict__ row_ptr,
                                                              int32_t* __restrict__ col, int32_t* __restrict__ etype,
                                                              int32_t* __restrict__ e_src, int32_t* __restrict__ e_dst,
                                                              int32_t* __restrict__ e_src2, int32_t* __restrict__ e_dst2) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap_edges) return;
    const int E = counts[RENET_BB_E];
    if (i < E) {
        const int a = ord_dt[i], b = ord_t[i];
        col[i] = src[a]; etype[i] = et[a];
        e_src[i] = src[b]; e_dst[i] = dst[b];
    }
    if (!e_src2) return;                                   // (full-graph batches have no row prefix)
    const int E_out = row_ptr[counts[RENET_BB_NA]];
    if (i < E_out) { const int c = ord_t2[i]; e_src2[i] = src[c]; e_dst2[i] = dst[c]; }
}

// norm = 1 / max(in-degree, 1) (utils.py:126-127), hub flags, light-row item counts
__global__ __launch_bounds__(256) void bb_rows_kernel(const int32_t* __restrict__ counts, int cap_nodes, int heavy_thr,
                                                      const int32_t* __restrict__ deg, float* __restrict__ norm,
                                                      int32_t* __restrict__ heavy_flag, int32_t* __restrict__ item_cnt,
                                                      int32_t* __restrict__ light_id) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v > cap_nodes) return;
    const int N = counts[RENET_BB_N];
    int hf = 0, ic = 0, li = -1;
    if (v < N) {
        const int d = deg[v];
        norm[v] = 1.f / (float)max(d, 1);
        hf = d > heavy_thr;
        if (!hf) { ic = d + 1; li = v; }
    }
    heavy_flag[v] = hf; item_cnt[v] = ic; light_id[v] = li;
}

__global__ __launch_bounds__(256) void bb_heavy_kernel(const int32_t* __restrict__ counts_c, int32_t* __restrict__ counts,
                                                       int cap_nodes, const int32_t* __restrict__ heavy_flag,
                                                       const int32_t* __restrict__ heavy_pos,
                                                       int32_t* __restrict__ heavy_rows) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = counts_c[RENET_BB_N], nA = counts_c[RENET_BB_NA];
    if (v < N && heavy_flag[v]) heavy_rows[heavy_pos[v]] = v;
    if (v == 0) {
        counts[RENET_BB_NHEAVY] = N > 0 ? heavy_pos[N - 1] + heavy_flag[N - 1] : 0;
        counts[RENET_BB_NHEAVY_OUT] = nA > 0 ? heavy_pos[nA - 1] + heavy_flag[nA - 1] : 0;
    }
    (void)cap_nodes;
}

// chunk lists of the relation-bucketed edge list: <= chunk edges of ONE relation per work item (ONE workgroup per
// list; T2 <= 1024 relation types)
__global__ __launch_bounds__(1024) void bb_chunks_kernel(const int32_t* __restrict__ tc_a, const int32_t* __restrict__ tc_b,
                                                         int T2, int chunk, int cap_chunks,
                                                         int32_t* __restrict__ tcp_a, int32_t* __restrict__ tcp_b,
                                                         int32_t* __restrict__ ctype_a, int32_t* __restrict__ cptr_a,
                                                         int32_t* __restrict__ ctype_b, int32_t* __restrict__ cptr_b,
                                                         int32_t* __restrict__ counts, int32_t* __restrict__ err) {
    __shared__ int wsum[16];
    const int which = blockIdx.x;
    const int32_t* tc = which ? tc_b : tc_a;
    int32_t* tcp = which ? tcp_b : tcp_a;
    int32_t* ctype = which ? ctype_b : ctype_a;
    int32_t* cptr = which ? cptr_b : cptr_a;
    const int t = threadIdx.x;
    const int n = t < T2 ? tc[t] : 0;
    const int nch = (n + chunk - 1) / chunk;
    int tot_e, tot_c;
    const int e0 = block_excl_scan_1024(n, &tot_e, wsum);
    const int c0 = block_excl_scan_1024(nch, &tot_c, wsum);
    if (t < T2) tcp[t] = c0;
    if (t == 0) {
        tcp[T2] = tot_c;
        counts[which ? RENET_BB_NCHUNKS2 : RENET_BB_NCHUNKS] = tot_c;
        if (tot_c > cap_chunks) atomicOr(err, RENET_BB_ERR_EDGES);
    }
    if (tot_c > cap_chunks) return;
    for (int w = 0; w < nch; ++w) { ctype[c0 + w] = t; cptr[c0 + w] = e0 + w * chunk; }
    if (t == 0) cptr[tot_c] = tot_e;
}

// ---- stage G: gather item stream + wave groups (graph.plan_gather_items) --------------------------------------------
__global__ __launch_bounds__(256) void bb_items_kernel(const int32_t* __restrict__ counts, int budget,
                                                       const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                       const int32_t* __restrict__ etype, const int32_t* __restrict__ item_cnt,
                                                       const int32_t* __restrict__ item_start,
                                                       const int32_t* __restrict__ prev_light,
                                                       int32_t* __restrict__ it_src, int32_t* __restrict__ it_type,
                                                       int32_t* __restrict__ first_flag, int32_t* __restrict__ first_out) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = counts[RENET_BB_N], nA = counts[RENET_BB_NA];
    int ff = 0, fo = 0;
    if (v < N && item_cnt[v] > 0) {
        const int st = item_start[v], e0 = row_ptr[v], d = item_cnt[v] - 1;
        for (int q = 0; q < d; ++q) { it_src[st + q] = col[e0 + q]; it_type[st + q] = etype[e0 + q]; }
        it_src[st + d] = v; it_type[st + d] = -1;
        const int pl = prev_light[v];                     // the previous light row, -1 if none
        const int side = v >= nA;
        ff = pl < 0 || (item_start[pl] / budget) != (st / budget) || ((pl >= nA) != side);
        fo = ff && !side;
    }
    if (v <= N) { first_flag[v] = ff; first_out[v] = fo; }
}

__global__ __launch_bounds__(256) void bb_groups_kernel(const int32_t* __restrict__ counts_c, int32_t* __restrict__ counts,
                                                        int cap_nodes, const int32_t* __restrict__ first_flag,
                                                        const int32_t* __restrict__ first_pos,
                                                        const int32_t* __restrict__ first_out_pos,
                                                        const int32_t* __restrict__ first_out,
                                                        const int32_t* __restrict__ item_start,
                                                        const int32_t* __restrict__ item_cnt,
                                                        int32_t* __restrict__ grp_ptr) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = counts_c[RENET_BB_N];
    if (v < N && first_flag[v]) grp_ptr[first_pos[v]] = item_start[v];
    if (v == 0) {
        const int ng = N > 0 ? first_pos[N - 1] + first_flag[N - 1] : 0;
        const int total = N > 0 ? item_start[N - 1] + item_cnt[N - 1] : 0;
        grp_ptr[ng] = total;
        counts[RENET_BB_NGROUPS] = ng;
        counts[RENET_BB_NGROUPS_OUT] = N > 0 ? first_out_pos[N - 1] + first_out[N - 1] : 0;
        counts[RENET_BB_NITEMS] = total;
    }
    (void)cap_nodes;
}

// ---- stage H: segmented-add plans (graph.SegPlan): rows sorted stably by key, segment starts, segment targets ----
__global__ __launch_bounds__(256) void bb_plan_keys_kernel(const int32_t* __restrict__ idx, const int32_t* __restrict__ n_ptr,
                                                           int n_fixed, int cap, uint32_t sentinel,
                                                           uint32_t* __restrict__ key, int32_t* __restrict__ iota) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap) return;
    const int n = n_ptr ? *n_ptr : n_fixed;
    key[i] = i < n ? (uint32_t)idx[i] : sentinel;
    iota[i] = i;
}

__global__ __launch_bounds__(256) void bb_plan_flags_kernel(const uint32_t* __restrict__ skey, const int32_t* __restrict__ n_ptr,
                                                            int n_fixed, int cap, int32_t* __restrict__ flag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > cap) return;
    const int n = n_ptr ? *n_ptr : n_fixed;
    flag[i] = (i < n && (i == 0 || skey[i] != skey[i - 1])) ? 1 : 0;
}

__global__ __launch_bounds__(256) void bb_plan_segs_kernel(const uint32_t* __restrict__ skey, const int32_t* __restrict__ n_ptr,
                                                           int n_fixed, int cap, const int32_t* __restrict__ flag,
                                                           const int32_t* __restrict__ pos, int32_t* __restrict__ seg_ptr,
                                                           int32_t* __restrict__ target, int32_t* __restrict__ count_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = n_ptr ? *n_ptr : n_fixed;
    if (i < n && flag[i]) { seg_ptr[pos[i]] = i; target[pos[i]] = (int32_t)skey[i]; }
    if (i == 0) {
        const int u = n > 0 ? pos[n - 1] + flag[n - 1] : 0;
        seg_ptr[u] = n;
        *count_out = u;
    }
    (void)cap;
}

__global__ void bb_finish_kernel(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ step_off,
                                 int32_t* __restrict__ counts) {
    const int t = threadIdx.x;
    if (t <= BB_MAXL) counts[RENET_BB_STEP_OFF + t] = step_off[t];
    if (t == 0) counts[RENET_BB_EOUT] = row_ptr[counts[RENET_BB_NA]];
}

}  // namespace

bool TailBufs::carve_tail(Carver& cv, int cap_nodes, int cap_edges, int cap_steps, int cap_facts, bool pruned) {
    src = cv.take<int32_t>(cap_edges);
    dst = cv.take<int32_t>(cap_edges);
    et = cv.take<int32_t>(cap_edges);
    key_dt = cv.take<uint32_t>(cap_edges);
    key_t = cv.take<uint32_t>(cap_edges);
    key_t2 = pruned ? cv.take<uint32_t>(cap_edges) : nullptr;
    key_sorted = cv.take<uint32_t>(max(cap_edges, max(cap_nodes, cap_steps)));
    iota = cv.take<int32_t>(max(cap_edges, max(cap_nodes, cap_steps)));
    ord_dt = cv.take<int32_t>(cap_edges);
    ord_t = cv.take<int32_t>(cap_edges);
    ord_t2 = pruned ? cv.take<int32_t>(cap_edges) : nullptr;
    deg = cv.take<int32_t>(cap_nodes + 2);
    tc = cv.take<int32_t>(pruned ? 2048 : 1024);
    tc2 = pruned && tc ? tc + 1024 : nullptr;
    heavy_flag = cv.take<int32_t>(cap_nodes + 2);
    heavy_pos = cv.take<int32_t>(cap_nodes + 2);
    item_cnt = cv.take<int32_t>(cap_nodes + 2);
    item_start = cv.take<int32_t>(cap_nodes + 2);
    light_id = cv.take<int32_t>(cap_nodes + 2);
    prev_light = cv.take<int32_t>(cap_nodes + 2);
    first_flag = cv.take<int32_t>(cap_nodes + 2);
    first_pos = cv.take<int32_t>(cap_nodes + 2);
    first_out = cv.take<int32_t>(cap_nodes + 2);
    first_out_pos = pruned ? cv.take<int32_t>(cap_nodes + 2) : nullptr;
    pkey = cv.take<uint32_t>(max(cap_nodes, cap_steps));
    pflag = cv.take<int32_t>(max(cap_nodes, cap_steps) + 2);
    ppos = cv.take<int32_t>(max(cap_nodes, cap_steps) + 2);
    // rocPRIM scratch: the largest need of the scans and of the pair sorts (plan 1 sorts cap_steps rows)
    size_t m = 0, t = 0;
    (void)rocprim::exclusive_scan(nullptr, t, (int*)nullptr, (int*)nullptr, 0,
                                  (size_t)max(max(cap_nodes + 1, cap_facts), 1), rocprim::plus<int>());
    m = max(m, t);
    (void)rocprim::exclusive_scan(nullptr, t, (int*)nullptr, (int*)nullptr, -1, (size_t)max(cap_nodes + 1, 1),
                                  rocprim::maximum<int>());
    m = max(m, t);
    (void)rocprim::radix_sort_pairs(nullptr, t, (uint32_t*)nullptr, (uint32_t*)nullptr, (int*)nullptr, (int*)nullptr,
                                    (size_t)max(max(cap_edges, cap_steps), max(cap_nodes, 1)), 0, 32);
    tmp_bytes = (max(m, t) + 255) & ~(size_t)255;
    tmp = cv.take<char>(tmp_bytes);
    return tmp != nullptr && cv.ok;
}

hipError_t scan_plus(const TailBufs& bf, int32_t* in, int32_t* out, size_t n, hipStream_t st) {
    size_t tb = bf.tmp_bytes;
    return rocprim::exclusive_scan(bf.tmp, tb, in, out, 0, n, rocprim::plus<int>(), st);
}
hipError_t scan_max(const TailBufs& bf, int32_t* in, int32_t* out, size_t n, hipStream_t st) {
    size_t tb = bf.tmp_bytes;
    return rocprim::exclusive_scan(bf.tmp, tb, in, out, -1, n, rocprim::maximum<int>(), st);
}
hipError_t sort_pairs(const TailBufs& bf, uint32_t* keys, int32_t* vals_out, size_t n, int bits, hipStream_t st) {
    size_t tb = bf.tmp_bytes;
    return rocprim::radix_sort_pairs(bf.tmp, tb, keys, bf.key_sorted, bf.iota, vals_out, n, 0, bits, st);
}
hipError_t sort_keys(void* tmp, size_t& tmp_bytes, uint64_t* in, uint64_t* out, size_t n, int bits, hipStream_t st) {
    return rocprim::radix_sort_keys(tmp, tmp_bytes, in, out, n, 0, bits, st);
}

int launch_seq_steps(const void* S_, const int32_t* idx, int B, int Q, int seq_len, const RenetBatchOut* out,
                     const SeqBufs& bf, int32_t* rel_label, int32_t* ent_label, hipStream_t st) {
    static_assert(sizeof(Store) == 19 * sizeof(void*) + 4 * sizeof(int), "Store: the layout the fronts fill");
    const Store& S = *static_cast<const Store*>(S_);
    RENET_LAUNCH(bb_seq_kernel, dim3(1), dim3(1024), 0, st, S, idx, B, Q, seq_len, out->perm, bf.seq_first, bf.seq_len_s,
                 bf.seq_start, out->s_sorted, out->r_sorted, rel_label, ent_label, out->step_off, out->counts);
    RENET_LAUNCH_CHECK();
    RENET_LAUNCH(bb_steps_kernel, dim3((Q * BB_MAXL + 255) / 256), dim3(256), 0, st, S, B, out->perm, bf.seq_first,
                 bf.seq_len_s, bf.seq_start, out->s_sorted, out->r_sorted, out->step_off, out->counts, bf.step_snap, bf.step_dense,
                 bf.step_packed, bf.slot_used, out->row_seq, out->row_ent, out->row_rel, out->glob_row, out->counts + RENET_BB_ERR);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}

int scan_set_e2(const TailBufs& bf, int32_t* flag, int32_t* pos, int32_t* counts, const int32_t* n_ptr, int cap, int cap_edges,
                hipStream_t st) {
    BB_HIP(scan_plus(bf, flag, pos, (size_t)cap, st));
    RENET_LAUNCH(bb_set_e2_kernel, dim3(1), dim3(1), 0, st, flag, pos, counts, n_ptr, cap, cap_edges);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}

// ---- the shared tail: stages F (sorts, rows, chunks), G (item stream, wave groups) and H (the first n_plans plans) over an
// edge list that a front has left in bf.src / dst / et with its keys, bf.deg and the histograms.  pruned = false: the
// batch has no row prefix (nA = N): the *2 lists, n_chunks2 and n_groups_out's own scan are not computed.
int build_tail(const TailBufs& bf, const RenetBatchOut* out, int cap_nodes, int cap_edges, int cap_steps, int num_ent, int T2,
               int key_bits, int heavy_thr, int group_budget, int chunk, int n_plans, int n_seq, bool pruned, hipStream_t st) {
    int32_t* counts = out->counts;
    int32_t* err = counts + RENET_BB_ERR;
    const int cap_chunks = cap_edges / chunk + T2 + 1;
    const int tbits = bits_for((uint64_t)T2);
    const size_t n_rows = (size_t)(cap_nodes + 1);
    BB_HIP(sort_pairs(bf, bf.key_dt, bf.ord_dt, (size_t)cap_edges, key_bits + 1, st));
    BB_HIP(sort_pairs(bf, bf.key_t, bf.ord_t, (size_t)cap_edges, tbits, st));
    if (pruned) BB_HIP(sort_pairs(bf, bf.key_t2, bf.ord_t2, (size_t)cap_edges, tbits, st));
    // rows
    BB_HIP(scan_plus(bf, bf.deg, out->row_ptr, n_rows, st));
    RENET_LAUNCH(bb_rows_kernel, dim3((cap_nodes + 1 + 255) / 256), dim3(256), 0, st, counts, cap_nodes, heavy_thr, bf.deg,
                 out->norm, bf.heavy_flag, bf.item_cnt, bf.light_id);
    RENET_LAUNCH_CHECK();
    RENET_LAUNCH(bb_apply_orders_kernel, dim3((cap_edges + 255) / 256), dim3(256), 0, st, counts, cap_edges, bf.src, bf.dst, bf.et,
                 bf.ord_dt, bf.ord_t, bf.ord_t2, out->row_ptr, out->col, out->etype, out->e_src, out->e_dst,
                 pruned ? out->e_src2 : nullptr, pruned ? out->e_dst2 : nullptr);
    RENET_LAUNCH_CHECK();
    BB_HIP(scan_plus(bf, bf.heavy_flag, bf.heavy_pos, n_rows, st));
    RENET_LAUNCH(bb_heavy_kernel, dim3((cap_nodes + 255) / 256), dim3(256), 0, st, counts, counts, cap_nodes, bf.heavy_flag,
                 bf.heavy_pos, out->heavy_rows);
    RENET_LAUNCH_CHECK();
    RENET_LAUNCH(bb_chunks_kernel, dim3(pruned ? 2 : 1), dim3(1024), 0, st, bf.tc, bf.tc2, T2, chunk, cap_chunks, out->type_chunk_ptr,
                 out->type_chunk_ptr2, out->chunk_type, out->chunk_ptr, out->chunk_type2, out->chunk_ptr2, counts, err);
    RENET_LAUNCH_CHECK();
    // gather item plan
    BB_HIP(scan_plus(bf, bf.item_cnt, bf.item_start, n_rows, st));
    BB_HIP(scan_max(bf, bf.light_id, bf.prev_light, n_rows, st));
    RENET_LAUNCH(bb_items_kernel, dim3((cap_nodes + 1 + 255) / 256), dim3(256), 0, st, counts, group_budget, out->row_ptr,
                 out->col, out->etype, bf.item_cnt, bf.item_start, bf.prev_light, out->it_src, out->it_type, bf.first_flag, bf.first_out);
    RENET_LAUNCH_CHECK();
    BB_HIP(scan_plus(bf, bf.first_flag, bf.first_pos, n_rows, st));
    if (pruned) BB_HIP(scan_plus(bf, bf.first_out, bf.first_out_pos, n_rows, st));
    // (without a row prefix every group is a group of the prefix: first_out == first_flag, n_groups_out == n_groups)
    RENET_LAUNCH(bb_groups_kernel, dim3((cap_nodes + 255) / 256), dim3(256), 0, st, counts, counts, cap_nodes, bf.first_flag,
                 bf.first_pos, pruned ? bf.first_out_pos : bf.first_pos, pruned ? bf.first_out : bf.first_flag, bf.item_start,
                 bf.item_cnt, out->grp_ptr);
    RENET_LAUNCH_CHECK();
    // segmented-add plans: 0 node_ent (N rows), 1 subj_row (S rows), 2 s_sorted, 3 r_sorted (n_ptr = nullptr: n_seq rows, every
    // sequence); bound: the keys are below it
    const struct { const int32_t* idx; const int32_t* n_ptr; int cap; uint64_t bound; } plans[4] = {
        {out->node_ent, counts + RENET_BB_N, cap_nodes, (uint64_t)num_ent},
        {out->subj_row, counts + RENET_BB_S, cap_steps, (uint64_t)cap_nodes},
        {out->s_sorted, nullptr, n_seq, (uint64_t)num_ent},
        {out->r_sorted, nullptr, n_seq, (uint64_t)T2}};
    for (int pl = 0; pl < n_plans; ++pl) {
        const int32_t* n_ptr = plans[pl].n_ptr;
        const int cap = plans[pl].cap, kb = bits_for(plans[pl].bound);
        RENET_LAUNCH(bb_plan_keys_kernel, dim3((cap + 255) / 256), dim3(256), 0, st, plans[pl].idx, n_ptr, n_seq, cap,
                     (uint32_t)(1u << kb), bf.pkey, bf.iota);
        RENET_LAUNCH_CHECK();
        BB_HIP(sort_pairs(bf, bf.pkey, out->plan_order[pl], (size_t)cap, kb + 1, st));
        RENET_LAUNCH(bb_plan_flags_kernel, dim3((cap + 1 + 255) / 256), dim3(256), 0, st, bf.key_sorted, n_ptr, n_seq, cap,
                     bf.pflag);
        RENET_LAUNCH_CHECK();
        BB_HIP(scan_plus(bf, bf.pflag, bf.ppos, (size_t)(cap + 1), st));
        RENET_LAUNCH(bb_plan_segs_kernel, dim3((cap + 255) / 256), dim3(256), 0, st, bf.key_sorted, n_ptr, n_seq, cap, bf.pflag,
                     bf.ppos, out->plan_seg[pl], out->plan_target[pl], counts + RENET_BB_NSEG0 + pl);
        RENET_LAUNCH_CHECK();
    }
    return RENET_OK;
}

int finish_batch(const SeqBufs& bf, const RenetBatchOut* out, int cap_nodes, int cap_edges, int cap_steps, int num_ent,
                 int num_rels, int key_bits, int heavy_thr, int group_budget, int chunk, int n_seq, hipStream_t st) {
    RENET_LAUNCH(bb_expand_kernel, dim3(min((cap_edges + 255) / 256, 1024)), dim3(256), 0, st, out->counts, num_rels, cap_edges,
                 key_bits, bf.half_src, bf.half_dst, bf.half_et, bf.src, bf.dst, bf.et, bf.key_dt, bf.key_t, bf.key_t2, bf.iota, bf.deg, bf.tc, bf.tc2);
    RENET_LAUNCH_CHECK();
    if (int rc = build_tail(bf, out, cap_nodes, cap_edges, cap_steps, num_ent, 2 * num_rels, key_bits, heavy_thr, group_budget, chunk,
                            4, n_seq, true, st))
        return rc;
    RENET_LAUNCH(bb_finish_kernel, dim3(1), dim3(64), 0, st, out->row_ptr, out->step_off, out->counts);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}
