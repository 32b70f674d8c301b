// Batch-graph builder ON THE DEVICE for the FULL-GRAPH batches of the global model (graph.build_full_graphs; reference
// Aggregator.py:44-55 / 87-98: dgl.batch of the whole graphs of a list of timestamps): the front of
// renet_build_full_graphs.  Nothing is induced or renumbered here: the per-timestamp node lists and LOCAL fact endpoints
// are resident (RenetFullStoreDev), member graph k is the graph of timestamp index tidx[k] shifted by the node offset of
// k.  Three front kernels leave the edge list where the shared tail (build_tail, builder_tail.hip) expects it;
// tests/test_gpu_full_graph_builder.py compares every array with the host builder's.
#include "builder_common.h"

namespace {

struct FullStore {
    const int32_t* node_ptr;
    const int32_t* node_ent_all;
    const int32_t* trip_ptr;
    const int32_t *trip_ls, *trip_r, *trip_lo;
    int T, num_rels;
};

// ---- full-graph stage A (ONE workgroup, G <= 1024): node / fact counts of the member graphs and their scans --------
__global__ __launch_bounds__(1024) void fg_counts_kernel(FullStore st, const int32_t* __restrict__ tidx, int G, int cap_nodes,
                                                         int cap_edges, int32_t* __restrict__ gti, int32_t* __restrict__ seg_ptr,
                                                         int32_t* __restrict__ fact_off, int32_t* __restrict__ counts) {
    __shared__ int wsum[16];
    __shared__ int s_bad;
    const int k = threadIdx.x;
    if (k == 0) s_bad = 0;
    __syncthreads();
    int ti = -1, nn = 0, nf = 0;
    if (k < G) {
        ti = tidx[k];
        if (ti < 0 || ti >= st.T) { ti = -1; s_bad = 1; }            // (not a timestamp of the store: an empty member graph)
        else { nn = st.node_ptr[ti + 1] - st.node_ptr[ti]; nf = st.trip_ptr[ti + 1] - st.trip_ptr[ti]; }
        gti[k] = ti;
    }
    int N, F;
    const int noff = block_excl_scan_1024(nn, &N, wsum);
    const int foff = block_excl_scan_1024(nf, &F, wsum);               // (its first barrier also publishes s_bad)
    int e = s_bad ? RENET_BB_ERR_TIME : 0;
    if (N > cap_nodes) e |= RENET_BB_ERR_NODES;
    if (2 * (long long)F > cap_edges) e |= RENET_BB_ERR_EDGES;
    if (k < G) { seg_ptr[k] = noff; fact_off[k] = foff; }
    if (k == 0) {
        seg_ptr[G] = N; fact_off[G] = F;
        if (e) { N = 0; F = 0; }                                       // every later stage then sees an EMPTY graph (no OOB access)
        counts[RENET_BB_ERR] = e;
        counts[RENET_BB_TB] = G;
        counts[RENET_BB_N] = N; counts[RENET_BB_NA] = N;
        counts[RENET_BB_FACTS] = F; counts[RENET_BB_E2] = F; counts[RENET_BB_E] = 2 * F; counts[RENET_BB_EOUT] = 2 * F;
    }
}

// last k in [0, G) with off[k] <= v (off non-decreasing, off[0] = 0 <= v; member graphs may be empty)
__device__ __forceinline__ int last_le_i32(const int32_t* off, int G, int v) {
    int lo = 0, hi = G;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (off[mid] <= v) lo = mid; else hi = mid; }
    return lo;
}

// ---- full-graph stage B: node_ent = ragged copy of the member graphs' node lists ----------------------------------------
__global__ __launch_bounds__(256) void fg_nodes_kernel(FullStore st, const int32_t* __restrict__ counts, int G, int cap_nodes,
                                                       const int32_t* __restrict__ gti, const int32_t* __restrict__ seg_ptr,
                                                       int32_t* __restrict__ node_ent) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= cap_nodes || v >= counts[RENET_BB_N]) return;
    const int k = last_le_i32(seg_ptr, G, v);
    node_ent[v] = st.node_ent_all[st.node_ptr[gti[k]] + (v - seg_ptr[k])];
}

// ---- full-graph stage C: the edge list, in the order of graph.build_full_graphs' concatenation: member graph k owns
// positions [2 fact_off[k], 2 fact_off[k + 1]): first ls -> lo with type r for all its facts, then lo -> ls with type
// r + R (graph.TimeGraph.edges; the halves are per GRAPH).  Also what bb_expand_kernel leaves for the tail: the sort
// keys (sentinels behind E), iota, the in-degrees and the relation histogram.
__global__ __launch_bounds__(256) void fg_edges_kernel(FullStore st, const int32_t* __restrict__ counts, int G, int cap_edges,
                                                       int key_bits, const int32_t* __restrict__ gti,
                                                       const int32_t* __restrict__ seg_ptr, const int32_t* __restrict__ fact_off,
                                                       int32_t* __restrict__ src, int32_t* __restrict__ dst,
                                                       int32_t* __restrict__ et, uint32_t* __restrict__ key_dt,
                                                       uint32_t* __restrict__ key_t, int32_t* __restrict__ iota,
                                                       int32_t* __restrict__ deg, int32_t* __restrict__ tc,
                                                       int32_t* __restrict__ err) {
    __shared__ int h1[1024];                               // (workgroup-local histogram, flushed once: see bb_expand_kernel)
    const int T2 = 2 * st.num_rels;
    for (int i = threadIdx.x; i < T2; i += blockDim.x) h1[i] = 0;
    __syncthreads();
    const int E = counts[RENET_BB_E], N = counts[RENET_BB_N];
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < cap_edges; e += gridDim.x * blockDim.x) {
        iota[e] = e;
        if (e >= E) {                                     // sentinels: sorted behind every valid key
            key_dt[e] = 1u << key_bits;
            key_t[e] = (uint32_t)T2;
            continue;
        }
        const int k = last_le_i32(fact_off, G, e >> 1);    // 2 fact_off[k] <= e  <=>  fact_off[k] <= e / 2
        const int f0 = fact_off[k], nf = fact_off[k + 1] - f0, off = seg_ptr[k];
        const int local = e - 2 * f0, rev = local >= nf;
        const int j = st.trip_ptr[gti[k]] + (rev ? local - nf : local);
        const int a = st.trip_ls[j] + off, b = st.trip_lo[j] + off;
        const int s = rev ? b : a, d = rev ? a : b;
        const int t = st.trip_r[j] + (rev ? st.num_rels : 0);
        if ((unsigned)d >= (unsigned)N || (unsigned)s >= (unsigned)N || (unsigned)t >= (unsigned)T2) {
            // (the store is range-checked on the host; never index with a bad id all the same)
            atomicOr(err, RENET_BB_ERR_EDGES);
            src[e] = 0; dst[e] = 0; et[e] = 0;
            key_dt[e] = 1u << key_bits; key_t[e] = (uint32_t)T2;
            continue;
        }
        src[e] = s; dst[e] = d; et[e] = t;
        key_dt[e] = (uint32_t)d * (uint32_t)T2 + (uint32_t)t;
        key_t[e] = (uint32_t)t;
        atomicAdd(&deg[d], 1);
        atomicAdd(&h1[t], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < T2; i += blockDim.x)
        if (h1[i]) atomicAdd(&tc[i], h1[i]);
}

// scratch of the full-graph front + the tail
struct FullBufs : TailBufs {
    int32_t* gti;                  // [G] validated timestamp index of every member graph
    int32_t* fact_off;             // [G + 1] scan of the fact counts
    bool carve(Carver& cv, int G, int cap_nodes, int cap_edges) {
        gti = cv.take<int32_t>(G);
        fact_off = cv.take<int32_t>(G + 1);
        return carve_tail(cv, cap_nodes, cap_edges, 0, 0, false);
    }
};

}  // namespace

extern "C" {

size_t renet_build_full_graphs_workspace(const RenetFullStoreDev* sd, int G, int cap_nodes, int cap_edges) {
    if (!sd || G <= 0 || G > 1024 || cap_nodes <= 0 || cap_edges <= 0) return 0;
    return workspace_of<FullBufs>(G, cap_nodes, max(cap_edges & ~1, 2));
}

int renet_build_full_graphs(const RenetFullStoreDev* sd, const int32_t* tidx_dev, int G, int heavy_thr, int group_items,
                            int chunk, RenetBatchOut* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!sd || !out || !tidx_dev || G <= 0 || G > 1024 || out->cap_nodes <= 0 || out->cap_edges <= 0 || !out->seg_ptr)
        return RENET_ERR_BADARG;
    const int cap_nodes = out->cap_nodes, cap_edges = max(out->cap_edges & ~1, 2);
    int T2, key_bits;
    if (sd->num_rels <= 0 || check_common(sd->num_rels, sd->T, heavy_thr, group_items, chunk, cap_nodes, &T2, &key_bits))
        return RENET_ERR_UNSUPPORTED;
    if (workspace_bytes < renet_build_full_graphs_workspace(sd, G, out->cap_nodes, out->cap_edges)) return RENET_ERR_WORKSPACE;
    if ((uint64_t)cap_nodes * T2 >= (1ull << 31)) return RENET_ERR_UNSUPPORTED;      // the (dst, type) sort keys are 32 bits
    hipStream_t st = (hipStream_t)stream;
    FullStore S;
    S.node_ptr = sd->node_ptr; S.node_ent_all = sd->node_ent_all; S.trip_ptr = sd->trip_ptr;
    S.trip_ls = sd->trip_ls; S.trip_r = sd->trip_r; S.trip_lo = sd->trip_lo; S.T = sd->T; S.num_rels = sd->num_rels;

    Carver cv{reinterpret_cast<char*>(workspace), workspace_bytes};
    FullBufs bf;
    if (!bf.carve(cv, G, cap_nodes, cap_edges)) return RENET_ERR_WORKSPACE;
    int32_t* counts = out->counts;

    BB_HIP(hipMemsetAsync(counts, 0, RENET_BB_NCOUNTS * sizeof(int32_t), st));
    BB_HIP(hipMemsetAsync(bf.deg, 0, (size_t)(cap_nodes + 2) * sizeof(int32_t), st));
    BB_HIP(hipMemsetAsync(bf.tc, 0, bf.tc_bytes(), st));

    RENET_LAUNCH(fg_counts_kernel, dim3(1), dim3(1024), 0, st, S, tidx_dev, G, cap_nodes, out->cap_edges & ~1, bf.gti,
                 out->seg_ptr, bf.fact_off, counts);
    RENET_LAUNCH_CHECK();
    RENET_LAUNCH(fg_nodes_kernel, dim3((cap_nodes + 255) / 256), dim3(256), 0, st, S, counts, G, cap_nodes, bf.gti, out->seg_ptr,
                 out->node_ent);
    RENET_LAUNCH_CHECK();
    RENET_LAUNCH(fg_edges_kernel, dim3(min((cap_edges + 255) / 256, 1024)), dim3(256), 0, st, S, counts, G, cap_edges, key_bits,
                 bf.gti, out->seg_ptr, bf.fact_off, bf.src, bf.dst, bf.et, bf.key_dt, bf.key_t, bf.iota, bf.deg, bf.tc,
                 counts + RENET_BB_ERR);
    RENET_LAUNCH_CHECK();
    // only plan 0 (node_ent): a full-graph batch has no sequences
    return build_tail(bf, out, cap_nodes, cap_edges, 0, sd->num_ent, T2, key_bits, heavy_thr, group_items, chunk, 1, 0, false, st);
}

}  // extern "C"
