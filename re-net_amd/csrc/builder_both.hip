// Batch-graph builder ON THE DEVICE for the merged training batch (graph.build_batch_both; reference
// utils.py:209-244 get_sorted_s_r_embed_rgcn + utils.py:115-131 make_subgraph + dgl.batch, both directions of
// train.py:136-137 in one batch): the front of renet_build_batch_both.  From a batch of quadruple indices, over the
// resident quadruples, history index and graph store (RenetStoreDev): the length sort and the packed sequence layout
// (builder_tail.hip), then this file's own stages -- the per-(direction, timestamp) node sets, marked in a [slot][entity]
// byte table and numbered, and the node-induced edges; the tail (builder_tail.hip) takes over at the half edges.  The host
// uploads 4 KB of indices and reads back ~200 bytes of counts.  tests/test_gpu_builder.py compares every array with the
// host builder's.
#include "builder_common.h"

namespace {

// ---- stage C: slots (ONE workgroup): compact the used (direction, timestamp) pairs in (direction, time) order ----
__global__ __launch_bounds__(1024) void bb_slots_kernel(Store st, const int32_t* __restrict__ slot_used,
                                                        int32_t* __restrict__ slot_of_dense, int32_t* __restrict__ slot_ti,
                                                        int32_t* __restrict__ slot_group, int32_t* __restrict__ fact_off,
                                                        int32_t* __restrict__ counts) {
    __shared__ int wsum[16];
    __shared__ int s_tb;
    const int n = 2 * st.T;
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += 1024) {
        const int d = c0 + threadIdx.x;
        const int used = d < n ? slot_used[d] : 0;
        int tot;
        const int off = block_excl_scan_1024(used, &tot, wsum);
        if (used) {
            const int c = base + off;
            slot_of_dense[d] = c;
            slot_ti[c] = d % st.T;
            slot_group[c] = d / st.T;
        }
        base += tot;
    }
    if (threadIdx.x == 0) { s_tb = base; counts[RENET_BB_TB] = base; }
    __syncthreads();
    const int Tb = s_tb;
    base = 0;
    for (int c0 = 0; c0 < Tb; c0 += 1024) {              // fact offsets of the slots' timestamps
        const int c = c0 + threadIdx.x;
        int nf = 0;
        if (c < Tb) { const int ti = slot_ti[c]; nf = st.trip_ptr[ti + 1] - st.trip_ptr[ti]; }
        int tot;
        const int off = block_excl_scan_1024(nf, &tot, wsum);
        if (c < Tb) fact_off[c] = base + off;
        base += tot;
    }
    if (threadIdx.x == 0) { fact_off[Tb] = base; counts[RENET_BB_FACTS] = base; }
}

// ---- stage D: node marking: byte table [slot][entity]: bit 0 = in the node set, bit 1 = a subject (row prefix) ----
__device__ __forceinline__ void mark_byte(uint32_t* table, size_t key, uint32_t bits) {
    atomicOr(&table[key >> 2], bits << (8 * (key & 3)));
}

// one WAVE per step: lane-strided over the snapshot's neighbours
__global__ __launch_bounds__(256) void bb_mark_kernel(Store st, const int32_t* __restrict__ counts,
                                                      const int32_t* __restrict__ step_snap,
                                                      const int32_t* __restrict__ step_dense,
                                                      const int32_t* __restrict__ step_packed,
                                                      const int32_t* __restrict__ row_ent,
                                                      const int32_t* __restrict__ slot_of_dense,
                                                      uint32_t* __restrict__ table) {
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= counts[RENET_BB_S]) return;
    const int lane = threadIdx.x & 63;
    const int sv = step_snap[k], role = sv >> 30, snap = sv & 0x3FFFFFFF;
    const size_t base = (size_t)slot_of_dense[step_dense[k]] * st.num_ent;
    if (lane == 0) mark_byte(table, base + row_ent[step_packed[k]], 3u);
    const int b = st.snap_ptr[role][snap], e = st.snap_ptr[role][snap + 1];
    for (int n = b + lane; n < e; n += 64) mark_byte(table, base + st.nbr_o[role][n], 1u);
}

// ---- stage E: numbering: rows of the subject keys first (in key order), then the other keys (in key order) ----
constexpr int NUM_TILE = 4096;
__global__ __launch_bounds__(256) void bb_tile_count_kernel(const uint8_t* __restrict__ table, size_t entries_cap,
                                                            const int32_t* __restrict__ counts, int num_ent,
                                                            int2* __restrict__ tile_cnt) {
    __shared__ int ra[4], rb[4];
    const size_t entries = (size_t)counts[RENET_BB_TB] * num_ent;
    const size_t i0 = (size_t)blockIdx.x * NUM_TILE;
    int a = 0, b = 0;
    for (int u = threadIdx.x; u < NUM_TILE; u += 256) {
        const size_t i = i0 + u;
        if (i < entries && i < entries_cap) { const uint8_t v = table[i]; a += (v & 2) != 0; b += v == 1; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
    if ((threadIdx.x & 63) == 0) { ra[threadIdx.x >> 6] = a; rb[threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = make_int2(ra[0] + ra[1] + ra[2] + ra[3], rb[0] + rb[1] + rb[2] + rb[3]);
}

__global__ __launch_bounds__(1024) void bb_tile_scan_kernel(int2* __restrict__ tile_cnt, int n_tiles,
                                                            int32_t* __restrict__ counts, int cap_nodes,
                                                            int32_t* __restrict__ err) {
    __shared__ int wsum[16];
    int base_a = 0, base_b = 0;
    for (int c0 = 0; c0 < n_tiles; c0 += 1024) {
        const int c = c0 + threadIdx.x;
        const int2 v = c < n_tiles ? tile_cnt[c] : make_int2(0, 0);
        int ta, tb;
        const int oa = block_excl_scan_1024(v.x, &ta, wsum);
        const int ob = block_excl_scan_1024(v.y, &tb, wsum);
        if (c < n_tiles) tile_cnt[c] = make_int2(base_a + oa, base_b + ob);
        base_a += ta; base_b += tb;
    }
    if (threadIdx.x == 0) {
        const bool over = base_a + base_b > cap_nodes;
        if (over) atomicOr(err, RENET_BB_ERR_NODES);      // every later stage then sees an EMPTY graph (no OOB access)
        counts[RENET_BB_NA] = over ? 0 : base_a;
        counts[RENET_BB_N] = over ? 0 : base_a + base_b;
    }
}

__global__ __launch_bounds__(256) void bb_number_kernel(const uint8_t* __restrict__ table,
                                                        const int2* __restrict__ tile_off,
                                                        const int32_t* __restrict__ counts, int num_ent, int cap_nodes,
                                                        int32_t* __restrict__ new_id, int32_t* __restrict__ node_ent,
                                                        int32_t* __restrict__ node_slot) {
    __shared__ int wa[4], wb[4];
    const size_t entries = (size_t)counts[RENET_BB_TB] * num_ent;
    const int nA = counts[RENET_BB_NA];
    if (counts[RENET_BB_ERR] & RENET_BB_ERR_NODES) return;
    (void)cap_nodes;
    const size_t i0 = (size_t)blockIdx.x * NUM_TILE;
    if (i0 >= entries) return;
    const int2 toff = tile_off[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int run_a = toff.x, run_b = toff.y;
    // 16 rounds of 256 consecutive entries: order inside the tile = entry order
    for (int r = 0; r < NUM_TILE / 256; ++r) {
        const size_t i = i0 + (size_t)r * 256 + threadIdx.x;
        uint8_t v = 0;
        if (i < entries) v = table[i];
        const int fa = (v & 2) != 0, fb = v == 1;
        int ia = fa, ib = fb;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int ta = __shfl_up(ia, o), tb = __shfl_up(ib, o);
            if (lane >= o) { ia += ta; ib += tb; }
        }
        __syncthreads();
        if (lane == 63) { wa[wave] = ia; wb[wave] = ib; }
        __syncthreads();
        int pa = 0, pb = 0, ta = 0, tb = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) { pa += wa[w]; pb += wb[w]; }
            ta += wa[w]; tb += wb[w];
        }
        if (v) {
            const int id = fa ? run_a + pa + ia - 1 : nA + run_b + pb + ib - 1;
            new_id[i] = id;
            node_ent[id] = (int)(i % (size_t)num_ent);
            node_slot[id] = (int)(i / (size_t)num_ent);
        }
        run_a += ta; run_b += tb;
    }
}

// subject row of every step, in packed order
__global__ __launch_bounds__(256) void bb_subj_row_kernel(int num_ent, const int32_t* __restrict__ counts,
                                                          const int32_t* __restrict__ step_dense,
                                                          const int32_t* __restrict__ step_packed,
                                                          const int32_t* __restrict__ row_ent,
                                                          const int32_t* __restrict__ slot_of_dense,
                                                          const int32_t* __restrict__ new_id,
                                                          int32_t* __restrict__ subj_row) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= counts[RENET_BB_S]) return;
    const int p = step_packed[k];
    subj_row[p] = new_id[(size_t)slot_of_dense[step_dense[k]] * num_ent + row_ent[p]];
}

// ---- stage F: node-induced edges ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bb_fact_flag_kernel(Store st, const int32_t* __restrict__ counts,
                                                           const int32_t* __restrict__ fact_off,
                                                           const int32_t* __restrict__ slot_ti,
                                                           const uint8_t* __restrict__ table, int cap_facts,
                                                           int32_t* __restrict__ flag, int32_t* __restrict__ fslot) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= cap_facts) return;
    int keep = 0, c = 0;
    if (f < counts[RENET_BB_FACTS]) {
        const int Tb = counts[RENET_BB_TB];
        int lo = 0, hi = Tb;                              // last slot with fact_off <= f
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (fact_off[mid] <= f) lo = mid; else hi = mid; }
        c = lo;
        const int j = st.trip_ptr[slot_ti[c]] + (f - fact_off[c]);
        const size_t base = (size_t)c * st.num_ent;
        keep = (table[base + st.trip_s[j]] != 0) && (table[base + st.trip_o[j]] != 0);
    }
    flag[f] = keep;
    fslot[f] = c;
}

// both directions of every kept fact (utils.py:74-76): edge e < E2: ls -> lo with type r; e >= E2: lo -> ls with
// type r + R; the object-side member graphs (group 1) store type_o = (type_s + R) mod 2R (model.py:78).
// Also: sort keys, in-degree and relation histograms.
__global__ __launch_bounds__(256) void bb_edges_kernel(Store st, const int32_t* __restrict__ counts,
                                                       const int32_t* __restrict__ fact_off,
                                                       const int32_t* __restrict__ slot_ti,
                                                       const int32_t* __restrict__ slot_group,
                                                       const int32_t* __restrict__ flag, const int32_t* __restrict__ pos,
                                                       const int32_t* __restrict__ fslot,
                                                       const int32_t* __restrict__ new_id, int cap_facts, int cap_edges,
                                                       int32_t* __restrict__ half_src, int32_t* __restrict__ half_dst,
                                                       int32_t* __restrict__ half_et, int32_t* __restrict__ err) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= cap_facts || f >= counts[RENET_BB_FACTS] || !flag[f]) return;
    const int m = pos[f];
    if (m >= counts[RENET_BB_E2]) return;                  // (E2 was zeroed on overflow / error)
    (void)err; (void)cap_edges;
    const int c = fslot[f];
    const int j = st.trip_ptr[slot_ti[c]] + (f - fact_off[c]);
    const size_t base = (size_t)c * st.num_ent;
    half_src[m] = new_id[base + st.trip_s[j]];
    half_dst[m] = new_id[base + st.trip_o[j]];
    int t = st.trip_r[j];
    if (slot_group[c]) t += st.num_rels;                  // type_o of the forward edge
    half_et[m] = t;
}

// scratch of the merged front + the tail
struct Bufs : SeqBufs {
    int32_t *slot_of_dense, *slot_ti, *slot_group, *fact_off;
    uint32_t* table;
    int32_t* new_id;
    int2* tile_cnt;
    int32_t *flag, *pos, *fslot;
    // carves every scratch array out of `cv`; false if it does not fit
    bool carve(Carver& cv, const RenetStoreDev* sd, int B, int cap_nodes, int cap_edges) {
        const int cap_facts = 2 * sd->n_facts, cap_steps = 2 * B * BB_MAXL;
        const size_t entries_cap = (size_t)2 * sd->T * sd->num_ent;
        const int n_tiles = (int)((entries_cap + NUM_TILE - 1) / NUM_TILE);
        seq_first = cv.take<int32_t>(BB_MAXQ); seq_len_s = cv.take<int32_t>(BB_MAXQ); seq_start = cv.take<int32_t>(BB_MAXQ);
        step_snap = cv.take<int32_t>(cap_steps); step_dense = cv.take<int32_t>(cap_steps);
        step_packed = cv.take<int32_t>(cap_steps); slot_used = cv.take<int32_t>(2 * sd->T + 2);
        slot_of_dense = cv.take<int32_t>(2 * sd->T + 2);
        slot_ti = cv.take<int32_t>(2 * sd->T + 2);
        slot_group = cv.take<int32_t>(2 * sd->T + 2);
        fact_off = cv.take<int32_t>(2 * sd->T + 2);
        table = cv.take<uint32_t>(entries_cap / 4 + 16);
        new_id = cv.take<int32_t>(entries_cap);
        tile_cnt = cv.take<int2>(n_tiles + 1);
        flag = cv.take<int32_t>(cap_facts + 1);
        pos = cv.take<int32_t>(cap_facts + 1);
        fslot = cv.take<int32_t>(cap_facts + 1);
        half_src = cv.take<int32_t>(cap_edges / 2); half_dst = cv.take<int32_t>(cap_edges / 2); half_et = cv.take<int32_t>(cap_edges / 2);
        return carve_tail(cv, cap_nodes, cap_edges, cap_steps, cap_facts, true);
    }
};

}  // namespace

extern "C" {

size_t renet_build_batch_workspace(const RenetStoreDev* sd, int B, int cap_nodes, int cap_edges) {
    if (!sd || B <= 0 || cap_nodes <= 0 || cap_edges <= 0) return 0;
    return workspace_of<Bufs>(sd, B, cap_nodes, cap_edges & ~1);
}

int renet_build_batch_both(const RenetStoreDev* sd, const int32_t* idx_dev, int B, int seq_len, int heavy_thr,
                           int group_budget, int chunk, const RenetBatchOut* out, void* workspace,
                           size_t workspace_bytes, void* stream) {
    if (!sd || !out || !idx_dev || B <= 0 || 2 * B > BB_MAXQ || seq_len <= 0 || seq_len > BB_MAXL) return RENET_ERR_BADARG;
    const int cap_nodes = out->cap_nodes, cap_edges = out->cap_edges & ~1;
    int T2, key_bits;
    if (check_common(sd->num_rels, sd->T, heavy_thr, group_budget, chunk, cap_nodes, &T2, &key_bits)) return RENET_ERR_UNSUPPORTED;
    if (workspace_bytes < renet_build_batch_workspace(sd, B, out->cap_nodes, out->cap_edges)) return RENET_ERR_WORKSPACE;
    if ((uint64_t)cap_nodes * T2 >= (1ull << 31)) return RENET_ERR_UNSUPPORTED;      // the (dst, type) sort keys are 32 bits
    hipStream_t st = (hipStream_t)stream;
    Store S = fill_store(sd, sd->q_s, sd->q_r, sd->q_o);
    for (int r = 0; r < 2; ++r) {
        S.h_first[r] = sd->h_first[r]; S.h_count[r] = sd->h_count[r]; S.snap_t[r] = sd->snap_t[r];
        S.snap_ptr[r] = sd->snap_ptr[r]; S.nbr_o[r] = sd->nbr_o[r];
    }
    const int cap_facts = 2 * sd->n_facts, cap_steps = 2 * B * BB_MAXL;
    const size_t entries_cap = (size_t)2 * sd->T * sd->num_ent;
    const int n_tiles = (int)((entries_cap + NUM_TILE - 1) / NUM_TILE);

    Carver cv{reinterpret_cast<char*>(workspace), workspace_bytes};
    Bufs bf;
    if (!bf.carve(cv, sd, B, cap_nodes, cap_edges)) return RENET_ERR_WORKSPACE;
    int32_t* counts = out->counts;
    int32_t* err = counts + RENET_BB_ERR;

    BB_HIP(hipMemsetAsync(counts, 0, RENET_BB_NCOUNTS * sizeof(int32_t), st));
    BB_HIP(hipMemsetAsync(bf.slot_used, 0, (size_t)(2 * sd->T + 2) * sizeof(int32_t), st));
    BB_HIP(hipMemsetAsync(bf.table, 0, entries_cap + 64, st));
    BB_HIP(hipMemsetAsync(bf.deg, 0, (size_t)(cap_nodes + 2) * sizeof(int32_t), st));
    BB_HIP(hipMemsetAsync(bf.tc, 0, bf.tc_bytes(), st));

    // A, B: length sort and steps of the 2B sequences (subject side, then object side)
    if (int rc = launch_seq_steps(&S, idx_dev, B, 2 * B, seq_len, out, bf, out->rel_label, out->ent_label, st)) return rc;
    // C, D, E: slots, node marking, numbering
    RENET_LAUNCH(bb_slots_kernel, dim3(1), dim3(1024), 0, st, S, bf.slot_used, bf.slot_of_dense, bf.slot_ti, bf.slot_group, bf.fact_off,
                 counts);
    RENET_LAUNCH_CHECK();
    RENET_LAUNCH(bb_mark_kernel, dim3((cap_steps + 3) / 4), dim3(256), 0, st, S, counts, bf.step_snap, bf.step_dense,
                 bf.step_packed, out->row_ent, bf.slot_of_dense, bf.table);
    RENET_LAUNCH_CHECK();
    RENET_LAUNCH(bb_tile_count_kernel, dim3(n_tiles), dim3(256), 0, st, (const uint8_t*)bf.table, entries_cap, counts,
                 sd->num_ent, bf.tile_cnt);
    RENET_LAUNCH_CHECK();
    RENET_LAUNCH(bb_tile_scan_kernel, dim3(1), dim3(1024), 0, st, bf.tile_cnt, n_tiles, counts, cap_nodes, err);
    RENET_LAUNCH_CHECK();
    RENET_LAUNCH(bb_number_kernel, dim3(n_tiles), dim3(256), 0, st, (const uint8_t*)bf.table, bf.tile_cnt, counts, sd->num_ent,
                 cap_nodes, bf.new_id, out->node_ent, out->node_slot);
    RENET_LAUNCH_CHECK();
    RENET_LAUNCH(bb_subj_row_kernel, dim3((cap_steps + 255) / 256), dim3(256), 0, st, sd->num_ent, counts, bf.step_dense,
                 bf.step_packed, out->row_ent, bf.slot_of_dense, bf.new_id, out->subj_row);
    RENET_LAUNCH_CHECK();
    // F: induced edges
    RENET_LAUNCH(bb_fact_flag_kernel, dim3((cap_facts + 255) / 256), dim3(256), 0, st, S, counts, bf.fact_off, bf.slot_ti,
                 (const uint8_t*)bf.table, cap_facts, bf.flag, bf.fslot);
    RENET_LAUNCH_CHECK();
    if (int rc = scan_set_e2(bf, bf.flag, bf.pos, counts, counts + RENET_BB_FACTS, cap_facts, cap_edges, st)) return rc;
    RENET_LAUNCH(bb_edges_kernel, dim3((cap_facts + 255) / 256), dim3(256), 0, st, S, counts, bf.fact_off, bf.slot_ti,
                 bf.slot_group, bf.flag, bf.pos, bf.fslot, bf.new_id, cap_facts, cap_edges, bf.half_src, bf.half_dst, bf.half_et, err);
    RENET_LAUNCH_CHECK();
    return finish_batch(bf, out, cap_nodes, cap_edges, cap_steps, sd->num_ent, sd->num_rels, key_bits, heavy_thr, group_budget,
                        chunk, 2 * B, st);
}

}  // extern "C"
