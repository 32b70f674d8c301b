// =================================================================================================
// Item-stream gather (renet_rgcn_gather_items): the row-group kernel of rgcn_csr.hip walks CSR rows and pays one
// dependent load chain per row boundary (the epilogue's self-loop addend is fetched only when the row
// is flushed) on top of {row_ptr} -> {indices} -> {rows}: 16+ serialised memory latencies per wave and
// 91-105 VGPRs (4-5 waves per SIMD, a 2048-block launch needs two rounds) -- latency-, not bandwidth-bound.
//
// Here the host planner (graph.plan_gather_items) linearises the light rows (in-degree <= heavy_thresh) into
// ONE item stream: the in-edges of row v as (source row, edge type) followed by a FLUSH item (v, -1), cut
// into groups of <= 64 items (balanced by item count, never straddling the pruned-layer row prefix).  A wave
// takes one group: one coalesced fetch brings all of its items, then the items go through the load pipe
// UNR at a time -- an edge item loads the source row + its relation blocks, a flush item loads the row's
// self-loop addend and norm -- so the addend is just another in-flight load and nothing in the loop depends on
// anything but the item registers.  Chain per wave: {group bounds} -> {items} -> ceil(n/UNR) batches.
// Hub rows (in-degree > heavy_thresh) are not in the stream: the first n_heavy workgroups of the launch reduce
// one each with all their waves (longest work first), prefetching 64 edge indices per coalesced fetch.
// Every branch is wave-uniform; no atomics; results do not depend on the launch geometry.
// =================================================================================================
#include "rgcn_common.h"

namespace {

struct ItemArgs {
    GatherArgs g;
    const int32_t* it_src;      // item stream: source row of an edge item / destination row of a flush item
    const int32_t* it_type;     // edge type (type_s) or -1 for a flush item
    const int32_t* grp_ptr;     // [n_groups + 1] item offsets of the groups
    int n_groups;
};

// the WCH float4 of one lane's relation-block slice: fp32 (16 WCH bytes at wo; 12 WCH at SI = 3) or bf16 (8 WCH bytes at wo)
template <int WCH, bool B16>
__device__ __forceinline__ void load_wblock(__amdgpu_buffer_rsrc_t rw, uint32_t wo, uint32_t ws, float4 (&w)[WCH]) {
    static_assert(!(B16 && WCH == 3), "no bf16 storage of 3x3 relation blocks");
    if constexpr (!B16) {
        constexpr int VW = vw_of<WCH>();
#pragma unroll
        for (int q = 0; q < WCH; ++q) w[q] = buf_loadvs<VW>(rw, wo + (4u * VW) * q, ws);
    } else if constexpr (WCH == 1) {
        w[0] = buf_load4s_bf16(rw, wo, ws);
    } else {
#pragma unroll
        for (int q = 0; q < WCH / 2; ++q) {
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rw, (int)(wo + 16u * q), (int)ws, 0);
            w[2 * q] = make_float4(bf_lo(v.x), bf_hi(v.x), bf_lo(v.y), bf_hi(v.y));
            w[2 * q + 1] = make_float4(bf_lo(v.z), bf_hi(v.z), bf_lo(v.w), bf_hi(v.w));
        }
    }
}

constexpr int kItemFlush = -1;   // it_type of a flush item
constexpr int kItemNop = -2;     // lanes past the end of a group
// it_type <= kItemFlushMap: a flush item whose self-loop addend lives in row (kItemFlushMap - it_type) of the addend
// tensor instead of row it_src (layer 1 on the entity table: addend = (ent_embeds @ W_loop)[entity of the row])
constexpr int kItemFlushMap = -3;

template <int SI, int NCH, bool TR>
__device__ __forceinline__ void row_epilogue(const GatherArgs& g, int row, bool has_ad, float sc, int lane,
                                             const float4 (&acc)[NCH], const float4 (&ad)[NCH]) {
    constexpr int D = 100 * SI, VW = vw_of<SI>();
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(g.out + (size_t)row * D, D * 4);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int ch = lane + 64 * c;
        float4 o = f4_scale(acc[c], sc);
        if (has_ad) o = f4_add(o, f4_mul(ad[c], drop_chunk<VW, D>(g.drop, (uint64_t)row, ch)));
        if (g.relu) {
            o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f);
        }
        buf_storev<VW>(ro, (uint32_t)ch * (4u * VW), o);     // lanes past the row: out of range => dropped
    }
}

// COMPACT (the pruned backward launch, round 4): that launch walks the item stream of ALL rows for the edges whose source
// lies in the row prefix (src < src_limit: 150 k of the 268 k edges of the bench batch), and a skipped edge still
// occupied one of the UNR slots of a batch (no memory traffic, but a third of the loop iterations).  The wave now
// ballots which of its <= 64 items are live (flush items always; edges by their source) and pops the set bits of that
// mask instead of counting 0..n: only live items reach the load pipe; order, and therefore the result, is unchanged.
template <int SI, int NCH, int UNR, bool TR, int MX, bool COMPACT = false>
__device__ __forceinline__ void gather_item_group(const ItemArgs& a, int grp) {
    constexpr bool XB = MX == 2, WB = MX >= 1;
    constexpr int D = 100 * SI;
    constexpr int VW = vw_of<SI>();
    constexpr uint32_t CB = 4u * VW;                     // bytes of one fp32 chunk
    constexpr int CH = D / VW;
    constexpr int WCH = SI;
    constexpr uint32_t ROWB = D * 4;                     // bytes of one fp32 feature row (addend, output)
    const uint32_t XROWB = a.g.x_rowb;                   // bytes of one row of x (fp32: ROWB; bf16: 2 * its row stride)
    const uint32_t WROWB = a.g.w_rowb;                   // bytes of one relation's blocks
    const int lane = threadIdx.x & 63;
    const GatherArgs& g = a.g;
    const int i0 = a.grp_ptr[grp];
    const int n = a.grp_ptr[grp + 1] - i0;               // <= 64 by construction of the plan
    int my_src = 0, my_t = kItemNop;
    if (lane < n) { my_src = a.it_src[i0 + lane]; my_t = a.it_type[i0 + lane]; }
    // pin the wait for the item fetch HERE: left to the compiler it becomes an `s_waitcnt vmcnt(0)` at the loop
    // header, which from the second batch on also waits for the previous batch's output stores
    asm volatile("" : "+v"(my_src), "+v"(my_t));
    const float* sp = g.scale ? g.scale : g.x;           // always a readable address
    // whole-tensor descriptors (kernel arguments => provably wave-uniform, no waterfall loops); the row goes into
    // the scalar offset, the lane into the vector offset; kOob in the vector offset = "do not load, return 0"
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(g.x, kBufSpan);
    const __amdgpu_buffer_rsrc_t rad = make_rsrc(g.addend ? g.addend : g.x, kBufSpan);
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(g.W, kBufSpan);
    uint32_t xoff[NCH], woff[NCH], aoff[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const uint32_t ch = (uint32_t)(lane + 64 * c);
        xoff[c] = ch < (uint32_t)CH ? ch * (XB ? 8u : CB) : kOob;
        aoff[c] = ch < (uint32_t)CH ? ch * CB : kOob;                  // the addend is always fp32
        woff[c] = ch < (uint32_t)CH ? ch * ((WB ? 8u : CB) * WCH) : kOob;
    }
    float4 acc[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);

    unsigned long long live = 0ull;
    if constexpr (COMPACT) live = __builtin_amdgcn_ballot_w64(lane < n && (my_t < 0 || my_src < g.src_limit));
    for (int k = 0; COMPACT ? live != 0ull : k < n; k += UNR) {
        float4 xv[UNR][NCH];
        float4 wv[UNR][NCH][WCH];
        float scv[UNR];
        int pick[UNR];                                   // item index of slot u (63 + "nop" when the batch runs short)
        bool have[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            if constexpr (COMPACT) {
                have[u] = live != 0ull;
                pick[u] = have[u] ? __builtin_ctzll(live) : 63;
                live &= live - 1ull;                     // (0 stays 0)
            } else {
                have[u] = (k + u) < n;
                pick[u] = min(k + u, 63);
            }
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int idx = pick[u];
            const int src = __builtin_amdgcn_readlane(my_src, idx);            // wave-uniform (SGPR)
            const int t = have[u] ? __builtin_amdgcn_readlane(my_t, idx) : kItemNop;       // (n may be 64)
            const bool edge = t >= 0 && src < g.src_limit;
            const bool flush = t == kItemFlush || t <= kItemFlushMap;
            const bool flush_ad = flush && g.addend != nullptr && src < g.addend_rows;
            int tt = t + g.shift;
            if (tt >= g.T) tt -= g.T;
            const int ldrow = t <= kItemFlushMap ? kItemFlushMap - t : src;      // row the x / addend load reads
            const uint32_t xs = edge ? (uint32_t)ldrow * XROWB : flush_ad ? (uint32_t)ldrow * ROWB : 0u;
            const uint32_t ws = edge ? (uint32_t)tt * WROWB : 0u;
            scv[u] = sp[flush ? src : 0];
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                // an item that loads nothing gets the out-of-range vector offset (a per-item descriptor with
                // num_records = 0 would do the same in SGPRs, but costs 4 SGPRs per load in flight: > 96 SGPRs
                // and one wave per SIMD less)
                const uint32_t wo = edge ? woff[c] : kOob;
                if constexpr (!XB) {
                    const uint32_t xo = (edge || flush_ad) ? xoff[c] : kOob;
                    xv[u][c] = flush_ad ? buf_loadvs<VW>(rad, xo, xs) : buf_loadvs<VW>(rx, xo, xs);
                } else {
                    // bf16 source rows and fp32 addend rows differ in load width: two unconditional loads, the one that
                    // does not apply gets the out-of-range offset (no memory access); exactly one of them is non-zero
                    const float4 xe = buf_load4s_bf16(rx, edge ? xoff[c] : kOob, xs);
                    const float4 xa = buf_load4s(rad, flush_ad ? aoff[c] : kOob, xs);
                    xv[u][c] = f4_add(xe, xa);
                }
                load_wblock<WCH, WB>(rw, wo, ws, wv[u][c]);
            }
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int idx = pick[u];
            const int src = __builtin_amdgcn_readlane(my_src, idx);
            const int t = have[u] ? __builtin_amdgcn_readlane(my_t, idx) : kItemNop;
            if (t >= 0) {                                     // (a skipped edge multiplied zeros: harmless)
#pragma unroll
                for (int c = 0; c < NCH; ++c) blockmul<SI, TR>(xv[u][c], wv[u][c], acc[c]);
            } else if (t == kItemFlush || t <= kItemFlushMap) {
                const bool has_ad = g.addend != nullptr && src < g.addend_rows;
                row_epilogue<SI, NCH, TR>(g, src, has_ad, g.scale ? scv[u] : 1.f, lane, acc, xv[u]);
#pragma unroll
                for (int c = 0; c < NCH; ++c) acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    }
}

// One workgroup per hub row: 64 edge indices per coalesced fetch, wave w takes entries w, w + WAVES, ... of
// the window UNR at a time (unconditional buffer loads as above); wave 0 prefetches the row's addend;
// fixed-order LDS combine => deterministic.
template <int SI, int NCH, int UNR, bool TR, int WAVES, int MX, bool COMPACT = false>
__device__ __forceinline__ void gather_hub_row(const GatherArgs& a, int v) {
    constexpr bool XB = MX == 2, WB = MX >= 1;
    constexpr int D = 100 * SI;
    constexpr int VW = vw_of<SI>();
    constexpr uint32_t CB = 4u * VW;
    constexpr int CH = D / VW;
    constexpr int WCH = SI;
    constexpr uint32_t ROWB = D * 4;
    const uint32_t XROWB = a.x_rowb, WROWB = a.w_rowb;
    __shared__ float4 red[WAVES][CH];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int e0 = a.row_ptr[v], e1 = a.row_ptr[v + 1];
    const bool has_ad = a.addend != nullptr && v < a.addend_rows;
    const int adrow = (has_ad && a.row_map) ? a.row_map[v] : v;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.x, kBufSpan);
    const __amdgpu_buffer_rsrc_t rad = make_rsrc(a.addend ? a.addend : a.x, kBufSpan);
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(a.W, kBufSpan);
    uint32_t xoff[NCH], woff[NCH];
    float4 adv[NCH];
    float4 acc[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const uint32_t ch = (uint32_t)(lane + 64 * c);
        xoff[c] = ch < (uint32_t)CH ? ch * (XB ? 8u : CB) : kOob;
        woff[c] = ch < (uint32_t)CH ? ch * ((WB ? 8u : CB) * WCH) : kOob;
        acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        adv[c] = buf_loadvs<VW>(rad, (has_ad && wave == 0 && ch < (uint32_t)CH) ? ch * CB : kOob,
                            has_ad ? (uint32_t)adrow * ROWB : 0u);
    }
    for (int base = e0; base < e1; base += 64) {
        const int cnt = min(64, e1 - base);
        int my_col = 0x7fffffff, my_t = 0;
        if (lane < cnt) {
            my_col = a.col[base + lane];
            my_t = a.etype[base + lane] + a.shift;
            if (my_t >= a.T) my_t -= a.T;
        }
        // COMPACT (pruned backward): only the window's LIVE edges (source inside the row prefix) are dealt to the waves --
        // lane l's rank among the live lanes is mbcnt(live); wave w takes ranks w, w + WAVES, ...; the lane holding a
        // rank is found with one ballot.  Otherwise: entries w, w + WAVES, ... of the window, skipped ones included.
        const bool lv = COMPACT && lane < cnt && my_col < a.src_limit;
        const unsigned long long live = COMPACT ? __builtin_amdgcn_ballot_w64(lv) : 0ull;
        const int rank = COMPACT ? (int)__builtin_amdgcn_mbcnt_hi((unsigned)(live >> 32),
                                                                 __builtin_amdgcn_mbcnt_lo((unsigned)live, 0u)) : 0;
        const int n_walk = COMPACT ? __builtin_popcountll(live) : cnt;
        for (int k = wave; k < n_walk; k += WAVES * UNR) {
            float4 xv[UNR][NCH];
            float4 wv[UNR][NCH][WCH];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                int kk;
                bool in_walk = (k + u * WAVES) < n_walk;
                if constexpr (COMPACT) {
                    const unsigned long long sel = __builtin_amdgcn_ballot_w64(lv && rank == k + u * WAVES);
                    kk = sel ? __builtin_ctzll(sel) : 63;
                    in_walk = sel != 0ull;
                } else {
                    kk = min(k + u * WAVES, 63);
                }
                const int src = __builtin_amdgcn_readlane(my_col, kk);      // lanes >= cnt hold INT_MAX => skipped
                const int t = __builtin_amdgcn_readlane(my_t, kk);
                const bool ok = in_walk && src < a.src_limit;
                const uint32_t xs = ok ? (uint32_t)src * XROWB : 0u;
                const uint32_t ws = ok ? (uint32_t)t * WROWB : 0u;
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    if constexpr (XB) xv[u][c] = buf_load4s_bf16(rx, ok ? xoff[c] : kOob, xs);
                    else xv[u][c] = buf_loadvs<VW>(rx, ok ? xoff[c] : kOob, xs);
                    load_wblock<WCH, WB>(rw, ok ? woff[c] : kOob, ws, wv[u][c]);
                }
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
#pragma unroll
                for (int c = 0; c < NCH; ++c) blockmul<SI, TR>(xv[u][c], wv[u][c], acc[c]);   // zeros when skipped
            }
        }
    }
    if (wave != 0) {
#pragma unroll
        for (int c = 0; c < NCH; ++c)
            if (lane + 64 * c < CH) red[wave][lane + 64 * c] = acc[c];
    }
    __syncthreads();
    if (wave == 0) {
        const float sc = a.scale ? a.scale[v] : 1.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int ch = lane + 64 * c;
            if (ch < CH) {
#pragma unroll
                for (int w = 1; w < WAVES; ++w) acc[c] = f4_add(acc[c], red[w][ch]);
            }
        }
        row_epilogue<SI, NCH, TR>(a, v, has_ad, sc, lane, acc, adv);
    }
}

template <int SI, int NCH, int UNR, bool TR, int MX, bool COMPACT = false>
__device__ __forceinline__ void gather_items_body(const ItemArgs& a) {
    if ((int)blockIdx.x < a.g.n_heavy) {
        gather_hub_row<SI, NCH, UNR, TR, kWaves, MX, COMPACT>(a.g, a.g.heavy[blockIdx.x]);
        return;
    }
    const int nb = gridDim.x - a.g.n_heavy;
    const int vb = renet_xcd_block(blockIdx.x - a.g.n_heavy, nb);
    const int grp = vb * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // neighbouring rows share an XCD
    if (grp < a.n_groups) gather_item_group<SI, NCH, UNR, TR, MX, COMPACT>(a, grp);
}

// Four entry kernels with distinct names so that a rocprof kernel trace separates the launch classes of a
// training step: forward over the full batch graph (layer 1), forward over the subject-row prefix (layer 2),
// and their backward-wrt-h counterparts (transposed relation blocks).
#define RENET_GATHER_KERNEL(NAME, TRV, COMPACTV)                                                                       \
    template <int SI, int NCH, int UNR, int MX = 0>                                                                    \
    __global__ __launch_bounds__(kThreads) void NAME(ItemArgs a) { gather_items_body<SI, NCH, UNR, TRV, MX, COMPACTV>(a); }
RENET_GATHER_KERNEL(rgcn_gather_fwd_full, false, false)
RENET_GATHER_KERNEL(rgcn_gather_fwd_pruned, false, false)
RENET_GATHER_KERNEL(rgcn_gather_bwdh_full, true, false)
RENET_GATHER_KERNEL(rgcn_gather_bwdh_pruned, true, true)       // the only class with a source limit: compacted item walk
#undef RENET_GATHER_KERNEL

template <int SI, int NCH, int UNR, int MX = 0>
int launch_gather_items(const ItemArgs& a, bool tr, bool pruned, hipStream_t st) {
    int blocks = (a.n_groups + kWaves - 1) / kWaves;
    blocks = max(8, (blocks + 7) & ~7);                    // multiple of 8 for the XCD remap
    const dim3 grid(blocks + a.g.n_heavy), blk(kThreads);  // hub rows first, then the groups, in ONE launch
    if (!tr && !pruned) RENET_LAUNCH((rgcn_gather_fwd_full<SI, NCH, UNR, MX>), grid, blk, 0, st, a);
    else if (!tr) RENET_LAUNCH((rgcn_gather_fwd_pruned<SI, NCH, UNR, MX>), grid, blk, 0, st, a);
    else if (!pruned) RENET_LAUNCH((rgcn_gather_bwdh_full<SI, NCH, UNR, MX>), grid, blk, 0, st, a);
    else RENET_LAUNCH((rgcn_gather_bwdh_pruned<SI, NCH, UNR, MX>), grid, blk, 0, st, a);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}

// edges in flight per wave (tuning knob, read once): RENET_GATHER_UNR in {2, 3, 4, 6, 8}; 0 / unset, or a value the
// width has no instantiation for (gather_items_impl: 6 and 8 exist at D = 100 / 200 only) = that width's default
int gather_unr() {
    static const int v = renet_env_int("RENET_GATHER_UNR", 0, 0, 8);
    return v;
}

// ---- index composition for the table-addressed first layer --------------------------------------------
__global__ __launch_bounds__(256) void compose_table_items_kernel(const int32_t* __restrict__ row_map,
                                                                  const int32_t* __restrict__ it_src,
                                                                  const int32_t* __restrict__ it_type, int n_items,
                                                                  const int32_t* __restrict__ col,
                                                                  const int32_t* __restrict__ e_src, int E,
                                                                  int32_t* __restrict__ it_src_t,
                                                                  int32_t* __restrict__ it_type_t,
                                                                  int32_t* __restrict__ col_t,
                                                                  int32_t* __restrict__ e_src_t) {
    const int total = n_items + 2 * E;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        if (i < n_items) {
            const int s = it_src[i], t = it_type[i];
            if (t >= 0) { it_src_t[i] = row_map[s]; it_type_t[i] = t; }            // edge item: source -> table row
            else if (t == -1) { it_src_t[i] = s; it_type_t[i] = -3 - row_map[s]; }  // flush: keep the output row, carry
            else { it_src_t[i] = s; it_type_t[i] = t; }                            //        its table row in the type
        } else if (i < n_items + E) {
            col_t[i - n_items] = row_map[col[i - n_items]];
        } else {
            e_src_t[i - n_items - E] = row_map[e_src[i - n_items - E]];
        }
    }
}

// the launch with UNR = the knob's value where it is one of ALT..., else the width's default DFLT
template <int SI, int DFLT, int... ALT>
int launch_items_unr(int unr, const ItemArgs& a, bool tr, bool pruned, hipStream_t st) {
    int rc = RENET_OK;
    const bool hit = ((unr == ALT && (rc = launch_gather_items<SI, nch_of<SI>(), ALT>(a, tr, pruned, st), true)) || ...);
    return hit ? rc : launch_gather_items<SI, nch_of<SI>(), DFLT>(a, tr, pruned, st);
}

// `a`: filled by the entry (the item stream, gather_fill, row_map).  mx = 0: fp32 operands; bf16 storage: mx = 1: W is a
// bf16 matrix with row stride w_ld elements; mx = 2: x (a table) too, row stride x_ld.  x_rows: rows of x.
int gather_items_impl(ItemArgs& a, int D, float drop_p, int mx, int x_ld, int w_ld, int x_rows, bool tr, bool pruned,
                      hipStream_t st) {
    if (const int rc = gather_check(D, a.g, drop_p)) return rc;
    if (a.n_groups < 0) return RENET_ERR_BADARG;
    if (a.g.N == 0 || (a.n_groups == 0 && a.g.n_heavy == 0)) return RENET_OK;
    // 32-bit buffer offsets with the skip marker at the span (kBufSpan / kOob): tensors must stay below 2 GiB
    const size_t span = (size_t)1 << 31, fb = sizeof(float);
    if ((size_t)max(a.g.N, x_rows) * D * fb >= span || (size_t)a.g.T * D * (D / 100) * fb >= span) return RENET_ERR_UNSUPPORTED;
    if (mx < 0 || mx > 2 || (mx >= 1 && w_ld < D * (D / 100)) || (mx == 2 && x_ld < D)) return RENET_ERR_BADARG;
    if (mx != 0 && D == 300) return RENET_ERR_UNSUPPORTED;      // no bf16 storage of 3x3 blocks
    a.g.heavy_thresh = 0;
    a.g.x_rowb = mx == 2 ? (uint32_t)x_ld * 2u : (uint32_t)D * 4u;
    a.g.w_rowb = mx >= 1 ? (uint32_t)w_ld * 2u : (uint32_t)D * (D / 100) * 4u;
    const int unr = gather_unr();
    return with_si(D, [&](auto si) -> int {
        constexpr int SI = decltype(si)::value;
        constexpr int NCH = nch_of<SI>(), UNR = SI == 1 ? 6 : SI == 2 ? 3 : 2;     // UNR: the width's default
        if constexpr (SI != 3) {
            if (mx == 1) return launch_gather_items<SI, NCH, UNR, 1>(a, tr, pruned, st);
            if (mx == 2) return launch_gather_items<SI, NCH, UNR, 2>(a, tr, pruned, st);
        }
        // fp32 operands: the knob's variants (defaults: 60 VGPRs, 8 waves per SIMD at D = 200; 87-91, 5 waves at D = 300)
        if constexpr (SI == 1) return launch_items_unr<SI, UNR, 4, 8>(unr, a, tr, pruned, st);
        else if constexpr (SI == 2) return launch_items_unr<SI, UNR, 2, 4, 6, 8>(unr, a, tr, pruned, st);
        else return launch_items_unr<SI, UNR, 3, 4>(unr, a, tr, pruned, st);
    });
}

}  // namespace

extern "C" {

int renet_rgcn_gather_items(const float* x, int D, const int32_t* it_src, const int32_t* it_type,
                            const int32_t* grp_ptr, int n_groups, const int32_t* row_ptr, const int32_t* col,
                            const int32_t* etype, const float* scale, const float* W, int T, int type_shift,
                            int transpose_w, const float* addend, float drop_p, uint64_t seed, int relu,
                            float* out, int N, const int32_t* heavy_rows, int n_heavy, int src_limit,
                            int addend_rows, int pruned, void* stream) {
    ItemArgs a{{}, it_src, it_type, grp_ptr, n_groups};
    gather_fill(a.g, x, row_ptr, col, etype, scale, W, T, type_shift, addend, drop_p, seed, relu, out, N, heavy_rows,
                n_heavy, src_limit, addend_rows);
    return gather_items_impl(a, D, drop_p, 0, 0, 0, N, transpose_w != 0, pruned != 0, (hipStream_t)stream);
}

int renet_rgcn_gather_items_bf16(const float* x, int D, const int32_t* it_src, const int32_t* it_type,
                                 const int32_t* grp_ptr, int n_groups, const int32_t* row_ptr, const int32_t* col,
                                 const int32_t* etype, const float* scale, const void* W_bf16, int w_ld, int T,
                                 int type_shift, int transpose_w, const float* addend, float drop_p, uint64_t seed,
                                 int relu, float* out, int N, const int32_t* heavy_rows, int n_heavy, int src_limit,
                                 int addend_rows, int pruned, void* stream) {
    ItemArgs a{{}, it_src, it_type, grp_ptr, n_groups};
    gather_fill(a.g, x, row_ptr, col, etype, scale, (const float*)W_bf16, T, type_shift, addend, drop_p, seed, relu, out, N,
                heavy_rows, n_heavy, src_limit, addend_rows);
    return gather_items_impl(a, D, drop_p, 1, 0, w_ld, N, transpose_w != 0, pruned != 0, (hipStream_t)stream);
}

int renet_rgcn_gather_items_table(const float* table, int table_rows, int D, const int32_t* it_src_t,
                                  const int32_t* it_type_t, const int32_t* grp_ptr, int n_groups,
                                  const int32_t* row_ptr, const int32_t* col_t, const int32_t* etype,
                                  const int32_t* row_map, const float* scale, const float* W, int T, int type_shift,
                                  const float* addend_table, float drop_p, uint64_t seed, int relu, float* out, int N,
                                  const int32_t* heavy_rows, int n_heavy, void* stream) {
    if (!row_map || table_rows <= 0) return RENET_ERR_BADARG;
    ItemArgs a{{}, it_src_t, it_type_t, grp_ptr, n_groups};
    gather_fill(a.g, table, row_ptr, col_t, etype, scale, W, T, type_shift, addend_table, drop_p, seed, relu, out, N,
                heavy_rows, n_heavy, 0, 0);
    a.g.row_map = row_map;
    return gather_items_impl(a, D, drop_p, 0, 0, 0, table_rows, false, false, (hipStream_t)stream);
}

int renet_rgcn_gather_items_table_bf16(const void* table_bf16, int table_ld, int table_rows, int D,
                                       const int32_t* it_src_t, const int32_t* it_type_t, const int32_t* grp_ptr,
                                       int n_groups, const int32_t* row_ptr, const int32_t* col_t, const int32_t* etype,
                                       const int32_t* row_map, const float* scale, const void* W_bf16, int w_ld, int T,
                                       int type_shift, const float* addend_table, float drop_p, uint64_t seed, int relu,
                                       float* out, int N, const int32_t* heavy_rows, int n_heavy, void* stream) {
    if (!row_map || table_rows <= 0) return RENET_ERR_BADARG;
    ItemArgs a{{}, it_src_t, it_type_t, grp_ptr, n_groups};
    gather_fill(a.g, (const float*)table_bf16, row_ptr, col_t, etype, scale, (const float*)W_bf16, T, type_shift,
                addend_table, drop_p, seed, relu, out, N, heavy_rows, n_heavy, 0, 0);
    a.g.row_map = row_map;
    return gather_items_impl(a, D, drop_p, 2, table_ld, w_ld, table_rows, false, false, (hipStream_t)stream);
}

int renet_compose_table_items(const int32_t* row_map, const int32_t* it_src, const int32_t* it_type, int n_items,
                              const int32_t* col, const int32_t* e_src, int E, int32_t* it_src_t,
                              int32_t* it_type_t, int32_t* col_t, int32_t* e_src_t, void* stream) {
    if (n_items < 0 || E < 0 || !row_map) return RENET_ERR_BADARG;
    const int total = n_items + 2 * E;
    if (total == 0) return RENET_OK;
    RENET_LAUNCH(compose_table_items_kernel, dim3(min(2048, (total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                 row_map, it_src, it_type, n_items, col, e_src, E, it_src_t, it_type_t, col_t, e_src_t);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}

}  // extern "C"
