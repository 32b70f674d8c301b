// The plain-CSR gather-SpMM (renet_rgcn_gather): destination rows walked in groups of 8 straight from row_ptr / col / etype,
// 64-bit addressing.  In production the fallback of the item-stream gather (rgcn_items.hip) for tensors of 2 GiB and more.
#include "rgcn_common.h"

namespace {

template <int SI>
__device__ __forceinline__ void gather_epilogue(const GatherArgs& a, int v, int ch, float4 o, float sc) {
    constexpr int VW = vw_of<SI>(), D = 100 * SI, CH = D / VW;
    o = f4_scale(o, sc);
    if (a.addend && v < a.addend_rows) {
        float4 ad = ld_chunk<VW>(a.addend, (size_t)v * CH + ch);
        if constexpr (VW == 4) ad = f4_mul(ad, renet_drop4(a.drop, (uint64_t)v * CH + ch));
        else ad = f4_mul(ad, drop_chunk<VW, D>(a.drop, (uint64_t)v, ch));
        o = f4_add(o, ad);
    }
    if (a.relu) {
        o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f);
    }
    st_chunk<VW>(a.out, (size_t)v * CH + ch, o);
}

// SI = D/100 (relation block size); NCH = float4 chunks per lane = ceil(D/4/64); UNR = edges whose
// operand loads are in flight together.
//
// A wave owns a GROUP of R = 8 consecutive destination rows: one coalesced fetch brings the group's
// row_ptr slice (and norm), one more the source/type indices of its in-edges (rows are short: the
// group's CSR segment is ~20-40 contiguous edges), so the dependent-load chain is
// {row_ptr} -> {indices} -> {source rows + relation blocks} for 8 rows at once instead of per row.
// Edges are walked in CSR order in batches of UNR with all UNR source-row / weight loads issued
// before the first FMA; a row is flushed (norm, +self-loop addend with dropout, ReLU, store) when the
// walk crosses its row_ptr boundary.  Hub rows (in-degree > heavy_thresh; a Zipf tail of a few hundred
// rows with up to ~300 in-edges) would serialise one wave for the whole launch, so they are skipped
// by the row-group walk and reduced by a whole workgroup each (gather_heavy_row, same launch).  Everything that steers
// control flow is wave-uniform (SGPR).
template <int SI, int NCH, int UNR, bool TR>
__device__ __forceinline__ void gather_heavy_row(const GatherArgs& a, int v);

template <int SI, int NCH, int UNR, bool TR>
__global__ __launch_bounds__(kThreads) void rgcn_gather_kernel(GatherArgs a) {
    constexpr int D = 100 * SI;
    constexpr int VW = vw_of<SI>();         // floats per chunk
    constexpr int CH = D / VW;              // chunks per feature row
    constexpr int WCH = SI;                 // weight loads per chunk
    constexpr int WROW4 = D * SI / 4;       // float4 per relation weight row
    constexpr int R = 8;                    // rows per group
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    // the first n_heavy workgroups of the launch each reduce one hub row (longest work items first);
    // the rest walk row groups
    if ((int)blockIdx.x < a.n_heavy) {
        gather_heavy_row<SI, NCH, UNR, TR>(a, a.heavy[blockIdx.x]);
        return;
    }
    const int nb = gridDim.x - a.n_heavy;
    const int vb = renet_xcd_block(blockIdx.x - a.n_heavy, nb);
    const int ngroups = (a.N + R - 1) / R;
    const int gpb = (ngroups + nb - 1) / nb;
    const int g0 = vb * gpb;
    const int g1 = min(ngroups, g0 + gpb);
    const float4* __restrict__ x4 = reinterpret_cast<const float4*>(a.x);       // (the float4 widths read through these)
    const float4* __restrict__ w4 = reinterpret_cast<const float4*>(a.W);

    for (int grp = g0 + wave; grp < g1; grp += kWaves) {
        const int v0 = grp * R;
        const int nrows = min(R, a.N - v0);
        int my_rp = 0;
        float my_sc = 1.f;
        if (lane <= nrows) my_rp = a.row_ptr[v0 + lane];
        if (a.scale && lane < nrows) my_sc = a.scale[v0 + lane];
        const int e_end = __builtin_amdgcn_readlane(my_rp, nrows);
        int e = __builtin_amdgcn_readlane(my_rp, 0);
        int r = 0;                                       // current row; [row_beg, row_end) its edges
        int row_end = __builtin_amdgcn_readlane(my_rp, 1);
        bool row_heavy = (row_end - e) > a.heavy_thresh;
        float4 acc[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);

        auto flush = [&]() {
            if (!row_heavy) {
                const float sc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_sc), r));
#pragma unroll
                for (int c = 0; c < NCH; ++c)
                    if (lane + 64 * c < CH) gather_epilogue<SI>(a, v0 + r, lane + 64 * c, acc[c], sc);
            }
#pragma unroll
            for (int c = 0; c < NCH; ++c) acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
            ++r;
            const int beg = row_end;
            row_end = r < nrows ? __builtin_amdgcn_readlane(my_rp, r + 1) : 0x7fffffff;
            row_heavy = r < nrows && (row_end - beg) > a.heavy_thresh;
        };

        int eb = e - 64;                                 // start of the index window held in registers
        int my_col = 0, my_t = 0;
        while (e < e_end) {
            while (e >= row_end) flush();                // row boundary (also empty rows)
            if (row_heavy) { e = row_end; continue; }    // hub row: left to the heavy kernel
            if (e >= eb + 64) {                          // refill the 64-edge index window (coalesced)
                eb = e;
                const int my_e = eb + lane;
                my_col = 0; my_t = 0;
                if (my_e < e_end) {
                    my_col = a.col[my_e];
                    my_t = a.etype[my_e] + a.shift;
                    if (my_t >= a.T) my_t -= a.T;
                }
            }
            const int k0 = e - eb;
            const int cnt = min(64, e_end - eb);
            float4 xv[UNR][NCH];
            float4 wv[UNR][NCH][WCH];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                if (k0 + u < cnt && __builtin_amdgcn_readlane(my_col, k0 + u) < a.src_limit) {
                    const int src = __builtin_amdgcn_readlane(my_col, k0 + u);   // wave-uniform -> SGPR base
                    const int t = __builtin_amdgcn_readlane(my_t, k0 + u);
                    if constexpr (VW == 4) {
                        const float4* xr = x4 + (size_t)src * CH;
                        const float4* wr = w4 + (size_t)t * WROW4;
#pragma unroll
                        for (int c = 0; c < NCH; ++c) {
                            const int ch = lane + 64 * c;
                            if (ch < CH) {
                                xv[u][c] = xr[ch];
#pragma unroll
                                for (int q = 0; q < WCH; ++q) wv[u][c][q] = wr[ch * WCH + q];
                            }
                        }
                    } else {
                        const float* xr = a.x + (size_t)src * D;
                        const float* wr = a.W + (size_t)t * (D * SI);
#pragma unroll
                        for (int c = 0; c < NCH; ++c) {
                            const int ch = lane + 64 * c;
                            if (ch < CH) {
                                xv[u][c] = ld_chunk<VW>(xr, ch);
#pragma unroll
                                for (int q = 0; q < WCH; ++q) wv[u][c][q] = ld_chunk<VW>(wr, ch * WCH + q);
                            }
                        }
                    }
                }
            }
            // (a batch may run into the next rows; loads past a hub row's start are simply unused)
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                if (k0 + u < cnt && e == eb + k0 + u) {
                    while (e >= row_end) flush();
                    if (!row_heavy) {
                        if (__builtin_amdgcn_readlane(my_col, k0 + u) < a.src_limit) {
#pragma unroll
                            for (int c = 0; c < NCH; ++c)
                                if (lane + 64 * c < CH) blockmul<SI, TR>(xv[u][c], wv[u][c], acc[c]);
                        }
                        ++e;
                    }
                }
            }
        }
        while (r < nrows) flush();
    }
}

// One workgroup (4 waves) per hub row: wave w takes in-edges w, w+4, ... in batches of UNR, then a
// fixed-order LDS combine and the same fused epilogue => deterministic.
template <int SI, int NCH, int UNR, bool TR>
__device__ __forceinline__ void gather_heavy_row(const GatherArgs& a, int v) {
    constexpr int D = 100 * SI;
    constexpr int VW = vw_of<SI>();
    constexpr int CH = D / VW;
    constexpr int WCH = SI;
    constexpr int WROW4 = D * SI / 4;
    __shared__ float4 red[kWaves][CH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e0 = a.row_ptr[v], e1 = a.row_ptr[v + 1];
    const float4* __restrict__ x4 = reinterpret_cast<const float4*>(a.x);
    const float4* __restrict__ w4 = reinterpret_cast<const float4*>(a.W);
    float4 acc[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int e = e0 + wave; e < e1; e += kWaves * UNR) {
        float4 xv[UNR][NCH];
        float4 wv[UNR][NCH][WCH];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int ee = e + u * kWaves;
            if (ee < e1 && a.col[ee] < a.src_limit) {
                const int src = a.col[ee];
                int t = a.etype[ee] + a.shift;
                if (t >= a.T) t -= a.T;
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    const int ch = lane + 64 * c;
                    if (ch < CH) {
                        if constexpr (VW == 4) {
                            xv[u][c] = x4[(size_t)src * CH + ch];
#pragma unroll
                            for (int q = 0; q < WCH; ++q) wv[u][c][q] = w4[(size_t)t * WROW4 + ch * WCH + q];
                        } else {
                            xv[u][c] = ld_chunk<VW>(a.x, (size_t)src * CH + ch);
#pragma unroll
                            for (int q = 0; q < WCH; ++q)
                                wv[u][c][q] = ld_chunk<VW>(a.W, (size_t)t * (CH * WCH) + ch * WCH + q);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            if (e + u * kWaves < e1 && a.col[e + u * kWaves] < a.src_limit) {
#pragma unroll
                for (int c = 0; c < NCH; ++c)
                    if (lane + 64 * c < CH) blockmul<SI, TR>(xv[u][c], wv[u][c], acc[c]);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c)
        if (lane + 64 * c < CH) red[wave][lane + 64 * c] = acc[c];
    __syncthreads();
    if (wave == 0) {
        const float sc = a.scale ? a.scale[v] : 1.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int ch = lane + 64 * c;
            if (ch < CH) {
                float4 s = red[0][ch];
#pragma unroll
                for (int w = 1; w < kWaves; ++w) s = f4_add(s, red[w][ch]);
                gather_epilogue<SI>(a, v, ch, s, sc);
            }
        }
    }
}

template <int SI, int NCH, int UNR>
int launch_gather(const GatherArgs& a, bool tr, hipStream_t st) {
    // one 8-row group per wave where possible; multiple of 8 blocks for the XCD remap
    const int ngroups = (a.N + 7) / 8;
    int blocks = (ngroups + kWaves - 1) / kWaves;
    blocks = max(8, min(blocks, 256 * 8));
    blocks = (blocks + 7) & ~7;
    const int grid = blocks + a.n_heavy;         // hub rows first, then the row groups, in ONE launch
    if (tr) RENET_LAUNCH((rgcn_gather_kernel<SI, NCH, UNR, true>), dim3(grid), dim3(kThreads), 0, st, a);
    else RENET_LAUNCH((rgcn_gather_kernel<SI, NCH, UNR, false>), dim3(grid), dim3(kThreads), 0, st, a);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}

}  // namespace

extern "C" {

int renet_rgcn_gather(const float* x, int D, const int32_t* row_ptr, const int32_t* col,
                      const int32_t* etype, const float* scale, const float* W, int T, int type_shift,
                      int transpose_w, const float* addend, float drop_p, uint64_t seed, int relu,
                      float* out, int N, const int32_t* heavy_rows, int n_heavy, int heavy_thresh,
                      int src_limit, int addend_rows, void* stream) {
    GatherArgs a{};
    gather_fill(a, x, row_ptr, col, etype, scale, W, T, type_shift, addend, drop_p, seed, relu, out, N, heavy_rows, n_heavy,
                src_limit, addend_rows);
    if (const int rc = gather_check(D, a, drop_p)) return rc;
    if (n_heavy > 0 && heavy_thresh < 1) return RENET_ERR_BADARG;
    if (N == 0) return RENET_OK;
    a.heavy_thresh = n_heavy > 0 ? heavy_thresh : 0x7fffffff;
    return with_si(D, [&](auto si) {
        constexpr int SI = decltype(si)::value;
        return launch_gather<SI, nch_of<SI>(), SI <= 2 ? 4 : 2>(a, transpose_w != 0, (hipStream_t)stream);
    });
}

}  // extern "C"
