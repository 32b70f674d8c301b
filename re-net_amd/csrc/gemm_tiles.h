// What the tiled MFMA GEMM families share (gemm_split.hip, gemm_h3.hip, gemm_bf16s.hip, gemm_planes.hip): the output
// tile geometry and vector types, the argument struct of the epilogue, the workgroup -> tile map, the raw-buffer operand
// loader of the two-phase kernels, the accumulator store, and the host rules for the tile order.  Everything sits in the
// anonymous namespace of the including translation unit (device helpers are inlined; every family keeps its own kernels).
#ifndef RENET_GEMM_TILES_H
#define RENET_GEMM_TILES_H
#include <type_traits>
#include "common.h"

// split-K reduction C = alpha * sum_z partial[z] (+ bias) (+ beta * C): split_reduce_kernel / split_reduce4_kernel, defined
// in gemm_split.hip and shared by the families that write SplitArgs::partial planes
__attribute__((visibility("hidden"))) int renet_split_reduce(const float* partial, int split_k, int M, int N, float alpha,
                                                             float beta, const float* bias, float* C, int ldc,
                                                             hipStream_t st);

namespace {

constexpr int BM = 128, BN = 128, BK = 32;
constexpr int LDS_ROW = 40;                     // bf16 per LDS row (80 B)

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

struct SplitArgs {
    const float* A;
    const float* B;
    float* C;
    const float* bias;
    int M, N, K, lda, ldb, ldc;
    float alpha, beta;
    int k_tiles_per_split;
    int split_k;
    float* partial;
    int xcd_order;          // 0: plain order; w >= 1: XCD-aware virtual tile order with panels of <= w tiles (tile_of_block)
    int staged;             // epilogue: 1 = 16-byte rows through LDS (store_tile_staged), 0 = straight from the MFMA layout
};


// Optional phase tracing (tools/gemm_trace.py builds a separate library with -DRENET_GEMM_TRACE; the shipped
// library contains none of this): s_memtime stamps per wave and k-step for the first TRACE_BLOCKS workgroups.
#ifdef RENET_GEMM_TRACE
constexpr int TRACE_BLOCKS = 64, TRACE_STEPS = 320;
__device__ unsigned long long* g_trace = nullptr;          // [TRACE_BLOCKS][8 waves][TRACE_STEPS][4]
__device__ __forceinline__ void trace_put(int wave8, int step, int slot, unsigned long long v) {
    const int flat = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    // workgroups 0-31 and 256-287: the second set usually lands on the same CUs as the first
    if (g_trace && flat < 512 && (flat & 255) < 32 && step < TRACE_STEPS && (threadIdx.x & 63) == 0)
        g_trace[(((size_t)((flat >> 8) * 32 + (flat & 255)) * 8 + wave8) * TRACE_STEPS + step) * 4 + slot] = v;
}
#define TRACE_T(wave8, step, slot) trace_put(wave8, step, slot, __builtin_amdgcn_s_memtime())
#define TRACE_V(wave8, step, slot, v) trace_put(wave8, step, slot, (unsigned long long)(v))
#else
#define TRACE_T(wave8, step, slot)
#define TRACE_V(wave8, step, slot, v)
#endif

// Tile of this workgroup.  The dispatcher deals workgroups to the 8 XCDs round-robin (block b -> XCD b % 8, each
// XCD with its own 4 MB L2), so the plain (blockIdx.x, blockIdx.y) order makes every XCD sweep the WHOLE of the
// long operand once per tile row of the short one (PMC: 215 MB of fabric traffic per GEMM launch of the step
// against ~60 MB of operands + output; 127 MB with this order).  Virtual order instead: XCD x owns one contiguous
// 1/8 of the tile sequence, and in that sequence the SHORT grid dimension runs fastest, so the tiles that share
// a slab of the long operand are consecutive on one XCD and the slab is fetched once.  RENET_GEMM_TILE_ORDER=0
// in the environment restores the plain order (tools/gemm_bench.py).
__device__ __forceinline__ void tile_of_block(int nbx, int nby, int xcd_order, int& bx, int& by, int& bz) {
    bz = blockIdx.z;
    if (!xcd_order) { bx = blockIdx.x; by = blockIdx.y; return; }
    const int nb = nbx * nby;
    int t;                                                   // position in the tile sequence of one k-slice
    if (gridDim.z == 1) {
        const int per = nb >> 3;
        const int L = blockIdx.x + nbx * blockIdx.y;
        t = L < 8 * per ? (L & 7) * per + (L >> 3) : L;
    } else {
        // split-K grids (round 4): the dispatcher deals the FLATTENED index (x fastest, then y, then z) to the XCDs, so the
        // 2-D rule above spreads every k-slice over all eight L2s whenever nbx * nby is not a multiple of 8 -- and even
        // when it is, each slice's operand slabs are fetched by all XCDs (PMC, tools/pmc_by_shape.py: 600 x 800 x 16000 / 14
        // read 421 MB for 90 MB of operands, dfeat 2048 x 600 x 23033 / 6 689 MB for 244).  Here XCD x owns one contiguous
        // eighth of the (k-slice, tile) sequence: whole k-slices, read by one L2 (two where a slice straddles).
        const int total = nb * (int)gridDim.z, per3 = total >> 3;
        const int L3 = blockIdx.x + nbx * (blockIdx.y + nby * blockIdx.z);
        const int v = L3 < 8 * per3 ? (L3 & 7) * per3 + (L3 >> 3) : L3;
        bz = v / nb;
        t = v - bz * nb;
    }
    // sequence: panels of <= 8 tiles across the SHORT dimension, the long dimension sweeping each panel
    // (a square problem becomes 8 x 8 blocks of concurrently resident tiles per XCD instead of 2 x 32)
    const int ns = min(nbx, nby), nl = max(nbx, nby);
    const int w = min(ns, xcd_order);
    const int p = t / (w * nl), r = t - p * (w * nl);
    const int wp = min(w, ns - p * w);                       // width of this (possibly last, narrower) panel
    const int l = r / wp, sh = p * w + (r - l * wp);
    if (nby <= nbx) { bx = l; by = sh; }
    else { by = l; bx = sh; }
}

// item i of this thread (f = tid + threads * i) of a ROWS x 32 operand tile:
//   CONTIG_K: row = f>>3, k = 4*(f&7);  else: row = f % ROWS, k = 4*(f / ROWS)
template <bool CONTIG_K, int ROWS = 128>
__device__ __forceinline__ void item_pos(int f, int& row, int& k) {
    if constexpr (CONTIG_K) { row = f >> 3; k = (f & 7) << 2; }
    else { row = f & (ROWS - 1); k = (f / ROWS) << 2; }
}

__device__ __forceinline__ uint2 pack4(bf16x2 lo, bf16x2 hi) {
    uint2 u;
    u.x = __builtin_bit_cast(unsigned, lo);
    u.y = __builtin_bit_cast(unsigned, hi);
    return u;
}

// Raw-buffer loader (f16x3 kernels since round 3, bf16x6 two-phase kernels since round 4): raw buffer loads -- a descriptor of the operand (SGPRs) plus a per-lane 32-bit byte
// offset computed once and advanced by the tile's uniform k offset (one v_add per load): no 64-bit address arithmetic and
// NO BRANCH inside the MFMA phase.  (tools/gemm_trace.py: with the generic ItemLoader -- clamped addresses, a
// uniform branch per item -- every load piece cost the issuing wave ~180 cycles between two MFMAs, 2.4x the
// matrix-pipe time of the 24-MFMA phase.)  Nothing is clamped along k: the descriptor's num_records is the operand's
// exact extent, every dword beyond it reads as 0 without touching memory (raw buffers are range-checked per dword:
// tests/test_gpu_parity.py runs K % 4 != 0 with odd row strides, where the last row's last 16-byte load straddles the
// end), reads beyond K inside it (the next row) are zeroed by store_items_h's EDGE path like the clamped rows.
// Requires rows * ld * 4 < 2^32 (checked on the host; larger operands run the bf16x6 kernels).
typedef uint32_t h3_u32x4 __attribute__((ext_vector_type(4)));

template <bool CONTIG_K, int NT, int ROWS, int NI>
struct TileLoaderH {
    __amdgpu_buffer_rsrc_t rs;
    uint32_t off[NI];          // bytes: CONTIG_K: (row * ld + kk) * 4      else: (row + kk * ld) * 4
    uint32_t ldb;              // row stride in bytes

    __device__ __forceinline__ void init(const float* P, int ld, int rows, int K, int row0, int tid) {
        const uint32_t extent = CONTIG_K ? (uint32_t)(rows - 1) * (uint32_t)ld + (uint32_t)K
                                         : (uint32_t)(K - 1) * (uint32_t)ld + (uint32_t)rows;
        rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(P), (short)0, (int)(extent * 4u),
                                               0x00020000);
        ldb = (uint32_t)ld * 4u;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            int row, k;
            item_pos<CONTIG_K, ROWS>(tid + NT * i, row, k);
            row = min(row0 + row, rows - 1);
            off[i] = (CONTIG_K ? (uint32_t)row * (uint32_t)ld + (uint32_t)k : (uint32_t)row + (uint32_t)k * (uint32_t)ld) * 4u;
        }
    }

    __device__ __forceinline__ void load_item(int i, int k0, float4& r) const {
#ifdef RENET_PROBE_NOLOAD           // probe builds only (tools/gemm_split_probe.py): the k-loop without its global loads
        if (k0 > 0) return;
#endif
        if constexpr (CONTIG_K) {
            const h3_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(off[i] + (uint32_t)k0 * 4u), 0, 0);
            r = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
        } else {
            const uint32_t b0 = off[i] + (uint32_t)k0 * ldb;
            r.x = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (int)b0, 0, 0));
            r.y = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (int)(b0 + ldb), 0, 0));
            r.z = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (int)(b0 + 2u * ldb), 0, 0));
            r.w = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (int)(b0 + 3u * ldb), 0, 0));
        }
    }

    __device__ __forceinline__ void load(int k0, float4 (&r)[NI]) const {
#pragma unroll
        for (int i = 0; i < NI; ++i) load_item(i, k0, r[i]);
    }
};

// out-of-range fix-up of one UNCLAMPED item: rows past the operand and k past K become zeros
__device__ __forceinline__ float4 fix_item_h(float4 v, int rows, int K, int row0, int k0, int row, int k) {
    const int kg = k0 + k;
    const bool rok = row0 + row < rows;
    if (!rok || kg >= K) v.x = 0.f;
    if (!rok || kg + 1 >= K) v.y = 0.f;
    if (!rok || kg + 2 >= K) v.z = 0.f;
    if (!rok || kg + 3 >= K) v.w = 0.f;
    return v;
}

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// ---- staged epilogue -------------------------------------------------------------------------------------------------
// A wave's 64 x 64 outputs leave the CU as 16-byte row pieces instead of 64 dword stores per lane (an epilogue of many
// narrow stores per lane is bound by store ISSUE, not by bandwidth).  The accumulators go through a region of the
// workgroup's LDS that is private to the wave -- the operand images are dead by then; every kernel makes sure of it with a
// workgroup barrier behind its last fragment read -- in passes of ROWS rows x 64 columns:
//   write  32 (16) ds_write_b32 in the MFMA layout: lanes 0-31 one row, 32 consecutive dwords (a ds_write_b32 is served in
//          two groups of 32 lanes over 32 banks: no conflict at any pitch);
//   read   ROWS / 4 ds_read_b128 in the row layout: lane l owns the 16 bytes at row (l >> 4) + 4 k, columns 4 (l & 15)..;
//          a ds_read_b128 is served in four groups of 16 lanes that each cover halves of TWO rows (lanes 0-3, 12-15 of one
//          and 4-11 of the next) over 64 banks: free of conflicts exactly when the pitch is a multiple of 64 dwords;
//   store  one wave-instruction = 4 rows x 256 contiguous bytes.
// LDS operations of one wave execute in order, so only the compiler has to be held (wavefront fence) between a pass's
// writes and reads.  Element arithmetic: the expressions of the direct path, on the same operands -- same bits.
constexpr int EPI_PITCH = 64;                              // dwords per staged row
constexpr int EPI_WAVE_FLOATS = 32 * EPI_PITCH;            // a wave's region (8 KB); 16-row passes use half of it

struct EpiOut {
    float* base;            // C, or the split-K partial plane of this k-slice
    size_t ld;              // its row stride (elements)
    int M, n_main;          // rows; columns [0, n_main) go to base
    float* col_out;         // optional (planes GEMM): column n_main goes to col_out[row]
    const float* bias;      // optional, per column of base
    float alpha, beta;
    bool raw;               // split-K partial plane: the raw accumulators
    bool accumulate;        // beta != 0: read - modify - write
};

__device__ __forceinline__ bool epi_staged_ok(const SplitArgs& g, const float* base, size_t ld) {
    return g.staged && ((reinterpret_cast<uintptr_t>(base) & 15) == 0) && ((ld & 3) == 0);
}

// workgroup-uniform: this launch's tiles of k-slice z take the staged path (what store_tile decides; the kernels key the
// barrier in front of the staging on it)
__device__ __forceinline__ bool tile_staged(const SplitArgs& g, int z) {
    const bool split = g.split_k > 1;
    return epi_staged_ok(g, split ? g.partial + (size_t)z * g.M * g.N : g.C, (size_t)(split ? g.N : g.ldc));
}

// row0 / col0: the first output row / column of this wave's 64 x 64 block.  EDGE (wave-uniform): the block reaches beyond row M
// or beyond column n_main -- only then are there per-lane row and column checks, and straddling groups.
template <int ROWS, bool EDGE>
__device__ __forceinline__ void store_block_staged(const EpiOut& o, float* stage, int row0, int col0, int lane,
                                                   const f32x16 (&acc)[2][2]) {
    typedef __attribute__((address_space(3))) float lds_f32;
    typedef __attribute__((address_space(3))) f32x4 lds_f32x4;
    constexpr int NK = ROWS / 4;                           // 16-byte pieces per lane and pass
    lds_f32* st = (lds_f32*)stage;
    const int half = lane >> 5;
    const int rl = lane >> 4;                              // row of this lane inside a group of 4
    const int c4 = col0 + 4 * (lane & 15);
    const int nv = EDGE ? o.n_main - c4 : 4;               // columns of this lane's group that go to base (>= 4: all)
    const bool full = nv >= 4;
    const int cv = (EDGE && o.col_out && nv >= 0 && nv < 4) ? nv : -1;    // element of the group that is the col_out column
    float bv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) bv[e] = (!o.raw && o.bias && e < nv) ? o.bias[c4 + e] : 0.f;
    // element e of row `row` of a straddling group: its address, or null where nothing may be touched
    auto edge_ptr = [&](int row, int e) -> float* {
        return e < nv ? o.base + (size_t)row * o.ld + c4 + e : e == cv ? o.col_out + row : nullptr;
    };
#pragma unroll
    for (int p = 0; p < 64 / ROWS; ++p) {
        constexpr int RPB = 32 / ROWS;                     // passes per 32-row MFMA block
        const int i = p / RPB, r0 = (p % RPB) * (ROWS / 2);
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < ROWS / 2; ++r)
                st[((r & 3) + 8 * (r >> 2) + 4 * half) * EPI_PITCH + j * 32 + (lane & 31)] = acc[i][j][r0 + r];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        f32x4 v[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) v[k] = *(const lds_f32x4*)(st + (rl + 4 * k) * EPI_PITCH + 4 * (lane & 15));
        __builtin_amdgcn_s_waitcnt(0xC07F);                // lgkmcnt(0): the region is free for the next pass
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int rowp = row0 + p * ROWS + rl;
        // beta != 0: ALL reads of the pass first, then its stores (see the direct path)
        f32x4 old[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) old[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (o.accumulate) {
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int row = rowp + 4 * k;
                if (EDGE && row >= o.M) continue;
                if (full) {
                    old[k] = *reinterpret_cast<const f32x4*>(o.base + (size_t)row * o.ld + c4);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float* q = edge_ptr(row, e);
                        if (q) old[k][e] = *q;
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int row = rowp + 4 * k;
            if (EDGE && row >= o.M) continue;
            f32x4 w;
            if (o.raw) {
                w = v[k];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) w[e] = o.alpha * v[k][e] + bv[e] + (o.accumulate ? o.beta * old[k][e] : 0.f);
            }
            if (full) {
                *reinterpret_cast<f32x4*>(o.base + (size_t)row * o.ld + c4) = w;
            } else {
                // the group straddles column n_main: its valid columns one by one, nothing at or beyond n_main
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float* q = edge_ptr(row, e);
                    if (q) *q = w[e];
                }
            }
        }
    }
}

template <int ROWS>
__device__ __forceinline__ void store_tile_staged(const EpiOut& o, float* stage, int row0, int col0, int lane,
                                                  const f32x16 (&acc)[2][2]) {
    static_assert(ROWS == 32 || ROWS == 16, "a pass is one or one half of a 32-row MFMA block");
    const int n_all = o.n_main + (o.col_out ? 1 : 0);
    if (row0 >= o.M || col0 >= n_all) return;              // wave-uniform
    // (the epilogue's lane arithmetic starts here: hoisted above the k-loop it costs every kernel 4 VGPRs in the loop)
    asm volatile("" : "+v"(lane));
    if (row0 + 64 <= o.M && col0 + 64 <= o.n_main) store_block_staged<ROWS, false>(o, stage, row0, col0, lane, acc);
    else store_block_staged<ROWS, true>(o, stage, row0, col0, lane, acc);
}

// accumulators -> C (or the split-K partial plane).  C/D layout of the 32x32 MFMA: col = lane & 31,
// row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).  `stage`: this wave's EPI_WAVE_FLOATS (ROWS = 32) or half of that
// (ROWS = 16) of dead LDS.  The staged path needs a 16-byte aligned output with a row stride that is a multiple of 4 floats;
// any other output, and RENET_GEMM_EPILOGUE=direct, take the direct path below.  STAGED = false: a kernel that has only the
// direct path (gemm_bf16_kernel, gemm_split_fused_kernel: no measured gain from the staged form, profiles/gemm_epilogue.md).
template <int ROWS = 32, bool STAGED = true>
__device__ __forceinline__ void store_tile(const SplitArgs& g, int m0, int n0, int z, int wm, int wn, int lane,
                                           const f32x16 (&acc)[2][2], float* stage) {
#ifdef RENET_PROBE_NOSTORE          // probe builds only (tools/gemm_split_probe.py): what the C-store epilogue costs
    if (acc[0][0][0] != 12345.678f) return;
#endif
    const bool split = g.split_k > 1;
    float* Cout = split ? g.partial + (size_t)z * g.M * g.N : g.C;
    const int ldo = split ? g.N : g.ldc;
    const int half = lane >> 5;
    const bool accumulate = !split && g.beta != 0.f;
    if (STAGED && epi_staged_ok(g, Cout, (size_t)ldo)) {
        EpiOut o;
        o.base = Cout; o.ld = (size_t)ldo; o.M = g.M; o.n_main = g.N; o.col_out = nullptr;
        o.bias = g.bias; o.alpha = g.alpha; o.beta = g.beta; o.raw = split; o.accumulate = accumulate;
        store_tile_staged<ROWS>(o, stage, m0 + wm * 64, n0 + wn * 64, lane, acc);
        return;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = n0 + wn * 64 + j * 32 + (lane & 31);
            if (col >= g.N) continue;
            const float bv = (!split && g.bias) ? g.bias[col] : 0.f;
            const int row_base = m0 + wm * 64 + i * 32 + 4 * half;
            // beta != 0 (in-place gradient accumulation): ALL 16 reads of C first, then the 16 stores.  Written as
            // load / fma / store per element the compiler must assume that a store aliases the next load and chains
            // 64 memory round trips per lane at the end of every tile.
            float old[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) old[r] = 0.f;
            if (accumulate) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = min(row_base + (r & 3) + 8 * (r >> 2), g.M - 1);
                    old[r] = Cout[(size_t)row * ldo + col];
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = row_base + (r & 3) + 8 * (r >> 2);
                if (row < g.M) {
                    float* p = Cout + (size_t)row * ldo + col;
                    if (split) *p = acc[i][j][r];
                    else *p = g.alpha * acc[i][j][r] + bv + (accumulate ? g.beta * old[r] : 0.f);
                }
            }
        }
}

// An explicit RENET_GEMM_PANEL_W pins the panel width of the XCD-aware order (renet_gemm_tile_order() in common.h)
inline bool panel_w_pinned() {
    static const bool v = getenv("RENET_GEMM_PANEL_W") != nullptr;
    return v;
}

// Panel width for an UN-SPLIT grid that takes several rounds of tiles per XCD.  The short operand is swept once per round
// by every XCD; when all of it (ns tiles) does not fit the 4 MB L2 next to the streamed long operand, that cyclic sweep
// misses (PMC, tools/pmc_by_shape.py: the 256-row logits GEMM fetched 313 MB for 60 MB of operands, 258 MB of it the
// 4.9 MB `feat`).  Narrower panels keep one panel of the short operand resident (<= 2.5 MB) and re-read the long operand
// once per extra panel: taken when that costs less than the sweep does (so NOT for dW = dlogits^T feat, whose long
// operand is 189 MB).  An explicit RENET_GEMM_PANEL_W, the plain order, or a split k range leaves the width alone.
inline int panel_width(int base, int nbx, int nby, int tile_m, int K, int split_k, int slots_per_xcd) {
    if (base != 8 || split_k != 1 || panel_w_pinned()) return base;
    const bool short_is_m = nby <= nbx;
    const int ns = short_is_m ? nby : nbx, nl = short_is_m ? nbx : nby;
    const double slab = (double)(short_is_m ? tile_m : BN) * K * 4.0;           // short-operand bytes of one tile row / column
    const double long_total = (double)(short_is_m ? BN : tile_m) * K * 4.0 * nl;
    const double short_total = slab * ns;
    const double rounds = (double)nbx * nby / (8.0 * slots_per_xcd);
    if (short_total <= 3.0e6 || rounds <= 1.0) return base;
    const int w = max(1, min(8, (int)(2.5e6 / slab)));
    const int w0 = min(ns, 8);
    if (w >= w0) return base;
    const int extra_panels = (ns + w - 1) / w - (ns + w0 - 1) / w0;
    if (long_total * extra_panels >= short_total * rounds * 8.0) return base;
    return w;
}

}  // namespace

#endif  // RENET_GEMM_TILES_H
