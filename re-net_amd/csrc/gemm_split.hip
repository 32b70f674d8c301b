// fp32-accurate GEMM on the bf16 matrix cores of gfx950 ("bf16x6 split"):
//
//   every fp32 operand value is split EXACTLY-to-rounding into three bf16 terms  x = x1 + x2 + x3
//   (x1 = rne(x), x2 = rne(x - x1), x3 = rne(x - x1 - x2); |x - x1 - x2 - x3| <= 2^-25 |x|), and the
//   product a*b is evaluated with the six term pairs of weight >= 2^-16:
//        a1 b1 + (a1 b2 + a2 b1) + (a1 b3 + a2 b2 + a3 b1)
//   each on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  bf16 x bf16 products are exact in fp32;
//   the dropped pairs (a2 b3, a3 b2, a3 b3) are <= 2^-23 |a b|, i.e. at the fp32 rounding level, so the
//   result is an fp32-class GEMM (every kernel here against fp64 in tests/test_gpu_gemm_products.py: single products
//   within 2^-22, which no five of the six pairs keep, dense products in units of the dot product's own fp32 bound next to
//   the v_mfma_f32_32x32x2_f32 kernel of gemm.hip, integers exactly) -- while the matrix pipe runs 16x faster per product:
//   6 bf16 MFMAs replace 16/6 = 2.67x their time in f32-input MFMAs.
//
// Two k-loop structures share the tile (128x128x32, 4 waves 2x2, each wave 2x2 MFMA tiles of 32x32) and the
// LDS image: gemm_split_kernel (two phases per k-tile, two workgroups per CU) and gemm_split_fused_kernel
// (split interleaved with the MFMAs, one workgroup per CU); kernel_choice() picks by grid size.  Staging: every thread owns
// (row, 4 consecutive k) items: one global_load_dwordx4 when k is contiguous in memory, four dword loads
// (coalesced across lanes along the row index) otherwise; the split happens in registers on the way into
// LDS; three bf16 planes per operand, image [row][k] with an 80-byte row stride (16-byte aligned, rows
// spread over all banks); fragments are one ds_read_b128 per plane (8 consecutive k per lane).
// Out-of-range elements are clamped at load time and zeroed at LDS-store time (never right behind the
// load, see gemm.hip).
#include <cstdlib>
#include <type_traits>
#include "gemm_tiles.h"
#include "gemm_skinny.h"

namespace {

constexpr int PLANE = BM * LDS_ROW;             // bf16 per plane
constexpr int THREADS = 256;

// Per-thread load state: the row part of every item's address is computed ONCE (the per-tile work is an
// add); integer multiplies inside the k loop cost more issue slots than the MFMAs they feed.
template <bool CONTIG_K, int NT = 256, int ROWS = 128, int NI = 4>
struct ItemLoader {
    const float* base[NI];     // CONTIG_K: P + row*ld          else: P + row
    int kk[NI];                // k offset of the item inside a tile
    size_t ld;
    int K;

    __device__ __forceinline__ void init(const float* P, int ld_, int rows, int K_, int row0, int tid) {
        ld = (size_t)ld_;
        K = K_;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            int row, k;
            item_pos<CONTIG_K, ROWS>(tid + NT * i, row, k);
            row = min(row0 + row, rows - 1);
            kk[i] = k;
            base[i] = CONTIG_K ? P + (size_t)row * ld : P + row;
        }
    }

    __device__ __forceinline__ void load(int k0, float4 (&r)[NI]) const {
#pragma unroll
        for (int i = 0; i < NI; ++i) load_item(i, k0, r[i]);
    }

    __device__ __forceinline__ void load_item(int i, int k0, float4& r) const {
        const bool full = k0 + BK <= K;                     // workgroup-uniform
        const int k = k0 + kk[i];
        if constexpr (CONTIG_K) {
            if (K >= 4) {
                r = *reinterpret_cast<const float4*>(base[i] + (full ? k : min(k, K - 4)));
            } else {
                const float* p = base[i];
                r = make_float4(p[min(k, K - 1)], p[min(k + 1, K - 1)], p[min(k + 2, K - 1)], p[min(k + 3, K - 1)]);
            }
        } else {
            if (full) {
                const float* p = base[i] + (size_t)k * ld;
                r = make_float4(p[0], p[ld], p[2 * ld], p[3 * ld]);
            } else {
                const float* p = base[i];
                r.x = p[(size_t)min(k, K - 1) * ld];
                r.y = p[(size_t)min(k + 1, K - 1) * ld];
                r.z = p[(size_t)min(k + 2, K - 1) * ld];
                r.w = p[(size_t)min(k + 3, K - 1) * ld];
            }
        }
    }
};

// Out-of-range fix-up of one clamped item (see ItemLoader::load_item): (row, k) are the item's coordinates
// inside the tile.
template <bool CONTIG_K>
__device__ __forceinline__ float4 fix_item(float4 v, int rows, int K, int row0, int k0, int row, int k) {
    const int kg = k0 + k;
    if constexpr (CONTIG_K) {
        if (K >= 4 && kg > K - 4 && kg < K) {      // the float4 was loaded from K-4: shift it back
            const int d = kg - (K - 4);
            v = d == 1 ? make_float4(v.y, v.z, v.w, 0.f) : d == 2 ? make_float4(v.z, v.w, 0.f, 0.f)
                                                                 : make_float4(v.w, 0.f, 0.f, 0.f);
        }
    }
    const bool rok = row0 + row < rows;
    if (!rok || kg >= K) v.x = 0.f;
    if (!rok || kg + 1 >= K) v.y = 0.f;
    if (!rok || kg + 2 >= K) v.z = 0.f;
    if (!rok || kg + 3 >= K) v.w = 0.f;
    return v;
}

// registers -> three bf16 planes in LDS.  EDGE (workgroup-uniform: the tile touches the end of the matrix
// in either dimension) enables the out-of-range fix-up of the clamped loads; interior tiles -- almost all of
// them -- run the bare split: 6 v_cvt_pk_bf16_f32, 4 packed subtractions and 3 ds_write_b64 per item.
template <bool CONTIG_K, bool EDGE, int NT = 256, int ROWS = 128, int NI = 4, bool RAW = false>
__device__ __forceinline__ void store_items(__bf16* __restrict__ S, int rows, int K, int row0, int k0, int tid,
                                            const float4 (&r)[NI]) {
    constexpr int PLANE = ROWS * LDS_ROW;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        int row, k;
        item_pos<CONTIG_K, ROWS>(tid + NT * i, row, k);
        float4 v = r[i];
        if constexpr (EDGE) {
            if constexpr (RAW) v = fix_item_h(v, rows, K, row0, k0, row, k);      // unclamped loads (TileLoaderH)
            else v = fix_item<CONTIG_K>(v, rows, K, row0, k0, row, k);
        }
        f32x2 lo = {v.x, v.y}, hi = {v.z, v.w};
        __bf16* dst = S + row * LDS_ROW + k;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const bf16x2 blo = __builtin_convertvector(lo, bf16x2);        // v_cvt_pk_bf16_f32 (RNE)
            const bf16x2 bhi = __builtin_convertvector(hi, bf16x2);
#ifdef RENET_PROBE_NOLDSW           // probe builds only: the split without its LDS stores (one plane still written)
            if (p == 2) *reinterpret_cast<uint2*>(dst) = pack4(blo, bhi);
#else
            *reinterpret_cast<uint2*>(dst + p * PLANE) = pack4(blo, bhi);
#endif
#ifdef RENET_PROBE_NOSPLIT          // probe builds only: three roundings, no residual arithmetic
            if (false)
#endif
            if (p < 2) {
                lo -= __builtin_convertvector(blo, f32x2);                  // exact residuals
                hi -= __builtin_convertvector(bhi, f32x2);
            }
        }
    }
}


// One 128x128x32 tile step of a wave: 24 fragment reads (ds_read_b128) and 48 MFMAs.
template <int PLANE_A = PLANE, int PLANE_B = PLANE>
__device__ __forceinline__ void mfma_tile(const __bf16* __restrict__ sA, const __bf16* __restrict__ sB, int arow,
                                          int brow, int ksel, f32x16 (&acc)[2][2]) {
#pragma unroll
    for (int slab = 0; slab < 2; ++slab) {
        const int ko = slab * 16 + ksel;
        bf16x8 a[2][3], b[2][3];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                a[t][p] = *reinterpret_cast<const bf16x8*>(&sA[p * PLANE_A + arow + t * 32 * LDS_ROW + ko]);
                b[t][p] = *reinterpret_cast<const bf16x8*>(&sB[p * PLANE_B + brow + t * 32 * LDS_ROW + ko]);
            }
        // six term pairs, smallest first; consecutive MFMAs go to DIFFERENT accumulators so that none
        // waits on the previous one's result
        constexpr int PA[6] = {2, 1, 0, 1, 0, 0};
        constexpr int PB[6] = {0, 1, 2, 0, 1, 0};
#pragma unroll
        for (int q = 0; q < 6; ++q)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][PA[q]], b[j][PB[q]], acc[i][j], 0, 0, 0);
    }
}

// The MFMA phase of the two-phase kernels with the NEXT tile's global loads spread over it: issued in one
// burst right after the barrier (8 x 1 KB per wave, every wave of the CU at once) they fill the vector-memory
// queue -- the texture-address unit takes 64 B/clk, 16 cycles per dwordx4 wave-instruction -- and the waves
// sit in the load issue for ~1000-1500 cycles before their first MFMA (tools/gemm_trace.py).  Order pinned with
// sched_barrier: slab-0 fragments, then 48 MFMAs with the slab-1 fragment reads behind the first 12 and one
// load piece behind every fifth.
template <int PLANE_A, int PLANE_B, int NPIECES, class LoadFn>
__device__ __forceinline__ void mfma_tile_ld(const __bf16* __restrict__ sA, const __bf16* __restrict__ sB, int arow,
                                             int brow, int ksel, f32x16 (&acc)[2][2], LoadFn&& load_piece) {
    bf16x8 F0[12], F1[12];                       // index = operand + 2 * t + 4 * plane
    auto read = [&](auto frc, bf16x8 (&F)[12], int slab) {
        constexpr int fr = frc.value, op = fr & 1, t = (fr >> 1) & 1, p = fr >> 2;
        const __bf16* base = op ? sB + p * PLANE_B + brow : sA + p * PLANE_A + arow;
        F[fr] = *reinterpret_cast<const bf16x8*>(base + t * 32 * LDS_ROW + slab * 16 + ksel);
    };
    // in the order the term pairs consume them (lgkmcnt retires LDS reads in order: the first MFMA waits for
    // two fragments, not twelve)
    constexpr int ORDER[12] = {8, 1, 3, 10, 4, 5, 7, 6, 0, 9, 11, 2};
    static_for<0, 12>([&](auto n) { read(std::integral_constant<int, ORDER[n.value]>{}, F0, 0); });
    constexpr int PA[6] = {2, 1, 0, 1, 0, 0};
    constexpr int PB[6] = {0, 1, 2, 0, 1, 0};
    static_for<0, 48>([&](auto gc) {
        constexpr int g = gc.value, w = g % 24, q = w >> 2, i = (w >> 1) & 1, j = w & 1;
        if constexpr (g < 24)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(F0[2 * i + 4 * PA[q]], F0[1 + 2 * j + 4 * PB[q]], acc[i][j], 0, 0, 0);
        else
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(F1[2 * i + 4 * PA[q]], F1[1 + 2 * j + 4 * PB[q]], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (g < 12) read(std::integral_constant<int, ORDER[g]>{}, F1, 1);
        if constexpr (g % 5 == 2 && g / 5 < NPIECES) load_piece(std::integral_constant<int, g / 5>{});
        __builtin_amdgcn_sched_barrier(0);
    });
}

// RAW: operands addressed through raw buffer descriptors (TileLoaderH; both operands below 2^30 elements of reach, checked
// on the host) -- the generic ItemLoader otherwise.
// (Round 6 tried a 64-byte-row image with XOR-swizzled chunks here -- no LDS bank conflicts, 48 KB per tile: no change at two
// workgroups per CU, 15-50 % SLOWER at three (168 registers: spills); profiles/r06_a_planes_ablation.md.  Not kept.)
template <bool TA, bool TB, bool RAW>
__global__ __launch_bounds__(THREADS) void gemm_split_kernel(SplitArgs g) {
    constexpr int PL = BM * LDS_ROW;
    __shared__ __attribute__((aligned(16))) __bf16 sA[3 * PL];
    __shared__ __attribute__((aligned(16))) __bf16 sB[3 * PL];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    int bx, by, z;
    tile_of_block(gridDim.x, gridDim.y, g.xcd_order, bx, by, z);
    const int m0 = by * BM, n0 = bx * BN;
    const int kt0 = z * g.k_tiles_per_split;
    const int kt_total = (g.K + BK - 1) / BK;
    const int kt1 = min(kt_total, kt0 + g.k_tiles_per_split);
    constexpr bool A_CK = !TA;
    constexpr bool B_CK = TB;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    float4 ra[4], rb[4];
    std::conditional_t<RAW, TileLoaderH<A_CK, THREADS, BM, 4>, ItemLoader<A_CK>> la;
    std::conditional_t<RAW, TileLoaderH<B_CK, THREADS, BN, 4>, ItemLoader<B_CK>> lb;
    la.init(g.A, g.lda, g.M, g.K, m0, tid);
    lb.init(g.B, g.ldb, g.N, g.K, n0, tid);
    if (kt0 < kt1) {
        la.load(kt0 * BK, ra);
        lb.load(kt0 * BK, rb);
    }
    const bool a_edge = m0 + BM > g.M, b_edge = n0 + BN > g.N;
    const int ra_ = wm * 64 + (lane & 31), rb_ = wn * 64 + (lane & 31);
    const int arow = ra_ * LDS_ROW, brow = rb_ * LDS_ROW;
    const int ksel = (lane >> 5) * 8;

    TRACE_V(wave, TRACE_STEPS - 1, 0, __builtin_amdgcn_s_getreg((31 << 11) | 4));      // HW_ID
    TRACE_V(wave, TRACE_STEPS - 1, 1, __builtin_amdgcn_s_getreg((31 << 11) | 20));     // XCC_ID
    for (int kt = kt0; kt < kt1; ++kt) {
        __syncthreads();                               // previous tile fully consumed
        TRACE_T(wave, kt - kt0, 0);
        const bool k_edge = (kt + 1) * BK > g.K;
        if (a_edge || k_edge) store_items<A_CK, true, THREADS, BM, 4, RAW>(sA, g.M, g.K, m0, kt * BK, tid, ra);
        else store_items<A_CK, false, THREADS, BM, 4, RAW>(sA, g.M, g.K, m0, kt * BK, tid, ra);
        if (b_edge || k_edge) store_items<B_CK, true, THREADS, BN, 4, RAW>(sB, g.N, g.K, n0, kt * BK, tid, rb);
        else store_items<B_CK, false, THREADS, BN, 4, RAW>(sB, g.N, g.K, n0, kt * BK, tid, rb);
        TRACE_T(wave, kt - kt0, 1);
        __syncthreads();
        TRACE_T(wave, kt - kt0, 2);
        const int k0n = min(kt + 1, kt1 - 1) * BK;     // next tile (the last step reloads its own: harmless)
        mfma_tile_ld<PL, PL, 8>(sA, sB, arow, brow, ksel, acc, [&](auto ic) {
            constexpr int i = ic.value;
            if constexpr (i < 4) la.load_item(i, k0n, ra[i]);
            else lb.load_item(i - 4, k0n, rb[i - 4]);
        });
        TRACE_T(wave, kt - kt0, 3);
    }

    // staged epilogue: waves 0, 1 take 8 KB each of the A image, waves 2, 3 of the B image, once every wave has read its
    // last fragments
    if (tile_staged(g, z)) __syncthreads();
    static_assert(2 * EPI_WAVE_FLOATS * sizeof(float) <= 3 * PL * sizeof(__bf16), "staging fits an operand image");
    const int ws = __builtin_amdgcn_readfirstlane(wave);
    store_tile(g, m0, n0, z, wm, wn, lane, acc, reinterpret_cast<float*>(ws < 2 ? sA : sB) + (ws & 1) * EPI_WAVE_FLOATS);
}

// ------------------------------------------------------------------------------------------------------
// TALL variant of the two-phase kernel: 256 x 128 tile, 8 waves (4 x 2, each 64 x 64 as above), one workgroup per
// CU.  The in-loop split is paid per operand ELEMENT: a 256 x 128 x 32 step splits 12 288 elements for 2 x the MACs of
// a 128 x 128 x 32 step (8 192 elements), i.e. 0.75x the VALU / LDS-store work per flop -- the resource the k-loop
// is bound by (header of the fused variant).  Used for outputs with >= 1000 such tiles (use_tall).
// ------------------------------------------------------------------------------------------------------
constexpr int BMT = 256, THREADS_T = 512;
constexpr int PLANE_T = BMT * LDS_ROW;
constexpr size_t TALL_LDS = (size_t)(3 * PLANE_T + 3 * PLANE) * sizeof(__bf16);

template <bool TA, bool TB, bool RAW>
__global__ __launch_bounds__(THREADS_T) void gemm_split_tall_kernel(SplitArgs g) {
    extern __shared__ __attribute__((aligned(16))) __bf16 smem_t[];
    __bf16* sA = smem_t;
    __bf16* sB = smem_t + 3 * PLANE_T;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    int bx, by, z;
    tile_of_block(gridDim.x, gridDim.y, g.xcd_order, bx, by, z);
    const int m0 = by * BMT, n0 = bx * BN;
    const int kt0 = z * g.k_tiles_per_split;
    const int kt_total = (g.K + BK - 1) / BK;
    const int kt1 = min(kt_total, kt0 + g.k_tiles_per_split);
    constexpr bool A_CK = !TA;
    constexpr bool B_CK = TB;
    constexpr int NIA = BMT * 8 / THREADS_T, NIB = BN * 8 / THREADS_T;         // 4 and 2 items per thread

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    float4 ra[NIA], rb[NIB];
    std::conditional_t<RAW, TileLoaderH<A_CK, THREADS_T, BMT, NIA>, ItemLoader<A_CK, THREADS_T, BMT, NIA>> la;
    std::conditional_t<RAW, TileLoaderH<B_CK, THREADS_T, BN, NIB>, ItemLoader<B_CK, THREADS_T, BN, NIB>> lb;
    la.init(g.A, g.lda, g.M, g.K, m0, tid);
    lb.init(g.B, g.ldb, g.N, g.K, n0, tid);
    if (kt0 < kt1) {
        la.load(kt0 * BK, ra);
        lb.load(kt0 * BK, rb);
    }
    const bool a_edge = m0 + BMT > g.M, b_edge = n0 + BN > g.N;
    const int arow = (wm * 64 + (lane & 31)) * LDS_ROW;
    const int brow = (wn * 64 + (lane & 31)) * LDS_ROW;
    const int ksel = (lane >> 5) * 8;
    for (int kt = kt0; kt < kt1; ++kt) {
        __syncthreads();                               // previous tile fully consumed
        const bool k_edge = (kt + 1) * BK > g.K;
        if (a_edge || k_edge) store_items<A_CK, true, THREADS_T, BMT, NIA, RAW>(sA, g.M, g.K, m0, kt * BK, tid, ra);
        else store_items<A_CK, false, THREADS_T, BMT, NIA, RAW>(sA, g.M, g.K, m0, kt * BK, tid, ra);
        if (b_edge || k_edge) store_items<B_CK, true, THREADS_T, BN, NIB, RAW>(sB, g.N, g.K, n0, kt * BK, tid, rb);
        else store_items<B_CK, false, THREADS_T, BN, NIB, RAW>(sB, g.N, g.K, n0, kt * BK, tid, rb);
        __syncthreads();
        const int k0n = min(kt + 1, kt1 - 1) * BK;     // next tile (the last step reloads its own: harmless)
        mfma_tile_ld<PLANE_T, PLANE, NIA + NIB>(sA, sB, arow, brow, ksel, acc, [&](auto ic) {
            constexpr int i = ic.value;
            if constexpr (i < NIA) la.load_item(i, k0n, ra[i]);
            else lb.load_item(i - NIA, k0n, rb[i - NIA]);
        });
    }
    if (tile_staged(g, z)) __syncthreads();            // staged epilogue: every wave has read its last fragments
    static_assert((THREADS_T / 64) * EPI_WAVE_FLOATS * sizeof(float) <= TALL_LDS, "staging fits the images");
    store_tile(g, m0, n0, z, wm, wn, lane, acc, reinterpret_cast<float*>(smem_t) + __builtin_amdgcn_readfirstlane(wave) * EPI_WAVE_FLOATS);
}

// ------------------------------------------------------------------------------------------------------
// FUSED variant: every wave runs its MFMAs and the split of the NEXT k-tile in ONE instruction stream.
//
// Measured on MI355X (tools/mfma_probe.hip, tools/fill_probe.hip; shader cycles per 128x128x32 k-tile):
//   48 v_mfma_f32_32x32x16_bf16 of one wave                       1536   (32.0 each, any accumulator order)
//   ... plus its 24 ds_read_b128                                  1697
//   split of a k-tile (8 items/thread) + LDS stores, alone        1114
//   the same split as a SECOND wave beside an MFMA wave           2657   (s_setprio changes nothing)
//   free in a 32-cycle MFMA shadow of the same wave: ~4 plain VALU, 2 ds_read_b128; v_cvt_pk_bf16_f32 counts
//   double, v_pk_add_f32 and ds_write_b64 do not overlap at all (the LDS store path moves ~85 B/clk/CU: the
//   48 KB of planes of one k-tile cost ~650 cycles whichever wave issues them)
// so neither two independent workgroups per CU (gemm_split_kernel: both drift into lockstep, 3300 cycles per
// k-tile and CU) nor barrier-anti-phased halves (tried: 3650) hide the split behind the matrix pipe.  Here each
// of the 48 MFMAs of a k-step is followed by one "micro-step" of the split (4 independent plain VALU, at times
// one ds_write_b64 / ds_read_b128 / global load), the order pinned with sched_barrier: 2540 cycles per k-tile
// (1623 without the split; the LDS stores are ~650 of the difference).
//
// LDS is double buffered (2 x 61 440 B, one 4-wave workgroup per CU) with ONE barrier per k-tile, and the
// k-loop is rotated by half a tile so that no MFMA waits for LDS after the barrier:
//     barrier(kt): tile kt visible in buf[kt&1]; every wave holds slab 1 of tile kt-1 in registers (F1)
//       reads  F0 <- slab 0 of tile kt                   (first 4 up front, 8 in the first MFMA shadows)
//       MFMAs   0..23 : slab 1 of tile kt-1 (F1)         | split micro-steps 0..23 of tile kt+1 -> buf[~kt&1]
//       MFMAs  24..47 : slab 0 of tile kt   (F0)         | micro-steps 24..47, reads F1 <- slab 1 of tile kt
//     (buf[~kt&1] held tile kt-1, whose last reads -- F1 -- completed before barrier(kt) in every wave)
// The global loads of tile kt+2 are issued from the micro-steps that free their registers.
// Loader of the fused kernel: every item's address is  UNIFORM tile base (SGPRs, advanced per k-tile by the
// scalar unit) + a per-lane 32-bit element offset computed once (global_load saddr form: no VALU address math
// in the k-loop).  Requires rows * ld < 2^31 elements and, for CONTIG_K, K >= 4 (checked on the host).
template <bool CONTIG_K>
struct TileLoader {
    const float* P;
    int off[4];                // CONTIG_K: row * ld + kk       else: row + kk * ld
    int rowc[4], kk[4];        // clamped row / k offset inside a tile (for the partial last k-tile)
    int ld, K;

    __device__ __forceinline__ void init(const float* P_, int ld_, int rows, int K_, int row0, int tid) {
        P = P_; ld = ld_; K = K_;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int row, k;
            item_pos<CONTIG_K>(tid + THREADS * i, row, k);
            row = min(row0 + row, rows - 1);
            rowc[i] = row;
            kk[i] = k;
            off[i] = CONTIG_K ? row * ld + k : row + k * ld;
        }
    }

    template <bool FAST>
    __device__ __forceinline__ void load_item(int i, int k0, float4& r) const {
        if (FAST || k0 + BK <= K) {                         // workgroup-uniform: all but the last partial tile
            if constexpr (CONTIG_K) {
                r = *reinterpret_cast<const float4*>(P + k0 + off[i]);
            } else {
                const float* t0 = P + (size_t)k0 * ld;
                r = make_float4(t0[off[i]], (t0 + ld)[off[i]], (t0 + 2 * (size_t)ld)[off[i]],
                                (t0 + 3 * (size_t)ld)[off[i]]);
            }
        } else {
            const int k = k0 + kk[i];
            if constexpr (CONTIG_K) {
                r = *reinterpret_cast<const float4*>(P + (size_t)rowc[i] * ld + min(k, K - 4));
            } else {
                const float* p = P + rowc[i];
                r.x = p[(size_t)min(k, K - 1) * ld];
                r.y = p[(size_t)min(k + 1, K - 1) * ld];
                r.z = p[(size_t)min(k + 2, K - 1) * ld];
                r.w = p[(size_t)min(k + 3, K - 1) * ld];
            }
        }
    }

    __device__ __forceinline__ void load(int k0, float4 (&r)[4]) const {
#pragma unroll
        for (int i = 0; i < 4; ++i) load_item<false>(i, k0, r[i]);
    }
};

constexpr int BUF = 6 * PLANE;                              // bf16 per buffer: A planes, then B planes
constexpr size_t FUSED_LDS = (size_t)2 * BUF * sizeof(__bf16);

struct SplitState {
    float x[4];          // the item, then its residuals
    bf16x2 blo, bhi;     // the bf16 terms just split off (pairs x[0..1], x[2..3])
};

__device__ __forceinline__ float bf16_lo_as_f32(bf16x2 b) {
    return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, b) << 16);
}
__device__ __forceinline__ float bf16_hi_as_f32(bf16x2 b) {
    return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, b) & 0xffff0000u);
}
__device__ __forceinline__ bf16x2 rne_pair(float lo, float hi) {          // v_cvt_pk_bf16_f32
    return __builtin_convertvector(f32x2{lo, hi}, bf16x2);
}

// Micro-step ST (0..5) of one item: the SAME three round-to-nearest terms as store_items (both kernels feed
// the matrix cores identical planes), cut into pieces that issue beside an MFMA (tools/fill_probe.hip: ~4 plain
// VALU per 32-cycle shadow; v_cvt_pk_bf16_f32 counts double; v_pk_add_f32 does not overlap at all, hence the
// scalar subtractions); dependent instructions sit in different steps.
template <int ST>
__device__ __forceinline__ void split_step(SplitState& t, __bf16* dst) {
    if constexpr (ST == 0) {
        t.blo = rne_pair(t.x[0], t.x[1]);
        t.bhi = rne_pair(t.x[2], t.x[3]);
        *reinterpret_cast<uint2*>(dst) = pack4(t.blo, t.bhi);
    } else if constexpr (ST == 1) {
        t.x[0] -= bf16_lo_as_f32(t.blo);
        t.x[1] -= bf16_hi_as_f32(t.blo);
    } else if constexpr (ST == 2) {
        t.x[2] -= bf16_lo_as_f32(t.bhi);
        t.x[3] -= bf16_hi_as_f32(t.bhi);
    } else if constexpr (ST == 3) {
        t.blo = rne_pair(t.x[0], t.x[1]);
        t.bhi = rne_pair(t.x[2], t.x[3]);
        *reinterpret_cast<uint2*>(dst + PLANE) = pack4(t.blo, t.bhi);
    } else if constexpr (ST == 4) {
        t.x[0] -= bf16_lo_as_f32(t.blo);
        t.x[1] -= bf16_hi_as_f32(t.blo);
        t.x[2] -= bf16_lo_as_f32(t.bhi);
        t.x[3] -= bf16_hi_as_f32(t.bhi);
    } else {
        *reinterpret_cast<uint2*>(dst + 2 * PLANE) = pack4(rne_pair(t.x[0], t.x[1]), rne_pair(t.x[2], t.x[3]));
    }
}

template <bool TA, bool TB>
struct FusedCtx {
    static constexpr bool A_CK = !TA, B_CK = TB;
    TileLoader<A_CK> la;
    TileLoader<B_CK> lb;
    float4 ra[4], rb[4];                 // fp32 items of the tile being split next
    bf16x8 F0[12], F1[12];               // fragments: index = operand + 2 * t + 4 * plane
    SplitState st;
    int M, N, K, m0, n0, tid;
    int frag_a, frag_b;                  // element offsets of this lane's fragment rows inside a plane
    bool a_edge, b_edge;

    // item `it` (0..7): operand it&1 (0 = A), slot it>>1
    // FAST: the tile being split needs no out-of-range fix-up and the tile being loaded is a full one
    template <int IT, bool FAST>
    __device__ __forceinline__ void item_begin(int k0_tile, int k0_next, __bf16* wbuf, __bf16*& dst) {
        constexpr int i = IT >> 1;
        int row, k;
        float4 v;
        if constexpr ((IT & 1) == 0) {
            item_pos<A_CK>(tid + THREADS * i, row, k);
            v = ra[i];
            if (!FAST && (a_edge || k0_tile + BK > K)) v = fix_item<A_CK>(v, M, K, m0, k0_tile, row, k);
            dst = wbuf + row * LDS_ROW + k;
        } else {
            item_pos<B_CK>(tid + THREADS * i, row, k);
            v = rb[i];
            if (!FAST && (b_edge || k0_tile + BK > K)) v = fix_item<B_CK>(v, N, K, n0, k0_tile, row, k);
            dst = wbuf + 3 * PLANE + row * LDS_ROW + k;
        }
        st.x[0] = v.x; st.x[1] = v.y; st.x[2] = v.z; st.x[3] = v.w;
        if constexpr ((IT & 1) == 0) la.template load_item<FAST>(i, k0_next, ra[i]);      // the register is free again
        else lb.template load_item<FAST>(i, k0_next, rb[i]);
    }

    template <int FR>
    __device__ __forceinline__ void read_frag(bf16x8 (&F)[12], const __bf16* rbuf, int slab) {
        constexpr int op = FR & 1, t = (FR >> 1) & 1, p = FR >> 2;
        const __bf16* base = rbuf + (op ? 3 * PLANE + frag_b : frag_a);
        F[FR] = *reinterpret_cast<const bf16x8*>(base + p * PLANE + t * 32 * LDS_ROW + slab * 16);
    }
};

template <int W>
__device__ __forceinline__ void mfma_w(const bf16x8 (&F)[12], f32x16 (&acc)[2][2]) {
    constexpr int PA[6] = {2, 1, 0, 1, 0, 0};
    constexpr int PB[6] = {0, 1, 2, 0, 1, 0};
    constexpr int q = W >> 2, i = (W >> 1) & 1, j = W & 1;
    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(F[2 * i + 4 * PA[q]], F[1 + 2 * j + 4 * PB[q]], acc[i][j], 0, 0, 0);
}

// one rotated k-step (see the header comment).  WITH_OLD: slab 1 of the previous tile is pending in F1;
// WITH_CONV: there is a next tile to split.
template <bool TA, bool TB, bool WITH_OLD, bool WITH_CONV, bool FAST>
__device__ __forceinline__ void fused_step(FusedCtx<TA, TB>& c, f32x16 (&acc)[2][2], const __bf16* rbuf,
                                           __bf16* wbuf, int k0_tile, int k0_next) {
    static_for<0, 4>([&](auto fr) { c.template read_frag<fr.value>(c.F0, rbuf, 0); });
    __bf16* dst = nullptr;
    static_for<0, 48>([&](auto gc) {
        constexpr int g = gc.value;
        if constexpr (g < 24) {
            if constexpr (WITH_OLD) mfma_w<g>(c.F1, acc);
        } else {
            mfma_w<g - 24>(c.F0, acc);
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (g < 8) c.template read_frag<4 + g>(c.F0, rbuf, 0);
        if constexpr (g >= 24 && g < 36) c.template read_frag<g - 24>(c.F1, rbuf, 1);
        if constexpr (WITH_CONV) {
            constexpr int it = g / 6, stp = g % 6;
            if constexpr (stp == 0) c.template item_begin<it, FAST>(k0_tile, k0_next, wbuf, dst);
            split_step<stp>(c.st, dst);
        }
        __builtin_amdgcn_sched_barrier(0);
    });
}

template <bool TA, bool TB>
__global__ __launch_bounds__(THREADS) void gemm_split_fused_kernel(SplitArgs g) {
    extern __shared__ __attribute__((aligned(16))) __bf16 smem[];           // [2][A planes | B planes]
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    int bx, by, z;
    tile_of_block(gridDim.x, gridDim.y, g.xcd_order, bx, by, z);
    const int m0 = by * BM, n0 = bx * BN;
    const int kt0 = z * g.k_tiles_per_split;
    const int kt_total = (g.K + BK - 1) / BK;
    const int kt1 = min(kt_total, kt0 + g.k_tiles_per_split);

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    if (kt0 < kt1) {
        FusedCtx<TA, TB> c;
        c.M = g.M; c.N = g.N; c.K = g.K; c.m0 = m0; c.n0 = n0; c.tid = tid;
        c.a_edge = m0 + BM > g.M;
        c.b_edge = n0 + BN > g.N;
        c.frag_a = (wm * 64 + (lane & 31)) * LDS_ROW + (lane >> 5) * 8;
        c.frag_b = (wn * 64 + (lane & 31)) * LDS_ROW + (lane >> 5) * 8;
        c.la.init(g.A, g.lda, g.M, g.K, m0, tid);
        c.lb.init(g.B, g.ldb, g.N, g.K, n0, tid);
        c.la.load(kt0 * BK, c.ra);
        c.lb.load(kt0 * BK, c.rb);
        // prologue: split tile kt0 into buffer 0 (nothing to overlap it with), loads of tile kt0+1
        {
            const int k0_next = min(kt0 + 1, kt1 - 1) * BK;
            __bf16* dst = nullptr;
            static_for<0, 48>([&](auto gc) {
                constexpr int it = gc.value / 6, stp = gc.value % 6;
                if constexpr (stp == 0) c.template item_begin<it, false>(kt0 * BK, k0_next, smem, dst);
                split_step<stp>(c.st, dst);
            });
        }
        __syncthreads();
        // the loop is peeled so that its body is ONE straight-line variant (accumulators stay in place)
        auto step = [&](int kt, auto with_old, auto with_conv, auto fast) {
            const int cur = (kt - kt0) & 1;
            const int k0_tile = (kt + 1) * BK;                        // the tile being split in this step
            const int k0_next = min(kt + 2, kt1 - 1) * BK;            // the tile being loaded (clamped, harmless)
            fused_step<TA, TB, with_old.value, with_conv.value, fast.value>(
                c, acc, smem + cur * BUF, smem + (cur ^ 1) * BUF, k0_tile, k0_next);
            __syncthreads();
        };
        using T = std::true_type;
        using F = std::false_type;
        if (kt0 + 1 < kt1) {
            step(kt0, F{}, T{}, F{});
            int kt = kt0 + 1;
            if (!c.a_edge && !c.b_edge)          // interior tile: steady state without any edge handling
                for (; kt < kt1 - 1 && (min(kt + 2, kt1 - 1) + 1) * BK <= g.K; ++kt) step(kt, T{}, T{}, T{});
            for (; kt < kt1 - 1; ++kt) step(kt, T{}, T{}, F{});
            step(kt1 - 1, T{}, F{}, F{});
        } else {
            step(kt0, F{}, F{}, F{});
        }
        static_for<0, 24>([&](auto w) { mfma_w<w.value>(c.F1, acc); });     // slab 1 of the last tile
    }
    // (direct epilogue only: this kernel runs grids of <= 256 tiles, small outputs, in the step beside the head's planes GEMMs:
    // no gain from the staged form that a trace could tell from its own spread)
    store_tile<32, false>(g, m0, n0, z, wm, wn, lane, acc, nullptr);
}

// ------------------------------------------------------------------------------------------------------
// bf16 mode (renet_gemm_bf16; BASELINE config 5 "n_hidden=400 bf16"): the SAME tile, loaders and LDS image with ONE
// bf16 plane per operand -- every fp32 operand value is rounded to bf16 (RNE) on its way into LDS and the product
// is a single v_mfma_f32_32x32x16_bf16 with fp32 accumulation (standard bf16 mixed precision: bf16 multiplicands,
// fp32 sums, fp32 storage of every tensor).  1/6 of the matrix-pipe work of the bf16x6 kernels; the k-loop is then
// bound by staging, so the next tile's global loads are issued before the MFMA phase and land behind it.
// ------------------------------------------------------------------------------------------------------
template <bool CONTIG_K, bool EDGE>
__device__ __forceinline__ void store_items_1(__bf16* __restrict__ S, int rows, int K, int row0, int k0, int tid,
                                              const float4 (&r)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int row, k;
        item_pos<CONTIG_K>(tid + THREADS * i, row, k);
        float4 v = r[i];
        if constexpr (EDGE) v = fix_item<CONTIG_K>(v, rows, K, row0, k0, row, k);
        const f32x2 lo = {v.x, v.y}, hi = {v.z, v.w};
        *reinterpret_cast<uint2*>(S + row * LDS_ROW + k) =
            pack4(__builtin_convertvector(lo, bf16x2), __builtin_convertvector(hi, bf16x2));
    }
}

template <bool TA, bool TB>
__global__ __launch_bounds__(THREADS) void gemm_bf16_kernel(SplitArgs g) {
    __shared__ __attribute__((aligned(16))) __bf16 sA[2][PLANE];
    __shared__ __attribute__((aligned(16))) __bf16 sB[2][PLANE];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    int bx, by, z;
    tile_of_block(gridDim.x, gridDim.y, g.xcd_order, bx, by, z);
    const int m0 = by * BM, n0 = bx * BN;
    const int kt0 = z * g.k_tiles_per_split;
    const int kt_total = (g.K + BK - 1) / BK;
    const int kt1 = min(kt_total, kt0 + g.k_tiles_per_split);
    constexpr bool A_CK = !TA;
    constexpr bool B_CK = TB;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    float4 ra[4], rb[4];
    ItemLoader<A_CK> la;
    ItemLoader<B_CK> lb;
    la.init(g.A, g.lda, g.M, g.K, m0, tid);
    lb.init(g.B, g.ldb, g.N, g.K, n0, tid);
    if (kt0 < kt1) {
        la.load(kt0 * BK, ra);
        lb.load(kt0 * BK, rb);
    }
    const bool a_edge = m0 + BM > g.M, b_edge = n0 + BN > g.N;
    const int arow = (wm * 64 + (lane & 31)) * LDS_ROW;
    const int brow = (wn * 64 + (lane & 31)) * LDS_ROW;
    const int ksel = (lane >> 5) * 8;
    for (int kt = kt0; kt < kt1; ++kt) {
        const int buf = (kt - kt0) & 1;                 // LDS double buffer: ONE barrier per k-tile
        const bool k_edge = (kt + 1) * BK > g.K;
        if (a_edge || k_edge) store_items_1<A_CK, true>(sA[buf], g.M, g.K, m0, kt * BK, tid, ra);
        else store_items_1<A_CK, false>(sA[buf], g.M, g.K, m0, kt * BK, tid, ra);
        if (b_edge || k_edge) store_items_1<B_CK, true>(sB[buf], g.N, g.K, n0, kt * BK, tid, rb);
        else store_items_1<B_CK, false>(sB[buf], g.N, g.K, n0, kt * BK, tid, rb);
        __syncthreads();
        if (kt + 1 < kt1) {                             // in flight behind the MFMAs
            la.load((kt + 1) * BK, ra);
            lb.load((kt + 1) * BK, rb);
        }
#pragma unroll
        for (int slab = 0; slab < 2; ++slab) {
            const int ko = slab * 16 + ksel;
            bf16x8 a[2], b[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                a[t] = *reinterpret_cast<const bf16x8*>(&sA[buf][arow + t * 32 * LDS_ROW + ko]);
                b[t] = *reinterpret_cast<const bf16x8*>(&sB[buf][brow + t * 32 * LDS_ROW + ko]);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
    // (direct epilogue only: staged, this kernel gained 2-3 % of the bf16 step in most runs and lost as much in some)
    store_tile<32, false>(g, m0, n0, z, wm, wn, lane, acc, nullptr);
}

__global__ __launch_bounds__(256) void split_reduce_kernel(const float* __restrict__ partial, int split_k,
                                                           int M, int N, float alpha, float beta,
                                                           const float* __restrict__ bias,
                                                           float* __restrict__ C, int ldc) {
    const size_t total = (size_t)M * N;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (size_t)gridDim.x * blockDim.x) {
        const int m = (int)(i / N), n = (int)(i % N);
        float s = 0.f;
        for (int zz = 0; zz < split_k; ++zz) s += partial[(size_t)zz * total + i];
        float v = alpha * s + (bias ? bias[n] : 0.f);
        float* p = C + (size_t)m * ldc + n;
        if (beta != 0.f) v += beta * (*p);
        *p = v;
    }
}

// The same reduction for SMALL outputs with many slices (dW of the 200x200 / 600x200 weights: 40k-120k elements,
// 39-128 slices): one thread per element leaves most of the chip idle and walks the slices serially, so the 4
// waves of a workgroup split the slices (wave w takes z = w, w+4, ...: every load a coalesced 256-byte row
// segment) and combine through LDS in a fixed order.
__global__ __launch_bounds__(256) void split_reduce4_kernel(const float* __restrict__ partial, int split_k,
                                                            int M, int N, float alpha, float beta,
                                                            const float* __restrict__ bias,
                                                            float* __restrict__ C, int ldc) {
    __shared__ float red[4][64];
    const size_t total = (size_t)M * N;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t i = (size_t)blockIdx.x * 64 + lane;
    float s0 = 0.f, s1 = 0.f;
    if (i < total) {
        int zz = wave;
        for (; zz + 4 < split_k; zz += 8) {
            s0 += partial[(size_t)zz * total + i];
            s1 += partial[(size_t)(zz + 4) * total + i];
        }
        if (zz < split_k) s0 += partial[(size_t)zz * total + i];
    }
    red[wave][lane] = s0 + s1;
    __syncthreads();
    if (wave == 0 && i < total) {
        const int m = (int)(i / N), n = (int)(i % N);
        const float s = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
        float v = alpha * s + (bias ? bias[n] : 0.f);
        float* p = C + (size_t)m * ldc + n;
        if (beta != 0.f) v += beta * (*p);
        *p = v;
    }
}

template <bool TA, bool TB>
int launch_fused(const SplitArgs& g, dim3 grid, hipStream_t st) {
    static bool attr_set = false;      // benign race: the attribute is idempotent
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute((const void*)gemm_split_fused_kernel<TA, TB>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)FUSED_LDS);
        if (e != hipSuccess) return (int)e;
        attr_set = true;
    }
    RENET_LAUNCH((gemm_split_fused_kernel<TA, TB>), grid, dim3(THREADS), FUSED_LDS, st, g);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}

template <bool TA, bool TB, bool RAW>
int launch_tall(const SplitArgs& g, dim3 grid, hipStream_t st) {
    static bool attr_set = false;      // benign race: the attribute is idempotent
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute((const void*)gemm_split_tall_kernel<TA, TB, RAW>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)TALL_LDS);
        if (e != hipSuccess) return (int)e;
        attr_set = true;
    }
    RENET_LAUNCH((gemm_split_tall_kernel<TA, TB, RAW>), grid, dim3(THREADS_T), TALL_LDS, st, g);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}

// 256-row tiles when the output has enough of them to fill the chip a few times (RENET_GEMM_TALL=0 disables,
// =<n> sets the minimum tile count)
bool use_tall(int ta, int M, int nbx, int split_k) {
    static const int forced = renet_env_int("RENET_GEMM_TALL", -1, 0, 0x7fffffff);      // -1: not set
    const long tiles = (long)nbx * ((M + BMT - 1) / BMT) * split_k;
    if (forced >= 0) return forced > 0 && tiles >= forced;
    // measured: logits 2048 x 23033 x 600 (1440 tiles) 395 -> 362 us; dW 23033 x 600 x 2048 (450 tiles: 1.76 rounds) 447 -> 480 us
    // round 4: as for the f16x3 kernels (use_tall_h3), K-contiguous A with a split k range from 200 tiles on (dfeat)
    return tiles >= 1000 || (!ta && split_k >= 4 && tiles >= 200);
}

// Which k-loop: the fused kernel (one workgroup per CU, 122.9 KB LDS) when the whole grid fits in ONE round of
// 256 workgroups -- there a lone workgroup finishes a k-tile in ~2500 cycles against ~3900 for the two-phase
// kernel (MI355X: 51 vs 35 TFLOP/s on a 64-tile problem, 155 vs 126 on 256 tiles) -- and the two-phase kernel
// with two co-resident workgroups per CU beyond that, where its second workgroup covers the prologue, the
// C-store epilogue and the barrier waits of the first (short K loops: 133 vs 117 TFLOP/s on the 1440-tile
// K=600 logits GEMM).  RENET_GEMM_KERNEL=fused|split forces one of them (tools/gemm_bench.py).
int kernel_choice(int ntiles) {
    static const int forced = renet_env_is("RENET_GEMM_KERNEL", "split") ? 1 : renet_env_is("RENET_GEMM_KERNEL", "fused") ? 0 : -1;
    if (forced >= 0) return forced;
    return ntiles <= 256 ? 0 : 1;
}

}  // namespace

int renet_split_reduce(const float* partial, int split_k, int M, int N, float alpha, float beta, const float* bias,
                       float* C, int ldc, hipStream_t st) {
    const size_t total = (size_t)M * N;
    if (total <= (size_t)256 * 1024 && split_k >= 8) {
        RENET_LAUNCH(split_reduce4_kernel, dim3((unsigned)((total + 63) / 64)), dim3(256), 0, st, partial, split_k, M, N,
                     alpha, beta, bias, C, ldc);
    } else {
        int blocks = (int)min((size_t)2048, (total + 255) / 256);
        RENET_LAUNCH(split_reduce_kernel, dim3(blocks), dim3(256), 0, st, partial, split_k, M, N, alpha, beta, bias, C, ldc);
    }
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}

extern "C" {

#ifdef RENET_GEMM_TRACE
int renet_gemm_h3_trace_set(unsigned long long* buf);      // gemm_h3.hip: every translation unit has its own g_trace
int renet_gemm_trace_set(unsigned long long* buf) {
    const int e = (int)hipMemcpyToSymbol(HIP_SYMBOL(g_trace), &buf, sizeof(buf));
    return e ? e : renet_gemm_h3_trace_set(buf);
}
#endif

// What the bf16x6 / bf16 launcher does for a problem: ONE function decides, the launcher executes it and
// renet_gemm_split_plan reports it (host logic only -- testable without a GPU).
struct SplitPlan {
    int kernel;            // 0 fused (one workgroup per CU), 1 two-phase 128 x 128, 2 two-phase 256 x 128, 3 weight-resident
                           // (gemm_skinny.hip), 4 single-plane bf16 (renet_gemm_bf16)
    int raw;               // two-phase kernels: operands through raw buffer descriptors
    int xcd_order;         // 0 plain tile order, w: XCD-aware order with panels of <= w tiles
    int gx, gy, gz;        // grid
    int split_k;           // clamped split
};

static SplitPlan plan_split(bool bf16_mode, int ta, int tb, int M, int N, int K, const float* A, int lda, const float* B,
                            int ldb, int split_k) {
    SplitPlan p;
    const int kt_total = (K + BK - 1) / BK;
    if (split_k < 1) split_k = 1;
    if (split_k > kt_total) split_k = max(kt_total, 1);
    p.split_k = split_k;
    p.raw = 0;
    p.xcd_order = renet_gemm_tile_order();
    const int nbx = (N + BN - 1) / BN, nby = (M + BM - 1) / BM;
    p.gx = nbx; p.gy = nby; p.gz = split_k;
    // tall activation x small weight (K <= 208, N <= 256): the weight-resident kernel of gemm_skinny.hip
    // (RENET_GEMM_SKINNY=0 in the environment keeps the general kernels, for A/B runs)
    if (!bf16_mode && split_k == 1 && renet_gemm_skinny_enabled() && renet_gemm_skinny_eligible(ta, M, N, K, A, lda, B, ldb, tb)) {
        p.kernel = 3;
        return p;
    }
    const int ntiles = nbx * nby * split_k;
    int choice = bf16_mode ? 2 : kernel_choice(ntiles);
    // the fused kernel addresses with 32-bit element offsets and float4 loads along a contiguous K
    if (choice == 0 && (K < 4 || (size_t)(ta ? K : M) * lda >= (1u << 31) || (size_t)(tb ? N : K) * ldb >= (1u << 31)))
        choice = 1;
    if (choice == 0) { p.kernel = 0; return p; }
    if (choice == 2) { p.kernel = 4; return p; }
    // two-phase kernels: raw buffer descriptors (32-bit byte offsets) while both operands reach less than 2^30 elements
    // (the generic 64-bit loader beyond that)
    p.raw = (size_t)(ta ? K : M) * lda < ((size_t)1 << 30) && (size_t)(tb ? N : K) * ldb < ((size_t)1 << 30);
    if (use_tall(ta, M, nbx, split_k)) {
        p.kernel = 2;
        p.gy = (M + BMT - 1) / BMT;
        p.xcd_order = panel_width(p.xcd_order, nbx, p.gy, BMT, K, split_k, 32);
    } else {
        p.kernel = 1;
        p.xcd_order = panel_width(p.xcd_order, nbx, nby, BM, K, split_k, 64);
    }
    return p;
}

static int gemm_split_launch(bool bf16_mode, int ta, int tb, int M, int N, int K, float alpha, const float* A, int lda,
                              const float* B, int ldb, float beta, float* C, int ldc, const float* bias,
                              int split_k, float* workspace, size_t workspace_bytes, void* stream) {
    if (M < 0 || N < 0 || K < 1 || lda <= 0 || ldb <= 0 || ldc < N) return RENET_ERR_BADARG;
    if (M == 0 || N == 0) return RENET_OK;
    const SplitPlan p = plan_split(bf16_mode, ta, tb, M, N, K, A, lda, B, ldb, split_k);
    split_k = p.split_k;
    const int kt_total = (K + BK - 1) / BK;
    if (split_k > 1 && workspace_bytes < renet_gemm_workspace(M, N, split_k)) return RENET_ERR_WORKSPACE;
    if (p.kernel == 3) return renet_gemm_skinny_launch(tb, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, bias, stream);
    SplitArgs g;
    g.A = A; g.B = B; g.C = C; g.bias = bias; g.M = M; g.N = N; g.K = K;
    g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.alpha = alpha; g.beta = beta;
    g.split_k = split_k;
    g.k_tiles_per_split = max(1, (kt_total + split_k - 1) / split_k);
    g.partial = workspace;
    g.xcd_order = p.xcd_order;
    g.staged = renet_gemm_epilogue_staged();
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(p.gx, p.gy, p.gz);
    const bool raw = p.raw != 0;
    int e = RENET_OK;
    if (p.kernel == 0) {
        if (!ta && !tb) e = launch_fused<false, false>(g, grid, st);
        else if (!ta && tb) e = launch_fused<false, true>(g, grid, st);
        else if (ta && !tb) e = launch_fused<true, false>(g, grid, st);
        else e = launch_fused<true, true>(g, grid, st);
    } else if (p.kernel == 4) {
        if (!ta && !tb) RENET_LAUNCH((gemm_bf16_kernel<false, false>), grid, dim3(THREADS), 0, st, g);
        else if (!ta && tb) RENET_LAUNCH((gemm_bf16_kernel<false, true>), grid, dim3(THREADS), 0, st, g);
        else if (ta && !tb) RENET_LAUNCH((gemm_bf16_kernel<true, false>), grid, dim3(THREADS), 0, st, g);
        else RENET_LAUNCH((gemm_bf16_kernel<true, true>), grid, dim3(THREADS), 0, st, g);
    } else if (p.kernel == 2) {
#define RENET_TALL_LAUNCH(RAWV)                                                     \
        do {                                                                        \
            if (!ta && !tb) e = launch_tall<false, false, RAWV>(g, grid, st);       \
            else if (!ta && tb) e = launch_tall<false, true, RAWV>(g, grid, st);    \
            else if (ta && !tb) e = launch_tall<true, false, RAWV>(g, grid, st);    \
            else e = launch_tall<true, true, RAWV>(g, grid, st);                    \
        } while (0)
        if (raw) RENET_TALL_LAUNCH(true);
        else RENET_TALL_LAUNCH(false);
#undef RENET_TALL_LAUNCH
    } else {
#define RENET_SPLIT_LAUNCH(RAWV)                                                                                    \
        do {                                                                                                        \
            if (!ta && !tb) RENET_LAUNCH((gemm_split_kernel<false, false, RAWV>), grid, dim3(THREADS), 0, st, g);   \
            else if (!ta && tb) RENET_LAUNCH((gemm_split_kernel<false, true, RAWV>), grid, dim3(THREADS), 0, st, g); \
            else if (ta && !tb) RENET_LAUNCH((gemm_split_kernel<true, false, RAWV>), grid, dim3(THREADS), 0, st, g); \
            else RENET_LAUNCH((gemm_split_kernel<true, true, RAWV>), grid, dim3(THREADS), 0, st, g);                \
        } while (0)
        if (raw) RENET_SPLIT_LAUNCH(true);
        else RENET_SPLIT_LAUNCH(false);
#undef RENET_SPLIT_LAUNCH
    }
    if (e != RENET_OK) return e;
    RENET_LAUNCH_CHECK();
    if (split_k > 1) return renet_split_reduce(workspace, split_k, M, N, alpha, beta, bias, C, ldc, st);
    return RENET_OK;
}


int renet_gemm_f32_split(int ta, int tb, int M, int N, int K, float alpha, const float* A, int lda,
                         const float* B, int ldb, float beta, float* C, int ldc, const float* bias,
                         int split_k, float* workspace, size_t workspace_bytes, void* stream) {
    return gemm_split_launch(false, ta, tb, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, bias, split_k, workspace,
                              workspace_bytes, stream);
}

int renet_gemm_split_plan(int ta, int tb, int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                          int split_k, int* plan) {
    if (!plan || M < 1 || N < 1 || K < 1 || lda <= 0 || ldb <= 0) return RENET_ERR_BADARG;
    const SplitPlan p = plan_split(false, ta, tb, M, N, K, A, lda, B, ldb, split_k);
    plan[0] = p.kernel; plan[1] = p.raw; plan[2] = p.xcd_order; plan[3] = p.gx; plan[4] = p.gy; plan[5] = p.gz;
    plan[6] = p.split_k;
    plan[7] = 0;
    return RENET_OK;
}

int renet_gemm_bf16(int ta, int tb, int M, int N, int K, float alpha, const float* A, int lda,
                    const float* B, int ldb, float beta, float* C, int ldc, const float* bias,
                    int split_k, float* workspace, size_t workspace_bytes, void* stream) {
    return gemm_split_launch(true, ta, tb, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, bias, split_k, workspace,
                              workspace_bytes, stream);
}

}  // extern "C"
