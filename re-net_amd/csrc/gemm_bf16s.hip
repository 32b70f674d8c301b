// bf16-STORAGE GEMM (renet_gemm_bf16s, BASELINE config 5 "n_hidden=400 bf16"): both operands are bf16 matrices in
// HBM ([Rp][Cp], padded with zeros to multiples of 128), ONE product per fragment
// pair, fp32 accumulation.  The LDS-DMA ring, wave specialisation, images and swizzles described above; a
// ring slot holds TWO 32-wide k sub-tiles per operand (4 x 8 KB = 32 KB per slot, 3 slots), so a stage is 128 x 128 x 64: 16 MFMAs per MFMA wave and barrier.  With one product per
// element pair the k-loop moves 16 KB of operands per 1 MFLOP: the kernel is bound by the L2 -> LDS stream, not by
// the matrix pipe.  Either operand may be consumed K-contiguous or K-strided (ds_read_b64_tr_b16).
//
// LDS-DMA ring of this kernel (the three-plane "planes" GEMM that introduced it in round 2 was
// measured against the in-loop split, not adopted -- DESIGN 4b -- and removed in round 5): operands are bf16 matrices
// [rows][cols] in HBM, both dims padded with zeros to multiples of 128 (no edge handling in the loop); a k-tile is
// global_load_lds_dwordx4 pieces (no VGPRs, no VALU, no ds_write) into a 3-deep LDS ring with ONE raw s_barrier per
// k-tile.  An operand is consumed in one of two roles:
//   K-CONTIGUOUS (tr = 0): rows = the operand's M (N) index, cols = K.  Tile image in LDS: [128 rows][32 k], 64-byte
//       rows, the four 16-byte chunks of a row XOR-swizzled by (row >> 2) & 3 -- applied on the SOURCE address of
//       the DMA (the LDS side of global_load_lds is lane-linear) -- which makes every ds_read_b128 fragment read
//       conflict free.
//   K-STRIDED (tr = 1): rows = K, cols = the operand's M (N) index (the tensor as stored when the contraction runs
//       over its rows: dW = dlogits^T feat, dfeat = dlogits W).  Tile image [32 k][128 cols], 256-byte rows, the
//       sixteen 16-byte chunks XOR-swizzled by 4 * (k & 3); fragments come from two ds_read_b64_tr_b16 each (gfx950's
//       transposing LDS read: in a 16-lane group, lane i receives element i & 3 of the 8-byte chunks addressed by
//       lanes (i >> 2) + 4 j, j = 0..3 -- measured with tools/probes/tr_probe.hip).
// ------------------------------------------------------------------------------------------------------
// Wave specialisation: a workgroup is 8 waves -- waves 0..3 (one per SIMD) only read fragments and issue MFMAs, waves
// 4..7 (their SIMD partners) only issue the LDS-DMA.  A global_load_lds costs the issuing wave ~60-100 cycles of issue
// time (12 per k-tile and wave: as much as half the tile's MFMA time when the MFMA wave has to issue them itself,
// measured: 3200 cycles per k-tile against 1536 of matrix-pipe time); from a partner wave it overlaps the MFMAs.
//   ring of 3 slots, ONE s_barrier per round, all 8 waves:
//     loader, round k : issue tile k + 2 into slot (k + 2) % 3   [held tile k - 1: every MFMA wave finished reading it
//                                                                 before barrier k - 1]
//                       s_waitcnt vmcnt(12)                       [tile k + 1 landed; tile k + 2 stays in flight]
//                       barrier k
//     MFMA wave, round k : fragments of tile k (slot k % 3), 48 MFMAs with the slab-1 reads behind the first 12,
//                          s_waitcnt lgkmcnt(0), barrier k
#include "gemm_tiles.h"

namespace {

constexpr int P3_LOADERS = 4;                           // loader waves per workgroup (48 DMA pieces per k-tile)
constexpr int P3_THREADS = 64 * (4 + P3_LOADERS);

struct Bf16sArgs {
    const __bf16* A;
    const __bf16* B;
    int lda, ldb;               // row stride (elements)
    SplitArgs out;              // M, N, K, C, ldc, alpha, beta, bias, split-K fields; k_tiles_per_split in 64-wide STAGES
};

constexpr int B1_SUB = 2;                                 // k sub-tiles per operand and ring slot
constexpr int B1_BK = 32 * B1_SUB;                        // k per stage
constexpr int B1_STAGE = 2 * B1_SUB * 8192;
constexpr int B1_SLOTS = 3;
constexpr size_t B1_LDS = (size_t)B1_STAGE * B1_SLOTS;
constexpr size_t B1_LDS_TALL = (size_t)B1_SUB * (256 * 64 + 8192) * B1_SLOTS;

// TALL: 256 x 128 tile, 8 MFMA waves (4 x 2, two per SIMD: one wave's barrier wait is covered by its partner's
// MFMAs) + 4 loader waves; A images are 16 KB (256 rows K-contiguous / 256 columns K-strided).  0.75x the operand
// bytes per flop of the 128 x 128 tile.
template <bool A_TR, bool B_TR, bool TALL>
__global__ __launch_bounds__(TALL ? 768 : P3_THREADS) void gemm_bf16s_kernel(Bf16sArgs pa) {
    constexpr int TBM = TALL ? 256 : 128;
    constexpr int MW = TALL ? 8 : 4;                       // MFMA waves
    constexpr int AIMG = TBM * 64;                         // bytes of one A sub-tile image
    constexpr int APIECES = TBM / 16;                      // 1 KB DMA pieces per A image
    constexpr int STAGE = B1_SUB * (AIMG + 8192);
    constexpr int NPIECE = B1_SUB * (APIECES + 8);
    constexpr int PER = NPIECE / P3_LOADERS;               // 8 (128-row tile) or 12 (256-row tile)
    extern __shared__ __attribute__((aligned(16))) char ring1[];
    const SplitArgs& g = pa.out;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int bx, by, z;
    tile_of_block(gridDim.x, gridDim.y, g.xcd_order, bx, by, z);
    const int m0 = by * TBM, n0 = bx * BN;
    const int st_total = (g.K + B1_BK - 1) / B1_BK;
    const int s0 = z * g.k_tiles_per_split;
    const int s1 = min(st_total, s0 + g.k_tiles_per_split);
    const int nk = max(s1 - s0, 0);

    if (wave >= MW) {
        if (nk == 0) return;
        const int lw = wave - MW;
        const __bf16* src[PER];
        int dst[PER];
        bool is_b[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int id = lw + P3_LOADERS * i;
            // pieces 0 .. B1_SUB * APIECES - 1: A (sub-tile major), then B
            const int opnd = id >= B1_SUB * APIECES ? 1 : 0;
            const int idl = opnd ? id - B1_SUB * APIECES : id;
            const int per_sub = opnd ? 8 : APIECES;
            const int sub = idl / per_sub, piece = idl % per_sub;
            is_b[i] = opnd != 0;
            const bool tr = opnd ? B_TR : A_TR;
            const __bf16* base = opnd ? pa.B : pa.A;
            const int ld = opnd ? pa.ldb : pa.lda;
            const int r0 = opnd ? n0 : m0;
            const size_t k0 = (size_t)s0 * B1_BK + sub * 32;
            size_t off;
            int img_off;
            if (!tr) {                                   // [rows][32 k]: piece = 16 rows x 64 B
                const int row = 16 * piece + (lane >> 2);
                const int chunk = (lane & 3) ^ ((row >> 2) & 3);
                off = (size_t)(r0 + row) * ld + k0 + chunk * 8;
                img_off = piece * 1024;
            } else {                                     // [32 k][cols]: 128-column panels of 8 KB, piece = 4 k x 256 B
                const int panel = piece >> 3, pc = piece & 7;
                const int kk = 4 * pc + (lane >> 4);
                const int log16 = (lane & 15) ^ (4 * (kk & 3));
                off = (k0 + kk) * ld + r0 + panel * 128 + log16 * 8;
                img_off = panel * 8192 + pc * 1024;
            }
            src[i] = base + off;
            dst[i] = (opnd ? B1_SUB * AIMG + sub * 8192 : sub * AIMG) + img_off;
        }
        const size_t a_step = A_TR ? (size_t)B1_BK * pa.lda : (size_t)B1_BK;
        const size_t b_step = B_TR ? (size_t)B1_BK * pa.ldb : (size_t)B1_BK;
        auto issue_all = [&](int slot) {
            char* base = ring1 + slot * STAGE;
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src[i],
                                                 (__attribute__((address_space(3))) void*)(base + dst[i]), 16, 0, 0);
                src[i] += is_b[i] ? b_step : a_step;
            }
        };
        static_assert(PER == 8 || PER == 12, "counted waits below");
        auto wait_one_stage = [&]() {
            if constexpr (PER == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        };
        issue_all(0);
        if (nk > 1) {
            issue_all(1);
            wait_one_stage();
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();                                     // barrier -1: stage 0 visible
        for (int kt = 0; kt < nk; ++kt) {
            if (kt + 2 < nk) {
                issue_all((kt + 2) % B1_SLOTS);
                wait_one_stage();
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            __builtin_amdgcn_s_barrier();                                 // barrier kt: stage kt + 1 visible
        }
        return;
    }

    // ---------------- MFMA waves ----------------
    const int wm = wave >> 1, wn = wave & 1;               // wm: 0..1 (128-row tile) or 0..3 (256-row tile)
    int offA[2][2], offB[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if constexpr (!A_TR) {
                const int row = wm * 64 + 32 * t + (lane & 31);
                offA[t][u] = row * 64 + (((2 * u + (lane >> 5)) ^ ((row >> 2) & 3)) * 16);
            } else {
                const int sl = lane & 15;
                const int colf = wm * 64 + 32 * t + 16 * ((lane >> 4) & 1) + 4 * (sl & 3);
                const int col = colf & 127;                  // inside its 128-column panel
                const int kk = 8 * (lane >> 5) + 4 * u + (sl >> 2);
                offA[t][u] = (colf >> 7) * 8192 + kk * 256 + (((col >> 3) ^ (4 * (kk & 3))) * 16) + ((col >> 2) & 1) * 8;
            }
            if constexpr (!B_TR) {
                const int row = wn * 64 + 32 * t + (lane & 31);
                offB[t][u] = row * 64 + (((2 * u + (lane >> 5)) ^ ((row >> 2) & 3)) * 16);
            } else {
                const int sl = lane & 15;
                const int col = wn * 64 + 32 * t + 16 * ((lane >> 4) & 1) + 4 * (sl & 3);
                const int kk = 8 * (lane >> 5) + 4 * u + (sl >> 2);
                offB[t][u] = kk * 256 + (((col >> 3) ^ (4 * (kk & 3))) * 16) + ((col >> 2) & 1) * 8;
            }
        }
    auto frag_tr = [&](const char* img, const int (&off)[2], int slab) {
        bf16x8 r;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (__attribute__((address_space(3))) s16x4*)(img + off[q] + slab * 4096));
#pragma unroll
            for (int j = 0; j < 4; ++j) r[4 * q + j] = __builtin_bit_cast(__bf16, (short)v[j]);
        }
        return r;
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    if (nk > 0) __builtin_amdgcn_s_barrier();                             // barrier -1
    for (int kt = 0; kt < nk; ++kt) {
        const char* st = ring1 + (kt % B1_SLOTS) * STAGE;
        bf16x8 fa[B1_SUB][2][2], fb[B1_SUB][2][2];                        // [sub][slab][t]: all 16 reads issued up front
#pragma unroll
        for (int sb = 0; sb < B1_SUB; ++sb)
#pragma unroll
            for (int slab = 0; slab < 2; ++slab)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const char* ia = st + sb * AIMG;
                    const char* ib = st + B1_SUB * AIMG + sb * 8192;
                    if constexpr (!A_TR) fa[sb][slab][t] = *reinterpret_cast<const bf16x8*>(ia + offA[t][slab]);
                    else fa[sb][slab][t] = frag_tr(ia, offA[t], slab);
                    if constexpr (!B_TR) fb[sb][slab][t] = *reinterpret_cast<const bf16x8*>(ib + offB[t][slab]);
                    else fb[sb][slab][t] = frag_tr(ib, offB[t], slab);
                }
#pragma unroll
        for (int sb = 0; sb < B1_SUB; ++sb)
#pragma unroll
            for (int slab = 0; slab < 2; ++slab)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[sb][slab][i], fb[sb][slab][j], acc[i][j], 0, 0, 0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                                     // barrier kt
    }
    // staged epilogue: MFMA wave w's 8 KB of the ring (32 / 64 KB of 96 / 144); the last round's barrier stands behind every
    // fragment read and behind the loaders' vmcnt(0)
    static_assert((size_t)MW * EPI_WAVE_FLOATS * sizeof(float) <= (TALL ? B1_LDS_TALL : B1_LDS), "staging fits the ring");
    store_tile(g, m0, n0, z, wm, wn, lane, acc, reinterpret_cast<float*>(ring1) + wave * EPI_WAVE_FLOATS);
}

// fp32 [R, C] (row stride ldx) -> ONE bf16 matrix [Rp][Cp] (RNE), padding written as zeros
__global__ __launch_bounds__(256) void pack_bf16_kernel(const float* __restrict__ X, int R, int C, int ldx, int Rp,
                                                        int Cp, __bf16* __restrict__ P) {
    const size_t total = (size_t)Rp * Cp / 4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(i / (Cp / 4)), c = (int)(i % (Cp / 4)) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < R) {
            const float* x = X + (size_t)row * ldx + c;
            if (c + 3 < C && ((ldx & 3) == 0) && ((reinterpret_cast<uintptr_t>(X) & 15) == 0)) {
                v = *reinterpret_cast<const float4*>(x);
            } else {
                if (c < C) v.x = x[0];
                if (c + 1 < C) v.y = x[1];
                if (c + 2 < C) v.z = x[2];
                if (c + 3 < C) v.w = x[3];
            }
        }
        const bf16x2 lo = __builtin_convertvector(f32x2{v.x, v.y}, bf16x2);
        const bf16x2 hi = __builtin_convertvector(f32x2{v.z, v.w}, bf16x2);
        *reinterpret_cast<uint2*>(P + (size_t)row * Cp + c) = pack4(lo, hi);
    }
}

template <bool A_TR, bool B_TR, bool TALL>
int launch_bf16s(const Bf16sArgs& pa, dim3 grid, hipStream_t st) {
    constexpr size_t lds = TALL ? B1_LDS_TALL : B1_LDS;
    static bool attr_set = false;      // benign race: the attribute is idempotent
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute((const void*)gemm_bf16s_kernel<A_TR, B_TR, TALL>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
        attr_set = true;
    }
    RENET_LAUNCH((gemm_bf16s_kernel<A_TR, B_TR, TALL>), grid, dim3(TALL ? 768 : P3_THREADS), lds, st, pa);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}

}  // namespace

extern "C" {

size_t renet_bf16_bytes(int R, int C) {
    const size_t rp = ((size_t)R + 255) & ~(size_t)255, cp = ((size_t)C + 255) & ~(size_t)255;
    return rp * cp * sizeof(__bf16);
}

int renet_pack_bf16(const float* X, int R, int C, int ldx, void* out, void* stream) {
    if (R < 0 || C < 0 || ldx < C || !out) return RENET_ERR_BADARG;
    const int Rp = (R + 255) & ~255, Cp = (C + 255) & ~255;
    if (Rp == 0 || Cp == 0) return RENET_OK;
    const size_t total = (size_t)Rp * Cp / 4;
    const int blocks = (int)min((size_t)4096, (total + 255) / 256);
    RENET_LAUNCH(pack_bf16_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, X, R, C, ldx, Rp, Cp, (__bf16*)out);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}

int renet_bf16_zero_padding(void* P, int rows, int C, int ld, int rows_alloc, void* stream) {
    if (!P || rows < 0 || C < 0 || ld < C || rows_alloc < rows) return RENET_ERR_BADARG;
    __bf16* p = (__bf16*)P;
    hipStream_t st = (hipStream_t)stream;
    const int c16 = min((C + 63) & ~63, ld), r16 = min((rows + 63) & ~63, rows_alloc);
    if (c16 > C && rows > 0) {
        hipError_t e = hipMemset2DAsync(p + C, (size_t)ld * sizeof(__bf16), 0, (size_t)(c16 - C) * sizeof(__bf16),
                                        (size_t)rows, st);
        if (e != hipSuccess) return (int)e;
    }
    if (r16 > rows) {
        hipError_t e = hipMemsetAsync(p + (size_t)rows * ld, 0, (size_t)(r16 - rows) * ld * sizeof(__bf16), st);
        if (e != hipSuccess) return (int)e;
    }
    return RENET_OK;
}

int renet_gemm_bf16s(int a_tr, int b_tr, int M, int N, int K, float alpha, const void* Ap, int lda, const void* Bp,
                     int ldb, float beta, float* C, int ldc, const float* bias, int split_k, float* workspace,
                     size_t workspace_bytes, void* stream) {
    if (M < 0 || N < 0 || K < 1 || ldc < N || !Ap || !Bp) return RENET_ERR_BADARG;
    if (M == 0 || N == 0) return RENET_OK;
    const int Mp = (M + 255) & ~255, Np = (N + 255) & ~255, Kp = (K + 255) & ~255;
    if (lda < (a_tr ? Mp : Kp) || ldb < (b_tr ? Np : Kp) || (lda & 7) || (ldb & 7)) return RENET_ERR_BADARG;
    if (split_k < 1) split_k = 1;
    const int st_total = (K + B1_BK - 1) / B1_BK;
    if (split_k > st_total) split_k = max(st_total, 1);
    if (split_k > 1 && workspace_bytes < renet_gemm_workspace(M, N, split_k)) return RENET_ERR_WORKSPACE;
    Bf16sArgs pa;
    pa.A = (const __bf16*)Ap; pa.B = (const __bf16*)Bp;
    pa.lda = lda; pa.ldb = ldb;
    SplitArgs& g = pa.out;
    g.A = nullptr; g.B = nullptr; g.C = C; g.bias = bias; g.M = M; g.N = N; g.K = K;
    g.lda = 0; g.ldb = 0; g.ldc = ldc; g.alpha = alpha; g.beta = beta;
    g.split_k = split_k;
    g.k_tiles_per_split = max(1, (st_total + split_k - 1) / split_k);
    g.partial = workspace;
    g.xcd_order = renet_gemm_tile_order();
    g.staged = renet_gemm_epilogue_staged();
    hipStream_t st = (hipStream_t)stream;
    // 256 x 128 tiles when they still fill the chip (>= 256 workgroups); the matrices are padded to multiples of
    // 256 in both dimensions, so a 256-row (or, K-strided, 256-column) A image never leaves the buffer
    const int nbx = (N + BN - 1) / BN;
    const bool tall = (size_t)nbx * (Mp / 256) * split_k >= 256;
    dim3 grid(nbx, tall ? Mp / 256 : (M + BM - 1) / BM, split_k);
    int e;
    if (tall) {
        if (!a_tr && !b_tr) e = launch_bf16s<false, false, true>(pa, grid, st);
        else if (!a_tr && b_tr) e = launch_bf16s<false, true, true>(pa, grid, st);
        else if (a_tr && !b_tr) e = launch_bf16s<true, false, true>(pa, grid, st);
        else e = launch_bf16s<true, true, true>(pa, grid, st);
    } else {
        if (!a_tr && !b_tr) e = launch_bf16s<false, false, false>(pa, grid, st);
        else if (!a_tr && b_tr) e = launch_bf16s<false, true, false>(pa, grid, st);
        else if (a_tr && !b_tr) e = launch_bf16s<true, false, false>(pa, grid, st);
        else e = launch_bf16s<true, true, false>(pa, grid, st);
    }
    if (e != RENET_OK) return e;
    if (split_k > 1) return renet_split_reduce(workspace, split_k, M, N, alpha, beta, bias, C, ldc, st);
    return RENET_OK;
}

}  // extern "C"
