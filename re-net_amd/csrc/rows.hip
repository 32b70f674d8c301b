// Row gather and deterministic segmented add (the embedding lookups and their gradients), and the ABI version.
#include "common.h"

namespace {

// ---- row gather / segmented add ---------------------------------------------------------------
__global__ __launch_bounds__(256) void gather_rows_kernel(const float4* __restrict__ table,
                                                          const int32_t* __restrict__ idx, int n, int CH,
                                                          float4* __restrict__ out) {
    const size_t total = (size_t)n * CH;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (size_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / CH), c = (int)(i % CH);
        out[i] = table[(size_t)idx[r] * CH + c];
    }
}

// dst[target[u]] += sum of the rows src[order[k]], k in [seg_ptr[u], seg_ptr[u+1])  -- deterministic (fixed association
// order per segment length), no atomics.  Segment lengths are Zipf-like (most entities own 1-8 rows of a batch, the
// hottest entity / relation hundreds), and both ends are latency problems, not bandwidth problems:
//   * short segments (<= kSegShort rows): ONE WAVE per segment, all its row loads in flight at once (clamped,
//     branch-free) -- 16 segments per 1024-thread workgroup instead of one 256-thread workgroup per 2-row segment;
//   * long segments: the workgroup's 16 waves walk the segment together, 8 independent row loads per wave and round
//     (128 rows in flight), then a fixed-order LDS combine.
// blockIdx.y selects one of two (source, destination) pairs that share the plan (renet_segment_add2).
constexpr int kSegWaves = 16, kSegShort = 16, kSegUnr = 8;
__global__ __launch_bounds__(kSegWaves * 64) void segment_add_kernel(const float4* __restrict__ src0,
                                                                     const float4* __restrict__ src1,
                                                                     const int32_t* __restrict__ order,
                                                                     const int32_t* __restrict__ seg_ptr,
                                                                     const int32_t* __restrict__ seg_target,
                                                                     int U, int CH, float4* __restrict__ dst0,
                                                                     float4* __restrict__ dst1) {
    const float4* __restrict__ src = blockIdx.y ? src1 : src0;
    float4* __restrict__ dst = blockIdx.y ? dst1 : dst0;
    __shared__ float4 red[kSegWaves][128];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // segment j of workgroup b is b + j * gridDim.x: plans are sorted by target id and the hot ids of a Zipf batch are
    // neighbours -- dealt out contiguously, one workgroup would walk all the long segments one after the other
    const int nwg = gridDim.x;
    // ---- phase A: this wave's own segment, if short
    {
        const int u = blockIdx.x + wave * nwg;
        const int k0 = u < U ? seg_ptr[u] : 0, k1 = u < U ? seg_ptr[u + 1] : 0;
        const int len = k1 - k0;
        if (len > 0 && len <= kSegShort) {
            const size_t tgt = (size_t)seg_target[u] * CH;
            for (int ch = lane; ch < CH; ch += 64) {
                float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
                for (int k = k0; k < k1; k += kSegUnr) {
                    float4 v[kSegUnr];
#pragma unroll
                    for (int j = 0; j < kSegUnr; ++j) v[j] = src[(size_t)order[min(k + j, k1 - 1)] * CH + ch];
#pragma unroll
                    for (int j = 0; j < kSegUnr; ++j)
                        if (k + j < k1) s = f4_add(s, v[j]);
                }
                dst[tgt + ch] = f4_add(dst[tgt + ch], s);
            }
        }
    }
    // ---- phase B: the long segments of this workgroup's 16, one after the other, all waves together
    for (int j = 0; j < kSegWaves; ++j) {
        const int u = blockIdx.x + j * nwg;
        if (u >= U) break;
        const int k0 = seg_ptr[u], k1 = seg_ptr[u + 1];                   // workgroup-uniform
        if (k1 - k0 <= kSegShort) continue;
        const size_t tgt = (size_t)seg_target[u] * CH;
        for (int ch = lane; ch < CH; ch += 64) {
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int k = k0 + wave * kSegUnr; k < k1; k += kSegWaves * kSegUnr) {
                float4 v[kSegUnr];
#pragma unroll
                for (int q = 0; q < kSegUnr; ++q) v[q] = src[(size_t)order[min(k + q, k1 - 1)] * CH + ch];
#pragma unroll
                for (int q = 0; q < kSegUnr; ++q)
                    if (k + q < k1) s = f4_add(s, v[q]);
            }
            red[wave][ch] = s;
        }
        __syncthreads();
        if (wave == 0) {
            for (int ch = lane; ch < CH; ch += 64) {
                float4 r = red[0][ch];
#pragma unroll
                for (int w = 1; w < kSegWaves; ++w) r = f4_add(r, red[w][ch]);
                dst[tgt + ch] = f4_add(dst[tgt + ch], r);
            }
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" {

int renet_version(void) { return RENET_ABI_VERSION; }

int renet_gather_rows(const float* table, const int32_t* idx, int n, int D, float* out, void* stream) {
    if (n < 0 || D <= 0 || (D & 3)) return RENET_ERR_BADARG;
    if (n == 0) return RENET_OK;
    const int CH = D / 4;
    const size_t total = (size_t)n * CH;
    int blocks = (int)min((size_t)2048, (total + 255) / 256);
    RENET_LAUNCH(gather_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)table, idx, n, CH, (float4*)out);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}

// Workgroups of a segmented add over U segments: one per segment while that still fills the chip (a plan over 20
// relations is 20 long segments -- 16 of them dealt to ONE workgroup would be walked one after the other), 16
// segments per workgroup beyond that.
static int seg_grid(int U) { return U <= 512 ? U : max(512, (U + kSegWaves - 1) / kSegWaves); }

int renet_segment_add(const float* src, const int32_t* order, const int32_t* seg_ptr,
                      const int32_t* seg_target, int U, int D, float* dst, void* stream) {
    if (U < 0 || D <= 0 || (D & 3)) return RENET_ERR_BADARG;
    if (U == 0) return RENET_OK;
    if (D > 512) return RENET_ERR_UNSUPPORTED;
    RENET_LAUNCH(segment_add_kernel, dim3(seg_grid(U)), dim3(kSegWaves * 64), 0,
                       (hipStream_t)stream, (const float4*)src, (const float4*)src, order, seg_ptr, seg_target, U, D / 4,
                       (float4*)dst, (float4*)dst);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}

int renet_segment_add2(const float* src0, const float* src1, const int32_t* order, const int32_t* seg_ptr,
                       const int32_t* seg_target, int U, int D, float* dst0, float* dst1, void* stream) {
    if (U < 0 || D <= 0 || (D & 3)) return RENET_ERR_BADARG;
    if (U == 0) return RENET_OK;
    if (D > 512) return RENET_ERR_UNSUPPORTED;
    RENET_LAUNCH(segment_add_kernel, dim3(seg_grid(U), 2), dim3(kSegWaves * 64), 0,
                       (hipStream_t)stream, (const float4*)src0, (const float4*)src1, order, seg_ptr, seg_target, U, D / 4,
                       (float4*)dst0, (float4*)dst1);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}

}  // extern "C"
