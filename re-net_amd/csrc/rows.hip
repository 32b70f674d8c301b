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

// ---- several segmented adds in one launch (renet_segment_add_multi) ------------------------------------------------------
// The small scatters of the backward pass are latency chains (pointer -> order -> rows -> read-modify-write of the
// destination), a few microseconds of dependent round trips each whatever their bytes: up to 4 jobs share ONE grid (a
// contiguous range of workgroups per job, the job table in the kernel arguments), and a job may carry a second stage over
// the same plan whose sum is added to the destination row while it is still in registers (short segments) or by the thread
// that wrote it (long ones).  Inside a job the segments are dealt to workgroups and waves as segment_add_kernel deals them,
// and every sum is formed by seg_rows_sum in that kernel's order; `a0 + a1` is one addition per element at load.
struct SegJobK {
    const float4 *a0, *a1, *b;
    const int32_t *order, *seg_ptr, *seg_target;
    float4* dst;
    int U, nwg, blk0, overwrite;
};
struct SegJobsK { SegJobK j[RENET_SEGADD_MAX_JOBS]; int n; };

// sum of the rows order[k], k = kbeg + i * stride + q (q < kSegUnr) below k1, in increasing k: kSegUnr loads in flight
template <bool TWO>
__device__ __forceinline__ float4 seg_rows_sum(const float4* __restrict__ a0, const float4* __restrict__ a1,
                                               const int32_t* __restrict__ order, int CH, int ch, int kbeg, int k1,
                                               int stride) {
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = kbeg; k < k1; k += stride) {
        float4 v[kSegUnr];
        if (TWO) {                                     // two halves: the same 8 loads in flight, 4 rows of each source
#pragma unroll
            for (int h = 0; h < kSegUnr; h += kSegUnr / 2) {
                float4 w[kSegUnr / 2];
#pragma unroll
                for (int q = 0; q < kSegUnr / 2; ++q) {
                    const size_t at = (size_t)order[min(k + h + q, k1 - 1)] * CH + ch;
                    v[h + q] = a0[at];
                    w[q] = a1[at];
                }
#pragma unroll
                for (int q = 0; q < kSegUnr / 2; ++q) v[h + q] = f4_add(v[h + q], w[q]);
            }
        } else {
#pragma unroll
            for (int q = 0; q < kSegUnr; ++q) v[q] = a0[(size_t)order[min(k + q, k1 - 1)] * CH + ch];
        }
#pragma unroll
        for (int q = 0; q < kSegUnr; ++q)
            if (k + q < k1) s = f4_add(s, v[q]);
    }
    return s;
}

__device__ __forceinline__ float4 seg_stage_sum(const float4* a0, const float4* a1, const int32_t* order, int CH, int ch,
                                                int kbeg, int k1, int stride) {
    return a1 ? seg_rows_sum<true>(a0, a1, order, CH, ch, kbeg, k1, stride)
              : seg_rows_sum<false>(a0, nullptr, order, CH, ch, kbeg, k1, stride);
}

// (8 waves per SIMD = two workgroups per CU, as segment_add_kernel has: the registers stay at 64)
__global__ __launch_bounds__(kSegWaves * 64, 8) void segment_add_multi_kernel(const SegJobsK js, int CH) {
    __shared__ float4 red[kSegWaves][128];
    SegJobK J = js.j[0];                                                   // workgroup-uniform selection
#pragma unroll
    for (int i = 1; i < RENET_SEGADD_MAX_JOBS; ++i)
        if (i < js.n && (int)blockIdx.x >= js.j[i].blk0) J = js.j[i];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int bl = blockIdx.x - J.blk0, nwg = J.nwg, U = J.U;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    // ---- this wave's own segment, if short (an empty one is written only where the job overwrites)
    {
        const int u = bl + wave * nwg;
        const int k0 = u < U ? J.seg_ptr[u] : 0, k1 = u < U ? J.seg_ptr[u + 1] : 0;
        const int len = k1 - k0;
        if (u < U && len <= kSegShort && (len > 0 || J.overwrite)) {
            const size_t tgt = (size_t)__builtin_amdgcn_readfirstlane(J.seg_target[u]) * CH;     // (u is wave-uniform)
            for (int ch = lane; ch < CH; ch += 64) {
                const float4 sa = seg_stage_sum(J.a0, J.a1, J.order, CH, ch, k0, k1, kSegUnr);
                float4 d = f4_add(J.overwrite ? zero : J.dst[tgt + ch], sa);
                if (J.b) d = f4_add(d, seg_stage_sum(J.b, nullptr, J.order, CH, ch, k0, k1, kSegUnr));
                J.dst[tgt + ch] = d;
            }
        }
    }
    // ---- the long segments of this workgroup's 16, one after the other, all waves together; stage after stage
    const int stages = J.b ? 2 : 1;
    for (int j = 0; j < kSegWaves; ++j) {
        const int u = bl + j * nwg;
        if (u >= U) break;
        const int k0 = J.seg_ptr[u], k1 = J.seg_ptr[u + 1];                // workgroup-uniform
        if (k1 - k0 <= kSegShort) continue;
        const size_t tgt = (size_t)__builtin_amdgcn_readfirstlane(J.seg_target[u]) * CH;
        for (int st = 0; st < stages; ++st) {
            const float4* s0 = st ? J.b : J.a0;
            const float4* s1 = st ? nullptr : J.a1;
            for (int ch = lane; ch < CH; ch += 64)
                red[wave][ch] = seg_stage_sum(s0, s1, J.order, CH, ch, k0 + wave * kSegUnr, k1, kSegWaves * kSegUnr);
            __syncthreads();
            if (wave == 0) {
                for (int ch = lane; ch < CH; ch += 64) {
                    float4 r = red[0][ch];
#pragma unroll 5                                                           // (LDS reads in three batches: registers)
                    for (int w = 1; w < kSegWaves; ++w) r = f4_add(r, red[w][ch]);
                    const float4 d = (st == 0 && J.overwrite) ? zero : J.dst[tgt + ch];   // (stage B: this thread's own store)
                    J.dst[tgt + ch] = f4_add(d, r);
                }
            }
            __syncthreads();
        }
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

int renet_segment_add_multi(int n, const RenetSegAddJob* jobs, int D, void* stream) {
    if (n < 1 || n > RENET_SEGADD_MAX_JOBS || !jobs || D <= 0 || (D & 3)) return RENET_ERR_BADARG;
    for (int i = 0; i < n; ++i) {
        const RenetSegAddJob& q = jobs[i];
        if (q.U < 0 || !q.dst || !q.a0) return RENET_ERR_BADARG;
        if (q.U > 0 && (!q.order || !q.seg_ptr || !q.seg_target)) return RENET_ERR_BADARG;
        if (q.overwrite && q.U != q.dst_rows) return RENET_ERR_BADARG;   // a row outside the plan would keep its old value
        for (int k = 0; k < i; ++k)
            if (jobs[k].dst == q.dst) return RENET_ERR_BADARG;           // two jobs updating one destination race
    }
    if (D > 512) return RENET_ERR_UNSUPPORTED;
    SegJobsK js{};
    int blocks = 0;
    for (int i = 0; i < n; ++i) {
        const RenetSegAddJob& q = jobs[i];
        if (q.U == 0) continue;
        SegJobK& k = js.j[js.n++];
        k = {(const float4*)q.a0, (const float4*)q.a1, (const float4*)q.b, q.order, q.seg_ptr, q.seg_target, (float4*)q.dst,
             q.U, seg_grid(q.U), blocks, q.overwrite ? 1 : 0};
        blocks += k.nwg;
    }
    if (js.n == 0) return RENET_OK;
    RENET_LAUNCH(segment_add_multi_kernel, dim3(blocks), dim3(kSegWaves * 64), 0, (hipStream_t)stream, js, D / 4);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}

}  // extern "C"
