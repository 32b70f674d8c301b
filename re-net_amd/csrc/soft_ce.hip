// Softmax cross-entropy against SPARSE SOFT targets (the global model's loss, global_model.py:52-55 / utils.py
// soft_cross_entropy, with the target distribution of a row given as its non-zero columns): one workgroup per row, the
// streamed three-pass form of softmax_ce_kernel (csrc/seq.hip).
#include "common.h"

namespace {

__device__ __forceinline__ float sce_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float sce_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Weight of column c in the row's target list col[beg, end) (ascending, distinct): 0 when it is not a target.
__device__ __forceinline__ float sce_weight_of(const int32_t* __restrict__ col, const float* __restrict__ w, int beg,
                                               int end, int c) {
    int lo = beg, hi = end;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (col[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return (lo < end && col[lo] == c) ? w[lo] : 0.f;
}

// `dlogits` may ALIAS `logits` (neither pointer is __restrict__, see softmax_ce_kernel).  The only reads of the row that
// are not a thread's own columns are the target logits: they are read FIRST, summed, and pinned in front of the first
// barrier -- three barriers before any thread stores to the row.  Every sum runs in a fixed order (a thread's strided
// terms, the xor butterfly, four partials from LDS): the result is a function of the inputs alone, and nothing is atomic.
__global__ __launch_bounds__(256) void soft_ce_sparse_kernel(const float* logits, int C, int ld,
                                                             const int32_t* __restrict__ tgt_ptr,
                                                             const int32_t* __restrict__ tgt_col,
                                                             const float* __restrict__ tgt_w, float grad_scale,
                                                             float* __restrict__ row_loss, float* dlogits) {
    __shared__ float red[4], red_w[4], red_wx[4];
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* x = logits + (size_t)b * ld;
    const int beg = tgt_ptr[b], end = tgt_ptr[b + 1];
    if (end <= beg) {                                   // (block-uniform) an empty row: loss 0, gradient 0
        if (threadIdx.x == 0) row_loss[b] = 0.f;
        if (dlogits) {
            float* dx = dlogits + (size_t)b * ld;
            for (int c = threadIdx.x; c < C; c += 256) dx[c] = 0.f;
        }
        return;
    }
    float W = 0.f, wx = 0.f;
    for (int k = beg + (int)threadIdx.x; k < end; k += 256) {
        const int c = tgt_col[k];
        const float w = tgt_w[k];
        if ((unsigned)c < (unsigned)C) {                // (a column outside the row is not read)
            W += w;
            if (w != 0.f) wx += w * x[c];               // (weight 0 on a -inf logit contributes 0)
        }
    }
    W = sce_wave_sum(W);
    wx = sce_wave_sum(wx);
    if (lane == 0) {
        red_w[wave] = W;
        red_wx[wave] = wx;
    }
    __syncthreads();
    W = (red_w[0] + red_w[1]) + (red_w[2] + red_w[3]);
    wx = (red_wx[0] + red_wx[1]) + (red_wx[2] + red_wx[3]);
    asm volatile("" : "+v"(W), "+v"(wx) :: "memory");  // the target logits are consumed HERE, before any store below
    float m = -INFINITY;
    for (int c = threadIdx.x; c < C; c += 256) m = fmaxf(m, x[c]);
    m = sce_wave_max(m);
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float s = 0.f;
    for (int c = threadIdx.x; c < C; c += 256) s += expf(x[c] - m);
    s = sce_wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    s = (red[0] + red[1]) + (red[2] + red[3]);
    if (threadIdx.x == 0) row_loss[b] = W * (logf(s) + m) - wx;
    if (dlogits) {
        float* dx = dlogits + (size_t)b * ld;
        const float inv = 1.f / s;
        for (int c = threadIdx.x; c < C; c += 256) {    // a thread reads its own column before it writes it
            const float p = expf(x[c] - m) * inv;
            const float wc = sce_weight_of(tgt_col, tgt_w, beg, end, c);
            dx[c] = (W * p - wc) * grad_scale;
        }
    }
}

}  // namespace

int renet_soft_ce_sparse(const float* logits, int B, int C, int ld, const int32_t* tgt_ptr, const int32_t* tgt_col,
                         const float* tgt_w, float grad_scale, float* row_loss, float* dlogits, void* stream) {
    if (B < 0 || C <= 0 || ld < C) return RENET_ERR_BADARG;
    if (B == 0) return RENET_OK;
    if (!logits || !tgt_ptr || !row_loss) return RENET_ERR_BADARG;
    RENET_LAUNCH(soft_ce_sparse_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, logits, C, ld, tgt_ptr, tgt_col, tgt_w,
                 grad_scale, row_loss, dlogits);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}
