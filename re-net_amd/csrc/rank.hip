// Evaluation metric kernel for gfx950 (reference model.py:365-381 raw ranks, 391-418 filtered ranks, 358-361 loss).
// The reference ranks the gold entity of a test quadruple in a score row with a sigmoid copy, an index write of zeros over
// the other known-true completions and two compare-and-sum passes, and reads the same row once more for the cross-entropy.
//   renet_rank_rows : ONE read of every row of scores[n, C] gives
//                       greater[i] = #columns whose value is  > the gold column's
//                       equal[i]   = #columns whose value is == the gold column's (the gold column itself included)
//                       row_loss[i] = logsumexp(scores[i, :]) - scores[i, label[i]]
//                     The filtered setting compares sigmoid(score), computed as torch.sigmoid computes it (1 / (1 + exp(-x))
//                     in fp32, IEEE division): fp32 sigmoid maps many logits onto one value, saturates to 1 and underflows
//                     to 0, and the reference's averaged ties count exactly those collapses, so the comparison cannot move
//                     to logit space.  The filter lists (CSR, every column at most once per row) are applied as a
//                     CORRECTION after the sweep: a listed column other than the label loses its own contribution and
//                     contributes the value 0 instead (equal when the gold value is 0, never greater).  scores is not
//                     written.
//   renet_rank_rows3: the same ONE read of every row gives the counts of THREE settings at once (int32 counts[6, n]):
//                       raw            the scores against the gold score                      (model.py:365-381)
//                       filtered       sigmoid(score), the time-agnostic list zeroed          (model.py:391-418)
//                       time_filtered  sigmoid(score), the list of the query's own timestamp zeroed
//                     and the loss.  The sweep counts every element against the gold score and its sigmoid against the
//                     gold sigmoid; the two filtered settings are two independent corrections of the same swept sigmoid
//                     counts, each by its own list, addressed IN PLACE in a resident table (cols, start[row], count[row]:
//                     filter_index.FilterIndex.ranges -- no gathered copy of the lists).  The sweep is rank_rows_kernel's,
//                     statement for statement (rk_take4<false, LOSS> + four sigmoid counts), so the loss is summed in the
//                     same order; rank_rows_kernel itself is untouched.
// One workgroup of 256 threads per row: a row is 40-92 KB (10 k - 23 k entities), n is a few thousand, so the grid covers
// the chip several times over and a row's counters never leave the workgroup (wave shuffles + LDS, no global atomics).
// 16-byte loads from the first 16-byte aligned element of the row, scalar head and tail.  The logsumexp is online per
// thread (running maximum, rescaled only when the maximum moves: one exp per element) and is carried in fp64 -- exp of the
// exact difference, fp64 sums, one rounding to fp32 at the end: an online sum rescales partial sums that are close to
// the largest term, and in fp32 that cost up to a few tenths of an ulp of the loss on rows with few dominant columns
// (renet_softmax_ce subtracts the row maximum first and has no such step).  With it the loss is the correctly rounded
// value; the counts, which are what a row without a loss costs, stay fp32.
#include "common.h"
#include <float.h>
#include <math.h>

namespace {

constexpr int RK_THREADS = 256;
constexpr int RK_WAVES = RK_THREADS / 64;

// torch.sigmoid's fp32 formula, operation for operation
__device__ __forceinline__ float rk_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

template <bool SIG>
__device__ __forceinline__ void rk_count(float x, float ground, int& gt, int& eq) {
    const float v = SIG ? rk_sigmoid(x) : x;
    gt += v > ground ? 1 : 0;
    eq += v == ground ? 1 : 0;
}

__device__ __forceinline__ double rk_exp(float a, float b) { return exp((double)a - (double)b); }      // exp(a - b)

// running (maximum m, sum s of exp(x - m)) of one thread
__device__ __forceinline__ void rk_lse1(float x, float& m, double& s) {
    if (x > m) {
        s *= rk_exp(m, x);
        m = x;
    }
    s += rk_exp(x, m);
}

template <bool SIG, bool LOSS>
__device__ __forceinline__ void rk_take4(const float4 v, float ground, float& m, double& s, int& gt, int& eq) {
    if (LOSS) {
        const float cm = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
        if (cm > m) {
            s *= rk_exp(m, cm);
            m = cm;
        }
        s += (rk_exp(v.x, m) + rk_exp(v.y, m)) + (rk_exp(v.z, m) + rk_exp(v.w, m));
    }
    rk_count<SIG>(v.x, ground, gt, eq);
    rk_count<SIG>(v.y, ground, gt, eq);
    rk_count<SIG>(v.z, ground, gt, eq);
    rk_count<SIG>(v.w, ground, gt, eq);
}

__device__ __forceinline__ int rk_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <bool SIG, bool LOSS>
__global__ __launch_bounds__(RK_THREADS) void rank_rows_kernel(const float* __restrict__ scores, int ld, int C,
                                                               const int32_t* __restrict__ label,
                                                               const int32_t* __restrict__ filt_ptr,
                                                               const int32_t* __restrict__ filt_col,
                                                               int32_t* __restrict__ greater, int32_t* __restrict__ equal,
                                                               float* __restrict__ row_loss) {
    __shared__ int s_gt[RK_WAVES], s_eq[RK_WAVES];
    __shared__ float s_m[RK_WAVES];
    __shared__ double s_s[RK_WAVES];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const float* x = scores + (size_t)row * ld;
    // a label outside [0, C) is clamped, never dereferenced as given (the labels live on the device: no host check)
    const int lab = min(max(label[row], 0), C - 1);
    const float xl = x[lab];
    const float ground = SIG ? rk_sigmoid(xl) : xl;

    float m = -FLT_MAX;
    double s = 0.0;
    int gt = 0, eq = 0;
    // [0, head) scalar up to the first 16-byte aligned element, [head, head + 4 * nvec) as float4, the rest scalar
    const int head = min(C, (int)((4 - (((uintptr_t)x >> 2) & 3)) & 3));
    const int nvec = (C - head) >> 2;
    const float4* xv = reinterpret_cast<const float4*>(x + head);
    int i = tid;
    for (; i + 3 * RK_THREADS < nvec; i += 4 * RK_THREADS) {
        float4 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = xv[i + q * RK_THREADS];
#pragma unroll
        for (int q = 0; q < 4; ++q) rk_take4<SIG, LOSS>(v[q], ground, m, s, gt, eq);
    }
    for (; i < nvec; i += RK_THREADS) rk_take4<SIG, LOSS>(xv[i], ground, m, s, gt, eq);
    const int ntail = C - head - 4 * nvec;                       // < 4; head < 4
    if (tid < head + ntail) {
        const float v = x[tid < head ? tid : 4 * nvec + tid];     // tid >= head: column head + 4 * nvec + (tid - head)
        if (LOSS) rk_lse1(v, m, s);
        rk_count<SIG>(v, ground, gt, eq);
    }

    if (SIG && filt_ptr) {
        const int zero_eq = ground == 0.f ? 1 : 0;
        const int end = filt_ptr[row + 1];
        for (int k = filt_ptr[row] + tid; k < end; k += RK_THREADS) {
            const int c = filt_col[k];
            if (c == lab || c < 0 || c >= C) continue;           // (columns outside the row are ignored, never read)
            int g1 = 0, e1 = 0;
            rk_count<true>(x[c], ground, g1, e1);
            gt -= g1;
            eq += zero_eq - e1;
        }
    }

    gt = rk_wave_sum(gt);
    eq = rk_wave_sum(eq);
    double sd = 0.0;
    if (LOSS) {
        float wm = m;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) wm = fmaxf(wm, __shfl_xor(wm, o));
        sd = s * rk_exp(m, wm);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sd += __shfl_xor(sd, o);
        m = wm;
    }
    if (lane == 0) {
        s_gt[wave] = gt;
        s_eq[wave] = eq;
        s_m[wave] = m;
        s_s[wave] = sd;
    }
    __syncthreads();
    if (tid == 0) {
        int G = 0, E = 0;
#pragma unroll
        for (int w = 0; w < RK_WAVES; ++w) {
            G += s_gt[w];
            E += s_eq[w];
        }
        greater[row] = G;
        equal[row] = E;
        if (LOSS) {
            float M = s_m[0];
#pragma unroll
            for (int w = 1; w < RK_WAVES; ++w) M = fmaxf(M, s_m[w]);
            double S = 0.0;
#pragma unroll
            for (int w = 0; w < RK_WAVES; ++w) S += s_s[w] * rk_exp(s_m[w], M);
            row_loss[row] = (float)(log(S) + (double)M - (double)xl);
        }
    }
}

// this thread's share of one filter list, cols[start, start + count) cut to the table [0, len): rank_rows_kernel's rule
__device__ __forceinline__ void rk_correct(const float* __restrict__ x, int C, int lab, float ground,
                                           const int32_t* __restrict__ cols, int len, int start, int count, int tid,
                                           int& gt, int& eq) {
    const int zero_eq = ground == 0.f ? 1 : 0;
    const int end = (int)min((long long)start + (long long)max(count, 0), (long long)len);
    for (int k = max(start, 0) + tid; k < end; k += RK_THREADS) {
        const int c = cols[k];
        if (c == lab || c < 0 || c >= C) continue;               // (columns outside the row are ignored, never read)
        int g1 = 0, e1 = 0;
        rk_count<true>(x[c], ground, g1, e1);
        gt -= g1;
        eq += zero_eq - e1;
    }
}

// raw counts through rk_take4<false, LOSS> (with the logsumexp, exactly as rank_rows_kernel<false, LOSS> takes an element),
// sigmoid counts beside them
template <bool LOSS>
__device__ __forceinline__ void rk_take4_both(const float4 v, float xl, float gs, float& m, double& s, int* c) {
    rk_take4<false, LOSS>(v, xl, m, s, c[0], c[1]);
    rk_count<true>(v.x, gs, c[2], c[3]);
    rk_count<true>(v.y, gs, c[2], c[3]);
    rk_count<true>(v.z, gs, c[2], c[3]);
    rk_count<true>(v.w, gs, c[2], c[3]);
}

template <bool LOSS>
__global__ __launch_bounds__(RK_THREADS) void rank_rows3_kernel(const float* __restrict__ scores, int ld, int n, int C,
                                                                const int32_t* __restrict__ label,
                                                                const int32_t* __restrict__ cols_a,
                                                                const int32_t* __restrict__ start_a,
                                                                const int32_t* __restrict__ count_a, int len_a,
                                                                const int32_t* __restrict__ cols_t,
                                                                const int32_t* __restrict__ start_t,
                                                                const int32_t* __restrict__ count_t, int len_t,
                                                                int32_t* __restrict__ counts, float* __restrict__ row_loss) {
    __shared__ int s_cnt[6][RK_WAVES];
    __shared__ float s_m[RK_WAVES];
    __shared__ double s_s[RK_WAVES];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const float* x = scores + (size_t)row * ld;
    const int lab = min(max(label[row], 0), C - 1);              // clamped as in rank_rows_kernel
    const float xl = x[lab];
    const float gs = rk_sigmoid(xl);

    float m = -FLT_MAX;
    double s = 0.0;
    int c[6] = {0, 0, 0, 0, 0, 0};               // raw greater, equal; sigmoid greater, equal; the time-aware pair (below)
    const int head = min(C, (int)((4 - (((uintptr_t)x >> 2) & 3)) & 3));
    const int nvec = (C - head) >> 2;
    const float4* xv = reinterpret_cast<const float4*>(x + head);
    int i = tid;
    for (; i + 3 * RK_THREADS < nvec; i += 4 * RK_THREADS) {
        float4 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = xv[i + q * RK_THREADS];
#pragma unroll
        for (int q = 0; q < 4; ++q) rk_take4_both<LOSS>(v[q], xl, gs, m, s, c);
    }
    for (; i < nvec; i += RK_THREADS) rk_take4_both<LOSS>(xv[i], xl, gs, m, s, c);
    const int ntail = C - head - 4 * nvec;
    if (tid < head + ntail) {
        const float v = x[tid < head ? tid : 4 * nvec + tid];
        if (LOSS) rk_lse1(v, m, s);
        rk_count<false>(v, xl, c[0], c[1]);
        rk_count<true>(v, gs, c[2], c[3]);
    }

    // two corrections of the SAME swept sigmoid counts: the time-aware setting starts from this thread's swept share, then
    // each list is applied to its own pair
    c[4] = c[2];
    c[5] = c[3];
    if (cols_a) rk_correct(x, C, lab, gs, cols_a, len_a, start_a[row], count_a[row], tid, c[2], c[3]);
    if (cols_t) rk_correct(x, C, lab, gs, cols_t, len_t, start_t[row], count_t[row], tid, c[4], c[5]);

#pragma unroll
    for (int k = 0; k < 6; ++k) c[k] = rk_wave_sum(c[k]);
    double sd = 0.0;
    if (LOSS) {
        float wm = m;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) wm = fmaxf(wm, __shfl_xor(wm, o));
        sd = s * rk_exp(m, wm);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sd += __shfl_xor(sd, o);
        m = wm;
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) s_cnt[k][wave] = c[k];
        s_m[wave] = m;
        s_s[wave] = sd;
    }
    __syncthreads();
    if (tid < 6) {
        int T = 0;
#pragma unroll
        for (int w = 0; w < RK_WAVES; ++w) T += s_cnt[tid][w];
        counts[(size_t)tid * n + row] = T;
    }
    if (LOSS && tid == 0) {
        float M = s_m[0];
#pragma unroll
        for (int w = 1; w < RK_WAVES; ++w) M = fmaxf(M, s_m[w]);
        double S = 0.0;
#pragma unroll
        for (int w = 0; w < RK_WAVES; ++w) S += s_s[w] * rk_exp(s_m[w], M);
        row_loss[row] = (float)(log(S) + (double)M - (double)xl);
    }
}

}  // namespace

int renet_rank_rows(const float* scores, int ld, int n, int C, const int32_t* label, const int32_t* filt_ptr,
                    const int32_t* filt_col, int filtered, int32_t* greater, int32_t* equal, float* row_loss,
                    void* stream) {
    if (n < 0 || C < 1 || ld < C) return RENET_ERR_BADARG;
    if (n == 0) return RENET_OK;
    if (!scores || !label || !greater || !equal) return RENET_ERR_BADARG;
    if (filt_ptr && (!filtered || !filt_col)) return RENET_ERR_BADARG;       // lists belong to the filtered setting
    const dim3 grid(n), blk(RK_THREADS);
    hipStream_t st = (hipStream_t)stream;
#define RK_GO(SIG, LOSS)                                                                                                 \
    RENET_LAUNCH((rank_rows_kernel<SIG, LOSS>), grid, blk, 0, st, scores, ld, C, label, filt_ptr, filt_col, greater, equal, \
                 row_loss)
    if (filtered) {
        if (row_loss) RK_GO(true, true);
        else RK_GO(true, false);
    } else {
        if (row_loss) RK_GO(false, true);
        else RK_GO(false, false);
    }
#undef RK_GO
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}

int renet_rank_rows3(const float* scores, int ld, int n, int C, const int32_t* label, const int32_t* cols_a,
                     const int32_t* start_a, const int32_t* count_a, int len_a, const int32_t* cols_t,
                     const int32_t* start_t, const int32_t* count_t, int len_t, int32_t* counts, float* row_loss,
                     void* stream) {
    if (n < 0 || C < 1 || ld < C) return RENET_ERR_BADARG;
    if (n == 0) return RENET_OK;
    if (!scores || !label || !counts) return RENET_ERR_BADARG;
    // a list is (cols, start, count) with the length of its table, or nothing at all
    if ((start_a || count_a || cols_a) && (!start_a || !count_a || !cols_a || len_a < 0)) return RENET_ERR_BADARG;
    if ((start_t || count_t || cols_t) && (!start_t || !count_t || !cols_t || len_t < 0)) return RENET_ERR_BADARG;
    const dim3 grid(n), blk(RK_THREADS);
    hipStream_t st = (hipStream_t)stream;
#define RK_GO3(LOSS)                                                                                                    \
    RENET_LAUNCH((rank_rows3_kernel<LOSS>), grid, blk, 0, st, scores, ld, n, C, label, cols_a, start_a, count_a, len_a,    \
                 cols_t, start_t, count_t, len_t, counts, row_loss)
    if (row_loss) RK_GO3(true);
    else RK_GO3(false);
#undef RK_GO3
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}
