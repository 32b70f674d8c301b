// Joint (relation, entity) ranks of an event under observed history, for gfx950 (not in the reference).
// The model factorises an event as p(o | s, r, history) * p(r | s, history).  For one history ("group") the entity head
// gives a block scores[R, C] -- row r the logits of the query whose relation is r -- and the relation head one row
// logits_r[R].  The joint log-probability of the pair (r, c) is
//     J[r, c] = scores[r, c] + off[r],     off[r] = fp32( logsoftmax64(logits_r)[r] - logsumexp64(scores[r, :]) )
// as ONE fp32 addition (__fadd_rn: never contracted, never moved to the other side of a comparison), so that a host
// restatement on the same off array compares the same fp32 values.  The joint itself is never stored.
//   renet_joint_row_offsets : one read of every row of the [G * R, C] block -> off [G * R].  The logsumexp is rank.hip's:
//                             online per thread (running maximum, rescaled only when it moves), carried in fp64, merged in
//                             wave order; the relation row's log-softmax (R <= 1024: at most four elements per thread) goes
//                             through the same reduction.  One rounding to fp32 at the end.
//   renet_joint_rank_rows   : one workgroup per (query, relation) row sweeps row group[q] * R + r once and counts J > v and
//                             J == v against the gold value v = J[gold_r[q], gold_c[q]], which every workgroup reads from the
//                             gold row's two floats.  The filtered settings are CORRECTIONS of the swept counts by the row's
//                             own lists ((cols, start, count) ranges of the resident tables, the form of renet_rank_rows3): a
//                             listed column is NO candidate (the renet_topk_rows convention, not the sigmoid-and-zero one of
//                             the entity filter) and loses its contribution; the gold pair always stays.  While walking a
//                             list the workgroup notes whether gold_c[q] is on it, and it writes J[row, gold_c[q]]: the
//                             relation ranks given both endpoints are read from those R values per query.
// One workgroup of 256 threads per row as in rank.hip: 16-byte loads from the first 16-byte aligned element of the row,
// scalar head and tail, any C and any row alignment; the counters never leave the workgroup (wave shuffles + LDS, no global
// atomics) and scores is never written.  The per-row counts are summed over the R rows of a query by the caller.
#include "common.h"
#include <float.h>
#include <math.h>

namespace {

constexpr int JR_THREADS = 256;
constexpr int JR_WAVES = JR_THREADS / 64;
constexpr int JR_MAX_R = 1024;

__device__ __forceinline__ double jr_exp(float a, float b) { return exp((double)a - (double)b); }      // exp(a - b)

// running (maximum m, sum s of exp(x - m)) of one thread (rank.hip: rk_lse1 / rk_take4's logsumexp part)
__device__ __forceinline__ void jr_lse1(float x, float& m, double& s) {
    if (x > m) {
        s *= jr_exp(m, x);
        m = x;
    }
    s += jr_exp(x, m);
}

__device__ __forceinline__ void jr_lse4(const float4 v, float& m, double& s) {
    const float cm = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
    if (cm > m) {
        s *= jr_exp(m, cm);
        m = cm;
    }
    s += (jr_exp(v.x, m) + jr_exp(v.y, m)) + (jr_exp(v.z, m) + jr_exp(v.w, m));
}

__device__ __forceinline__ int jr_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the threads' (m, s) pairs -> the wave's, every lane holding it
__device__ __forceinline__ void jr_wave_lse(float& m, double& s) {
    float wm = m;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wm = fmaxf(wm, __shfl_xor(wm, o));
    double sd = s * jr_exp(m, wm);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sd += __shfl_xor(sd, o);
    m = wm;
    s = sd;
}

// log(sum) + maximum of the waves' pairs, in wave order
__device__ __forceinline__ double jr_merge(const float* s_m, const double* s_s) {
    float M = s_m[0];
#pragma unroll
    for (int w = 1; w < JR_WAVES; ++w) M = fmaxf(M, s_m[w]);
    double S = 0.0;
#pragma unroll
    for (int w = 0; w < JR_WAVES; ++w) S += s_s[w] * jr_exp(s_m[w], M);
    return log(S) + (double)M;
}

__global__ __launch_bounds__(JR_THREADS) void joint_row_offsets_kernel(const float* __restrict__ scores, int ld, int R, int C,
                                                                       const float* __restrict__ logits_r, int ld_r,
                                                                       float* __restrict__ off_out) {
    __shared__ float s_m[2][JR_WAVES];
    __shared__ double s_s[2][JR_WAVES];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const float* x = scores + (size_t)row * ld;
    const float* lr = logits_r + (size_t)(row / R) * ld_r;

    float m = -FLT_MAX;
    double s = 0.0;
    // [0, head) scalar up to the first 16-byte aligned element, [head, head + 4 * nvec) as float4, the rest scalar
    const int head = min(C, (int)((4 - (((uintptr_t)x >> 2) & 3)) & 3));
    const int nvec = (C - head) >> 2;
    const float4* xv = reinterpret_cast<const float4*>(x + head);
    int i = tid;
    for (; i + 3 * JR_THREADS < nvec; i += 4 * JR_THREADS) {
        float4 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = xv[i + q * JR_THREADS];
#pragma unroll
        for (int q = 0; q < 4; ++q) jr_lse4(v[q], m, s);
    }
    for (; i < nvec; i += JR_THREADS) jr_lse4(xv[i], m, s);
    const int ntail = C - head - 4 * nvec;                       // < 4; head < 4
    if (tid < head + ntail) jr_lse1(x[tid < head ? tid : 4 * nvec + tid], m, s);

    float mr = -FLT_MAX;                                         // the relation row: R <= 1024, at most four per thread
    double sr = 0.0;
    for (int k = tid; k < R; k += JR_THREADS) jr_lse1(lr[k], mr, sr);

    jr_wave_lse(m, s);
    jr_wave_lse(mr, sr);
    if (lane == 0) {
        s_m[0][wave] = m;
        s_s[0][wave] = s;
        s_m[1][wave] = mr;
        s_s[1][wave] = sr;
    }
    __syncthreads();
    if (tid == 0) {
        const double lse_b = jr_merge(s_m[0], s_s[0]), lse_r = jr_merge(s_m[1], s_s[1]);
        off_out[row] = (float)(((double)lr[row % R] - lse_r) - lse_b);
    }
}

__device__ __forceinline__ void jr_count(float x, float o, float v, int& gt, int& eq) {
    const float j = __fadd_rn(x, o);
    gt += j > v ? 1 : 0;
    eq += j == v ? 1 : 0;
}

// this thread's share of one filter list, cols[start, start + count) cut to the table [0, len): a listed column other than
// the gold pair (gold_col < 0: this is not the gold row) is no candidate and loses its contribution
__device__ __forceinline__ void jr_correct(const float* __restrict__ x, int C, float o, float v, int gold_col, int gc,
                                           const int32_t* __restrict__ cols, int len, int start, int count, int tid,
                                           int& gt, int& eq, int& seen) {
    const int end = (int)min((long long)start + (long long)max(count, 0), (long long)len);
    for (int k = max(start, 0) + tid; k < end; k += JR_THREADS) {
        const int c = cols[k];
        if (c < 0 || c >= C) continue;                           // (columns outside the row are ignored, never read)
        seen |= c == gc ? 1 : 0;
        if (c == gold_col) continue;
        int g1 = 0, e1 = 0;
        jr_count(x[c], o, v, g1, e1);
        gt -= g1;
        eq -= e1;
    }
}

__global__ __launch_bounds__(JR_THREADS) void joint_rank_rows_kernel(
    const float* __restrict__ scores, int ld, int G, int C, int R, const float* __restrict__ off, int Q,
    const int32_t* __restrict__ group, const int32_t* __restrict__ gold_r, const int32_t* __restrict__ gold_c,
    const int32_t* __restrict__ cols_a, const int32_t* __restrict__ start_a, const int32_t* __restrict__ count_a, int len_a,
    const int32_t* __restrict__ cols_t, const int32_t* __restrict__ start_t, const int32_t* __restrict__ count_t, int len_t,
    int32_t* __restrict__ counts, float* __restrict__ at_gold, int32_t* __restrict__ listed) {
    __shared__ int s_cnt[8][JR_WAVES];
    const int out = blockIdx.x, tid = threadIdx.x;               // out = q * R + r
    const int lane = tid & 63, wave = tid >> 6;
    const int q = out / R, r = out - q * R;
    const size_t n = (size_t)Q * R;
    // the indices live on the device (no host check): clamped, never dereferenced as given
    const int g = min(max(group[q], 0), G - 1);
    const int gr = min(max(gold_r[q], 0), R - 1);
    const int gc = min(max(gold_c[q], 0), C - 1);
    const size_t grow = (size_t)g * R + gr, row = (size_t)g * R + r;
    const float v = __fadd_rn(scores[grow * ld + gc], off[grow]);
    const float o = off[row];
    const float* x = scores + row * ld;

    int c[8] = {0, 0, 0, 0, 0, 0, 0, 0};         // raw greater, equal; filtered; time_filtered; gold_c on list a, on list t
    const int head = min(C, (int)((4 - (((uintptr_t)x >> 2) & 3)) & 3));
    const int nvec = (C - head) >> 2;
    const float4* xv = reinterpret_cast<const float4*>(x + head);
    int i = tid;
    for (; i + 3 * JR_THREADS < nvec; i += 4 * JR_THREADS) {
        float4 w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = xv[i + k * JR_THREADS];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            jr_count(w[k].x, o, v, c[0], c[1]);
            jr_count(w[k].y, o, v, c[0], c[1]);
            jr_count(w[k].z, o, v, c[0], c[1]);
            jr_count(w[k].w, o, v, c[0], c[1]);
        }
    }
    for (; i < nvec; i += JR_THREADS) {
        const float4 w = xv[i];
        jr_count(w.x, o, v, c[0], c[1]);
        jr_count(w.y, o, v, c[0], c[1]);
        jr_count(w.z, o, v, c[0], c[1]);
        jr_count(w.w, o, v, c[0], c[1]);
    }
    const int ntail = C - head - 4 * nvec;
    if (tid < head + ntail) jr_count(x[tid < head ? tid : 4 * nvec + tid], o, v, c[0], c[1]);

    // two corrections of the SAME swept counts, each by its own list
    c[2] = c[4] = c[0];
    c[3] = c[5] = c[1];
    const int gold_col = r == gr ? gc : -1;
    if (cols_a) jr_correct(x, C, o, v, gold_col, gc, cols_a, len_a, start_a[out], count_a[out], tid, c[2], c[3], c[6]);
    if (cols_t) jr_correct(x, C, o, v, gold_col, gc, cols_t, len_t, start_t[out], count_t[out], tid, c[4], c[5], c[7]);

#pragma unroll
    for (int k = 0; k < 8; ++k) c[k] = jr_wave_sum(c[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) s_cnt[k][wave] = c[k];
    }
    __syncthreads();
    if (tid < 8) {
        int T = 0;
#pragma unroll
        for (int w = 0; w < JR_WAVES; ++w) T += s_cnt[tid][w];
        if (tid < 6) counts[(size_t)tid * n + out] = T;
        else listed[(size_t)(tid - 6) * n + out] = T != 0 ? 1 : 0;      // (a column is listed at most once per row)
    }
    if (tid == 8) at_gold[out] = __fadd_rn(x[gc], o);
}

}  // namespace

int renet_joint_row_offsets(const float* scores, int ld, int G, int R, int C, const float* logits_r, int ld_r,
                            float* off_out, void* stream) {
    if (G < 0 || R < 1 || R > JR_MAX_R || C < 1 || ld < C || ld_r < R) return RENET_ERR_BADARG;
    if ((long long)G * R > 0x7fffffffLL) return RENET_ERR_BADARG;
    if (G == 0) return RENET_OK;
    if (!scores || !logits_r || !off_out) return RENET_ERR_BADARG;
    const dim3 grid(G * R), blk(JR_THREADS);
    RENET_LAUNCH(joint_row_offsets_kernel, grid, blk, 0, (hipStream_t)stream, scores, ld, R, C, logits_r, ld_r, off_out);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}

int renet_joint_rank_rows(const float* scores, int ld, int G, int C, int R, const float* off, int Q, const int32_t* group,
                          const int32_t* gold_r, const int32_t* gold_c, const int32_t* cols_a, const int32_t* start_a,
                          const int32_t* count_a, int len_a, const int32_t* cols_t, const int32_t* start_t,
                          const int32_t* count_t, int len_t, int32_t* counts, float* at_gold, int32_t* listed,
                          void* stream) {
    if (Q < 0 || G < 1 || R < 1 || C < 1 || ld < C) return RENET_ERR_BADARG;
    if ((long long)Q * R > 0x7fffffffLL || (long long)G * R > 0x7fffffffLL) return RENET_ERR_BADARG;
    if (Q == 0) return RENET_OK;
    if (!scores || !off || !group || !gold_r || !gold_c || !counts || !at_gold || !listed) return RENET_ERR_BADARG;
    // a list is (cols, start, count) with the length of its table, or nothing at all
    if ((start_a || count_a || cols_a) && (!start_a || !count_a || !cols_a || len_a < 0)) return RENET_ERR_BADARG;
    if ((start_t || count_t || cols_t) && (!start_t || !count_t || !cols_t || len_t < 0)) return RENET_ERR_BADARG;
    const dim3 grid(Q * R), blk(JR_THREADS);
    RENET_LAUNCH(joint_rank_rows_kernel, grid, blk, 0, (hipStream_t)stream, scores, ld, G, C, R, off, Q, group, gold_r, gold_c,
                 cols_a, start_a, count_a, len_a, cols_t, start_t, count_t, len_t, counts, at_gold, listed);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}
