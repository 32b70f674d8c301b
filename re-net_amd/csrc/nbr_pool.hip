// Neighbour pooling of the mean / attentive history encoders (Aggregator.py:239-361 MeanAggregator, AttnAggregator).
// One SEGMENT is the neighbour list of one time step of one sequence: a ragged gather of entity rows followed by a
// segment mean, or by a segment softmax over a_j = v . tanh(P[nbr_j] + q) and a weighted sum.  Gather-bound work:
//   * one wave per segment; a row is CH = D / 4 float4 chunks, lane l owns chunks l and l + 64 (25 / 50 / 75 / 100 lanes
//     of the first round are busy; D = 300 and 400 take a second chunk per lane), every load is 16 bytes, branch-free
//     (clamped chunk / neighbour index), kNpUnr* neighbours in flight per wave;
//   * attention is an ONLINE softmax: running maximum m, sum l and accumulator, rescaled only when a batch of
//     neighbours moves the maximum; the raw scores are parked in the per-neighbour weight array and normalised once the
//     segment's (m, l) are known -- each lane re-reads only what it wrote itself;
//   * a segment of more than kNpSplit neighbours is split into kNpWaves contiguous ranges, one per wave of the
//     workgroup, and the partial (m, l, acc) triples are merged in LDS in WAVE ORDER: the association order of every sum
//     is a function of the segment length alone, never of scheduling -- no atomics anywhere, results are bit-reproducible;
//   * the result and the E[s] / R[r] column blocks go straight into the packed (time-major) GRU input at out_row.
// Backward: per segment the scores' tanh is recomputed and the per-neighbour contribution rows (towards dE and dP) are
// written with plain 16-byte stores; the caller sums them per destination entity with renet_segment_add2.
#include <math.h>

#include "common.h"

namespace {

constexpr int kNpWaves = 4;        // waves per workgroup = segments per workgroup
constexpr int kNpSplit = 256;      // a longer segment is walked by all waves of its workgroup
constexpr int kNpUnrMean = 8;      // neighbours in flight per wave (row loads: 1 per neighbour in mean mode, 2 in attention)
constexpr int kNpUnrAttn = 4;
constexpr int kNpMaxCh = 128;      // LDS row of the merge (CH <= 100)

struct NpFwdArgs {
    const float4 *E, *R, *P, *q, *v;
    const int32_t *nbr, *seg_ptr, *seg_s, *seg_r, *seg_q, *out_row;
    int S, CH;
    float4* out;
    float* stats;
    float* w;
};

struct NpBwdArgs {
    const float4 *dOut, *out, *E, *P, *q, *v;
    const float* w;
    const int32_t *nbr, *seg_ptr, *seg_q, *out_row;
    int S, CH;
    float4 *cE, *cP, *dq_rows, *dv_rows, *ds_rows, *dr_rows;
};

__device__ __forceinline__ float np_wave_sum(float x) {          // butterfly: every lane ends with the same bits
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
    return x;
}
__device__ __forceinline__ float np_dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
__device__ __forceinline__ float4 np_tanh4(float4 a, float4 b) {
    return make_float4(tanhf(a.x + b.x), tanhf(a.y + b.y), tanhf(a.z + b.z), tanhf(a.w + b.w));
}
__device__ __forceinline__ float4 np_zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// the range of wave `wave` when a segment [k0, k1) is split over the workgroup
__device__ __forceinline__ void np_sub_range(int k0, int k1, int wave, int& b, int& e) {
    const int sub = (k1 - k0 + kNpWaves - 1) / kNpWaves;
    b = min(k0 + wave * sub, k1);
    e = min(b + sub, k1);
}

// ---- forward ------------------------------------------------------------------------------------------------------
// One contiguous range [kb, ke) of a segment's neighbours, by one wave.  Mean: acc += E[nbr_k] in k order.  Attention:
// the online softmax state (m, l, acc) of the range; the raw score of neighbour k is left in w[k] by lane (k - kb) & 63.
template <int NCH, bool ATTN>
__device__ __forceinline__ void np_fwd_range(const NpFwdArgs& a, int kb, int ke, int lane, const int (&ch)[NCH],
                                             const float4 (&qv)[NCH], const float4 (&vv)[NCH], float& m, float& l,
                                             float4 (&acc)[NCH]) {
    constexpr int UNR = ATTN ? kNpUnrAttn : kNpUnrMean;
    for (int k = kb; k < ke; k += UNR) {
        float4 e[UNR][NCH], p[UNR][NCH];
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            const size_t row = (size_t)a.nbr[min(k + j, ke - 1)] * a.CH;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                e[j][c] = a.E[row + ch[c]];
                if (ATTN) p[j][c] = a.P[row + ch[c]];
            }
        }
        if (ATTN) {
            float s[UNR];
            float mb = m;
#pragma unroll
            for (int j = 0; j < UNR; ++j) {
                float d = 0.f;
#pragma unroll
                for (int c = 0; c < NCH; ++c) d += np_dot4(vv[c], np_tanh4(p[j][c], qv[c]));
                d = np_wave_sum(d);
                const bool live = k + j < ke;
                if (live && lane == ((k + j - kb) & 63)) a.w[k + j] = d;
                s[j] = live ? d : -INFINITY;
                mb = fmaxf(mb, s[j]);
            }
            if (mb > m) {                                          // wave-uniform: the maximum moved
                const float r = expf(m - mb);                      // (m = -inf at the start: r = 0 on l = acc = 0)
                l *= r;
#pragma unroll
                for (int c = 0; c < NCH; ++c) acc[c] = f4_scale(acc[c], r);
                m = mb;
            }
#pragma unroll
            for (int j = 0; j < UNR; ++j) {
                const float wj = expf(s[j] - m);                   // 0 for the clamped tail
                l += wj;
#pragma unroll
                for (int c = 0; c < NCH; ++c) acc[c] = f4_add(acc[c], f4_scale(e[j][c], wj));
            }
        } else {
#pragma unroll
            for (int j = 0; j < UNR; ++j)
                if (k + j < ke) {
#pragma unroll
                    for (int c = 0; c < NCH; ++c) acc[c] = f4_add(acc[c], e[j][c]);
                }
        }
    }
}

// raw scores of [kb, ke) -> softmax weights, by the wave that wrote them
__device__ __forceinline__ void np_normalise(float* __restrict__ w, int kb, int ke, int lane, float m, float inv_l) {
    for (int k = kb + lane; k < ke; k += 64) w[k] = expf(w[k] - m) * inv_l;
}

template <int NCH, bool ATTN>
__device__ __forceinline__ void np_fwd_store(const NpFwdArgs& a, int u, int lane, const int (&ch)[NCH],
                                             const float4 (&res)[NCH]) {
    constexpr int PARTS = ATTN ? 3 : 2;
    const size_t row = (size_t)a.out_row[u] * PARTS * a.CH;
    const size_t es = (size_t)a.seg_s[u] * a.CH;
    const size_t rr = ATTN ? (size_t)a.seg_r[u] * a.CH : 0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        if (lane + 64 * c < a.CH) {
            a.out[row + ch[c]] = res[c];
            a.out[row + a.CH + ch[c]] = a.E[es + ch[c]];
            if (ATTN) a.out[row + 2 * a.CH + ch[c]] = a.R[rr + ch[c]];
        }
    }
}

template <int NCH, bool ATTN>
__global__ __launch_bounds__(kNpWaves * 64) void nbr_pool_fwd_kernel(NpFwdArgs a) {
    __shared__ float4 s_acc[kNpWaves][kNpMaxCh];
    __shared__ float s_m[kNpWaves], s_l[kNpWaves];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int ch[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) ch[c] = min(lane + 64 * c, a.CH - 1);
    float4 qv[NCH], vv[NCH];

    // ---- phase A: this wave's own segment, if it is short
    {
        const int u = blockIdx.x * kNpWaves + wave;
        const int k0 = u < a.S ? a.seg_ptr[u] : 0, k1 = u < a.S ? a.seg_ptr[u + 1] : 0;
        const int len = k1 - k0;
        if (len > 0 && len <= kNpSplit) {
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const bool on = lane + 64 * c < a.CH;
                qv[c] = ATTN ? a.q[(size_t)a.seg_q[u] * a.CH + ch[c]] : np_zero4();
                vv[c] = (ATTN && on) ? a.v[ch[c]] : np_zero4();     // idle lanes add 0 to every score
            }
            float m = -INFINITY, l = 0.f;
            float4 acc[NCH];
#pragma unroll
            for (int c = 0; c < NCH; ++c) acc[c] = np_zero4();
            np_fwd_range<NCH, ATTN>(a, k0, k1, lane, ch, qv, vv, m, l, acc);
            if (ATTN) {
                const float inv = 1.f / l;
#pragma unroll
                for (int c = 0; c < NCH; ++c) acc[c] = f4_scale(acc[c], inv);
                np_normalise(a.w, k0, k1, lane, m, inv);
                if (lane == 0) {
                    a.stats[2 * (size_t)u] = m;
                    a.stats[2 * (size_t)u + 1] = logf(l);
                }
            } else {
                const float n = (float)len;
#pragma unroll
                for (int c = 0; c < NCH; ++c)
                    acc[c] = make_float4(acc[c].x / n, acc[c].y / n, acc[c].z / n, acc[c].w / n);
            }
            np_fwd_store<NCH, ATTN>(a, u, lane, ch, acc);
        }
    }
    // ---- phase B: the long segments of this workgroup, one after the other, all waves together
    for (int j = 0; j < kNpWaves; ++j) {
        const int u = blockIdx.x * kNpWaves + j;
        if (u >= a.S) break;
        const int k0 = a.seg_ptr[u], k1 = a.seg_ptr[u + 1];                 // workgroup-uniform
        if (k1 - k0 <= kNpSplit) continue;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const bool on = lane + 64 * c < a.CH;
            qv[c] = ATTN ? a.q[(size_t)a.seg_q[u] * a.CH + ch[c]] : np_zero4();
            vv[c] = (ATTN && on) ? a.v[ch[c]] : np_zero4();
        }
        int kb, ke;
        np_sub_range(k0, k1, wave, kb, ke);
        float m = -INFINITY, l = 0.f;
        float4 acc[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) acc[c] = np_zero4();
        np_fwd_range<NCH, ATTN>(a, kb, ke, lane, ch, qv, vv, m, l, acc);
#pragma unroll
        for (int c = 0; c < NCH; ++c)
            if (lane + 64 * c < a.CH) s_acc[wave][lane + 64 * c] = acc[c];
        if (lane == 0) {
            s_m[wave] = m;
            s_l[wave] = l;
        }
        __syncthreads();
        // every wave forms the segment's (M, L) the same way, in wave order
        float M = s_m[0];
#pragma unroll
        for (int w = 1; w < kNpWaves; ++w) M = fmaxf(M, s_m[w]);
        float L = 0.f;
        float f[kNpWaves];
#pragma unroll
        for (int w = 0; w < kNpWaves; ++w) {
            f[w] = ATTN ? expf(s_m[w] - M) : 1.f;
            L += s_l[w] * f[w];
        }
        if (ATTN) np_normalise(a.w, kb, ke, lane, M, 1.f / L);
        if (wave == 0) {
            float4 res[NCH];
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                float4 r = np_zero4();
                if (lane + 64 * c < a.CH) {
#pragma unroll
                    for (int w = 0; w < kNpWaves; ++w) r = f4_add(r, f4_scale(s_acc[w][lane + 64 * c], f[w]));
                }
                if (ATTN) {
                    res[c] = f4_scale(r, 1.f / L);
                } else {
                    const float n = (float)(k1 - k0);
                    res[c] = make_float4(r.x / n, r.y / n, r.z / n, r.w / n);
                }
            }
            if (ATTN && lane == 0) {
                a.stats[2 * (size_t)u] = M;
                a.stats[2 * (size_t)u + 1] = logf(L);
            }
            np_fwd_store<NCH, ATTN>(a, u, lane, ch, res);
        }
        __syncthreads();
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------
// One contiguous range of a segment: writes the contribution rows cE[k] (and cP[k]) and accumulates the range's part of
// the segment's dq / dv rows.  g: the gradient of the pooled block of this segment's packed row (idle lanes hold 0).
template <int NCH, bool ATTN>
__device__ __forceinline__ void np_bwd_range(const NpBwdArgs& a, int kb, int ke, int lane, const int (&ch)[NCH],
                                             const float4 (&g)[NCH], const float4 (&qv)[NCH], const float4 (&vv)[NCH],
                                             float c0, float inv_n, float4 (&dq)[NCH], float4 (&dv)[NCH]) {
    constexpr int UNR = ATTN ? kNpUnrAttn : kNpUnrMean;
    if (!ATTN) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            if (lane + 64 * c < a.CH) {
                const float4 r = f4_scale(g[c], inv_n);
                for (int k = kb; k < ke; ++k) a.cE[(size_t)k * a.CH + ch[c]] = r;
            }
        }
        return;
    }
    for (int k = kb; k < ke; k += UNR) {
        float4 e[UNR][NCH], p[UNR][NCH];
        float wj[UNR];
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            const int kk = min(k + j, ke - 1);
            const size_t row = (size_t)a.nbr[kk] * a.CH;
            wj[j] = a.w[kk];
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                e[j][c] = a.E[row + ch[c]];
                p[j][c] = a.P[row + ch[c]];
            }
        }
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            float d = 0.f;
#pragma unroll
            for (int c = 0; c < NCH; ++c) d += np_dot4(g[c], e[j][c]);
            d = np_wave_sum(d);
            if (k + j < ke) {                                      // wave-uniform
                const float da = wj[j] * (d - c0);
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    const float4 t = np_tanh4(p[j][c], qv[c]);
                    const float4 one_t2 = make_float4(1.f - t.x * t.x, 1.f - t.y * t.y, 1.f - t.z * t.z, 1.f - t.w * t.w);
                    const float4 up = f4_scale(f4_mul(vv[c], one_t2), da);
                    dq[c] = f4_add(dq[c], up);
                    dv[c] = f4_add(dv[c], f4_scale(t, da));
                    if (lane + 64 * c < a.CH) {
                        a.cP[(size_t)(k + j) * a.CH + ch[c]] = up;
                        a.cE[(size_t)(k + j) * a.CH + ch[c]] = f4_scale(g[c], wj[j]);
                    }
                }
            }
        }
    }
}

template <int NCH, bool ATTN>
__device__ __forceinline__ void np_bwd_load(const NpBwdArgs& a, int u, int lane, const int (&ch)[NCH], float4 (&g)[NCH],
                                            float4 (&qv)[NCH], float4 (&vv)[NCH], float& c0, bool copy_blocks) {
    constexpr int PARTS = ATTN ? 3 : 2;
    const size_t row = (size_t)a.out_row[u] * PARTS * a.CH;
    float d = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const bool on = lane + 64 * c < a.CH;
        g[c] = on ? a.dOut[row + ch[c]] : np_zero4();
        qv[c] = ATTN ? a.q[(size_t)a.seg_q[u] * a.CH + ch[c]] : np_zero4();
        vv[c] = (ATTN && on) ? a.v[ch[c]] : np_zero4();
        if (ATTN) d += np_dot4(g[c], a.out[row + ch[c]]);
        if (copy_blocks && on) {                                    // the E[s] / R[r] column blocks of this packed row
            a.ds_rows[(size_t)u * a.CH + ch[c]] = a.dOut[row + a.CH + ch[c]];
            if (ATTN) a.dr_rows[(size_t)u * a.CH + ch[c]] = a.dOut[row + 2 * a.CH + ch[c]];
        }
    }
    c0 = ATTN ? np_wave_sum(d) : 0.f;
}

template <int NCH, bool ATTN>
__global__ __launch_bounds__(kNpWaves * 64) void nbr_pool_bwd_kernel(NpBwdArgs a) {
    __shared__ float4 s_dq[kNpWaves][kNpMaxCh], s_dv[kNpWaves][kNpMaxCh];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int ch[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) ch[c] = min(lane + 64 * c, a.CH - 1);
    float4 g[NCH], qv[NCH], vv[NCH], dq[NCH], dv[NCH];
    float c0;
    {
        const int u = blockIdx.x * kNpWaves + wave;
        const int k0 = u < a.S ? a.seg_ptr[u] : 0, k1 = u < a.S ? a.seg_ptr[u + 1] : 0;
        const int len = k1 - k0;
        if (len > 0 && len <= kNpSplit) {
            np_bwd_load<NCH, ATTN>(a, u, lane, ch, g, qv, vv, c0, true);
#pragma unroll
            for (int c = 0; c < NCH; ++c) dq[c] = dv[c] = np_zero4();
            np_bwd_range<NCH, ATTN>(a, k0, k1, lane, ch, g, qv, vv, c0, 1.f / (float)len, dq, dv);
            if (ATTN) {
#pragma unroll
                for (int c = 0; c < NCH; ++c)
                    if (lane + 64 * c < a.CH) {
                        a.dq_rows[(size_t)u * a.CH + ch[c]] = dq[c];
                        a.dv_rows[(size_t)u * a.CH + ch[c]] = dv[c];
                    }
            }
        }
    }
    for (int j = 0; j < kNpWaves; ++j) {
        const int u = blockIdx.x * kNpWaves + j;
        if (u >= a.S) break;
        const int k0 = a.seg_ptr[u], k1 = a.seg_ptr[u + 1];                 // workgroup-uniform
        if (k1 - k0 <= kNpSplit) continue;
        np_bwd_load<NCH, ATTN>(a, u, lane, ch, g, qv, vv, c0, wave == 0);
        int kb, ke;
        np_sub_range(k0, k1, wave, kb, ke);
#pragma unroll
        for (int c = 0; c < NCH; ++c) dq[c] = dv[c] = np_zero4();
        np_bwd_range<NCH, ATTN>(a, kb, ke, lane, ch, g, qv, vv, c0, 1.f / (float)(k1 - k0), dq, dv);
        if (!ATTN) continue;                                                // kernel-uniform: nothing to merge
#pragma unroll
        for (int c = 0; c < NCH; ++c)
            if (lane + 64 * c < a.CH) {
                s_dq[wave][lane + 64 * c] = dq[c];
                s_dv[wave][lane + 64 * c] = dv[c];
            }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int c = 0; c < NCH; ++c)
                if (lane + 64 * c < a.CH) {
                    float4 rq = s_dq[0][lane + 64 * c], rv = s_dv[0][lane + 64 * c];
#pragma unroll
                    for (int w = 1; w < kNpWaves; ++w) {
                        rq = f4_add(rq, s_dq[w][lane + 64 * c]);
                        rv = f4_add(rv, s_dv[w][lane + 64 * c]);
                    }
                    a.dq_rows[(size_t)u * a.CH + ch[c]] = rq;
                    a.dv_rows[(size_t)u * a.CH + ch[c]] = rv;
                }
        }
        __syncthreads();
    }
}

bool np_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// seg_ptr as the host knows it: S + 1 non-decreasing offsets from 0 -- and no empty segment (the softmax of nothing)
int np_check_segments(const int32_t* seg_ptr_host, int S) {
    if (!seg_ptr_host || seg_ptr_host[0] != 0) return RENET_ERR_BADARG;
    for (int u = 0; u < S; ++u)
        if (seg_ptr_host[u + 1] <= seg_ptr_host[u]) return RENET_ERR_BADARG;
    return RENET_OK;
}

}  // namespace

extern "C" {

int renet_nbr_pool_fwd(const float* E, const float* R, const float* P, const float* q, const float* v,
                       const int32_t* nbr, const int32_t* seg_ptr, const int32_t* seg_ptr_host, const int32_t* seg_s,
                       const int32_t* seg_r, const int32_t* seg_q, const int32_t* out_row, int S, int D, int attn,
                       float* out, float* stats, float* w, void* stream) {
    if (!renet_dim_ok(D)) return RENET_ERR_UNSUPPORTED;
    if (S < 0) return RENET_ERR_BADARG;
    if (S == 0) return RENET_OK;
    if (!E || !nbr || !seg_ptr || !seg_s || !out_row || !out) return RENET_ERR_BADARG;
    if (attn && (!R || !P || !q || !v || !seg_r || !seg_q || !stats || !w)) return RENET_ERR_BADARG;
    if (!np_aligned(E) || !np_aligned(R) || !np_aligned(P) || !np_aligned(q) || !np_aligned(v) || !np_aligned(out))
        return RENET_ERR_BADARG;
    const int rc = np_check_segments(seg_ptr_host, S);
    if (rc != RENET_OK) return rc;
    NpFwdArgs a;
    a.E = (const float4*)E, a.R = (const float4*)R, a.P = (const float4*)P, a.q = (const float4*)q, a.v = (const float4*)v;
    a.nbr = nbr, a.seg_ptr = seg_ptr, a.seg_s = seg_s, a.seg_r = seg_r, a.seg_q = seg_q, a.out_row = out_row;
    a.S = S, a.CH = D / 4, a.out = (float4*)out, a.stats = stats, a.w = w;
    const dim3 grid((S + kNpWaves - 1) / kNpWaves), block(kNpWaves * 64);
    hipStream_t st = (hipStream_t)stream;
    if (attn) {
        if (a.CH > 64) RENET_LAUNCH((nbr_pool_fwd_kernel<2, true>), grid, block, 0, st, a);
        else RENET_LAUNCH((nbr_pool_fwd_kernel<1, true>), grid, block, 0, st, a);
    } else {
        if (a.CH > 64) RENET_LAUNCH((nbr_pool_fwd_kernel<2, false>), grid, block, 0, st, a);
        else RENET_LAUNCH((nbr_pool_fwd_kernel<1, false>), grid, block, 0, st, a);
    }
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}

int renet_nbr_pool_bwd(const float* dOut, const float* out, const float* E, const float* P, const float* q,
                       const float* v, const float* w, const int32_t* nbr, const int32_t* seg_ptr,
                       const int32_t* seg_ptr_host, const int32_t* seg_q, const int32_t* out_row, int S, int D, int attn,
                       float* cE, float* cP, float* dq_rows, float* dv_rows, float* ds_rows, float* dr_rows,
                       void* stream) {
    if (!renet_dim_ok(D)) return RENET_ERR_UNSUPPORTED;
    if (S < 0) return RENET_ERR_BADARG;
    if (S == 0) return RENET_OK;
    if (!dOut || !nbr || !seg_ptr || !out_row || !cE || !ds_rows) return RENET_ERR_BADARG;
    if (attn && (!out || !E || !P || !q || !v || !w || !seg_q || !cP || !dq_rows || !dv_rows || !dr_rows))
        return RENET_ERR_BADARG;
    if (!np_aligned(dOut) || !np_aligned(out) || !np_aligned(E) || !np_aligned(P) || !np_aligned(q) || !np_aligned(v) ||
        !np_aligned(cE) || !np_aligned(cP) || !np_aligned(dq_rows) || !np_aligned(dv_rows) || !np_aligned(ds_rows) ||
        !np_aligned(dr_rows))
        return RENET_ERR_BADARG;
    const int rc = np_check_segments(seg_ptr_host, S);
    if (rc != RENET_OK) return rc;
    NpBwdArgs a;
    a.dOut = (const float4*)dOut, a.out = (const float4*)out, a.E = (const float4*)E, a.P = (const float4*)P;
    a.q = (const float4*)q, a.v = (const float4*)v, a.w = w;
    a.nbr = nbr, a.seg_ptr = seg_ptr, a.seg_q = seg_q, a.out_row = out_row;
    a.S = S, a.CH = D / 4;
    a.cE = (float4*)cE, a.cP = (float4*)cP, a.dq_rows = (float4*)dq_rows, a.dv_rows = (float4*)dv_rows;
    a.ds_rows = (float4*)ds_rows, a.dr_rows = (float4*)dr_rows;
    const dim3 grid((S + kNpWaves - 1) / kNpWaves), block(kNpWaves * 64);
    hipStream_t st = (hipStream_t)stream;
    if (attn) {
        if (a.CH > 64) RENET_LAUNCH((nbr_pool_bwd_kernel<2, true>), grid, block, 0, st, a);
        else RENET_LAUNCH((nbr_pool_bwd_kernel<1, true>), grid, block, 0, st, a);
    } else {
        if (a.CH > 64) RENET_LAUNCH((nbr_pool_bwd_kernel<2, false>), grid, block, 0, st, a);
        else RENET_LAUNCH((nbr_pool_bwd_kernel<1, false>), grid, block, 0, st, a);
    }
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}

}  // extern "C"
