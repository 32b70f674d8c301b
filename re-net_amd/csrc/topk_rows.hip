// Ranked, filtered top-k of every row of a score matrix for gfx950 (extension of the reference API: what RENet.predict_topk_batch
// serves -- "the k most probable objects of (s, r, ?, t) that are not already known").  In torch this is a clone, a scatter of
// -inf over the known completions, a log_softmax, torch.topk and a gather: five or six passes over an [n, num_ent] matrix of
// a few hundred MB, with an unspecified order among ties.
//   renet_topk_rows : ONE read of every row of scores[n, C] gives the k best candidates of the row -- all columns minus the
//                     row's filter list (addressed in place in a resident table, as renet_rank_rows3 takes it), a listed
//                     column equal to keep[row] staying in -- ordered by score descending, then column ascending, with
//                     their log-probabilities under the softmax of the WHOLE row (the filter removes candidates, not mass).
// One workgroup of 1024 threads per row, as in rank.hip (the grid covers the chip many times over, nothing of a row leaves
// its workgroup, no global atomics), but here the row is STAGED IN LDS, because a selection needs it several times:
//   1. sweep  16-byte loads from the first 16-byte aligned element, scalar head and tail (rank.hip's sweep).  Every element
//             becomes an order-preserving 32-bit key (unsigned comparison of keys == float comparison of the values, -0.0
//             as +0.0, a NaN below -inf), stored with one 16-byte LDS store per group -- the row sits in LDS shifted by
//             0..3 slots so that the aligned groups of the global row are aligned groups in LDS --, counted into the
//             histogram of the first radix digit, and summed into the online fp64 logsumexp of rank.hip (when asked for).
//   2. filter every listed column's key is exchanged for the code 0, below every real key (a -inf score keeps its own key
//             0x007fffff: an ordinary candidate that sorts last), and taken out of the histogram.  An exchange, so a column
//             listed twice is still removed once.
//   3. select radix select of the k-th largest key, digits of 11 + 11 + 10 bits: the first histogram is the sweep's, the two
//             others are 16-byte LDS reads of the staged row.  Integer LDS atomics: the counts are deterministic.  A row
//             with at most k candidates skips the selection (threshold 0: every candidate is taken), and the selection
//             stops at the first digit after which the threshold bin and everything above it fit the sort (1024 entries):
//             one digit for k = 10 of 23 k normal scores, two for k = 1000; all three only under heavy ties.
//   4. gather every thread owns a CONTIGUOUS chunk of columns (an odd number of them: a conflict-free stride); one block scan
//             of the (above, at the threshold) counts places the keys above the threshold and the FIRST columns among
//             those at it, which is what makes ties at the k-th value come out lowest column first.
//   5. sort   the at most 1024 survivors as (key, ~column) in 64 bits, bitonic, one entry per thread (shuffles inside a wave,
//             LDS across waves): no two entries are equal, so the order -- and with it the whole result -- is the same from
//             run to run.  The first k leave.
// The values written are decoded from the keys: the scores bit for bit, except that -0.0 comes back as +0.0 (they tie, and
// share a key), so the row is not touched a second time (re-reading the k selected columns was measured 4 % slower
// at k = 1000).  logp = (float)((double)score - lse): one rounding, as rank.hip's loss.
// Why this shape: the row (92 KB at 23 k entities) is touched once in HBM and steps 2-5 read LDS only (the CU's 160 KiB:
// C <= 32768, renet_joint_softmax's bound), at 128-256 B/clk.  All LDS is carved from the dynamic region at multiples of
// 16 bytes and sized by C, so two workgroups share a CU below ~16 k columns; above that a CU holds ONE row at a time and
// the phases of a row -- HBM wait, fp64 exps, the barrier-separated chain of steps 3-5 -- overlap with nothing, which is
// where the time goes (profiles/topk_rows.md: several times one HBM read of the matrix, several times faster than the
// torch passes).  16 waves per workgroup keep the 16-byte loads of the sweep in flight.  No MFMA: integer and exp work.
//   renet_topk_rows_wide : the same contract for rows that do not fit LDS (C <= RENET_TOPK_ROWS_WIDE_MAX_C), in two launches:
//     slices  a (slice, row) grid runs steps 1-5 above -- the same kernel, instantiated with SLICE -- on the columns
//             [slice * S, slice * S + S) of its row: the piece's own 16-byte alignment, the row's whole list with the columns
//             outside the piece passed over (so a column is exchanged by the one piece that holds it, once), and leaves in
//             the workspace its min(k, candidates) best as sorted (key, ~column) entries, its candidate count and its fp64
//             (max, sum) pair.  S <= 32768, so the 16 + 16 bit packing of the gather holds per piece.
//     merge   one workgroup per row folds the slices in slice order into a running sorted top-k held one entry per thread:
//             max(running[i], slice[P - 1 - i]) is a bitonic sequence of the P best of both, and one bitonic merge sorts it
//             (log2 P exchanges, shuffles inside a wave).  Exact: the row's top-k is contained in the union of the per-slice
//             top-k, entries are distinct, and per-slice ties already come out lowest column first.  The candidate count
//             is the sum over slices, the logsumexp the fixed-order fp64 combination of the pairs.
//   S defaults to an even split of the row into pieces of at most 15360 columns (78 KB of LDS: two workgroups share a CU,
//   so the phases of one piece overlap with another's); the caller may set it (tests make the pieces small).
#include "common.h"
#include <float.h>
#include <math.h>

namespace {

constexpr int TR_THREADS = 1024;
constexpr int TR_WAVES = TR_THREADS / 64;
constexpr int TR_MAX_C = 32768;          // keys of one row: 128 KB of LDS; the (above, at) counts are packed in 16 + 16 bits
constexpr int TR_MAX_K = 1024;           // one survivor per thread in the sort and the write
constexpr int TR_BINS = 2048;            // 11-bit digits (the last one 10)
constexpr int TRW_MAX_C = RENET_TOPK_ROWS_WIDE_MAX_C;
constexpr int TRW_MIN_STAGE = 64;        // a caller's piece: [64, TR_MAX_C] columns
constexpr int TRW_STAGE = 15360;         // the default piece is at most this wide: tr_lds_bytes = 78 KB, two workgroups per CU
constexpr int TRW_ROWS = 32768;          // rows of one launch of the (slice, row) grid

// what a slice leaves beside its entries
struct TrSlice {
    double m, s;                         // sum over the piece of exp(x - m), m its maximum (only with LOGP)
    long long ncand;                     // its columns that are candidates
};

// Order-preserving key: never 0 for a real value (0 is the code of a filtered column)
__device__ __forceinline__ unsigned tr_key(float v) {
    const unsigned u = __float_as_uint(v);
    if (v != v) return 1u;                                   // NaN: below -inf (0x007fffff), above the filtered code
    if (v == 0.f) return 0x80000000u;                        // -0.0 ties with +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the score of a key (of a real value other than -0.0 and NaN: bit for bit)
__device__ __forceinline__ float tr_value(unsigned key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

// rank.hip's online logsumexp (rk_exp, rk_lse1, the float4 step of rk_take4), carried in fp64
__device__ __forceinline__ double tr_exp(float a, float b) { return exp((double)a - (double)b); }      // exp(a - b)

__device__ __forceinline__ void tr_lse1(float x, float& m, double& s) {
    if (x > m) {
        s *= tr_exp(m, x);
        m = x;
    }
    s += tr_exp(x, m);
}

__device__ __forceinline__ void tr_lse4(const float4 v, float& m, double& s) {
    const float cm = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
    if (cm > m) {
        s *= tr_exp(m, cm);
        m = cm;
    }
    s += (tr_exp(v.x, m) + tr_exp(v.y, m)) + (tr_exp(v.z, m) + tr_exp(v.w, m));
}

// one aligned group of the row: keys to LDS (one 16-byte store), first-digit histogram, logsumexp
template <bool LOGP>
__device__ __forceinline__ void tr_take4(const float4 v, uint4* dst, unsigned* hist, float& m, double& s) {
    const uint4 q = make_uint4(tr_key(v.x), tr_key(v.y), tr_key(v.z), tr_key(v.w));
    *dst = q;
    atomicAdd(&hist[q.x >> 21], 1u);
    atomicAdd(&hist[q.y >> 21], 1u);
    atomicAdd(&hist[q.z >> 21], 1u);
    atomicAdd(&hist[q.w >> 21], 1u);
    if (LOGP) tr_lse4(v, m, s);
}

// inclusive scan of v over the workgroup in thread order (s_w: TR_WAVES ints)
__device__ __forceinline__ int tr_block_scan(int v, int* s_w, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    __syncthreads();                                         // (s_w may still be read by the scan before this one)
    if (lane == 63) s_w[wave] = v;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += s_w[w];
    return v + base;
}

// One digit of the selection.  Thread t owns the bins TR_BINS - 1 - 2t and the one below it (the scan runs from the top
// bin down), reads and CLEARS them, and the thread whose bins hold the need-th largest key publishes s_sel[0] = that bin,
// s_sel[1] = the number of keys in the bins above it, s_sel[3] = the number in it; s_sel[2] = the number of keys counted.
// Ends with a barrier.
__device__ __forceinline__ void tr_pick(unsigned* hist, int need, int* s_w, int* s_sel, int tid) {
    const int b1 = TR_BINS - 1 - 2 * tid;
    const int c1 = (int)hist[b1], c0 = (int)hist[b1 - 1];
    hist[b1] = 0u;
    hist[b1 - 1] = 0u;
    const int incl = tr_block_scan(c1 + c0, s_w, tid);
    const int excl = incl - (c1 + c0);
    if (excl < need && need <= incl) {
        const bool upper = excl + c1 >= need;
        s_sel[0] = upper ? b1 : b1 - 1;
        s_sel[1] = upper ? excl : excl + c1;
        s_sel[3] = upper ? c1 : c0;
    }
    if (tid == TR_THREADS - 1) s_sel[2] = incl;
    __syncthreads();
}

// One compare-exchange of a bitonic network over one entry per thread: partners less than a wave apart trade through
// shuffles, the others through sbuf; `larger`: this end of the pair keeps the larger entry.
__device__ __forceinline__ unsigned long long tr_exchange(unsigned long long ent, int stride, bool larger,
                                                          unsigned long long* sbuf, int tid) {
    unsigned long long other;
    if (stride < 64) {
        other = __shfl_xor(ent, stride);
    } else {
        __syncthreads();
        sbuf[tid] = ent;
        __syncthreads();
        other = sbuf[tid ^ stride];
    }
    return (larger == (ent > other)) ? ent : other;
}

// thread tid < k writes place tid of the row's result from its sorted entry
template <bool LOGP>
__device__ __forceinline__ void tr_write(int row, int k, int tid, int nvalid, unsigned long long ent, double lse,
                                         int32_t* __restrict__ out_idx, float* __restrict__ out_val,
                                         float* __restrict__ out_logp, int32_t* __restrict__ out_n) {
    if (tid < k) {                                                       // k <= TR_THREADS
        const size_t o = (size_t)row * k + tid;
        if (tid < nvalid) {
            const float v = tr_value((unsigned)(ent >> 32));
            out_idx[o] = (int)(0xFFFFFFFFu - (unsigned)ent);
            out_val[o] = v;
            if (LOGP) out_logp[o] = v == -INFINITY ? -INFINITY : (float)((double)v - lse);
        } else {
            out_idx[o] = -1;
            out_val[o] = -INFINITY;
            if (LOGP) out_logp[o] = -INFINITY;
        }
    }
    if (tid == 0) out_n[row] = nvalid;
}

// SLICE = false: renet_topk_rows, one workgroup per row (grid.x), the results written.  SLICE = true: workgroup
// (blockIdx.x, row0 + blockIdx.y) takes the columns [blockIdx.x * stage, + stage) of its row and leaves its sorted entries
// (at most ws_per) and its TrSlice in the workspace; the out_* arrays are not used.
template <bool LOGP, bool SLICE>
__global__ __launch_bounds__(TR_THREADS) void topk_rows_kernel(const float* __restrict__ scores, int ld, int C_row, int k,
                                                               const int32_t* __restrict__ cols,
                                                               const int32_t* __restrict__ start,
                                                               const int32_t* __restrict__ count, int len,
                                                               const int32_t* __restrict__ keep,
                                                               int32_t* __restrict__ out_idx, float* __restrict__ out_val,
                                                               float* __restrict__ out_logp, int32_t* __restrict__ out_n,
                                                               int stage, int row0, unsigned long long* __restrict__ ws_ent,
                                                               int ws_per, TrSlice* __restrict__ ws_stat) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tr_smem[];
    const int c0 = SLICE ? (int)blockIdx.x * stage : 0;                  // the first column of this workgroup's piece
    const int C = SLICE ? min(stage, C_row - c0) : C_row;                // and its width
    const int nalloc = (C + 7) & ~3;                         // the row shifted by at most 3, rounded up to whole groups
    unsigned* keys = reinterpret_cast<unsigned*>(tr_smem);
    unsigned* hist = keys + nalloc;
    unsigned long long* sbuf = reinterpret_cast<unsigned long long*>(hist + TR_BINS);
    double* s_s = reinterpret_cast<double*>(sbuf + TR_MAX_K);            // [TR_WAVES] partial sums, [TR_WAVES] the row's lse
    float* s_m = reinterpret_cast<float*>(s_s + TR_WAVES + 2);
    int* s_w = reinterpret_cast<int*>(s_m + TR_WAVES);
    int* s_sel = s_w + TR_WAVES;

    const int row = SLICE ? row0 + (int)blockIdx.y : (int)blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const float* x = scores + (size_t)row * ld + c0;
    // [0, head) scalar up to the first 16-byte aligned element, [head, head + 4 * nvec) as float4, the rest scalar; column c
    // lives at keys[off + c], so that column head is the start of a group
    const int head = min(C, (int)((4 - (((uintptr_t)x >> 2) & 3)) & 3));
    const int off = (4 - head) & 3;
    const int nvec = (C - head) >> 2;

    // the row's filter list [l_beg, l_end) of cols and this thread's first entry of it: asked for now, used after the sweep
    int kept = -1, l_beg = 0, l_end = 0, l_first = -1;
    if (cols) {
        if (keep) kept = keep[row];
        const int st = start[row];
        l_end = (int)min((long long)st + (long long)max(count[row], 0), (long long)len);
        l_beg = min(max(st, 0), max(l_end, 0));
        if (l_beg + tid < l_end) l_first = cols[l_beg + tid];
    }

    for (int i = tid; i < TR_BINS; i += TR_THREADS) hist[i] = 0u;
    if (tid < off) keys[tid] = 0u;                                       // the slots around the row hold the filtered code
    if (off + C + tid < nalloc) keys[off + C + tid] = 0u;                // (nalloc - off - C < 8)
    __syncthreads();

    // ---- 1. sweep
    float m = -FLT_MAX;
    double s = 0.0;
    const float4* xv = reinterpret_cast<const float4*>(x + head);
    uint4* kv = reinterpret_cast<uint4*>(keys + off + head);
    int i = tid;
    for (; i + 3 * TR_THREADS < nvec; i += 4 * TR_THREADS) {
        float4 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = xv[i + q * TR_THREADS];
#pragma unroll
        for (int q = 0; q < 4; ++q) tr_take4<LOGP>(v[q], kv + i + q * TR_THREADS, hist, m, s);
    }
    for (; i < nvec; i += TR_THREADS) tr_take4<LOGP>(xv[i], kv + i, hist, m, s);
    const int ntail = C - head - 4 * nvec;                               // < 4; head < 4
    if (tid < head + ntail) {
        const int c = tid < head ? tid : 4 * nvec + tid;                 // tid >= head: column head + 4 * nvec + (tid - head)
        const float v = x[c];
        const unsigned key = tr_key(v);
        keys[off + c] = key;
        atomicAdd(&hist[key >> 21], 1u);
        if (LOGP) tr_lse1(v, m, s);
    }
    if (LOGP) {
        float wm = m;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) wm = fmaxf(wm, __shfl_xor(wm, o));
        double sd = s * tr_exp(m, wm);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sd += __shfl_xor(sd, o);
        if (lane == 0) {
            s_m[wave] = wm;
            s_s[wave] = sd;
        }
    }
    __syncthreads();

    // ---- 2. filter (and the logsumexp of the row: wave 0, one lane per wave's partial sum)
    if (LOGP && wave == 0) {
        const float mw = lane < TR_WAVES ? s_m[lane] : -FLT_MAX;
        float M = mw;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) M = fmaxf(M, __shfl_xor(M, o));
        double S = lane < TR_WAVES ? s_s[lane] * tr_exp(mw, M) : 0.0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) S += __shfl_xor(S, o);
        if (lane == 0) {
            if (SLICE) {                                                 // the piece's pair: the merge forms the row's
                TrSlice* st = ws_stat + (size_t)row * gridDim.x + blockIdx.x;
                st->m = (double)M;
                st->s = S;
            } else {
                s_s[TR_WAVES] = log(S) + (double)M;
            }
        }
    }
    for (int j = l_beg + tid, c = l_first; j < l_end;) {
        if (c != kept && c >= c0 && c < c0 + C) {                        // (columns outside the row, or the piece, are passed over)
            const unsigned old = atomicExch(&keys[off + c - c0], 0u);
            if (old) atomicSub(&hist[old >> 21], 1u);
        }
        j += TR_THREADS;
        if (j < l_end) c = cols[j];
    }
    __syncthreads();

    // ---- 3. select: every key above thr and the first n_eq of those equal to it go on to the sort, n_take in all.  As soon
    // as the threshold bin and the bins above it hold no more than the sort takes, the selection stops there (thr = the
    // bottom of that bin, less one) and leaves the rest to the sort; only a row with more ties than that around its k-th value
    // goes through all three digits, to the k-th key itself.
    tr_pick(hist, k, s_w, s_sel, tid);                                   // (nobody publishes a bin when k > candidates)
    const int ncand = s_sel[2];
    const int nvalid = min(k, ncand);
    unsigned thr = 0u;                                                   // at most k candidates: all of them
    int n_eq = 0, n_take = nvalid;
    if (ncand > k) {                                                     // the same in every thread: barriers inside
        const uint4* k4 = reinterpret_cast<const uint4*>(keys);
        const int ngrp = nalloc >> 2;
        unsigned prefix = (unsigned)s_sel[0];
        int above = s_sel[1];
        if (above + s_sel[3] <= TR_MAX_K) {
            thr = max(prefix << 21, 1u) - 1u;
            n_take = above + s_sel[3];
        } else {
            for (int g = tid; g < ngrp; g += TR_THREADS) {
                const uint4 q = k4[g];
                if (q.x && (q.x >> 21) == prefix) atomicAdd(&hist[(q.x >> 10) & 0x7FFu], 1u);
                if (q.y && (q.y >> 21) == prefix) atomicAdd(&hist[(q.y >> 10) & 0x7FFu], 1u);
                if (q.z && (q.z >> 21) == prefix) atomicAdd(&hist[(q.z >> 10) & 0x7FFu], 1u);
                if (q.w && (q.w >> 21) == prefix) atomicAdd(&hist[(q.w >> 10) & 0x7FFu], 1u);
            }
            __syncthreads();
            tr_pick(hist, k - above, s_w, s_sel, tid);
            prefix = (prefix << 11) | (unsigned)s_sel[0];
            above += s_sel[1];
            if (above + s_sel[3] <= TR_MAX_K) {
                thr = max(prefix << 10, 1u) - 1u;
                n_take = above + s_sel[3];
            } else {
                for (int g = tid; g < ngrp; g += TR_THREADS) {
                    const uint4 q = k4[g];
                    if (q.x && (q.x >> 10) == prefix) atomicAdd(&hist[q.x & 0x3FFu], 1u);
                    if (q.y && (q.y >> 10) == prefix) atomicAdd(&hist[q.y & 0x3FFu], 1u);
                    if (q.z && (q.z >> 10) == prefix) atomicAdd(&hist[q.z & 0x3FFu], 1u);
                    if (q.w && (q.w >> 10) == prefix) atomicAdd(&hist[q.w & 0x3FFu], 1u);
                }
                __syncthreads();
                tr_pick(hist, k - above, s_w, s_sel, tid);
                thr = (prefix << 10) | (unsigned)s_sel[0];
                above += s_sel[1];
                n_eq = k - above;
                n_take = k;
            }
        }
    }
    const int n_gt = n_take - n_eq;

    // ---- 4. gather in column order
    const int per = ((C + TR_THREADS - 1) / TR_THREADS) | 1;
    const int c_lo = min(C, tid * per), c_hi = min(C, c_lo + per);
    int packed = 0;                                                      // (above << 16) | at: above <= 1024, at <= 32768
    for (int c = c_lo; c < c_hi; ++c) {
        const unsigned key = keys[off + c];
        packed += key > thr ? 0x10000 : key == thr ? 1 : 0;
    }
    const int before = tr_block_scan(packed, s_w, tid) - packed;
    int g_pos = before >> 16, e_pos = before & 0xFFFF;
    for (int c = c_lo; c < c_hi; ++c) {
        const unsigned key = keys[off + c];
        const unsigned long long ent = ((unsigned long long)key << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)c);
        if (key > thr) sbuf[g_pos++] = ent;
        else if (key == thr) {
            if (e_pos < n_eq) sbuf[n_gt + e_pos] = ent;
            ++e_pos;
        }
    }
    __syncthreads();

    // ---- 5. sort descending (key, then the lower column), one entry per thread: partners less than a wave apart trade
    // through shuffles, the others through LDS
    int npow = 1;
    while (npow < n_take) npow <<= 1;
    unsigned long long ent = tid < n_take ? sbuf[tid] : 0ull;            // 0: below every entry (their key halves are >= 1)
    for (int size = 2; size <= npow; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1)
            ent = tr_exchange(ent, stride, ((tid & size) == 0) == ((tid & stride) == 0), sbuf, tid);
    }

    if (SLICE) {                                                         // nvalid <= min(k, stage) = ws_per
        const size_t piece = (size_t)row * gridDim.x + blockIdx.x;
        if (tid < nvalid) ws_ent[piece * ws_per + tid] = ent - (unsigned)c0;     // ~column of the row: no borrow, c0 + c < C_row
        if (tid == 0) ws_stat[piece].ncand = ncand;
    } else {
        tr_write<LOGP>(row, k, tid, nvalid, ent, LOGP ? s_s[TR_WAVES] : 0.0, out_idx, out_val, out_logp, out_n);
    }
}

// The merge of renet_topk_rows_wide: one workgroup of P = blockDim.x threads (a power of two, max(k, 64) <= P <= 1024) per
// row folds the nsl slices' sorted entries, in slice order, into the row's sorted k best, and writes the row's results.
template <bool LOGP>
__global__ __launch_bounds__(TR_THREADS) void topk_rows_merge_kernel(const unsigned long long* __restrict__ ws_ent, int ws_per,
                                                                     const TrSlice* __restrict__ ws_stat, int nsl, int k,
                                                                     int32_t* __restrict__ out_idx,
                                                                     float* __restrict__ out_val,
                                                                     float* __restrict__ out_logp,
                                                                     int32_t* __restrict__ out_n) {
    __shared__ unsigned long long sbuf[TR_MAX_K];
    __shared__ double s_lse;
    __shared__ int s_ncand;
    const int row = blockIdx.x, tid = threadIdx.x, P = blockDim.x;
    const TrSlice* st = ws_stat + (size_t)row * nsl;
    const unsigned long long* e = ws_ent + (size_t)row * nsl * ws_per;
    if (tid < 64) {                                                      // wave 0: lane l takes the slices l, l + 64, ...
        int nc = 0;
        double M = -DBL_MAX, S = 0.0;
        for (int s = tid; s < nsl; s += 64) {
            nc += (int)st[s].ncand;                                      // (C_row < 2^31)
            if (LOGP) M = fmax(M, st[s].m);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            nc += __shfl_xor(nc, o);
            if (LOGP) M = fmax(M, __shfl_xor(M, o));
        }
        if (LOGP) {
            for (int s = tid; s < nsl; s += 64) S += st[s].s * exp(st[s].m - M);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) S += __shfl_xor(S, o);
        }
        if (tid == 0) {
            s_ncand = nc;
            s_lse = LOGP ? log(S) + M : 0.0;
        }
    }
    int cnt = min(k, (int)st[0].ncand);
    unsigned long long ent = tid < cnt ? e[tid] : 0ull;                  // 0: below every entry
    for (int s = 1; s < nsl; ++s) {
        cnt = min(k, (int)st[s].ncand);
        if (cnt == 0) continue;                                          // (the same in every thread)
        const int j = P - 1 - tid;
        const unsigned long long other = j < cnt ? e[(size_t)s * ws_per + j] : 0ull;
        ent = ent > other ? ent : other;                                 // the P best of both, a bitonic sequence
        for (int stride = P >> 1; stride > 0; stride >>= 1) ent = tr_exchange(ent, stride, (tid & stride) == 0, sbuf, tid);
    }
    __syncthreads();
    tr_write<LOGP>(row, k, tid, min(k, s_ncand), ent, s_lse, out_idx, out_val, out_logp, out_n);
}

// dynamic LDS of one workgroup: keys, histogram, sort buffer, the reduction slots (every part a multiple of 16 bytes)
inline size_t tr_lds_bytes(int C) {
    return (size_t)((C + 7) & ~3) * 4 + TR_BINS * 4 + TR_MAX_K * 8 + (TR_WAVES + 2) * 8 + TR_WAVES * 4 + TR_WAVES * 4 + 16;
}

// the argument checks both entries share, before anything depends on the width
inline bool tr_badarg(int ld, int n, int C, int k, const int32_t* cols, const int32_t* start, const int32_t* count, int len) {
    if (n < 0 || C < 1 || ld < C || k < 1 || k > TR_MAX_K || len < 0) return true;
    // a list is (cols, start, count) with the length of its table, or nothing at all
    return (cols || start || count) && (!cols || !start || !count);
}

// every instantiation may ask for the LDS of the widest piece
template <bool LOGP, bool SLICE>
inline hipError_t tr_set_lds() {
    return hipFuncSetAttribute((const void*)topk_rows_kernel<LOGP, SLICE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)tr_lds_bytes(TR_MAX_C));
}

// the piece width of a row of C columns: the caller's, or an even split into pieces of at most TRW_STAGE columns that start
// on multiples of 4 columns
inline int trw_stage(int C, int stage_cols) {
    if (stage_cols) return stage_cols;
    const int pieces = (C + TRW_STAGE - 1) / TRW_STAGE;
    return ((C + pieces - 1) / pieces + 3) & ~3;
}

}  // namespace

int renet_topk_rows(const float* scores, int ld, int n, int C, int k, const int32_t* cols, const int32_t* start,
                    const int32_t* count, int len, const int32_t* keep, int32_t* out_idx, float* out_val, float* out_logp,
                    int32_t* out_n, void* stream) {
    if (tr_badarg(ld, n, C, k, cols, start, count, len)) return RENET_ERR_BADARG;
    if (C > TR_MAX_C) return RENET_ERR_UNSUPPORTED;
    if (n == 0) return RENET_OK;
    if (!scores || !out_idx || !out_val || !out_n) return RENET_ERR_BADARG;
    static bool attr_set = false;          // benign race: the attribute is idempotent
    if (!attr_set) {
        hipError_t e = tr_set_lds<true, false>();
        if (e == hipSuccess) e = tr_set_lds<false, false>();
        if (e != hipSuccess) return (int)e;
        attr_set = true;
    }
    const dim3 grid(n), blk(TR_THREADS);
    const size_t lds = tr_lds_bytes(C);
    hipStream_t st = (hipStream_t)stream;
#define TR_GO(LOGP)                                                                                                     \
    RENET_LAUNCH((topk_rows_kernel<LOGP, false>), grid, blk, lds, st, scores, ld, C, k, cols, start, count, len, keep,     \
                 out_idx, out_val, out_logp, out_n, 0, 0, nullptr, 0, nullptr)
    if (out_logp) TR_GO(true);
    else TR_GO(false);
#undef TR_GO
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}

size_t renet_topk_rows_wide_workspace(int n, int C, int k, int stage_cols) {
    if (n < 1 || C < 1 || C > TRW_MAX_C || k < 1 || k > TR_MAX_K) return 0;
    if (stage_cols && (stage_cols < TRW_MIN_STAGE || stage_cols > TR_MAX_C)) return 0;
    const int stage = trw_stage(C, stage_cols), nsl = (C + stage - 1) / stage;
    return (size_t)n * nsl * ((size_t)min(k, stage) * sizeof(unsigned long long) + sizeof(TrSlice));
}

int renet_topk_rows_wide(const float* scores, int ld, int n, int C, int k, const int32_t* cols, const int32_t* start,
                         const int32_t* count, int len, const int32_t* keep, int32_t* out_idx, float* out_val,
                         float* out_logp, int32_t* out_n, int stage_cols, void* workspace, size_t workspace_bytes,
                         void* stream) {
    if (tr_badarg(ld, n, C, k, cols, start, count, len)) return RENET_ERR_BADARG;
    if (stage_cols && (stage_cols < TRW_MIN_STAGE || stage_cols > TR_MAX_C)) return RENET_ERR_BADARG;
    if (C > TRW_MAX_C) return RENET_ERR_UNSUPPORTED;
    if (n == 0) return RENET_OK;
    if (!scores || !out_idx || !out_val || !out_n) return RENET_ERR_BADARG;
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < renet_topk_rows_wide_workspace(n, C, k, stage_cols))
        return RENET_ERR_WORKSPACE;
    static bool attr_set = false;          // benign race: the attribute is idempotent
    if (!attr_set) {
        hipError_t e = tr_set_lds<true, true>();
        if (e == hipSuccess) e = tr_set_lds<false, true>();
        if (e != hipSuccess) return (int)e;
        attr_set = true;
    }
    const int stage = trw_stage(C, stage_cols), nsl = (C + stage - 1) / stage, per = min(k, stage);
    unsigned long long* ws_ent = (unsigned long long*)workspace;         // [n, nsl, per] entries, then [n, nsl] TrSlice
    TrSlice* ws_stat = (TrSlice*)(ws_ent + (size_t)n * nsl * per);
    const size_t lds = tr_lds_bytes(min(stage, C));
    hipStream_t st = (hipStream_t)stream;
    for (int row0 = 0; row0 < n; row0 += TRW_ROWS) {                     // (grid.y holds 65535 rows at most)
        const dim3 grid(nsl, min(n - row0, TRW_ROWS)), blk(TR_THREADS);
#define TR_GO(LOGP)                                                                                                     \
    RENET_LAUNCH((topk_rows_kernel<LOGP, true>), grid, blk, lds, st, scores, ld, C, k, cols, start, count, len, keep,      \
                 nullptr, nullptr, nullptr, nullptr, stage, row0, ws_ent, per, ws_stat)
        if (out_logp) TR_GO(true);
        else TR_GO(false);
#undef TR_GO
        RENET_LAUNCH_CHECK();
    }
    int P = 64;                                                          // one entry per thread: the power of two >= k
    while (P < k) P <<= 1;
    if (out_logp)
        RENET_LAUNCH((topk_rows_merge_kernel<true>), dim3(n), dim3(P), 0, st, ws_ent, per, ws_stat, nsl, k, out_idx, out_val,
                     out_logp, out_n);
    else
        RENET_LAUNCH((topk_rows_merge_kernel<false>), dim3(n), dim3(P), 0, st, ws_ent, per, ws_stat, nsl, k, out_idx,
                     out_val, out_logp, out_n);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}
