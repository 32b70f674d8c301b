// Recurrence prior on the resident stream: "what did (entity, relation) connect to before, how often, how recently".
//   renet_pair_append         keeps the relation-keyed view of one role's fact runs sorted under an append
//                             (host statement: preprocess.PairIndex.appended, array for array)
//   renet_recurrence_mix_rows turns that view into normalised log-probability rows, mixed with the model's logits
//                             (host statement: preprocess.PairIndex.prior_rows + tests/recurrence_statement.py mix_rows);
//                             renet_recurrence_mix_rows_gated is the same kernel body with one gate per row
//   renet_recurrence_gold_rows the prior mass of ONE column per row, q = w[gold] / W, and W: what the loss through the mix
//                             needs of the prior (host statement: tests/copy_gate_statement.py gold_rows)
//   renet_recurrence_mix_rows_decay / renet_recurrence_gold_rows_decay are the same two kernel bodies with ONE DECAY PER ROW,
//                             ihl_row[i] in the launch scalar's place -- a learned per-relation half-life -- and, for the gold
//                             entry, dq / d(decay) beside q (host statement: tests/half_life_statement.py)
//
// PAIR TABLES.  Per role the facts of entity e are the index range run(e) = [snap_ptr[ent_ptr[e]], snap_ptr[ent_ptr[e + 1]])
// of the resident history index (renet_store_append keeps it contiguous).  The pair tables p_rel / p_other / p_t hold the
// same facts over the same ranges, sorted inside a run by (relation, partner, time): the facts of one (e, r) are a
// contiguous sub-run, found by two binary searches over p_rel, and inside it every partner is one contiguous group,
// ascending in time.  Equal keys are indistinguishable, so the tables are a function of the multiset of facts.
//
// APPEND.  With the m new facts sorted by (entity, relation, partner, time), every place is a rank inside ONE entity:
//   old fact j of e      -> run'(e) + (j - run(e)) + #{new facts of e with key <  key_j}
//   i-th new fact of e   -> run'(e) + i            + #{old facts of e with key <= key_i}
// one thread per old fact and one per new fact, a binary search each; nothing is re-sorted, no atomics, no read-back.
//
// MIX.  One workgroup of 256 threads per row i = (ent, rel, t, as_of):
//   1. the (ent, rel) sub-run [a, b) -- every thread searches for itself (the loads are uniform across the workgroup);
//   2. one strided pass over the sub-run's facts with t' < as_of: W = sum of 2^(-(t - t') inv_half_life) in fp64, the
//      facts counted and the partner groups whose first (earliest) fact counts;
//   3. one sweep of the logits row for its logsumexp, online in fp64 as csrc/rank.hip does it, and the sums of 2. through
//      the same fixed wave-shuffle / LDS tree;
//   4. the dense term out[c] = fp32(l[c] - (lse - log(1 - a))), a = alpha when W > 0 and 0 otherwise;
//   5. after a barrier, the head of every partner group finds the group's counted facts (two binary searches: the group is
//      contiguous and ascending in time), sums them in time order -- a group of more than 128 facts is handed to a whole
//      wave instead -- and overwrites ITS column with fp32(log((1 - a) exp(l[o] - lse) + a w / W)).  Partner columns are
//      distinct inside a sub-run, so no two writers share an address; the barrier orders the overwrite behind the dense store.
// Every sum runs in an order fixed by the sub-run's content and the block size: no floating-point atomics, the same bits
// from run to run.  Traffic: the row is read twice (the second time from L2) and written once.  Rows of any width up to
// 2^20 columns are swept from memory; nothing is staged in LDS.
#include "common.h"
#include "recurrence_common.h"                            // the walk's geometry, rc_lower, rc_run, rc_weight, rc_pair_run, rc_cross
#include <float.h>
#include <math.h>

namespace {

// (rel, other, t) of fact k against the key (r, o, t): < 0, 0, > 0
__device__ __forceinline__ int rc_cmp(const int32_t* __restrict__ p_rel, const int32_t* __restrict__ p_other,
                                      const int32_t* __restrict__ p_t, int k, int r, int o, int t) {
    const int a = p_rel[k];
    if (a != r) return a < r ? -1 : 1;
    const int b = p_other[k];
    if (b != o) return b < o ? -1 : 1;
    const int c = p_t[k];
    return c < t ? -1 : (c > t ? 1 : 0);
}

// the first k of [lo, hi) whose key is >= (UPPER: >) the key (r, o, t); the range is sorted by key
template <bool UPPER>
__device__ __forceinline__ int rc_key_bound(const int32_t* __restrict__ p_rel, const int32_t* __restrict__ p_other,
                                            const int32_t* __restrict__ p_t, int lo, int hi, int r, int o, int t) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        const int c = rc_cmp(p_rel, p_other, p_t, mid, r, o, t);
        if (UPPER ? c <= 0 : c < 0) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// thread per old fact j
__global__ __launch_bounds__(RC_THREADS) void pair_append_old_kernel(
    const int32_t* __restrict__ p_rel, const int32_t* __restrict__ p_other, const int32_t* __restrict__ p_t, int n,
    const int32_t* __restrict__ ent_ptr, const int32_t* __restrict__ snap_ptr, int n_snaps,
    const int32_t* __restrict__ ent_ptr2, const int32_t* __restrict__ snap_ptr2, int n_snaps2, int num_ent,
    const int32_t* __restrict__ new_ent, const int32_t* __restrict__ new_rel, const int32_t* __restrict__ new_other,
    const int32_t* __restrict__ new_t, int m, int32_t* __restrict__ rel_out, int32_t* __restrict__ other_out,
    int32_t* __restrict__ t_out) {
    const int j = blockIdx.x * RC_THREADS + threadIdx.x;
    if (j >= n) return;
    // its entity: the last e with run(e) <= j (an entity without facts shares its start with the next one)
    int lo = 0, hi = num_ent + 1;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (rc_run(ent_ptr, snap_ptr, n_snaps, n, mid) <= j) lo = mid + 1; else hi = mid;
    }
    const int e = lo - 1;
    if (e < 0 || e >= num_ent) return;
    const int r = p_rel[j], o = p_other[j], t = p_t[j];
    const int na = rc_lower(new_ent, 0, m, e), nb = rc_lower(new_ent, na, m, e + 1);
    const int before = rc_key_bound<false>(new_rel, new_other, new_t, na, nb, r, o, t) - na;
    const long long p = (long long)rc_run(ent_ptr2, snap_ptr2, n_snaps2, n + m, e) +
                        (j - rc_run(ent_ptr, snap_ptr, n_snaps, n, e)) + before;
    if (p < 0 || p >= (long long)n + m) return;
    rel_out[p] = r;
    other_out[p] = o;
    t_out[p] = t;
}

// thread per sorted new fact i
__global__ __launch_bounds__(RC_THREADS) void pair_append_new_kernel(
    const int32_t* __restrict__ p_rel, const int32_t* __restrict__ p_other, const int32_t* __restrict__ p_t, int n,
    const int32_t* __restrict__ ent_ptr, const int32_t* __restrict__ snap_ptr, int n_snaps,
    const int32_t* __restrict__ ent_ptr2, const int32_t* __restrict__ snap_ptr2, int n_snaps2, int num_ent,
    const int32_t* __restrict__ new_ent, const int32_t* __restrict__ new_rel, const int32_t* __restrict__ new_other,
    const int32_t* __restrict__ new_t, int m, int32_t* __restrict__ rel_out, int32_t* __restrict__ other_out,
    int32_t* __restrict__ t_out) {
    const int i = blockIdx.x * RC_THREADS + threadIdx.x;
    if (i >= m) return;
    const int e = new_ent[i];
    if (e < 0 || e >= num_ent) return;
    const int r = new_rel[i], o = new_other[i], t = new_t[i];
    const int a = rc_run(ent_ptr, snap_ptr, n_snaps, n, e), b = max(a, rc_run(ent_ptr, snap_ptr, n_snaps, n, e + 1));
    const int upto = n > 0 ? rc_key_bound<true>(p_rel, p_other, p_t, a, b, r, o, t) - a : 0;
    const long long p = (long long)rc_run(ent_ptr2, snap_ptr2, n_snaps2, n + m, e) + (i - rc_lower(new_ent, 0, m, e)) + upto;
    if (p < 0 || p >= (long long)n + m) return;
    rel_out[p] = r;
    other_out[p] = o;
    t_out[p] = t;
}

// ---- the mix ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double rc_exp(float a, float b) { return exp((double)a - (double)b); }

// running (maximum m, sum s of exp(x - m)) of one thread: csrc/rank.hip's convention
__device__ __forceinline__ void rc_lse1(float x, float& m, double& s) {
    if (x > m) {
        s *= rc_exp(m, x);
        m = x;
    }
    s += rc_exp(x, m);
}
__device__ __forceinline__ void rc_lse4(const float4 v, float& m, double& s) {
    const float cm = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
    if (cm > m) {
        s *= rc_exp(m, cm);
        m = cm;
    }
    s += (rc_exp(v.x, m) + rc_exp(v.y, m)) + (rc_exp(v.z, m) + rc_exp(v.w, m));
}

__device__ __forceinline__ float rc_dense(float l, double shift) { return (float)((double)l - shift); }

// GATED: the gate of row i is alpha_row[i] instead of the launch's scalar; DECAY: its decay is ihl_row[i] instead of the
// launch's inv_half_life (steps 2 and 5 read it: the strided pass, the per-head sums, the whole-wave sums); everything else
// is one body
template <bool GATED, bool DECAY>
__global__ __launch_bounds__(RC_THREADS) void recurrence_mix_rows_kernel(
    const int32_t* __restrict__ q_ent, const int32_t* __restrict__ q_rel, const int32_t* __restrict__ q_t,
    const int32_t* __restrict__ q_as_of, const int32_t* __restrict__ p_rel, const int32_t* __restrict__ p_other,
    const int32_t* __restrict__ p_t, int n_facts, const int32_t* __restrict__ ent_ptr, const int32_t* __restrict__ snap_ptr,
    int n_snaps, int num_ent, const float* __restrict__ logits, int ld, int C, float alpha,
    const float* __restrict__ alpha_row, float inv_half_life, const float* __restrict__ ihl_row, float* __restrict__ out,
    int32_t* __restrict__ stats, float* __restrict__ stats_w) {
    __shared__ float s_m[RC_WAVES];
    __shared__ double s_s[RC_WAVES], s_w[RC_WAVES];
    __shared__ int s_np[RC_WAVES], s_nf[RC_WAVES];
    __shared__ int s_long[RC_LIST], s_cut[RC_LIST], s_nlong;
    const int row = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int e = q_ent[row], r = q_rel[row], t = q_t[row], as_of = q_as_of[row];
    const double ihl = DECAY ? (double)ihl_row[row] : (double)inv_half_life;

    // 1. the (e, r) sub-run [a, b)
    int a, b;
    rc_pair_run(p_rel, n_facts, ent_ptr, snap_ptr, n_snaps, num_ent, e, r, a, b);

    // 2. this thread's share of W and of the counts
    double w_sum = 0.0;
    int n_part = 0, n_fact = 0;
    for (int k = a + tid; k < b; k += RC_THREADS) {
        const int tp = p_t[k];
        if (tp >= as_of) continue;
        w_sum += rc_weight(t, tp, ihl);
        n_fact += 1;
        n_part += (k == a || p_other[k - 1] != p_other[k]) ? 1 : 0;     // (a group's first fact is its earliest)
    }

    // 3. the row's logsumexp (a NULL row is uniform: log C)
    const float* x = logits ? logits + (size_t)row * ld : nullptr;
    float* y = out + (size_t)row * C;
    float m = -FLT_MAX;
    double s = 0.0;
    const int head = x ? min(C, (int)((4 - (((uintptr_t)x >> 2) & 3)) & 3)) : 0;
    const int nvec = x ? (C - head) >> 2 : 0;
    if (x) {
        const float4* xv = reinterpret_cast<const float4*>(x + head);
        int i = tid;
        for (; i + 3 * RC_THREADS < nvec; i += 4 * RC_THREADS) {
            float4 v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = xv[i + q * RC_THREADS];
#pragma unroll
            for (int q = 0; q < 4; ++q) rc_lse4(v[q], m, s);
        }
        for (; i < nvec; i += RC_THREADS) rc_lse4(xv[i], m, s);
        const int ntail = C - head - 4 * nvec;                       // < 4; head < 4
        if (tid < head + ntail) rc_lse1(x[tid < head ? tid : 4 * nvec + tid], m, s);
    }

    float wm = m;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wm = fmaxf(wm, __shfl_xor(wm, o));
    double sd = s * rc_exp(m, wm);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sd += __shfl_xor(sd, o);
        w_sum += __shfl_xor(w_sum, o);
        n_part += __shfl_xor(n_part, o);
        n_fact += __shfl_xor(n_fact, o);
    }
    if (lane == 0) {
        s_m[wave] = wm;
        s_s[wave] = sd;
        s_w[wave] = w_sum;
        s_np[wave] = n_part;
        s_nf[wave] = n_fact;
    }
    __syncthreads();
    // every thread folds the four wave results in the same order: the same values everywhere
    float M = s_m[0];
#pragma unroll
    for (int w = 1; w < RC_WAVES; ++w) M = fmaxf(M, s_m[w]);
    double S = 0.0, W = 0.0;
    int NP = 0, NF = 0;
#pragma unroll
    for (int w = 0; w < RC_WAVES; ++w) {
        S += s_s[w] * rc_exp(s_m[w], M);
        W += s_w[w];
        NP += s_np[w];
        NF += s_nf[w];
    }
    const double lse = x ? log(S) + (double)M : log((double)C);
    const double al = W > 0.0 ? (double)(GATED ? alpha_row[row] : alpha) : 0.0;
    if (tid == 0 && stats) {
        stats[2 * (size_t)row] = NP;
        stats[2 * (size_t)row + 1] = NF;
        stats_w[row] = (float)W;
    }

    // 4. the dense term
    const double shift = lse - log1p(-al);                               // out = l - lse + log(1 - a)
    if (!x) {
        const float v = rc_dense(0.f, shift);
        for (int c = tid; c < C; c += RC_THREADS) y[c] = v;
    } else if (head == min(C, (int)((4 - (((uintptr_t)y >> 2) & 3)) & 3))) {
        // both rows reach 16-byte alignment at the same column: 16-byte loads and stores
        const float4* xv = reinterpret_cast<const float4*>(x + head);
        float4* yv = reinterpret_cast<float4*>(y + head);
        for (int i = tid; i < nvec; i += RC_THREADS) {
            const float4 v = xv[i];
            yv[i] = make_float4(rc_dense(v.x, shift), rc_dense(v.y, shift), rc_dense(v.z, shift), rc_dense(v.w, shift));
        }
        const int ntail = C - head - 4 * nvec;
        if (tid < head + ntail) {
            const int c = tid < head ? tid : 4 * nvec + tid;
            y[c] = rc_dense(x[c], shift);
        }
    } else {
        for (int c = tid; c < C; c += RC_THREADS) y[c] = rc_dense(x[c], shift);
    }
    if (!(al > 0.0)) return;                                              // (uniform over the workgroup)

    // 5. the partner groups, each found by its head, behind the dense stores.  The counted facts of a group are [k, cut):
    // the group ends where the partner changes and is ascending in time, two binary searches.  Up to RC_LONG facts are
    // summed by the head's thread in time order; a longer group goes to a list in LDS and is summed by a whole wave (lane-
    // strided shares, then the shuffle tree).  Which way a group goes depends on its length alone, and a tile of RC_TILE
    // positions holds at most RC_TILE / RC_LONG + 1 heads of long groups, so the list never overflows: the order of every
    // sum is fixed by the content.  (The order in which the list fills is not, and does not matter: one writer per column.)
    const double scale = al / W, keep = 1.0 - al;
    for (int base = a; base < b; base += RC_TILE) {                      // (uniform over the workgroup; one tile as a rule)
        if (tid == 0) s_nlong = 0;
        __syncthreads();                                                  // also: the dense stores are behind us
        const int tile_end = min(b, base + RC_TILE);
        for (int k = base + tid; k < tile_end; k += RC_THREADS) {
            const int o = p_other[k];
            if ((k != a && p_other[k - 1] == o) || o < 0 || o >= C) continue;   // (a partner outside the row is never addressed)
            const int cut = rc_lower(p_t, k, rc_lower(p_other, k, b, o + 1), as_of);
            if (cut - k > RC_LONG) {
                const int slot = atomicAdd(&s_nlong, 1);
                if (slot < RC_LIST) {                                     // (always: see above)
                    s_long[slot] = k;
                    s_cut[slot] = cut;
                    continue;
                }
            }
            double w = 0.0;
            for (int j = k; j < cut; ++j) w += rc_weight(t, p_t[j], ihl);
            if (w > 0.0) y[o] = (float)log(keep * exp((x ? (double)x[o] : 0.0) - lse) + scale * w);
        }
        __syncthreads();
        const int nl = min(s_nlong, RC_LIST);
        for (int g = wave; g < nl; g += RC_WAVES) {
            const int k = s_long[g], cut = s_cut[g];
            double w = 0.0;
            for (int j = k + lane; j < cut; j += 64) w += rc_weight(t, p_t[j], ihl);
#pragma unroll
            for (int q = 32; q > 0; q >>= 1) w += __shfl_xor(w, q);
            const int o = p_other[k];
            if (lane == 0 && w > 0.0) y[o] = (float)log(keep * exp((x ? (double)x[o] : 0.0) - lse) + scale * w);
        }
        __syncthreads();                                                  // the list is reset at the top of the next tile
    }
}

// ---- the gold column's prior mass ---------------------------------------------------------------------------------------
// One workgroup per row, the mix kernel's steps 1 and 2 and its reduction tree for W (the same operations in the same order:
// W here is stats_w there, bit for bit), and beside them the gold partner's group [k, cut) -- contiguous, ascending in time,
// three binary searches -- summed in the same strided shares through the same tree.  Two floats out per row, nothing else.
// DECAY: the row's decay is ihl_row[row], and two more sums ride the same shares and the same tree, WD = sum of D w over the
// sub-run and GD over the gold group (D = t - t' the lag): q = G / W has dq / d(decay) = -ln2 (GD W - G WD) / W^2, a third
// float per row.  The DECAY = false instance holds none of it: the arithmetic it had.
template <bool DECAY>
__global__ __launch_bounds__(RC_THREADS) void recurrence_gold_rows_kernel(
    const int32_t* __restrict__ q_ent, const int32_t* __restrict__ q_rel, const int32_t* __restrict__ q_t,
    const int32_t* __restrict__ q_as_of, const int32_t* __restrict__ q_gold, const int32_t* __restrict__ p_rel,
    const int32_t* __restrict__ p_other, const int32_t* __restrict__ p_t, int n_facts, const int32_t* __restrict__ ent_ptr,
    const int32_t* __restrict__ snap_ptr, int n_snaps, int num_ent, int C, float inv_half_life,
    const float* __restrict__ ihl_row, float* __restrict__ q_out, float* __restrict__ w_out, float* __restrict__ dq_out) {
    __shared__ double s_w[RC_WAVES], s_g[RC_WAVES];
    __shared__ double s_wd[DECAY ? RC_WAVES : 1], s_gd[DECAY ? RC_WAVES : 1];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int e = q_ent[row], r = q_rel[row], t = q_t[row], as_of = q_as_of[row], g = q_gold[row];
    const double ihl = DECAY ? (double)ihl_row[row] : (double)inv_half_life;
    int a, b;
    rc_pair_run(p_rel, n_facts, ent_ptr, snap_ptr, n_snaps, num_ent, e, r, a, b);
    double w_sum = 0.0, wd_sum = 0.0;
    for (int k = a + tid; k < b; k += RC_THREADS) {
        const int tp = p_t[k];
        if (tp >= as_of) continue;
        const double w = rc_weight(t, tp, ihl);
        w_sum += w;
        if (DECAY) wd_sum += ((double)t - (double)tp) * w;
    }
    double g_sum = 0.0, gd_sum = 0.0;
    if (g >= 0 && g < C && a < b) {                                       // (uniform over the workgroup)
        const int k0 = rc_lower(p_other, a, b, g);
        const int cut = rc_lower(p_t, k0, rc_lower(p_other, k0, b, g + 1), as_of);
        for (int j = k0 + tid; j < cut; j += RC_THREADS) {
            const int tp = p_t[j];
            const double w = rc_weight(t, tp, ihl);
            g_sum += w;
            if (DECAY) gd_sum += ((double)t - (double)tp) * w;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        w_sum += __shfl_xor(w_sum, o);
        g_sum += __shfl_xor(g_sum, o);
        if (DECAY) {
            wd_sum += __shfl_xor(wd_sum, o);
            gd_sum += __shfl_xor(gd_sum, o);
        }
    }
    if (lane == 0) {
        s_w[wave] = w_sum;
        s_g[wave] = g_sum;
        if (DECAY) {
            s_wd[wave] = wd_sum;
            s_gd[wave] = gd_sum;
        }
    }
    __syncthreads();
    if (tid != 0) return;
    double W = 0.0, G = 0.0, WD = 0.0, GD = 0.0;
#pragma unroll
    for (int w = 0; w < RC_WAVES; ++w) {
        W += s_w[w];
        G += s_g[w];
        if (DECAY) {
            WD += s_wd[w];
            GD += s_gd[w];
        }
    }
    w_out[row] = (float)W;
    q_out[row] = W > 0.0 ? (float)(G / W) : 0.f;
    if (DECAY) dq_out[row] = (W > 0.0 && G > 0.0) ? (float)(-M_LN2 * rc_cross(GD, W, G, WD) / (W * W)) : 0.f;
}

inline int rc_blocks(long long n) { return (int)((n + RC_THREADS - 1) / RC_THREADS); }

}  // namespace

extern "C" int renet_pair_append(const int32_t* p_rel, const int32_t* p_other, const int32_t* p_t, int n,
                                 const int32_t* ent_ptr, const int32_t* snap_ptr, int n_snaps, const int32_t* ent_ptr_new,
                                 const int32_t* snap_ptr_new, int n_snaps_new, int num_ent, const int32_t* new_ent,
                                 const int32_t* new_rel, const int32_t* new_other, const int32_t* new_t, int m,
                                 int32_t* p_rel_out, int32_t* p_other_out, int32_t* p_t_out, void* stream) {
    if (n < 0 || m < 0 || num_ent < 0 || n_snaps < 0 || n_snaps_new < 0) return RENET_ERR_BADARG;
    if ((long long)n + m > 0x7fffffffLL - RC_THREADS || (long long)num_ent + 1 > 0x7fffffffLL - RC_THREADS)
        return RENET_ERR_UNSUPPORTED;
    if (n + m == 0) return RENET_OK;
    if (!ent_ptr || !snap_ptr || !ent_ptr_new || !snap_ptr_new || !p_rel_out || !p_other_out || !p_t_out) return RENET_ERR_BADARG;
    if (n > 0 && (!p_rel || !p_other || !p_t)) return RENET_ERR_BADARG;
    if (m > 0 && (!new_ent || !new_rel || !new_other || !new_t)) return RENET_ERR_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (n > 0) {
        RENET_LAUNCH(pair_append_old_kernel, dim3(rc_blocks(n)), dim3(RC_THREADS), 0, st, p_rel, p_other, p_t, n, ent_ptr,
                     snap_ptr, n_snaps, ent_ptr_new, snap_ptr_new, n_snaps_new, num_ent, new_ent, new_rel, new_other, new_t, m,
                     p_rel_out, p_other_out, p_t_out);
        RENET_LAUNCH_CHECK();
    }
    if (m > 0) {
        RENET_LAUNCH(pair_append_new_kernel, dim3(rc_blocks(m)), dim3(RC_THREADS), 0, st, p_rel, p_other, p_t, n, ent_ptr,
                     snap_ptr, n_snaps, ent_ptr_new, snap_ptr_new, n_snaps_new, num_ent, new_ent, new_rel, new_other, new_t, m,
                     p_rel_out, p_other_out, p_t_out);
        RENET_LAUNCH_CHECK();
    }
    return RENET_OK;
}

static int recurrence_mix_front(const int32_t* ent, const int32_t* rel, const int32_t* t, const int32_t* as_of, int n,
                                const int32_t* p_rel, const int32_t* p_other, const int32_t* p_t, int n_facts,
                                const int32_t* ent_ptr, const int32_t* snap_ptr, int n_snaps, int num_ent, const float* logits,
                                int ld, int C, float alpha, const float* alpha_row, bool gated, float inv_half_life,
                                const float* ihl_row, bool decay, float* out, int32_t* stats, float* stats_w, void* stream) {
    if (n < 0 || C < 1 || C > RENET_RECURRENCE_MAX_C || n_facts < 0 || n_snaps < 0 || num_ent < 0) return RENET_ERR_BADARG;
    if (!(alpha >= 0.f && alpha < 1.f) || !(inv_half_life >= 0.f) || !(inv_half_life <= FLT_MAX)) return RENET_ERR_BADARG;
    if (logits && ld < C) return RENET_ERR_BADARG;
    if ((stats == nullptr) != (stats_w == nullptr)) return RENET_ERR_BADARG;
    if (n == 0) return RENET_OK;
    if (!ent || !rel || !t || !as_of || !out || !ent_ptr || !snap_ptr || (gated && !alpha_row) || (decay && !ihl_row))
        return RENET_ERR_BADARG;
    if (n_facts > 0 && (!p_rel || !p_other || !p_t)) return RENET_ERR_BADARG;
    if (decay)                                                            // (one gate per row as well: the learned prior's entry)
        RENET_LAUNCH((recurrence_mix_rows_kernel<true, true>), dim3(n), dim3(RC_THREADS), 0, (hipStream_t)stream, ent, rel, t,
                     as_of, p_rel, p_other, p_t, n_facts, ent_ptr, snap_ptr, n_snaps, num_ent, logits, ld, C, alpha, alpha_row,
                     inv_half_life, ihl_row, out, stats, stats_w);
    else if (gated)
        RENET_LAUNCH((recurrence_mix_rows_kernel<true, false>), dim3(n), dim3(RC_THREADS), 0, (hipStream_t)stream, ent, rel, t, as_of,
                     p_rel, p_other, p_t, n_facts, ent_ptr, snap_ptr, n_snaps, num_ent, logits, ld, C, alpha, alpha_row,
                     inv_half_life, ihl_row, out, stats, stats_w);
    else
        RENET_LAUNCH((recurrence_mix_rows_kernel<false, false>), dim3(n), dim3(RC_THREADS), 0, (hipStream_t)stream, ent, rel, t, as_of,
                     p_rel, p_other, p_t, n_facts, ent_ptr, snap_ptr, n_snaps, num_ent, logits, ld, C, alpha, alpha_row,
                     inv_half_life, ihl_row, out, stats, stats_w);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}

extern "C" int renet_recurrence_mix_rows(const int32_t* ent, const int32_t* rel, const int32_t* t, const int32_t* as_of, int n,
                                         const int32_t* p_rel, const int32_t* p_other, const int32_t* p_t, int n_facts,
                                         const int32_t* ent_ptr, const int32_t* snap_ptr, int n_snaps, int num_ent,
                                         const float* logits, int ld, int C, float alpha, float inv_half_life, float* out,
                                         int32_t* stats, float* stats_w, void* stream) {
    return recurrence_mix_front(ent, rel, t, as_of, n, p_rel, p_other, p_t, n_facts, ent_ptr, snap_ptr, n_snaps, num_ent, logits,
                                ld, C, alpha, nullptr, false, inv_half_life, nullptr, false, out, stats, stats_w, stream);
}

// alpha_row is DEVICE memory: its range [0, 1) is the caller's to keep (renet_hip.recurrence_mix_rows_gated checks it where
// the gate is built); a NaN or a gate >= 1 gives a non-finite row, never an address
extern "C" int renet_recurrence_mix_rows_gated(const int32_t* ent, const int32_t* rel, const int32_t* t, const int32_t* as_of,
                                               int n, const int32_t* p_rel, const int32_t* p_other, const int32_t* p_t,
                                               int n_facts, const int32_t* ent_ptr, const int32_t* snap_ptr, int n_snaps,
                                               int num_ent, const float* logits, int ld, int C, const float* alpha_row,
                                               float inv_half_life, float* out, int32_t* stats, float* stats_w, void* stream) {
    return recurrence_mix_front(ent, rel, t, as_of, n, p_rel, p_other, p_t, n_facts, ent_ptr, snap_ptr, n_snaps, num_ent, logits,
                                ld, C, 0.f, alpha_row, true, inv_half_life, nullptr, false, out, stats, stats_w, stream);
}

// alpha_row and ihl_row are DEVICE memory: the gate's range [0, 1) and the decay's (finite, >= 0) are the caller's to keep
// (recurrence.CopyGate.check reads both tables back where they change); a bad decay gives a non-finite row, never an address:
// it only feeds exp2
extern "C" int renet_recurrence_mix_rows_decay(const int32_t* ent, const int32_t* rel, const int32_t* t, const int32_t* as_of,
                                               int n, const int32_t* p_rel, const int32_t* p_other, const int32_t* p_t,
                                               int n_facts, const int32_t* ent_ptr, const int32_t* snap_ptr, int n_snaps,
                                               int num_ent, const float* logits, int ld, int C, const float* alpha_row,
                                               const float* ihl_row, float* out, int32_t* stats, float* stats_w, void* stream) {
    return recurrence_mix_front(ent, rel, t, as_of, n, p_rel, p_other, p_t, n_facts, ent_ptr, snap_ptr, n_snaps, num_ent, logits,
                                ld, C, 0.f, alpha_row, true, 0.f, ihl_row, true, out, stats, stats_w, stream);
}

extern "C" int renet_recurrence_gold_rows(const int32_t* ent, const int32_t* rel, const int32_t* t, const int32_t* as_of,
                                          const int32_t* gold, int n, const int32_t* p_rel, const int32_t* p_other,
                                          const int32_t* p_t, int n_facts, const int32_t* ent_ptr, const int32_t* snap_ptr,
                                          int n_snaps, int num_ent, int C, float inv_half_life, float* q, float* W,
                                          void* stream) {
    if (n < 0 || C < 1 || C > RENET_RECURRENCE_MAX_C || n_facts < 0 || n_snaps < 0 || num_ent < 0) return RENET_ERR_BADARG;
    if (!(inv_half_life >= 0.f) || !(inv_half_life <= FLT_MAX)) return RENET_ERR_BADARG;
    if (n == 0) return RENET_OK;
    if (!ent || !rel || !t || !as_of || !gold || !q || !W || !ent_ptr || !snap_ptr) return RENET_ERR_BADARG;
    if (n_facts > 0 && (!p_rel || !p_other || !p_t)) return RENET_ERR_BADARG;
    RENET_LAUNCH(recurrence_gold_rows_kernel<false>, dim3(n), dim3(RC_THREADS), 0, (hipStream_t)stream, ent, rel, t, as_of, gold,
                 p_rel, p_other, p_t, n_facts, ent_ptr, snap_ptr, n_snaps, num_ent, C, inv_half_life, nullptr, q, W, nullptr);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}

extern "C" int renet_recurrence_gold_rows_decay(const int32_t* ent, const int32_t* rel, const int32_t* t, const int32_t* as_of,
                                                const int32_t* gold, int n, const int32_t* p_rel, const int32_t* p_other,
                                                const int32_t* p_t, int n_facts, const int32_t* ent_ptr, const int32_t* snap_ptr,
                                                int n_snaps, int num_ent, int C, const float* ihl_row, float* q, float* W,
                                                float* dq, void* stream) {
    if (n < 0 || C < 1 || C > RENET_RECURRENCE_MAX_C || n_facts < 0 || n_snaps < 0 || num_ent < 0) return RENET_ERR_BADARG;
    if (n == 0) return RENET_OK;
    if (!ent || !rel || !t || !as_of || !gold || !ihl_row || !q || !W || !dq || !ent_ptr || !snap_ptr) return RENET_ERR_BADARG;
    if (n_facts > 0 && (!p_rel || !p_other || !p_t)) return RENET_ERR_BADARG;
    RENET_LAUNCH(recurrence_gold_rows_kernel<true>, dim3(n), dim3(RC_THREADS), 0, (hipStream_t)stream, ent, rel, t, as_of, gold,
                 p_rel, p_other, p_t, n_facts, ent_ptr, snap_ptr, n_snaps, num_ent, C, 0.f, ihl_row, q, W, dq);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}
