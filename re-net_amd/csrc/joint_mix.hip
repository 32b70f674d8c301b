// Recurrence prior for EVENT forecasts: the joint copy mix over (relation, entity) pairs, for gfx950 (not in the reference).
//   renet_joint_mix_rows mixes "what did this entity do before, and with whom" into the joint blocks of csrc/joint_rank.hip, in
//                        place, between renet_joint_row_offsets and the rank / top-k kernels
//                        (host statement: preprocess.PairIndex.event_rows + tests/event_prior_statement.py mix_block).
//   renet_joint_gold_rows(_decay) the prior's mass on ONE (relation, partner) pair per row, q = G / W with the same entity-wide
//                        W (and dq / d(decay)): what the loss THROUGH this mix needs of the prior (renet_joint_mix_ce in
//                        csrc/seq.hip; host statement: tests/event_gate_statement.py gold_rows).  At the end of this file.
//
// A GROUP g is one history: the entity ent[g], the query time t[g] and the as_of[g] <= t[g] its window was built with.  Over
// the facts (e, r, c, t' < as_of) of the entity's run of the role's pair tables (csrc/recurrence.hip):
//     w[r, c] = sum of 2^(-(t - t') inv_half_life),   W = the sum over ALL of them, every relation,   a = alpha if W > 0 else 0
// and with J = scores[g R + r, c] + off[g R + r] (the ONE fp32 addition of joint_rank.hip), widened to fp64,
//     M = fp32(J + log1p(-a))                            for a pair without a counted fact,
//     M = fp32(log((1 - a) exp(J) + a w[r, c] / W))      for a pair with counted facts;
// scores[g R + r, c] = M and off[g R + r] = 0, so that scores + off in one fp32 addition IS M for everything downstream.  A
// group that abstains (a = 0 because W = 0) keeps its rows and its off, bit for bit.
//
// TWO LAUNCHES.  W is entity-wide -- tens of thousands of facts for a busy entity -- and R row workgroups would each sum it
// again: a first launch of one workgroup per group sums it once (a strided pass over the entity's run, wave shuffles, four
// wave results folded in wave order) into mass [G], fp64, which the row launch reads and the caller may keep.
//
// THE ROW LAUNCH, one workgroup of 256 threads per (g, r), works IN PLACE, so a pair's J must be read before its column is
// overwritten and the dense pass must not touch a column twice.  Per window of JM_WIN columns (one window up to 65536
// entities; the windows start at the row's first 16-byte aligned element):
//   1. the walk of recurrence_mix_rows_kernel, step 5, over the window's piece of the (e, r) sub-run (the partners ascend
//      inside a sub-run: two binary searches cut the piece): every partner group's head finds the group's counted facts, sums
//      up to RC_LONG of them in time order -- a longer group goes to a list in LDS and is summed by a whole wave --, reads J
//      of ITS column, writes M there and sets the column's bit in an LDS bitmap.  Tiles of RC_TILE positions, as there.
//   2. after a barrier the dense pass: one 16-byte read and one 16-byte write per four columns, scalar head and tail as in
//      joint_rank.hip; a column whose bit is set is passed through as it stands.
// Every sum is in fp64 in an order fixed by the tables' content and the block size: no floating-point atomics (the bitmap's
// atomicOr is an integer OR), the same bits from run to run.  alpha = 0 with W > 0 walks nothing and writes fp32(J + 0) = J.
#include "common.h"
#include "recurrence_common.h"
#include <float.h>
#include <math.h>

namespace {

constexpr int JM_MAX_R = 1024;
constexpr int JM_WIN = 1 << 16;                           // columns per window of the bitmap
constexpr int JM_PAD = 4;                                 // bit of column c of window base wb: c - wb + JM_PAD (the scalar head sits below wb)
constexpr int JM_WORDS = JM_WIN / 32 + 1;

// one workgroup per group: mass[g] = W
__global__ __launch_bounds__(RC_THREADS) void joint_mix_mass_kernel(
    const int32_t* __restrict__ q_ent, const int32_t* __restrict__ q_t, const int32_t* __restrict__ q_as_of,
    const int32_t* __restrict__ p_t, int n_facts, const int32_t* __restrict__ ent_ptr, const int32_t* __restrict__ snap_ptr,
    int n_snaps, int num_ent, float inv_half_life, double* __restrict__ mass) {
    __shared__ double s_w[RC_WAVES];
    const int g = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int t = q_t[g], as_of = q_as_of[g];
    const double ihl = (double)inv_half_life;
    int a, b;
    rc_ent_run(n_facts, ent_ptr, snap_ptr, n_snaps, num_ent, q_ent[g], a, b);
    double w = 0.0;
    for (int k = a + tid; k < b; k += RC_THREADS) {
        const int tp = p_t[k];
        if (tp < as_of) w += rc_weight(t, tp, ihl);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) w += __shfl_xor(w, o);
    if (lane == 0) s_w[wave] = w;
    __syncthreads();
    if (tid != 0) return;
    double W = 0.0;
#pragma unroll
    for (int k = 0; k < RC_WAVES; ++k) W += s_w[k];
    mass[g] = W;
}

__device__ __forceinline__ float jm_dense(float x, float o, double lg) { return (float)((double)__fadd_rn(x, o) + lg); }

// the head's (or its wave's lane 0's) write of a pair with counted facts; x is the row, still holding the scores here
__device__ __forceinline__ void jm_put(float* x, int c, float o, double keep, double scaled_w, unsigned* s_bits,
                                       int wb) {
    x[c] = (float)log(keep * exp((double)__fadd_rn(x[c], o)) + scaled_w);
    const int bit = c - wb + JM_PAD;
    atomicOr(&s_bits[bit >> 5], 1u << (bit & 31));
}

// the bits of the four columns of vector v of the window: one nibble of one word
__device__ __forceinline__ unsigned jm_nib(const unsigned* s_bits, int v) {
    const int bit = 4 * v + JM_PAD;
    return (s_bits[bit >> 5] >> (bit & 31)) & 15u;
}

__device__ __forceinline__ float4 jm_dense4(float4 v, unsigned nib, float o, double lg) {
    return make_float4(nib & 1 ? v.x : jm_dense(v.x, o, lg), nib & 2 ? v.y : jm_dense(v.y, o, lg),
                       nib & 4 ? v.z : jm_dense(v.z, o, lg), nib & 8 ? v.w : jm_dense(v.w, o, lg));
}

__global__ __launch_bounds__(RC_THREADS) void joint_mix_rows_kernel(
    const int32_t* __restrict__ q_ent, const int32_t* __restrict__ q_t, const int32_t* __restrict__ q_as_of,
    const int32_t* __restrict__ p_rel, const int32_t* __restrict__ p_other, const int32_t* __restrict__ p_t, int n_facts,
    const int32_t* __restrict__ ent_ptr, const int32_t* __restrict__ snap_ptr, int n_snaps, int num_ent, float* scores, int ld,
    int R, int C, float* off, float alpha, float inv_half_life, const double* __restrict__ mass) {
    __shared__ unsigned s_bits[JM_WORDS];
    __shared__ int s_long[RC_LIST], s_cut[RC_LIST], s_nlong;
    const int row = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int g = row / R, r = row - g * R;
    const double W = mass[g];
    if (!(W > 0.0)) return;                                               // the prior abstains (uniform over the workgroup)
    const float o = off[row];
    __syncthreads();                                                      // every thread holds off[row]: thread 0 may zero it below
    const int t = q_t[g], as_of = q_as_of[g];
    const double ihl = (double)inv_half_life, al = (double)alpha;
    const double lg = log1p(-al), scale = al / W, keep = 1.0 - al;
    float* x = scores + (size_t)row * ld;

    int a = 0, b = 0;                                                     // the (e, r) sub-run; alpha = 0 walks nothing
    if (al > 0.0) rc_pair_run(p_rel, n_facts, ent_ptr, snap_ptr, n_snaps, num_ent, q_ent[g], r, a, b);

    // [0, head) scalar up to the first 16-byte aligned element, [head, head + 4 * nvec) as float4, the rest scalar
    const int head = min(C, (int)((4 - (((uintptr_t)x >> 2) & 3)) & 3));
    const int nvec = (C - head) >> 2;
    float4* xv = reinterpret_cast<float4*>(x + head);
    const bool one_window = head + JM_WIN >= C;

    for (int wi = 0; wi == 0 || head + wi * JM_WIN < C; ++wi) {
        const int wb = head + wi * JM_WIN;                                // window: the columns [lo, hi)
        const int lo = wi == 0 ? 0 : wb, hi = min(C, wb + JM_WIN);
        const bool last = wb + JM_WIN >= C;
        int pa = a, pb = b;                                               // its piece of the sub-run
        if (a < b && !one_window) {
            pa = rc_lower(p_other, a, b, lo);
            pb = rc_lower(p_other, pa, b, hi);
        }
        const bool walk = pa < pb;                                        // (uniform over the workgroup)
        if (walk) {
            if (wi > 0) __syncthreads();                                  // the previous window's dense pass has read the bitmap
            for (int i = tid; i < JM_WORDS; i += RC_THREADS) s_bits[i] = 0u;
        }

        // 1. the partner groups of the piece, each found by its head.  The counted facts of a group are [k, cut): the group
        // ends where the partner changes and is ascending in time, two binary searches.  A tile of RC_TILE positions holds at
        // most RC_TILE / RC_LONG + 1 heads of long groups, so the list never overflows.
        for (int base = pa; base < pb; base += RC_TILE) {                 // (one tile as a rule)
            if (tid == 0) s_nlong = 0;
            __syncthreads();                                              // also: the bitmap is zero
            const int tile_end = min(pb, base + RC_TILE);
            for (int k = base + tid; k < tile_end; k += RC_THREADS) {
                const int c = p_other[k];
                if ((k != a && p_other[k - 1] == c) || c < lo || c >= hi) continue;    // (a partner outside the row is never addressed)
                const int cut = rc_lower(p_t, k, rc_lower(p_other, k, b, c + 1), as_of);
                if (cut - k > RC_LONG) {
                    const int slot = atomicAdd(&s_nlong, 1);
                    if (slot < RC_LIST) {                                 // (always: see above)
                        s_long[slot] = k;
                        s_cut[slot] = cut;
                        continue;
                    }
                }
                double w = 0.0;
                for (int j = k; j < cut; ++j) w += rc_weight(t, p_t[j], ihl);
                if (w > 0.0) jm_put(x, c, o, keep, scale * w, s_bits, wb);
            }
            __syncthreads();
            const int nl = min(s_nlong, RC_LIST);
            for (int q = wave; q < nl; q += RC_WAVES) {
                const int k = s_long[q], cut = s_cut[q];
                double w = 0.0;
                for (int j = k + lane; j < cut; j += 64) w += rc_weight(t, p_t[j], ihl);
#pragma unroll
                for (int s = 32; s > 0; s >>= 1) w += __shfl_xor(w, s);
                if (lane == 0 && w > 0.0) jm_put(x, p_other[k], o, keep, scale * w, s_bits, wb);
            }
            __syncthreads();                                              // the list is reset at the top of the next tile; the
        }                                                                 // columns and the bitmap are written

        // 2. the dense pass over the window: vectors [v0, v1), and the scalar head (first window) and tail (last window)
        const int v0 = wi * (JM_WIN / 4), v1 = min(nvec, v0 + JM_WIN / 4);
        int i = v0 + tid;
        for (; i + 3 * RC_THREADS < v1; i += 4 * RC_THREADS) {
            float4 v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = xv[i + q * RC_THREADS];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                xv[i + q * RC_THREADS] = jm_dense4(v[q], walk ? jm_nib(s_bits, i + q * RC_THREADS - v0) : 0u, o, lg);
        }
        for (; i < v1; i += RC_THREADS) xv[i] = jm_dense4(xv[i], walk ? jm_nib(s_bits, i - v0) : 0u, o, lg);
        const int ntail = last ? C - head - 4 * nvec : 0;                 // < 4; head < 4
        const int nhead = wi == 0 ? head : 0;
        if (tid < nhead + ntail) {
            const int c = tid < nhead ? tid : 4 * nvec + tid - nhead + head;
            const int bit = c - wb + JM_PAD;
            if (!(walk && ((s_bits[bit >> 5] >> (bit & 31)) & 1u))) x[c] = jm_dense(x[c], o, lg);
        }
    }
    if (tid == 0) off[row] = 0.f;
}

// ---- the gold pair's prior mass: what the loss THROUGH the joint mix needs of the prior ---------------------------------
// One workgroup per row (e, r*, t, as_of, gold).  W: the strided pass, shuffle tree and wave fold of joint_mix_mass_kernel over
// the entity's whole run -- the same operations in the same order, so W here is fp32(mass[g]) there, bit for bit.  G: the gold
// group [k0, cut) of the (e, r*) sub-run -- contiguous, ascending in time, found as recurrence_gold_rows_kernel finds it --
// summed in the same strided shares through the same tree.  DECAY: the row's decay is ihl_row[row], and WD = sum of D w over the
// run and GD over the gold group (D = t - t' the lag) ride beside them: dq = -ln2 (GD W - G WD) / W^2.  The DECAY = false
// instance holds none of it.  Two (three) floats out per row, no atomics, no workspace.
template <bool DECAY>
__global__ __launch_bounds__(RC_THREADS) void joint_gold_rows_kernel(
    const int32_t* __restrict__ q_ent, const int32_t* __restrict__ q_rel, const int32_t* __restrict__ q_t,
    const int32_t* __restrict__ q_as_of, const int32_t* __restrict__ q_gold, const int32_t* __restrict__ p_rel,
    const int32_t* __restrict__ p_other, const int32_t* __restrict__ p_t, int n_facts, const int32_t* __restrict__ ent_ptr,
    const int32_t* __restrict__ snap_ptr, int n_snaps, int num_ent, int R, int C, float inv_half_life,
    const float* __restrict__ ihl_row, float* __restrict__ q_out, float* __restrict__ w_out, float* __restrict__ dq_out) {
    __shared__ double s_w[RC_WAVES], s_g[RC_WAVES];
    __shared__ double s_wd[DECAY ? RC_WAVES : 1], s_gd[DECAY ? RC_WAVES : 1];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int e = q_ent[row], r = q_rel[row], t = q_t[row], as_of = q_as_of[row], g = q_gold[row];
    const double ihl = DECAY ? (double)ihl_row[row] : (double)inv_half_life;
    int a, b;
    rc_ent_run(n_facts, ent_ptr, snap_ptr, n_snaps, num_ent, e, a, b);
    double w = 0.0, wd_sum = 0.0;                                         // (w: joint_mix_mass_kernel's accumulator, operation for operation)
    for (int k = a + tid; k < b; k += RC_THREADS) {
        const int tp = p_t[k];
        if (tp < as_of) {
            const double wk = rc_weight(t, tp, ihl);
            w += wk;
            if (DECAY) wd_sum += ((double)t - (double)tp) * wk;
        }
    }
    double g_sum = 0.0, gd_sum = 0.0;
    if (g >= 0 && g < C && r >= 0 && r < R && a < b) {                    // (uniform over the workgroup)
        // the (e, r*) sub-run: rc_pair_run()'s two searches inside the entity run [a, b) this kernel already holds (rc_pair_run
        // would look the run up again; keep the two alike).  r < R <= 1024: r + 1 cannot overflow
        const int ra = rc_lower(p_rel, a, b, r), rb = rc_lower(p_rel, ra, b, r + 1);
        const int k0 = rc_lower(p_other, ra, rb, g);
        const int cut = rc_lower(p_t, k0, rc_lower(p_other, k0, rb, g + 1), as_of);
        for (int j = k0 + tid; j < cut; j += RC_THREADS) {
            const int tp = p_t[j];
            const double wj = rc_weight(t, tp, ihl);
            g_sum += wj;
            if (DECAY) gd_sum += ((double)t - (double)tp) * wj;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        w += __shfl_xor(w, o);
        g_sum += __shfl_xor(g_sum, o);
        if (DECAY) {
            wd_sum += __shfl_xor(wd_sum, o);
            gd_sum += __shfl_xor(gd_sum, o);
        }
    }
    if (lane == 0) {
        s_w[wave] = w;
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
    for (int k = 0; k < RC_WAVES; ++k) {
        W += s_w[k];
        G += s_g[k];
        if (DECAY) {
            WD += s_wd[k];
            GD += s_gd[k];
        }
    }
    w_out[row] = (float)W;
    q_out[row] = W > 0.0 ? (float)(G / W) : 0.f;
    if (DECAY) dq_out[row] = (W > 0.0 && G > 0.0) ? (float)(-M_LN2 * rc_cross(GD, W, G, WD) / (W * W)) : 0.f;
}

static int joint_gold_front(const int32_t* ent, const int32_t* rel, const int32_t* t, const int32_t* as_of, const int32_t* gold,
                            int n, const int32_t* p_rel, const int32_t* p_other, const int32_t* p_t, int n_facts,
                            const int32_t* ent_ptr, const int32_t* snap_ptr, int n_snaps, int num_ent, int R, int C,
                            float inv_half_life, const float* ihl_row, bool decay, float* q, float* W, float* dq, void* stream) {
    if (n < 0 || R < 1 || R > JM_MAX_R || C < 1 || C > RENET_RECURRENCE_MAX_C || n_facts < 0 || n_snaps < 0 || num_ent < 0)
        return RENET_ERR_BADARG;
    if (!decay && (!(inv_half_life >= 0.f) || !(inv_half_life <= FLT_MAX))) return RENET_ERR_BADARG;
    if (n == 0) return RENET_OK;
    if (!ent || !rel || !t || !as_of || !gold || !q || !W || !ent_ptr || !snap_ptr || (decay && (!ihl_row || !dq)))
        return RENET_ERR_BADARG;
    if (n_facts > 0 && (!p_rel || !p_other || !p_t)) return RENET_ERR_BADARG;
    if (decay)
        RENET_LAUNCH(joint_gold_rows_kernel<true>, dim3(n), dim3(RC_THREADS), 0, (hipStream_t)stream, ent, rel, t, as_of, gold,
                     p_rel, p_other, p_t, n_facts, ent_ptr, snap_ptr, n_snaps, num_ent, R, C, 0.f, ihl_row, q, W, dq);
    else
        RENET_LAUNCH(joint_gold_rows_kernel<false>, dim3(n), dim3(RC_THREADS), 0, (hipStream_t)stream, ent, rel, t, as_of, gold,
                     p_rel, p_other, p_t, n_facts, ent_ptr, snap_ptr, n_snaps, num_ent, R, C, inv_half_life, nullptr, q, W,
                     nullptr);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}

}  // namespace

int renet_joint_gold_rows(const int32_t* ent, const int32_t* rel, const int32_t* t, const int32_t* as_of, const int32_t* gold,
                          int n, const int32_t* p_rel, const int32_t* p_other, const int32_t* p_t, int n_facts,
                          const int32_t* ent_ptr, const int32_t* snap_ptr, int n_snaps, int num_ent, int R, int C,
                          float inv_half_life, float* q, float* W, void* stream) {
    return joint_gold_front(ent, rel, t, as_of, gold, n, p_rel, p_other, p_t, n_facts, ent_ptr, snap_ptr, n_snaps, num_ent, R, C,
                            inv_half_life, nullptr, false, q, W, nullptr, stream);
}

// ihl_row is DEVICE memory: its range (finite, >= 0) is the caller's to keep; a bad decay gives a non-finite output, never an
// address: it only feeds exp2
int renet_joint_gold_rows_decay(const int32_t* ent, const int32_t* rel, const int32_t* t, const int32_t* as_of,
                                const int32_t* gold, int n, const int32_t* p_rel, const int32_t* p_other, const int32_t* p_t,
                                int n_facts, const int32_t* ent_ptr, const int32_t* snap_ptr, int n_snaps, int num_ent, int R,
                                int C, const float* ihl_row, float* q, float* W, float* dq, void* stream) {
    return joint_gold_front(ent, rel, t, as_of, gold, n, p_rel, p_other, p_t, n_facts, ent_ptr, snap_ptr, n_snaps, num_ent, R, C,
                            0.f, ihl_row, true, q, W, dq, stream);
}

int renet_joint_mix_rows(const int32_t* ent, const int32_t* t, const int32_t* as_of, int G, const int32_t* p_rel,
                         const int32_t* p_other, const int32_t* p_t, int n_facts, const int32_t* ent_ptr,
                         const int32_t* snap_ptr, int n_snaps, int num_ent, float* scores, int ld, int R, int C, float* off,
                         float alpha, float inv_half_life, double* mass, void* stream) {
    if (G < 0 || R < 1 || R > JM_MAX_R || C < 1 || C > RENET_RECURRENCE_MAX_C || ld < C) return RENET_ERR_BADARG;
    if (n_facts < 0 || n_snaps < 0 || num_ent < 0 || (long long)G * R > 0x7fffffffLL) return RENET_ERR_BADARG;
    if (!(alpha >= 0.f && alpha < 1.f) || !(inv_half_life >= 0.f) || !(inv_half_life <= FLT_MAX)) return RENET_ERR_BADARG;
    if (G == 0) return RENET_OK;
    if (!ent || !t || !as_of || !scores || !off || !mass || !ent_ptr || !snap_ptr) return RENET_ERR_BADARG;
    if (n_facts > 0 && (!p_rel || !p_other || !p_t)) return RENET_ERR_BADARG;
    hipStream_t st = (hipStream_t)stream;
    RENET_LAUNCH(joint_mix_mass_kernel, dim3(G), dim3(RC_THREADS), 0, st, ent, t, as_of, p_t, n_facts, ent_ptr, snap_ptr, n_snaps,
                 num_ent, inv_half_life, mass);
    RENET_LAUNCH_CHECK();
    RENET_LAUNCH(joint_mix_rows_kernel, dim3(G * R), dim3(RC_THREADS), 0, st, ent, t, as_of, p_rel, p_other, p_t, n_facts,
                 ent_ptr, snap_ptr, n_snaps, num_ent, scores, ld, R, C, off, alpha, inv_half_life, mass);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}
