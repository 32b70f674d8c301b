// What the kernels that read the resident PAIR TABLES share (csrc/recurrence.hip, csrc/joint_mix.hip): the walk's geometry,
// the fact run of an entity, the (entity, relation) sub-run and the weight of a fact.  The tables are described at the top of
// csrc/recurrence.hip.
#pragma once
#include "common.h"

namespace {

constexpr int RC_THREADS = 256;
constexpr int RC_WAVES = RC_THREADS / 64;
constexpr int RC_LONG = 128;                              // a partner group with more counted facts is summed by a whole wave
constexpr int RC_TILE = 1 << 15;                          // positions of a sub-run per pass over its heads
constexpr int RC_LIST = RC_TILE / RC_LONG + 8;            // long groups a tile can hold at most, and a little

__device__ __forceinline__ int rc_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

// first index of a[lo .. hi) with a[i] >= v
__device__ __forceinline__ int rc_lower(const int32_t* __restrict__ a, int lo, int hi, int v) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// start of the fact run of entity e, e in [0, num_ent]: snap_ptr[ent_ptr[e]], both reads kept inside their arrays
__device__ __forceinline__ int rc_run(const int32_t* __restrict__ ent_ptr, const int32_t* __restrict__ snap_ptr, int n_snaps,
                                      int n_facts, int e) {
    return rc_clamp(snap_ptr[rc_clamp(ent_ptr[e], 0, n_snaps)], 0, n_facts);
}

// the weight of a fact at t' for a query at t: 2^(-(t - t') inv_half_life); inv_half_life = 0 gives exactly 1
__device__ __forceinline__ double rc_weight(int t, int tp, double ihl) { return exp2(-((double)t - (double)tp) * ihl); }

// the whole fact run [a, b) of entity e in the pair tables; empty for an entity outside [0, num_ent)
__device__ __forceinline__ void rc_ent_run(int n_facts, const int32_t* __restrict__ ent_ptr, const int32_t* __restrict__ snap_ptr,
                                           int n_snaps, int num_ent, int e, int& a, int& b) {
    a = 0;
    b = 0;
    if (e >= 0 && e < num_ent && n_facts > 0) {
        a = rc_run(ent_ptr, snap_ptr, n_snaps, n_facts, e);
        b = max(a, rc_run(ent_ptr, snap_ptr, n_snaps, n_facts, e + 1));
    }
}

// the (e, r) sub-run [a, b) of the pair tables; empty for an entity outside [0, num_ent)
__device__ __forceinline__ void rc_pair_run(const int32_t* __restrict__ p_rel, int n_facts, const int32_t* __restrict__ ent_ptr,
                                            const int32_t* __restrict__ snap_ptr, int n_snaps, int num_ent, int e, int r,
                                            int& a, int& b) {
    int ra, rb;
    rc_ent_run(n_facts, ent_ptr, snap_ptr, n_snaps, num_ent, e, ra, rb);
    a = rc_lower(p_rel, ra, rb, r);
    b = r == 0x7fffffff ? rb : rc_lower(p_rel, a, rb, r + 1);
}

// a b - c d with BOTH products rounded (no fused multiply-add): equal products cancel to exactly 0, so a pair whose only
// counted partner is the gold one (q = 1 whatever the decay) has dq = 0, not the rounding residue of one product
__device__ __forceinline__ double rc_cross(double a, double b, double c, double d) {
#pragma clang fp contract(off)
    const double ab = a * b, cd = c * d;
    return ab - cd;
}

}  // namespace
