// Device-side APPEND of newly observed facts to the resident history index of one role (renet_store_append) and the flat
// append of an int32 array (renet_append_i32): the "observe" half of a forecast / observe loop without a host rebuild.
// The host statement is preprocess.HistoryIndex.appended, array for array; the result equals the index of the longer
// stream bit for bit (tests/test_gpu_observed_append.py).
//
// New facts have t >= every old fact and come later in file order, so in the (entity, time, file order) sort they land at
// the END of their entity's run: nothing is re-sorted.  With the m new facts sorted the same way (the caller's work, m is
// small), every shift is a RANK in that sorted order:
//   fshift[e] = new facts of entities < e          = lower_bound(new_ent, e)
//   sshift[e] = snapshots OPENED by entities < e   = (exclusive scan of the open flags)[fshift[e]]
// where a new fact opens a snapshot when it starts an (entity, time) group that does not join the entity's last old snapshot
// (same timestamp).  The only scan is the one over the m + 1 open flags -- blocked, three launches, any m -- and the
// per-entity exclusive sums of length num_ent + 1 follow from it by one binary search per entity.  Then
//   ent_ptr'[e] = ent_ptr[e] + sshift[e];   old snapshot k of e -> k + sshift[e], snap_ptr' = snap_ptr[k] + fshift[e]
//   old sorted fact f of e -> f + fshift[e];   sorted new fact j of e -> (old facts of entities <= e) + j
//   old quadruple i: first' = first + sshift[its entity], count' = count;   new: first = max(ent_ptr'[e], sid - L)
// snap_ptr' is the scan of the merged snapshot sizes in the statement; here both kinds of snapshot know their start in
// closed form.  Integer work over a few MB: int32, no atomics, no LDS beyond the block scan, deterministic.  The old arrays
// are only read; every output is the caller's fresh allocation.
#include "common.h"

namespace {

constexpr int AP_THREADS = 256;
constexpr int AP_ITEMS = 4;
constexpr int AP_SPAN = AP_THREADS * AP_ITEMS;           // flags per block of the scan

// first index of a[0 .. n) with a[i] >= v / > v
__device__ __forceinline__ int ap_lower(const int32_t* __restrict__ a, int n, int v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ int ap_upper(const int32_t* __restrict__ a, int n, int v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// exclusive scan of one value per thread over the block's AP_THREADS threads (4 waves of 64); *total = the block's sum
__device__ __forceinline__ int ap_block_excl_scan(int v, int* total, int* wsum /* [4] LDS */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    __syncthreads();                                   // wsum may still be read by the previous call
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < AP_THREADS / 64; ++w) {
        const int s = wsum[w];
        if (w < wave) base += s;
        tot += s;
    }
    *total = tot;
    return base + inc - v;
}

// open[j], j < m: sorted new fact j starts an (entity, time) group that is a NEW snapshot; open[m] = 0 (the scan's end)
__global__ __launch_bounds__(AP_THREADS) void ap_open_kernel(const int32_t* __restrict__ ent_ptr,
                                                             const int32_t* __restrict__ snap_t,
                                                             const int32_t* __restrict__ new_ent,
                                                             const int32_t* __restrict__ new_t, int m, int num_ent,
                                                             int32_t* __restrict__ open) {
    const int j = blockIdx.x * AP_THREADS + threadIdx.x;
    if (j > m) return;
    int o = 0;
    if (j < m) {
        const int e = new_ent[j], t = new_t[j];
        const bool head_e = j == 0 || new_ent[j - 1] != e;
        o = head_e || new_t[j - 1] != t;
        if (head_e && e >= 0 && e < num_ent) {
            const int a = ent_ptr[e], b = ent_ptr[e + 1];
            if (b > a && snap_t[b - 1] == t) o = 0;                  // joins the entity's last old snapshot
        }
    }
    open[j] = o;
}

// ---- exclusive scan of in[0 .. n): block sums, the scan of the sums by ONE block, the blocks' own scans ----------------
__global__ __launch_bounds__(AP_THREADS) void ap_scan_sums_kernel(const int32_t* __restrict__ in, int n,
                                                                  int32_t* __restrict__ bsum) {
    __shared__ int wsum[AP_THREADS / 64];
    const int base = blockIdx.x * AP_SPAN + threadIdx.x * AP_ITEMS;
    int s = 0;
#pragma unroll
    for (int i = 0; i < AP_ITEMS; ++i)
        if (base + i < n) s += in[base + i];
    int tot;
    (void)ap_block_excl_scan(s, &tot, wsum);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

__global__ __launch_bounds__(AP_THREADS) void ap_scan_blocks_kernel(int32_t* __restrict__ bsum, int nb) {
    __shared__ int wsum[AP_THREADS / 64];
    int carry = 0;
    for (int c = 0; c < nb; c += AP_THREADS) {
        const int i = c + threadIdx.x;
        const int v = i < nb ? bsum[i] : 0;
        int tot;
        const int ex = ap_block_excl_scan(v, &tot, wsum);
        if (i < nb) bsum[i] = carry + ex;
        carry += tot;
    }
}

__global__ __launch_bounds__(AP_THREADS) void ap_scan_apply_kernel(const int32_t* __restrict__ in, int n,
                                                                   const int32_t* __restrict__ bsum,
                                                                   int32_t* __restrict__ out) {
    __shared__ int wsum[AP_THREADS / 64];
    const int base = blockIdx.x * AP_SPAN + threadIdx.x * AP_ITEMS;
    int v[AP_ITEMS], s = 0;
#pragma unroll
    for (int i = 0; i < AP_ITEMS; ++i) {
        v[i] = base + i < n ? in[base + i] : 0;
        s += v[i];
    }
    int tot;
    int run = bsum[blockIdx.x] + ap_block_excl_scan(s, &tot, wsum);
#pragma unroll
    for (int i = 0; i < AP_ITEMS; ++i) {
        if (base + i < n) out[base + i] = run;
        run += v[i];
    }
}

// thread per e in [0, num_ent]: the two exclusive sums, ent_ptr', and efp[e] = old facts of entities < e.  The thread of
// e = num_ent also writes the totals and, when the capacity is the true count, the end of snap_ptr'.
__global__ __launch_bounds__(AP_THREADS) void ap_entity_kernel(const int32_t* __restrict__ ent_ptr,
                                                               const int32_t* __restrict__ snap_ptr,
                                                               const int32_t* __restrict__ new_ent, int m, int num_ent,
                                                               int n_snaps, int n_quads,
                                                               const int32_t* __restrict__ oexc, int cap_snaps,
                                                               int32_t* __restrict__ fshift, int32_t* __restrict__ sshift,
                                                               int32_t* __restrict__ efp, int32_t* __restrict__ ent_ptr_out,
                                                               int32_t* __restrict__ snap_ptr_out,
                                                               int32_t* __restrict__ totals) {
    const int e = blockIdx.x * AP_THREADS + threadIdx.x;
    if (e > num_ent) return;
    const int lb = ap_lower(new_ent, m, e);
    const int ss = oexc[lb];
    const int k = ent_ptr[e];
    fshift[e] = lb;
    sshift[e] = ss;
    ent_ptr_out[e] = k + ss;
    efp[e] = snap_ptr[min(k, n_snaps)];
    if (e == num_ent) {
        totals[0] = k + ss;                              // snapshots of the longer index
        totals[1] = ss;                                  // of which opened by the new facts
        if (k + ss == cap_snaps) snap_ptr_out[cap_snaps] = n_quads + m;
    }
}

// thread per old snapshot k: its entity by search in ent_ptr, then the shifted copy
__global__ __launch_bounds__(AP_THREADS) void ap_old_snaps_kernel(const int32_t* __restrict__ ent_ptr,
                                                                  const int32_t* __restrict__ snap_t,
                                                                  const int32_t* __restrict__ snap_ptr, int num_ent,
                                                                  int n_snaps, const int32_t* __restrict__ fshift,
                                                                  const int32_t* __restrict__ sshift, int cap_snaps,
                                                                  int32_t* __restrict__ snap_t_out,
                                                                  int32_t* __restrict__ snap_ptr_out) {
    const int k = blockIdx.x * AP_THREADS + threadIdx.x;
    if (k >= n_snaps) return;
    const int e = ap_upper(ent_ptr, num_ent + 1, k) - 1;             // ent_ptr[e] <= k < ent_ptr[e + 1]
    if (e < 0 || e >= num_ent) return;
    const int k2 = k + sshift[e];
    if (k2 < 0 || k2 >= cap_snaps) return;
    snap_t_out[k2] = snap_t[k];
    snap_ptr_out[k2] = snap_ptr[k] + fshift[e];
}

// old sorted facts and old quadruples (both n_quads long), AP_ITEMS consecutive per thread: 16-byte loads of nbr_o, h_first,
// h_count, q_ent and 16-byte stores of first' / count' when `vec` (every pointer 16-byte aligned); nbr_o' is stored by
// element, its shift being arbitrary
__global__ __launch_bounds__(AP_THREADS) void ap_old_facts_kernel(const int32_t* __restrict__ nbr_o,
                                                                  const int32_t* __restrict__ h_first,
                                                                  const int32_t* __restrict__ h_count,
                                                                  const int32_t* __restrict__ q_ent, int num_ent,
                                                                  int n_quads, int m, const int32_t* __restrict__ efp,
                                                                  const int32_t* __restrict__ fshift,
                                                                  const int32_t* __restrict__ sshift, int vec,
                                                                  int32_t* __restrict__ nbr_o_out,
                                                                  int32_t* __restrict__ h_first_out,
                                                                  int32_t* __restrict__ h_count_out) {
    const int base = (blockIdx.x * AP_THREADS + threadIdx.x) * AP_ITEMS;
    if (base >= n_quads) return;
    alignas(16) int nb[AP_ITEMS], hf[AP_ITEMS], hc[AP_ITEMS], qe[AP_ITEMS];
    const bool full = vec && base + AP_ITEMS <= n_quads;
    if (full) {
        *reinterpret_cast<int4*>(nb) = *reinterpret_cast<const int4*>(nbr_o + base);
        *reinterpret_cast<int4*>(hf) = *reinterpret_cast<const int4*>(h_first + base);
        *reinterpret_cast<int4*>(hc) = *reinterpret_cast<const int4*>(h_count + base);
        *reinterpret_cast<int4*>(qe) = *reinterpret_cast<const int4*>(q_ent + base);
    } else {
#pragma unroll
        for (int i = 0; i < AP_ITEMS; ++i) {
            const int f = min(base + i, n_quads - 1);
            nb[i] = nbr_o[f]; hf[i] = h_first[f]; hc[i] = h_count[f]; qe[i] = q_ent[f];
        }
    }
    // the entity of sorted fact `base`; the next facts mostly stay in it, else move on a few entities
    int e = ap_upper(efp, num_ent + 1, base) - 1;
#pragma unroll
    for (int i = 0; i < AP_ITEMS; ++i) {
        const int f = base + i;
        if (f >= n_quads) break;
        while (e + 1 < num_ent && efp[e + 1] <= f) ++e;
        const int p = f + fshift[max(e, 0)];
        if (p >= 0 && p < n_quads + m) nbr_o_out[p] = nb[i];
        const int q = qe[i];
        hf[i] += (q >= 0 && q < num_ent) ? sshift[q] : 0;
    }
    if (full) {
        *reinterpret_cast<int4*>(h_first_out + base) = *reinterpret_cast<const int4*>(hf);
        *reinterpret_cast<int4*>(h_count_out + base) = *reinterpret_cast<const int4*>(hc);
    } else {
#pragma unroll
        for (int i = 0; i < AP_ITEMS; ++i)
            if (base + i < n_quads) { h_first_out[base + i] = hf[i]; h_count_out[base + i] = hc[i]; }
    }
}

// thread per sorted new fact j: its place behind its entity's old run, its snapshot (opened here when open[j]), and the
// history window of the new quadruple it came from (input position new_pos[j])
__global__ __launch_bounds__(AP_THREADS) void ap_new_kernel(const int32_t* __restrict__ new_ent,
                                                            const int32_t* __restrict__ new_t,
                                                            const int32_t* __restrict__ new_other,
                                                            const int32_t* __restrict__ new_pos, int m, int num_ent,
                                                            int n_quads, int history_len, const int32_t* __restrict__ open,
                                                            const int32_t* __restrict__ oexc,
                                                            const int32_t* __restrict__ fshift,
                                                            const int32_t* __restrict__ sshift,
                                                            const int32_t* __restrict__ efp,
                                                            const int32_t* __restrict__ ent_ptr_out, int cap_snaps,
                                                            int32_t* __restrict__ snap_t_out,
                                                            int32_t* __restrict__ snap_ptr_out,
                                                            int32_t* __restrict__ nbr_o_out,
                                                            int32_t* __restrict__ h_first_out,
                                                            int32_t* __restrict__ h_count_out) {
    const int j = blockIdx.x * AP_THREADS + threadIdx.x;
    if (j >= m) return;
    const int e = new_ent[j];
    if (e < 0 || e >= num_ent) return;
    const int rank = oexc[j + 1] - oexc[fshift[e]];                  // snapshots opened by e up to and including j's
    const int sid = ent_ptr_out[e + 1] - (sshift[e + 1] - sshift[e]) + rank - 1;
    const int pos = efp[e + 1] + j;
    if (pos >= 0 && pos < n_quads + m) nbr_o_out[pos] = new_other[j];
    if (open[j] && sid >= 0 && sid < cap_snaps) {
        snap_t_out[sid] = new_t[j];
        snap_ptr_out[sid] = pos;
    }
    const int q = new_pos[j];
    if (q >= 0 && q < m) {
        const int first = max(ent_ptr_out[e], sid - history_len);
        h_first_out[n_quads + q] = first;
        h_count_out[n_quads + q] = sid - first;
    }
}

__global__ void ap_totals_kernel(int32_t* __restrict__ totals, int n_snaps, int opened) {
    totals[0] = n_snaps;
    totals[1] = opened;
}

// out = old[0 .. n_old) ++ add[0 .. n_add), 16 bytes per thread where both sides allow it
__global__ __launch_bounds__(AP_THREADS) void ap_concat_kernel(const int32_t* __restrict__ old, int n_old,
                                                               const int32_t* __restrict__ add, int n_add, int vec,
                                                               int32_t* __restrict__ out) {
    const int base = (blockIdx.x * AP_THREADS + threadIdx.x) * AP_ITEMS;
    const int n = n_old + n_add;
    if (base >= n) return;
    if (vec && base + AP_ITEMS <= n_old) {
        *reinterpret_cast<int4*>(out + base) = *reinterpret_cast<const int4*>(old + base);
        return;
    }
#pragma unroll
    for (int i = 0; i < AP_ITEMS; ++i) {
        const int p = base + i;
        if (p < n) out[p] = p < n_old ? old[p] : add[p - n_old];
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline int blocks_for(long long n) { return (int)((n + AP_THREADS - 1) / AP_THREADS); }
inline size_t pad256(size_t n_ints) { return (n_ints * sizeof(int32_t) + 255) & ~(size_t)255; }

}  // namespace

extern "C" size_t renet_store_append_workspace(int num_ent, int m) {
    if (num_ent < 0 || m < 0) return 0;
    const size_t nb = ((size_t)m + 1 + AP_SPAN - 1) / AP_SPAN;
    return 2 * pad256((size_t)m + 1) + pad256(nb) + 3 * pad256((size_t)num_ent + 1);
}

extern "C" int renet_store_append(const int32_t* ent_ptr, const int32_t* snap_t, const int32_t* snap_ptr,
                                  const int32_t* nbr_o, const int32_t* h_first, const int32_t* h_count,
                                  const int32_t* q_ent, int num_ent, int n_snaps, int n_quads, int history_len,
                                  const int32_t* new_ent, const int32_t* new_t, const int32_t* new_other,
                                  const int32_t* new_pos, int m, int cap_snaps, int32_t* ent_ptr_out, int32_t* snap_t_out,
                                  int32_t* snap_ptr_out, int32_t* nbr_o_out, int32_t* h_first_out, int32_t* h_count_out,
                                  int32_t* totals, void* workspace, size_t workspace_bytes, void* stream) {
    if (num_ent < 0 || n_snaps < 0 || n_quads < 0 || history_len < 0 || m < 0 || cap_snaps < 0) return RENET_ERR_BADARG;
    if (!ent_ptr || !snap_ptr || !ent_ptr_out || !snap_ptr_out || !totals) return RENET_ERR_BADARG;
    if (n_snaps > 0 && (!snap_t || !snap_t_out)) return RENET_ERR_BADARG;
    if (n_quads > 0 && (!nbr_o || !h_first || !h_count || !q_ent)) return RENET_ERR_BADARG;
    if (m > 0 && (!new_ent || !new_t || !new_other || !new_pos || !snap_t_out)) return RENET_ERR_BADARG;
    if (n_quads + m > 0 && (!nbr_o_out || !h_first_out || !h_count_out)) return RENET_ERR_BADARG;
    // totals beyond int32: refused before any launch (AP_ITEMS facts per thread are indexed in int, too)
    const long long lim = 0x7fffffffLL - AP_SPAN;
    if ((long long)n_quads + m > lim || (long long)n_snaps + m > lim || (long long)num_ent + 1 > lim) return RENET_ERR_UNSUPPORTED;
    if (cap_snaps < n_snaps || cap_snaps > n_snaps + m) return RENET_ERR_BADARG;
    hipStream_t st = (hipStream_t)stream;

    if (m == 0) {                                        // nothing observed: copies
        (void)hipGetLastError();
        hipError_t err = hipMemcpyAsync(ent_ptr_out, ent_ptr, ((size_t)num_ent + 1) * 4, hipMemcpyDeviceToDevice, st);
        if (err == hipSuccess) err = hipMemcpyAsync(snap_ptr_out, snap_ptr, ((size_t)n_snaps + 1) * 4, hipMemcpyDeviceToDevice, st);
        if (err == hipSuccess && n_snaps) err = hipMemcpyAsync(snap_t_out, snap_t, (size_t)n_snaps * 4, hipMemcpyDeviceToDevice, st);
        if (err == hipSuccess && n_quads) err = hipMemcpyAsync(nbr_o_out, nbr_o, (size_t)n_quads * 4, hipMemcpyDeviceToDevice, st);
        if (err == hipSuccess && n_quads) err = hipMemcpyAsync(h_first_out, h_first, (size_t)n_quads * 4, hipMemcpyDeviceToDevice, st);
        if (err == hipSuccess && n_quads) err = hipMemcpyAsync(h_count_out, h_count, (size_t)n_quads * 4, hipMemcpyDeviceToDevice, st);
        if (err != hipSuccess) return (int)err;
        RENET_LAUNCH(ap_totals_kernel, dim3(1), dim3(1), 0, st, totals, n_snaps, 0);
        RENET_LAUNCH_CHECK();
        return RENET_OK;
    }

    if (!workspace || workspace_bytes < renet_store_append_workspace(num_ent, m)) return RENET_ERR_BADARG;
    const int n_flags = m + 1, nb = (n_flags + AP_SPAN - 1) / AP_SPAN;
    char* w = static_cast<char*>(workspace);
    int32_t* open = reinterpret_cast<int32_t*>(w);    w += pad256(n_flags);
    int32_t* oexc = reinterpret_cast<int32_t*>(w);    w += pad256(n_flags);
    int32_t* bsum = reinterpret_cast<int32_t*>(w);    w += pad256(nb);
    int32_t* fshift = reinterpret_cast<int32_t*>(w);  w += pad256((size_t)num_ent + 1);
    int32_t* sshift = reinterpret_cast<int32_t*>(w);  w += pad256((size_t)num_ent + 1);
    int32_t* efp = reinterpret_cast<int32_t*>(w);

    RENET_LAUNCH(ap_open_kernel, dim3(blocks_for(n_flags)), dim3(AP_THREADS), 0, st, ent_ptr, snap_t, new_ent, new_t, m,
                 num_ent, open);
    RENET_LAUNCH_CHECK();
    RENET_LAUNCH(ap_scan_sums_kernel, dim3(nb), dim3(AP_THREADS), 0, st, open, n_flags, bsum);
    RENET_LAUNCH_CHECK();
    RENET_LAUNCH(ap_scan_blocks_kernel, dim3(1), dim3(AP_THREADS), 0, st, bsum, nb);
    RENET_LAUNCH_CHECK();
    RENET_LAUNCH(ap_scan_apply_kernel, dim3(nb), dim3(AP_THREADS), 0, st, open, n_flags, bsum, oexc);
    RENET_LAUNCH_CHECK();
    RENET_LAUNCH(ap_entity_kernel, dim3(blocks_for((long long)num_ent + 1)), dim3(AP_THREADS), 0, st, ent_ptr, snap_ptr,
                 new_ent, m, num_ent, n_snaps, n_quads, oexc, cap_snaps, fshift, sshift, efp, ent_ptr_out, snap_ptr_out,
                 totals);
    RENET_LAUNCH_CHECK();
    if (n_snaps > 0) {
        RENET_LAUNCH(ap_old_snaps_kernel, dim3(blocks_for(n_snaps)), dim3(AP_THREADS), 0, st, ent_ptr, snap_t, snap_ptr,
                     num_ent, n_snaps, fshift, sshift, cap_snaps, snap_t_out, snap_ptr_out);
        RENET_LAUNCH_CHECK();
    }
    if (n_quads > 0) {
        const int vec = aligned16(nbr_o) && aligned16(h_first) && aligned16(h_count) && aligned16(q_ent) &&
                        aligned16(h_first_out) && aligned16(h_count_out);
        RENET_LAUNCH(ap_old_facts_kernel, dim3(blocks_for(((long long)n_quads + AP_ITEMS - 1) / AP_ITEMS)), dim3(AP_THREADS),
                     0, st, nbr_o, h_first, h_count, q_ent, num_ent, n_quads, m, efp, fshift, sshift, vec, nbr_o_out,
                     h_first_out, h_count_out);
        RENET_LAUNCH_CHECK();
    }
    RENET_LAUNCH(ap_new_kernel, dim3(blocks_for(m)), dim3(AP_THREADS), 0, st, new_ent, new_t, new_other, new_pos, m, num_ent,
                 n_quads, history_len, open, oexc, fshift, sshift, efp, ent_ptr_out, cap_snaps, snap_t_out, snap_ptr_out,
                 nbr_o_out, h_first_out, h_count_out);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}

extern "C" int renet_append_i32(const int32_t* old, int n_old, const int32_t* add, int n_add, int32_t* out, void* stream) {
    if (n_old < 0 || n_add < 0) return RENET_ERR_BADARG;
    if ((long long)n_old + n_add > 0x7fffffffLL - AP_SPAN) return RENET_ERR_UNSUPPORTED;
    if (n_old + n_add == 0) return RENET_OK;
    if ((n_old && !old) || (n_add && !add) || !out) return RENET_ERR_BADARG;
    const int vec = aligned16(old) && aligned16(out);
    RENET_LAUNCH(ap_concat_kernel, dim3(blocks_for(((long long)n_old + n_add + AP_ITEMS - 1) / AP_ITEMS)), dim3(AP_THREADS), 0,
                 (hipStream_t)stream, old, n_old, add, n_add, vec, out);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}
