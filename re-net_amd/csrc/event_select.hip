// Global choice of the generated events of one timestamp (reference model.py:229-258: the num_k best continuations over all
// sampled entities, an entity sampled m times counted m times; host numpy in this project's multi-step path:
// model._winners_pruned's tail).  renet_select_events takes one block of per-row top-k lists (renet_topk_rows on a joint
// block [G * R, N_ent]) plus the winners carried from the blocks before it and leaves the shortest prefix, in
// (value descending, carry first, flat position ascending) order, whose summed multiplicity reaches num_k.
//
// Every candidate gets a UNIQUE 64-bit key whose unsigned order is that order:
//     key = order-preserving key of the fp32 value V (topk.hip's topk_key) << 32  |  ~place,
//     place = i for carry entry i (< 1024),  1024 + flat position for a block candidate (flat position < 2^31).
// A WEIGHTED radix select on that key -- six histogram passes over 12 + 12 + 8 value bits and 12 + 12 + 8 place bits, a
// bin's count being the summed multiplicity of its candidates -- finds the key T of the last candidate of the prefix; the
// candidates with key >= T (at most num_k, as every weight is >= 1) are collected in arrival order and one workgroup sorts
// them by key in LDS and writes the outputs.  The keys being unique, the result does not depend on the arrival order:
// integer histogram atomics and one slot counter are the only atomics.  A candidate's weight enters the histograms as
// min(max(mult, 1), num_k): the prefix is the same (a weight >= num_k ends it wherever it stands) and the 64-bit bin sums
// cannot overflow.  HBM-bound: each pass reads the first min(k, num_k) slots of every row (a row is sorted, so no later
// slot can be among num_k winners).
#include "common.h"
#include <math.h>

namespace {

constexpr int ES_BINS = 4096;
constexpr int ES_THREADS = 512;
constexpr int ES_MAX = 1024;                 // num_k, k, R and the carry length are at most this

struct EsState {
    unsigned long long prefix;               // the key bits decided so far (the high bits)
    unsigned long long need;                 // weight still to be covered inside the prefix's candidates
    int take_all;                            // the total weight is below num_k: every candidate is a winner
    int count;                               // collect pass: slot cursor
};

struct EsArgs {
    const int32_t* ent; const float* val; const float* off;
    const int32_t* g_ent; const float* g_lprior; const int32_t* g_mult;
    const int32_t *in_given, *in_rel, *in_other; const float* in_val; const int32_t* in_mult; const int32_t* in_n;
    int G, R, k, kk, num_k;                  // kk = min(k, num_k): the slots of a row that can matter
    long long total;                         // G * R * kk
};

__host__ __device__ constexpr int es_shift(int pass) {
    return pass == 0 ? 52 : pass == 1 ? 40 : pass == 2 ? 32 : pass == 3 ? 20 : pass == 4 ? 8 : 0;
}
__host__ __device__ constexpr int es_bits(int pass) { return (pass == 2 || pass == 5) ? 8 : 12; }

// topk.hip's key: unsigned order of keys == float order of the values; -0.0 as +0.0, a NaN below everything
__device__ __forceinline__ unsigned es_vkey(float v) {
    unsigned u = __float_as_uint(v);
    if (v != v) return 0u;
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned long long es_key(float v, unsigned place) {
    return ((unsigned long long)es_vkey(v) << 32) | (unsigned long long)(~place);
}
__device__ __forceinline__ unsigned es_weight(int mult, int num_k) { return (unsigned)min(max(mult, 1), num_k); }
__device__ __forceinline__ int es_carry_len(const EsArgs& a) { return a.in_n ? min(max(a.in_n[0], 0), a.num_k) : 0; }

// block candidate at flat index i of the [G * R, kk] view: false for an empty slot
__device__ __forceinline__ bool es_block_cand(const EsArgs& a, long long i, unsigned long long& key, float& v, int& g,
                                              int& r, int& other) {
    const int row = (int)(i / a.kk), j = (int)(i - (long long)row * a.kk);
    const size_t at = (size_t)row * a.k + j;
    other = a.ent[at];
    if (other < 0) return false;
    g = row / a.R;
    r = row - g * a.R;
    v = __fadd_rn(__fadd_rn(a.val[at], a.off[row]), a.g_lprior[g]);
    key = es_key(v, (unsigned)ES_MAX + (unsigned)at);
    return true;
}

__global__ void es_init_kernel(EsState* st, unsigned long long* hist, int num_k) {
    for (int i = threadIdx.x; i < ES_BINS; i += blockDim.x) hist[i] = 0ull;
    if (threadIdx.x == 0) { st->prefix = 0ull; st->need = (unsigned long long)num_k; st->take_all = 0; st->count = 0; }
}

// a workgroup histograms its slice of the block (workgroup 0 the carry too) in LDS -- a slice holds at most 2^21
// candidates of weight <= 1024: 32-bit bins -- and flushes the non-empty bins with 64-bit integer atomics
template <int PASS>
__global__ __launch_bounds__(ES_THREADS) void es_hist_kernel(EsArgs a, const EsState* __restrict__ st,
                                                             unsigned long long* __restrict__ hist) {
    if (PASS > 0 && st->take_all) return;
    __shared__ unsigned h[ES_BINS];
    constexpr int SH = es_shift(PASS), NB = 1 << es_bits(PASS), HI = SH + es_bits(PASS);
    for (int i = threadIdx.x; i < NB; i += ES_THREADS) h[i] = 0u;
    __syncthreads();
    const unsigned long long prefix = st->prefix;
    if (blockIdx.x == 0) {
        const int n_in = es_carry_len(a);
        for (int i = threadIdx.x; i < n_in; i += ES_THREADS) {
            const unsigned long long key = es_key(a.in_val[i], (unsigned)i);
            if (PASS == 0 || (key >> (HI & 63)) == prefix)
                atomicAdd(&h[(unsigned)(key >> SH) & (NB - 1)], es_weight(a.in_mult[i], a.num_k));
        }
    }
    const long long per = (a.total + gridDim.x - 1) / gridDim.x;
    const long long i0 = (long long)blockIdx.x * per, i1 = min(a.total, i0 + per);
    for (long long i = i0 + threadIdx.x; i < i1; i += ES_THREADS) {
        unsigned long long key;
        float v;
        int g, r, other;
        if (!es_block_cand(a, i, key, v, g, r, other)) continue;
        if (PASS == 0 || (key >> (HI & 63)) == prefix)
            atomicAdd(&h[(unsigned)(key >> SH) & (NB - 1)], es_weight(a.g_mult[g], a.num_k));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NB; i += ES_THREADS)
        if (h[i]) atomicAdd(&hist[i], (unsigned long long)h[i]);
}

// one workgroup: the highest bin b with (weight of the bins above b) < need <= (weight of the bins from b up); the prefix
// grows by b's bits, need shrinks by the weight above b; the histogram is cleared for the next pass.  Pass 0 also
// decides take_all.
template <int PASS>
__global__ __launch_bounds__(256) void es_pick_kernel(EsState* __restrict__ st, unsigned long long* __restrict__ hist) {
    constexpr int NB = 1 << es_bits(PASS), PER = NB / 256;   // thread t owns bins [t * PER, (t + 1) * PER)
    if (PASS > 0 && st->take_all) return;
    __shared__ unsigned long long part[256];
    __shared__ int s_owner;
    __shared__ unsigned long long s_above;
    unsigned long long loc[PER], tot = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) { loc[j] = hist[threadIdx.x * PER + j]; tot += loc[j]; }
    part[threadIdx.x] = tot;
    const unsigned long long need = st->need;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long above = 0;
        int t = 255;
        for (; t >= 0; --t) {
            if (above + part[t] >= need) break;
            above += part[t];
        }
        s_owner = t;                                           // -1: the total weight is short of need
        s_above = above;
    }
    __syncthreads();
    const int owner = s_owner;
    if (owner < 0) {
        if (threadIdx.x == 0) st->take_all = 1;                // (pass 0 only: later passes sum to >= need by construction)
    } else if ((int)threadIdx.x == owner) {
        unsigned long long above = s_above;
        int j = PER - 1;
        for (; j > 0; --j) {
            if (above + loc[j] >= need) break;
            above += loc[j];
        }
        st->prefix = (st->prefix << es_bits(PASS)) | (unsigned long long)(owner * PER + j);
        st->need = need - above;
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) hist[threadIdx.x * PER + j] = 0ull;
}

// the winners' records, in arrival order: key, then the five output columns
struct EsBuf {
    unsigned long long* key;
    int32_t *given, *rel, *other, *mult;
    float* val;
};

__global__ __launch_bounds__(ES_THREADS) void es_collect_kernel(EsArgs a, EsState* __restrict__ st, EsBuf w) {
    const unsigned long long T = st->take_all ? 0ull : st->prefix;
    if (blockIdx.x == 0) {
        const int n_in = es_carry_len(a);
        for (int i = threadIdx.x; i < n_in; i += ES_THREADS) {
            const float v = a.in_val[i];
            const unsigned long long key = es_key(v, (unsigned)i);
            if (key < T) continue;
            const int slot = atomicAdd(&st->count, 1);
            if (slot < a.num_k) {
                w.key[slot] = key; w.given[slot] = a.in_given[i]; w.rel[slot] = a.in_rel[i]; w.other[slot] = a.in_other[i];
                w.val[slot] = v; w.mult[slot] = a.in_mult[i];
            }
        }
    }
    const long long per = (a.total + gridDim.x - 1) / gridDim.x;
    const long long i0 = (long long)blockIdx.x * per, i1 = min(a.total, i0 + per);
    for (long long i = i0 + threadIdx.x; i < i1; i += ES_THREADS) {
        unsigned long long key;
        float v;
        int g, r, other;
        if (!es_block_cand(a, i, key, v, g, r, other) || key < T) continue;
        const int slot = atomicAdd(&st->count, 1);
        if (slot < a.num_k) {
            w.key[slot] = key; w.given[slot] = a.g_ent[g]; w.rel[slot] = r; w.other[slot] = other;
            w.val[slot] = v; w.mult[slot] = a.g_mult[g];
        }
    }
}

// one workgroup: bitonic sort of the (key, slot) pairs by key descending in LDS (keys are unique and non-zero; the padding
// is key 0), then the outputs in that order and the fill behind out_n
__global__ __launch_bounds__(ES_MAX) void es_sort_kernel(const EsState* __restrict__ st, EsBuf w, int num_k,
                                                         int32_t* __restrict__ out_given, int32_t* __restrict__ out_rel,
                                                         int32_t* __restrict__ out_other, float* __restrict__ out_val,
                                                         int32_t* __restrict__ out_mult, int32_t* __restrict__ out_n) {
    __shared__ unsigned long long key[ES_MAX];
    __shared__ int slot[ES_MAX];
    const int t = threadIdx.x;
    const int n = min(st->count, num_k);
    key[t] = t < n ? w.key[t] : 0ull;
    slot[t] = t;
    __syncthreads();
    for (int size = 2; size <= ES_MAX; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const int p = t ^ stride;
            if (p > t) {
                const bool desc = (t & size) == 0;
                const unsigned long long ka = key[t], kb = key[p];
                if (desc ? ka < kb : ka > kb) {
                    key[t] = kb; key[p] = ka;
                    const int sa = slot[t]; slot[t] = slot[p]; slot[p] = sa;
                }
            }
            __syncthreads();
        }
    }
    if (t < num_k) {
        if (t < n) {
            const int s = slot[t];
            out_given[t] = w.given[s]; out_rel[t] = w.rel[s]; out_other[t] = w.other[s]; out_val[t] = w.val[s];
            out_mult[t] = w.mult[s];
        } else {
            out_given[t] = -1; out_rel[t] = -1; out_other[t] = -1; out_val[t] = -INFINITY; out_mult[t] = 0;
        }
    }
    if (t == 0) out_n[0] = n;
}

constexpr size_t ES_OFF_STATE = (size_t)ES_BINS * sizeof(unsigned long long);
constexpr size_t ES_OFF_KEY = ES_OFF_STATE + 64;
constexpr size_t ES_OFF_COLS = ES_OFF_KEY + (size_t)ES_MAX * sizeof(unsigned long long);
constexpr size_t ES_WORKSPACE = ES_OFF_COLS + 5 * (size_t)ES_MAX * 4;
static_assert(sizeof(EsState) <= 64, "state slot");

bool es_dims_ok(int G, int R, int k, int num_k) {
    return G >= 0 && R >= 1 && R <= ES_MAX && k >= 1 && k <= ES_MAX && num_k >= 1 && num_k <= ES_MAX;
}

template <int PASS>
int es_pass(const EsArgs& a, int grid, EsState* st, unsigned long long* hist, hipStream_t s) {
    RENET_LAUNCH((es_hist_kernel<PASS>), dim3(grid), dim3(ES_THREADS), 0, s, a, st, hist);
    RENET_LAUNCH_CHECK();
    RENET_LAUNCH((es_pick_kernel<PASS>), dim3(1), dim3(256), 0, s, st, hist);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}

}  // namespace

extern "C" {

size_t renet_select_events_workspace(int G, int R, int k, int num_k) {
    return es_dims_ok(G, R, k, num_k) ? ES_WORKSPACE : 0;
}

int renet_select_events(const int32_t* ent, const float* val, const float* off, const int32_t* g_ent, const float* g_lprior,
                        const int32_t* g_mult, int G, int R, int k, int num_k, const int32_t* in_given,
                        const int32_t* in_rel, const int32_t* in_other, const float* in_val, const int32_t* in_mult,
                        const int32_t* in_n, int32_t* out_given, int32_t* out_rel, int32_t* out_other, float* out_val,
                        int32_t* out_mult, int32_t* out_n, void* workspace, size_t workspace_bytes, void* stream) {
    if (!es_dims_ok(G, R, k, num_k)) return RENET_ERR_BADARG;
    if (!out_given || !out_rel || !out_other || !out_val || !out_mult || !out_n) return RENET_ERR_BADARG;
    if (G > 0 && (!ent || !val || !off || !g_ent || !g_lprior || !g_mult)) return RENET_ERR_BADARG;
    const int n_carry = (in_given != 0) + (in_rel != 0) + (in_other != 0) + (in_val != 0) + (in_mult != 0) + (in_n != 0);
    if (n_carry != 0 && n_carry != 6) return RENET_ERR_BADARG;
    if ((long long)G * R * k > 0x7FFFFFFFll) return RENET_ERR_UNSUPPORTED;
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < ES_WORKSPACE) return RENET_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    unsigned long long* hist = (unsigned long long*)ws;
    EsState* st = (EsState*)(ws + ES_OFF_STATE);
    EsBuf w;
    w.key = (unsigned long long*)(ws + ES_OFF_KEY);
    int32_t* cols = (int32_t*)(ws + ES_OFF_COLS);
    w.given = cols; w.rel = cols + ES_MAX; w.other = cols + 2 * ES_MAX; w.mult = cols + 3 * ES_MAX;
    w.val = (float*)(cols + 4 * ES_MAX);
    EsArgs a;
    a.ent = ent; a.val = val; a.off = off; a.g_ent = g_ent; a.g_lprior = g_lprior; a.g_mult = g_mult;
    a.in_given = in_given; a.in_rel = in_rel; a.in_other = in_other; a.in_val = in_val; a.in_mult = in_mult; a.in_n = in_n;
    a.G = G; a.R = R; a.k = k; a.kk = min(k, num_k); a.num_k = num_k;
    a.total = (long long)G * R * a.kk;
    // ~8 k candidates per workgroup, at most 1024 workgroups (a slice then holds at most 2^21 candidates)
    const int grid = (int)max(1ll, min(1024ll, (a.total + 8191) / 8192));
    RENET_LAUNCH(es_init_kernel, dim3(1), dim3(256), 0, s, st, hist, num_k);
    RENET_LAUNCH_CHECK();
    int rc;
    if ((rc = es_pass<0>(a, grid, st, hist, s)) != RENET_OK) return rc;
    if ((rc = es_pass<1>(a, grid, st, hist, s)) != RENET_OK) return rc;
    if ((rc = es_pass<2>(a, grid, st, hist, s)) != RENET_OK) return rc;
    if ((rc = es_pass<3>(a, grid, st, hist, s)) != RENET_OK) return rc;
    if ((rc = es_pass<4>(a, grid, st, hist, s)) != RENET_OK) return rc;
    if ((rc = es_pass<5>(a, grid, st, hist, s)) != RENET_OK) return rc;
    RENET_LAUNCH(es_collect_kernel, dim3(grid), dim3(ES_THREADS), 0, s, a, st, w);
    RENET_LAUNCH_CHECK();
    RENET_LAUNCH(es_sort_kernel, dim3(1), dim3(ES_MAX), 0, s, st, w, num_k, out_given, out_rel, out_other, out_val,
                 out_mult, out_n);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}

}  // extern "C"
