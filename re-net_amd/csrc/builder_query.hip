// History windows of ARBITRARY (entity, as_of) queries against the resident history index (renet_query_histories): the
// lookup that preprocess.HistoryIndex does for the stream's own facts while it is built, as one kernel, so that queries
// which are already device tensors become a builder batch without a host round trip.  A front of its own beside the three
// builder fronts: it shares no kernel and no scratch with them (builder_common.h is not included), so their code objects
// do not change.  Integer work, a few KB per call: no LDS, no atomics, plain vector stores.
#include "common.h"

namespace {

struct QueryIndex {
    const int32_t* ent_ptr[2];
    const int32_t* snap_t[2];
};

// thread per (role, query) pair p in [0, 2 n): role = p >= n.  sid = the first snapshot of the entity's range
// [ent_ptr[e], ent_ptr[e + 1]) with snap_t >= as_of (binary search); the window is the <= history_len snapshots before it.
// An entity outside [0, num_ent) -- an absent side -- gives (0, 0).
__global__ __launch_bounds__(256) void query_histories_kernel(QueryIndex ix, int num_ent, int history_len,
                                                              const int32_t* __restrict__ ent,
                                                              const int32_t* __restrict__ as_of, int n,
                                                              int32_t* __restrict__ h_first,
                                                              int32_t* __restrict__ h_count) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= 2 * n) return;
    const int role = p >= n;
    const int e = ent[p];
    int first = 0, count = 0;
    if (e >= 0 && e < num_ent) {
        const int32_t* __restrict__ st = ix.snap_t[role];
        const int begin = ix.ent_ptr[role][e];
        const int t = as_of[p - role * n];
        int lo = begin, hi = ix.ent_ptr[role][e + 1];
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (st[mid] < t) lo = mid + 1; else hi = mid;
        }
        first = max(begin, lo - history_len);
        count = lo - first;
    }
    h_first[p] = first;
    h_count[p] = count;
}

}  // namespace

extern "C" int renet_query_histories(const int32_t* ent_ptr0, const int32_t* ent_ptr1, const int32_t* snap_t0,
                                     const int32_t* snap_t1, int num_ent, int history_len, const int32_t* ent,
                                     const int32_t* as_of, int n, int32_t* h_first, int32_t* h_count, void* stream) {
    if (n < 0 || n > (1 << 29) || num_ent < 0 || history_len < 0) return RENET_ERR_BADARG;
    if (n == 0) return RENET_OK;
    if (!ent_ptr0 || !ent_ptr1 || !ent || !as_of || !h_first || !h_count) return RENET_ERR_BADARG;
    QueryIndex ix;
    ix.ent_ptr[0] = ent_ptr0; ix.ent_ptr[1] = ent_ptr1;
    ix.snap_t[0] = snap_t0; ix.snap_t[1] = snap_t1;
    const int total = 2 * n;
    RENET_LAUNCH(query_histories_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, ix, num_ent,
                 history_len, ent, as_of, n, h_first, h_count);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}
