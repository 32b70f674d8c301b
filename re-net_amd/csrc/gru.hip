// Fused GRU over the packed <= seq_len history window (torch.nn.GRU semantics: 1 layer, h0 = 0,
// gate order r,z,n; reference model.py:28-29,86,94 and global_model.py:25,49).
//
// The input projection Gi = X W_ih^T + b_ih is one large GEMM done by the caller.  The recurrence is ONE
// persistent launch per direction of time: a workgroup owns 16 sequences (sequences are independent,
// so there is no inter-workgroup traffic) and walks all their steps with the hidden state resident in
// LDS.  Per step the 16 x 3H recurrent product h W_hh^T runs on the f32-input MFMA
// (v_mfma_f32_16x16x4_f32, exact fp32): a wave owns blocks of 16 hidden units and accumulates the r, z
// and n gates of the same (sequence, unit) pairs in three accumulators that share one C layout, so the
// whole gate non-linearity is lane-local -- no G_h tensor, no per-step kernel boundary.
// W_hh (<= 1.9 MB) is streamed from L2 every step as float4 B-fragments: a group of 4 MFMA k-steps
// covers 16 consecutive k, lane (j, kq) holding k = 16*kg + 4*kq + {0..3} for both operands, which
// turns both fragment fetches into 16-byte loads (ds_read_b128 for h, global_load_dwordx4 for W_hh).
// The batch is length-sorted, so the sequences alive at step j are a prefix; rows past it are masked.
//
// Default arithmetic ("bf16x6", as in gemm_split.hip): W_hh is split ONCE per launch into three bf16 planes
// (k-padded to a multiple of 32), h / dGh are split into planes in LDS as they are produced, and every 16x16x32
// product runs as the six leading term pairs on v_mfma_f32_16x16x32_bf16 with fp32 accumulation -- fp32-class
// results at 2.7x the f32-input MFMA rate (the recurrence was matrix-pipe bound: 13 unit blocks x 156 f32 MFMAs
// per step on 4 SIMDs).  RENET_GEMM=f32 selects the exact-fp32 kernels (v_mfma_f32_16x16x4_f32).
//
// The split is also an entry point of its own (renet_gru_split_weights) with recurrence entries that trust the slots
// (renet_gru_{fwd,bwd}_layouts_presplit): the training step issues it early on its side stream (csrc/step.cpp).
//
// Sources: this file is the host front (layout validation, workspace, choice of the recurrence, the exported entry points);
// the kernels live with their launchers in gru_f32.hip (exact fp32), gru_planes.hip (persistent, bf16 planes) and
// gru_steps.hip (one launch per time step, RENET_GRU=steps); gru_common.h holds what they share.
#include "gru_common.h"

namespace {

bool use_f32() {                        // RENET_GEMM=f32: exact-fp32 products everywhere (gemm.hip too)
    static const bool v = renet_env_is("RENET_GEMM", "f32");
    return v;
}

// Which bf16x6 recurrence runs.  Measured on MI355X (merged step, 2 x 2048 sequences; profiles/r02_gru_steps.md):
//   H = 200: persistent 189 / 167 us (fwd / bwd) per launch;  step kernels 10 x 20.8 / 10 x 28.3 us
//   H = 400, L = 15: persistent 858 us average;                step kernels 814 us
// The step kernels cut the W_hh stream 4x, but a launch whose workgroups all load, multiply and store in lockstep
// leaves the memory system idle during the MFMA phase and the matrix pipe idle during the epilogue (the epilogue
// alone -- Gi in, saved / h / planes out, 46 B per element and step -- is 12.6 us of a 20.8 us forward step),
// while the persistent workgroups drift apart and overlap the two.  With the W_hh stream of the persistent workgroups
// de-synchronised (rot_k / rot_u in the kernels: 188 -> 142 us at H = 200, 858 -> ~790 us at H = 400) the persistent
// kernels are the default everywhere; RENET_GRU=steps selects the per-step launches.
// (Read per launch, unlike every other switch: tests/test_gpu_parity.py runs both structures in ONE process.)
bool use_persistent() { return !renet_env_is("RENET_GRU", "steps"); }

bool fill_offsets(const int32_t* step_off, int L, StepOff& so, int& B) {
    if (L < 1 || L > MAXL || !step_off) return false;
    for (int j = 0; j <= L; ++j) so.off[j] = step_off[j];
    for (int j = L + 1; j <= MAXL; ++j) so.off[j] = step_off[L];
    B = step_off[1] - step_off[0];
    for (int j = 1; j < L; ++j)                                   // batch sizes must be non-increasing
        if (step_off[j + 1] - step_off[j] > step_off[j] - step_off[j - 1]) return false;
    return B >= 0;
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline int nub(int H) { return (H + 15) / 16; }
inline size_t fwd_plane_bytes(int H) { return (size_t)nub(H) * ((H + 31) / 32) * 9 * 1024; }          // 1 KB chunks
inline size_t bwd_t_bytes(int H) { return align256((size_t)3 * H * H * sizeof(float)); }
inline size_t bwd_plane_bytes(int H) { return (size_t)nub(H) * ((3 * H + 31) / 32) * 3 * 1024; }

// per GRU: forward = the bf16 planes of W_hh; backward = those of W_hh^T (bf16x6) or W_hh^T in fp32 (RENET_GEMM=f32)
size_t slice_bytes(int B, int H) {
    size_t m = fwd_plane_bytes(H);
    if (bwd_t_bytes(H) > m) m = bwd_t_bytes(H);
    if (bwd_plane_bytes(H) > m) m = bwd_plane_bytes(H);
    m = align256(m);
    if (B > 0) {                        // step kernels: A-operand planes (ping-pong, sized for K = 3H) + dh
        const size_t rp = (size_t)rows_pad_of(B);
        m += align256((size_t)2 * 3 * rp * kp_of(3 * H) * sizeof(__bf16)) + align256(rp * H * sizeof(float));
    }
    return m;
}

// Groups the n (1 .. MAXP) problems by packed layout (equal step_off POINTERS = same layout) and validates each layout.
// rows_in[k]: forward = rows of h_last of problem k, backward = ignored (B of the layout is used).
int make_layouts(int n, const int32_t* const* step_off, const int* Ls, const int* rows_in, bool fwd, Layouts& ly,
                 int* B_of) {
    if (n < 1 || n > MAXP) return RENET_ERR_BADARG;
    const int32_t* seen[MAXLAY] = {nullptr, nullptr};
    int nl = 0;
    for (int i = 0; i < MAXLAY; ++i) {
        ly.L[i] = 0; ly.rows[i] = 0;
        for (int j = 0; j <= MAXL; ++j) ly.so[i].off[j] = 0;
    }
    for (int k = 0; k < MAXP; ++k) ly.lay_of[k] = 0;
    static const int rot_mod = renet_env_int("RENET_GRU_ROT", 0, 0, 0x7fffffff);
    ly.rot_mod = rot_mod;
    for (int k = 0; k < n; ++k) {
        int l = -1;
        for (int i = 0; i < nl; ++i)
            if (seen[i] == step_off[k] && ly.L[i] == Ls[k]) l = i;
        if (l < 0) {
            if (nl == MAXLAY) return RENET_ERR_BADARG;
            l = nl++;
            seen[l] = step_off[k];
            ly.L[l] = Ls[k];
            int B = 0;
            if (Ls[k] > 0 && !fill_offsets(step_off[k], Ls[k], ly.so[l], B)) return RENET_ERR_BADARG;
            ly.rows[l] = fwd ? 0 : B;
        }
        const int B = ly.L[l] > 0 ? ly.so[l].off[1] - ly.so[l].off[0] : 0;
        if (fwd) {
            if (rows_in[k] < B) return RENET_ERR_BADARG;
            if (ly.rows[l] != 0 && ly.rows[l] != rows_in[k]) return RENET_ERR_BADARG;   // one h_last height per layout
            ly.rows[l] = rows_in[k];
        }
        ly.lay_of[k] = l;
        B_of[k] = B;
    }
    return RENET_OK;
}

// state region of problem k inside its workspace slice (behind the weight planes)
StepState carve_state(char* slice, int H, int Bmax, size_t kp) {
    StepState t;
    const size_t rp = (size_t)rows_pad_of(Bmax);
    char* base = slice + align256(slice_bytes(0, H));
    t.plane_stride = rp * kp;
    t.A[0] = reinterpret_cast<__bf16*>(base);
    t.A[1] = t.A[0] + 3 * t.plane_stride;
    t.dh = reinterpret_cast<float*>(base + align256((size_t)2 * 3 * rp * kp_of(3 * H) * sizeof(__bf16)));
    return t;
}

// W_hh planes are split once per DISTINCT weight pointer (the subject and object passes share the encoders)
int plane_slot(int k, const float* const* W) {
    for (int i = 0; i < k; ++i)
        if (W[i] == W[k]) return i;
    return k;
}

// the two fragment-ordered splits of W_hh [3H, H] (the recurrences and renet_gru_split_weights issue the same launches)
int split_fwd(const float* W, int H, void* planes, hipStream_t st, int npl) {
    return renet_gru_split_frag(W, H, H, 3, (size_t)H * H, (size_t)H, 1, planes, st, npl);
}
int split_bwd(const float* W, int H, void* planes, hipStream_t st, int npl) {
    return renet_gru_split_frag(W, H, 3 * H, 1, 0, 1, (size_t)H, planes, st, npl);
}

// whether the recurrence of arithmetic npl reads bf16 planes from workspace slots whose place does not depend on the batch:
// not the exact-fp32 kernels (no planes), not the step kernels (their slices carry per-batch state)
bool planes_in_fixed_slots(int npl) { return npl == 3 && !use_f32() && use_persistent(); }

int max_batch(int n, const int* B_of) {
    int Bmax = 0;
    for (int k = 0; k < n; ++k) Bmax = B_of[k] > Bmax ? B_of[k] : Bmax;
    return Bmax;
}

// npl: 3 = bf16x6 (the exact-fp32 kernels in a RENET_GEMM=f32 process), 1 = bf16 mode, 0 = the exact-fp32 kernels asked
// for by the caller (per model)
int gru_fwd_impl(int npl, int n, const float* const* Gi, const int32_t* const* step_off, const int* L, int H,
                 const float* const* Whh, const float* const* bhh, float* const* h_last, const int* out_rows,
                 float* const* saved, float* workspace, size_t workspace_bytes, void* stream, bool presplit = false) {
    Layouts ly;
    int B_of[MAXP];
    if (presplit && !planes_in_fixed_slots(npl)) return RENET_ERR_UNSUPPORTED;
    const int e0 = make_layouts(n, step_off, L, out_rows, true, ly, B_of);
    if (e0 != RENET_OK) return e0;
    if (max_rows(ly) == 0) return RENET_OK;
    if (!renet_dim_ok(H) || (npl == 1 && H == 300)) return RENET_ERR_UNSUPPORTED;   // (no bf16 storage mode at 300)
    hipStream_t st = (hipStream_t)stream;
    if (npl == 0 || (use_f32() && npl == 3)) {
        FwdProbs ps;
        for (int i = 0; i < MAXP; ++i) {
            const int k = i < n ? i : 0;
            ps.p[i] = {Gi[k], Whh[k], bhh[k], h_last[k], saved[k]};
        }
        return renet_gru_f32_fwd(H, &ps, n, &ly, st);
    }
    const bool steps = npl == 3 && !use_persistent();
    const int Bmax = max_batch(n, B_of);
    const size_t per = slice_bytes(steps ? Bmax : 0, H);
    if (!workspace || workspace_bytes < (size_t)n * per) return RENET_ERR_WORKSPACE;
    char* ws = reinterpret_cast<char*>(workspace);
    FwdProbsB ps;
    for (int i = 0; i < MAXP; ++i) {
        const int k = i < n ? i : 0;
        const int slot = plane_slot(k, Whh);
        bf16x8* planes = reinterpret_cast<bf16x8*>(ws + (size_t)slot * per);
        if (i < n && slot == k && !presplit) {      // gate g of unit u, input k: W_hh[g*H + u][k]
            const int e = split_fwd(Whh[k], H, planes, st, npl);
            if (e != RENET_OK) return e;
        }
        ps.p[i] = {Gi[k], planes, bhh[k], h_last[k], saved[k]};
    }
    if (steps) {
        StepState stt[MAXP];
        for (int i = 0; i < n; ++i) stt[i] = carve_state(ws + (size_t)i * per, H, Bmax, kp_of(H));
        return renet_gru_steps_fwd(H, n, &ps, &ly, stt, Bmax, st);
    }
    return renet_gru_planes_fwd(H, npl, &ps, n, &ly, st);
}

// out_ld > 0 (npl = 1 only): dGi / dGh are bf16 matrices of that row stride; bounds: per problem, one max |dGi| per workgroup
int gru_bwd_impl(int npl, int n, const float* const* dh_last, const int32_t* const* step_off, const int* L, int H,
                 const float* const* Whh, const float* const* saved, float* const* dGi, float* const* dGh,
                 float* workspace, size_t workspace_bytes, void* stream, int out_ld = 0,
                 float* const* bounds = nullptr, bool presplit = false) {
    Layouts ly;
    int B_of[MAXP];
    if (presplit && !planes_in_fixed_slots(npl)) return RENET_ERR_UNSUPPORTED;
    const int e0 = make_layouts(n, step_off, L, nullptr, false, ly, B_of);
    if (e0 != RENET_OK) return e0;
    if (max_rows(ly) == 0) return RENET_OK;
    if (!renet_dim_ok(H) || (npl == 1 && H == 300)) return RENET_ERR_UNSUPPORTED;   // (no bf16 storage mode at 300)
    hipStream_t st = (hipStream_t)stream;
    const bool f32 = npl == 0 || (use_f32() && npl == 3);
    const bool steps = npl == 3 && !f32 && !use_persistent();
    if (bounds && (f32 || steps || npl != 3)) return RENET_ERR_UNSUPPORTED;   // only the persistent bf16x6 kernel emits them
    const int Bmax = max_batch(n, B_of);
    const size_t per = slice_bytes(steps ? Bmax : 0, H);
    if (!workspace || workspace_bytes < (size_t)n * per) return RENET_ERR_WORKSPACE;
    char* ws = reinterpret_cast<char*>(workspace);
    char* wt[MAXP];                                 // W_hh^T of each problem: fp32, or bf16 planes
    for (int i = 0; i < MAXP; ++i) {
        const int k = i < n ? i : 0;
        const int slot = plane_slot(k, Whh);
        wt[i] = ws + (size_t)slot * per;
        if (i < n && slot == k && !presplit) {      // W_hh^T: unit u = hidden unit, k = gate column c: W_hh[c][u]
            const int e = f32 ? renet_gru_transpose(Whh[k], 3 * H, H, reinterpret_cast<float*>(wt[i]), st)
                              : split_bwd(Whh[k], H, wt[i], st, npl);
            if (e != RENET_OK) return e;
        }
    }
    if (f32) {
        BwdProbs ps;
        for (int i = 0; i < MAXP; ++i) {
            const int k = i < n ? i : 0;
            ps.p[i] = {dh_last[k], reinterpret_cast<float*>(wt[i]), saved[k], dGi[k], dGh[k]};
        }
        return renet_gru_f32_bwd(H, &ps, n, &ly, st);
    }
    BwdProbsB pb;
    for (int i = 0; i < MAXP; ++i) {
        const int k = i < n ? i : 0;
        pb.p[i] = {dh_last[k], reinterpret_cast<bf16x8*>(wt[i]), saved[k], dGi[k], dGh[k], out_ld, bounds ? bounds[k] : nullptr};
    }
    if (steps) {
        StepState stt[MAXP];
        for (int i = 0; i < n; ++i) stt[i] = carve_state(ws + (size_t)i * per, H, Bmax, kp_of(3 * H));
        return renet_gru_steps_bwd(H, n, &pb, &ly, stt, B_of, Bmax, st);
    }
    return renet_gru_planes_bwd(H, npl, out_ld > 0, &pb, n, &ly, st);
}

}  // namespace

extern "C" {

size_t renet_gru_workspace(int B, int H) { return slice_bytes(B, H); }

// the entry points of one direction differ in the arithmetic they ask for (npl of the implementations) only
#define GRU_FWD_PARAMS                                                                                                \
    int n, const float* const* Gi, const int32_t* const* step_off, const int* L, int H, const float* const* Whh,      \
    const float* const* bhh, float* const* h_last, const int* out_rows, float* const* saved, float* workspace,        \
    size_t workspace_bytes, void* stream
#define GRU_FWD_ARGS n, Gi, step_off, L, H, Whh, bhh, h_last, out_rows, saved, workspace, workspace_bytes, stream
int renet_gru_fwd_layouts(GRU_FWD_PARAMS) { return gru_fwd_impl(3, GRU_FWD_ARGS); }
int renet_gru_fwd_layouts_f32(GRU_FWD_PARAMS) { return gru_fwd_impl(0, GRU_FWD_ARGS); }
int renet_gru_fwd_layouts_bf16(GRU_FWD_PARAMS) { return gru_fwd_impl(1, GRU_FWD_ARGS); }

#define GRU_BWD_PARAMS                                                                                                \
    int n, const float* const* dh_last, const int32_t* const* step_off, const int* L, int H, const float* const* Whh, \
    const float* const* saved, float* const* dGi, float* const* dGh, float* workspace, size_t workspace_bytes,        \
    void* stream
#define GRU_BWD_ARGS n, dh_last, step_off, L, H, Whh, saved, dGi, dGh, workspace, workspace_bytes, stream
int renet_gru_bwd_layouts(GRU_BWD_PARAMS) { return gru_bwd_impl(3, GRU_BWD_ARGS); }
int renet_gru_bwd_layouts_f32(GRU_BWD_PARAMS) { return gru_bwd_impl(0, GRU_BWD_ARGS); }
int renet_gru_bwd_layouts_bf16(GRU_BWD_PARAMS) { return gru_bwd_impl(1, GRU_BWD_ARGS); }

int renet_gru_fwd_layouts_presplit(GRU_FWD_PARAMS) { return gru_fwd_impl(3, GRU_FWD_ARGS, true); }
int renet_gru_bwd_layouts_presplit(GRU_BWD_PARAMS) { return gru_bwd_impl(3, GRU_BWD_ARGS, 0, nullptr, true); }

int renet_gru_split_weights(int n, const float* const* Whh, int H, int backward, float* workspace, size_t workspace_bytes,
                            void* stream) {
    if (n < 1 || n > MAXP || !Whh) return RENET_ERR_BADARG;
    for (int k = 0; k < n; ++k)
        if (!Whh[k]) return RENET_ERR_BADARG;
    if (!renet_dim_ok(H) || !planes_in_fixed_slots(3)) return RENET_ERR_UNSUPPORTED;
    const size_t per = slice_bytes(0, H);
    if (!workspace || workspace_bytes < (size_t)n * per) return RENET_ERR_WORKSPACE;
    char* ws = reinterpret_cast<char*>(workspace);
    for (int k = 0; k < n; ++k) {
        if (plane_slot(k, Whh) != k) continue;
        const int e = backward ? split_bwd(Whh[k], H, ws + (size_t)k * per, (hipStream_t)stream, 3)
                               : split_fwd(Whh[k], H, ws + (size_t)k * per, (hipStream_t)stream, 3);
        if (e != RENET_OK) return e;
    }
    return RENET_OK;
}

int renet_gru_bound_parts(int max_rows) { return max(1, (max_rows + MT - 1) / MT); }

int renet_gru_bwd_layouts_bounds(int n, const float* const* dh_last, const int32_t* const* step_off, const int* L, int H,
                                 const float* const* Whh, const float* const* saved, float* const* dGi,
                                 float* const* dGh, float* const* bounds, float* workspace, size_t workspace_bytes,
                                 void* stream) {
    if (!bounds) return RENET_ERR_BADARG;
    return gru_bwd_impl(3, n, dh_last, step_off, L, H, Whh, saved, dGi, dGh, workspace, workspace_bytes, stream, 0,
                        bounds);
}

int renet_gru_bwd_layouts_bf16out(int n, const float* const* dh_last, const int32_t* const* step_off, const int* L,
                                  int H, const float* const* Whh, const float* const* saved, void* const* dGi16,
                                  void* const* dGh16, int out_ld, float* workspace, size_t workspace_bytes,
                                  void* stream) {
    if (out_ld < 3 * H) return RENET_ERR_BADARG;
    return gru_bwd_impl(1, n, dh_last, step_off, L, H, Whh, saved, reinterpret_cast<float* const*>(dGi16),
                        reinterpret_cast<float* const*>(dGh16), workspace, workspace_bytes, stream, out_ld);
}

// n (<= 4) GRUs over ONE packed layout
int renet_gru_fwd_multi(int n, const float* const* Gi, const int32_t* step_off, int L, int H,
                        const float* const* Whh, const float* const* bhh, float* const* h_last, int out_rows,
                        float* const* saved, float* workspace, size_t workspace_bytes, void* stream) {
    if (n < 1 || n > MAXP) return RENET_ERR_BADARG;
    const int32_t* so[MAXP];
    int Ls[MAXP], rows[MAXP];
    for (int k = 0; k < n; ++k) { so[k] = step_off; Ls[k] = L; rows[k] = out_rows; }
    return renet_gru_fwd_layouts(n, Gi, so, Ls, H, Whh, bhh, h_last, rows, saved, workspace, workspace_bytes, stream);
}

int renet_gru_fwd(const float* Gi, const int32_t* step_off, int L, int H, const float* Whh,
                  const float* bhh, float* h_last, int out_rows, float* saved, float* workspace,
                  size_t workspace_bytes, void* stream) {
    return renet_gru_fwd_multi(1, &Gi, step_off, L, H, &Whh, &bhh, &h_last, out_rows, &saved, workspace,
                               workspace_bytes, stream);
}

int renet_gru_bwd_multi(int n, const float* const* dh_last, const int32_t* step_off, int L, int H,
                        const float* const* Whh, const float* const* saved, float* const* dGi,
                        float* const* dGh, float* workspace, size_t workspace_bytes, void* stream) {
    if (n < 1 || n > MAXP) return RENET_ERR_BADARG;
    const int32_t* so[MAXP];
    int Ls[MAXP];
    for (int k = 0; k < n; ++k) { so[k] = step_off; Ls[k] = L; }
    return renet_gru_bwd_layouts(n, dh_last, so, Ls, H, Whh, saved, dGi, dGh, workspace, workspace_bytes, stream);
}

int renet_gru_bwd(const float* dh_last, const int32_t* step_off, int L, int H, const float* Whh,
                  const float* saved, float* dGi, float* dGh, float* workspace,
                  size_t workspace_bytes, void* stream) {
    return renet_gru_bwd_multi(1, &dh_last, step_off, L, H, &Whh, &saved, &dGi, &dGh, workspace,
                               workspace_bytes, stream);
}

}  // extern "C"
