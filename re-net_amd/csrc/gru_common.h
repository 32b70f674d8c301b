// What the GRU kernel families share (gru_f32.hip, gru_planes.hip, gru_steps.hip) and what the host front (gru.hip) hands
// them: the workgroup geometry, the packed-layout argument, the per-problem argument packs, the bf16 plane split and its
// MFMA products, and the launchers each family exports to the front.  Everything but those launchers sits in the anonymous
// namespace of the including translation unit (device helpers are inlined; every family keeps its own kernels).
#ifndef RENET_GRU_COMMON_H
#define RENET_GRU_COMMON_H
#include <type_traits>
#include <utility>
#include "common.h"

// ---- the families' launchers (library-internal) ----------------------------------------------------------------------
// The argument packs are kernel parameter types of the anonymous namespace, and a function whose signature names such a
// type cannot be defined in another translation unit: packs, layouts and step states cross as const void* (read back
// with as<T>).  H is 100, 200, 300 or 400 (the front has answered RENET_ERR_UNSUPPORTED for anything else).
#define RENET_GRU_HIDDEN __attribute__((visibility("hidden")))
// gru_f32.hip: the exact-fp32 recurrences (probs: FwdProbs / BwdProbs), and W_hh [rows, cols] -> W_hh^T
RENET_GRU_HIDDEN int renet_gru_f32_fwd(int H, const void* probs, int np, const void* layouts, hipStream_t st);
RENET_GRU_HIDDEN int renet_gru_f32_bwd(int H, const void* probs, int np, const void* layouts, hipStream_t st);
RENET_GRU_HIDDEN int renet_gru_transpose(const float* in, int rows, int cols, float* out, hipStream_t st);
// gru_planes.hip: W -> bf16 planes in fragment order (split_frag_kernel; out: bf16x8), and the persistent recurrences on
// them (probs: FwdProbsB / BwdProbsB): npl = 3 (bf16x6) | 1 (bf16 mode); out16: dGi / dGh written as bf16 (npl = 1 only)
RENET_GRU_HIDDEN int renet_gru_split_frag(const float* in, int U, int K, int G, size_t sg, size_t su, size_t sk, void* out,
                                          hipStream_t st, int npl);
RENET_GRU_HIDDEN int renet_gru_planes_fwd(int H, int npl, const void* probs, int np, const void* layouts, hipStream_t st);
RENET_GRU_HIDDEN int renet_gru_planes_bwd(int H, int npl, bool out16, const void* probs, int np, const void* layouts,
                                          hipStream_t st);
// gru_steps.hip: the per-step launches of the bf16x6 recurrence over the first n problems of a FwdProbsB / BwdProbsB;
// states: StepState[n], carved by the front
RENET_GRU_HIDDEN int renet_gru_steps_fwd(int H, int n, const void* probs, const void* layouts, const void* states, int Bmax,
                                         hipStream_t st);
RENET_GRU_HIDDEN int renet_gru_steps_bwd(int H, int n, const void* probs, const void* layouts, const void* states,
                                         const int* B_of, int Bmax, hipStream_t st);

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int MT = 16;           // sequences per workgroup (MFMA M)
#ifndef RENET_GRU_NW
#define RENET_GRU_NW 8
#endif
constexpr int NW = RENET_GRU_NW; // waves per workgroup: 2 per SIMD so that W_hh fetch latency hides behind the partner's MFMAs
constexpr int NT = NW * 64;
constexpr int MAXL = 32;         // max packed steps (seq_len is 10 / 15 in the reference configs)

struct StepOff { int off[MAXL + 1]; };

// Up to MAXP independent GRUs run in ONE launch (blockIdx.y selects the problem); they may belong to up to MAXLAY
// different packed layouts: RE-Net's `encoder` and `encoder_r` consume the same batch (model.py:86,94), and the
// subject and object passes of a training step (train.py:136-137) are independent until their losses are added, so
// a step can run all four recurrences -- each only ~60 workgroups -- side by side on the 256 CUs.
constexpr int MAXP = 4, MAXLAY = 2;
struct Layouts {
    StepOff so[MAXLAY];
    int L[MAXLAY];
    int rows[MAXLAY];           // forward: rows of h_last (>= B); backward: B
    int lay_of[MAXP];
    int rot_mod;                // backward: number of distinct starting k groups of the W stream (0 = default; RENET_GRU_ROT)
};

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + __expf(-x)); }

template <int H>
struct Cfg {
    static constexpr int NUB = (H + 15) / 16;          // blocks of 16 hidden units
    static constexpr int KG = (H + 15) / 16;           // groups of 16 k over K = H
    static constexpr int LDH = NUB * 16 + 4;           // LDS row stride of the h / dh tile (16 B aligned)
    static constexpr int K3 = 3 * H;
    static constexpr int KG3 = (K3 + 15) / 16;         // groups of 16 k over K = 3H (backward)
    static constexpr int LDG = KG3 * 16 + 4;
};

template <int H>
struct BCfg {
    static constexpr int KG = (H + 31) / 32;           // groups of 32 k over K = H (forward)
    static constexpr int KP = KG * 32;                 // padded K of the W_hh planes
    static constexpr int LDP = KP + 8;                 // bf16 row stride of the h planes in LDS (16 B aligned)
    static constexpr int KG3 = (3 * H + 31) / 32;      // K = 3H (backward)
    static constexpr int KP3 = KG3 * 32;
    static constexpr int LDP3 = KP3 + 8;
};

// ---- per-problem argument packs -------------------------------------------------------------------------------------
// exact fp32 (gru_f32.hip)
struct FwdProb { const float* Gi; const float* Whh; const float* bhh; float* h_last; float* saved; };
struct FwdProbs { FwdProb p[MAXP]; };
struct BwdProb { const float* dh_last; const float* WhhT; const float* saved; float* dGi; float* dGh; };
struct BwdProbs { BwdProb p[MAXP]; };
// bf16 planes (gru_planes.hip; gru_steps.hip builds its per-step packs from them)
struct FwdProbB { const float* Gi; const bf16x8* Wp; const float* bhh; float* h_last; float* saved; };
struct FwdProbsB { FwdProbB p[MAXP]; };
struct BwdProbB { const float* dh_last; const bf16x8* WTp; const float* saved; float* dGi; float* dGh; int out_ld;
                  float* bound; /* optional: bound[blockIdx.x] = this workgroup's max |dGi| (f16x3 GEMM operand bound) */ };
struct BwdProbsB { BwdProbB p[MAXP]; };

// step kernels: state of one problem in its workspace slice (carve_state, gru.hip): bf16 plane ping-pong of the A operand + fp32 dh
struct StepState {
    __bf16* A[2];
    float* dh;
    size_t plane_stride;                // elements between two planes of one buffer
};
constexpr int SR = 64;                  // sequences per workgroup of the step kernels: 4 MFMA row tiles
inline int rows_pad_of(int rows) { return (rows + SR - 1) / SR * SR; }
inline size_t kp_of(int K) { return (size_t)((K + 31) / 32) * 32; }

// ---- bf16 planes ----------------------------------------------------------------------------------------------------
struct Planes3 { __bf16 p[3]; };

// x = p0 + p1 + p2 (round-to-nearest terms, as gemm_split.hip)
__device__ __forceinline__ Planes3 split3(float x) {
    Planes3 r;
    r.p[0] = (__bf16)x;
    const float r1 = x - (float)r.p[0];
    r.p[1] = (__bf16)r1;
    r.p[2] = (__bf16)(r1 - (float)r.p[1]);
    return r;
}

// six leading term pairs of a (16 x 32) x (32 x 16) product, smallest first
__device__ __forceinline__ f32x4 mfma6(const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[0], acc, 0, 0, 0);
    return acc;
}

// NPL = 3: the six leading term pairs (fp32-class); NPL = 1: ONE bf16 product (bf16 mode, BASELINE config 5)
template <int NPL>
__device__ __forceinline__ f32x4 mfma_p(const bf16x8 (&a)[NPL], const bf16x8 (&b)[NPL], f32x4 acc) {
    if constexpr (NPL == 3) return mfma6(a, b, acc);
    else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[0], acc, 0, 0, 0);
}

// ---- host helpers of the launchers ------------------------------------------------------------------------------------
template <class T>
const T& as(const void* p) { return *static_cast<const T*>(p); }
// the run-time H as a template argument: f(std::integral_constant<int, H>{}) for the supported widths
template <class F>
int with_h(int H, F&& f) {
    switch (H) {
        case 100: return f(std::integral_constant<int, 100>{});
        case 200: return f(std::integral_constant<int, 200>{});
        case 300: return f(std::integral_constant<int, 300>{});
        case 400: return f(std::integral_constant<int, 400>{});
        default: return RENET_ERR_UNSUPPORTED;
    }
}

template <class KernelT>
int set_lds(KernelT kernel, size_t lds, bool& done) {
    if (!done && lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    done = true;                       // benign race: the attribute is idempotent
    return RENET_OK;
}

inline int max_rows(const Layouts& ly) { return ly.rows[0] > ly.rows[1] ? ly.rows[0] : ly.rows[1]; }

}  // namespace

#endif  // RENET_GRU_COMMON_H
