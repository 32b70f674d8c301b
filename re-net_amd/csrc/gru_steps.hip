// Step kernels (RENET_GRU=steps; the persistent kernels of gru_planes.hip are the default): the bf16x6 recurrence as ONE
// launch per time step, GEMM-shaped tiles.  Measured against the persistent kernels in profiles/r02_gru_steps.md.
//
// The persistent kernels give a workgroup 16 sequences and ALL hidden units, so every workgroup re-streams
// the whole of W_hh (0.8 MB of planes at H = 200, 3 MB at H = 400) from L2 every step: 213 MB of L2 -> L1 traffic per
// step at H = 200 with 256 workgroups, and the 64 B/clk L1 fill rate of a CU -- not the matrix pipe -- bounds the step
// (PMC: r02 DESIGN 4).  Here a workgroup owns 64 sequences x 64 hidden units (4 waves, one block of 16 units each,
// 4 MFMA row tiles per wave): a W fragment is used for 4 row tiles, the A operand (bf16 planes of h, or of dGh in the
// backward pass) is staged through LDS in double-buffered chunks of 128 k and shared by the 4 waves, and the state
// travels between steps through L2 (fp32 h / dh in place, bf16 planes ping-pong) -- the kernel boundary is the
// grid-wide barrier the step needs.  W traffic per step drops 4x (16x per sequence tile), the step becomes
// matrix-pipe / epilogue-traffic bound, and later steps launch only the row tiles that are still alive.
// The epilogue is the gate math on the MFMA C layout exactly as in the persistent kernels; backward launch j forms dh(j-1) and, in the
// same epilogue, the gate gradients of step j-1 (they need dh(j-1) at the lane's own (sequence, unit) pairs only).
#include "gru_common.h"

namespace {

constexpr int SRT = SR / 16;
constexpr int SW = 4;                           // waves per workgroup, one block of 16 hidden units each
constexpr int SNT = SW * 64;
constexpr int CKG = 4;                          // k groups (32 k each) per LDS chunk
constexpr int CK = CKG * 32;
constexpr int LDC = CK + 8;                     // bf16 row stride of a chunk in LDS (ds_read_b128 conflict free)
constexpr int CHUNK_ELEMS = 3 * SR * LDC;       // one chunk buffer: three planes
constexpr int STAGE_V = 3 * SR * (CK / 8) / SNT;        // 16-byte vectors per thread and chunk (12)
constexpr size_t STEP_LDS = (size_t)2 * CHUNK_ELEMS * sizeof(__bf16);

struct StageRegs { uint4 v[STAGE_V]; };

// A operand in global memory: [3][rows_pad][KPg] bf16 planes, rows_pad a multiple of SR, k padding zero
template <int KPg>
__device__ __forceinline__ void stage_load(const __bf16* __restrict__ A, size_t plane_stride, int r0, int kbase, int tid,
                                           StageRegs& s) {
#pragma unroll
    for (int q = 0; q < STAGE_V; ++q) {
        const int idx = tid + SNT * q;
        const int plane = idx / (SR * (CK / 8));
        const int rem = idx - plane * (SR * (CK / 8));
        const int row = rem / (CK / 8), seg = rem - row * (CK / 8);
        const int k = kbase + seg * 8;
        const uint4 v = *reinterpret_cast<const uint4*>(A + plane * plane_stride + (size_t)(r0 + row) * KPg + (k < KPg ? k : 0));
        s.v[q] = k < KPg ? v : make_uint4(0u, 0u, 0u, 0u);
    }
}

__device__ __forceinline__ void stage_store(__bf16* __restrict__ buf, int tid, const StageRegs& s) {
#pragma unroll
    for (int q = 0; q < STAGE_V; ++q) {
        const int idx = tid + SNT * q;
        const int plane = idx / (SR * (CK / 8));
        const int rem = idx - plane * (SR * (CK / 8));
        const int row = rem / (CK / 8), seg = rem - row * (CK / 8);
        *reinterpret_cast<uint4*>(buf + plane * (SR * LDC) + row * LDC + seg * 8) = s.v[q];
    }
}

// LDS-only barrier: the global loads that prefetch the next chunk / the next W fragments stay in flight across it
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
}

struct StepF {
    const float* Gi; const bf16x8* Wp; const float* bhh; float* h; float* saved;
    const __bf16* Ain; __bf16* Aout;
    int p0, bs;                         // packed row of sequence 0 at this step, sequences alive at this step
    size_t plane_stride;
};
struct StepsF { StepF p[MAXP]; };

template <int H, bool GEMM>
__global__ __launch_bounds__(SNT) void gru_step_fwd_kernel(StepsF ps) {
    using C = Cfg<H>;
    using Bc = BCfg<H>;
    const StepF& P = ps.p[blockIdx.z];
    const int r0 = blockIdx.x * SR;
    if (r0 >= P.bs) return;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __bf16* bufs = reinterpret_cast<__bf16*>(smem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ub = blockIdx.y * SW + wave;
    const bool wave_on = ub < C::NUB;                                   // wave-uniform
    const int jj = lane & 15, kq = lane >> 4, ai = lane & 15;
    const int u = ub * 16 + jj;
    const bool uok = wave_on && u < H;
    const int uc = uok ? u : 0;
    const int bs = P.bs;

    // operands of the epilogue, requested before the matrix work (unconditional loads from clamped rows)
    float gr[SRT][4], gz[SRT][4], gn[SRT][4], hp[SRT][4];
#pragma unroll
    for (int t = 0; t < SRT; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int row = min(r0 + 16 * t + 4 * kq + reg, bs - 1);
            const float* gi = P.Gi + (size_t)(P.p0 + row) * C::K3 + uc;
            gr[t][reg] = gi[0]; gz[t][reg] = gi[H]; gn[t][reg] = gi[2 * H];
            hp[t][reg] = GEMM ? P.h[(size_t)row * H + uc] : 0.f;
        }
    const float b_r = P.bhh[uc], b_z = P.bhh[H + uc], b_n = P.bhh[2 * H + uc];

    f32x4 ar[SRT], az[SRT], an[SRT];
#pragma unroll
    for (int t = 0; t < SRT; ++t) { ar[t] = {0.f, 0.f, 0.f, 0.f}; az[t] = ar[t]; an[t] = ar[t]; }

    if constexpr (GEMM) {
        constexpr int NC = (Bc::KG + CKG - 1) / CKG;
        const bf16x8* wf = P.Wp + (size_t)(wave_on ? ub : 0) * Bc::KG * 9 * 64 + lane;      // fragment order
        bf16x8 wcur[3][3], wnext[3][3];                                   // [gate][plane]
#pragma unroll
        for (int f = 0; f < 9; ++f) wcur[f / 3][f % 3] = wf[f * 64];
        StageRegs sr;
        stage_load<Bc::KP>(P.Ain, P.plane_stride, r0, 0, tid, sr);
        stage_store(bufs, tid, sr);
        if (NC > 1) stage_load<Bc::KP>(P.Ain, P.plane_stride, r0, CK, tid, sr);
        lds_barrier();
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const __bf16* cur = bufs + (c & 1) * CHUNK_ELEMS;
            if (c + 1 < NC) {
                stage_store(bufs + ((c + 1) & 1) * CHUNK_ELEMS, tid, sr);
                if (c + 2 < NC) stage_load<Bc::KP>(P.Ain, P.plane_stride, r0, (c + 2) * CK, tid, sr);
            }
            if (wave_on) {
                const __bf16* ha = cur + ai * LDC + kq * 8;
#pragma unroll
                for (int kk = 0; kk < CKG; ++kk) {
                    const int kg = c * CKG + kk;
                    if (kg < Bc::KG) {
                        if (kg + 1 < Bc::KG) {
#pragma unroll
                            for (int f = 0; f < 9; ++f) wnext[f / 3][f % 3] = wf[((kg + 1) * 9 + f) * 64];
                        }
#pragma unroll
                        for (int t = 0; t < SRT; ++t) {
                            bf16x8 a[3];
#pragma unroll
                            for (int p = 0; p < 3; ++p)
                                a[p] = *reinterpret_cast<const bf16x8*>(ha + p * (SR * LDC) + t * 16 * LDC + kk * 32);
                            ar[t] = mfma6(a, wcur[0], ar[t]);
                            az[t] = mfma6(a, wcur[1], az[t]);
                            an[t] = mfma6(a, wcur[2], an[t]);
                        }
                        if (kg + 1 < Bc::KG) {
#pragma unroll
                            for (int f = 0; f < 9; ++f) wcur[f / 3][f % 3] = wnext[f / 3][f % 3];
                        }
                    }
                }
            }
            lds_barrier();
        }
    }

    if (uok) {
        // C layout: column = lane & 15 (unit u), row = 4 * (lane >> 4) + reg (sequence of the row tile)
#pragma unroll
        for (int t = 0; t < SRT; ++t)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int row = r0 + 16 * t + 4 * kq + reg;
                if (row < bs) {
                    const size_t p = (size_t)(P.p0 + row);
                    const float hn = an[t][reg] + b_n;
                    const float r = sigmoidf_(gr[t][reg] + ar[t][reg] + b_r);
                    const float z = sigmoidf_(gz[t][reg] + az[t][reg] + b_z);
                    const float n = tanhf(gn[t][reg] + r * hn);
                    const float hpv = hp[t][reg];
                    const float hv = (1.f - z) * n + z * hpv;
                    float* sv = P.saved + p * 5 * H;
                    sv[u] = r; sv[H + u] = z; sv[2 * H + u] = n; sv[3 * H + u] = hn; sv[4 * H + u] = hpv;
                    P.h[(size_t)row * H + u] = hv;
                    const Planes3 sp = split3(hv);
                    __bf16* dst = P.Aout + (size_t)row * Bc::KP + u;
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) dst[pl * P.plane_stride] = sp.p[pl];
                }
            }
    }
}

struct StepB {
    const float* saved; const bf16x8* WTp; float* dh; float* dGi; float* dGh;
    const __bf16* Ain; __bf16* Aout;
    int bs_cur;                         // sequences alive at the step whose dGh is contracted (0: none)
    int p0_prev, bs_prev;               // packed row 0 / sequences alive at the step whose gate gradients are formed
    size_t plane_stride;
};
struct StepsB { StepB p[MAXP]; };

// launch for step j:  dh(j-1) = dh(j) z(j) [already in dh] + dGh(j) W_hh  for the sequences alive at step j, then the
// gate gradients of step j-1 for the sequences alive at step j-1 (a superset: sequences whose last step is j-1 enter
// with dh = dh_last).  GEMM = false is the first launch (step L-1's gate gradients from dh_last alone).
template <int H, bool GEMM>
__global__ __launch_bounds__(SNT) void gru_step_bwd_kernel(StepsB ps) {
    using C = Cfg<H>;
    using Bc = BCfg<H>;
    const StepB& P = ps.p[blockIdx.z];
    const int r0 = blockIdx.x * SR;
    if (r0 >= P.bs_prev) return;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __bf16* bufs = reinterpret_cast<__bf16*>(smem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ub = blockIdx.y * SW + wave;
    const bool wave_on = ub < C::NUB;
    const int jj = lane & 15, kq = lane >> 4, ai = lane & 15;
    const int u = ub * 16 + jj;
    const bool uok = wave_on && u < H;
    const int uc = uok ? u : 0;
    const int bsp = P.bs_prev;

    float sv_r[SRT][4], sv_z[SRT][4], sv_n[SRT][4], sv_hn[SRT][4], sv_hp[SRT][4], gin[SRT][4];
#pragma unroll
    for (int t = 0; t < SRT; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int row = min(r0 + 16 * t + 4 * kq + reg, bsp - 1);
            const float* sv = P.saved + (size_t)(P.p0_prev + row) * 5 * H + uc;
            sv_r[t][reg] = sv[0]; sv_z[t][reg] = sv[H]; sv_n[t][reg] = sv[2 * H]; sv_hn[t][reg] = sv[3 * H];
            sv_hp[t][reg] = sv[4 * H];
            gin[t][reg] = P.dh[(size_t)row * H + uc];
        }

    f32x4 acc[SRT];
#pragma unroll
    for (int t = 0; t < SRT; ++t) acc[t] = {0.f, 0.f, 0.f, 0.f};

    if (GEMM && r0 < P.bs_cur) {                                        // workgroup-uniform
        constexpr int NC = (Bc::KG3 + CKG - 1) / CKG;
        const bf16x8* wf = P.WTp + (size_t)(wave_on ? ub : 0) * Bc::KG3 * 3 * 64 + lane;
        bf16x8 wcur[3], wnext[3];
#pragma unroll
        for (int f = 0; f < 3; ++f) wcur[f] = wf[f * 64];
        StageRegs sr;
        stage_load<Bc::KP3>(P.Ain, P.plane_stride, r0, 0, tid, sr);
        stage_store(bufs, tid, sr);
        if (NC > 1) stage_load<Bc::KP3>(P.Ain, P.plane_stride, r0, CK, tid, sr);
        lds_barrier();
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const __bf16* cur = bufs + (c & 1) * CHUNK_ELEMS;
            if (c + 1 < NC) {
                stage_store(bufs + ((c + 1) & 1) * CHUNK_ELEMS, tid, sr);
                if (c + 2 < NC) stage_load<Bc::KP3>(P.Ain, P.plane_stride, r0, (c + 2) * CK, tid, sr);
            }
            if (wave_on) {
                const __bf16* ga = cur + ai * LDC + kq * 8;
#pragma unroll
                for (int kk = 0; kk < CKG; ++kk) {
                    const int kg = c * CKG + kk;
                    if (kg < Bc::KG3) {
                        if (kg + 1 < Bc::KG3) {
#pragma unroll
                            for (int f = 0; f < 3; ++f) wnext[f] = wf[((kg + 1) * 3 + f) * 64];
                        }
#pragma unroll
                        for (int t = 0; t < SRT; ++t) {
                            bf16x8 a[3];
#pragma unroll
                            for (int p = 0; p < 3; ++p)
                                a[p] = *reinterpret_cast<const bf16x8*>(ga + p * (SR * LDC) + t * 16 * LDC + kk * 32);
                            acc[t] = mfma6(a, wcur, acc[t]);
                        }
                        if (kg + 1 < Bc::KG3) {
#pragma unroll
                            for (int f = 0; f < 3; ++f) wcur[f] = wnext[f];
                        }
                    }
                }
            }
            lds_barrier();
        }
    }

    if (uok) {
#pragma unroll
        for (int t = 0; t < SRT; ++t)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int row = r0 + 16 * t + 4 * kq + reg;
                if (row < bsp) {
                    const size_t p = (size_t)(P.p0_prev + row);
                    const float r = sv_r[t][reg], z = sv_z[t][reg], n = sv_n[t][reg], hn = sv_hn[t][reg];
                    const float hpv = sv_hp[t][reg];
                    const float g = gin[t][reg] + ((GEMM && row < P.bs_cur) ? acc[t][reg] : 0.f);
                    const float dan = g * (1.f - z) * (1.f - n * n);
                    const float daz = g * (hpv - n) * z * (1.f - z);
                    const float dar = dan * hn * r * (1.f - r);
                    float* gi = P.dGi + p * C::K3;
                    float* gh = P.dGh + p * C::K3;
                    gi[u] = dar; gi[H + u] = daz; gi[2 * H + u] = dan;
                    gh[u] = dar; gh[H + u] = daz; gh[2 * H + u] = dan * r;
                    P.dh[(size_t)row * H + u] = g * z;                  // direct path h_prev -> h
                    const Planes3 s0 = split3(dar), s1 = split3(daz), s2 = split3(dan * r);
                    __bf16* dst = P.Aout + (size_t)row * Bc::KP3 + u;
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) {
                        dst[pl * P.plane_stride] = s0.p[pl];
                        dst[pl * P.plane_stride + H] = s1.p[pl];
                        dst[pl * P.plane_stride + 2 * H] = s2.p[pl];
                    }
                }
            }
    }
}

// The launch loop of both directions: launch s handles one time step of every problem that has one (forward: step s,
// backward: step L-1-s).  fill(P, offsets, L, s) sets the per-step fields of problem P and returns its row count.
template <auto First, auto Rest, int NUB, class Pack, class Fill>
int run_steps(int n, const Layouts& ly, const Pack& base, const StepState* stt, hipStream_t st, Fill fill) {
    static bool a0 = false, a1 = false;
    int e = set_lds(First, STEP_LDS, a0);
    if (e != RENET_OK) return e;
    e = set_lds(Rest, STEP_LDS, a1);
    if (e != RENET_OK) return e;
    int maxL = 0;
    for (int k = 0; k < n; ++k) maxL = ly.L[ly.lay_of[k]] > maxL ? ly.L[ly.lay_of[k]] : maxL;
    for (int s = 0; s < maxL; ++s) {
        Pack ps;
        int maxbs = 0;
        for (int i = 0; i < MAXP; ++i) {
            const int k = i < n ? i : 0;
            const int lay = ly.lay_of[k];
            ps.p[i] = base.p[k];                                        // (its per-step fields are zero: no rows)
            ps.p[i].Aout = stt[k].A[s & 1];
            ps.p[i].Ain = stt[k].A[(s + 1) & 1];
            const int bs = (i < n && s < ly.L[lay]) ? fill(ps.p[i], ly.so[lay], ly.L[lay], s) : 0;
            maxbs = bs > maxbs ? bs : maxbs;
        }
        if (maxbs == 0) continue;
        const dim3 grid((maxbs + SR - 1) / SR, (NUB + SW - 1) / SW, n);
        if (s == 0) RENET_LAUNCH(First, grid, dim3(SNT), STEP_LDS, st, ps);
        else RENET_LAUNCH(Rest, grid, dim3(SNT), STEP_LDS, st, ps);
        RENET_LAUNCH_CHECK();
    }
    return RENET_OK;
}

}  // namespace

int renet_gru_steps_fwd(int H, int n, const void* probs, const void* layouts, const void* states, int Bmax,
                        hipStream_t st) {
    const FwdProbsB& pr = as<FwdProbsB>(probs);
    const Layouts& ly = as<Layouts>(layouts);
    const StepState* stt = &as<StepState>(states);
    const size_t kp = kp_of(H);
    StepsF base;
    for (int i = 0; i < n; ++i) {
        const FwdProbB& p = pr.p[i];                                    // (Ain / Aout, p0 / bs: per step)
        base.p[i] = {p.Gi, p.Wp, p.bhh, p.h_last, p.saved, nullptr, nullptr, 0, 0, stt[i].plane_stride};
        // h0 = 0 (also the rows of the empty histories past B); k padding of the A planes = 0
        hipError_t he = hipMemsetAsync(p.h_last, 0, (size_t)ly.rows[ly.lay_of[i]] * H * sizeof(float), st);
        if (he != hipSuccess) return (int)he;
        if (kp > (size_t)H) {
            he = hipMemset2DAsync(stt[i].A[0] + H, kp * sizeof(__bf16), 0, (kp - H) * sizeof(__bf16),
                                  (size_t)2 * 3 * rows_pad_of(Bmax), st);
            if (he != hipSuccess) return (int)he;
        }
    }
    return with_h(H, [&](auto h) {
        constexpr int HH = decltype(h)::value;
        return run_steps<gru_step_fwd_kernel<HH, false>, gru_step_fwd_kernel<HH, true>, Cfg<HH>::NUB>(
            n, ly, base, stt, st, [](StepF& P, const StepOff& so, int, int j) {
                P.p0 = so.off[j];
                P.bs = so.off[j + 1] - so.off[j];
                return P.bs;
            });
    });
}

int renet_gru_steps_bwd(int H, int n, const void* probs, const void* layouts, const void* states, const int* B_of,
                        int Bmax, hipStream_t st) {
    const BwdProbsB& pr = as<BwdProbsB>(probs);
    const Layouts& ly = as<Layouts>(layouts);
    const StepState* stt = &as<StepState>(states);
    const size_t kp = kp_of(3 * H);
    StepsB base;
    for (int i = 0; i < n; ++i) {
        const BwdProbB& p = pr.p[i];                                    // (Ain / Aout, bs_cur, p0_prev / bs_prev: per step)
        base.p[i] = {p.saved, p.WTp, stt[i].dh, p.dGi, p.dGh, nullptr, nullptr, 0, 0, 0, stt[i].plane_stride};
        if (B_of[i] > 0) {
            hipError_t he = hipMemcpyAsync(stt[i].dh, p.dh_last, (size_t)B_of[i] * H * sizeof(float),
                                           hipMemcpyDeviceToDevice, st);
            if (he != hipSuccess) return (int)he;
            if (kp > (size_t)3 * H) {
                he = hipMemset2DAsync(stt[i].A[0] + 3 * H, kp * sizeof(__bf16), 0, (kp - 3 * H) * sizeof(__bf16),
                                      (size_t)2 * 3 * rows_pad_of(Bmax), st);
                if (he != hipSuccess) return (int)he;
            }
        }
    }
    return with_h(H, [&](auto h) {
        constexpr int HH = decltype(h)::value;
        return run_steps<gru_step_bwd_kernel<HH, false>, gru_step_bwd_kernel<HH, true>, Cfg<HH>::NUB>(
            n, ly, base, stt, st, [](StepB& P, const StepOff& so, int L, int s) {
                const int jp = L - 1 - s;
                P.p0_prev = so.off[jp];
                P.bs_prev = so.off[jp + 1] - so.off[jp];
                if (s > 0) P.bs_cur = so.off[jp + 2] - so.off[jp + 1];
                return P.bs_prev;
            });
    });
}
