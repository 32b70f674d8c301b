// The exact-fp32 GRU recurrences (RENET_GEMM=f32, or a model's gemm_mode 'f32'): the persistent kernels described at the
// head of gru.hip on the f32-input MFMA (v_mfma_f32_16x16x4_f32), W_hh streamed as float4 B-fragments.
#include "gru_common.h"

namespace {

// ---- forward --------------------------------------------------------------------------------
template <int H>
__global__ __launch_bounds__(NT) void gru_fwd_kernel(FwdProbs ps, Layouts ly) {
    const int lay = ly.lay_of[blockIdx.y];
    const StepOff& so = ly.so[lay];
    const int L = ly.L[lay], out_rows = ly.rows[lay];
    if ((int)blockIdx.x * MT >= out_rows) return;
    using C = Cfg<H>;
    const float* __restrict__ Gi = ps.p[blockIdx.y].Gi;
    const float* __restrict__ Whh = ps.p[blockIdx.y].Whh;
    const float* __restrict__ bhh = ps.p[blockIdx.y].bhh;
    float* __restrict__ h_last = ps.p[blockIdx.y].h_last;
    float* __restrict__ saved = ps.p[blockIdx.y].saved;
    __shared__ __attribute__((aligned(16))) float Hs[MT * C::LDH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.x * MT;
    const int B = so.off[1] - so.off[0];
    for (int t = tid; t < MT * C::LDH; t += NT) Hs[t] = 0.f;          // h0 = 0 (and zero k-padding)
    __syncthreads();

    const int jj = lane & 15;          // B column / C column: hidden unit within the block
    const int kq = lane >> 4;          // k quad within a 16-k group; C rows 4*kq .. 4*kq+3
    const int ai = lane & 15;          // A row: sequence within the tile

    for (int j = 0; j < L; ++j) {
        const int p0 = so.off[j];
        const int bs = so.off[j + 1] - p0;
        if (i0 >= bs) break;                                            // whole tile finished (sorted batch)
        f32x4 hnew[(C::NUB + NW - 1) / NW];
#pragma unroll
        for (int q = 0; q < (C::NUB + NW - 1) / NW; ++q) {
            const int ub = wave + NW * q;
            if (ub < C::NUB) {
                const int u = ub * 16 + jj;                             // this lane's hidden unit
                const bool uok = u < H;
                f32x4 ar = {0.f, 0.f, 0.f, 0.f}, az = ar, an = ar;
                const float* wr = Whh + (size_t)(uok ? u : 0) * H;
                const float* wz = wr + (size_t)H * H;
                const float* wn = wz + (size_t)H * H;
#pragma unroll 4
                for (int kg = 0; kg < C::KG; ++kg) {
                    const int k = kg * 16 + 4 * kq;
                    const float4 a = *reinterpret_cast<const float4*>(&Hs[ai * C::LDH + k]);
                    float4 br = make_float4(0.f, 0.f, 0.f, 0.f), bz = br, bn = br;
                    if (uok && k < H) {
                        br = *reinterpret_cast<const float4*>(wr + k);
                        bz = *reinterpret_cast<const float4*>(wz + k);
                        bn = *reinterpret_cast<const float4*>(wn + k);
                    }
                    ar = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, br.x, ar, 0, 0, 0);
                    az = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, bz.x, az, 0, 0, 0);
                    an = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, bn.x, an, 0, 0, 0);
                    ar = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, br.y, ar, 0, 0, 0);
                    az = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, bz.y, az, 0, 0, 0);
                    an = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, bn.y, an, 0, 0, 0);
                    ar = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, br.z, ar, 0, 0, 0);
                    az = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, bz.z, az, 0, 0, 0);
                    an = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, bn.z, an, 0, 0, 0);
                    ar = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, br.w, ar, 0, 0, 0);
                    az = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, bz.w, az, 0, 0, 0);
                    an = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, bn.w, an, 0, 0, 0);
                }
                // C layout: column = lane & 15 (unit u), row = 4 * (lane >> 4) + reg (sequence)
                const float b_r = uok ? bhh[u] : 0.f, b_z = uok ? bhh[H + u] : 0.f, b_n = uok ? bhh[2 * H + u] : 0.f;
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int i = 4 * kq + reg;
                    const float hp = Hs[i * C::LDH + (uok ? u : 0)];
                    float hv = hp;
                    if (uok && i0 + i < bs) {
                        const size_t p = (size_t)(p0 + i0 + i);
                        const float* gi = Gi + p * C::K3;
                        const float hn = an[reg] + b_n;
                        const float r = sigmoidf_(gi[u] + ar[reg] + b_r);
                        const float z = sigmoidf_(gi[H + u] + az[reg] + b_z);
                        const float n = tanhf(gi[2 * H + u] + r * hn);
                        hv = (1.f - z) * n + z * hp;
                        float* sv = saved + p * 5 * H;
                        sv[u] = r; sv[H + u] = z; sv[2 * H + u] = n; sv[3 * H + u] = hn; sv[4 * H + u] = hp;
                    }
                    hnew[q][reg] = hv;
                }
            }
        }
        __syncthreads();                                                // every wave is done reading Hs
#pragma unroll
        for (int q = 0; q < (C::NUB + NW - 1) / NW; ++q) {
            const int ub = wave + NW * q;
            const int u = ub * 16 + jj;
            if (ub < C::NUB && u < H) {
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) Hs[(4 * kq + reg) * C::LDH + u] = hnew[q][reg];
            }
        }
        __syncthreads();
    }
    (void)B;
    for (int t = tid; t < MT * H; t += NT) {                  // rows >= B were never touched: still h0 = 0
        const int i = t / H, u = t - i * H;
        if (i0 + i < out_rows) h_last[(size_t)(i0 + i) * H + u] = Hs[i * C::LDH + u];
    }
}

// ---- backward (BPTT): dh lives in LDS; per step the gate gradients are formed element-wise, written out
// as dGi / dGh rows (the caller turns them into dW_ih, dW_hh, dX with large GEMMs) and dGh is kept in
// LDS as the A operand of   dh_prev = dh * z + dGh W_hh   (K = 3H, B fragments from W_hh^T [H, 3H]).
template <int H>
__global__ __launch_bounds__(NT) void gru_bwd_kernel(BwdProbs ps, Layouts ly) {
    const int lay = ly.lay_of[blockIdx.y];
    const StepOff& so = ly.so[lay];
    const int L = ly.L[lay];
    if ((int)blockIdx.x * MT >= ly.rows[lay]) return;
    using C = Cfg<H>;
    const float* __restrict__ dh_last = ps.p[blockIdx.y].dh_last;
    const float* __restrict__ WhhT = ps.p[blockIdx.y].WhhT;          // [H, 3H]
    const float* __restrict__ saved = ps.p[blockIdx.y].saved;
    float* __restrict__ dGi = ps.p[blockIdx.y].dGi;
    float* __restrict__ dGh = ps.p[blockIdx.y].dGh;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* dHs = smem;                         // [MT][LDH]
    float* Gs = smem + MT * C::LDH;            // [MT][LDG]  dGh tile (k-padded with zeros)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.x * MT;
    const int B = so.off[1] - so.off[0];
    for (int t = tid; t < MT * C::LDH; t += NT) {
        const int i = t / C::LDH, u = t - i * C::LDH;
        dHs[t] = (u < H && i0 + i < B) ? dh_last[(size_t)(i0 + i) * H + u] : 0.f;
    }
    for (int t = tid; t < MT * C::LDG; t += NT) Gs[t] = 0.f;
    __syncthreads();
    const int jj = lane & 15, kq = lane >> 4, ai = lane & 15;

    for (int j = L - 1; j >= 0; --j) {
        const int p0 = so.off[j];
        const int bs = so.off[j + 1] - p0;
        if (i0 >= bs) continue;                                         // tile not alive yet at this step
        // phase 1: gate gradients of the live rows
        for (int t = tid; t < MT * H; t += NT) {
            const int i = t / H, u = t - i * H;
            float gr = 0.f, gz = 0.f, gn = 0.f;
            if (i0 + i < bs) {
                const size_t p = (size_t)(p0 + i0 + i);
                const float* sv = saved + p * 5 * H;
                const float r = sv[u], z = sv[H + u], n = sv[2 * H + u], hn = sv[3 * H + u], hp = sv[4 * H + u];
                const float g = dHs[i * C::LDH + u];
                const float dan = g * (1.f - z) * (1.f - n * n);
                const float daz = g * (hp - n) * z * (1.f - z);
                const float dar = dan * hn * r * (1.f - r);
                float* gi = dGi + p * C::K3;
                float* gh = dGh + p * C::K3;
                gi[u] = dar; gi[H + u] = daz; gi[2 * H + u] = dan;
                gr = dar; gz = daz; gn = dan * r;
                gh[u] = gr; gh[H + u] = gz; gh[2 * H + u] = gn;
                dHs[i * C::LDH + u] = g * z;                            // direct path h_prev -> h
            }
            Gs[i * C::LDG + u] = gr; Gs[i * C::LDG + H + u] = gz; Gs[i * C::LDG + 2 * H + u] = gn;
        }
        __syncthreads();
        if (j > 0) {
            // phase 2: dh_prev += dGh W_hh  (rows of dead sequences have dGh = 0 and keep their dh)
#pragma unroll
            for (int q = 0; q < (C::NUB + NW - 1) / NW; ++q) {
                const int ub = wave + NW * q;
                if (ub < C::NUB) {
                    const int u = ub * 16 + jj;
                    const bool uok = u < H;
                    f32x4 acc;
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) acc[reg] = dHs[(4 * kq + reg) * C::LDH + (uok ? u : 0)];
                    const float* wt = WhhT + (size_t)(uok ? u : 0) * C::K3;
#pragma unroll 4
                    for (int kg = 0; kg < C::KG3; ++kg) {
                        const int k = kg * 16 + 4 * kq;
                        const float4 a = *reinterpret_cast<const float4*>(&Gs[ai * C::LDG + k]);
                        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (uok && k < C::K3) b = *reinterpret_cast<const float4*>(wt + k);
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
                    }
                    if (uok) {
#pragma unroll
                        for (int reg = 0; reg < 4; ++reg) dHs[(4 * kq + reg) * C::LDH + u] = acc[reg];
                    }
                }
            }
            __syncthreads();
        }
    }
}

// W_hh [3H, H] -> W_hh^T [H, 3H]  (tiny; once per backward call)
__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ in, int rows, int cols,
                                                        float* __restrict__ out) {
    __shared__ float tile[32][33];
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;       // 32 x 8
    for (int r = ty; r < 32; r += 8)
        if (by + r < rows && bx + tx < cols) tile[r][tx] = in[(size_t)(by + r) * cols + bx + tx];
    __syncthreads();
    for (int r = ty; r < 32; r += 8)
        if (bx + r < cols && by + tx < rows) out[(size_t)(bx + r) * rows + by + tx] = tile[tx][r];
}

}  // namespace

int renet_gru_f32_fwd(int H, const void* probs, int np, const void* layouts, hipStream_t st) {
    const Layouts& ly = as<Layouts>(layouts);
    return with_h(H, [&](auto h) -> int {
        RENET_LAUNCH((gru_fwd_kernel<decltype(h)::value>), dim3((max_rows(ly) + MT - 1) / MT, np), dim3(NT), 0, st,
                     as<FwdProbs>(probs), ly);
        RENET_LAUNCH_CHECK();
        return RENET_OK;
    });
}

int renet_gru_f32_bwd(int H, const void* probs, int np, const void* layouts, hipStream_t st) {
    const Layouts& ly = as<Layouts>(layouts);
    return with_h(H, [&](auto h) -> int {
        using C = Cfg<decltype(h)::value>;
        const size_t lds = (size_t)MT * (C::LDH + C::LDG) * sizeof(float);
        static bool attr_set = false;
        const int e = set_lds(gru_bwd_kernel<decltype(h)::value>, lds, attr_set);
        if (e != RENET_OK) return e;
        RENET_LAUNCH((gru_bwd_kernel<decltype(h)::value>), dim3((max_rows(ly) + MT - 1) / MT, np), dim3(NT), lds, st,
                     as<BwdProbs>(probs), ly);
        RENET_LAUNCH_CHECK();
        return RENET_OK;
    });
}

int renet_gru_transpose(const float* in, int rows, int cols, float* out, hipStream_t st) {
    RENET_LAUNCH(transpose_kernel, dim3((cols + 31) / 32, (rows + 31) / 32), dim3(256), 0, st, in, rows, cols, out);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}
