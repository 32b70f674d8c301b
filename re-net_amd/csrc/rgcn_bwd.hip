// RGCN backward: the prologue (ReLU mask, norm, self-loop dropout of the incoming gradient) and the weight gradient
// (per-chunk partial outer products, then a per-type reduce).  The gradient wrt h is a transposed gather (rgcn_items.hip).
#include "rgcn_common.h"

namespace {

// ---- backward prologue ----------------------------------------------------------------------
typedef float nt_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 nt_load4(const float4* p) {
    const nt_f4 v = __builtin_nontemporal_load(reinterpret_cast<const nt_f4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void nt_store4(float4* p, float4 v) {
    nt_f4 t = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(t, reinterpret_cast<nt_f4*>(p));
}

__global__ __launch_bounds__(256) void rgcn_bwd_prep_kernel(const float4* __restrict__ g_out,
                                                            const float4* __restrict__ out,
                                                            const float* __restrict__ norm, int relu,
                                                            DropCfg drop, int N, int CH,
                                                            float4* __restrict__ gn,
                                                            float4* __restrict__ g_loop,
                                                            float* __restrict__ bound_part) {
    // bound_part (optional): per-workgroup maxima of |g_loop|, the operand bound of the f16x3 GEMM that consumes it
    __shared__ float red[4];
    float mx = 0.f;
    const size_t total = (size_t)N * CH;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (size_t)gridDim.x * blockDim.x) {
        const int v = (int)(i / CH);
        // streaming operands (read once / consumed by matrix-bound GEMMs) bypass the caches: what should still be
        // cache resident when this kernel ends is gn, which the bandwidth-bound gather reads next
        float4 g = nt_load4(g_out + i);
        if (relu) {
            const float4 o = nt_load4(out + i);
            g.x = o.x > 0.f ? g.x : 0.f; g.y = o.y > 0.f ? g.y : 0.f;
            g.z = o.z > 0.f ? g.z : 0.f; g.w = o.w > 0.f ? g.w : 0.f;
        }
        gn[i] = f4_scale(g, norm[v]);
        const float4 gl = f4_mul(g, renet_drop4(drop, i));
        nt_store4(g_loop + i, gl);
        mx = fmaxf(fmaxf(mx, fmaxf(fabsf(gl.x), fabsf(gl.y))), fmaxf(fabsf(gl.z), fabsf(gl.w)));
    }
    if (bound_part) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
        __syncthreads();
        if (threadIdx.x == 0) bound_part[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    }
}

// ---- dW: per-chunk partial outer products -----------------------------------------------------
// one wave per chunk (all edges of the chunk have the same relation type); lane = float4 chunk of
// the feature row; SI*4 accumulators per lane-chunk (the si x so block entries).  Row loads are unconditional
// buffer loads (see the item-stream gather): an edge slot past the chunk's end reads nothing and multiplies zeros.
// A workgroup takes kBwdWGroup CONSECUTIVE chunks (chunks are sorted by type) and adds up, through LDS and in chunk
// order, the chunks of one type before anything is written: the partial of a run lands in the slot of the run's first
// chunk -- the group's first chunk or the first chunk of a type -- and the reduce kernel below reads only those slots
// (the hottest relation of a Zipf batch owns > 1000 chunks: 8x fewer dependent rounds on its critical path).
// BIG: x / gmat of 2 GiB and more (renet_rgcn_bwd_w64) -- 64-bit global addressing instead of the 32-bit buffer offsets.
// SI = 3: lane = one 3x3 block (3-float chunks of x and gmat, see vw_of): 9 products per edge, kept as three xyz rows;
// the block's 9 entries are consecutive floats of the relation row, which is 225 float4 -- LDS and the partial rows are
// written per float; the 64 lanes of a run's first wave then add the run's rows and store them, one float4 each.
constexpr int kBwdWGroup = 8;
template <int SI, int NCH, bool BIG = false>
__global__ __launch_bounds__(kBwdWGroup * 64) void rgcn_bwd_w_partial_kernel(
    const float* __restrict__ x, const float* __restrict__ gmat, const int32_t* __restrict__ e_src,
    const int32_t* __restrict__ e_dst, const int32_t* __restrict__ chunk_ptr, const int32_t* __restrict__ chunk_type,
    int n_chunks, float4* __restrict__ partial) {
    constexpr int D = 100 * SI;
    constexpr int VW = vw_of<SI>();
    constexpr int CH = D / VW;
    constexpr int WROW4 = D * SI / 4;
    constexpr uint32_t ROWB = D * 4;
    constexpr int UNR = (SI == 4) ? 2 : (SI == 3) ? 4 : 8;   // edges with both row loads in flight together
    __shared__ float4 red[kBwdWGroup][WROW4];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = blockIdx.x * kBwdWGroup + wave;
    const bool live = c < n_chunks;
    const int e0 = live ? chunk_ptr[c] : 0, e1 = live ? chunk_ptr[c + 1] : 0;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(x, kBufSpan);
    const __amdgpu_buffer_rsrc_t rg = make_rsrc(gmat, kBufSpan);
    uint32_t off[NCH];
#pragma unroll
    for (int q = 0; q < NCH; ++q) off[q] = (uint32_t)(lane + 64 * q) < (uint32_t)CH ? (uint32_t)(lane + 64 * q) * (4u * VW) : kOob;
    float4 acc[NCH][SI];
#pragma unroll
    for (int q = 0; q < NCH; ++q)
#pragma unroll
        for (int i = 0; i < SI; ++i) acc[q][i] = make_float4(0.f, 0.f, 0.f, 0.f);

    for (int eb = e0; eb < e1; eb += 64) {
        const int my_e = eb + lane;
        int my_s = 0, my_d = 0;
        if (my_e < e1) { my_s = e_src[my_e]; my_d = e_dst[my_e]; }
        asm volatile("" : "+v"(my_s), "+v"(my_d));          // wait for the indices here, not inside the loop
        const int cnt = min(64, e1 - eb);
        for (int k0 = 0; k0 < cnt; k0 += UNR) {
            float4 xv[UNR][NCH], gv[UNR][NCH];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int kk = min(k0 + u, 63);
                const bool ok = (k0 + u) < cnt;
                const uint32_t so = ok ? (uint32_t)__builtin_amdgcn_readlane(my_s, kk) * ROWB : 0u;
                const uint32_t dof = ok ? (uint32_t)__builtin_amdgcn_readlane(my_d, kk) * ROWB : 0u;
#pragma unroll
                for (int q = 0; q < NCH; ++q) {
                    if constexpr (BIG) {
                        const int ch = lane + 64 * q;
                        const bool on = ok && ch < CH;
                        const size_t sr = (size_t)__builtin_amdgcn_readlane(my_s, kk) * CH + ch;
                        const size_t dr = (size_t)__builtin_amdgcn_readlane(my_d, kk) * CH + ch;
                        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
                        if constexpr (VW == 4) {
                            xv[u][q] = on ? reinterpret_cast<const float4*>(x)[sr] : z;
                            gv[u][q] = on ? reinterpret_cast<const float4*>(gmat)[dr] : z;
                        } else {
                            xv[u][q] = on ? ld_chunk<VW>(x, sr) : z;
                            gv[u][q] = on ? ld_chunk<VW>(gmat, dr) : z;
                        }
                    } else {
                        xv[u][q] = buf_loadvs<VW>(rx, ok ? off[q] : kOob, so);
                        gv[u][q] = buf_loadvs<VW>(rg, ok ? off[q] : kOob, dof);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
#pragma unroll
                for (int q = 0; q < NCH; ++q) {
                    if constexpr (SI == 1) {
                        acc[q][0].x = fmaf(xv[u][q].x, gv[u][q].x, acc[q][0].x);
                        acc[q][0].y = fmaf(xv[u][q].y, gv[u][q].y, acc[q][0].y);
                        acc[q][0].z = fmaf(xv[u][q].z, gv[u][q].z, acc[q][0].z);
                        acc[q][0].w = fmaf(xv[u][q].w, gv[u][q].w, acc[q][0].w);
                    } else if constexpr (SI == 2) {
                        // block0: dW[i][j] = x_i g_j (i,j in {0,1}); block1 with elements 2,3
                        acc[q][0].x = fmaf(xv[u][q].x, gv[u][q].x, acc[q][0].x);
                        acc[q][0].y = fmaf(xv[u][q].x, gv[u][q].y, acc[q][0].y);
                        acc[q][0].z = fmaf(xv[u][q].y, gv[u][q].x, acc[q][0].z);
                        acc[q][0].w = fmaf(xv[u][q].y, gv[u][q].y, acc[q][0].w);
                        acc[q][1].x = fmaf(xv[u][q].z, gv[u][q].z, acc[q][1].x);
                        acc[q][1].y = fmaf(xv[u][q].z, gv[u][q].w, acc[q][1].y);
                        acc[q][1].z = fmaf(xv[u][q].w, gv[u][q].z, acc[q][1].z);
                        acc[q][1].w = fmaf(xv[u][q].w, gv[u][q].w, acc[q][1].w);
                    } else if constexpr (SI == 3) {
                        // dW[i][j] = x_i g_j of this lane's block: acc[q][i] = row i (xyz)
                        const float xs[3] = {xv[u][q].x, xv[u][q].y, xv[u][q].z};
#pragma unroll
                        for (int i = 0; i < 3; ++i) {
                            acc[q][i].x = fmaf(xs[i], gv[u][q].x, acc[q][i].x);
                            acc[q][i].y = fmaf(xs[i], gv[u][q].y, acc[q][i].y);
                            acc[q][i].z = fmaf(xs[i], gv[u][q].z, acc[q][i].z);
                        }
                    } else {
                        const float xs[4] = {xv[u][q].x, xv[u][q].y, xv[u][q].z, xv[u][q].w};
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            acc[q][i].x = fmaf(xs[i], gv[u][q].x, acc[q][i].x);
                            acc[q][i].y = fmaf(xs[i], gv[u][q].y, acc[q][i].y);
                            acc[q][i].z = fmaf(xs[i], gv[u][q].z, acc[q][i].z);
                            acc[q][i].w = fmaf(xs[i], gv[u][q].w, acc[q][i].w);
                        }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NCH; ++q) {
        const int ch = lane + 64 * q;
        if (ch < CH) {
            if constexpr (SI == 3) {
                float* rf = reinterpret_cast<float*>(red[wave]) + ch * 9;    // (stride 9 floats: conflict-free)
#pragma unroll
                for (int i = 0; i < 3; ++i) { rf[3 * i] = acc[q][i].x; rf[3 * i + 1] = acc[q][i].y; rf[3 * i + 2] = acc[q][i].z; }
            } else {
#pragma unroll
                for (int i = 0; i < SI; ++i) red[wave][ch * SI + i] = acc[q][i];
            }
        }
    }
    __syncthreads();
    if (!live) return;
    const int ty = chunk_type[c];
    if (wave != 0 && chunk_type[c - 1] == ty) return;         // not the first chunk of its run
    int run = 1;                                              // chunks of this run inside the group
    while (wave + run < kBwdWGroup && c + run < n_chunks && chunk_type[c + run] == ty) ++run;
    if constexpr (SI == 3) {
        for (int k = lane; k < WROW4; k += 64) {
            float4 r = red[wave][k];
            for (int w = 1; w < run; ++w) r = f4_add(r, red[wave + w][k]);
            partial[(size_t)c * WROW4 + k] = r;
        }
        return;
    }
#pragma unroll
    for (int q = 0; q < NCH; ++q) {
        const int ch = lane + 64 * q;
        if (ch < CH) {
#pragma unroll
            for (int i = 0; i < SI; ++i) {
                float4 r = red[wave][ch * SI + i];
                for (int w = 1; w < run; ++w) r = f4_add(r, red[wave + w][ch * SI + i]);
                partial[(size_t)c * WROW4 + ch * SI + i] = r;
            }
        }
    }
}

// dW[t, :] = sum over the chunks of type t (fixed order => deterministic); grid = (T, ceil(WROW4/64)).
// Relation frequencies are Zipf-like: on the ICEWS18-shaped merged batch the hottest type owns > 1000 of the ~4500
// chunks, and its workgroup is the kernel's critical path (40 us with 4 waves x 4 loads in flight: 80 dependent
// rounds).  16 waves x 4 independent partial-sum loads each walk the chunk range 64 chunks per round; fixed
// association order (per wave, then an LDS tree over the waves) => still deterministic.
constexpr int kRedWaves = 16;
__global__ __launch_bounds__(kRedWaves * 64) void rgcn_bwd_w_reduce_kernel(
    const float4* __restrict__ partial, const int32_t* __restrict__ type_chunk_ptr, int WROW4,
    int T, int shift, float beta, float4* __restrict__ dW) {
    __shared__ float4 red[kRedWaves][64];
    const int t = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int colq = blockIdx.y * 64 + lane;
    const int c0 = type_chunk_ptr[t], c1 = type_chunk_ptr[t + 1];
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (colq < WROW4 && c1 > c0) {
        // the slots that hold a run's sum (rgcn_bwd_w_partial_kernel): c0 itself, then every group start inside the type
        if (wave == 0) s = partial[(size_t)c0 * WROW4 + colq];
        const int g0 = c0 / kBwdWGroup + 1;                                   // first group that starts behind c0
        const int g1 = (c1 + kBwdWGroup - 1) / kBwdWGroup;                   // groups starting before c1
        float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1, s3 = s1;
        int gq = g0 + wave;
        for (; gq + 3 * kRedWaves < g1; gq += 4 * kRedWaves) {
            const float4 v0 = partial[(size_t)gq * kBwdWGroup * WROW4 + colq];
            const float4 v1 = partial[(size_t)(gq + kRedWaves) * kBwdWGroup * WROW4 + colq];
            const float4 v2 = partial[(size_t)(gq + 2 * kRedWaves) * kBwdWGroup * WROW4 + colq];
            const float4 v3 = partial[(size_t)(gq + 3 * kRedWaves) * kBwdWGroup * WROW4 + colq];
            s = f4_add(s, v0); s1 = f4_add(s1, v1); s2 = f4_add(s2, v2); s3 = f4_add(s3, v3);
        }
        for (; gq < g1; gq += kRedWaves) s = f4_add(s, partial[(size_t)gq * kBwdWGroup * WROW4 + colq]);
        s = f4_add(f4_add(s, s1), f4_add(s2, s3));
    }
    red[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && colq < WROW4) {
        float4 r = red[0][lane];
#pragma unroll
        for (int w = 1; w < kRedWaves; ++w) r = f4_add(r, red[w][lane]);
        int to = t + shift;
        if (to >= T) to -= T;
        float4* o = dW + (size_t)to * WROW4 + colq;
        if (beta != 0.f) {
            const float4 p = *o;
            r = make_float4(r.x + beta * p.x, r.y + beta * p.y, r.z + beta * p.z, r.w + beta * p.w);
        }
        *o = r;
    }
}

template <int SI, class... Args>                            // args: the kernel's, after the launch configuration
int launch_bwd_w_partial(bool big, int n_chunks, hipStream_t st, Args... args) {
    const dim3 grid((n_chunks + kBwdWGroup - 1) / kBwdWGroup), blk(kBwdWGroup * 64);
    if (big) RENET_LAUNCH((rgcn_bwd_w_partial_kernel<SI, nch_of<SI>(), true>), grid, blk, 0, st, args...);
    else RENET_LAUNCH((rgcn_bwd_w_partial_kernel<SI, nch_of<SI>()>), grid, blk, 0, st, args...);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}

}  // namespace

extern "C" {

static int bwd_prep_impl(const float* g_out, const float* out, const float* norm, int relu, float drop_p,
                         uint64_t seed, int N, int D, float* gn, float* g_loop, float* bound_part, void* stream) {
    if (N < 0 || D <= 0 || (D & 3) || drop_p < 0.f || drop_p >= 1.f) return RENET_ERR_BADARG;
    if (N == 0) return bound_part ? RENET_ERR_BADARG : RENET_OK;
    const size_t total = (size_t)N * (D / 4);
    int blocks = (int)min((size_t)(bound_part ? 1024 : 2048), (total + 255) / 256);     // = renet_bound_parts(total)
    RENET_LAUNCH(rgcn_bwd_prep_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)g_out, (const float4*)out, norm, relu, make_drop(drop_p, seed), N,
                       D / 4, (float4*)gn, (float4*)g_loop, bound_part);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}

int renet_rgcn_bwd_prep(const float* g_out, const float* out, const float* norm, int relu,
                        float drop_p, uint64_t seed, int N, int D, float* gn, float* g_loop,
                        void* stream) {
    return bwd_prep_impl(g_out, out, norm, relu, drop_p, seed, N, D, gn, g_loop, nullptr, stream);
}

int renet_rgcn_bwd_prep_bounds(const float* g_out, const float* out, const float* norm, int relu,
                               float drop_p, uint64_t seed, int N, int D, float* gn, float* g_loop,
                               float* bound_part, void* stream) {
    if (!bound_part) return RENET_ERR_BADARG;
    return bwd_prep_impl(g_out, out, norm, relu, drop_p, seed, N, D, gn, g_loop, bound_part, stream);
}

size_t renet_rgcn_bwd_w_workspace(int n_chunks, int D) {
    return (size_t)max(n_chunks, 0) * (size_t)(D * (D / 100)) * sizeof(float);
}

static int bwd_w_impl(bool big, const float* x, const float* gn, const int32_t* e_src, const int32_t* e_dst,
                      const int32_t* chunk_ptr, const int32_t* chunk_type, int n_chunks,
                      const int32_t* type_chunk_ptr, int T, int type_shift, int D, float* dW, float beta,
                      float* workspace, size_t workspace_bytes, void* stream) {
    if (!renet_dim_ok(D)) return RENET_ERR_UNSUPPORTED;
    if (n_chunks > 0 && !chunk_type) return RENET_ERR_BADARG;
    if (n_chunks < 0 || T <= 0 || type_shift < 0 || type_shift >= T) return RENET_ERR_BADARG;
    if (workspace_bytes < renet_rgcn_bwd_w_workspace(n_chunks, D)) return RENET_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int WROW4 = D * (D / 100) / 4;
    if (n_chunks > 0) {
        const int rc = with_si(D, [&](auto si) {
            return launch_bwd_w_partial<decltype(si)::value>(big, n_chunks, st, x, gn, e_src, e_dst, chunk_ptr, chunk_type,
                                                             n_chunks, (float4*)workspace);
        });
        if (rc != RENET_OK) return rc;
    }
    RENET_LAUNCH(rgcn_bwd_w_reduce_kernel, dim3(T, (WROW4 + 63) / 64), dim3(kRedWaves * 64), 0, st,
                       (const float4*)workspace, type_chunk_ptr, WROW4, T, type_shift, beta, (float4*)dW);
    RENET_LAUNCH_CHECK();
    return RENET_OK;
}

int renet_rgcn_bwd_w(const float* x, const float* gn, const int32_t* e_src, const int32_t* e_dst,
                     const int32_t* chunk_ptr, const int32_t* chunk_type, int n_chunks,
                     const int32_t* type_chunk_ptr, int T, int type_shift, int D, float* dW, float beta,
                     float* workspace, size_t workspace_bytes, void* stream) {
    return bwd_w_impl(false, x, gn, e_src, e_dst, chunk_ptr, chunk_type, n_chunks, type_chunk_ptr, T, type_shift, D, dW,
                      beta, workspace, workspace_bytes, stream);
}

int renet_rgcn_bwd_w64(const float* x, const float* gn, const int32_t* e_src, const int32_t* e_dst,
                       const int32_t* chunk_ptr, const int32_t* chunk_type, int n_chunks,
                       const int32_t* type_chunk_ptr, int T, int type_shift, int D, float* dW, float beta,
                       float* workspace, size_t workspace_bytes, void* stream) {
    return bwd_w_impl(true, x, gn, e_src, e_dst, chunk_ptr, chunk_type, n_chunks, type_chunk_ptr, T, type_shift, D, dW,
                      beta, workspace, workspace_bytes, stream);
}

}  // extern "C"
